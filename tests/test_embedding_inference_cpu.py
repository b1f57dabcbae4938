"""Host logic of Inference on chunk-resolution (embedding) models -- window="sliding" / "whole", crop with one segment
or a list -- against the reference's own Inference (core/inference.py:182-496, run through tests/refharness.py), both
driving the same torch-CPU oracle network; the SpeakerEmbedding voice-activity weights against the reference formula
(pipelines/speaker_verification.py:838-856); the length bucketing of EmbeddingEngine.forward_ragged.  The device
kernels under them are covered on the GPU (tests/test_embedding_inference_gpu.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import refharness
from pyannote_audio_amd.core import Segment
from pyannote_audio_amd.inference import Inference

SR = 16000


@pytest.fixture(scope="module")
def net():
    from oracle.models import WeSpeakerResNet34
    torch.manual_seed(5)
    return WeSpeakerResNet34(num_blocks=(1, 1, 1, 1)).eval()


class _OracleEngine:
    """EmbeddingEngine stand-in: strided chunks of a flat waveform (zeros past its end, as k_fbank reads them)
    through the oracle network"""
    READS_PAST_END_AS_ZERO = True

    def __init__(self, net):
        self.net, self.calls = net, []

    def forward_strided(self, wav, stride, count, window, masks=None):
        self.calls.append((wav.numel(), stride, count, window))
        chunks = [F.pad(wav[c * stride:c * stride + window], (0, max(0, c * stride + window - wav.numel())))
                  for c in range(count)]
        with torch.inference_mode():
            return self.net(torch.stack(chunks)[:, None])[:, None]


class _PaddingEngine(_OracleEngine):
    READS_PAST_END_AS_ZERO = False     # (the x-vector front end: the orphan chunk is padded by Inference)


class _Audio:
    sample_rate = 16000

    def get_num_samples(self, duration, sample_rate=None):
        return round(duration * (sample_rate or 16000))


class _Model:
    def __init__(self, engine):
        from pyannote_audio_amd.model import embedding_specifications
        self.engine, self.specifications, self.audio = engine, embedding_specifications(), _Audio()
        self.device = torch.device("cpu")

    def eval(self):
        return self

    def to(self, device):
        return self

    def __call__(self, waveforms, weights=None):
        with torch.inference_mode():
            return self.engine.net(waveforms)


@pytest.fixture(scope="module")
def reference(net):
    if not refharness.available():
        pytest.skip("the reference sources are not on this machine")
    with refharness.reference_modules(third_party=True) as ref:
        top = ref.load_core()
        task = ref.load("pyannote.audio.core.task")

        class RefModel(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.net = net
                self.specifications = task.Specifications(problem=task.Problem.REPRESENTATION,
                                                          resolution=task.Resolution.CHUNK, duration=5.0)
                self.audio = top.Audio(sample_rate=SR, mono="downmix")
                self.receptive_field = None

            @property
            def device(self):
                return torch.device("cpu")

            def forward(self, waveforms, weights=None):
                return self.net(waveforms)

        yield top.Inference, RefModel()


def _file(seconds, seed):
    g = torch.Generator().manual_seed(seed)
    return {"waveform": (0.1 * torch.randn(1, round(seconds * SR), generator=g)).clamp(-1, 1), "sample_rate": SR,
            "uri": "f"}


def _same(got, want):
    if hasattr(want, "sliding_window"):
        a, b = got.sliding_window, want.sliding_window
        assert (a.start, a.duration, a.step) == (b.start, b.duration, b.step)
        got, want = got.data, want.data
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)


@pytest.mark.parametrize("engine_class", [_OracleEngine, _PaddingEngine])
@pytest.mark.parametrize("seconds", [20.5, 2.0, 7.0])
def test_sliding_window_matches_reference(net, reference, engine_class, seconds):
    RefInference, ref_model = reference
    file = _file(seconds, seed=int(seconds * 10))
    engine = engine_class(net)
    ours, theirs = [], []
    got = Inference(_Model(engine), duration=3.0, step=1.0, batch_size=4)(file, hook=lambda **k: ours.append(k))
    want = RefInference(ref_model, duration=3.0, step=1.0, batch_size=4)(file, hook=lambda **k: theirs.append(k))
    _same(got, want)
    assert ours == theirs
    n, last = Inference.num_chunks(file["waveform"].shape[1], 3 * SR, SR)
    assert got.data.shape[0] == n + last
    if engine_class is _OracleEngine:          # orphan chunk read past the end of the waveform, in the same call
        assert engine.calls == [(file["waveform"].shape[1], SR, n + last, 3 * SR)]


def test_whole_window_and_crop_match_reference(net, reference):
    RefInference, ref_model = reference
    file = _file(12.0, seed=1)
    whole, ref_whole = Inference(_Model(_OracleEngine(net)), window="whole"), RefInference(ref_model, window="whole")
    _same(whole(file), ref_whole(file))
    assert whole(file).shape == (256,)
    segs = [Segment(0.5, 2.5), Segment(7.0, 9.75)]
    _same(whole.crop(file, Segment(1.3, 6.1)), ref_whole.crop(file, Segment(1.3, 6.1)))
    _same(whole.crop(file, segs), ref_whole.crop(file, segs))              # the excerpts concatenated
    sliding = Inference(_Model(_OracleEngine(net)), duration=3.0, step=1.0)
    ref_sliding = RefInference(ref_model, duration=3.0, step=1.0)
    got = sliding.crop(file, segs)                                         # smallest segment holding both
    _same(got, ref_sliding.crop(file, segs))
    assert got.sliding_window.start == 0.5 and got.data.shape == (8, 256)
    _same(sliding.crop(file, Segment(2.25, 8.0)), ref_sliding.crop(file, Segment(2.25, 8.0)))


def test_vad_weights_follow_the_reference_formula():
    from pyannote_audio_amd.speaker_verification import vad_weights
    rng = np.random.default_rng(3)
    scores = rng.random((589, 1)).astype(np.float32)
    scores[rng.random(589) < 0.1] = np.nan
    # pipelines/speaker_verification.py:848-852
    weights = scores.copy()
    weights[np.isnan(weights)] = 0.0
    want = torch.from_numpy(weights ** 3)[None, :, 0]
    got = vad_weights(scores)
    assert got.shape == (589,) and np.isnan(scores).any()
    assert torch.equal(torch.from_numpy(got)[None], want)


def test_speaker_embedding_needs_a_local_model():
    from pyannote_audio_amd import SpeakerEmbedding
    from pyannote_audio_amd.pipeline import get_class_by_name
    with pytest.raises(ValueError, match="embedding"):
        SpeakerEmbedding()
    assert get_class_by_name("pyannote.audio.pipelines.SpeakerEmbedding") is SpeakerEmbedding


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_length_buckets_cover_every_utterance_in_order(seed):
    from pyannote_audio_amd.embedding import EmbeddingEngine, length_buckets
    rng = np.random.default_rng(seed)
    lengths = np.round(np.clip(np.exp(rng.normal(np.log(7.0), 0.4, 4874)), 4.0, 20.0) * SR).astype(np.int64)
    if seed == 2:
        lengths = rng.integers(400, 400000, 500)
    srt = np.sort(lengths)
    buckets = length_buckets(srt)
    assert buckets[0][0] == 0 and buckets[-1][1] == srt.size
    assert all(a[1] == b[0] and a[0] < a[1] for a, b in zip(buckets, buckets[1:]))     # contiguous, none empty
    for b0, b1 in buckets:
        assert srt[b1 - 1] <= EmbeddingEngine.RAGGED_RATIO * srt[b0]
        assert b1 == srt.size or srt[b1] > EmbeddingEngine.RAGGED_RATIO * srt[b0]       # greedy: as wide as allowed
    padded = sum(int(srt[b1 - 1]) * (b1 - b0) for b0, b1 in buckets)
    assert 1.0 - srt.sum() / padded < 1.0 - 1.0 / EmbeddingEngine.RAGGED_RATIO
