"""GPU parity of the public embedding interfaces -- Inference(window="whole" | "sliding"), Inference.crop,
SpeakerEmbedding.apply / apply_batch -- and of the ragged batch under them (EmbeddingEngine.forward_ragged,
pa_emb_forward_ragged), against the torch-CPU oracle run on each utterance alone.  Tolerance: the north_star float
contract for embeddings, |d| <= 1e-5 + 1e-4 |ref|."""
import numpy as np
import pytest
import torch

from conftest import PYANNET_HPARAMS, WESPEAKER_HPARAMS, north_star_ratio

pytestmark = pytest.mark.gpu

SR = 16000
XVECTOR_HPARAMS = {"sincnet": {"stride": 10, "sample_rate": 16000}, "dimension": 512, "sample_rate": 16000,
                   "num_channels": 1}


def _wave(num_samples, seed):
    g = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(1, num_samples, generator=g)
    x += 0.05 * torch.sin(torch.arange(num_samples) * (0.03 + 0.001 * (seed % 7)))[None] + 0.01
    return x.clamp(-1, 1)


def _file(wav):
    return {"waveform": wav, "sample_rate": SR, "uri": f"utt{wav.shape[1]}"}


@pytest.fixture(scope="module")
def models(gpu_device):
    import pyannote_audio_amd.model as pm
    from oracle import seeded_wespeaker, seeded_xvector
    wes_o, xv_o = seeded_wespeaker(seed=4321), seeded_xvector()
    wes = pm.WeSpeakerResNet34(wes_o.state_dict(), WESPEAKER_HPARAMS, pm.embedding_specifications()).to(gpu_device)
    xv = pm.XVectorSincNet(xv_o.state_dict(), XVECTOR_HPARAMS, pm.embedding_specifications()).to(gpu_device)
    return {"wespeaker": (wes_o, wes), "xvector": (xv_o, xv)}


def _oracle(model, wav, weights=None):
    with torch.inference_mode():
        return model(wav[None], weights=weights).numpy()


# ------------------------------------------------------------------------------------------------ Inference
@pytest.mark.parametrize("name,seconds", [("wespeaker", 2.5), ("wespeaker", 7.3), ("wespeaker", 61.0),
                                          ("xvector", 2.5), ("xvector", 7.3)])
def test_whole_window(models, name, seconds):
    from pyannote_audio_amd import Inference
    oracle, model = models[name]
    wav = _wave(round(seconds * SR), seed=int(seconds * 10))
    got = Inference(model, window="whole")(_file(wav))
    want = _oracle(oracle, wav)[0]
    assert got.shape == want.shape == (model.dimension,)
    assert north_star_ratio(f"{name}_whole_{seconds}s", torch.from_numpy(got), torch.from_numpy(want)) <= 1.0


@pytest.mark.parametrize("name", ["wespeaker", "xvector"])
def test_sliding_window_with_orphan_chunk(models, name):
    from pyannote_audio_amd import Inference
    oracle, model = models[name]
    wav = _wave(int(20.5 * SR), seed=3)
    calls = []
    inference = Inference(model, window="sliding", duration=3.0, step=1.0, batch_size=8)
    out = inference(_file(wav), hook=lambda **k: calls.append(k))
    window, step = 3 * SR, SR
    n = (wav.shape[1] - window) // step + 1
    chunks = [wav[:, c * step:c * step + window] for c in range(n)]
    last = torch.zeros(1, window)
    last[:, :wav.shape[1] - n * step] = wav[:, n * step:]
    with torch.inference_mode():
        want = oracle(torch.stack(chunks + [last])).numpy()
    assert out.data.shape == (n + 1, model.dimension) == (19, model.dimension)
    sw = out.sliding_window
    assert (sw.start, sw.duration, sw.step) == (0.0, 3.0, 1.0)
    assert calls == [{"completed": c, "total": 19} for c in (0, 8, 16, 24, 19)]
    assert north_star_ratio(f"{name}_sliding", torch.from_numpy(out.data), torch.from_numpy(want)) <= 1.0


@pytest.mark.parametrize("name", ["wespeaker", "xvector"])
def test_crop(models, name):
    from pyannote_audio_amd import Audio, Inference, Segment
    oracle, model = models[name]
    wav = _wave(12 * SR, seed=5)
    file = _file(wav)
    audio = Audio(SR, mono="downmix")
    whole = Inference(model, window="whole")
    seg = Segment(1.3, 6.1)
    got = whole.crop(file, seg)
    want = _oracle(oracle, audio.crop(file, seg)[0])[0]
    assert north_star_ratio(f"{name}_crop", torch.from_numpy(got), torch.from_numpy(want)) <= 1.0
    segs = [Segment(0.5, 2.5), Segment(7.0, 9.75)]
    got = whole.crop(file, segs)
    want = _oracle(oracle, torch.cat([audio.crop(file, s)[0] for s in segs], dim=1))[0]
    assert north_star_ratio(f"{name}_crop_list", torch.from_numpy(got), torch.from_numpy(want)) <= 1.0
    sliding = Inference(model, window="sliding", duration=3.0, step=1.0)
    out = sliding.crop(file, segs)                # = crop on Segment(0.5, 9.75), frames shifted to 0.5 s
    ref = sliding.crop(file, Segment(0.5, 9.75))
    assert out.sliding_window.start == 0.5 and out.data.shape == ref.data.shape == (8, model.dimension)
    crop = audio.crop(file, Segment(0.5, 9.75))[0]
    want = np.concatenate([_oracle(oracle, crop[:, c * SR:c * SR + 3 * SR]) for c in range(7)]
                          + [_oracle(oracle, torch.nn.functional.pad(crop[:, 7 * SR:], (0, 10 * SR - crop.shape[1])))])
    assert north_star_ratio(f"{name}_crop_sliding", torch.from_numpy(out.data), torch.from_numpy(want)) <= 1.0


# ------------------------------------------------------------------------------------------------ SpeakerEmbedding
@pytest.fixture(scope="module")
def segmentation(gpu_device):
    import pyannote_audio_amd.model as pm
    from oracle import seeded_pyannet
    return pm.PyanNet(seeded_pyannet().state_dict(), PYANNET_HPARAMS,
                      pm.segmentation_specifications(10.0, True)).to(gpu_device)


def test_speaker_embedding_apply(models, segmentation):
    from pyannote_audio_amd import Inference, SpeakerEmbedding
    from pyannote_audio_amd.speaker_verification import vad_weights
    from pyannote_audio_amd.voice_activity_detection import any_speaker
    oracle, model = models["wespeaker"]
    wav = _wave(int(12.4 * SR), seed=9)
    got = SpeakerEmbedding(embedding=model)(_file(wav))
    assert got.shape == (1, 256)
    assert north_star_ratio("speaker_embedding", torch.from_numpy(got), torch.from_numpy(_oracle(oracle, wav))) <= 1.0
    weights = vad_weights(Inference(segmentation, pre_aggregation_hook=any_speaker)(_file(wav)).data)
    pipeline = SpeakerEmbedding(embedding=model, segmentation=segmentation)
    got = pipeline.apply(_file(wav))
    want = _oracle(oracle, wav, torch.from_numpy(weights)[None])
    assert north_star_ratio("speaker_embedding_vad", torch.from_numpy(got), torch.from_numpy(want)) <= 1.0
    # (a seeded segmentation model hears speech everywhere) scores with silences, fractions and NaN in its place
    scores = np.random.default_rng(4).random((731, 1)).astype(np.float32)
    scores[100:300] = 0.0
    scores[500:520] = np.nan
    pipeline._segmentation = _Scores(scores)
    got = pipeline.apply(_file(wav))
    weights = vad_weights(scores)
    assert 0.0 < weights.mean() < 0.5
    want = _oracle(oracle, wav, torch.from_numpy(weights)[None])
    assert north_star_ratio("speaker_embedding_vad_scores", torch.from_numpy(got), torch.from_numpy(want)) <= 1.0
    assert north_star_ratio("speaker_embedding_vad_not_plain", torch.from_numpy(got),
                            torch.from_numpy(_oracle(oracle, wav))) > 1.0


class _Scores:
    """stands in for the segmentation Inference of SpeakerEmbedding: fixed aggregated scores"""

    def __init__(self, data):
        self.data = data

    def __call__(self, file):
        from pyannote_audio_amd.core import SlidingWindow, SlidingWindowFeature
        return SlidingWindowFeature(self.data.copy(), SlidingWindow(start=0.0, duration=0.0619375, step=0.016875))


def test_apply_batch_equals_apply(models, segmentation):
    from pyannote_audio_amd import SpeakerEmbedding
    for name in ("wespeaker", "xvector"):
        _, model = models[name]
        files = [_file(_wave(int(s * SR), seed=i)) for i, s in enumerate([4.2, 9.0, 4.0, 6.6, 4.2])]
        for tag, seg in (("plain", None), ("vad", segmentation), ("scores", "scores")):
            pipeline = SpeakerEmbedding(embedding=model, segmentation=None if seg == "scores" else seg)
            if seg == "scores":
                scores = np.random.default_rng(5).random((300, 1)).astype(np.float32)
                scores[40:90] = np.nan
                pipeline.segmentation = "stub"
                pipeline._segmentation = _Scores(scores)
            batch = pipeline.apply_batch(files)
            assert len(batch) == len(files)
            for i, f in enumerate(files):
                assert north_star_ratio(f"{name}_apply_batch_{i}_{tag}", torch.from_numpy(batch[i]),
                                        torch.from_numpy(pipeline.apply(f))) <= 1.0


# ------------------------------------------------------------------------------------------------ forward_ragged
def _ragged_lengths():
    """24+ lengths over 0.5 - 20 s: every residue of T_b mod 8, most not a multiple of 160 samples"""
    frames = np.unique(np.geomspace(48, 1998, 26).astype(int))
    lengths = []
    for i, t in enumerate(frames):
        t = t - t % 8 + i % 8
        lengths.append(400 + (t - 1) * 160 + (37 * i) % 160)
    lengths.append(8000)                                   # 0.5 s exactly
    return lengths


def _concat(lengths, seed=0):
    waves = [_wave(n, seed + i)[0] for i, n in enumerate(lengths)]
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    return waves, offsets, torch.cat(waves)


def _nan_workspace(eng, lib, lengths):
    nbytes = lib.pa_emb_ragged_workspace_bytes(eng.pack.struct, len(lengths), max(lengths))
    eng._ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=eng.pack.device)   # all-ones bytes = NaN floats


def _check_ragged(oracle, eng, lengths, tag, with_masks=True):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    dev = eng.pack.device
    assert {(1 + (n - 400) // 160) % 8 for n in lengths} == set(range(8))
    assert any(n % 160 for n in lengths) and len(lengths) >= 24
    waves, offsets, wav = _concat(lengths)
    g = torch.Generator().manual_seed(17)
    masks = [(torch.rand(eng.num_pool_frames(n) + 9, generator=g) < 0.7).float() for n in lengths]
    for use_masks in ((False, True) if with_masks else (False,)):
        wants, alones = [], []
        for i, x in enumerate(waves):
            w = masks[i][None] if use_masks else None
            wants.append(torch.from_numpy(_oracle(oracle, x[None], w)))
            alones.append(eng.forward(x.view(1, 1, -1).to(dev), w.to(dev) if w is not None else None))
        # the default buckets (<= 1.10 x), then every utterance in ONE launch group (0.5 s padded to 20 s)
        for ratio in (eng.RAGGED_RATIO, 1e9):
            eng.RAGGED_RATIO = ratio
            try:
                _nan_workspace(eng, lib, lengths)
                m = [x.to(dev) for x in masks] if use_masks else None
                got = eng.forward_ragged(wav.to(dev), offsets, lengths, m)
            finally:
                del eng.RAGGED_RATIO
            assert got.shape == (len(lengths), 256) and torch.isfinite(got).all()
            for i in range(len(waves)):
                name = f"{tag}_ragged_{i}_{use_masks}_{ratio:g}"
                assert north_star_ratio(name, got[i:i + 1], wants[i]) <= 1.0
                assert north_star_ratio(name + "_vs_alone", got[i:i + 1], alones[i]) <= 1.0


def test_forward_ragged_basicblock(models):
    oracle, model = models["wespeaker"]
    lengths = _ragged_lengths()
    perm = np.random.default_rng(0).permutation(len(lengths))      # input order != length order
    _check_ragged(oracle, model.engine, [lengths[i] for i in perm], "basic")


def test_forward_ragged_bottleneck(gpu_device):
    from oracle.models import Bottleneck, WeSpeakerResNet34 as OracleNet
    from pyannote_audio_amd.embedding import EmbeddingEngine
    from pyannote_audio_amd.weights import EmbeddingPack
    torch.manual_seed(11)
    model = OracleNet(num_blocks=(1, 1, 1, 1), block=Bottleneck).eval()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.6, 1.2)
                m.bias.normal_(0, 0.1)
    eng = EmbeddingEngine(EmbeddingPack(model.state_dict(), gpu_device))
    _check_ragged(model, eng, _ragged_lengths(), "bottleneck")


def test_forward_ragged_rejects_short_utterance(models):
    _, model = models["wespeaker"]
    wav = torch.zeros(20000, device=model.device)
    with pytest.raises(ValueError, match="utterance 1"):
        model.engine.forward_ragged(wav, [0, 8000, 9000], [8000, 399, 8000])


def test_fallbacks_span_checkpoint_and_xvector(models, gpu_device):
    """fbank_centering_span and XVectorSincNet run one launch sequence per distinct length"""
    from oracle import seeded_wespeaker
    from pyannote_audio_amd.embedding import EmbeddingEngine
    from pyannote_audio_amd.weights import EmbeddingPack
    oracle = seeded_wespeaker(seed=4321)
    oracle.fbank_centering_span = 0.4
    eng = EmbeddingEngine(EmbeddingPack(oracle.state_dict(), gpu_device, center_kernel=39))
    xo, xv = models["xvector"]
    lengths = [48000, 70000, 48000, 33333, 70000]
    waves, offsets, wav = _concat(lengths, seed=30)
    g = torch.Generator().manual_seed(2)
    for tag, o, e in (("span", oracle, eng), ("xvector", xo, xv.engine)):
        masks = [(torch.rand(e.num_pool_frames(n) + 5, generator=g) < 0.6).float() for n in lengths]
        for use_masks in (False, True):
            got = e.forward_ragged(wav.to(gpu_device), offsets, lengths,
                                   [m.to(gpu_device) for m in masks] if use_masks else None)
            for i, x in enumerate(waves):
                want = torch.from_numpy(_oracle(o, x[None], masks[i][None] if use_masks else None))
                assert north_star_ratio(f"{tag}_fallback_{i}_{use_masks}", got[i:i + 1], want) <= 1.0
