"""GPU parity of XVectorMFCC (models/embedding/xvector.py:42-202): the HIP MFCC front end (csrc/mfcc.hip,
`pa_mfcc_features`) against the float64 restatement of torchaudio's MFCC, the whole model (`pa_xvec_mfcc_forward`)
against the float32 oracle module at the north_star tolerance |d| <= 1e-5 + 1e-4 |ref|, and the public paths built
on it (Inference, SpeakerEmbedding, SpeakerDiarization).  The oracle is pinned to the reference's class by
tests/test_xvector_mfcc_cpu.py."""
import math

import numpy as np
import pytest
import torch

import xvector_mfcc_oracle as xo
from conftest import north_star_ratio

pytestmark = pytest.mark.gpu

SR = 16000
CONFIGS = {"default": None, "uncentred_hop160": {"melkwargs": {"center": False, "hop_length": 160}},
           "log_mels": {"log_mels": True}, "n_mfcc24": {"n_mfcc": 24}, "n_mfcc64": {"n_mfcc": 64}}


def _noise(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(n, generator=g)).clamp(-1, 1)


def _band_limited_with_silence(n, seed):
    """noise low-passed to ~2 kHz (a 9-tap moving average), with stretches of exact digital silence"""
    x = torch.nn.functional.avg_pool1d(_noise(n + 8, seed)[None, None], 9, stride=1)[0, 0] * 3.0
    for a, b in ((0.3, 0.9), (1.7, 1.75), (3.0, 3.6)):
        x[int(a * SR):int(b * SR)] = 0.0
    return x


def _tone(n, seed):
    """a -30 dBFS 440 Hz tone: most mel cells sit on the -80 dB clamp"""
    t = torch.arange(n, dtype=torch.float64) / SR
    return (10 ** (-30 / 20) * torch.sin(2 * math.pi * 440.0 * t + 0.1 * seed)).float()


SIGNALS = {"noise": _noise, "band_silence": _band_limited_with_silence, "tone": _tone}


def _model(gpu_device, mfcc=None, seed=3579):
    import pyannote_audio_amd as pa
    oracle = xo.seeded_xvector_mfcc(seed=seed, mfcc=mfcc)
    model = pa.XVectorMFCC(oracle.state_dict(), xo.xvector_mfcc_hparams(oracle), pa.model.embedding_specifications())
    return oracle, model.to(gpu_device)


def _chunks(wav, step, count, size):
    """the reference's chunks: the last ones zero-padded past the end of the waveform"""
    out = torch.zeros(count, 1, size)
    for c in range(count):
        seg = wav[c * step:c * step + size]
        out[c, 0, :seg.numel()] = seg
    return out


# ------------------------------------------------------------------------------------------------ front end
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("signal", list(SIGNALS))
def test_mfcc_features_against_float64(gpu_device, config, signal):
    oracle, model = _model(gpu_device, CONFIGS[config])
    total, N, step, C = 72000, 32000, 16000, 4            # chunk 3 runs 8000 samples past the end
    wav = SIGNALS[signal](total, seed=7)
    got = model.engine.features(wav.to(gpu_device), step, C, N).cpu().double()
    exact = xo.MFCC(**oracle.hparams_mfcc, dtype=torch.float64)
    with torch.inference_mode():
        want = exact(_chunks(wav, step, C, N).double()).squeeze(1).transpose(1, 2)
    assert got.shape == want.shape
    assert torch.isfinite(got).all()
    for c in range(C):
        err = (got[c] - want[c]).abs().max().item()
        scale = want[c].abs().max().item()
        assert err <= 2e-4 * scale, f"chunk {c}: |d| = {err:.3e} > 2e-4 x {scale:.3e}"


def test_mfcc_features_of_a_silent_chunk(gpu_device):
    """all-zero input: every mel energy is 0 -> -100 dB everywhere (the clamp at -180 never acts)"""
    oracle, model = _model(gpu_device)
    got = model.engine.features(torch.zeros(48000, device=gpu_device), 16000, 2, 32000).cpu().double()
    with torch.inference_mode():
        want = xo.MFCC(**oracle.hparams_mfcc, dtype=torch.float64)(torch.zeros(2, 1, 32000, dtype=torch.float64))
    want = want.squeeze(1).transpose(1, 2)
    assert (got - want).abs().max().item() <= 2e-4 * want.abs().max().item()


# ------------------------------------------------------------------------------------------------ embeddings
@pytest.mark.parametrize("B,N", [(1, 48000), (5, 80000), (19, 160000)])
def test_embeddings_against_oracle(gpu_device, B, N):
    oracle, model = _model(gpu_device)
    g = torch.Generator().manual_seed(B)
    wav = torch.stack([_noise(N, seed=B * 10 + b) + 0.05 * _tone(N, b) for b in range(B)])[:, None]
    Tp = model.num_frames(N)
    Fm = Tp + 14
    weights = (torch.rand(B, 3, Fm, generator=g) < 0.6).float()
    weights[0, 1] = 0.0                                    # an all-zero mask
    with torch.inference_mode():
        want = torch.stack([oracle(wav, weights=weights[:, s]) for s in range(3)], dim=1)
        want_u = oracle(wav)
    got = model(wav.to(gpu_device), weights.to(gpu_device))
    assert got.shape == (B, 3, 512)
    assert north_star_ratio(f"xvector_mfcc_B{B}_N{N}", got, want) <= 1.0
    got_u = model(wav.to(gpu_device))
    assert north_star_ratio(f"xvector_mfcc_unweighted_B{B}_N{N}", got_u, want_u) <= 1.0


@pytest.mark.parametrize("config", ["uncentred_hop160", "log_mels", "n_mfcc64"])
def test_strided_chunks_past_the_end(gpu_device, config):
    oracle, model = _model(gpu_device, CONFIGS[config])
    total, N, step, C = 16000 * 14 - 3000, 80000, 16000, 10    # the last chunks zero-padded
    wav = _band_limited_with_silence(total, seed=2)
    g = torch.Generator().manual_seed(5)
    masks = (torch.rand(C, 3, 293, generator=g) < 0.7).float()
    masks[2, 0] = 0.0
    with torch.inference_mode():
        want = torch.stack([oracle(_chunks(wav, step, C, N), weights=masks[:, s]) for s in range(3)], dim=1)
    got = model.engine.forward_strided(wav.to(gpu_device), step, C, N, masks.to(gpu_device))
    assert north_star_ratio(f"xvector_mfcc_strided_{config}", got, want) <= 1.0


def test_tone_no_worse_than_float32_reference(gpu_device):
    """a -30 dBFS tone puts most cells on the -80 dB clamp.  The HIP front end adds no more error than the reference's
    own float32 MFCC: the oracle's float32 layers fed with the HIP MFCCs are within twice the float32 oracle's distance
    to the float64 oracle.  The whole HIP model stays well inside the north_star tolerance of both oracles (measured:
    0.058 of it against float64, where the float32 oracle is at 0.017 -- the difference is the TDNN GEMMs' float32
    summation order, shared with XVectorSincNet)."""
    oracle, model = _model(gpu_device)
    wav = torch.stack([_tone(80000, s) for s in range(3)])[:, None]
    exact = xo.as_float64(oracle)
    feats = model.engine.features(wav.view(-1).to(gpu_device), 80000, 3, 80000).cpu().transpose(1, 2)
    with torch.inference_mode():
        want64 = exact(wav.double())
        want32 = oracle(wav)
        mixed = feats
        for tdnn in oracle.tdnns:
            mixed = tdnn(mixed)
        mixed = oracle.embedding(oracle.stats_pool(mixed))
    got = model(wav.to(gpu_device))
    r32 = north_star_ratio("xvector_mfcc_tone_f32_vs_f64", want32, want64)
    rfront = north_star_ratio("xvector_mfcc_tone_hip_mfcc_f32_layers_vs_f64", mixed, want64)
    assert rfront <= 2.0 * r32, (rfront, r32)
    assert north_star_ratio("xvector_mfcc_tone_hip_vs_f64", got, want64) <= 0.25
    assert north_star_ratio("xvector_mfcc_tone_hip_vs_f32", got, want32) <= 1.0


def test_too_short(gpu_device):
    _, model = _model(gpu_device)
    assert model.num_frames(2799) == 0 and model.num_frames(2800) == 1
    assert model.engine.num_pool_frames(2799) == 0 and model.engine.num_pool_frames(2800) == 1
    with pytest.raises(ValueError, match="2799"):
        model.engine.forward(torch.zeros(1, 1, 2799, device=gpu_device))
    with pytest.raises(ValueError, match="2799 samples"):
        model.engine.forward_ragged(torch.zeros(9000, device=gpu_device), [0, 3000], [4000, 2799])


# ------------------------------------------------------------------------------------------------ public paths
def _file(wav):
    return {"waveform": wav, "sample_rate": SR, "uri": f"utt{wav.shape[1]}"}


def test_inference_sliding_whole_crop(gpu_device):
    from pyannote_audio_amd import Audio, Inference, Segment
    oracle, model = _model(gpu_device)
    wav = (_noise(int(20.5 * SR), 3) + _tone(int(20.5 * SR), 1))[None]
    out = Inference(model, window="sliding", duration=3.0, step=1.0, batch_size=8)(_file(wav))
    window, step = 3 * SR, SR
    n = (wav.shape[1] - window) // step + 1
    with torch.inference_mode():
        want = oracle(_chunks(wav[0], step, n + 1, window)).numpy()
    assert out.data.shape == (n + 1, 512)
    assert north_star_ratio("xvector_mfcc_sliding", torch.from_numpy(out.data), torch.from_numpy(want)) <= 1.0
    whole = Inference(model, window="whole")
    got = whole(_file(wav))                             # 1 601 MFCC frames: the long pooling kernel
    with torch.inference_mode():
        want = oracle(wav[None]).numpy()[0]
    assert north_star_ratio("xvector_mfcc_whole", torch.from_numpy(got), torch.from_numpy(want)) <= 1.0
    seg = Segment(1.25, 7.5)
    got = whole.crop(_file(wav), seg)
    with torch.inference_mode():
        want = oracle(Audio(SR, mono="downmix").crop(_file(wav), seg)[0][None]).numpy()[0]
    assert north_star_ratio("xvector_mfcc_crop", torch.from_numpy(got), torch.from_numpy(want)) <= 1.0


def test_speaker_embedding_apply_batch_equals_apply(gpu_device):
    from pyannote_audio_amd import SpeakerEmbedding
    oracle, model = _model(gpu_device)
    pipeline = SpeakerEmbedding(embedding=model)
    lengths = [int(2.0 * SR), int(3.3 * SR), int(2.0 * SR), int(6.1 * SR), int(4.4 * SR)]
    files = [_file((_noise(n, i) + 0.5 * _tone(n, i))[None]) for i, n in enumerate(lengths)]
    batch = pipeline.apply_batch(files)
    for i, f in enumerate(files):
        one = pipeline.apply(f)
        assert north_star_ratio(f"xvector_mfcc_apply_batch_{i}", torch.from_numpy(batch[i]),
                                torch.from_numpy(one)) <= 1.0
        with torch.inference_mode():
            want = oracle(f["waveform"][None]).numpy()
        assert north_star_ratio(f"xvector_mfcc_apply_{i}", torch.from_numpy(one), torch.from_numpy(want)) <= 1.0


def test_pipeline_with_xvector_mfcc_embeddings(synthetic_models, gpu_device, tmp_path):
    """the diarization pipeline with an XVectorMFCC checkpoint as `embedding` (config.yaml directory): loader,
    wrapper properties (min_num_samples 2800 = one pool frame), all stages against the oracle"""
    import os
    import pyannote_audio_amd as pa
    from conftest import write_pipeline_dir
    from oracle.pipeline import diarize
    from oracle.synthetic import synth_conversation
    from pyannote_audio_amd.model import embedding_specifications, save_checkpoint
    seg_o, _ = synthetic_models
    emb_o = xo.seeded_xvector_mfcc()
    write_pipeline_dir(tmp_path, seg_o, emb_o)
    save_checkpoint(os.path.join(str(tmp_path), "embedding", "pytorch_model.bin"), emb_o.state_dict(),
                    xo.xvector_mfcc_hparams(emb_o), pa.XVectorMFCC.ARCHITECTURE, embedding_specifications())
    pipeline = pa.Pipeline.from_pretrained(str(tmp_path)).to(gpu_device)
    assert isinstance(pipeline._embedding.model_, pa.XVectorMFCC)
    assert pipeline._embedding.dimension == 512 and pipeline._embedding.min_num_samples == 2800
    conv, _ = synth_conversation(26.0, seed=4)
    seen = {}

    def hook(name, artefact, file=None, **kw):
        if artefact is not None and kw.get("total") is None:
            seen[name] = np.array(getattr(artefact, "data", artefact), copy=True)

    out = pipeline({"waveform": conv, "sample_rate": SR, "uri": "conv"}, hook=hook)
    want = diarize(seg_o, emb_o, conv, exclude_overlap=True, min_num_samples=2800)
    assert np.array_equal(seen["segmentation"], want.segmentations)
    assert north_star_ratio("xvector_mfcc_pipeline_embeddings", seen["embeddings"], want.embeddings) <= 1.0
    got = [(s.start, s.end, l) for s, _, l in out.speaker_diarization.itertracks(yield_label=True)]
    assert got == want.diarization


@pytest.mark.parametrize("case", ["one_sample_short", "workspace_one_byte_short"])
def test_pa_xvec_mfcc_forward_refusals(gpu_device, case):
    """what pa_xvec_mfcc_forward refuses, it refuses with code 3, the same words as ever and no write (tests/refusals.py)"""
    import pyannote_audio_amd.ffi as ffi
    from refusals import check_refusal, smallest_accepted
    lib = ffi.load()
    eng = _model(gpu_device)[1].engine
    B, N, S = 2, 16000, 1
    w, n = eng.pack.struct, N
    g = torch.Generator().manual_seed(9)
    wav = (0.1 * torch.randn(B * N, generator=g)).clamp(-1, 1).to(gpu_device)
    need = lib.pa_xvec_mfcc_workspace_bytes(w, B, N, S)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    if case == "one_sample_short":
        n = smallest_accepted(eng.num_pool_frames) - 1
        message = f"pa_xvec_mfcc_forward: {n} samples leave no frame after the MFCC front end + the TDNN stack"
    else:
        need -= 1
        message = f"pa_xvec_mfcc_forward: workspace too small ({need} < {need + 1} bytes)"
    check_refusal(lambda emb: lib.pa_xvec_mfcc_forward(w, ffi.ptr(wav), wav.numel(), N, B, n, None, S, 0, None, emb,
                                                     ffi.ptr(ws), need, ffi.stream()),
                  [((B, S, w.dimension), torch.float32)], message, gpu_device)
