"""pa_emb_forward on chunks that overlap by whole frame shifts: the fbank frames of the span are computed once, the
per-chunk means go beside them and the stem subtracts while it stages (csrc/emb_forward.cpp: `shared`).  By construction
that is bit for bit the per-chunk sequence, so every comparison here is `torch.equal`, on the embeddings of the seeded
ResNet34 and of the Bottleneck network of tests/entry_cases.py:

  * the default against PA_EMB_SHARED_FBANK=0 (the per-chunk sequence on the same overlapping chunks);
  * the default against the same chunks gathered into a non-overlapping copy (zero padded past the end of the signal),
    which is what a pipeline's inactive-chunk skip hands over and which takes the per-chunk sequence by itself.

Which sequence a call took is read from the built-in profiler (the mean kernel has a scope of its own) and held against
the selection rule: chunk_stride a positive multiple of 160, B >= 2, and (B - 1) fps + T frames + B means within the
B T rows the plan reserves -- T - fps = 2 is the first overlap that fits, T - fps = 1 does not.

Shapes: T = 3 (the two halo frames of a chunk are both chunk edges), 4 (one whole FB_FPB block), 7, 48 (several stem
columns per thread, fps = 10 fits); B = 1, 2, 5, 9 (the span's last k_fbank block is partial or not); strides that share
(160, 320, 1 600 at T = 48, T - fps = 2) and that do not (T - fps = 1, 161, N, 1 600 at T < 12); a signal that ends with
the span, inside the last frame of the last chunk, and before the last chunk begins.  The signal is noise under an
amplitude ramp: neighbouring frames and the means of neighbouring chunks differ, so a frame of the wrong chunk, a halo
read from the neighbouring file frame or a mean of the wrong rows changes bits.  The workspace and the output hold NaN
before every call."""
import pytest
import torch

import entry_cases as ec

pytestmark = pytest.mark.gpu

S, FM = 3, 11                    # masks per chunk; mask frames (any rate: mapped to the pool frames by nearest index)
ENV = "PA_EMB_SHARED_FBANK"


def _samples(T):
    return 400 + 160 * (T - 1)


def _strides(T):
    """sharing and falling back, without repeats: T - fps = 1 (does not fit), T - fps = 2 (the first that does)"""
    N = _samples(T)
    return [s for s in dict.fromkeys([160, 320, 1600, 160 * (T - 1), 160 * (T - 2), 161, N]) if s > 0]


def _shares(T, B, stride):
    """the selection rule of emb_forward_impl for a network with global centring"""
    if stride % 160 != 0 or B < 2:
        return False
    fps = stride // 160
    return (B - 1) * fps + T + B <= B * T


def _signal(n, seed):
    g = torch.Generator().manual_seed(seed)
    ramp = torch.linspace(0.05, 1.0, n)
    return (0.3 * torch.randn(n, generator=g) * ramp + 0.01).clamp(-1, 1)


def _masks(B, seed):
    g = torch.Generator().manual_seed(seed)
    masks = (torch.rand(B, S, FM, generator=g) < 0.6).float()
    masks[B - 1, 0] = 0.0        # an empty mask: the bias path
    return masks


def _forward(eng, dev, wav, stride, B, N, masks, idx):
    """one pa_emb_forward on a workspace and an output full of NaN -> (embeddings, kernels the profiler saw)"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    w = eng.pack.struct
    need = lib.pa_emb_workspace_bytes(w, B, N, S)
    assert need % 4 == 0
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=dev)
    emb = torch.full((B, S, 256), float("nan"), dtype=torch.float32, device=dev)
    ffi.prof_enable(True)
    try:
        ffi.prof_report()
        rc = lib.pa_emb_forward(w, ec.p(wav), wav.numel(), stride, B, N, ec.p(masks), S, FM, ec.p(idx), ec.p(emb),
                                ec.p(ws), need, ffi.stream())
        torch.cuda.synchronize()
        kernels = ffi.prof_report()
    finally:
        ffi.prof_enable(False)
    assert rc == 0, lib.pa_last_error()
    assert not torch.isnan(emb).any()
    return emb, kernels


def _check(eng, dev, monkeypatch, T, B, stride, ending):
    N = _samples(T)
    span = (B - 1) * stride + N
    wav_len = {"span": span, "cut": span - 137, "early": max((B - 1) * stride - 3, 1)}[ending]
    what = f"T={T} B={B} stride={stride} wav_len={wav_len} of {span}"
    x = _signal(wav_len, seed=1000 * T + 10 * B + stride % 7)
    padded = torch.cat([x, torch.zeros(span - wav_len)])
    compact = torch.stack([padded[b * stride:b * stride + N] for b in range(B)]).reshape(-1)
    wav, compact = x.to(dev), compact.to(dev)
    masks = _masks(B, seed=B + T).to(dev)
    idx = eng.nearest_index(FM, eng.num_pool_frames(N))

    monkeypatch.delenv(ENV, raising=False)
    got, kernels = _forward(eng, dev, wav, stride, B, N, masks, idx)
    shared = "k_fbank_chunk_mean" in kernels
    assert shared == _shares(T, B, stride), what
    flops = kernels["k_fbank"]["flops"]
    monkeypatch.setenv(ENV, "0")
    per_chunk, kernels = _forward(eng, dev, wav, stride, B, N, masks, idx)
    assert "k_fbank_chunk_mean" not in kernels, what
    # the scope k_fbank declares the frames it computes (the report prints seven digits)
    frames = (B - 1) * (stride // 160) + T if shared else B * T
    assert flops * B * T == pytest.approx(kernels["k_fbank"]["flops"] * frames, rel=1e-5), what
    monkeypatch.delenv(ENV)
    gathered, kernels = _forward(eng, dev, compact, N, B, N, masks, idx)
    assert "k_fbank_chunk_mean" not in kernels, what
    assert torch.equal(per_chunk, gathered), what       # (the two per-chunk runs: the test's own inputs agree)
    assert torch.equal(got, per_chunk), what
    assert torch.equal(got, gathered), what


@pytest.mark.parametrize("T", [3, 4, 7, 48])
def test_shared_frames_give_the_bits_of_the_per_chunk_sequence(gpu_device, monkeypatch, T):
    _, eng = ec.emb_models(gpu_device)["basic"]
    ran = 0
    for B in (1, 2, 5, 9):
        for stride in _strides(T):
            for ending in ("span", "cut", "early"):
                _check(eng, gpu_device, monkeypatch, T, B, stride, ending)
                ran += _shares(T, B, stride)
    assert ran >= 9, "every B >= 2 shares at a stride of one frame shift, with every ending"


@pytest.mark.parametrize("T", [7, 48])
def test_shared_frames_under_a_bottleneck_network(gpu_device, monkeypatch, T):
    _, eng = ec.emb_models(gpu_device)["bottleneck"]
    for B in (2, 5):
        for stride in _strides(T):
            for ending in ("span", "cut", "early"):
                _check(eng, gpu_device, monkeypatch, T, B, stride, ending)


def test_the_switch_is_read_on_every_call(gpu_device, monkeypatch):
    """PA_EMB_SHARED_FBANK is no static of the library: one process takes both sequences, in either order"""
    _, eng = ec.emb_models(gpu_device)["basic"]
    T, B, stride = 7, 5, 320
    N = _samples(T)
    wav = _signal((B - 1) * stride + N, seed=3).to(gpu_device)
    masks = _masks(B, seed=2).to(gpu_device)
    idx = eng.nearest_index(FM, eng.num_pool_frames(N))
    seen = []
    for value in ("0", None, "1", "0", None):
        if value is None:
            monkeypatch.delenv(ENV, raising=False)
        else:
            monkeypatch.setenv(ENV, value)
        _, kernels = _forward(eng, gpu_device, wav, stride, B, N, masks, idx)
        seen.append("k_fbank_chunk_mean" in kernels)
    assert seen == [False, True, True, False, True]
