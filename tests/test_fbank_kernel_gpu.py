"""The filterbank kernels (csrc/emb_fbank.hip: k_fbank<false / true>, k_fbank_center, k_fbank_center_ragged) through
`pa_fbank` and `pa_fbank_ragged`, against the float64 truth of tests/fbank_truth.py on signals with dynamics: quiet
frames beside loud ones, quiet bands beside strong ones, digital silence, a `wav_len` that ends inside a chunk, chunks
that overlap, 1 to 60000 frames through the centring.  Truth, tolerance, step model, signals and the admissibility of
each are checked on the CPU by tests/test_fbank_truth_cpu.py; the rules of the comparison are those of
tests/kernel_parity.py (outputs in NaN-filled guarded buffers, the waveform between blocks of +-1e30)."""
import numpy as np
import pytest
import torch

import fbank_truth as ft
from kernel_parity import Guarded, GuardedInput, assert_parity, dptr

pytestmark = pytest.mark.gpu


def _log(line):
    """every measured figure goes to the test's output (pytest -s, or the captured output of a failure)"""
    print(line)


@pytest.fixture(scope="module")
def fb(gpu_device):
    """(lib, the device tables of an EmbeddingPack -- kept alive by the pack)"""
    import pyannote_audio_amd.ffi as ffi
    from oracle import seeded_wespeaker
    from pyannote_audio_amd.weights import EmbeddingPack
    pack = EmbeddingPack(seeded_wespeaker(seed=4321).state_dict(), gpu_device, guard=False)
    return ffi.load(), pack


def _fbank(fb, wav_ptr, wav_len, stride, B, N, out_ptr, center):
    import pyannote_audio_amd.ffi as ffi
    lib, pack = fb
    w = pack.struct
    ffi.check(lib.pa_fbank(wav_ptr, wav_len, stride, B, N, w.fb_window, w.fb_tw256, w.fb_tw512, w.fb_mel_w, w.fb_mel_lo,
                           w.fb_mel_hi, ft.NMEL, out_ptr, center, ffi.stream()), "pa_fbank")


def _fbank_ragged(fb, wav_ptr, wav_len, offsets, lengths, nmax, out_ptr, device):
    import pyannote_audio_amd.ffi as ffi
    lib, pack = fb
    w = pack.struct
    od = torch.tensor(offsets, dtype=torch.int64, device=device)
    ld = torch.tensor(lengths, dtype=torch.int32, device=device)
    ffi.check(lib.pa_fbank_ragged(wav_ptr, wav_len, dptr(od), dptr(ld), len(lengths), nmax, w.fb_window, w.fb_tw256,
                                  w.fb_tw512, w.fb_mel_w, w.fb_mel_lo, w.fb_mel_hi, ft.NMEL, out_ptr, ffi.stream()),
              "pa_fbank_ragged")
    torch.cuda.synchronize()


def _single(fb, x, center, device):
    """pa_fbank of one chunk that is the whole (guarded) waveform -> (T, 80) on the CPU"""
    x = torch.as_tensor(x)
    n, T = x.numel(), ft.num_frames(x.numel())
    wav, out = GuardedInput(x, device), Guarded(T * ft.NMEL, device)
    _fbank(fb, wav.ptr, n, n, 1, n, out.ptr, center)
    return out.check(None, f"pa_fbank({n} samples, center={center})").view(T, ft.NMEL).clone()


def _hold_to_truth(name, got, chunks):
    """every chunk of `got` (B, T, 80) log features against its truth and against the step model; -> the worst ratios
    (float32 oracle, step model, kernel, kernel against the step model)"""
    worst = np.zeros(4)
    ulp = float(np.spacing(np.abs(ft.LOG_EPS32)))
    for b, ch in enumerate(chunks):
        assert ch["r_oracle"] <= 0.5 and ch["r_model"] <= 0.5, f"{name}: inadmissible case (chunk {b}): choose other inputs"
        g = got[b].numpy()
        assert g.shape == ch["Ef"].shape
        r = ft.ratio(g, ch["Ef"], ch["tol"])
        r_vs_model = ft.ratio(g, ch["model"].astype(np.float64), ch["tol"])
        _log(f"fbank_truth {name} chunk {b}: float32 oracle {ch['r_oracle']:.3f} step model {ch['r_model']:.3f} "
             f"kernel {r:.3f} kernel against the step model {r_vs_model:.3f} "
             f"({int(ch['floor'].sum())} of {g.shape[0]} frames at the floor)")
        limit = max(1.0, 2.0 * ch["r_oracle"])
        assert r <= limit, (name, b, r, ch["r_oracle"])
        assert r_vs_model <= limit, (name, b, r_vs_model, ch["r_oracle"])
        at_floor = g[ch["floor"]].astype(np.float64)
        assert (np.abs(at_floor - float(ft.LOG_EPS32)) <= ulp).all(), (name, b, "a silent frame off log(eps32)")
        worst = np.maximum(worst, [ch["r_oracle"], ch["r_model"], r, r_vs_model])
    return worst


@pytest.mark.parametrize("name", list(ft.SIGNALS))
def test_fbank_uncentred(fb, gpu_device, name):
    """3 chunks of 24000 samples every 12000, cut from 48000 samples of which the kernel is told 43000: the last chunk
    reads zeros from there on, with real samples and then +-1e30 behind"""
    case = ft.layout_case(name)
    B, T = case["B"], ft.num_frames(ft.N)
    assert B == 3 and (B - 1) * ft.STRIDE + ft.N == ft.TOTAL and case["wav_len"] == ft.TOTAL - ft.CUT
    wav, out = GuardedInput(torch.from_numpy(case["data"]), gpu_device), Guarded(B * T * ft.NMEL, gpu_device)
    _fbank(fb, wav.ptr, case["wav_len"], ft.STRIDE, B, ft.N, out.ptr, 0)
    got = out.check(None, name).view(B, T, ft.NMEL)
    worst = _hold_to_truth(name, got, case["chunks"])
    _log(f"fbank_truth {name}: float32 oracle {worst[0]:.3f} step model {worst[1]:.3f} kernel {worst[2]:.3f} "
         f"kernel against the step model {worst[3]:.3f}")


@pytest.mark.parametrize("name", ["harmonic_envelope", "silence_burst"])
def test_fbank_framing_edges_with_dynamics(fb, gpu_device, name):
    """the lengths of test_fuzz_fbank_lengths (one frame exactly, one sample more, one short of the next hop, ...) on two
    signals with silent stretches, two chunks back to back"""
    lib, _ = fb
    for n in ft.EDGE_LENGTHS:
        case = ft.edge_case(name, n)
        T = lib.pa_emb_num_fbank_frames(n)
        assert T == ft.num_frames(n) == case["chunks"][0]["Ef"].shape[0]
        wav, out = GuardedInput(torch.from_numpy(case["data"]), gpu_device), Guarded(2 * T * ft.NMEL, gpu_device)
        _fbank(fb, wav.ptr, 2 * n, n, 2, n, out.ptr, 0)
        _hold_to_truth(f"{name}_N{n}", out.check(None, f"{name} N {n}").view(2, T, ft.NMEL), case["chunks"])


RAGGED = [(400, "white"), (561, "dc025_envelope"), (719, "silence_clicks"), (4800, "impulses"), (23456, "speech"),
          (48001, "harmonic_envelope")]


def test_fbank_ragged_is_the_single_form_per_utterance(fb, gpu_device):
    """utterances of different signals at unaligned offsets, 37 samples of +-1e30 that belong to nobody between them:
    every utterance's rows are bit-identical to pa_fbank(center = 1) of that utterance alone, the rows behind its own
    frame count exact +0"""
    gap, lead = 37, 3
    xs = [torch.from_numpy(ft.signal(name, n, seed=77)) for n, name in RAGGED]
    total = lead + sum(n + gap for n, _ in RAGGED)
    data = torch.full((total,), GuardedInput.POISON)
    data[1::2] = -GuardedInput.POISON
    offsets, pos = [], lead
    for x in xs:
        offsets.append(pos)
        data[pos:pos + x.numel()] = x
        pos += x.numel() + gap
    lengths = [n for n, _ in RAGGED]
    nmax = max(lengths)
    T = ft.num_frames(nmax)
    wav, out = GuardedInput(data, gpu_device), Guarded(len(lengths) * T * ft.NMEL, gpu_device)
    _fbank_ragged(fb, wav.ptr, total, offsets, lengths, nmax, out.ptr, gpu_device)
    got = out.check(None, "pa_fbank_ragged").view(len(lengths), T, ft.NMEL)
    for b, (n, name) in enumerate(RAGGED):
        Tb = ft.num_frames(n)
        alone = _single(fb, xs[b], 1, gpu_device)
        assert torch.equal(got[b, :Tb], alone), (n, name, (got[b, :Tb] - alone).abs().max().item())
        assert bool((got[b, Tb:] == 0).all()) and not bool(torch.signbit(got[b, Tb:]).any()), (n, name)


# ---------------------------------------------------------------------------------------------------------------------
# centring alone
# ---------------------------------------------------------------------------------------------------------------------
_CENTRED = {}


def _centred(fb, device, T):
    """(x, U, C) of T frames of drifting noise: the waveform, pa_fbank(center = 0) and pa_fbank(center = 1) of it"""
    if T not in _CENTRED:
        x = torch.from_numpy(ft.drifting_noise(T))
        _CENTRED[T] = (x, _single(fb, x, 0, device), _single(fb, x, 1, device))
    return _CENTRED[T]


@pytest.mark.parametrize("T", ft.CENTER_FRAMES)
def test_fbank_centring(fb, gpu_device, T):
    """C = pa_fbank(center = 1) against U - mean over the frames of U = pa_fbank(center = 0), the mean in float64: the
    project's contract (rtol 1e-4 / atol 1e-5), whatever the number of frames the four partial sums are split over"""
    _, U, C = _centred(fb, gpu_device, T)
    assert tuple(U.shape) == tuple(C.shape) == (T, ft.NMEL)
    if T == 1:
        assert bool((C == 0).all())
        return
    truth = U.double() - U.double().mean(dim=0, keepdim=True)
    ref32 = U - U.mean(dim=0, keepdim=True)
    assert_parity(f"fbank_centring_T{T}", C, truth, ref32)
    _log(f"fbank_centring_T{T}: max |C - truth| = {(C.double() - truth).abs().max().item():.3e} "
         f"(float32 torch {(ref32.double() - truth).abs().max().item():.3e})")


@pytest.mark.parametrize("T", ft.CENTER_FRAMES)
def test_fbank_centring_ragged(fb, gpu_device, T):
    """the same frame counts through pa_fbank_ragged, a short utterance beside the long one: each centred on its own
    mean exactly as it is alone, and to the contract"""
    x, U, C = _centred(fb, gpu_device, T)
    Ts = max(1, min(3, T - 1))
    short = torch.from_numpy(ft.drifting_noise(Ts, seed=1))
    gap = 37
    data = torch.full((short.numel() + gap + x.numel(),), GuardedInput.POISON)
    data[1::2] = -GuardedInput.POISON
    data[:short.numel()] = short
    data[short.numel() + gap:] = x
    wav, out = GuardedInput(data, gpu_device), Guarded(2 * T * ft.NMEL, gpu_device)
    _fbank_ragged(fb, wav.ptr, data.numel(), [0, short.numel() + gap], [short.numel(), x.numel()], x.numel(), out.ptr,
                  gpu_device)
    got = out.check(None, f"pa_fbank_ragged T {T}").view(2, T, ft.NMEL)
    assert torch.equal(got[1], C), (T, (got[1] - C).abs().max().item())
    assert torch.equal(got[0, :Ts], _single(fb, short, 1, gpu_device)), T
    assert bool((got[0, Ts:] == 0).all()) and not bool(torch.signbit(got[0, Ts:]).any()), T
    if T == 1:
        assert bool((got[1] == 0).all())
    else:
        truth = U.double() - U.double().mean(dim=0, keepdim=True)
        assert_parity(f"fbank_centring_ragged_T{T}", got[1], truth, U - U.mean(dim=0, keepdim=True))


def test_fbank_silence_centres_to_exact_zeros(fb, gpu_device):
    """a chunk of digital silence: every feature is log(eps32), and the mean of equal values is that value"""
    for n in (ft.WIN, 880, ft.N, 160000):
        x = torch.zeros(n)
        U, C = _single(fb, x, 0, gpu_device), _single(fb, x, 1, gpu_device)
        assert bool((U == U[0, 0]).all()), n
        assert abs(float(U[0, 0]) - float(ft.LOG_EPS32)) <= float(np.spacing(np.abs(ft.LOG_EPS32))), n
        assert bool((C == 0).all()), (n, C.abs().max().item())
