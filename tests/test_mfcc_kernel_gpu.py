"""The MFCC kernels (csrc/mfcc.hip: k_mfcc_mel, k_mfcc_dct<false>) through `pa_mfcc_features`, against the float64 truth
and the per-cell tolerance of tests/mfcc_truth.py: every admissible (configuration, signal) pair, the top_db floor of
overlapping chunks of unequal loudness, every framing and batch edge, exact zeros and the refusals; and the rows form
(k_mfcc_dct<true>) through `pa_xvec_mfcc_forward` against the float64 oracle.  Truth, tolerance, signals and the
admissibility of each pair are checked on the CPU by tests/test_mfcc_truth_cpu.py; the rules of the comparison are those
of tests/kernel_parity.py (outputs in NaN-filled guarded buffers, the waveform between blocks of +-1e30)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import mfcc_truth as mt
import xvector_mfcc_oracle as xo
from kernel_parity import SEED_OFFSET, Guarded, GuardedInput, assert_parity

pytestmark = pytest.mark.gpu

_MODELS = {}


def _log(line):
    """every measured figure goes to the test's output (pytest -s, or the captured output of a failure)"""
    print(line)


def _model(device, config):
    """(oracle, XVectorMFCC on the device) of one configuration of mfcc_truth.CONFIGS, or of a `mfcc` dict, built once"""
    key = config if isinstance(config, str) else repr(sorted(config.items()))
    if key not in _MODELS:
        import pyannote_audio_amd as pa
        oracle = xo.seeded_xvector_mfcc(seed=3579, mfcc=mt.CONFIGS[config] if isinstance(config, str) else config)
        model = pa.XVectorMFCC(oracle.state_dict(), xo.xvector_mfcc_hparams(oracle), pa.model.embedding_specifications())
        _MODELS[key] = (oracle, model.to(device))
    return _MODELS[key]


def _struct(device, config):
    w = _model(device, config)[1].engine.pack.struct
    cfg = mt.tables(config)["cfg"]
    assert (w.n_mels, w.n_mfcc, w.hop_length, bool(w.center), bool(w.log_mels)) == \
        (cfg["n_mels"], cfg["n_mfcc"], cfg["hop_length"], cfg["center"], cfg["log_mels"])
    return w


def _workspace(w, B, T, device):
    """sized as XVectorMFCCEngine.features sizes it: the mel values, the chunk maxima, alignment"""
    return torch.empty(4 * (B * T * w.n_mels + B + 128), dtype=torch.uint8, device=device)


def _features(w, config, wav_ptr, wav_len, stride, B, N, device, what):
    """pa_mfcc_features into a guarded buffer -> (B, T, n_mfcc) on the CPU"""
    import pyannote_audio_amd.ffi as ffi
    T = mt.num_frames(config, N)
    ws, out = _workspace(w, B, T, device), Guarded(B * T * w.n_mfcc, device)
    ffi.check(ffi.load().pa_mfcc_features(w, wav_ptr, wav_len, stride, B, N, out.ptr, ffi.ptr(ws), ws.numel(),
                                          ffi.stream()), "pa_mfcc_features")
    return out.check(None, what).view(B, T, w.n_mfcc).clone()


def _offset(wav: GuardedInput, samples: int):
    return C.c_void_p(wav.ptr.value + 4 * samples)


def _hold_to_truth(name, config, got, chunks):
    """every chunk of `got` (B, T, n_mfcc) against its truth -> the worst (float32 oracle, kernel) ratios"""
    worst = np.zeros(2)
    for b, ch in enumerate(chunks):
        assert ch["r_oracle"] <= 0.5, f"{name}: inadmissible case (chunk {b}): choose other inputs"
        rc, rm = mt.ratios(config, got[b], ch)
        _log(f"mfcc_truth {name} chunk {b}: float32 oracle {ch['r_oracle']:.3f} kernel {max(rc, rm):.3f} "
             f"(coefficients {rc:.3f}, mel cells {rm:.3f}; {int(ch['on_floor'].sum())} of {ch['v'].size} cells on the "
             "floor)")
        assert max(rc, rm) <= max(1.0, 2.0 * ch["r_oracle"]), (name, b, rc, rm, ch["r_oracle"])
        worst = np.maximum(worst, [ch["r_oracle"], max(rc, rm)])
    return worst


@pytest.mark.parametrize("config", list(mt.CONFIGS))
def test_mfcc_every_admissible_pair(gpu_device, config):
    """three chunks every half chunk, `wav_len` ending inside the last one (the reflection mirrors zeros there, with real
    samples and then +-1e30 behind them in memory)"""
    w = _struct(gpu_device, config)
    assert mt.PAIRS[config]
    for name in mt.PAIRS[config]:
        case = mt.layout_case(config, name)
        wav = GuardedInput(torch.from_numpy(case["data"]), gpu_device)
        got = _features(w, config, wav.ptr, case["wav_len"], case["stride"], case["B"], case["N"], gpu_device, name)
        worst = _hold_to_truth(f"{config} {name}", config, got, case["chunks"])
        _log(f"mfcc_truth {config} {name}: float32 oracle {worst[0]:.3f} kernel {worst[1]:.3f}")


@pytest.mark.parametrize("config", ["default", "m256_c64", "m64_c64_hop160_uncentred"])
def test_mfcc_top_db_is_per_chunk(gpu_device, config):
    """a quiet chunk, a chunk that is half quiet and half 60 dB louder, a loud chunk, each overlapping the next: every
    chunk has its own floor -- it equals, bit for bit, what the kernels give for it alone -- and its own truth"""
    w = _struct(gpu_device, config)
    N, stride, B = 32000, 16000, 3
    g = torch.Generator().manual_seed(4100 + SEED_OFFSET)
    data = (0.3 * torch.randn(64000 + 8, generator=g)).clamp(-1, 1)
    data = torch.nn.functional.avg_pool1d(data[None, None], 9, stride=1)[0, 0].contiguous()    # low-passed: 40 dB of range
    data[:32000] *= 1e-3
    wav = GuardedInput(data, gpu_device)
    got = _features(w, config, wav.ptr, 64000, stride, B, N, gpu_device, "three chunks")
    chunks = [mt.evaluate(config, data[b * stride:b * stride + N].numpy()) for b in range(B)]
    peaks = [ch["v"].max() for ch in chunks]
    assert peaks[1] - peaks[0] > 55.0
    # the quiet half of chunk 1 is on that chunk's floor where the same samples, in chunk 0, are not
    assert int(chunks[0]["on_floor"].sum()) == 0 and int(chunks[1]["on_floor"].sum()) > 0
    _hold_to_truth(f"top_db {config}", config, got, chunks)
    for b in range(B):
        alone = _features(w, config, _offset(wav, b * stride), 64000 - b * stride, N, 1, N, gpu_device, f"chunk {b}")
        assert torch.equal(alone[0], got[b]), (config, b, (alone[0] - got[b]).abs().max().item())


@pytest.mark.parametrize("config", list(mt.EDGE_LENGTHS))
def test_mfcc_framing_edges(gpu_device, config):
    """one frame exactly, one sample more, one short of the next hop, one frame more or less than the 16-frame block of
    k_mfcc_dct and the 4-frame block of k_mfcc_mel: two chunks back to back, every output inside guards"""
    w = _struct(gpu_device, config)
    for name in mt.EDGE_SIGNALS:
        for n in mt.EDGE_LENGTHS[config]:
            case = mt.edge_case(config, name, n)
            wav = GuardedInput(torch.from_numpy(case["data"]), gpu_device)
            got = _features(w, config, wav.ptr, 2 * n, n, 2, n, gpu_device, f"{config} {name} N {n}")
            _hold_to_truth(f"{config} {name} N{n}", config, got, case["chunks"])


@pytest.mark.parametrize("B", [1, 17])
def test_mfcc_batch_edges(gpu_device, B):
    """one chunk, and seventeen (chunk 16 behind a 16-chunk tile boundary) of 17 frames each: every chunk to its truth,
    and the last equal to itself alone"""
    config, n = "default", 3200
    assert mt.num_frames(config, n) == 17
    w = _struct(gpu_device, config)
    case = mt.edge_case(config, "white", n, B)
    wav = GuardedInput(torch.from_numpy(case["data"]), gpu_device)
    got = _features(w, config, wav.ptr, B * n, n, B, n, gpu_device, f"B {B}")
    _hold_to_truth(f"batch B{B}", config, got, case["chunks"])
    alone = _features(w, config, _offset(wav, (B - 1) * n), n, n, 1, n, gpu_device, "the last chunk alone")
    assert torch.equal(alone[0], got[B - 1])


@pytest.mark.parametrize("config", ["default", "m256_c64", "dct_none", "log_mels", "m64_c64_hop160_uncentred"])
def test_mfcc_exact_zeros(gpu_device, config):
    """digital silence: every mel value is -100 dB (the floor at -180 never acts), log(1e-6) with log_mels, and every
    coefficient is the DCT of that constant column to the rounding of the dot product"""
    w = _struct(gpu_device, config)
    tb = mt.tables(config)
    n, B = 3201, 2
    wav = GuardedInput(torch.zeros(B * n), gpu_device)
    got = _features(w, config, wav.ptr, B * n, n, B, n, gpu_device, f"zeros {config}")
    tr = mt.truth(config, np.zeros(n, dtype=np.float32))
    v0 = float(np.log(1e-6)) if tb["cfg"]["log_mels"] else -100.0
    assert (tr["v"] == v0).all() and np.allclose(tr["c"], v0 * tb["D"].sum(axis=0)[None, :], rtol=0, atol=1e-9)
    for b in range(B):
        r = mt.ratio(config, got[b], tr)
        _log(f"mfcc_truth zeros {config} chunk {b}: kernel {r:.3f}")
        assert r <= 1.0, (config, b, r)
    assert torch.equal(got[0], got[1]) and bool((got[0] == got[0][0:1]).all())       # every frame the same bits


REFUSALS = {
    "n_mels_257": (dict(n_mels=257), "default", 32000,
                   "pa_mfcc: 1 <= n_mels <= 256, 1 <= n_mfcc <= 64 and 1 <= hop_length <= 400 required (got 257, 40, 200)"),
    "n_mfcc_65": (dict(n_mfcc=65), "default", 32000,
                  "pa_mfcc: 1 <= n_mels <= 256, 1 <= n_mfcc <= 64 and 1 <= hop_length <= 400 required (got 128, 65, 200)"),
    "hop_0": (dict(hop_length=0), "default", 32000, "pa_mfcc_features: 32000 samples leave no MFCC frame"),
    "hop_401": (dict(hop_length=401), "default", 32000, "pa_mfcc_features: 32000 samples leave no MFCC frame"),
    "N_200_centred": ({}, "default", 200, "pa_mfcc_features: 200 samples leave no MFCC frame"),
    "N_399_uncentred": ({}, "m64_c64_hop160_uncentred", 399, "pa_mfcc_features: 399 samples leave no MFCC frame"),
}


@pytest.mark.parametrize("case", list(REFUSALS) + ["workspace_one_byte_short"])
def test_pa_mfcc_features_refusals(gpu_device, case):
    """what pa_mfcc_features refuses, it refuses with code 3, a message and no write (tests/refusals.py); all buffers are
    full size for the altered geometry, so that a call wrongly accepted would compute in bounds"""
    import pyannote_audio_amd.ffi as ffi
    from refusals import altered, check_refusal
    lib = ffi.load()
    B = 2
    if case == "workspace_one_byte_short":
        config, N = "default", 32000
        w = _struct(gpu_device, config)
        T = mt.num_frames(config, N)
        wav = GuardedInput(torch.from_numpy(mt.signal("white", B * N)), gpu_device)
        ws = _workspace(w, B, T, gpu_device)
        # the entry point has no size query of its own: an empty workspace is refused with the size it wants
        assert lib.pa_mfcc_features(w, wav.ptr, B * N, N, B, N, None, ffi.ptr(ws), 0, ffi.stream()) == 3
        m = re.fullmatch(r"pa_mfcc_features: workspace too small \(0 < (\d+) bytes\)", lib.pa_last_error().decode())
        assert m, lib.pa_last_error().decode()
        need = int(m.group(1))
        assert 4 * (B * T * w.n_mels + B) <= need <= ws.numel()
        check_refusal(lambda out: lib.pa_mfcc_features(w, wav.ptr, B * N, N, B, N, out, ffi.ptr(ws), need - 1,
                                                       ffi.stream()),
                      [((B, T, w.n_mfcc), torch.float32)],
                      f"pa_mfcc_features: workspace too small ({need - 1} < {need} bytes)", gpu_device)
        out = Guarded(B * T * w.n_mfcc, gpu_device)                 # and exactly that many bytes are enough
        ffi.check(lib.pa_mfcc_features(w, wav.ptr, B * N, N, B, N, out.ptr, ffi.ptr(ws), need, ffi.stream()), case)
        out.check(None, case)
        return
    fields, config, N, message = REFUSALS[case]
    w = altered(_struct(gpu_device, config), **fields)
    T = 1 + N // 200                                               # at least the frames of any accepted neighbour
    wav = GuardedInput(torch.from_numpy(mt.signal("white", B * max(N, 400))), gpu_device)
    ws = torch.empty(4 * (B * T * 257 + B + 128), dtype=torch.uint8, device=gpu_device)
    check_refusal(lambda out: lib.pa_mfcc_features(w, wav.ptr, B * N, N, B, N, out, ffi.ptr(ws), ws.numel(),
                                                   ffi.stream()),
                  [((B, T, 65), torch.float32)], message, gpu_device)


def test_mfcc_rows_form_through_the_forward(gpu_device):
    """k_mfcc_dct<true> writes the TDNN input rows [(tile, t, b16)][64]: 17 chunks (one behind the tile boundary, 15
    padding chunks in the second tile) with n_mfcc = 24 (columns 24 .. 63 zeros) -- a non-zero among them, or a wrong
    row, moves the embedding.  A -30 dBFS tone, another pitch in every chunk: at least a quarter of the cells on the top_db floor.  Against the float64
    oracle under the rules of tests/kernel_parity.py."""
    oracle, model = _model(gpu_device, {"n_mfcc": 24})
    B, N, S = 17, 32000, 2
    g = torch.Generator().manual_seed(4200 + SEED_OFFSET)
    t = torch.arange(N, dtype=torch.float64) / mt.SR
    wav = torch.stack([(10 ** (-30 / 20) * torch.sin(2 * np.pi * (440.0 + 20 * b) * t + 0.3 * b)).float()
                       for b in range(B)])[:, None]
    assert all(mt.truth("default", wav[b, 0].numpy())["on_floor"].mean() >= 0.25 for b in (0, B - 1))
    Tp = model.num_frames(N)
    weights = (torch.rand(B, S, Tp, generator=g) < 0.6).float()
    exact = xo.as_float64(oracle)
    with torch.inference_mode():
        want64 = torch.stack([exact(wav.double(), weights=weights[:, s].double()) for s in range(S)], dim=1)
        want32 = torch.stack([oracle(wav, weights=weights[:, s]) for s in range(S)], dim=1)
        unweighted64, unweighted32 = exact(wav.double()), oracle(wav)
    got = model(wav.to(gpu_device), weights.to(gpu_device))
    assert got.shape == (B, S, 512)
    assert_parity("mfcc_rows_form_B17_n_mfcc24", got, want64, want32)
    assert_parity("mfcc_rows_form_B17_n_mfcc24_unweighted", model(wav.to(gpu_device)), unweighted64, unweighted32)
