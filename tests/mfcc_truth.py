"""Float64 truth, per-cell tolerance, configurations and signals of the MFCC front end (csrc/mfcc.hip: k_mfcc_mel,
k_mfcc_dct through `pa_mfcc_features`), shared by tests/test_mfcc_truth_cpu.py (the truth against the float64 oracle, the
admissibility of every pair in use, what each signal claims to be) and tests/test_mfcc_kernel_gpu.py (the kernels through
the C ABI).  Modelled on tests/fbank_truth.py.

Truth, in float64 from the float32 samples of ONE chunk (cut as the reference cuts it: samples past `wav_len` are zero
BEFORE the reflection): reflect padding of 200 when centred, frames of 400 every `hop`, periodic Hann window in float64,
P = |rfft_400|^2 (T, 201), E64 = P fb with the FLOAT32 mel table the pack uploads (weights.mfcc_tables) widened,
dB = 10 log10(max(E64, 1e-10)), v = max(dB, max over the chunk - 80) -- or v = log(E64 + 1e-6) with log_mels -- and
c = v D with the FLOAT32 DCT table the pack uploads, widened.

Tolerance.  Per mel cell, in the energy domain, the model of tests/fbank_truth.py with the same KAPPA = 1 (a float32 FFT
leaves in every bin an error whose square is about eps32^2 x the energy of the whole frame; a band collects
sum_k fb[k, m] of that), and no floor relative to a peak:

  n[t, m]  = (KAPPA eps32)^2 sum_k P[t, k] sum_k fb[k, m]
  tol_E    = 1e-4 E64 + 2 sqrt(E64 n) + n

carried to the dB domain as the largest move of the value under E64 +- tol_E,
  move     = max |dB(max(E64 +- tol_E, 1e-10)) - dB|            (log_mels: of log(max(E64 +- tol_E, 0) + 1e-6)),
plus what float32 must add to ANY value it stores: log10f is specified to 2 ulp (the HIP math API's table; torch's is
tighter), the product with 10 rounds once more, 2.5 ulp <= 3 eps32 |dB| in all (ulp(x) <= eps32 |x|), and the float32
argument of the logarithm (the constant 1e-10f included) is off by up to eps32 / 2 relative, 10 / ln 10 x that < 4.343
eps32 in dB:
  tol_dB   = move + 3 eps32 |dB| + 4.343 eps32                  (log_mels: logf 1 ulp + the rounding of E + 1e-6:
                                                                  move + 2 eps32 |v| + eps32)
An all-zero filter and a silent frame have E64 = 0 and n = 0: move = 0, and the cell is held to the float32 rounding of
-100 dB alone.

The top_db clamp is max(dB, floor) with floor = (largest dB of the chunk) - 80.  max is 1-Lipschitz in both arguments,
and so is the maximum over the chunk, so the floor carries the tolerance of the chunk's loudest cell, tol_floor:
  a cell surely above the floor (dB - tol_dB > floor + tol_floor)  keeps tol_dB,
  a cell surely below it        (dB + tol_dB < floor - tol_floor)  gets tol_floor,
  a cell within tolerance of it                                    gets max(tol_dB, tol_floor).

Coefficients: c[k] = sum_m v[m] D[m, k] in float32.  The products enter through fma or are rounded once each; a sum of
n terms in ANY order (sequential in the kernel, blocked in torch) is off by at most gamma_n sum |terms| with
gamma_n = n u / (1 - n u), u = eps32 / 2 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), below
1.001 n u for n <= 256 -- the constant below is that bound, not a fit:
  rnd[k]   = 1.001 (n_mels / 2) eps32 sum_m |D[m, k]| |v[m]|
  tol_c[k] = sum_m |D[m, k]| tol_v[m] + rnd[k]

Where n_mfcc == n_mels the DCT matrix is square and invertible (orthonormal with norm = "ortho", up to the float32
rounding of the table: tests/test_mfcc_truth_cpu.py holds D D^T = I to it), and a single wrong band cannot hide behind
the sum over bands: the coefficients are carried back, v' = c' D^-1 in float64 with the inverse of the widened table,
and every cell is judged on its own
  tol_cell[m] = tol_v[m] + sum_k |D^-1[k, m]| rnd[k].
`ratio` is the larger of the two figures where both exist.

Admissibility: the float32 oracle (xvector_mfcc_oracle.MFCC in float32) decides it on the CPU, before any kernel output
exists: a (configuration, signal) pair is in PAIRS only if the oracle is within 0.5 of the tolerance on every chunk.
With the rounding terms above written out, every pair is: the oracle is at 0.37 at the most (`impulses` at hop 1), so
EXCLUDED is empty and no signal had to be changed; tests/test_mfcc_truth_cpu.py holds each pair to the rule.

Signals.  The generators of tests/fbank_truth.py where they fit; `tone_bin` is bin-centred for THIS transform (bin 40 of
400 = 1600 Hz); `tone_440_m30dB` is the -30 dBFS tone that puts most cells on the top_db floor; `zeros_then_loud` has a
first chunk of exact zeros beside loud ones; `loud_in_reflection` has a burst in samples 1 .. 199 of the first chunk,
so that the reflected padding of frame 0 holds it a second time and the chunk's loudest cell -- the one that sets the
floor -- is in frame 0."""
import functools

import numpy as np
import torch

import fbank_truth as ft
import xvector_mfcc_oracle as xo

EPS32 = ft.EPS32
KAPPA = 1.0
NFFT, NBIN, PAD = 400, 201, 200
SR = 16000

#: name -> the `mfcc` hyper-parameters of XVectorMFCC (None = the defaults: 128 bands, 40 coefficients, hop 200, centred)
CONFIGS = {
    "default": None,
    "m40_c40": {"n_mfcc": 40, "melkwargs": {"n_mels": 40}},
    "m64_c64_hop160_uncentred": {"n_mfcc": 64, "melkwargs": {"n_mels": 64, "hop_length": 160, "center": False}},
    "m23_c13": {"n_mfcc": 13, "melkwargs": {"n_mels": 23}},
    "m256_c64": {"n_mfcc": 64, "melkwargs": {"n_mels": 256}},
    "m65": {"melkwargs": {"n_mels": 65}},
    "slaney": {"melkwargs": {"mel_scale": "slaney", "norm": "slaney"}},
    "band_300_3400": {"melkwargs": {"f_min": 300.0, "f_max": 3400.0}},
    "dct_none": {"norm": None},
    "log_mels": {"log_mels": True},
    "hop1": {"melkwargs": {"hop_length": 1}},
    "hop399": {"melkwargs": {"hop_length": 399}},
    "hop400": {"melkwargs": {"hop_length": 400}},
}
#: the configurations whose DCT is square: every mel cell judged on its own
SQUARE = ("m40_c40", "m64_c64_hop160_uncentred")
#: chunk geometry (N, stride, chunks, samples cut off the end): 3 chunks of 2 s every second, `wav_len` ending 5000
#: samples inside the last one; hop 1, 399 and 400 on short chunks only
LAYOUT = {"hop1": (1000, 500, 3, 300), "hop399": (2000, 1000, 3, 600), "hop400": (2000, 1000, 3, 600)}
DEFAULT_LAYOUT = (32000, 16000, 3, 5000)


def layout(config: str):
    return LAYOUT.get(config, DEFAULT_LAYOUT)


def hparams(config: str) -> dict:
    """what XVectorMFCC saves as its hyper-parameters"""
    return {"sample_rate": SR, "num_channels": 1, "mfcc": dict(xo.MFCC_DEFAULTS, **(CONFIGS[config] or {})),
            "dimension": 512}


def _oracle_mfcc(config: str, dtype):
    return xo.MFCC(sample_rate=SR, **dict(xo.MFCC_DEFAULTS, **(CONFIGS[config] or {})), dtype=dtype).eval()


@functools.lru_cache(maxsize=None)
def tables(config: str):
    """-> dict: cfg (weights.mfcc_config), fb (201, n_mels) and D (n_mels, n_mfcc) float64 = the pack's float32 tables
    widened, Dinv (n_mfcc, n_mels) where D is square"""
    from pyannote_audio_amd.weights import mfcc_config, mfcc_tables
    sd = {"mfcc." + k: v for k, v in _oracle_mfcc(config, torch.float32).state_dict().items()}
    _, fb, dct = mfcc_tables(sd, hparams(config))
    assert fb.dtype == torch.float32 and dct.dtype == torch.float32
    cfg = mfcc_config(hparams(config))
    D = dct.numpy().astype(np.float64)
    return dict(cfg=cfg, fb=fb.numpy().astype(np.float64), D=D,
                Dinv=np.linalg.inv(D) if D.shape[0] == D.shape[1] else None)


def num_frames(config: str, n: int) -> int:
    cfg = tables(config)["cfg"]
    hop = cfg["hop_length"]
    if cfg["center"]:
        return 1 + n // hop if n > PAD else 0
    return 1 + (n - NFFT) // hop if n >= NFFT else 0


def _db(e):
    return 10.0 * np.log10(np.maximum(e, 1e-10))


def truth(config: str, x):
    """one chunk of float32 samples (n,) -> dict of float64 arrays: P (T, 201), E (T, n_mels), v and tol_v (T, n_mels),
    c and tol_c (T, n_mfcc), rnd (T, n_mfcc), tol_cell (T, n_mels) or None, on_floor (T, n_mels) bool"""
    tb = tables(config)
    cfg, fb, D = tb["cfg"], tb["fb"], tb["D"]
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    if cfg["center"]:
        assert x.size > PAD
        x = np.pad(x, PAD, mode="reflect")
    assert x.size >= NFFT
    frames = np.lib.stride_tricks.sliding_window_view(x, NFFT)[::cfg["hop_length"]]
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT, dtype=np.float64) / NFFT)
    P = np.abs(np.fft.rfft(frames * window, NFFT, axis=1)) ** 2
    E = P @ fb
    n = (KAPPA * EPS32) ** 2 * P.sum(axis=1)[:, None] * fb.sum(axis=0)[None, :]
    tol_E = 1e-4 * E + 2.0 * np.sqrt(E * n) + n
    if cfg["log_mels"]:
        v = np.log(E + 1e-6)
        move = np.maximum(np.abs(np.log(E + tol_E + 1e-6) - v), np.abs(np.log(np.maximum(E - tol_E, 0.0) + 1e-6) - v))
        tol_v = move + 2.0 * EPS32 * np.abs(v) + EPS32
        on_floor = np.zeros(E.shape, dtype=bool)
    else:
        dB = _db(E)
        move = np.maximum(np.abs(_db(E + tol_E) - dB), np.abs(_db(E - tol_E) - dB))
        tol_dB = move + 3.0 * EPS32 * np.abs(dB) + 4.343 * EPS32
        loudest = np.unravel_index(np.argmax(dB), dB.shape)
        floor, tol_floor = dB[loudest] - 80.0, tol_dB[loudest]
        v = np.maximum(dB, floor)
        above = dB - tol_dB > floor + tol_floor
        below = dB + tol_dB < floor - tol_floor
        tol_v = np.where(above, tol_dB, np.where(below, tol_floor, np.maximum(tol_dB, tol_floor)))
        on_floor = dB <= floor
    absD = np.abs(D)
    rnd = 1.001 * (D.shape[0] / 2.0) * EPS32 * (np.abs(v) @ absD)
    out = dict(P=P, E=E, v=v, tol_v=tol_v, c=v @ D, rnd=rnd, tol_c=tol_v @ absD + rnd, tol_cell=None, on_floor=on_floor)
    if tb["Dinv"] is not None:
        out["tol_cell"] = tol_v + rnd @ np.abs(tb["Dinv"])
    return out


def ratios(config: str, got, tr):
    """coefficients `got` (T, n_mfcc) against one chunk's truth -> (worst coefficient, worst mel cell or 0.0), each in
    units of its own tolerance (inf where `got` is not finite)"""
    g = torch.as_tensor(got).detach().cpu().double().numpy()
    assert g.shape == tr["c"].shape, (g.shape, tr["c"].shape)
    if not np.isfinite(g).all():
        return float("inf"), float("inf")
    rc = float((np.abs(g - tr["c"]) / tr["tol_c"]).max(initial=0.0))
    rm = 0.0
    if tr["tol_cell"] is not None:
        rm = float((np.abs(g @ tables(config)["Dinv"] - tr["v"]) / tr["tol_cell"]).max(initial=0.0))
    return rc, rm


def ratio(config: str, got, tr) -> float:
    return max(ratios(config, got, tr))


def oracle(config: str, x, dtype=torch.float32):
    """the oracle's MFCC of one chunk (T, n_mfcc) in `dtype`; in float64 with the pack's float32 tables widened, so that
    it computes what `truth` computes"""
    m = _oracle_mfcc(config, dtype)
    if dtype == torch.float64:
        tb = tables(config)
        m.dct_mat.copy_(torch.from_numpy(tb["D"]))
        m.MelSpectrogram.mel_scale.fb.copy_(torch.from_numpy(tb["fb"]))
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype)
    with torch.inference_mode():
        return m(x.view(1, 1, -1))[0, 0].transpose(0, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# signals: name -> function of (n, seed) -> float64 numpy (n,), |x| <= 1
# ---------------------------------------------------------------------------------------------------------------------
def _zeros_then_loud(n, seed):
    x = np.zeros(n)
    half = n // 2
    x[half:] = np.clip(0.3 * ft._randn(n - half, seed), -1.0, 1.0)
    return x


def _loud_in_reflection(n, seed):
    x = 1e-3 * ft._randn(n, seed)
    x[1:200] = 0.9 * np.sin(2.0 * np.pi * 1000.0 * ft._t(199) + ft._phase(seed))
    return np.clip(x, -1.0, 1.0)


SIGNALS = {
    "white": ft.SIGNALS["white"],
    "speech": ft.SIGNALS["speech"],
    "harmonic_envelope": ft.SIGNALS["harmonic_envelope"],
    "tone_bin": lambda n, seed: 0.5 * np.sin(2.0 * np.pi * (40.0 * SR / NFFT) * ft._t(n) + ft._phase(seed)),
    "tone_440_m30dB": ft.SIGNALS["tone_440_m30dB"],
    "silence_burst": ft.SIGNALS["silence_burst"],
    "impulses": ft.SIGNALS["impulses"],
    "clipped_noise": ft.SIGNALS["clipped_noise"],
    "dc03_noise01": ft.SIGNALS["dc03_noise01"],
    "zeros_then_loud": _zeros_then_loud,
    "loud_in_reflection": _loud_in_reflection,
}


def signal(name: str, n: int, seed: int = 0):
    x = np.asarray(SIGNALS[name](n, 7000 + 1000 * list(SIGNALS).index(name) + seed), dtype=np.float64)
    assert x.shape == (n,) and np.abs(x).max(initial=0.0) <= 1.0
    return x.astype(np.float32)


def evaluate(config: str, x):
    """one chunk -> its truth with the float32 oracle's ratio added"""
    tr = truth(config, x)
    tr["r_oracle"] = ratio(config, oracle(config, x), tr)
    return tr


@functools.lru_cache(maxsize=None)
def layout_case(config: str, name: str):
    """one signal in the configuration's chunk geometry, computed once: data (total,), wav_len, N, stride, B and per chunk
    the `evaluate` of what the kernel must read"""
    N, stride, B, cut = layout(config)
    total = (B - 1) * stride + N
    data = signal(name, total)
    wav_len = total - cut
    return dict(data=data, wav_len=wav_len, N=N, stride=stride, B=B,
                chunks=[evaluate(config, ft.chunk_of(data, b, N, stride, wav_len)) for b in range(B)])


@functools.lru_cache(maxsize=None)
def edge_case(config: str, name: str, n: int, B: int = 2):
    """B chunks of n samples, back to back, of one signal"""
    data = signal(name, B * n, seed=n)
    return dict(data=data, chunks=[evaluate(config, data[b * n:(b + 1) * n]) for b in range(B)])


#: (configuration, signal) pairs the float32 oracle itself does not hold to half the tolerance: none
EXCLUDED = {}
#: configuration -> the signals in use: every signal but the excluded ones
PAIRS = {config: [s for s in SIGNALS if (config, s) not in EXCLUDED] for config in CONFIGS}

#: framing edges (tests/test_mfcc_kernel_gpu.py): configuration -> chunk lengths
EDGE_LENGTHS = {
    "default": [201, 202, 399, 400, 401, 3199, 3201],                       # hop 200: hop + 1, 2 hop - 1 .. 16 hop +- 1
    "hop399": [201, 202, 398, 399, 400, 401, 16 * 399 - 1, 16 * 399 + 1],   # hop - 1, hop, hop + 1
    "m64_c64_hop160_uncentred": [400, 401, 559, 560],
}
EDGE_SIGNALS = ("white", "silence_burst")
