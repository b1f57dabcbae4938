"""Float64 truth, tolerance, float32 step model and signals of the log-mel filterbank (csrc/emb_fbank.hip: `pa_fbank`,
`pa_fbank_ragged`), shared by tests/test_fbank_truth_cpu.py (the truth against the oracle, the admissibility of every
signal, the centring order) and tests/test_fbank_kernel_gpu.py (the kernels through the C ABI).

Truth, in float64 from the float32 samples: x 2^15, frames of 400 every 160 (snip_edges), per-frame mean removal,
pre-emphasis 0.97 with replicate padding, Hamming window, zero-pad to 512, P = |rfft|^2 (T, 257), E64 = P mel^T with the
FLOAT32 mel table of oracle.models.kaldi_mel_banks (plus the zero Nyquist column), and the FLOAT32 floor
Ef = max(E64, 2^-23).  The oracle's kaldi_fbank run in float64 floors at the float64 epsilon (-36 on silence where every
float32 implementation gives -15.94): it is the truth only where E64 >= 2^-23.

Tolerance, per element, in the energy domain.  A float32 FFT leaves in every bin an error whose square is about
eps32^2 x the energy of the whole frame, whatever the bin itself holds; a mel band collects sum_k mel[m, k] of that:

  n[t, m] = (KAPPA eps32)^2 sum_k P[t, k] sum_k mel[m, k]
  tol     = 1e-4 Ef + 2 sqrt(Ef n) + n          (|a + e|^2 - |a|^2 <= 2 |a| |e| + |e|^2)

and a result `got` (log features) is judged by max |exp(got) - Ef| / tol.  No floor relative to a peak: a quiet frame
beside a loud one, a quiet band beside a strong one and a silent frame are all held to their own energy.  KAPPA = 1 is no
fit to any implementation; tests/test_fbank_truth_cpu.py measures what the float32 oracle and the step model below make
of it and holds every signal to <= 0.5 (the admissibility rule: decided from the float32 oracle on the CPU, before any
kernel output exists).

Input rule (a frame whose samples are all EQUAL and non-zero is ill-posed in float32: float64 removes the mean exactly
and gives the floor, float32 leaves the rounding of sum / 400 as a residue, 6e5 x the tolerance at a DC of 0.3): a DC
offset over exactly constant stretches is used only at 0.25, where 400 x 8192 and every partial sum of it are exact in
float32 in any order, so that every implementation must give the floor exactly.  Any other DC offset rides on noise, and
on noise large enough that float32 mean removal does not leak into the lowest mel bins (0.5 under noise of 1e-3 does)."""
import functools
import os
import wave

import numpy as np
import torch

from kernel_parity import SEED_OFFSET

WIN, SHIFT, NFFT, NBIN, NMEL = 400, 160, 512, 257, 80
EPS32 = 1.1920928955078125e-07
KAPPA = 1.0
LOG_EPS32 = np.float32(np.log(np.float64(EPS32)))       # what a frame wholly at the floor holds
SAMPLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample.wav")

#: the uncentred cases: 3 chunks of N samples every STRIDE, cut from TOTAL samples of which the kernel is told TOTAL - CUT
TOTAL, N, STRIDE, CUT = 48000, 24000, 12000, 5000
#: the lengths of test_fuzz_fbank_lengths (tests/test_fuzz_gpu.py): every framing edge
EDGE_LENGTHS = [400, 401, 559, 560, 561, 719, 720, 1000, 4799, 4800, 16000, 23456, 48001]


def num_frames(n: int) -> int:
    return 0 if n < WIN else 1 + (n - WIN) // SHIFT


@functools.lru_cache(maxsize=None)
def mel_table():
    """float32 numpy (80, 257): the oracle's table and the zero Nyquist column"""
    from oracle.models import kaldi_mel_banks
    mel = kaldi_mel_banks(NMEL, NFFT, 16000.0)
    assert mel.dtype == torch.float32 and tuple(mel.shape) == (NMEL, NFFT // 2)
    return np.concatenate([mel.numpy(), np.zeros((NMEL, 1), dtype=np.float32)], axis=1)


def _frames(x, dtype):
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    assert x.size >= WIN
    scaled = x.astype(dtype) * dtype(32768.0)
    return np.lib.stride_tricks.sliding_window_view(scaled, WIN)[::SHIFT]


def truth(x):
    """float32 samples (n,) -> dict of float64 arrays: P (T, 257), E64, Ef, tol (T, 80) and floor (T,) bool, the frames
    wholly at the floor"""
    fr = _frames(x, np.float64)
    fr = fr - fr.mean(axis=1, keepdims=True)
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    window = 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(WIN, dtype=np.float64) / (WIN - 1))
    P = np.abs(np.fft.rfft((fr - 0.97 * prev) * window, NFFT, axis=1)) ** 2
    mel = mel_table().astype(np.float64)
    E64 = P @ mel.T
    Ef = np.maximum(E64, EPS32)
    n = (KAPPA * EPS32) ** 2 * P.sum(axis=1)[:, None] * mel.sum(axis=1)[None, :]
    tol = 1e-4 * Ef + 2.0 * np.sqrt(Ef * n) + n
    return dict(P=P, E64=E64, Ef=Ef, tol=tol, floor=(E64 <= EPS32).all(axis=1))


def energy_ratio(energies, want, tol):
    """-> (T,) max over the mel bins of |energies - want| / tol (inf where `energies` is not finite)"""
    e = np.asarray(energies, dtype=np.float64)
    r = np.abs(e - want) / tol
    r[~np.isfinite(e)] = np.inf
    return r.max(axis=1)


def ratio(got_log, want, tol) -> float:
    """the worst frame of log features `got_log` (T, 80) against the energies `want` (the truth's Ef, or the step
    model's)"""
    got = torch.as_tensor(got_log).detach().cpu().double().numpy()
    return float(energy_ratio(np.exp(got), want, tol).max(initial=0.0))


def oracle32(x):
    """the float32 oracle's log features (T, 80), float32 numpy"""
    from oracle.models import kaldi_fbank
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return kaldi_fbank((x * 32768.0).unsqueeze(0)).numpy()


# ---------------------------------------------------------------------------------------------------------------------
# float32 step model of k_fbank
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tables():
    from pyannote_audio_amd.weights import fbank_tables, kaldi_mel_banks
    window, tw256, tw512 = (t.numpy().astype(np.float32) for t in fbank_tables())
    mel = kaldi_mel_banks(NMEL, NFFT, 16000.0).numpy()
    nz = mel > 0
    lo = np.array([np.nonzero(r)[0][0] for r in nz])
    hi = np.array([np.nonzero(r)[0][-1] for r in nz])
    return window, tw256, tw512, mel, lo, hi


def _cmul(ax, ay, bx, by):
    return ax * bx - ay * by, ax * by + ay * bx


def step_model(x):
    """float32 samples (n,) -> float32 energies (T, 80), floored: k_fbank step by step in float32 numpy -- its tables
    (weights.fbank_tables), its lane sums and butterfly for the mean, the four radix-4 Stockham passes with its index
    arithmetic, its real unpack, its mel sum in ascending k.  Not bit-exact (numpy rounds every product where the
    compiler may fuse it into the sum): it says what float32 arithmetic of THIS algorithm costs"""
    window, tw256, tw512, mel, lo, hi = _tables()
    f32 = np.float32
    fr = np.ascontiguousarray(_frames(x, np.float32))
    T = fr.shape[0]
    lanes = np.concatenate([fr, np.zeros((T, 448 - WIN), dtype=f32)], axis=1).reshape(T, 7, 64)
    s = lanes[:, 0]
    for i in range(1, 7):
        s = s + lanes[:, i]
    h = 32
    while h:                                            # wave_sum: v += shfl_xor(v, h), as lane 0 sees it
        s = s[:, :h] + s[:, h:]
        h >>= 1
    xm = fr - s / f32(WIN)
    prev = np.concatenate([xm[:, :1], xm[:, :-1]], axis=1)
    y = np.zeros((T, NFFT), dtype=f32)
    y[:, :WIN] = (xm - f32(0.97) * prev) * window
    sx, sy = y[:, 0::2].copy(), y[:, 1::2].copy()       # 256 complex
    j = np.arange(64)
    for p in range(4):
        Ns, tstep = 1 << (2 * p), 64 >> (2 * p)
        k = j & (Ns - 1)
        v = []
        for r in range(4):
            w = tw256[(r * k * tstep) & 255]
            v.append(_cmul(sx[:, j + 64 * r], sy[:, j + 64 * r], w[:, 0], w[:, 1]))
        t0 = (v[0][0] + v[2][0], v[0][1] + v[2][1])
        t1 = (v[0][0] - v[2][0], v[0][1] - v[2][1])
        t2 = (v[1][0] + v[3][0], v[1][1] + v[3][1])
        d13 = (v[1][0] - v[3][0], v[1][1] - v[3][1])
        t3 = (d13[1], -d13[0])
        j0 = ((j - k) << 2) + k
        dx, dy = np.empty_like(sx), np.empty_like(sy)
        for q, (a, b, sign) in enumerate([(t0, t2, 1), (t1, t3, 1), (t0, t2, -1), (t1, t3, -1)]):
            dx[:, j0 + q * Ns] = a[0] + b[0] if sign > 0 else a[0] - b[0]
            dy[:, j0 + q * Ns] = a[1] + b[1] if sign > 0 else a[1] - b[1]
        sx, sy = dx, dy
    kk = np.arange(NBIN)
    zkx, zky = sx[:, kk & 255], sy[:, kk & 255]
    zcx, zcy = sx[:, (256 - kk) & 255], -sy[:, (256 - kk) & 255]
    ex, ey = f32(0.5) * (zkx + zcx), f32(0.5) * (zky + zcy)
    ddx, ddy = f32(0.5) * (zkx - zcx), f32(0.5) * (zky - zcy)
    wox, woy = _cmul(ddy, -ddx, tw512[:, 0], tw512[:, 1])
    re, im = ex + wox, ey + woy
    P = re * re + im * im
    acc = np.zeros((T, NMEL), dtype=f32)
    for u in range(int((hi - lo).max()) + 1):
        kq = np.minimum(lo + u, hi)
        acc = np.where((lo + u <= hi)[None, :], acc + P[:, kq] * mel[np.arange(NMEL), kq][None, :], acc)
    assert acc.dtype == f32
    return np.maximum(acc, f32(EPS32))


# ---------------------------------------------------------------------------------------------------------------------
# signals: name -> function of (n, seed) -> float32 numpy (n,)
# ---------------------------------------------------------------------------------------------------------------------
def _randn(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed + SEED_OFFSET)).double().numpy()


def _phase(seed):
    return float(torch.rand(1, generator=torch.Generator().manual_seed(seed + SEED_OFFSET))) * 2.0 * np.pi


def _t(n):
    return np.arange(n, dtype=np.float64) / 16000.0


def envelope(n, seed):
    """a slow (1 Hz) envelope that is EXACTLY zero for half of every second and EXACTLY one for a quarter of it"""
    return np.clip(1.5 * np.sin(2.0 * np.pi * 1.0 * _t(n) + _phase(seed)), 0.0, 1.0)


def _harmonics(n, seed):
    """120 Hz and its harmonics up to 8 kHz, -12 dB / octave (1 / h^2), peak below 0.5"""
    t, ph = _t(n), _phase(seed + 1)
    s = sum(np.sin(2.0 * np.pi * 120.0 * h * t + h * ph) / h ** 2 for h in range(1, 67))
    return 0.3 * s


@functools.lru_cache(maxsize=None)
def _speech():
    with wave.open(SAMPLE) as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000)
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float64) / 32768.0


def _sig_speech(n, seed):
    # from the last 8 s of the file, words and the pauses between them in every 1.5 s: the seed picks one of three starts
    s = _speech()
    start = (352000, 368000, 384000)[(seed + SEED_OFFSET) % 3]
    assert start + n <= s.size
    return s[start:start + n]


def _sig_burst(n, seed):
    x = np.zeros(n)
    start = n // 3
    m = min(10000, n - start)
    x[start:start + m] = 0.1 * _randn(m, seed)
    return x


def _sig_impulses(n, seed):
    x = np.zeros(n)
    x[(seed + SEED_OFFSET) % 401::4001] = 0.9
    return x


def _sig_clicks(n, seed):
    x = np.zeros(n)
    x[(seed + SEED_OFFSET) % 401::2999] = 1.0 / 32768.0
    return x


def _sig_dither(n, seed):
    g = torch.Generator().manual_seed(seed + SEED_OFFSET)
    return (torch.randint(-1, 2, (n,), generator=g).double() / 32768.0).numpy()


SIGNALS = {
    "white": lambda n, seed: np.clip(0.1 * _randn(n, seed), -1.0, 1.0),
    "speech": _sig_speech,
    "harmonic_envelope": lambda n, seed: _harmonics(n, seed) * envelope(n, seed),
    "tone_440_m30dB": lambda n, seed: 10.0 ** (-30.0 / 20.0) * np.sin(2.0 * np.pi * 440.0 * _t(n) + _phase(seed)),
    "tone_bin40": lambda n, seed: 0.5 * np.sin(2.0 * np.pi * (40.0 * 16000.0 / NFFT) * _t(n) + _phase(seed)),
    "dither_1lsb": _sig_dither,
    "silence_burst": _sig_burst,
    "impulses": _sig_impulses,
    "square_200": lambda n, seed: 0.99 * np.where((np.arange(n) + (seed + SEED_OFFSET) % 80) % 80 < 40, 1.0, -1.0),
    "clipped_noise": lambda n, seed: np.clip(2.0 * _randn(n, seed), -1.0, 1.0),
    "dc03_noise01": lambda n, seed: 0.3 + 0.1 * _randn(n, seed),
    "dc005_noise001": lambda n, seed: 0.05 + 0.01 * _randn(n, seed),
    "silence_clicks": _sig_clicks,
    # 0.25 wherever the envelope is not zero: stretches of exactly 0.25 and of 0 with a full step between them.  (0.25 x
    # the envelope itself would approach its plateau through frames of a tiny slope on a DC of 8192, which the rounding
    # of sum / 400 makes inadmissible at some phases: 2.2 x the tolerance for the float32 oracle.)
    "dc025_envelope": lambda n, seed: 0.25 * (envelope(n, seed) > 0.0),
}
#: what each signal claims to be (tests/test_fbank_truth_cpu.py asserts it from the truth)
HAS_FLOOR_FRAMES = {"harmonic_envelope", "silence_burst", "impulses", "silence_clicks", "dc025_envelope"}
HAS_100_DB = {"speech", "harmonic_envelope", "silence_burst"}


def signal(name: str, n: int, seed: int = 0):
    x = np.asarray(SIGNALS[name](n, 1000 * (1 + list(SIGNALS).index(name)) + seed), dtype=np.float64)
    assert x.shape == (n,) and np.abs(x).max() <= 1.0
    return x.astype(np.float32)


def chunk_of(data, b: int, n: int, stride: int, wav_len: int):
    """chunk b as the kernel must read it: samples [b stride, b stride + n) of `data`, zeros from `wav_len` on"""
    out = np.zeros(n, dtype=np.float32)
    lo, hi = b * stride, min(b * stride + n, wav_len)
    if hi > lo:
        out[:hi - lo] = data[lo:hi]
    return out


def evaluate(x):
    """one chunk -> its truth, with the float32 oracle's and the step model's ratios and the model's energies added"""
    tr = truth(x)
    tr["model"] = step_model(x)
    tr["r_oracle"] = ratio(oracle32(x), tr["Ef"], tr["tol"])
    tr["r_model"] = float(energy_ratio(tr["model"], tr["Ef"], tr["tol"]).max())
    return tr


@functools.lru_cache(maxsize=None)
def layout_case(name: str):
    """the uncentred case of one signal, computed once: data (TOTAL,), wav_len, and per chunk the `evaluate` of what the
    kernel must read (the last chunk ends CUT samples inside its buffer)"""
    data = signal(name, TOTAL)
    wav_len = TOTAL - CUT
    B = 1 + (TOTAL - N) // STRIDE
    return dict(data=data, wav_len=wav_len, B=B,
                chunks=[evaluate(chunk_of(data, b, N, STRIDE, wav_len)) for b in range(B)])


@functools.lru_cache(maxsize=None)
def edge_case(name: str, n: int):
    """two chunks of n samples, back to back, of one signal of 2 n samples"""
    data = signal(name, 2 * n, seed=n)
    return dict(data=data, chunks=[evaluate(data[b * n:(b + 1) * n]) for b in range(2)])


# ---------------------------------------------------------------------------------------------------------------------
# centring
# ---------------------------------------------------------------------------------------------------------------------
CENTER_FRAMES = [1, 2, 3, 4, 5, 7, 298, 6000, 60000]


def drifting_noise(T: int, seed: int = 0):
    """float32 samples of T frames: noise whose level drifts slowly (one cycle per 20 s) over 40 dB, 0.3 at the most"""
    n = WIN + SHIFT * (T - 1)
    level = 0.3 * 10.0 ** (-(1.0 + np.sin(2.0 * np.pi * _t(n) / 20.0 + _phase(50000 + T + seed))))
    g = torch.Generator().manual_seed(50000 + T + seed + SEED_OFFSET)
    return np.clip(level * torch.randn(n, generator=g).numpy(), -1.0, 1.0).astype(np.float32)


def kernel_order_mean(x, acc=np.float32):
    """(T, M) float32 -> (M,) float32: the mean in the order of k_fbank_center -- four partial sums over the frames
    p, p + 4, ..., each sequential, added in order, divided by T -- accumulated in `acc` (float32: the kernel as it was;
    float64: as it is) and rounded to float32 once at the end"""
    x = np.asarray(x, dtype=np.float32)
    T = x.shape[0]
    parts = []
    for p in range(4):
        s = np.zeros(x.shape[1], dtype=acc)
        for row in x[p::4]:
            s = s + row
        parts.append(s)
    return ((parts[0] + parts[1] + parts[2] + parts[3]) / acc(T)).astype(np.float32)
