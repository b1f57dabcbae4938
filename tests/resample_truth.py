"""Float64 truth, cases and exact models of the polyphase resampler (csrc/resample.hip: `pa_resample_poly`), shared by
tests/test_resample_truth_cpu.py (the truth against a double loop, the banks, the admissibility of every GPU case) and
tests/test_resample_kernel_gpu.py (the kernel through the C ABI, `resample_on_device`, the `Audio` front door).

  out[q P + p] = sum_k taps[p][k] x[q L - width + k],   0 <= k < K = 2 width + L,   x zero outside [0, n)

The taps are ALWAYS the float32 bank of `sinc_resample_bank`, promoted: a bank evaluated in float64 differs from it by up
to 5e-5 (tests/test_resample_cpu.py), four orders above what is measured here.  The tolerance is no measurement: any order
of float32 multiply-adds over K terms, fused or not, satisfies per output

  |got - truth| <= gamma_K mag + K 2^-126,   gamma_K = K u / (1 - K u),   u = 2^-24,   mag = sum_k |taps[p][k]| |x[..]|

(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; the second term covers products that underflow,
flushed or not)."""
import functools
import math

import numpy as np
import torch

from kernel_parity import SEED_OFFSET

#: (orig, new): both tap paths, both directions, the largest bank of a common rate, and two contrived rates whose banks
#: lie on either side of the 48 KiB switch between taps in LDS and taps in global memory
PAIRS = [(8000, 16000), (16000, 8000), (48000, 16000), (96000, 16000), (12000, 16000), (44100, 16000), (16000, 44100),
         (11025, 16000), (10000, 10100), (10400, 10500)]
#: what `Audio(sample_rate=r)` makes of the 22 050 Hz waveform of the front-door tests
FRONT_DOOR_RATE = 22050
FRONT_DOOR_PAIRS = [(FRONT_DOOR_RATE, r) for r in (8000, 16000, 44100)]
LDS_LIMIT = 48 * 1024

U = 2.0 ** -24
TINY = 2.0 ** -126


@functools.lru_cache(maxsize=None)
def bank(orig: int, new: int):
    """-> (taps float32 numpy (P, K), L, P, width) of the product's own bank"""
    from pyannote_audio_amd.audio import sinc_resample_bank
    taps, L, P, width = sinc_resample_bank(orig, new)
    assert taps.dtype == torch.float32 and tuple(taps.shape) == (P, 2 * width + L)
    return taps.numpy().copy(), L, P, width


def num_out(n: int, L: int, P: int) -> int:
    return -((-P * n) // L)


def resample_truth(x, taps, L: int, P: int, width: int):
    """-> (out64, mag64), both (ceil(P n / L),): one matrix product of the sliding windows of the zero-extended signal
    (stride L) with the bank, and the same with |taps| and |x|"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    taps = np.asarray(taps, dtype=np.float64)
    n, K = x.size, taps.shape[1]
    assert taps.shape == (P, K) and K == 2 * width + L
    n_out = num_out(n, L, P)
    Q = -(-n_out // P)
    if Q == 0:
        return np.zeros(0), np.zeros(0)
    xp = np.zeros(max(width + n, (Q - 1) * L + K))
    xp[width:width + n] = x
    windows = np.lib.stride_tricks.sliding_window_view(xp, K)[::L][:Q]          # (Q, K): row q = x[q L - width + k]
    out = windows @ taps.T
    mag = np.abs(windows) @ np.abs(taps).T
    return out.reshape(-1)[:n_out].copy(), mag.reshape(-1)[:n_out].copy()


def bound(mag, K: int):
    """the float32 summation bound per output (module docstring)"""
    return (K * U / (1.0 - K * U)) * np.asarray(mag, dtype=np.float64) + K * TINY


def err_over_bound(got, truth, mag, K: int) -> float:
    """max |got - truth| / bound (NaN or inf in `got` -> inf); 0 for no elements"""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return 0.0
    r = np.abs(got - truth) / bound(mag, K)
    return float("inf") if not np.isfinite(r).all() else float(r.max())


def lengths(orig: int, new: int) -> list:
    """input lengths of one pair: around 1, width and L, a partial last block, a few blocks, and -- for the two pairs
    that can -- the lengths whose outputs end at 255, 256 and 257 (a thread block is 256 outputs)"""
    _, L, P, width = bank(orig, new)
    ns = {1, 2, width - 1, width, width + 1, L - 1, L, L + 1, 2 * L + width + 3, 4 * L + 17, 1000}
    if (orig, new) == (48000, 16000):
        ns |= {763, 766, 769}              # ceil(n / 3) = 255, 256, 257, none of them a whole block
    if (orig, new) == (8000, 16000):
        ns |= {128}                        # 2 n = 256; 255 and 257 are cut from 128 and 129 samples: EDGE_OUTPUTS
    return sorted(n for n in ns if n >= 1)


#: (orig, new) -> [(n, n_out)] with n_out BELOW ceil(P n / L): the kernel takes n_out as an argument, and 8 kHz -> 16 kHz
#: has no length of its own with an odd number of outputs
EDGE_OUTPUTS = {(8000, 16000): [(128, 255), (129, 257), (1, 1)]}


def signals(orig: int, new: int, n: int) -> dict:
    """name -> float32 numpy (n,): noise, DC, and a tone at 0.45 of the lower Nyquist rate riding on 0.5"""
    seed = 7000 + SEED_OFFSET + 131 * PAIRS_AND_FRONT.index((orig, new)) + n
    noise = 0.3 * torch.randn(n, generator=torch.Generator().manual_seed(seed))
    f = 0.45 * min(orig, new) / 2.0
    tone = 0.5 * np.sin(2.0 * np.pi * f * np.arange(n, dtype=np.float64) / orig) + 0.5
    return {"noise": noise.numpy().astype(np.float32), "dc": np.full(n, 0.75, dtype=np.float32),
            "tone": tone.astype(np.float32)}


PAIRS_AND_FRONT = PAIRS + FRONT_DOOR_PAIRS


def oracle32(x, orig: int, new: int):
    """the float32 oracle (oracle/audio.py: strided conv1d of torch) on a float32 numpy signal -> float32 numpy"""
    from oracle.audio import resample
    return resample(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))[None], orig, new)[0].numpy()


@functools.lru_cache(maxsize=None)
def dense_cases(orig: int, new: int) -> tuple:
    """every dense case of one pair, computed once: dicts of name, x (float32), truth, mag (float64) and oracle (float32)"""
    taps, L, P, width = bank(orig, new)
    cases = []
    for n in lengths(orig, new):
        for name, x in signals(orig, new, n).items():
            truth, mag = resample_truth(x, taps, L, P, width)
            cases.append(dict(name=f"{name}_n{n}", n=n, x=x, truth=truth, mag=mag, oracle=oracle32(x, orig, new)))
    return tuple(cases)


# ---------------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------------
HEIGHT_EXPONENTS = (0, -3, 5)


def impulse_signals(n: int, K: int) -> list:
    """-> [(positions, heights)]: impulses of height 2^e at 0, at n - 1 and every K + 3 samples in between, any two of one
    signal at least K apart, so that no window of K samples holds two of them and every output is ONE exact product.
    Where the ends are closer than K (n - 1 < K) they go into two signals."""
    inner = [j for j in range(K + 3, n - 1, K + 3) if j + K <= n - 1]
    if n == 1:
        groups = [[0]]
    elif n - 1 < K:
        groups = [[0], [n - 1]]
    else:
        groups = [[0] + inner + [n - 1]]
    out, i = [], 0
    for g in groups:
        heights = []
        for _ in g:
            heights.append(2.0 ** HEIGHT_EXPONENTS[i % len(HEIGHT_EXPONENTS)])
            i += 1
        out.append((g, heights))
    return out


def end_tap_signals(L: int, width: int) -> list:
    """-> [(n, positions, heights)]: one impulse each, placed so that it meets tap K - 1 of block 1 and tap 0 of a later
    block (the first and the last trip of the kernel's k loop: taps at the clamp, which no dense signal can see), with
    width + L samples behind it so that every block in reach is written"""
    last = 2 * L + width - 1                       # k = j - q L + width = K - 1 for q = 1
    first = (width // L + 2) * L - width           # k = 0 for q = width // L + 2
    return [(j + width + L, [j], [2.0 ** e]) for j, e in ((last, -3), (first, 5))]


def impulse_input(n: int, positions, heights):
    x = np.zeros(n, dtype=np.float32)
    x[list(positions)] = np.asarray(heights, dtype=np.float32)
    return x


def impulse_expected(n: int, positions, heights, taps, L: int, P: int, width: int):
    """float32 (n_out,): taps[p][j - q L + width] * 2^e where impulse j is in reach of block q, else 0.  The product of a
    float32 tap with a power of two is exact (the CPU test checks that none underflows), so this is what ANY correct
    evaluation returns, whatever its order"""
    K = taps.shape[1]
    n_out = num_out(n, L, P)
    Q = -(-n_out // P)
    want = np.zeros((Q, P), dtype=np.float32)
    hits = np.zeros(Q, dtype=np.int64)
    for j, h in zip(positions, heights):
        for q in range(Q):
            k = j - q * L + width
            if 0 <= k < K:
                want[q] = taps[:, k] * np.float32(h)
                hits[q] += 1
    assert hits.max(initial=0) <= 1, "two impulses within one window: the case is not exact"
    return want.reshape(-1)[:n_out].copy()


def shift_lengths(orig: int, new: int) -> list:
    _, L, _, width = bank(orig, new)
    return [2 * L + width + 3, 1000]


def shift_input(orig: int, new: int, n: int):
    """-> (x, x') with x' = L zeros in front of x"""
    _, L, _, _ = bank(orig, new)
    x = signals(orig, new, n)["noise"]
    return x, np.concatenate([np.zeros(L, dtype=np.float32), x])


# ---------------------------------------------------------------------------------------------------------------------
# the front door
# ---------------------------------------------------------------------------------------------------------------------
FRONT_DOOR_SAMPLES = 6615            # 0.3 s at 22 050 Hz: odd, so the second row of the waveform is not 16-byte aligned
FRONT_DOOR_SEGMENT = (-0.04, 0.36)   # 882 samples in front of the waveform, 7938 - 6615 = 1323 behind it
FRONT_DOOR_LEAD, FRONT_DOOR_TRAIL = 882, 1323


def front_door_waveform():
    """(2, 6615) float32 torch: noise in one channel, the tone on its pedestal in the other"""
    s = signals(FRONT_DOOR_RATE, 16000, FRONT_DOOR_SAMPLES)
    return torch.from_numpy(np.stack([s["noise"], s["tone"]]))


def front_door_padded(w):
    return torch.nn.functional.pad(w, (FRONT_DOOR_LEAD, FRONT_DOOR_TRAIL))


def double_loop(x, taps, L: int, P: int, width: int):
    """the definition, term by term (for the small cases of the CPU test only)"""
    x = [float(v) for v in x]
    n, K = len(x), taps.shape[1]
    n_out = num_out(n, L, P)
    out, mag = np.zeros(n_out), np.zeros(n_out)
    for o in range(n_out):
        q, p = divmod(o, P)
        acc = mg = 0.0
        for k in range(K):
            i = q * L - width + k
            if 0 <= i < n:
                acc += float(taps[p, k]) * x[i]
                mg += abs(float(taps[p, k])) * abs(x[i])
        out[o], mag[o] = acc, mg
    return out, mag
