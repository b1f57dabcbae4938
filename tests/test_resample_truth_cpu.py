"""Everything about tests/test_resample_kernel_gpu.py that needs no GPU (tests/resample_truth.py): the float64 truth
against the definition written as a double loop; the product's filter bank against the oracle's, bit for bit, and against
the float64 closed form on every pair of the grid; where the grid sits relative to the kernel's 48 KiB switch; that the
impulse cases are exact; and the ADMISSIBILITY of every GPU case: the float32 oracle (oracle/audio.py) must itself lie
within half the summation bound and within half the project contract (rtol 1e-4 / atol 1e-5) of the truth, the rule of
tests/kernel_parity.py -- a case that float32 cannot do is found here, not on the GPU."""
import math

import numpy as np
import pytest
import torch

import resample_truth as T
from kernel_parity import ratio

_pair_ids = dict(ids=lambda p: f"{p[0]}to{p[1]}")


@pytest.mark.parametrize("orig,new,n,seed", [(8000, 16000, 9, 1), (48000, 16000, 50, 2), (12000, 16000, 23, 3)])
def test_truth_equals_double_loop(orig, new, n, seed):
    """n < width with two phases, a decimator with a partial last block, a rational pair: sum and magnitude"""
    taps, L, P, width = T.bank(orig, new)
    x = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    out, mag = T.resample_truth(x, taps, L, P, width)
    want, want_mag = T.double_loop(x, taps, L, P, width)
    assert out.shape == want.shape == (math.ceil(P * n / L),)
    # two float64 evaluations of sums of K <= 20 terms: K 2^-53 of the magnitude, eight orders below the float32 bound
    assert np.all(np.abs(out - want) <= taps.shape[1] * 2.0 ** -52 * want_mag)
    assert np.all(np.abs(mag - want_mag) <= taps.shape[1] * 2.0 ** -52 * want_mag)


def test_truth_of_nothing():
    taps, L, P, width = T.bank(48000, 16000)
    out, mag = T.resample_truth(np.zeros(0), taps, L, P, width)
    assert out.shape == mag.shape == (0,)


@pytest.mark.parametrize("pair", T.PAIRS_AND_FRONT, **_pair_ids)
def test_bank_matches_oracle_and_closed_form(pair):
    """tests/test_resample_cpu.py::test_filter_bank_matches_closed_form, with its bounds, on the whole grid"""
    from oracle.audio import sinc_resample_kernel
    orig, new = pair
    g = math.gcd(orig, new)
    kern, width = sinc_resample_kernel(orig, new, g)
    taps, L, P, w2 = T.bank(orig, new)
    assert (L, P, w2) == (orig // g, new // g, width) and taps.shape == (P, 2 * width + L)
    assert np.array_equal(kern[:, 0].numpy().view(np.int32), taps.view(np.int32))     # bit for bit
    cutoff = min(L, P) * 0.99
    k = np.arange(-width, width + L, dtype=np.float64)[None, :] / L
    p = -np.arange(P, dtype=np.float64)[:, None] / P
    t = np.clip((p + k) * cutoff, -6, 6)
    want = np.sinc(t) * np.cos(t * np.pi / 12) ** 2 * (cutoff / L)
    assert np.abs(taps - want).max() < 5e-5
    assert np.abs(taps.astype(np.float64).sum(axis=1) - 1.0).max() < 5e-3


def test_grid_sits_where_the_kernel_switches():
    """(L, P, K) of the grid as the kernel sees them: which banks go to LDS, how many trips the 256-thread fill loop
    makes, and the two contrived rates on either side of the 48 KiB switch"""
    shapes = {pair: (T.bank(*pair)[1], T.bank(*pair)[2], T.bank(*pair)[0].shape[1]) for pair in T.PAIRS}
    assert shapes[(8000, 16000)][:2] == (1, 2) and shapes[(16000, 8000)][:2] == (2, 1)
    assert shapes[(48000, 16000)][:2] == (3, 1) and shapes[(12000, 16000)][:2] == (3, 4)
    assert shapes[(96000, 16000)] == (6, 1, 80)
    assert shapes[(44100, 16000)] == (441, 160, 475)
    assert shapes[(16000, 44100)][:2] == (160, 441)
    assert shapes[(11025, 16000)] == (441, 640, 455)
    assert shapes[(10000, 10100)] == (100, 101, 114) and shapes[(10400, 10500)] == (104, 105, 118)
    size = {pair: 4 * P * K for pair, (L, P, K) in shapes.items()}
    assert size[(10000, 10100)] == 46056 <= T.LDS_LIMIT < 49560 == size[(10400, 10500)]
    assert math.ceil(101 * 114 / 256) == 45
    in_lds = {pair for pair in T.PAIRS if size[pair] <= T.LDS_LIMIT}
    assert in_lds == {(8000, 16000), (16000, 8000), (48000, 16000), (96000, 16000), (12000, 16000), (10000, 10100)}
    for pair in T.PAIRS:
        ns = T.lengths(*pair)
        L, P, _ = shapes[pair]
        assert ns[0] == 1 and max(ns) <= 1800 and max(T.num_out(n, L, P) for n in ns) <= 2800
        # a partial last block wherever one can exist (L = 1 gets its own from EDGE_OUTPUTS)
        assert any(T.num_out(n, L, P) % P for n in ns) or P == 1 or (L == 1 and pair in T.EDGE_OUTPUTS)
    assert [math.ceil(n / 3) for n in (763, 766, 769)] == [255, 256, 257]
    assert all(n_out < T.num_out(n, 1, 2) or (n, n_out) == (1, 1) for n, n_out in T.EDGE_OUTPUTS[(8000, 16000)])


@pytest.mark.parametrize("pair", T.PAIRS_AND_FRONT, **_pair_ids)
def test_every_gpu_case_is_admissible(pair):
    """the float32 oracle on every dense case of the pair: within half the bound, within half the contract"""
    orig, new = pair
    taps, L, P, width = T.bank(orig, new)
    K = taps.shape[1]
    worst_bound = worst_contract = 0.0
    for case in T.dense_cases(orig, new):
        assert case["oracle"].shape == case["truth"].shape == (math.ceil(P * case["n"] / L),), case["name"]
        assert np.abs(case["x"]).max() <= 1.5, case["name"]             # waveform scale (0.3 randn: 5 sigma)
        worst_bound = max(worst_bound, T.err_over_bound(case["oracle"], case["truth"], case["mag"], K))
        worst_contract = max(worst_contract, ratio(case["oracle"], case["truth"]))
    print(f"resample {orig}->{new}: float32 oracle max|err|/bound = {worst_bound:.3f}, of the contract {worst_contract:.4f}")
    assert worst_bound <= 0.5, f"inadmissible: the float32 oracle is at {worst_bound:.3f} of the summation bound"
    assert worst_contract <= 0.5, f"inadmissible: the float32 oracle is at {worst_contract:.3f} of the contract"


@pytest.mark.parametrize("pair", T.PAIRS, **_pair_ids)
def test_shift_and_front_door_inputs_are_admissible(pair):
    """the shifted noise signals of the block-shift test (their first block is held to the bound)"""
    orig, new = pair
    taps, L, P, width = T.bank(orig, new)
    for n in T.shift_lengths(orig, new):
        x, shifted = T.shift_input(orig, new, n)
        assert shifted.size == n + L and not shifted[:L].any() and np.array_equal(shifted[L:], x)
        truth, mag = T.resample_truth(shifted, taps, L, P, width)
        base, _ = T.resample_truth(x, taps, L, P, width)
        assert truth.size == base.size + P and np.array_equal(truth[P:], base)      # the property itself, in float64
        assert T.err_over_bound(T.oracle32(shifted, orig, new), truth, mag, taps.shape[1]) <= 0.5


def test_front_door_padded_excerpt_is_admissible():
    w = T.front_door_waveform()
    assert tuple(w.shape) == (2, T.FRONT_DOOR_SAMPLES)
    start, end = T.FRONT_DOOR_SEGMENT
    assert round(start * T.FRONT_DOOR_RATE) == -T.FRONT_DOOR_LEAD
    assert round(end * T.FRONT_DOOR_RATE) == T.FRONT_DOOR_SAMPLES + T.FRONT_DOOR_TRAIL
    for orig, new in T.FRONT_DOOR_PAIRS:
        taps, L, P, width = T.bank(orig, new)
        for wave in (w, T.front_door_padded(w)):
            for row in wave.numpy():
                truth, mag = T.resample_truth(row, taps, L, P, width)
                assert T.err_over_bound(T.oracle32(row, orig, new), truth, mag, taps.shape[1]) <= 0.5
                assert ratio(T.oracle32(row, orig, new), truth) <= 0.5


@pytest.mark.parametrize("pair", T.PAIRS, **_pair_ids)
def test_impulse_cases_are_exact(pair):
    """n = 4 L + 17 and n = 1: impulses at 0 and n - 1 in every case, no two within one window, no product that leaves
    the normal range of float32 (so flushing cannot matter), and the expected values equal the float64 truth exactly"""
    orig, new = pair
    taps, L, P, width = T.bank(orig, new)
    K = taps.shape[1]
    nonzero = np.abs(taps[taps != 0]).astype(np.float64)
    assert nonzero.min() * 2.0 ** min(T.HEIGHT_EXPONENTS) >= T.TINY
    assert nonzero.max() * 2.0 ** max(T.HEIGHT_EXPONENTS) < 2.0 ** 127
    for n in (4 * L + 17, 1):
        groups = T.impulse_signals(n, K)
        everywhere = sorted(j for g, _ in groups for j in g)
        assert everywhere[0] == 0 and everywhere[-1] == n - 1
        assert len(everywhere) >= 3 or n - 1 < 2 * K + 3
        for positions, heights in groups:
            assert all(b - a >= K for a, b in zip(positions, positions[1:]))
            x = T.impulse_input(n, positions, heights)
            want = T.impulse_expected(n, positions, heights, taps, L, P, width)
            truth, _ = T.resample_truth(x, taps, L, P, width)
            assert want.dtype == np.float32 and np.array_equal(want.astype(np.float64), truth)
            assert np.count_nonzero(want) > 0


@pytest.mark.parametrize("pair", T.PAIRS, **_pair_ids)
def test_end_tap_signals_meet_taps_0_and_K_minus_1(pair):
    """the two one-impulse signals return column K - 1 of the bank in block 1 and column 0 in a later block, whole"""
    taps, L, P, width = T.bank(*pair)
    K = taps.shape[1]
    (n1, pos1, h1), (n0, pos0, h0) = T.end_tap_signals(L, width)
    for n, positions, heights, k, q in ((n1, pos1, h1, K - 1, 1), (n0, pos0, h0, 0, width // L + 2)):
        assert len(positions) == 1 and 0 <= positions[0] < n <= 1800 and positions[0] - q * L + width == k
        want = T.impulse_expected(n, positions, heights, taps, L, P, width)
        assert want.size >= (q + 1) * P
        assert np.array_equal(want[q * P:(q + 1) * P], taps[:, k] * np.float32(heights[0]))
        truth, _ = T.resample_truth(T.impulse_input(n, positions, heights), taps, L, P, width)
        assert np.array_equal(want.astype(np.float64), truth)


def test_exact_values_reach_the_clamped_taps():
    """the taps at the clamp (|t| = 6 lobes: 1e-17 and below) are among the values the exact cases ask for: a loop that
    stops one tap early shows there and nowhere else when P = 1"""
    for pair in ((48000, 16000), (16000, 8000), (96000, 16000)):
        taps, L, P, width = T.bank(*pair)
        assert P == 1 and 0 < abs(taps[0, -1]) < 1e-17
        n, positions, heights = T.end_tap_signals(L, width)[0]
        want = T.impulse_expected(n, positions, heights, taps, L, P, width)
        assert want[1] == taps[0, -1] * np.float32(heights[0]) != 0
