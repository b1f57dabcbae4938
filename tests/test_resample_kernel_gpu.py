"""`pa_resample_poly` (csrc/resample.hip: k_resample_poly) through the C ABI on its own, then `resample_on_device` and
the `Audio` front door, against the float64 truth of tests/resample_truth.py.  Output between NaN guards, input AND tap
bank between blocks of +-1e30 (tests/kernel_parity.py).  tests/test_resample_truth_cpu.py checks without a GPU that every
case here is admissible and that the exact cases are exact.

(a) dense signals (noise, DC, a tone on a pedestal) on ten rate pairs -- both tap paths, the banks on either side of the
    48 KiB switch, interpolating and decimating, targets other than 16 kHz -- at lengths around 1, width, L and the
    256-thread block edge, element-wise within the float32 summation bound gamma_K mag + K 2^-126: a theorem, not a
    measurement.  The project contract (rtol 1e-4 / atol 1e-5) is asserted too; it is three orders looser here.
(b) exact cases, compared as values with no tolerance: isolated impulses of height 2^e return single taps; L zeros in
    front of a signal shift the output by one block, bit for bit; empty and refused calls write nothing.
(c) rows of a (3, n) waveform, n odd, equal three single-row calls; `Audio(sample_rate=r)` on a CPU waveform, a
    device-resident one and a padded crop, for r of 8000, 16000 and 44100.

One line per pair goes to the parity log that tests/conftest.py keeps (`report`); profiles/resample_parity.txt is a copy
of those lines."""
import math

import numpy as np
import pytest
import torch

import resample_truth as T
from conftest import north_star_ratio, report
from kernel_parity import Guarded, GuardedInput

pytestmark = pytest.mark.gpu

_pair_ids = dict(ids=lambda p: f"{p[0]}to{p[1]}")
REFUSED = "pa_resample_poly: inconsistent filter bank shape"


@pytest.fixture(scope="module")
def env(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    banks = {}
    for pair in T.PAIRS:
        taps, L, P, width = T.bank(*pair)
        banks[pair] = (GuardedInput(torch.from_numpy(taps), gpu_device), L, P, taps.shape[1], width)
    return dict(ffi=ffi, lib=ffi.load(), dev=gpu_device, banks=banks)


def _call(env, pair, x, n_out=None, tag=""):
    """one guarded call -> the n_out outputs as float32 numpy (n_out: ceil(P n / L) unless given)"""
    ffi, lib = env["ffi"], env["lib"]
    tp, L, P, K, width = env["banks"][pair]
    n = int(x.size)
    n_out = T.num_out(n, L, P) if n_out is None else n_out
    xin = GuardedInput(torch.from_numpy(x), env["dev"])
    out = Guarded(n_out, env["dev"])
    ffi.check(lib.pa_resample_poly(xin.ptr, n, tp.ptr, L, P, K, width, out.ptr, n_out, ffi.stream()), tag)
    return out.check(None, tag).numpy().copy()


def _assert_within_bound(got, truth, mag, K, what):
    assert got.shape == truth.shape, what
    r = T.err_over_bound(got, truth, mag, K)
    assert r <= 1.0, f"{what}: max |err| / bound = {r:.3f} (worst output {int(np.argmax(np.abs(got - truth) / T.bound(mag, K)))})"
    return r


# ---------------------------------------------------------------------------------------------------------------------
# (a) dense signals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", T.PAIRS, **_pair_ids)
def test_dense_signals_within_summation_bound(env, pair):
    orig, new = pair
    _, L, P, K, width = env["banks"][pair]
    tag = f"resample_kernel_{orig}to{new}"
    worst = worst32 = 0.0
    gots, truths = [], []
    for case in T.dense_cases(orig, new):
        what = f"{tag}_{case['name']}"
        got = _call(env, pair, case["x"], tag=what)
        worst = max(worst, _assert_within_bound(got, case["truth"], case["mag"], K, what))
        worst32 = max(worst32, T.err_over_bound(case["oracle"], case["truth"], case["mag"], K))
        gots.append(got)
        truths.append(case["truth"])
    for n, n_out in T.EDGE_OUTPUTS.get(pair, []):            # fewer outputs than the input gives: the block edge for L = 1
        for name, x in T.signals(orig, new, n).items():
            truth, mag = T.resample_truth(x, T.bank(orig, new)[0], L, P, width)
            what = f"{tag}_{name}_n{n}_out{n_out}"
            got = _call(env, pair, x, n_out=n_out, tag=what)
            worst = max(worst, _assert_within_bound(got, truth[:n_out], mag[:n_out], K, what))
            gots.append(got)
            truths.append(truth[:n_out])
    got, truth = np.concatenate(gots), np.concatenate(truths)
    contract = north_star_ratio(tag, torch.from_numpy(got), torch.from_numpy(truth))
    report(f"resample kernel {orig}->{new} (L {L}, P {P}, K {K}): max|err|/bound = {worst:.3f} (float32 oracle "
           f"{worst32:.3f}) over {len(gots)} calls; contract ratio {contract:.4f}", torch.from_numpy(got),
           torch.from_numpy(truth))
    assert worst32 <= 0.5          # (admissibility: tests/test_resample_truth_cpu.py holds the same cases to it)
    assert contract <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# (b) exact cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", T.PAIRS, **_pair_ids)
def test_impulses_return_single_taps(env, pair):
    """impulses of height 1, 1/8 and 32 at 0, at n - 1 and every K + 3 samples in between: every output is one exact
    product taps[p][j - q L + width] 2^e, or 0 where no impulse is in reach -- the tap row p K, the base q L - width and
    the zero fill on both sides, with nothing to hide behind (n = 4 L + 17 and n = 1)"""
    orig, new = pair
    taps, L, P, width = T.bank(orig, new)
    cases = [(n, positions, heights) for n in (4 * L + 17, 1) for positions, heights in T.impulse_signals(n, taps.shape[1])]
    for n, positions, heights in cases + T.end_tap_signals(L, width):      # (and taps 0 and K - 1, one impulse each)
        what = f"impulses {orig}->{new} n={n} at {positions}"
        got = _call(env, pair, T.impulse_input(n, positions, heights), tag=what)
        want = T.impulse_expected(n, positions, heights, taps, L, P, width)
        wrong = np.flatnonzero(got != want)
        assert wrong.size == 0, (f"{what}: {wrong.size} of {want.size} outputs differ, the first at o = {wrong[0]} "
                                 f"(q {wrong[0] // P}, p {wrong[0] % P}): got {got[wrong[0]]!r}, want {want[wrong[0]]!r}")


@pytest.mark.parametrize("pair", T.PAIRS, **_pair_ids)
def test_block_shift(env, pair):
    """L zeros in front of the signal: one more block in front, within the bound; everything behind it the same bits
    (the same operands in the same order)"""
    orig, new = pair
    taps, L, P, width = T.bank(orig, new)
    for n in T.shift_lengths(orig, new):
        x, shifted = T.shift_input(orig, new, n)
        what = f"shift {orig}->{new} n={n}"
        base = _call(env, pair, x, tag=what)
        got = _call(env, pair, shifted, tag=what + " shifted")
        assert got.size == base.size + P
        assert np.array_equal(got[P:].view(np.int32), base.view(np.int32)), f"{what}: blocks 1.. are not block 0.. of x"
        truth, mag = T.resample_truth(shifted, taps, L, P, width)
        _assert_within_bound(got[:P], truth[:P], mag[:P], taps.shape[1], what + " first block")


@pytest.mark.parametrize("pair", [(8000, 16000), (44100, 16000)], **_pair_ids)
def test_no_outputs(env, pair):
    """n_out = 0: returns 0, writes nothing (one pair per tap path)"""
    tp, L, P, K, width = env["banks"][pair]
    xin = GuardedInput(torch.ones(8), env["dev"])
    out = Guarded(16, env["dev"])
    assert env["lib"].pa_resample_poly(xin.ptr, 8, tp.ptr, L, P, K, width, out.ptr, 0, env["ffi"].stream()) == 0
    assert env["lib"].pa_resample_poly(xin.ptr, 0, tp.ptr, L, P, K, width, out.ptr, 0, env["ffi"].stream()) == 0
    assert out.untouched()


@pytest.mark.parametrize("change", [dict(K=-1), dict(K=+1), dict(width=+1), dict(L=0), dict(P=0), dict(L=-3), dict(P=-1)],
                         ids=["K_less", "K_more", "width_more", "L0", "P0", "L_negative", "P_negative"])
def test_refusals(env, change):
    """K != 2 width + L, L or P not positive: an error with its message, and nothing runs"""
    ffi, lib = env["ffi"], env["lib"]
    tp, L, P, K, width = env["banks"][(48000, 16000)]
    args = dict(L=L, P=P, K=K, width=width)
    for name, v in change.items():
        args[name] = args[name] + v if name in ("K", "width") else v
    xin = GuardedInput(torch.ones(64), env["dev"])
    out = Guarded(64, env["dev"])
    rc = lib.pa_resample_poly(xin.ptr, 64, tp.ptr, args["L"], args["P"], args["K"], args["width"], out.ptr, 22,
                              ffi.stream())
    assert rc == 3
    assert lib.pa_last_error().decode() == REFUSED
    with pytest.raises(ValueError, match="pa_resample_poly"):
        ffi.check(rc, "refusal")
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# (c) resample_on_device and the front door
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,n", [((8000, 16000), 1001), ((44100, 16000), 1783), ((10000, 10100), 333)],
                         ids=["8000to16000", "44100to16000", "10000to10100"])
def test_rows_equal_single_row_calls(env, pair, n):
    """(3, n), n odd: rows 1 and 2 start 4 and 8 bytes off a 16-byte boundary, and give the bits of one-row calls (whose
    row is aligned) -- which are the bits of the guarded C ABI call"""
    from pyannote_audio_amd.audio import resample_on_device
    orig, new = pair
    w = torch.from_numpy(np.stack([T.signals(orig, new, n + i)[name][:n]
                                   for i, name in enumerate(("noise", "tone", "noise"))]))
    assert n % 2 == 1 and tuple(w.shape) == (3, n)
    got = resample_on_device(w, orig, new, env["dev"])
    assert tuple(got.shape) == (3, math.ceil(new * n / orig)) and got.dtype == torch.float32
    for c in range(3):
        one = resample_on_device(w[c:c + 1].clone(), orig, new, env["dev"])
        assert np.array_equal(got[c].cpu().numpy().view(np.int32), one[0].cpu().numpy().view(np.int32)), f"row {c}"
        direct = _call(env, pair, w[c].numpy(), tag=f"row {c}")
        assert np.array_equal(one[0].cpu().numpy().view(np.int32), direct.view(np.int32)), f"row {c} vs the C ABI"


def _assert_front_door(got, sr, wave, rate, what):
    """`got` (channel, time) of the front door against the truth of each row of `wave` at 22 050 Hz -> rate"""
    taps, L, P, width = T.bank(T.FRONT_DOOR_RATE, rate)
    assert sr == rate and got.is_cuda and got.dtype == torch.float32
    assert tuple(got.shape) == (wave.shape[0], math.ceil(rate * wave.shape[1] / T.FRONT_DOOR_RATE)), what
    worst, truths = 0.0, []
    for c, row in enumerate(wave.numpy()):
        truth, mag = T.resample_truth(row, taps, L, P, width)
        worst = max(worst, _assert_within_bound(got[c].cpu().numpy(), truth, mag, taps.shape[1], f"{what} row {c}"))
        truths.append(truth)
    report(f"resample front door {T.FRONT_DOOR_RATE}->{rate} ({what}): max|err|/bound = {worst:.3f}", got,
           torch.from_numpy(np.stack(truths)))


@pytest.mark.parametrize("rate", [8000, 16000, 44100])
def test_front_door(env, rate):
    """a (2, 6615) waveform at 22 050 Hz through `Audio(sample_rate=rate, device=gpu)`: from the host, resident on the
    device, and cropped in "pad" mode by a segment that reaches past both ends (the truth of the padded excerpt)"""
    from pyannote_audio_amd.audio import Audio
    from pyannote_audio_amd.core import Segment
    audio = Audio(sample_rate=rate, mono=None, device=env["dev"])
    w = T.front_door_waveform()
    got, sr = audio({"waveform": w, "sample_rate": T.FRONT_DOOR_RATE})
    _assert_front_door(got, sr, w, rate, "host waveform")
    resident, sr = audio({"waveform": w.to(env["dev"]), "sample_rate": T.FRONT_DOOR_RATE})
    _assert_front_door(resident, sr, w, rate, "resident waveform")
    assert torch.equal(resident, got)
    for where, wave in (("host", w), ("resident", w.to(env["dev"]))):
        cropped, sr = audio.crop({"waveform": wave, "sample_rate": T.FRONT_DOOR_RATE}, Segment(*T.FRONT_DOOR_SEGMENT),
                                 mode="pad")
        _assert_front_door(cropped, sr, T.front_door_padded(w), rate, f"padded crop of the {where} waveform")
