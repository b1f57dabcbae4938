"""The three 3x3 convolution families (csrc/emb_resnet.hip: pa_conv3x3; csrc/emb_winograd.hip: pa_conv3x3_wino[_rows];
csrc/emb_winograd4.hip: pa_conv3x3_wino4[_rows]) through the C ABI on their own, by the rules of tests/kernel_parity.py.
Cases, inputs, truths, host replays and exact weight images are in tests/conv_truth.py; tests/test_conv_truth_cpu.py
proves without a GPU that the cases reach every instantiation, are admissible and cheap, and that every exact case is
exact.  The switches PA_WINO4_LINEAR, PA_WINO32 and PA_XCD_RANGES are read once per process: every launch here takes the
launcher's own choice.

  * float cases (five input families: white noise, post-ReLU maps, a large mean, per-input-channel and per-output-channel
    scales over two decades) against the float64 truth.  The direct kernel and F(2x2): kernel_parity.assert_parity.
    F(4x4): max |err| <= 1e-4 max |truth| AND element-wise ratio <= max(1, 2 x that of the float32 host replay of the
    kernel's own arithmetic) -- kernel, replay and quotient are printed, one line per case and variant
    (profiles/conv_truth_f4.txt holds the lines of one run; both ratios are also in the parity log of tests/conftest.py);
  * exact cases: integer inputs, sparse integer weights, weight images scaled so that every intermediate is an integer
    below 2^24: torch.equal with the integer convolution, no tolerance.  A dropped, doubled or misplaced tap, channel,
    halo element or tile changes an output by at least 1;
  * every output lives between NaN guard blocks; the rows a row-range launch does not own stay NaN;
  * two launches of a persistent kernel give the same bits; refused calls and B = 0 write nothing;
  * pa_absmax_diff, the measuring instrument of the Winograd guard, against numpy."""
import numpy as np
import pytest
import torch

import conv_truth as T
from conftest import north_star_ratio
from kernel_parity import GUARD, SEED_OFFSET, Guarded, GuardedInput, assert_parity, dptr, ratio
from refusals import check_refusal

pytestmark = pytest.mark.gpu

_ids = dict(ids=lambda c: c["name"])


def float_seed(case):
    return T.float_seed(case, SEED_OFFSET)


def exact_seed(case, variant):
    return T.exact_seed(case, variant, SEED_OFFSET)


@pytest.fixture(scope="module")
def env(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    return dict(ffi=ffi, lib=ffi.load(), dev=gpu_device)


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


def _float_image(case, w):
    from pyannote_audio_amd.weights import winograd4_pack, winograd4_weights, winograd_pack, winograd_weights
    if case["algo"] == "direct":
        return T.direct_image(w)
    if case["algo"] == "wino":
        return winograd_pack(winograd_weights(w))
    return winograd4_pack(winograd4_weights(w))


def _call(env, case, xd, wd, shd, rd, relu, out_ptr, **override):
    """one launch through the entry point the case is for -> return code"""
    ffi, lib = env["ffi"], env["lib"]
    c = dict(case, **override)
    head = (dptr(xd), c["B"], c["H"], c["W"], c["cin"], dptr(wd), dptr(shd), dptr(rd), out_ptr, c["cout"])
    if c["algo"] == "direct":
        return lib.pa_conv3x3(*head, c["stride"], int(relu), ffi.stream())
    if c["algo"] == "wino":
        if c["y_first"] == 0:
            return lib.pa_conv3x3_wino(*head, int(relu), ffi.stream())
        return lib.pa_conv3x3_wino_rows(*head, int(relu), c["y_first"], ffi.stream())
    if c["rows"] == c["H"]:
        return lib.pa_conv3x3_wino4(*head, int(relu), ffi.stream())
    return lib.pa_conv3x3_wino4_rows(*head, int(relu), c["rows"], ffi.stream())


def _run(env, case, xd, wd, shd, rd, relu, tag):
    """launch into a guarded output -> (B, cout, rows written, Wo) on the CPU; guards, and the rows of the map the launch
    does not own, are NaN afterwards, nothing it owns is"""
    B, cout = case["B"], case["cout"]
    Ho, Wo = T.out_hw(case["H"], case["W"], case["stride"])
    out = Guarded(B * Ho * Wo * cout, env["dev"])
    env["ffi"].check(_call(env, case, xd, wd, shd, rd, relu, out.ptr), tag)
    lo, hi = T.written_rows(case)
    written = None
    if (lo, hi) != (0, Ho):
        written = torch.zeros(B, Ho, Wo, cout, dtype=torch.bool)
        written[:, lo:hi] = True
    y = out.check(written, tag).view(B, Ho, Wo, cout)
    return y[:, lo:hi].permute(0, 3, 1, 2)


def _device_operands(env, x, image, shift, R):
    dev = env["dev"]
    return _nhwc(x, dev), image.contiguous().to(dev), shift.to(dev), _nhwc(R, dev)


# ---------------------------------------------------------------------------------------------------------------------
# float cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.FLOAT_CASES, **_ids)
def test_float_cases(env, case):
    x, w, shift, R = T.float_inputs(case, float_seed(case))
    image = _float_image(case, w)
    xd, wd, shd, rd = _device_operands(env, x, image, shift, R)
    c64, c32 = T.conv_of(x, w, case["stride"], torch.float64), T.conv_of(x, w, case["stride"], torch.float32)
    crep = T.wino4_replay(x, image) if case["algo"] == "wino4" else None
    lo, hi = T.written_rows(case)
    for use_res, relu in case["variants"]:
        tag = f"conv_truth_{case['name']}_{'res' if use_res else 'nores'}_{'relu' if relu else 'lin'}"
        got = _run(env, case, xd, wd, shd, rd if use_res else None, relu, tag)
        whole = T.finish(c64, shift, R, use_res, relu)
        truth, ref32 = whole[:, :, lo:hi], T.finish(c32, shift, R, use_res, relu)[:, :, lo:hi]
        if case["algo"] != "wino4":
            assert_parity(tag, got, truth, ref32)
            continue
        r32 = ratio(ref32, truth)
        assert r32 <= 0.5, f"{tag}: inadmissible case -- float32 torch is itself {r32:.3f} of the contract away"
        rep = T.finish(crep, shift, R, use_res, relu)[:, :, lo:hi]
        r_rep = north_star_ratio(tag + "__float32_replay", rep, truth)
        r = north_star_ratio(tag, got, truth)
        err = float((got.double() - truth).abs().max()) / float(whole.abs().max())
        line = (f"{case['name']:42s} {case['family']:10s} res={int(use_res)} relu={int(relu)}  kernel {r:7.3f}  "
                f"replay {r_rep:7.3f}  quotient {r / r_rep:5.2f}  max|err|/max|truth| {err:.2e}")
        print(line)
        assert err <= 1e-4, f"{tag}: max |err| = {err:.2e} max |truth|"
        assert r <= max(1.0, 2.0 * r_rep), f"{tag}: kernel {r:.3f}, float32 replay {r_rep:.3f} of the contract"


# ---------------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("case", T.EXACT_CASES, **_ids)
def test_exact_cases(env, case, variant):
    """integers in, the integer convolution out, bit for bit (the proof that nothing rounds: test_conv_truth_cpu)"""
    x, w, shift, R = T.exact_inputs(case, exact_seed(case, variant), variant)
    _, packed = T.exact_image(case, w)
    xd, wd, shd, rd = _device_operands(env, x, packed, shift, R)
    use_res, relu = case["variants"][variant]
    tag = f"conv_exact_{case['name']}_v{variant}"
    got = _run(env, case, xd, wd, shd, rd if use_res else None, relu, tag)
    lo, hi = T.written_rows(case)
    truth = T.exact_truth(case, x, w, shift, R, use_res, relu)[:, :, lo:hi]
    if not torch.equal(got, truth):
        bad = (got != truth)
        where = bad.nonzero()[0].tolist()
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} outputs differ from the integer convolution, "
                             f"first at (b, channel, row, column) = {where}: {float(got[tuple(where)])} instead of "
                             f"{float(truth[tuple(where)])}")


# ---------------------------------------------------------------------------------------------------------------------
# reproducibility, no work, refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in T.CASES if c["many"]], **_ids)
def test_two_launches_give_the_same_bits(env, case):
    """every persistent kernel, on the launch in which each workgroup claims several tiles: the tile counters decide who
    computes a tile, never how"""
    x, w, shift, R = T.float_inputs(case, float_seed(case))
    ops = _device_operands(env, x, _float_image(case, w), shift, R)
    first = _run(env, case, *ops, True, "repro_" + case["name"])
    second = _run(env, case, *ops, True, "repro_" + case["name"])
    assert torch.equal(first, second)


def _big(env, n=1 << 20):
    return torch.zeros(n, device=env["dev"])


@pytest.mark.parametrize("algo", ["direct", "wino", "wino4"])
def test_no_images_is_no_work(env, algo):
    case = T._case(algo, None, 0, 8, 8, 32, 32)
    out = Guarded(8 * 8 * 32, env["dev"])
    big = _big(env)
    assert _call(env, case, big, big, big, big, True, out.ptr) == 0
    assert out.untouched()


REFUSALS = [
    ("direct", dict(cin=24), "pa_conv3x3: cin % 16 and cout % 32 required"),
    ("direct", dict(cout=48), "pa_conv3x3: cin % 16 and cout % 32 required"),
    ("direct", dict(stride=3), "pa_conv3x3: stride 3 not supported"),
    ("direct", dict(stride=2, cout=96), "pa_conv3x3: stride 2 needs cout % 64 == 0"),
    ("wino", dict(cin=24), "pa_conv3x3_wino: cin % 16 and cout % 32 required"),
    ("wino", dict(cout=48), "pa_conv3x3_wino: cin % 16 and cout % 32 required"),
    ("wino", dict(y_first=3), "pa_conv3x3_wino_rows: y_first must be even and >= 0 (got 3)"),
    ("wino", dict(y_first=-2), "pa_conv3x3_wino_rows: y_first must be even and >= 0 (got -2)"),
    ("wino4", dict(cin=16), "pa_conv3x3_wino4: cin % 8 == 0, cin >= 32 and cout % 32 == 0 required"),
    ("wino4", dict(cin=36), "pa_conv3x3_wino4: cin % 8 == 0, cin >= 32 and cout % 32 == 0 required"),
    ("wino4", dict(cout=48), "pa_conv3x3_wino4: cin % 8 == 0, cin >= 32 and cout % 32 == 0 required"),
    ("wino4", dict(rows=6), "pa_conv3x3_wino4_rows: rows must be H or a multiple of 4 below it"),
    ("wino4", dict(rows=12), "pa_conv3x3_wino4_rows: rows must be H or a multiple of 4 below it"),
]


@pytest.mark.parametrize("algo,change,message", REFUSALS, ids=[f"{a}_{'_'.join(f'{k}{v}' for k, v in c.items())}"
                                                               for a, c, _ in REFUSALS])
def test_refusals_write_nothing(env, algo, change, message):
    """return code 3, the words of the source in pa_last_error, the output untouched; the operands are real and large
    enough for the refused shape, were it wrongly accepted"""
    case = dict(T._case(algo, None, 2, 8, 8, 64, 64), **change)
    big = _big(env)
    Ho, Wo = T.out_hw(8, 8, case["stride"])
    check_refusal(lambda out: _call(env, case, big, big, big, big, True, out),
                  [((2, Ho, Wo, case["cout"]), torch.float32)], message, env["dev"])


# ---------------------------------------------------------------------------------------------------------------------
# pa_absmax_diff
# ---------------------------------------------------------------------------------------------------------------------
def _absmax(env, got, ref, n, out2):
    ffi, lib = env["ffi"], env["lib"]
    g, r = GuardedInput(got, env["dev"]), GuardedInput(ref, env["dev"])      # +-1e30 around both: an over-read shows
    ffi.check(lib.pa_absmax_diff(g.ptr, r.ptr, n, out2.ptr, ffi.stream()), "pa_absmax_diff")


def _slots(out2):
    torch.cuda.synchronize()
    host = out2.buf.cpu()
    assert bool(torch.isnan(host[:GUARD]).all()) and bool(torch.isnan(host[GUARD + 2:]).all())
    return host[GUARD:GUARD + 2].numpy()


def _fresh(env, a=0.0, b=0.0):
    out2 = Guarded(2, env["dev"])
    out2.buf[GUARD:GUARD + 2] = torch.tensor([a, b], device=env["dev"])
    return out2


@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 2048 + 257])
def test_absmax_diff_against_numpy(env, n):
    """n around the block size, and past the grid cap of 2048 workgroups x 2048 elements (the strided loop takes more
    than its eight rounds); the largest |ref| and the largest |got - ref| sit at the last element in one call and
    at the first in the next; out2 accumulates over the two calls; nothing outside [0, n) is read"""
    g = torch.Generator().manual_seed(50 + SEED_OFFSET)
    ref, got = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ref[-1], got[-1] = -7.0, 9.5                                              # |ref| 7, |got - ref| 16.5 at n - 1
    out2 = _fresh(env)
    _absmax(env, got, ref, n, out2)
    want = np.array([np.abs(ref.numpy()).max(), np.abs(got.numpy() - ref.numpy()).max()], dtype=np.float32)
    assert want[0] == 7.0 and want[1] == 16.5
    assert np.array_equal(_slots(out2), want)
    # second call, smaller values: the slots keep their maxima; then larger ones at element 0: they move
    _absmax(env, 0.5 * got, 0.5 * ref, n, out2)
    assert np.array_equal(_slots(out2), want)
    ref2, got2 = ref.clone(), got.clone()
    ref2[0], got2[0] = 11.0, -11.0
    _absmax(env, got2, ref2, n, out2)
    assert np.array_equal(_slots(out2), np.array([11.0, 22.0], dtype=np.float32))
    # told of fewer elements than there are, it does not read the rest
    if n > 1:
        out3 = _fresh(env)
        _absmax(env, got2, ref2, n - 1, out3)
        want3 = np.array([np.abs(ref2[:-1].numpy()).max(), np.abs((got2 - ref2)[:-1].numpy()).max()], dtype=np.float32)
        assert np.array_equal(_slots(out3), want3)


def test_absmax_diff_no_elements(env):
    out2 = _fresh(env, 1.5, 2.5)
    _absmax(env, torch.ones(4), torch.ones(4), 0, out2)
    assert np.array_equal(_slots(out2), np.array([1.5, 2.5], dtype=np.float32))


def test_absmax_diff_signed_zeros(env):
    """-0.0 everywhere: both maxima are +0.0 (bit pattern 0 -- the integer atomicMax orders -0.0 above every float)"""
    n = 300
    out2 = _fresh(env)
    _absmax(env, torch.full((n,), -0.0), torch.full((n,), -0.0), n, out2)
    assert _slots(out2).view(np.uint32).tolist() == [0, 0]
    _absmax(env, torch.zeros(n), torch.full((n,), -0.0), n, out2)
    _absmax(env, torch.full((n,), -0.0), torch.zeros(n), n, out2)
    assert _slots(out2).view(np.uint32).tolist() == [0, 0]


@pytest.mark.parametrize("got_v,ref_v,max_ref", [
    (float("nan"), 1.0, 3.0), (float("inf"), 1.0, 3.0), (float("-inf"), 1.0, 3.0),
    (float("inf"), float("inf"), float("inf")),          # inf - inf is NaN: counted as +inf, like any NaN
    (1.0, float("nan"), 3.0),                            # NaN in ref: the difference is +inf, max |ref| skips it
    (float("nan"), float("nan"), 3.0),
], ids=["nan_got", "inf_got", "minf_got", "inf_both", "nan_ref", "nan_both"])
def test_absmax_diff_non_finite(env, got_v, ref_v, max_ref):
    """what the comment of k_absmax_diff states: a non-finite difference (NaN or +-inf in `got`, NaN in `ref`, inf on
    both sides) counts as +inf; max |ref| is taken over the elements of `ref` that are not NaN"""
    n = 257
    ref, got = torch.full((n,), -3.0), torch.full((n,), -2.0)
    got[200], ref[200] = got_v, ref_v
    out2 = _fresh(env)
    _absmax(env, got, ref, n, out2)
    slots = _slots(out2)
    assert slots[1] == np.inf and slots[0] == np.float32(max_ref)
