"""pa_conv3x3_s2_sc (csrc/emb_resnet.hip -> k_conv3x3_s2<4, 1, false, 1>, csrc/emb_conv_s2.hip): the entry of a stride-2
BasicBlock in one launch -- Y = [relu](conv3x3_s2(X) + shift) and the 1x1 stride-2 shortcut Ysc = conv1x1_s2(X) +
shift_sc, whose pixel (2y, 2x) is the 3x3 convolution's centre tap (a tenth tap with its own weights and accumulators).
By the rules of tests/kernel_parity.py with the inputs and truths of tests/conv_truth.py, on the <4, 32> half of the
grid of tests/test_conv_s2_gpu.py (B = 2; Ho = 19, 16, 17 x Wo = 31, 32, 33, each from an odd and an even input size;
cin = 16 and 48: one stage and three; cout = 64 and 128; ReLU on and off):

  * exact integer inputs: Y and Ysc both torch.equal to the integer truths;
  * float inputs: Y has the BITS of pa_conv3x3(..., stride 2) of the same library on the same operands (the nine-tap
    chain is untouched), Ysc is held to the float64 truth of the 1x1 stride-2 convolution (assert_parity); at cin = 32
    and 64 (what pa_gemm_tn_s2 accepts) its ratio and pa_gemm_tn_s2's go to the parity log side by side;
  * persistent launches (at least 3 tiles per workgroup on average, XCD-stripe holes): exact truths for both outputs,
    and two launches give the same bits;
  * B = 0 writes nothing; the refusals (Ho = 15, cout = 32, cin = 8, overlapping outputs) write nothing to either
    output and leave the documented message.
Every output lives between NaN guard blocks."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import conv_truth as T
import test_conv_s2_gpu as S2
from conftest import north_star_ratio
from kernel_parity import SEED_OFFSET, Guarded, assert_parity, dptr
from refusals import check_refusal

pytestmark = pytest.mark.gpu

CASES = [c for c in S2.CASES if c["tile"] == (4, 32)]
MANY = [c for c in S2.MANY if c["tile"] == (4, 32)]
assert len(CASES) == 9 and {(c["cin"], c["cout"]) for c in CASES} == {(16, 64), (48, 64), (16, 128), (48, 128)}
assert [(c["B"], c["H"], c["W"], c["cin"], c["cout"]) for c in MANY] == [(125, 33, 3, 16, 128), (101, 34, 4, 48, 128)]
_ids = dict(ids=lambda c: c["name"])


@pytest.fixture(scope="module")
def env(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    return dict(ffi=ffi, lib=ffi.load(), dev=gpu_device)


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


def float_shortcut(case, seed):
    """wsc (cout, cin), shift_sc (cout): the scale of conv_truth.float_inputs' 3x3 weights, one tap instead of nine"""
    g = torch.Generator().manual_seed(seed)
    wsc = torch.randn(case["cout"], case["cin"], generator=g) / case["cin"] ** 0.5
    return wsc.contiguous(), torch.randn(case["cout"], generator=g)


def exact_shortcut(case, seed):
    """dense integer weights in [-3, 3] and shifts in [-8, 8]: with |x| <= 8 every partial sum of the shortcut is an
    integer below 8 * 3 * cin + 8 < 2^24, whatever the order"""
    g = torch.Generator().manual_seed(seed)
    wsc = torch.randint(-3, 4, (case["cout"], case["cin"]), generator=g).float()
    return wsc, torch.randint(-8, 9, (case["cout"],), generator=g).float()


def shortcut_of(x, wsc, shift_sc, dtype):
    """conv1x1_s2(x) + shift_sc in `dtype`, (B, cout, Ho, Wo)"""
    return F.conv2d(x.to(dtype), wsc.to(dtype)[:, :, None, None], stride=2) + shift_sc.to(dtype).view(1, -1, 1, 1)


def _launch(env, case, xd, wd, shd, wscd, shscd, relu, y_ptr, ysc_ptr, **override):
    c = dict(case, **override)
    return env["lib"].pa_conv3x3_s2_sc(dptr(xd), c["B"], c["H"], c["W"], c["cin"], dptr(wd), dptr(shd), dptr(wscd),
                                       dptr(shscd), y_ptr, ysc_ptr, c["cout"], int(relu), env["ffi"].stream())


def _run(env, case, xd, wd, shd, wscd, shscd, relu, tag):
    """one launch into two guarded outputs -> Y, Ysc as (B, cout, Ho, Wo) on the CPU"""
    Ho, Wo = T.out_hw(case["H"], case["W"], 2)
    n = case["B"] * Ho * Wo * case["cout"]
    y, ysc = Guarded(n, env["dev"]), Guarded(n, env["dev"])
    env["ffi"].check(_launch(env, case, xd, wd, shd, wscd, shscd, relu, y.ptr, ysc.ptr), tag)
    shape = (case["B"], Ho, Wo, case["cout"])
    return (y.check(None, tag + "_Y").view(shape).permute(0, 3, 1, 2),
            ysc.check(None, tag + "_Ysc").view(shape).permute(0, 3, 1, 2))


def _unfused(env, case, xd, wd, shd, relu, tag):
    """pa_conv3x3(..., stride 2) of the same library on the same operands"""
    Ho, Wo = T.out_hw(case["H"], case["W"], 2)
    out = Guarded(case["B"] * Ho * Wo * case["cout"], env["dev"])
    env["ffi"].check(env["lib"].pa_conv3x3(dptr(xd), case["B"], case["H"], case["W"], case["cin"], dptr(wd), dptr(shd),
                                           None, out.ptr, case["cout"], 2, int(relu), env["ffi"].stream()), tag)
    return out.check(None, tag).view(case["B"], Ho, Wo, case["cout"]).permute(0, 3, 1, 2)


def _assert_exact(tag, got, truth):
    if not torch.equal(got, truth):
        bad = got != truth
        where = bad.nonzero()[0].tolist()
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} outputs differ from the integer truth, first at "
                             f"(b, channel, row, column) = {where}: {float(got[tuple(where)])} instead of "
                             f"{float(truth[tuple(where)])}")


def _exact_operands(env, case, seed, variant):
    x, w, shift, R = T.exact_inputs(case, seed, variant)
    wsc, shift_sc = exact_shortcut(case, seed + 500)
    _, packed = T.exact_image(case, w)
    dev = env["dev"]
    ops = (_nhwc(x, dev), packed.contiguous().to(dev), shift.to(dev), wsc.to(dev), shift_sc.to(dev))
    truth_sc = shortcut_of(x, wsc, shift_sc, torch.float64)
    assert bool((truth_sc == truth_sc.round()).all()) and float(truth_sc.abs().max()) < T.EXACT_LIMIT
    return ops, (x, w, shift, R), truth_sc.float()


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("case", CASES, **_ids)
def test_exact_cases(env, case, variant):
    """integers in, both integer convolutions out, bit for bit: a dropped, doubled or misplaced tap, channel, halo
    element or tile changes an output by at least 1; the ReLU alternates over the grid and never touches Ysc"""
    ops, (x, w, shift, R), truth_sc = _exact_operands(env, case, 23000 + 2 * case["index"] + variant + SEED_OFFSET,
                                                      variant)
    relu = (case["index"] + variant) % 2 == 0
    tag = f"conv_s2_sc_exact_{case['name']}_v{variant}"
    y, ysc = _run(env, case, *ops, relu, tag)
    _assert_exact(tag + "_Y", y, T.exact_truth(case, x, w, shift, R, False, relu))
    _assert_exact(tag + "_Ysc", ysc, truth_sc)


@pytest.mark.parametrize("case", CASES, **_ids)
def test_float_cases(env, case):
    """float32 inputs of the case's family, ReLU on and off: Y bit-equal to the unfused kernel's, Ysc against the
    float64 truth of the 1x1 stride-2 convolution"""
    x, w, shift, _ = T.float_inputs(case, 25000 + case["index"] + SEED_OFFSET)
    wsc, shift_sc = float_shortcut(case, 25500 + case["index"] + SEED_OFFSET)
    dev = env["dev"]
    xd, wd, shd = _nhwc(x, dev), T.direct_image(w).contiguous().to(dev), shift.to(dev)
    wscd, shscd = wsc.to(dev), shift_sc.to(dev)
    s64, s32 = shortcut_of(x, wsc, shift_sc, torch.float64), shortcut_of(x, wsc, shift_sc, torch.float32)
    for relu in (True, False):
        tag = f"conv_s2_sc_{case['name']}_{'relu' if relu else 'lin'}"
        y, ysc = _run(env, case, xd, wd, shd, wscd, shscd, relu, tag)
        want = _unfused(env, case, xd, wd, shd, relu, tag + "_unfused")
        assert torch.equal(y, want), f"{tag}: {int((y != want).sum())} of {y.numel()} outputs of Y differ from pa_conv3x3's"
        assert_parity(tag + "_Ysc", ysc, s64, s32)


@pytest.mark.parametrize("cin,cout,H,W", [(32, 64, 37, 65), (64, 128, 32, 62)])
def test_shortcut_beside_the_gemm(env, cin, cout, H, W):
    """the shapes pa_gemm_tn_s2 accepts (cin % 32 == 0): both shortcuts on the same operands against the same float64
    truth, their ratios side by side in the parity log; the fused one is held to the contract"""
    case = T._case("direct", None, 2, H, W, cin, cout, stride=2)
    case.update(index=50 + cin // 32, family="relu")
    x, w, shift, _ = T.float_inputs(case, 27000 + cin + SEED_OFFSET)
    wsc, shift_sc = float_shortcut(case, 27500 + cin + SEED_OFFSET)
    dev, ffi, lib = env["dev"], env["ffi"], env["lib"]
    xd, wd, shd = _nhwc(x, dev), T.direct_image(w).contiguous().to(dev), shift.to(dev)
    wscd, shscd = wsc.to(dev), shift_sc.to(dev)
    s64, s32 = shortcut_of(x, wsc, shift_sc, torch.float64), shortcut_of(x, wsc, shift_sc, torch.float32)
    tag = f"conv_s2_sc_{case['name']}_Ysc"
    _, ysc = _run(env, case, xd, wd, shd, wscd, shscd, True, tag)
    Ho, Wo = T.out_hw(H, W, 2)
    g = Guarded(2 * Ho * Wo * cout, dev)
    ffi.check(lib.pa_gemm_tn_s2(dptr(xd), 2, H, W, cin, dptr(wscd), cin, dptr(shscd), g.ptr, cout, cout, ffi.stream()),
              "pa_gemm_tn_s2")
    gemm = g.check(None, "pa_gemm_tn_s2").view(2, Ho, Wo, cout).permute(0, 3, 1, 2)
    assert_parity(tag, ysc, s64, s32)
    north_star_ratio(tag + "__pa_gemm_tn_s2", gemm, s64)


@pytest.mark.parametrize("case", MANY, **_ids)
def test_persistent_launches(env, case):
    """every workgroup claims tile after tile, the claims skip the holes of the index space: exact truths for both
    outputs, and a second launch gives the same bits"""
    ops, (x, w, shift, R), truth_sc = _exact_operands(env, case, 29000 + case["index"] + SEED_OFFSET, 0)
    tag = "conv_s2_sc_many_" + case["name"]
    y1, s1 = _run(env, case, *ops, True, tag)
    y2, s2 = _run(env, case, *ops, True, tag)
    _assert_exact(tag + "_Y", y1, T.exact_truth(case, x, w, shift, R, False, True))
    _assert_exact(tag + "_Ysc", s1, truth_sc)
    assert torch.equal(y1, y2) and torch.equal(s1, s2)


def test_no_images_is_no_work(env):
    case = T._case("direct", None, 0, 33, 8, 16, 64, stride=2)
    y, ysc = Guarded(17 * 4 * 64, env["dev"]), Guarded(17 * 4 * 64, env["dev"])
    big = torch.zeros(1 << 20, device=env["dev"])
    assert _launch(env, case, big, big, big, big, big, True, y.ptr, ysc.ptr) == 0
    assert y.untouched() and ysc.untouched()


REFUSALS = [
    (dict(H=30), "pa_conv3x3_s2_sc: at least 16 output rows required (got 15)"),
    (dict(cout=32), "pa_conv3x3_s2_sc: cout % 64 == 0 required"),
    (dict(cin=8), "pa_conv3x3_s2_sc: cin % 16 == 0 required"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[next(iter(c)) + str(next(iter(c.values()))) for c, _ in REFUSALS])
def test_refused_call_writes_nothing(env, change, message):
    """return code 3, the words of the source, both outputs untouched"""
    case = dict(T._case("direct", None, 2, 33, 8, 16, 64, stride=2), **change)
    assert env["lib"].pa_conv3x3_s2_sc_supported(case["H"], case["cin"], case["cout"]) == 0
    Ho, Wo = T.out_hw(case["H"], case["W"], 2)
    big = torch.zeros(1 << 20, device=env["dev"])
    out = ((2, Ho, Wo, case["cout"]), torch.float32)
    check_refusal(lambda y, ysc: _launch(env, case, big, big, big, big, big, True, y, ysc), [out, out], message,
                  env["dev"])


def test_overlapping_outputs_are_refused(env):
    """Ysc starting inside Y (and Y inside Ysc): refused although the shape is supported, nothing written"""
    case = T._case("direct", None, 2, 33, 8, 16, 64, stride=2)
    assert env["lib"].pa_conv3x3_s2_sc_supported(case["H"], case["cin"], case["cout"]) == 1
    n = 2 * 17 * 4 * 64
    big = torch.zeros(1 << 20, device=env["dev"])

    def inside(p, elements):
        return C.c_void_p(p.value + 4 * elements)
    for first in (0, 1):
        def launch(whole):
            a, b = whole, inside(whole, n - 1)
            return _launch(env, case, big, big, big, big, big, True, *((a, b) if first == 0 else (b, a)))
        check_refusal(launch, [((2 * n,), torch.float32)], "pa_conv3x3_s2_sc: Y and Ysc overlap", env["dev"])
    check_refusal(lambda whole: _launch(env, case, big, big, big, big, big, True, whole, whole),
                  [((n,), torch.float32)], "pa_conv3x3_s2_sc: Y and Ysc overlap", env["dev"])
