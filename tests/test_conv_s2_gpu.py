"""The stride-2 3x3 convolution kernel k_conv3x3_s2 (csrc/emb_conv_s2.hip) through pa_conv3x3(..., stride = 2, ...), on
shapes chosen for ITS tile geometry -- a workgroup tile of TH x TW output pixels x 64 output channels, 16 input channels
per stage; <TH, TW> = <4, 32> for Ho >= 16 and <2, 64> below -- by the rules of tests/kernel_parity.py with the inputs
and truths of tests/conv_truth.py:

  * output sizes one less than a tile multiple, a tile multiple and one more, in rows and columns, each reached from an
    odd and from an even input size; cin = 16 (one stage: no buffer swap, the next tile staged from the only run) and 48
    (three stages: both buffers, an odd count); cout = 64 and 128 (one and two channel slices of a pixel tile);
  * float inputs against the float64 truth (assert_parity) with the residual and the ReLU on and off; exact integer
    inputs against the integer convolution with torch.equal;
  * persistent launches on tiny maps in which every resident workgroup claims at least three tiles on average and the
    tile index space has XCD-stripe holes: exact truth, and two launches give the same bits;
  * B = 0 and a refused call (cout = 32) write nothing.
Every output lives between NaN guard blocks."""
import pytest
import torch

import conv_truth as T
from kernel_parity import SEED_OFFSET, Guarded, assert_parity, dptr
from refusals import check_refusal

pytestmark = pytest.mark.gpu

#: (TH, TW) of the launcher's two instantiations and the output heights that select them: a tile multiple - 1, a tile
#: multiple, a tile multiple + 1 (Ho >= 16 selects <4, 32>: 19 = 20 - 1, 16, 17)
GEOMETRIES = {(4, 32): (19, 16, 17), (2, 64): (1, 2, 3)}
EPILOGUES = ((True, True), (False, False), (True, False), (False, True))     # (residual, ReLU)


def instantiation(Ho):
    """launch_conv_s2 (csrc/emb_conv_s2.hip)"""
    return (4, 32) if Ho >= 16 else (2, 64)


def _cases():
    out = []
    for (th, tw), heights in GEOMETRIES.items():
        for i, Ho in enumerate(heights):
            for k, Wo in enumerate((tw - 1, tw, tw + 1)):
                g = 3 * i + k
                # every Ho and every Wo from an odd and from an even input size (the parities alternate over the grid)
                H, W = 2 * Ho - (i + k) % 2, 2 * Wo - (i + k + 1) % 2
                cin, cout = (16, 48)[g % 2], (64, 128)[(g // 2) % 2]
                c = T._case("direct", None, 2, H, W, cin, cout, stride=2)
                assert T.out_hw(H, W, 2) == (Ho, Wo) and instantiation(Ho) == (th, tw)
                c.update(index=len(out), family=T.FAMILIES[len(out) % len(T.FAMILIES)], tile=(th, tw))
                out.append(c)
    return out


def _many():
    """(tile, B, H, W, cin): cout = 128, so a pixel tile has two channel slices; B x pixel tiles is no multiple of 8
    (the index space is padded to whole XCD stripes: holes) and there are at least 3 tiles per compute unit ON AVERAGE
    (tiles are claimed at run time: what a single workgroup gets cannot be asserted)"""
    out = []
    for tile, B, H, W, cin in (((4, 32), 125, 33, 3, 16), ((4, 32), 101, 34, 4, 48), ((2, 64), 313, 5, 4, 16),
                               ((2, 64), 257, 6, 3, 48)):
        c = T._case("direct", None, B, H, W, cin, 128, stride=2, many=True)
        Ho, Wo = T.out_hw(H, W, 2)
        th, tw = tile
        pairs = B * T.cdiv(Ho, th) * T.cdiv(Wo, tw)
        assert instantiation(Ho) == tile and pairs % 8 != 0 and 2 * pairs >= 3 * T.CUS
        c.update(index=100 + len(out), family="randn", tile=tile)
        out.append(c)
    return out


CASES, MANY = _cases(), _many()
_ids = dict(ids=lambda c: c["name"])


@pytest.fixture(scope="module")
def env(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    return dict(ffi=ffi, lib=ffi.load(), dev=gpu_device)


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


def _launch(env, case, xd, wd, shd, rd, relu, out_ptr, **override):
    c = dict(case, **override)
    return env["lib"].pa_conv3x3(dptr(xd), c["B"], c["H"], c["W"], c["cin"], dptr(wd), dptr(shd), dptr(rd), out_ptr,
                                 c["cout"], 2, int(relu), env["ffi"].stream())


def _run(env, case, xd, wd, shd, rd, relu, tag):
    """one launch into a guarded output -> (B, cout, Ho, Wo) on the CPU; the guards are NaN afterwards, no output is"""
    Ho, Wo = T.out_hw(case["H"], case["W"], 2)
    out = Guarded(case["B"] * Ho * Wo * case["cout"], env["dev"])
    env["ffi"].check(_launch(env, case, xd, wd, shd, rd, relu, out.ptr), tag)
    return out.check(None, tag).view(case["B"], Ho, Wo, case["cout"]).permute(0, 3, 1, 2)


def _operands(env, x, image, shift, R):
    dev = env["dev"]
    return _nhwc(x, dev), image.contiguous().to(dev), shift.to(dev), _nhwc(R, dev)


def _assert_exact(tag, got, truth):
    if not torch.equal(got, truth):
        bad = got != truth
        where = bad.nonzero()[0].tolist()
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} outputs differ from the integer convolution, "
                             f"first at (b, channel, row, column) = {where}: {float(got[tuple(where)])} instead of "
                             f"{float(truth[tuple(where)])}")


@pytest.mark.parametrize("case", CASES, **_ids)
def test_float_cases(env, case):
    """float32 inputs of the case's family, all four epilogues, against the float64 truth"""
    x, w, shift, R = T.float_inputs(case, 17000 + case["index"] + SEED_OFFSET)
    xd, wd, shd, rd = _operands(env, x, T.direct_image(w), shift, R)
    c64, c32 = T.conv_of(x, w, 2, torch.float64), T.conv_of(x, w, 2, torch.float32)
    for use_res, relu in EPILOGUES:
        tag = f"conv_s2_{case['name']}_{'res' if use_res else 'nores'}_{'relu' if relu else 'lin'}"
        got = _run(env, case, xd, wd, shd, rd if use_res else None, relu, tag)
        assert_parity(tag, got, T.finish(c64, shift, R, use_res, relu), T.finish(c32, shift, R, use_res, relu))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("case", CASES, **_ids)
def test_exact_cases(env, case, variant):
    """integers in, the integer convolution out, bit for bit: a dropped, doubled or misplaced tap, channel, halo
    element or tile changes an output by at least 1"""
    x, w, shift, R = T.exact_inputs(case, 19000 + 2 * case["index"] + variant + SEED_OFFSET, variant)
    _, packed = T.exact_image(case, w)
    xd, wd, shd, rd = _operands(env, x, packed, shift, R)
    use_res, relu = EPILOGUES[(2 * case["index"] + variant) % 4]
    tag = f"conv_s2_exact_{case['name']}_v{variant}"
    got = _run(env, case, xd, wd, shd, rd if use_res else None, relu, tag)
    _assert_exact(tag, got, T.exact_truth(case, x, w, shift, R, use_res, relu))


@pytest.mark.parametrize("case", MANY, **_ids)
def test_persistent_launches(env, case):
    """every workgroup claims tile after tile, the claims skip the holes of the index space: exact truth, and the tile
    counters decide who computes a tile, never how -- a second launch gives the same bits"""
    x, w, shift, R = T.exact_inputs(case, 21000 + case["index"] + SEED_OFFSET, 0)
    _, packed = T.exact_image(case, w)
    ops = _operands(env, x, packed, shift, R)
    first = _run(env, case, *ops, True, "conv_s2_many_" + case["name"])
    second = _run(env, case, *ops, True, "conv_s2_many_" + case["name"])
    _assert_exact("conv_s2_many_" + case["name"], first, T.exact_truth(case, x, w, shift, R, True, True))
    assert torch.equal(first, second)


def test_no_images_is_no_work(env):
    case = T._case("direct", None, 0, 33, 8, 16, 64, stride=2)
    out = Guarded(17 * 4 * 64, env["dev"])
    big = torch.zeros(1 << 20, device=env["dev"])
    assert _launch(env, case, big, big, big, big, True, out.ptr) == 0
    assert out.untouched()


def test_refused_call_writes_nothing(env):
    """cout = 32 at stride 2: return code 3, the words of the source, the output untouched"""
    case = T._case("direct", None, 2, 33, 8, 16, 32, stride=2)
    big = torch.zeros(1 << 20, device=env["dev"])
    check_refusal(lambda out: _launch(env, case, big, big, big, big, True, out),
                  [((2, 17, 4, 32), torch.float32)], "pa_conv3x3: stride 2 needs cout % 64 == 0", env["dev"])
