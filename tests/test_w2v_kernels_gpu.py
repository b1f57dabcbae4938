"""Every kernel of the wav2vec 2.0 / WavLM encoder that is not a GEMM (csrc/w2v.hip: pa_w2v_conv0,
pa_w2v_group_norm_gelu, pa_w2v_layernorm, pa_w2v_posconv, pa_w2v_softmax, pa_w2v_axpy, pa_w2v_to_tiles) through the C ABI
on its own, by the rules of tests/kernel_parity.py: float64 truth, float32 torch within half the contract of it, the kernel
within max(1, 2 x float32 torch), outputs between NaN guards.  The cases, their inputs and the truths are in
tests/w2v_truth.py; tests/test_w2v_truth_cpu.py checks their admissibility and pins the truths to oracle.wav2vec2 without
a GPU.

None of these kernels ends in a max, so the poison is NaN throughout: the padding rows T .. P - 1 of every row-pitched
input, the padding columns T .. Tp - 1 of the scores, and a block in front of and behind every input.  A read of any of
them shows in the output.  Where a kernel must leave rows alone they hold NaN afterwards, bit for bit what was there.

The arithmetic of the kernels is what it was before their launchers were exported; what changed is that the launchers
now refuse the arguments the refusal tests of each section pass (groups = 0 used to be a host division by zero in
pa_w2v_posconv, T = 0 a device division by zero in pa_w2v_softmax and pa_w2v_group_norm_gelu)."""
import ctypes as C

import pytest
import torch

import w2v_truth as T
from conftest import north_star_ratio
from kernel_parity import GUARD, SEED_OFFSET, Guarded, GuardedInput, assert_parity

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
_ids = dict(ids=lambda c: c["name"])


@pytest.fixture(scope="module")
def env(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    return dict(ffi=ffi, lib=ffi.load(), dev=gpu_device)


class NanInput:
    """a kernel input between two blocks of NaN"""

    def __init__(self, data, device):
        data = data.reshape(-1).float()
        host = torch.full((data.numel() + 2 * GUARD,), T.NAN)
        host[GUARD:GUARD + data.numel()] = data
        self.buf = host.to(device)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD * 4)


def _nin(env, *tensors):
    return [NanInput(t, env["dev"]) for t in tensors]


def _in_place(env, data):
    """a Guarded buffer holding `data` (NaN where data has NaN: the padding)"""
    g = Guarded(data.numel(), env["dev"])
    g.buf[GUARD:GUARD + data.numel()] = data.reshape(-1).float().to(env["dev"])
    return g


def _row_mask(B, T_, P, C_):
    """(B, P, C) boolean: the valid rows"""
    return (torch.arange(P) < T_).view(1, P, 1).expand(B, P, C_).contiguous()


def _refused(env, rc, name, *outputs):
    assert rc == 3
    with pytest.raises(ValueError, match=name):
        env["ffi"].check(rc, "refusal")
    assert all(o.untouched() for o in outputs), f"{name}: refused, yet something was written"


# ---------------------------------------------------------------------------------------------------------------------
# pa_w2v_conv0
# ---------------------------------------------------------------------------------------------------------------------
def _conv0(env, wav_in, case, P, w, bias, tag):
    ffi, lib = env["ffi"], env["lib"]
    B, T_, C_ = case["B"], case["T"], case["C"]
    out = Guarded(B * P * C_, env["dev"])
    w_in, b_in = _nin(env, w, torch.zeros(1) if bias is None else bias)
    ffi.check(lib.pa_w2v_conv0(wav_in.ptr, case["wav_len"], case["step"], B, case["N"], T_, P, C_, case["K0"], case["S0"],
                               w_in.ptr, None if bias is None else b_in.ptr, out.ptr, ffi.stream()), tag)
    got = out.check(None, tag).view(B, P, C_)          # every row below P is written, nothing from row B * P on is
    assert bool((got[:, T_:] == 0).all()), f"{tag}: rows T .. P - 1 are not zero"
    return got[:, :T_]


@pytest.mark.parametrize("case", T.CONV0_CASES, **_ids)
def test_conv0(env, case):
    """K0 = 10 / S0 = 5 and away from it (16 / 16, 1 / 1, K0 > S0, K0 < S0), C above 256, T below 32, no multiple of 32
    and of many blocks, chunks overlapping and running off the waveform (poison behind it, inside the allocation), P == T
    and P = T + 9, with and without bias.  Then the one-tap weights (channel c: tap c % K0, value 1, no bias): the samples
    themselves, bit for bit."""
    wav, w, bias = T.conv0_input(case, 100 + SEED_OFFSET)
    wav_in = GuardedInput(wav, env["dev"], behind=case["end"] - case["wav_len"] + GUARD)
    for pad in T.CONV0_PADS:
        for b in (bias, None):
            tag = f"w2v_conv0_{case['name']}_pad{pad}_bias{int(b is not None)}"
            got = _conv0(env, wav_in, case, case["T"] + pad, w, b, tag)
            assert_parity(tag, got, T.conv0(wav, case, w, b, F64), T.conv0(wav, case, w, b, F32))
    w1, tap = T.conv0_exact_weights(case)
    tag = f"w2v_conv0_{case['name']}_exact"
    got = _conv0(env, wav_in, case, case["T"] + 9, w1, None, tag)
    want = T.conv0_exact(wav, case, tap)
    north_star_ratio(tag, got, want)
    assert torch.equal(got, want), f"{tag}: the one-tap weights do not return the samples bit for bit"


def test_conv0_refusals(env):
    ffi, lib = env["ffi"], env["lib"]
    wav_in, w_in = GuardedInput(torch.zeros(400), env["dev"]), NanInput(torch.zeros(64 * 17), env["dev"])
    out = Guarded(64 * 100, env["dev"])

    def run(N=400, T_=79, P=79, C_=64, K0=10, S0=5, B=1):
        return lib.pa_w2v_conv0(wav_in.ptr, 400, 400, B, N, T_, P, C_, K0, S0, w_in.ptr, None, out.ptr, ffi.stream())
    for kw in (dict(K0=17), dict(S0=17), dict(K0=0), dict(S0=0), dict(T_=0, P=0), dict(P=78), dict(C_=0)):
        _refused(env, run(**kw), "pa_w2v_conv0", out)
    assert run(B=0) == 0 and out.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# pa_w2v_group_norm_gelu
# ---------------------------------------------------------------------------------------------------------------------
def _group_norm(env, case, x, gamma, beta, tag):
    """-> y (B, T, C), mean (B, C), rstd (B, C) of the kernel; the padding rows hold NaN before and are asserted to hold
    it afterwards"""
    ffi, lib = env["ffi"], env["lib"]
    B, T_, P, C_ = case["B"], case["T"], case["P"], case["C"]
    buf = _in_place(env, T.pad_rows(x, P))
    mean, rstd = Guarded(B * C_, env["dev"]), Guarded(B * C_, env["dev"])
    g_in, b_in = _nin(env, gamma, beta)
    ffi.check(lib.pa_w2v_group_norm_gelu(buf.ptr, B, T_, P, C_, g_in.ptr, b_in.ptr, mean.ptr, rstd.ptr, ffi.stream()), tag)
    y = buf.check(_row_mask(B, T_, P, C_), tag).view(B, P, C_)[:, :T_]
    return y, mean.check(None, tag).view(B, C_), rstd.check(None, tag).view(B, C_)


@pytest.mark.parametrize("case", T.GN_CASES, **_ids)
def test_group_norm_gelu(env, case):
    """T of 499 down to 3 (a row lane without rows), C of 32 and 96 (half a 64-channel block idle) up to 512, P > T with
    NaN in the padding rows (out of the statistics, not rewritten), a channel mean of 3 against a spread of 0.1; the
    output and both scratch arrays against float64"""
    x, gamma, beta = T.gn_input(case, 200 + SEED_OFFSET)
    tag = "w2v_group_norm_" + case["name"]
    y, mean, rstd = _group_norm(env, case, x, gamma, beta, tag)
    y64, m64, r64 = T.group_norm_gelu(x, gamma, beta, F64)
    y32, m32, r32 = T.group_norm_gelu(x, gamma, beta, F32)
    assert_parity(tag, y, y64, y32)
    assert_parity(tag + "_mean", mean, m64, m32)
    assert_parity(tag + "_rstd", rstd, r64, r32)


def test_group_norm_gelu_of_one_row(env):
    """T = 1 (inadmissible by the rule, tests/w2v_truth.py): the row is its own mean, so the result is gelu(beta[c])
    whatever the row and gamma hold -- the closed form, within the contract; mean is the row bit for bit"""
    case = T.GN_ONE_ROW
    x, gamma, beta = T.gn_input(case, 200 + SEED_OFFSET)
    y, mean, rstd = _group_norm(env, case, 5.0 * x, 3.0 * gamma, beta, "w2v_group_norm_one_row")
    assert north_star_ratio("w2v_group_norm_one_row", y, T.gelu(beta.double()).expand(1, 1, -1)) <= 1.0
    assert torch.equal(mean, 5.0 * x[:, 0])
    assert north_star_ratio("w2v_group_norm_one_row_rstd", rstd, torch.full((1, case["C"]), T.EPS ** -0.5, dtype=F64)) <= 1.0


@pytest.mark.parametrize("B,T_,P,C_,kind", [(3, 49, 64, 96, "dyadic"), (2, 3, 4, 64, "dyadic"), (3, 49, 64, 96, "small"),
                                            (2, 3, 4, 64, "small")])
def test_group_norm_gelu_of_a_constant_column(env, B, T_, P, C_, kind):
    """an input constant along t gives gelu(beta[c]) for any gamma, within the contract.
    dyadic: values k / 2 up to 6 in size -- every partial sum of T of them and their mean are exact in float32, so the
    centred value is 0 whatever gamma is (up to 50 here, of both signs).
    small: random values.  What the contract can ask of float32 there: the mean of T equal values v is off by an ulp or
    two of v, and rstd = 1 / sqrt(eps) = 316 multiplies that, so atol 1e-5 admits |v gamma| up to about
    1e-5 / (316 * 1.2e-7) = 0.26 -- the offset-against-spread limit of tests/w2v_truth.py at its extreme.  Hence values
    of level 0.02 with gamma in [1, 2] (|v gamma| below 0.16 at four standard deviations).
    assert_parity checks that float32 torch agrees that the inputs are admissible."""
    g = torch.Generator().manual_seed(250 + SEED_OFFSET)
    if kind == "dyadic":
        col = ((torch.arange(B * C_) % 25 - 12) * 0.5).view(B, 1, C_)
        gamma = (1.0 + 49.0 * torch.rand(C_, generator=g)) * torch.where(torch.arange(C_) % 2 == 0, 1.0, -1.0)
    else:
        col = 0.02 * torch.randn(B, 1, C_, generator=g)
        gamma = 1.0 + torch.rand(C_, generator=g)
    x = col.expand(B, T_, C_).contiguous()
    beta = 0.3 * torch.randn(C_, generator=g)
    tag = f"w2v_group_norm_constant_{kind}_T{T_}_C{C_}"
    y, _, _ = _group_norm(env, dict(B=B, T=T_, P=P, C=C_), x, gamma, beta, tag)
    assert_parity(tag, y, T.gelu(beta.double()).expand(B, T_, C_), T.group_norm_gelu(x, gamma, beta, F32)[0])


def test_group_norm_gelu_refusals(env):
    ffi, lib = env["ffi"], env["lib"]
    buf = _in_place(env, torch.zeros(2 * 8 * 64))
    mean, rstd = Guarded(128, env["dev"]), Guarded(128, env["dev"])
    g_in, b_in = _nin(env, torch.ones(64), torch.zeros(64))
    before = buf.buf.clone()

    def run(B=2, T_=8, P=8, C_=64):
        return lib.pa_w2v_group_norm_gelu(buf.ptr, B, T_, P, C_, g_in.ptr, b_in.ptr, mean.ptr, rstd.ptr, ffi.stream())
    for kw in (dict(T_=0), dict(T_=8, P=7), dict(C_=0), dict(T_=-1, P=8)):
        _refused(env, run(**kw), "pa_w2v_group_norm_gelu", mean, rstd)
    assert run(B=0) == 0 and mean.untouched() and rstd.untouched()
    torch.cuda.synchronize()
    assert torch.equal(buf.buf.cpu().view(torch.int32), before.cpu().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# pa_w2v_layernorm
# ---------------------------------------------------------------------------------------------------------------------
def _layernorm(env, x, gamma, beta, with_gelu, in_place, tag):
    ffi, lib = env["ffi"], env["lib"]
    g_in, b_in = _nin(env, gamma, beta)
    if in_place:
        out = _in_place(env, x)
        src = out.ptr
    else:
        out, x_in = Guarded(x.numel(), env["dev"]), NanInput(x, env["dev"])
        src = x_in.ptr
    ffi.check(lib.pa_w2v_layernorm(src, out.ptr, x.shape[0], x.shape[1], g_in.ptr, b_in.ptr, int(with_gelu),
                                   ffi.stream()), tag)
    return out.check(None, tag).view(x.shape)


@pytest.mark.parametrize("case", T.LN_CASES, **_ids)
def test_layernorm(env, case):
    """C of 32 (half a wave idle), 96, 512, 768, 1000 (no multiple of 64) and 1024 (the limit: all 16 registers of every
    lane); 1 to 37 rows (blocks of four, the last one partly filled); with and without GELU, in place and not.  Then rows
    constant over C, of values with few mantissa bits (k / 4: every partial sum and the mean are exact in float32):
    beta, bit for bit."""
    x, gamma, beta = T.ln_input(case, 300 + SEED_OFFSET)
    for with_gelu in (False, True):
        y64, y32 = T.layer_norm(x, gamma, beta, with_gelu, F64), T.layer_norm(x, gamma, beta, with_gelu, F32)
        for in_place in (False, True):
            tag = f"w2v_layernorm_{case['name']}_gelu{int(with_gelu)}_inplace{int(in_place)}"
            assert_parity(tag, _layernorm(env, x, gamma, beta, with_gelu, in_place, tag), y64, y32)
    const = ((torch.arange(case["rows"]) % 7 - 3) * 0.25).view(-1, 1).expand(case["rows"], case["C"]).contiguous()
    for in_place in (False, True):
        got = _layernorm(env, const, gamma, beta, False, in_place, "w2v_layernorm_constant")
        assert torch.equal(got, beta.expand_as(got)), f"{case['name']}: a constant row does not return beta bit for bit"


@pytest.mark.parametrize("C_", [1025, 0, -64, 2048])
def test_layernorm_refusals(env, C_):
    ffi, lib = env["ffi"], env["lib"]
    x_in, g_in, b_in = _nin(env, torch.ones(4 * 2048), torch.ones(2048), torch.zeros(2048))
    out = Guarded(4 * 2048, env["dev"])
    _refused(env, lib.pa_w2v_layernorm(x_in.ptr, out.ptr, 4, C_, g_in.ptr, b_in.ptr, 0, ffi.stream()),
             "pa_w2v_layernorm", out)
    assert lib.pa_w2v_layernorm(x_in.ptr, out.ptr, 0, 64, g_in.ptr, b_in.ptr, 0, ffi.stream()) == 0 and out.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# pa_w2v_posconv
# ---------------------------------------------------------------------------------------------------------------------
def _posconv(env, case, x, w3, bias, tag):
    """x (B, T, D) valid rows; the padding rows of the input hold NaN, those of the output are asserted to stay NaN"""
    ffi, lib = env["ffi"], env["lib"]
    B, T_, P, D = case["B"], case["T"], case["P"], case["D"]
    x_in, w_in, b_in = _nin(env, T.pad_rows(x, P), w3, bias)
    out = Guarded(B * P * D, env["dev"])
    ffi.check(lib.pa_w2v_posconv(x_in.ptr, B, T_, P, D, case["groups"], case["KW"], w_in.ptr, b_in.ptr, out.ptr,
                                 ffi.stream()), tag)
    return out.check(_row_mask(B, T_, P, D), tag).view(B, P, D)[:, :T_]


@pytest.mark.parametrize("case", T.POSCONV_CASES, **_ids)
def test_posconv(env, case):
    """WavLM's geometry (CG = 48, kernel 128), an odd kernel (no frame dropped), kernel 1, T < pad, T = 1, tile edges at
    16 / 17 and 32 / 33 rows; P > T with NaN in the padding rows and P == T with the next chunk's rows at once behind:
    both must act as zeros.  The weight is generated in the reference layout (D, CG, KW) and re-packed here, by the
    expression of SSeRiouSSPack (tests/test_w2v_truth_cpu.py).  Then all-zero weight and bias: x, bit for bit."""
    x, w, bias = T.posconv_input(case, 400 + SEED_OFFSET)
    tag = "w2v_posconv_" + case["name"]
    got = _posconv(env, case, x, T.repack_pos_weight(w, case["groups"]), bias, tag)
    assert_parity(tag, got, T.posconv(x, w, bias, case["groups"], F64), T.posconv(x, w, bias, case["groups"], F32))
    got = _posconv(env, case, x, torch.zeros(w.numel()), torch.zeros(case["D"]), tag + "_zero")
    assert torch.equal(got, x), f"{tag}: zero weight and bias do not return x bit for bit"


@pytest.mark.parametrize("case", [T.POSCONV_CASES[0], T.POSCONV_CASES[2]], **_ids)
def test_posconv_orientation(env, case):
    """one non-zero weight at [g][j][ci][co], ci != co: x + gelu(w x[t + j - pad, g CG + ci]) in channel g CG + co and x,
    bit for bit, in every other channel; the first and the last tap among them"""
    x, _, _ = T.posconv_input(case, 450 + SEED_OFFSET)
    groups, KW, CG, D = case["groups"], case["KW"], case["CG"], case["D"]
    for g, j, ci, co in ((0, 0, 1, 2), (groups - 1, KW - 1, CG - 1, 0), (1, KW // 2, 0, CG - 1), (groups - 1, 1, 3, 5)):
        w3 = torch.zeros(groups, KW, CG, CG)
        w3[g, j, ci, co] = 1.5
        tag = f"w2v_posconv_{case['name']}_single_g{g}_j{j}_ci{ci}_co{co}"
        got = _posconv(env, case, x, w3, torch.zeros(D), tag)
        args = (x, case, g, j, ci, co, 1.5)
        want = T.posconv_single_weight(*args, F64)
        assert float((want[:, :, g * CG + co] - x[:, :, g * CG + co].double()).abs().max()) > 0.1
        assert_parity(tag, got, want, T.posconv_single_weight(*args, F32))
        others = torch.arange(D) != g * CG + co
        assert torch.equal(got[:, :, others], x[:, :, others]), f"{tag}: another channel moved"


@pytest.mark.parametrize("kw", [dict(D=100, groups=3), dict(groups=0), dict(D=1024, groups=1, KW=2), dict(KW=0),
                                dict(groups=-2), dict(T_=0), dict(T_=9, P=8), dict(D=64, groups=1, KW=242)],
                         ids=lambda kw: "_".join(f"{k}{v}" for k, v in kw.items()))
def test_posconv_refusals(env, kw):
    """D % groups != 0, groups = 0 (once a host division by zero), more than 64 KiB of LDS, and the rest of the argument
    rules: error 3, a message, nothing written"""
    ffi, lib = env["ffi"], env["lib"]
    x_in, w_in, b_in = _nin(env, torch.zeros(2 * 8 * 1024), torch.zeros(4096), torch.zeros(1024))
    out = Guarded(2 * 8 * 1024, env["dev"])

    def run(B=2, T_=8, P=8, D=64, groups=2, KW=3):
        return lib.pa_w2v_posconv(x_in.ptr, B, T_, P, D, groups, KW, w_in.ptr, b_in.ptr, out.ptr, ffi.stream())
    _refused(env, run(**kw), "pa_w2v_posconv", out)
    assert run(B=0) == 0 and out.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# pa_w2v_softmax
# ---------------------------------------------------------------------------------------------------------------------
def _softmax(env, case, S, scale, tag, bias=None, xin=None, gw=None, gb=None, gc=None):
    """S (B, H, T, T) -> (B, H, T, T); the padding columns hold NaN before and are asserted to be exactly 0 afterwards,
    every row to sum to 1"""
    ffi, lib = env["ffi"], env["lib"]
    B, H, T_, Tp, P, D = case["B"], case["H"], case["T"], case["Tp"], case["P"], case["D"]
    padded = torch.full((B, H, T_, Tp), T.NAN)
    padded[..., :T_] = S
    buf = _in_place(env, padded)
    if bias is None:
        ptrs = (None,) * 5
        keep = ()
    else:
        keep = _nin(env, bias, T.pad_rows(xin, P), gw, gb, gc)
        ptrs = tuple(k.ptr for k in keep)
    ffi.check(lib.pa_w2v_softmax(buf.ptr, B, H, T_, Tp, scale, ptrs[0], ptrs[1], P, D, ptrs[2], ptrs[3], ptrs[4],
                                 ffi.stream()), tag)
    got = buf.check(None, tag).view(B, H, T_, Tp)
    assert bool((got[..., T_:] == 0).all()), f"{tag}: the padding columns are not zero"
    assert float((got.double().sum(-1) - 1).abs().max()) <= 1e-6, f"{tag}: a row does not sum to 1"
    return got[..., :T_]


@pytest.mark.parametrize("case", T.SOFTMAX_CASES, **_ids)
def test_softmax(env, case):
    """head sizes 32, 64, 96 and 128 (above 64 the gate's dot product has a second half), T of 1, 63, 64, 65 and 499, Tp no
    multiple of 32, a row count no multiple of 4; scores of scaled standard deviation 2, a row shifted by +80, a score 60
    above the rest of its row.  Gated (bias, layer input at pitch P = T + 3 with NaN padding rows, a different constant
    per head) and plain (every pointer NULL)."""
    S, scale, bias, xin, gw, gb, gc = T.softmax_input(case, 500 + SEED_OFFSET)
    tag = "w2v_softmax_gated_" + case["name"]
    got = _softmax(env, case, S, scale, tag, bias, xin, gw, gb, gc)
    assert_parity(tag, got, T.attention_softmax(S, scale, F64, bias, xin, gw, gb, gc),
                  T.attention_softmax(S, scale, F32, bias, xin, gw, gb, gc))
    tag = "w2v_softmax_plain_" + case["name"]
    got = _softmax(env, case, S, scale, tag)
    assert_parity(tag, got, T.attention_softmax(S, scale, F64), T.attention_softmax(S, scale, F32))


@pytest.mark.parametrize("kw", [dict(H=2, D=320), dict(H=3, D=64), dict(T_=0), dict(T_=9, Tp=8), dict(H=0), dict(D=0),
                                dict(gated=True, xin=False), dict(gated=True, gw=False), dict(gated=True, gb=False),
                                dict(gated=True, gc=False), dict(gated=True, P=7)],
                         ids=lambda kw: "_".join(f"{k}{v}" for k, v in kw.items()))
def test_softmax_refusals(env, kw):
    """a head size of 160, D % H != 0, T = 0 (once a device division by zero), Tp < T, and a bias without one of the
    gate's operands: error 3, a message, the scores untouched"""
    ffi, lib = env["ffi"], env["lib"]
    S = Guarded(2 * 2 * 8 * 8, env["dev"])
    bias, xin, gw, gb, gc = _nin(env, torch.zeros(2 * 8 * 8), torch.zeros(2 * 8 * 320), torch.zeros(8 * 160),
                                 torch.zeros(8), torch.ones(2))

    def run(B=2, H=2, T_=8, Tp=8, P=8, D=64, gated=False, xin_=True, gw_=True, gb_=True, gc_=True):
        return lib.pa_w2v_softmax(S.ptr, B, H, T_, Tp, 0.125, bias.ptr if gated else None,
                                  xin.ptr if gated and xin_ else None, P, D, gw.ptr if gated and gw_ else None,
                                  gb.ptr if gated and gb_ else None, gc.ptr if gated and gc_ else None, ffi.stream())
    kw = {(k + "_" if k in ("xin", "gw", "gb", "gc") else k): v for k, v in kw.items()}
    _refused(env, run(**kw), "pa_w2v_softmax", S)
    assert run(B=0) == 0 and S.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# pa_w2v_axpy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", T.AXPY_SIZES)
def test_axpy(env, n):
    """n around one block of 256 float4 and beyond four of them.  first = 1: acc is NaN before and float32(w x) after,
    bit for bit; first = 0: acc + w x (one fma) within the contract.  Nothing from element n on is written."""
    ffi, lib = env["ffi"], env["lib"]
    g = torch.Generator().manual_seed(600 + SEED_OFFSET + n)
    x, acc0, w = torch.randn(n, generator=g), torch.randn(n, generator=g), 0.37
    (x_in,) = _nin(env, x)
    acc = Guarded(n, env["dev"])
    ffi.check(lib.pa_w2v_axpy(acc.ptr, x_in.ptr, w, n, 1, ffi.stream()), "axpy")
    got = acc.check(None, f"w2v_axpy_first_n{n}")
    assert torch.equal(got, torch.tensor(w, dtype=F32) * x), "first = 1 is not float32(w * x) bit for bit"
    acc = _in_place(env, acc0)
    ffi.check(lib.pa_w2v_axpy(acc.ptr, x_in.ptr, w, n, 0, ffi.stream()), "axpy")
    tag = f"w2v_axpy_n{n}"
    assert_parity(tag, acc.check(None, tag), T.axpy(acc0, x, w, 0, F64), T.axpy(acc0, x, w, 0, F32))


def test_axpy_refusal(env):
    ffi, lib = env["ffi"], env["lib"]
    (x_in,) = _nin(env, torch.ones(8))
    acc = Guarded(8, env["dev"])
    _refused(env, lib.pa_w2v_axpy(acc.ptr, x_in.ptr, 1.0, 6, 1, ffi.stream()), "pa_w2v_axpy", acc)
    assert lib.pa_w2v_axpy(acc.ptr, x_in.ptr, 1.0, 0, 1, ffi.stream()) == 0 and acc.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# pa_w2v_to_tiles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.TILES_CASES, **_ids)
def test_to_tiles(env, case):
    """B of 1, 16, 17 and 19 (one full tile, one chunk and three chunks into the second), D above one pass of the block
    and no multiple of 64, P > T with NaN padding rows: a bit-for-bit permutation of the valid rows, exact zeros for the
    chunks B .. 16 ntiles - 1, and no NaN anywhere"""
    ffi, lib = env["ffi"], env["lib"]
    B, T_, P, D = case["B"], case["T"], case["P"], case["D"]
    g = torch.Generator().manual_seed(700 + SEED_OFFSET)
    x = torch.randn(B, T_, D, generator=g)
    (x_in,) = _nin(env, T.pad_rows(x, P))
    want = T.to_tiles(x)
    out = Guarded(want.numel(), env["dev"])
    tag = "w2v_to_tiles_" + case["name"]
    ffi.check(lib.pa_w2v_to_tiles(x_in.ptr, B, T_, P, D, out.ptr, ffi.stream()), tag)
    got = out.check(None, tag).view(want.shape)                   # (no NaN: no padding row was copied)
    assert torch.equal(got, want), f"{tag}: not the permutation of the valid rows"
    if B % 16:
        assert bool((got[-1, :, B % 16:] == 0).all())


def test_to_tiles_refusals(env):
    ffi, lib = env["ffi"], env["lib"]
    (x_in,) = _nin(env, torch.ones(2 * 4 * 32))
    out = Guarded(16 * 4 * 32, env["dev"])
    for T_, P, D in ((0, 4, 32), (4, 3, 32), (4, 4, 0)):
        _refused(env, lib.pa_w2v_to_tiles(x_in.ptr, 2, T_, P, D, out.ptr, ffi.stream()), "pa_w2v_to_tiles", out)
    assert lib.pa_w2v_to_tiles(x_in.ptr, 0, 4, 4, 32, out.ptr, ffi.stream()) == 0 and out.untouched()
