"""Every entry point of the SincNet front end (csrc/seg_frontend.hip: pa_row_stats, pa_sinc_fir_pool at all eight built
strides, pa_sinc_fir_span + pa_sinc_fix_pool, pa_conv5_pool for 80 and 60 input channels, pa_norm_transpose) through the
C ABI on its own, by the rules of tests/kernel_parity.py: float64 truth, float32 torch within half the contract of it,
the kernel within max(1, 2 x float32 torch), outputs between NaN guards, inputs between blocks of +-1e30.  The cases,
their inputs and the truths are in tests/seg_frontend_truth.py; tests/test_seg_frontend_truth_cpu.py checks their
admissibility without a GPU.  Each kernel gets inputs of its own (means, rstds, gammas chosen by the case), so a failure
names one kernel.

The shared sinc pair is held to the float64 PER-CHUNK layer (normalise, filter, magnitude, pool), never to its own
formula.  With the formula on the raw span (before the span was re-centred by chunk 0's mean) the DC family measured, on
an MI355X, 0.73 (DC 0.05 / std 0.02), 3.49 and 1.95 (0.1 / 0.01 at 160 000 and 80 000 samples), 9.01 and 6.19 (0.1 / 0.003),
37.5 (constant chunk), 4.68 and 2.05 (stepped) of the contract; now 0.05 to 0.39 (profiles/seg_frontend_parity.txt)."""
import pytest
import torch

import seg_frontend_truth as T
from conftest import north_star_ratio
from kernel_parity import GUARD, SEED_OFFSET, Guarded, GuardedInput, assert_parity

pytestmark = pytest.mark.gpu

_ids = dict(ids=lambda c: c["name"])


@pytest.fixture(scope="module")
def env(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    from oracle import seeded_pyannet
    from pyannote_audio_amd.weights import SegmentationPack
    model = seeded_pyannet(seed=1234, num_layers=4)
    pack = SegmentationPack(model.state_dict(), {"lstm": {"num_layers": 4}}, 7, 3, 2, gpu_device)
    taps, gamma, beta = T.model_sinc()
    assert torch.equal(taps, pack.sinc_taps)
    assert (gamma, beta) == (pack.struct.wav_gamma, pack.struct.wav_beta)
    exact = GuardedInput(T.sinc_image(T.exact_taps()), gpu_device)
    return dict(ffi=ffi, lib=ffi.load(), dev=gpu_device, pack=pack, taps=taps, gamma=gamma, beta=beta, exact=exact)


def _gin(env, *tensors, behind=GUARD):
    return [GuardedInput(t, env["dev"], behind) for t in tensors]


# ---------------------------------------------------------------------------------------------------------------------
# pa_row_stats
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.ROW_STATS_CASES, **_ids)
def test_row_stats(env, case):
    """mean AND rstd of the zero-extended row against float64 mean / biased variance: lengths around the block size and
    160 000, row_stride <, ==, > len, a last row cut by total_len, rows wholly behind it (mean 0, rstd 1 / sqrt(eps)),
    constant rows, DC offsets of 1, 1e2 and 1e4 times the spread"""
    ffi, lib = env["ffi"], env["lib"]
    x = T.row_stats_input(case, 100 + SEED_OFFSET)
    (xin,) = _gin(env, x)
    mean, rstd = Guarded(case["rows"], env["dev"]), Guarded(case["rows"], env["dev"])
    tag = "row_stats_" + case["name"]
    ffi.check(lib.pa_row_stats(xin.ptr, case["stride"], case["total"], case["rows"], case["len"], T.EPS, mean.ptr,
                               rstd.ptr, ffi.stream()), tag)
    m64, r64 = T.row_stats(x, case, torch.float64)
    m32, r32 = T.row_stats(x, case, torch.float32)
    assert_parity(tag + "_mean", mean.check(None, tag), m64, m32)
    assert_parity(tag + "_rstd", rstd.check(None, tag), r64, r32)
    behind = torch.arange(case["rows"]) * case["stride"] >= case["total"]
    assert bool((m64[behind] == 0).all()) and bool((mean.check()[behind] == 0).all())


def test_row_stats_no_rows(env):
    ffi, lib = env["ffi"], env["lib"]
    (xin,) = _gin(env, torch.ones(8))
    mean, rstd = Guarded(1, env["dev"]), Guarded(1, env["dev"])
    assert lib.pa_row_stats(xin.ptr, 8, 8, 0, 8, T.EPS, mean.ptr, rstd.ptr, ffi.stream()) == 0
    assert mean.untouched() and rstd.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# pa_sinc_fir_pool
# ---------------------------------------------------------------------------------------------------------------------
def _sinc_fir_pool(env, wav_in, case, mean, rstd, gamma, beta, filt_ptr, tag):
    ffi, lib = env["ffi"], env["lib"]
    P = ((case["N"] - 251) // case["stride"] + 1) // 3
    out = Guarded(case["B"] * 80 * P, env["dev"])
    m, r = _gin(env, mean, rstd)
    ffi.check(lib.pa_sinc_fir_pool(wav_in.ptr, case["wav_len"], case["step"], case["B"], case["N"], case["stride"],
                                   m.ptr, r.ptr, gamma, beta, filt_ptr, out.ptr, ffi.stream()), tag)
    return out.check(None, tag).view(case["B"], 80, P)


@pytest.mark.parametrize("case", T.SINC_POOL_CASES, **_ids)
def test_sinc_fir_pool(env, case):
    """all eight built strides; P of 1, 127, 128, 129 and a full-size value, and L = 3; chunk_stride <, ==, > N (the gaps
    poisoned); the last chunk partly and wholly behind wav_len (poison behind the buffer, inside the allocation); B of
    1, 2, 3, 7.  Once with the packed filters of the seeded model against float64, once with the hand-made image (one tap
    of value 1 per filter, taps 0 and 250 among them; mean 0, rstd 1, gamma 1, beta 0): the largest |x| of the three
    positions, shifted by that tap, bit for bit."""
    wav, mean, rstd = T.sinc_pool_input(case, 200 + SEED_OFFSET)
    (wav_in,) = _gin(env, wav, behind=case["end"] - case["wav_len"] + GUARD)
    chunks = T.chunks_of(wav, case["wav_len"], case["step"], case["B"], case["N"])
    tag = "sinc_pool_" + case["name"]
    got = _sinc_fir_pool(env, wav_in, case, mean, rstd, case["gamma"], case["beta"], env["pack"].struct.sinc_filt, tag)
    args = (chunks, mean, rstd, case["gamma"], case["beta"], env["taps"], case["stride"])
    assert_parity(tag, got, T.sinc_pool_layer(*args, torch.float64), T.sinc_pool_layer(*args, torch.float32))
    one, zero = torch.ones(case["B"]), torch.zeros(case["B"])
    got = _sinc_fir_pool(env, wav_in, case, zero, one, 1.0, 0.0, env["exact"].ptr, tag + "_exact")
    want = T.sinc_pool_exact(chunks, case["stride"])
    north_star_ratio(tag + "_exact", got, want)
    assert torch.equal(got, want), f"{tag}: the one-tap image is not reproduced bit for bit"


@pytest.mark.parametrize("stride", T.SINC_STRIDES)
def test_sinc_fir_pool_without_output(env, stride):
    """N = 251: one position, no pooling window -- returns 0 and writes nothing"""
    ffi, lib = env["ffi"], env["lib"]
    wav_in, m, r = _gin(env, T.wave(2 * 251, 7), torch.zeros(2), torch.ones(2))
    out = Guarded(2 * 80, env["dev"])
    assert lib.pa_sinc_fir_pool(wav_in.ptr, 2 * 251, 251, 2, 251, stride, m.ptr, r.ptr, 1.0, 0.0,
                                env["pack"].struct.sinc_filt, out.ptr, ffi.stream()) == 0
    assert out.untouched()


@pytest.mark.parametrize("N,stride", [(250, 10), (1, 1), (16000, 3), (16000, 0), (16000, 32)])
def test_sinc_fir_pool_refusals(env, N, stride):
    """fewer samples than taps, a stride that is not built: an error, and nothing runs"""
    ffi, lib = env["ffi"], env["lib"]
    wav_in, m, r = _gin(env, T.wave(N, 7), torch.zeros(1), torch.ones(1))
    out = Guarded(80 * 6000, env["dev"])
    rc = lib.pa_sinc_fir_pool(wav_in.ptr, N, N, 1, N, stride, m.ptr, r.ptr, 1.0, 0.0, env["pack"].struct.sinc_filt,
                              out.ptr, ffi.stream())
    assert rc == 3
    with pytest.raises(ValueError, match="pa_sinc_fir_pool"):
        ffi.check(rc, "refusal")
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# pa_sinc_fir_span + pa_sinc_fix_pool
# ---------------------------------------------------------------------------------------------------------------------
def _span_pair(env, case, filt_ptr, taps, gamma, beta, wav, mean, rstd, tag, centred=True):
    """-> S (80, Pc) and the pooled output (B, 80, P) of the re-centred pair as pa_seg_forward calls it (centred=False:
    of the pair on the raw span); the tap sums are checked on the way (one float32 rounding of the float64 sum of the
    unpacked taps)"""
    ffi, lib, dev = env["ffi"], env["lib"], env["dev"]
    B, N, span = case["B"], case["N"], case["span"]
    Pc, P = (span - 251) // 10 + 1, ((N - 251) // 10 + 1) // 3
    wav_in, m, r = _gin(env, wav, mean, rstd, behind=span - case["wav_len"] + GUARD)
    Sg = Guarded(80 * Pc, dev)
    if centred:
        ffi.check(lib.pa_sinc_fir_span_centred(wav_in.ptr, case["wav_len"], span, m.ptr, r.ptr, filt_ptr, Sg.ptr,
                                               ffi.stream()), tag)
    else:
        ffi.check(lib.pa_sinc_fir_span(wav_in.ptr, case["wav_len"], span, filt_ptr, Sg.ptr, ffi.stream()), tag)
    S = Sg.check(None, tag + "_S").view(80, Pc)
    # (the fix-up reads S out of a poisoned buffer of its own: NaN guards would be swallowed by its fmaxf)
    (S_in,) = _gin(env, S)
    sums, out = Guarded(80, dev), Guarded(B * 80 * P, dev)
    if centred:
        ffi.check(lib.pa_sinc_fix_pool_centred(S_in.ptr, Pc, case["step"] // 10, B, P, wav_in.ptr, case["wav_len"], N,
                                               m.ptr, r.ptr, gamma, beta, filt_ptr, sums.ptr, out.ptr, ffi.stream()), tag)
    else:
        ffi.check(lib.pa_sinc_fix_pool(S_in.ptr, Pc, case["step"] // 10, B, P, m.ptr, r.ptr, gamma, beta, filt_ptr,
                                       sums.ptr, out.ptr, ffi.stream()), tag)
    if P == 0:
        assert sums.untouched() and out.untouched()
        return S, None
    s1, s1_64 = sums.check(None, tag + "_tapsum"), taps.double().sum(-1)
    assert_parity(tag + "_tapsum", s1, s1_64, taps.sum(-1))
    assert bool(((s1.double() - s1_64).abs() <= 2.0 ** -23 * s1_64.abs()).all()), f"{tag}: tap sums beyond one ulp"
    return S, out.check(None, tag).view(B, 80, P)


def _span_case(env, case, seed):
    gamma, beta = (env["gamma"], env["beta"]) if case["gamma"] is None else (case["gamma"], case["beta"])
    wav, mean, rstd = T.span_input(case, seed)
    tag = "span_" + case["name"]
    S, got = _span_pair(env, case, env["pack"].struct.sinc_filt, env["taps"], gamma, beta, wav, mean, rstd, tag)
    m0 = T.span_centre(mean, rstd)
    raw = (wav, case["wav_len"], case["span"], m0, env["taps"])
    assert_parity(tag + "_S", S, T.span_raw(*raw, torch.float64), T.span_raw(*raw, torch.float32))
    if got is None:
        return None
    chunks = T.chunks_of(wav, case["wav_len"], case["step"], case["B"], case["N"])
    args = (chunks, mean, rstd, gamma, beta, env["taps"], 10)
    assert_parity(tag + "_pool", got, T.sinc_pool_layer(*args, torch.float64), T.sinc_pool_layer(*args, torch.float32))
    # a chunk the device-side rule hands back is the per-chunk kernel's, bit for bit
    (wav_in,) = _gin(env, wav, behind=case["span"] - case["wav_len"] + GUARD)
    per_chunk = _sinc_fir_pool(env, wav_in, dict(case, stride=10), mean, rstd, gamma, beta,
                               env["pack"].struct.sinc_filt, tag + "_per_chunk")
    d = T.demoted(mean, rstd, m0)
    assert torch.equal(got[d], per_chunk[d]), f"{tag}: a demoted chunk is not the per-chunk kernel's"
    return d, m0


@pytest.mark.parametrize("case", T.SPAN_CASES, **_ids)
def test_shared_sinc_pair(env, case):
    """Pc of 1 (no pooled output: nothing written), 127, 128, 129 and a 7-chunk span; wav_len shorter than the span;
    Q = 3, 100, 800, 1 600; gammas of both signs and a beta, so that every term of the fix-up counts; the tap sums.
    These spans have no offset worth the name (|mean_0| rstd_0 <= 0.5): the re-centred pair must then be the pair on the
    raw span (pa_sinc_fir_span + pa_sinc_fix_pool), bit for bit, and that pair is held to the same truth."""
    done = _span_case(env, case, 300 + SEED_OFFSET)
    gamma, beta = case["gamma"], case["beta"]
    wav, mean, rstd = T.span_input(case, 300 + SEED_OFFSET)
    tag = "span_raw_" + case["name"]
    S_c, got_c = _span_pair(env, case, env["pack"].struct.sinc_filt, env["taps"], gamma, beta, wav, mean, rstd, tag)
    S_r, got_r = _span_pair(env, case, env["pack"].struct.sinc_filt, env["taps"], gamma, beta, wav, mean, rstd, tag,
                            centred=False)
    if done is None:                             # (Pc = 1: 257 samples, re-centred, no pooled output)
        assert got_c is None and got_r is None
        return
    d, m0 = done
    assert m0 == 0 and not bool(d.any())
    assert torch.equal(S_c, S_r)
    assert torch.equal(got_c, got_r), f"{tag}: without an offset the re-centred pair is not the raw one"
    chunks = T.chunks_of(wav, case["wav_len"], case["step"], case["B"], case["N"])
    args = (chunks, mean, rstd, gamma, beta, env["taps"], 10)
    assert_parity(tag + "_pool", got_r, T.sinc_pool_layer(*args, torch.float64), T.sinc_pool_layer(*args, torch.float32))


def test_shared_sinc_pair_exact_image(env):
    """the hand-made image through the pair: tap sums exactly 1, S the shifted samples minus m0"""
    case = T.SPAN_CASES[4]
    wav, mean, rstd = T.span_input(case, 300 + SEED_OFFSET)
    S, got = _span_pair(env, case, env["exact"].ptr, T.exact_taps(), 1.0, 0.0, wav, mean, rstd, "span_exact_image")
    x = T.rows_of(wav, case["wav_len"], 0, 1, case["span"])[0] - T.span_centre(mean, rstd)
    want = x[10 * torch.arange(S.shape[1]).view(1, -1) + T.exact_tap_positions().view(-1, 1)]
    assert torch.equal(S, want)
    assert got is not None


@pytest.mark.parametrize("case", T.DC_CASES, **_ids)
def test_shared_sinc_pair_dc_family(env, case):
    """quiet recordings with a DC offset, DC / std from 0.2 to 33 and the constant chunk, N of 32 000, 80 000, 160 000:
    against the float64 per-chunk layer.  Every span but the one at DC / std = 0.2 is re-centred; no chunk is handed
    back to the per-chunk kernel here."""
    d, m0 = _span_case(env, case, 300 + SEED_OFFSET)
    assert not bool(d.any())
    assert (m0 == 0) == (case["std"] > 0 and case["dc"] / case["std"] < 0.5)


@pytest.mark.parametrize("case", T.STEP_CASES, **_ids)
def test_shared_sinc_pair_stepped_dc(env, case):
    """the offset steps in the middle of the span, so chunk means differ from m0.  A step of a fifth of the spread: every
    chunk is fixed up.  A step of two spreads: the chunks further than half their standard deviation from m0 are the
    per-chunk kernel's (asserted bit for bit in _span_case), chunk 0 is not among them."""
    d, m0 = _span_case(env, case, 300 + SEED_OFFSET)
    assert m0 != 0
    if case is T.STEP_CASES[0]:
        assert not bool(d.any())
    else:
        assert bool(d.any()) and not bool(d[0])


# ---------------------------------------------------------------------------------------------------------------------
# pa_conv5_pool
# ---------------------------------------------------------------------------------------------------------------------
def _conv5(env, x, mean, rstd, gamma, beta, weight, bias, tag):
    ffi, lib = env["ffi"], env["lib"]
    B, cin, Lin = x.shape
    P = (Lin - 4) // 3
    bias64 = torch.zeros(64)
    bias64[:60] = bias
    xin, m, r, g, b, w, bb = _gin(env, x, mean, rstd, gamma, beta, T.conv5_image(weight), bias64)
    out = Guarded(B * 60 * P, env["dev"])
    ffi.check(lib.pa_conv5_pool(xin.ptr, B, cin, Lin, m.ptr, r.ptr, g.ptr, b.ptr, w.ptr, bb.ptr, out.ptr,
                                ffi.stream()), tag)
    return out.check(None, tag).view(B, 60, P)


@pytest.mark.parametrize("case", T.CONV5_CASES, **_ids)
def test_conv5_pool(env, case):
    """80 and 60 input channels; P of 1, 31, 32, 33 and the production lengths; B of 1, 2, 3, 37; gammas of both signs
    (both sides of the leaky ReLU and of the max); neighbouring rows 1e3 .. 1e6 apart in scale; a constant row with
    rstd = 1 / sqrt(1e-5).  Then one weight of value 1 per output channel with mean 0, rstd 1, gamma 1, beta 0: the
    largest leaky ReLU of the three positions plus the bias, bit for bit."""
    args = T.conv5_input(case, 500 + SEED_OFFSET)
    tag = "conv5_pool_" + case["name"]
    got = _conv5(env, *args, tag)
    assert_parity(tag, got, T.conv5_pool(*args, torch.float64), T.conv5_pool(*args, torch.float32))
    x, cin = args[0], case["cin"]
    R = x.shape[0] * cin
    w, c, t = T.conv5_exact_weights(cin)
    got = _conv5(env, x, torch.zeros(R), torch.ones(R), torch.ones(cin), torch.zeros(cin), w, args[6], tag + "_exact")
    want = T.conv5_pool_exact(x, c, t, args[6])
    north_star_ratio(tag + "_exact", got, want)
    assert torch.equal(got, want), f"{tag}: the one-weight image is not reproduced bit for bit"


@pytest.mark.parametrize("cin,Lin,rc", [(80, 6, 0), (60, 6, 0), (80, 4, 0), (64, 100, 3), (0, 100, 3)])
def test_conv5_pool_without_output_and_refusals(env, cin, Lin, rc):
    """Lin = 6: no pooling window, returns 0 and writes nothing; a channel count that is not built: an error"""
    ffi, lib = env["ffi"], env["lib"]
    ins = _gin(env, torch.ones(2 * 80 * 100), torch.zeros(160), torch.ones(160), torch.ones(80), torch.zeros(80),
               torch.zeros(64 * 400), torch.zeros(64))
    out = Guarded(2 * 60 * 32, env["dev"])
    assert lib.pa_conv5_pool(ins[0].ptr, 2, cin, Lin, *(i.ptr for i in ins[1:]), out.ptr, ffi.stream()) == rc
    if rc:
        with pytest.raises(ValueError, match="pa_conv5_pool"):
            ffi.check(rc, "refusal")
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# pa_norm_transpose
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.NORM_T_CASES, **_ids)
def test_norm_transpose(env, case):
    """B of 1, 15, 16, 17, 37 and T of 1, 63, 64, 65, 589: every element of the ntiles x T x 16 x 64 block is written,
    the guards are not; channels 60 .. 63 and the chunks from B on are exactly zero"""
    ffi, lib = env["ffi"], env["lib"]
    args = T.norm_transpose_input(case, 600 + SEED_OFFSET)
    B, Tn = case["B"], case["T"]
    ntiles = (B + 15) // 16
    ins = _gin(env, *args)
    out = Guarded(ntiles * Tn * 16 * 64, env["dev"])
    tag = "norm_transpose_" + case["name"]
    ffi.check(lib.pa_norm_transpose(ins[0].ptr, B, Tn, *(i.ptr for i in ins[1:]), out.ptr, ffi.stream()), tag)
    got = out.check(None, tag).view(ntiles, Tn, 16, 64)
    assert_parity(tag, got, T.norm_transpose(*args, torch.float64), T.norm_transpose(*args, torch.float32))
    assert bool((got[..., 60:] == 0).all())
    by_chunk = got.permute(0, 2, 1, 3).reshape(ntiles * 16, Tn, 64)
    assert bool((by_chunk[B:] == 0).all())


def test_norm_transpose_no_chunks(env):
    ffi, lib = env["ffi"], env["lib"]
    ins = _gin(env, torch.ones(60), torch.zeros(60), torch.ones(60), torch.ones(60), torch.zeros(60))
    out = Guarded(16 * 64, env["dev"])
    assert lib.pa_norm_transpose(ins[0].ptr, 0, 1, *(i.ptr for i in ins[1:]), out.ptr, ffi.stream()) == 0
    assert out.untouched()
