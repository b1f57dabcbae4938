"""Admissibility of every value case of tests/test_seg_frontend_gpu.py, checked where no GPU is needed: float32 torch,
doing the same operation, is within HALF the contract (rtol 1e-4 / atol 1e-5) of the float64 truth -- exactly what
kernel_parity.assert_parity demands on the GPU machine before it looks at the kernel.  A badly chosen case is found
here, not there.  The module also keeps the reason for the re-centred shared sinc layer on record in executable form:
a float32 emulation of the formula the kernels had before leaves the contract at DC 0.1 / std 0.01, the re-centred one
does not.  Nothing here says anything about a kernel."""
import pytest
import torch

import seg_frontend_truth as T
from kernel_parity import SEED_OFFSET, ratio

HALF = 0.5


def _admissible(name, ref32, truth64):
    r = ratio(ref32, truth64)
    print(f"{name}: float32 torch {r:.3f} of the contract")
    assert r <= HALF, f"{name}: inadmissible case -- float32 torch is {r:.3f} of the contract away from float64"


def test_the_two_packers_agree():
    from pyannote_audio_amd.weights import _mfma_b_image
    taps, _, _ = T.model_sinc()
    assert torch.equal(T.sinc_image(taps), _mfma_b_image(torch.nn.functional.pad(taps, (0, 1)), 5))
    image = T.sinc_image(T.exact_taps()).view(5, 63, 64)
    assert image.sum() == 80 and bool((image[:, 62, 48:] == 0).all())          # index 251 is padding


@pytest.mark.parametrize("case", T.ROW_STATS_CASES, ids=lambda c: c["name"])
def test_row_stats_cases_are_admissible(case):
    x = T.row_stats_input(case, 100 + SEED_OFFSET)
    m64, r64 = T.row_stats(x, case, torch.float64)
    m32, r32 = T.row_stats(x, case, torch.float32)
    assert bool((m64.abs() < 1e6).all()), "a row reads the poison"
    _admissible("row_stats_mean_" + case["name"], m32, m64)
    _admissible("row_stats_rstd_" + case["name"], r32, r64)


@pytest.mark.parametrize("case", T.SINC_POOL_CASES, ids=lambda c: c["name"])
def test_sinc_pool_cases_are_admissible(case):
    taps, _, _ = T.model_sinc()
    wav, mean, rstd = T.sinc_pool_input(case, 200 + SEED_OFFSET)
    chunks = T.chunks_of(wav, case["wav_len"], case["step"], case["B"], case["N"])
    assert bool((chunks.abs() < 10).all()), "a chunk reads the poison"
    args = (chunks, mean, rstd, case["gamma"], case["beta"], taps, case["stride"])
    truth = T.sinc_pool_layer(*args, torch.float64)
    assert truth.shape[-1] == ((case["N"] - 251) // case["stride"] + 1) // 3 >= 1
    _admissible("sinc_pool_" + case["name"], T.sinc_pool_layer(*args, torch.float32), truth)
    # the exact image: the float64 layer with the hand-made taps IS the gather
    one, zero = torch.ones(case["B"]), torch.zeros(case["B"])
    exact = T.sinc_pool_layer(chunks, zero, one, 1.0, 0.0, T.exact_taps(), case["stride"], torch.float64)
    assert torch.equal(exact.float(), T.sinc_pool_exact(chunks, case["stride"]))


def _span_truths(case, seed, m0_is_chunk0=True):
    taps, gamma, beta = T.model_sinc()
    gamma, beta = (gamma, beta) if case["gamma"] is None else (case["gamma"], case["beta"])
    wav, mean, rstd = T.span_input(case, seed)
    chunks = T.chunks_of(wav, case["wav_len"], case["step"], case["B"], case["N"])
    args = (chunks, mean, rstd, gamma, beta, taps, 10)
    return wav, mean, rstd, gamma, beta, taps, T.sinc_pool_layer(*args, torch.float64), \
        T.sinc_pool_layer(*args, torch.float32)


@pytest.mark.parametrize("case", T.SPAN_CASES + T.DC_CASES + T.STEP_CASES, ids=lambda c: c["name"])
def test_span_cases_are_admissible(case):
    wav, mean, rstd, gamma, beta, taps, truth, ref32 = _span_truths(case, 300 + SEED_OFFSET)
    m0 = T.span_centre(mean, rstd)
    _admissible("span_S_" + case["name"], T.span_raw(wav, case["wav_len"], case["span"], m0, taps, torch.float32),
                T.span_raw(wav, case["wav_len"], case["span"], m0, taps, torch.float64))
    if truth.shape[-1]:
        _admissible("span_pool_" + case["name"], ref32, truth)


def test_dc_family_is_complete():
    """none of the issue's DC family up to DC / std of about 30 is missing, the constant chunk is there, and the stepped
    spans make chunk means differ: the small step keeps every chunk, the large one demotes some"""
    have = {(c["N"], c["dc"], c["std"]) for c in T.DC_CASES}
    assert have >= set(T.DC_FAMILY) and (160000, 0.5, 0.0) in have
    assert {round(dc / std, 1) for _, dc, std in T.DC_FAMILY if std} >= {0.2, 2.5, 10.0, 33.3}
    assert {n for n, _, _ in T.DC_FAMILY} == {32000, 80000, 160000}
    small, large = (T.span_input(c, 300 + SEED_OFFSET) for c in T.STEP_CASES)
    assert T.span_centre(*small[1:]) == small[1][0] and T.span_centre(*large[1:]) == large[1][0]
    assert not bool(T.demoted(small[1], small[2], small[1][0]).any())
    d = T.demoted(large[1], large[2], large[1][0])
    assert bool(d.any()) and not bool(d[0])
    for c in T.DC_CASES:
        _, mean, rstd = T.span_input(c, 300 + SEED_OFFSET)
        m0 = T.span_centre(mean, rstd)
        assert (m0 == 0) == (c["std"] > 0 and c["dc"] / c["std"] < 0.5), c["name"]      # only DC / std = 0.2 stays raw
        assert not bool(T.demoted(mean, rstd, m0).any()), c["name"]
    for c in T.SPAN_CASES[1:]:                   # the ordinary spans keep the arithmetic of the raw span
        _, mean, rstd = T.span_input(c, 300 + SEED_OFFSET)
        assert T.span_centre(mean, rstd) == 0 and not bool(T.demoted(mean, rstd, torch.zeros(())).any()), c["name"]


@pytest.mark.parametrize("seed", [0, 1])
def test_float32_emulation_of_the_shared_formula(seed):
    """DC 0.1 / std 0.01, 4 chunks of 160 000: the formula on the raw span is outside the contract in float32, the
    per-chunk layer and the re-centred formula are inside"""
    case = T._span("emulation", 4, 160000, 16000, dc=0.1, std=0.01, tone=0.0)
    wav, mean, rstd, gamma, beta, taps, truth, ref32 = _span_truths(case, 400 + seed + SEED_OFFSET)
    args = (wav, case["wav_len"], case["step"], case["B"], case["N"], mean, rstd, gamma, beta, taps)
    raw, centred = ratio(T.shared_formula_f32(*args), truth), ratio(T.shared_formula_f32(*args, m0=mean[0]), truth)
    print(f"per chunk {ratio(ref32, truth):.2f}, shared on the raw span {raw:.2f}, re-centred {centred:.2f}")
    assert ratio(ref32, truth) <= HALF
    assert raw > 1.0
    assert centred <= 1.0


@pytest.mark.parametrize("case", T.CONV5_CASES, ids=lambda c: c["name"])
def test_conv5_cases_are_admissible(case):
    args = T.conv5_input(case, 500 + SEED_OFFSET)
    truth = T.conv5_pool(*args, torch.float64)
    assert truth.shape == (case["B"], 60, case["P"]) and case["P"] >= 1
    _admissible("conv5_pool_" + case["name"], T.conv5_pool(*args, torch.float32), truth)
    # both sides of the leaky ReLU are taken
    x, mean, rstd, gamma, beta = args[:5]
    pre = (x - mean.view(x.shape[0], -1, 1)) * (rstd.view(x.shape[0], -1) * gamma[None])[:, :, None] + beta[None, :, None]
    assert bool((pre > 0).any()) and bool((pre < 0).any()) and bool((gamma > 0).any()) and bool((gamma < 0).any())
    w, c, t = T.conv5_exact_weights(case["cin"])
    R = x.shape[0] * case["cin"]
    exact = T.conv5_pool(x, torch.zeros(R), torch.ones(R), torch.ones(case["cin"]), torch.zeros(case["cin"]), w,
                         args[6], torch.float32)
    assert torch.equal(exact, T.conv5_pool_exact(x, c, t, args[6]))


@pytest.mark.parametrize("case", T.NORM_T_CASES, ids=lambda c: c["name"])
def test_norm_transpose_cases_are_admissible(case):
    args = T.norm_transpose_input(case, 600 + SEED_OFFSET)
    truth = T.norm_transpose(*args, torch.float64)
    assert truth.shape == ((case["B"] + 15) // 16, case["T"], 16, 64)
    _admissible("norm_transpose_" + case["name"], T.norm_transpose(*args, torch.float32), truth)
