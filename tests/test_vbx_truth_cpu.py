"""Pins tests/vbx_truth.py (the longdouble truths that tests/test_vbx_kernels_gpu.py holds csrc/vbx.hip to) without a
GPU: against the oracle (oracle/vbx.py) over a whole chained run, against a case small enough to write out by hand
(evaluated a second time with mpmath at 50 digits), and against properties that the mathematics guarantees.  It also
runs, on the CPU, the admissibility half of every GPU parity case -- float64 numpy within half the contract of the
truth -- so that a badly chosen input is found here and not on a GPU."""
import os

import numpy as np
import pytest

from vbx_truth import (ELBO_RTOL, FA_FB, GAMMA_ATOL, GAMMA_RTOL, LARGE_SCORE, LD, VBX_SHAPES, assert_admissible,
                       elbo_ratio, gamma_ratio, plda_ratio, plda_truth, softmax_onehot, vbx_inputs,
                       vbx_iteration_numpy, vbx_iteration_truth, vbx_steps)

EPS_LD = float(np.finfo(LD).eps)


def _chain(fea, Phi, Fa, Fb, gamma0, iterations):
    """`iterations` truths in a row, gamma_in = the previous gamma_out rounded to float64 (what a float64 buffer holds)
    -> list of (gamma longdouble, ELBO)"""
    out, gamma = [], gamma0
    for it in range(iterations):
        g, e = vbx_iteration_truth(fea, Phi, Fa, Fb, gamma, first=it == 0)
        out.append((g, e))
        gamma = g.astype(np.float64)
    return out


@pytest.mark.parametrize("N,S,D,Fa,Fb,seed", [(300, 6, 128, 0.07, 0.8, 0), (200, 4, 40, 0.4, 0.05, 1),
                                              (150, 5, 64, 0.02, 12.0, 2)])
def test_chained_truth_reproduces_the_oracle(N, S, D, Fa, Fb, seed):
    """oracle.vbx.vbx from cluster_vbx's initialisation: responsibilities, priors and the whole ELBO list, within the
    contract (gamma rtol 1e-9 / atol 1e-12, ELBO 1e-9 relative); the ELBO of the chained truths does not decrease by
    more than 1e-6 (the 1e-8 of log(pi + eps) makes the bound approximately, not exactly, monotone)."""
    from oracle.vbx import vbx
    fea, Phi, gamma0 = vbx_inputs(N, S, D, seed)
    gamma, pi, Li = vbx(fea, Phi, Fa=Fa, Fb=Fb, pi=S, gamma=gamma0, maxIters=20)
    assert len(Li) >= 3, "the run is too short to pin a chain: choose other inputs"
    chain = _chain(fea, Phi, Fa, Fb, gamma0, len(Li))
    for it, ((_, elbo), (want,)) in enumerate(zip(chain, Li)):
        assert elbo_ratio(want, elbo) <= 1.0, f"ELBO of iteration {it}: oracle {want!r}, truth {elbo!r}"
    last = chain[-1][0]
    assert gamma_ratio(gamma, last) <= 1.0
    prior = last.sum(axis=0) / last.sum()
    assert float(np.max(np.abs(pi - prior) / (GAMMA_ATOL + GAMMA_RTOL * prior))) <= 1.0
    elbos = [e for _, e in chain]
    assert all(b - a >= -1e-6 for a, b in zip(elbos, elbos[1:])), [float(e) for e in elbos]


def test_plda_truth_reproduces_the_oracle(tmp_path):
    from oracle.vbx import PLDA, synth_plda
    d = synth_plda(str(tmp_path))
    ref = PLDA(os.path.join(d, "xvec_transform.npz"), os.path.join(d, "plda.npz"))
    x = np.random.default_rng(0).standard_normal((40, 256)).astype(np.float32)
    truth = plda_truth(x, ref.mean1, ref.lda, ref.mean2, ref.plda_mu, ref.plda_tr[:128].T)
    assert truth.dtype == LD and truth.shape == (40, 128)
    assert plda_ratio(ref(x), truth) <= 1.0


def test_one_frame_one_speaker_one_dimension_by_hand():
    """x = 3/2, Phi = 2, Fa = 1/2, Fb = 2, gamma_in = 1, uniform prior (pi = 1):
        Fa / Fb = 1/4;  invL = 1 / (1 + 1/4 * 1 * 2) = 2/3;  rho = 3/2 sqrt 2;
        alpha = 1/4 * 2/3 * 3/2 sqrt 2 = sqrt 2 / 4, alpha^2 = 1/8;  rho alpha = 3/4;
        log p = 1/2 (3/4 - 1/2 (2/3 + 1/8) 2 - 1/2 (9/4 + log 2 pi)) = -7/12 - 1/4 log 2 pi;
        log p(x) = log p + log(1 + 1e-8), gamma = exp(0) = 1 exactly;
        ELBO = log p(x) + Fb / 2 (log 2/3 - 2/3 - 1/8 + 1) = -3/8 - 1/4 log 2 pi + log(1 + 1e-8) + log 2/3"""
    import mpmath
    gamma, elbo = vbx_iteration_truth(np.array([[1.5]]), np.array([2.0]), 0.5, 2.0, np.array([[1.0]]), first=True)
    assert gamma.shape == (1, 1) and gamma[0, 0] == 1
    with mpmath.workdps(50):
        want = (-mpmath.mpf(3) / 8 - mpmath.log(2 * mpmath.pi) / 4 + mpmath.log1p(mpmath.mpf(10) ** -8)
                + mpmath.log(mpmath.mpf(2) / 3))
        got = mpmath.mpf(np.format_float_scientific(elbo, precision=25, unique=False))
        assert abs(got - want) <= 8 * EPS_LD * abs(want), (got, want)
    # the same from the second iteration on: pi = Nk / Nk = 1
    again = vbx_iteration_truth(np.array([[1.5]]), np.array([2.0]), 0.5, 2.0, np.array([[1.0]]), first=False)
    assert again[0][0, 0] == 1 and again[1] == elbo


@pytest.mark.parametrize("first", [True, False])
def test_two_identical_speakers_share_every_frame(first):
    """identical columns of gamma_in give identical models and scores: the two responsibilities of a frame are equal
    bit for bit, and 1/2 up to the rounding of score - log p(x) (eps |score|, |score| < 10 at D = 8: 1e-18)"""
    fea, Phi, _ = vbx_inputs(60, 2, 8, 3)
    column = np.random.default_rng(3).uniform(0.1, 0.9, 60)
    gamma, _ = vbx_iteration_truth(fea, Phi, 0.07, 0.8, np.stack([column, column], axis=1), first)
    assert np.array_equal(gamma[:, 0], gamma[:, 1])
    assert float(np.max(np.abs(gamma - LD(1) / 2))) <= 1e-18


def test_rows_sum_to_one():
    """within 1e-18.  A responsibility is exp(score - log p(x)), and the rounding of a score is eps |score|: the bound
    needs |score| of order 1, so D = 8 and the default Fa = 0.07 (|score| < 10) -- the rows of the D = 128 parity
    cases, |score| up to 1e5, sum to 1 within 1.4e-17."""
    fea, Phi, gamma0 = vbx_inputs(50, 4, 8, 5)
    for first in (True, False):
        gamma, _ = vbx_iteration_truth(fea, Phi, 0.07, 0.8, gamma0, first)
        assert float(np.max(np.abs(gamma.sum(axis=1) - 1))) <= 1e-18


def test_permuting_speakers_permutes_the_responsibilities():
    """and leaves the ELBO alone.  Only the ORDER of sums over speakers changes: N + S D = 1100 terms reordered move
    the ELBO by at most 1100 eps relative, 2e-16 to be safe; an element of gamma sees the reordered sum of log p(x)
    only, 5 terms."""
    fea, Phi, gamma0 = vbx_inputs(300, 5, 160, 6)
    perm = np.array([3, 0, 4, 1, 2])
    gamma, elbo = vbx_iteration_truth(fea, Phi, 0.07, 0.8, gamma0, first=False)
    gamma_p, elbo_p = vbx_iteration_truth(fea, Phi, 0.07, 0.8, gamma0[:, perm], first=False)
    assert float(np.abs(elbo_p - elbo)) <= 2e-16 * float(np.abs(elbo))
    assert float(np.max(np.abs(gamma_p - gamma[:, perm]) / (1e-30 + np.abs(gamma_p)))) <= 1e-15
    assert not np.array_equal(gamma_p, gamma), "the permutation moved nothing: the check is empty"


@pytest.mark.parametrize("N,S,D", VBX_SHAPES)
def test_gpu_parity_cases_are_admissible(N, S, D):
    """float64 numpy within half the contract of the truth, for every call of every kernel parity case"""
    for j, (Fa, Fb) in enumerate(FA_FB):
        _, _, steps = vbx_steps(N, S, D, Fa, Fb, 100 * VBX_SHAPES.index((N, S, D)) + j)
        for tag, _, gamma_in, (tg, te), (ng, ne) in steps:
            name = f"vbx[{N},{S},{D}|Fa={Fa},Fb={Fb}|{tag}]"
            assert_admissible(name + " gamma", gamma_ratio(ng, tg))
            assert_admissible(name + " ELBO", elbo_ratio(ne, te))
            if tag == "dead" and S > 1:
                assert not gamma_in[:, -1].any() and gamma_in[0, 0] == 1.0 and gamma_in[0].sum() == 1.0


def test_large_score_case_is_large_and_admissible():
    k = LARGE_SCORE
    fea, _, steps = vbx_steps(k["N"], k["S"], k["D"], k["Fa"], k["Fb"], 77, k["scale"])
    G = -0.5 * ((fea ** 2).sum(axis=1) + k["D"] * np.log(2 * np.pi))
    assert (k["Fa"] * G).max() < -700.0, "exp() of a raw score would not underflow: choose other inputs"
    for tag, _, _, (tg, te), (ng, ne) in steps:
        assert_admissible(f"vbx large scores {tag} gamma", gamma_ratio(ng, tg))
        assert_admissible(f"vbx large scores {tag} ELBO", elbo_ratio(ne, te))


def test_an_ill_conditioned_input_is_refused():
    """two speakers 1e-8 apart on features a thousand times too large: scores of 1e8 whose DIFFERENCE decides gamma.
    float64 numpy is then ten contracts away from the truth, and the rule must say so instead of letting a kernel
    pass at twice that distance."""
    fea, Phi, _ = vbx_inputs(40, 2, 64, 5, scale=1000.0)
    d = 1e-8 * np.random.default_rng(1).standard_normal(40)
    gamma_in = np.stack([0.5 + d, 0.5 - d], axis=1)
    truth, _ = vbx_iteration_truth(fea, Phi, 0.5, 0.8, gamma_in, first=True)
    got, _ = vbx_iteration_numpy(fea, Phi, 0.5, 0.8, gamma_in, first=True)
    with pytest.raises(AssertionError, match="choose other inputs"):
        assert_admissible("ill-conditioned", gamma_ratio(got, truth))


def test_driver_cases_stop_off_the_knife_edge(tmp_path):
    """tests/test_vbx_gpu.py asserts that the driver stops after as many iterations as the oracle.  That is a fair
    demand only where the stop is not decided by rounding: no consecutive ELBO difference of the oracle within 1e-8 of
    the 1e-4 threshold, and the new hyper-parameter rows not trivial (more than two iterations)."""
    from oracle.vbx import PLDA, synth_plda
    from test_vbx_gpu import CASES, DEFAULT_PARAMS, _embeddings, oracle_elbos
    d = synth_plda(str(tmp_path))
    plda = PLDA(os.path.join(d, "xvec_transform.npz"), os.path.join(d, "plda.npz"))
    assert sorted((kw["params"]["Fa"], kw["params"]["Fb"]) for *_, kw in CASES if "params" in kw) == [
        (0.02, 12.0), (0.4, 0.05)]
    for C, K, noise, seed, kw in CASES:
        emb, seg = _embeddings(C, K, noise, seed)
        elbos = oracle_elbos(emb, seg, plda, **kw.get("params", DEFAULT_PARAMS))
        steps = np.diff(elbos)
        assert len(elbos) > 2 and np.abs(steps - 1e-4).min() > 1e-8, (C, K, seed, elbos)


def test_contract_is_the_one_of_the_pipeline_test():
    assert (GAMMA_RTOL, GAMMA_ATOL, ELBO_RTOL) == (1e-9, 1e-12, 1e-9)
    q = softmax_onehot(np.array([1, 0]), 3)
    assert np.allclose(q.sum(axis=1), 1.0) and q[0, 1] == q[1, 0] > 0.99 and q[0, 0] == q[0, 2]
