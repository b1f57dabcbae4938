"""Extended-precision truths for the float64 kernels of csrc/vbx.hip: the PLDA projection (core/plda.py:47-60 over
utils/vbx.py:205-217) and ONE iteration of VBx (utils/vbx.py:106-133; Landini et al., "Bayesian HMM clustering of
x-vector sequences (VBx)...", equation numbers as in oracle/vbx.py), restated in plain numpy on np.longdouble.

A float64 kernel cannot be judged by a float64 reference: both carry the same 1.1e-16 of rounding per operation and
differ only in summation order.  np.longdouble on x86-64 is the 80-bit x87 type (64-bit mantissa, eps 1.08e-19), three
decimal digits more than the thing under test; numpy evaluates sqrt / log / exp / arctan of it with the C library's
long-double functions and its matrix product with a plain longdouble loop (no BLAS).  Every constant (2 pi, the 1e-8 of
log(pi + eps)) is built from longdouble arithmetic; the float64 INPUTS (fea, Phi, Fa, Fb, gamma) convert exactly.

Written from the formulas, not from the kernels: nothing here knows how vbx.hip splits its sums."""
import functools

import numpy as np

LD = np.longdouble

# A platform whose long double is float64 (MSVC, some ARM ABIs) would silently turn the truth into the thing under test.
assert np.finfo(LD).eps < 2e-19, (
    f"np.longdouble has eps {np.finfo(LD).eps:.3e} here: it is not an extended-precision type, and the truths of "
    "tests/vbx_truth.py would be no better than the float64 kernels they judge")

TWO_PI = LD(8) * np.arctan(LD(1))
PI_FLOOR = LD(1) / LD(10) ** 8            # the eps of log(pi + eps), utils/vbx.py:118


#: the float contract of this path, as tests/test_vbx_gpu.py asserts it against the oracle
GAMMA_RTOL, GAMMA_ATOL = 1e-9, 1e-12      # responsibilities, element-wise
ELBO_RTOL = 1e-9                          # |d ELBO| <= 1e-9 |ELBO|
PLDA_RTOL = 1e-11                         # max |d fea| <= 1e-11 max |fea|


def _ld(a):
    return np.asarray(a, dtype=LD)


def gamma_ratio(got, truth) -> float:
    """max |got - truth| / (atol + rtol |truth|), the difference taken in longdouble (NaN if anything is NaN)"""
    got, truth = _ld(got), _ld(truth)
    return float(np.max(np.abs(got - truth) / (GAMMA_ATOL + GAMMA_RTOL * np.abs(truth)))) if truth.size else 0.0


def elbo_ratio(got, truth) -> float:
    return float(np.abs(LD(got) - LD(truth)) / (ELBO_RTOL * np.abs(LD(truth))))


def plda_ratio(got, truth) -> float:
    got, truth = _ld(got), _ld(truth)
    return float(np.max(np.abs(got - truth)) / (PLDA_RTOL * np.max(np.abs(truth))))


def assert_admissible(name, ratio_numpy):
    """a case counts only if float64 numpy (the oracle's arithmetic) is itself within HALF the contract of the truth"""
    assert ratio_numpy <= 0.5, (f"{name}: inadmissible case -- float64 numpy is itself {ratio_numpy:.3e} of the "
                                "contract away from the longdouble truth: choose other inputs")


def vbx_iteration_numpy(fea, Phi, Fa, Fb, gamma_in, first):
    """the same single iteration in the oracle's float64 arithmetic (oracle/vbx.py, one pass of its loop)"""
    from oracle.vbx import vbx
    gamma_in = np.asarray(gamma_in, dtype=np.float64)
    S = gamma_in.shape[1]
    Nk = gamma_in.sum(axis=0)
    gamma, _, Li = vbx(np.asarray(fea, dtype=np.float64), np.asarray(Phi, dtype=np.float64), Fa=Fa, Fb=Fb,
                       pi=S if first else Nk / Nk.sum(), gamma=gamma_in, maxIters=1)
    return gamma, Li[0][0]


def softmax_onehot(labels, S, smoothing=7.0):
    """cluster_vbx's initialisation (utils/vbx.py:143-147): softmax(smoothing * one-hot), float64"""
    q = np.zeros((len(labels), S))
    q[np.arange(len(labels)), labels] = smoothing
    q = np.exp(q - q.max(axis=1, keepdims=True))
    return q / q.sum(axis=1, keepdims=True)


def vbx_inputs(N, S, D, seed, scale=1.0):
    """-> fea (N, D), Phi (D,) decreasing in (0.05, 6), gamma0 (N, S): `S` speaker centres two noise deviations apart,
    frames drawn around them, the initial responsibilities from labels that are RANDOM (not the true ones)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((S, D))
    who = rng.integers(0, S, N)
    fea = (centres[who] * 2.0 + rng.standard_normal((N, D))) * scale
    Phi = np.sort(rng.uniform(0.05, 6.0, D))[::-1].copy()
    return fea, Phi, softmax_onehot(rng.integers(0, S, N), S)


def dead_speaker_gamma(gamma):
    """`gamma` (N, S), every entry positive, with its LAST column exactly zero (a dead speaker: Nk = 0, pi = 0 ->
    log(1e-8), invL = 1, alpha = 0), rows renormalised over the rest, and row 0 one-hot.  With S = 1 there is no
    speaker to lose: the (already one-hot) rows are returned as they are."""
    g = np.array(gamma, dtype=np.float64)
    if g.shape[1] > 1:
        g[:, -1] = 0.0
        g /= g.sum(axis=1, keepdims=True)
    g[0] = 0.0
    g[0, 0] = 1.0
    return g


def _l2(m):
    return m / np.sqrt(np.sum(m * m, axis=1, keepdims=True))


def plda_truth(X_f32, mean1, lda, mean2, mu, trT):
    """x-vectors (n, DIN) float32 -> PLDA space (n, DOUT) longdouble:
    y = sqrt(DMID) l2(lda^T (sqrt(DIN) l2(x - mean1)) - mean2);  fea = (y - mu) trT, trT (DMID, DOUT) = tr[:DOUT]^T"""
    X, mean1, lda, mean2, mu, trT = (_ld(a) for a in (X_f32, mean1, lda, mean2, mu, trT))
    din, dmid = lda.shape
    x = np.sqrt(LD(din)) * _l2(X - mean1)
    y = np.sqrt(LD(dmid)) * _l2(x @ lda - mean2)
    return (y - mu) @ trT


def vbx_iteration_truth(fea, Phi, Fa, Fb, gamma_in, first):
    """One VB iteration from the responsibilities `gamma_in` (N, S): -> (gamma_out (N, S), ELBO), longdouble.
    `first`: the speaker priors are uniform (the first iteration of cluster_vbx), else pi = Nk / sum Nk -- what the
    previous iteration's `pi = gamma.sum(0) / gamma.sum()` hands on."""
    X, Phi, gamma = _ld(fea), _ld(Phi), _ld(gamma_in)
    Fa, Fb = LD(Fa), LD(Fb)
    N, D = X.shape
    S = gamma.shape[1]
    G = -(np.sum(X * X, axis=1) + D * np.log(TWO_PI)) / 2                   # constant term of (23)
    rho = X * np.sqrt(Phi)                                                   # (18)
    Nk = gamma.sum(axis=0)
    pi = np.full(S, LD(1) / LD(S)) if first else Nk / Nk.sum()
    invL = 1 / (1 + Fa / Fb * Nk[:, None] * Phi[None, :])                    # (17), (S, D)
    alpha = Fa / Fb * invL * (gamma.T @ rho)                                 # (16), (S, D)
    log_p = Fa * (rho @ alpha.T - ((invL + alpha * alpha) @ Phi)[None, :] / 2 + G[:, None])   # (23), (N, S)
    score = log_p + np.log(pi + PI_FLOOR)[None, :]
    top = score.max(axis=1)
    log_px = top + np.log(np.exp(score - top[:, None]).sum(axis=1))          # logsumexp by max-subtraction
    gamma_out = np.exp(score - log_px[:, None])
    elbo = log_px.sum() + Fb / 2 * np.sum(np.log(invL) - invL - alpha * alpha + 1)   # (25)
    return gamma_out, elbo


#: (N, S, D) of the kernel parity cases (tests/test_vbx_kernels_gpu.py) and why each is there
VBX_SHAPES = [
    (1, 1, 1), (2, 1, 3), (3, 2, 5), (7, 3, 128),      # empty first half of the M step's row split, unroll tail only,
                                                       # D < 128, S = 1
    (257, 5, 129), (1030, 7, 300), (4100, 12, 128),    # D one past 128 / past 256 (both stride loops), halves of N
                                                       # that are no multiple of 4, several rows per thread in Nk
    (600, 300, 128),                                   # S > 256: strided S loops, the D + S layout of the E step
    (2700, 9, 128),                                    # the shape the pipeline test reaches
]
#: the default of the pipeline and both corners of Fa / Fb over Uniform(0.01, 0.5) x Uniform(0.01, 15)
FA_FB = [(0.07, 0.8), (0.5, 0.01), (0.01, 15.0)]
#: large-score case: Fa G < -700 for every frame, exp() of a raw score underflows for every speaker
LARGE_SCORE = dict(N=257, S=5, D=300, Fa=0.5, Fb=0.8, scale=6.0)


@functools.lru_cache(maxsize=None)
def vbx_steps(N, S, D, Fa, Fb, seed, scale=1.0):
    """The calls of one parity case: -> fea, Phi, [(tag, first, gamma_in, (truth gamma, truth ELBO), (numpy gamma,
    numpy ELBO))].  Every gamma_in is CHOSEN (the truth's output rounded to float64, never the kernel's), so that
    errors do not chain (computed once per case and shared: leave the arrays unchanged):
      first  first = 1 from softmax(7 one-hot(random labels)): uniform priors, rho / G derived from fea
      next   first = 0 from the truth's responsibilities: non-uniform priors, rho / G reused
      dead   first = 0 with an exactly-zero column and a one-hot row"""
    fea, Phi, gamma0 = vbx_inputs(N, S, D, seed, scale)
    steps, gamma_in = [], gamma0
    for tag, first in (("first", 1), ("next", 0), ("dead", 0)):
        if tag == "dead":
            gamma_in = dead_speaker_gamma(gamma0)
        truth = vbx_iteration_truth(fea, Phi, Fa, Fb, gamma_in, first)
        steps.append((tag, first, gamma_in, truth, vbx_iteration_numpy(fea, Phi, Fa, Fb, gamma_in, first)))
        gamma_in = truth[0].astype(np.float64)
    return fea, Phi, steps
