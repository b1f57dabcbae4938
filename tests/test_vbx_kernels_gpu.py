"""The five float64 kernels of csrc/vbx.hip (k_plda_transform, k_vbx_prepare, k_vbx_mstep, k_vbx_estep, k_vbx_elbo)
through their own entry points, pa_plda_transform and pa_vbx_iteration, against the longdouble truths of
tests/vbx_truth.py -- one iteration at a time, at the sizes where the index arithmetic changes (D past 128 and 256, S
past 256, halves of N that are no multiple of 4, N = 1) and at the default and both corners of Fa / Fb.

Rules as in tests/kernel_parity.py, one precision up:
  * the truth is np.longdouble (80-bit) on the CPU, pinned without a GPU by tests/test_vbx_truth_cpu.py;
  * the contract is the one tests/test_vbx_gpu.py asserts for this path: responsibilities at rtol 1e-9 / atol 1e-12,
    |d ELBO| <= 1e-9 |ELBO|, PLDA features within 1e-11 max |fea|;
  * a case counts only if float64 numpy (the oracle's arithmetic) is itself within HALF the contract of the truth;
    the kernel is held to the contract, or to twice numpy's distance where that is larger;
  * gamma, the ELBO and the PLDA features live in NaN-guarded buffers, the workspace between 0xA5 guards and NaN-filled
    before the first call: nothing may depend on what it held, nothing is written outside its declared size;
  * every gamma_in is chosen (the truth's output rounded to float64), so that errors do not chain.
Every ratio goes to the suite's parity log with %.3e (numpy sits at 1e-4 of the contract and below)."""
import numpy as np
import pytest
import torch

from conftest import report
from kernel_parity import GUARD, SEED_OFFSET, U8_UNTOUCHED, Guarded, dptr
from vbx_truth import (FA_FB, LARGE_SCORE, VBX_SHAPES, assert_admissible, elbo_ratio, gamma_ratio, plda_ratio,
                       plda_truth, vbx_inputs, vbx_steps)

pytestmark = pytest.mark.gpu


def _log(name, value):
    """one figure into the suite's parity log, through conftest.report: `value` against 0, so that its max_abs column
    is the figure itself, printed with %.3e"""
    report(name, torch.tensor([value], dtype=torch.float64), torch.zeros(1, dtype=torch.float64))


def assert_parity64(name, kernel, numpy64):
    """`kernel`, `numpy64`: distances from the longdouble truth in units of the contract, both logged.  Admissibility
    of the case first, then the kernel: <= max(1, 2 x float64 numpy)."""
    _log(name + " kernel / contract", kernel)
    _log(name + " float64 numpy / contract", numpy64)
    assert_admissible(name, numpy64)
    assert kernel <= max(1.0, 2.0 * numpy64), (f"{name}: kernel {kernel:.3e}, float64 numpy {numpy64:.3e} of the "
                                               "contract")


class GuardedWorkspace:
    """`nbytes` of device memory between two blocks of 0xA5 bytes, NaN (as doubles) inside"""

    def __init__(self, nbytes: int, device):
        self.nbytes = int(nbytes)
        self.g = Guarded(self.nbytes, device, dtype=torch.uint8)
        self.g.buf[GUARD:GUARD + self.nbytes - self.nbytes % 8].view(torch.float64).fill_(float("nan"))
        self.before = self.g.buf.clone()

    @property
    def ptr(self):
        return self.g.ptr

    def guards_intact(self) -> bool:
        torch.cuda.synchronize()
        host = self.g.buf.cpu()
        return bool((host[:GUARD] == U8_UNTOUCHED).all()) and bool((host[GUARD + self.nbytes:] == U8_UNTOUCHED).all())

    def unchanged(self) -> bool:
        torch.cuda.synchronize()
        return torch.equal(self.g.buf, self.before)


class _Iteration:
    """device buffers of one problem and the call itself"""

    def __init__(self, fea, Phi, S, device, workspace_bytes=None):
        import pyannote_audio_amd.ffi as ffi
        self.ffi, self.lib = ffi, ffi.load()
        self.N, self.D, self.S = fea.shape[0], fea.shape[1], S
        self.fea = torch.from_numpy(np.ascontiguousarray(fea)).to(device)
        self.Phi = torch.from_numpy(np.ascontiguousarray(Phi)).to(device)
        self.gamma = Guarded(self.N * S, device, dtype=torch.float64)
        self.elbo = Guarded(1, device, dtype=torch.float64)
        need = self.lib.pa_vbx_workspace_bytes(self.N, S, self.D)
        self.ws = GuardedWorkspace(need if workspace_bytes is None else workspace_bytes, device)

    def set_gamma(self, gamma_in):
        self.gamma.buf[GUARD:GUARD + self.N * self.S] = torch.from_numpy(
            np.ascontiguousarray(gamma_in, dtype=np.float64)).reshape(-1).to(self.gamma.buf.device)

    def call(self, Fa, Fb, first, n=None, s=None) -> int:
        self.elbo.buf[GUARD] = float("nan")
        return self.lib.pa_vbx_iteration(dptr(self.fea), dptr(self.Phi), self.N if n is None else n,
                                         self.S if s is None else s, self.D, float(Fa), float(Fb), int(first),
                                         self.gamma.ptr, self.elbo.ptr, self.ws.ptr, self.ws.nbytes, self.ffi.stream())

    def result(self, what):
        """(gamma (N, S) float64, ELBO) after asserting: guards of all three buffers intact, no NaN in gamma / ELBO"""
        gamma = self.gamma.check(what=what + " gamma").numpy().reshape(self.N, self.S)
        elbo = float(self.elbo.check(what=what + " ELBO")[0])
        assert self.ws.guards_intact(), f"{what}: written outside the declared {self.ws.nbytes} bytes of workspace"
        return gamma, elbo


def _run_steps(name, it, steps, Fa, Fb):
    for tag, first, gamma_in, (truth_gamma, truth_elbo), (np_gamma, np_elbo) in steps:
        what = f"{name}|{tag}]"
        it.set_gamma(gamma_in)
        it.ffi.check(it.call(Fa, Fb, first), what)
        gamma, elbo = it.result(what)
        assert_parity64(what + " gamma", gamma_ratio(gamma, truth_gamma), gamma_ratio(np_gamma, truth_gamma))
        assert_parity64(what + " ELBO", elbo_ratio(elbo, truth_elbo), elbo_ratio(np_elbo, truth_elbo))
        rows = float(np.max(np.abs(gamma.astype(np.longdouble).sum(axis=1) - 1)))
        assert rows <= 1e-12, f"{what}: a row of gamma sums to 1 +- {rows:.3e}"
        assert gamma.max(axis=1).min() > 0.0, f"{what}: an all-zero row of gamma"


@pytest.mark.parametrize("Fa,Fb", FA_FB)
@pytest.mark.parametrize("N,S,D", VBX_SHAPES)
def test_vbx_iteration_matches_truth(gpu_device, N, S, D, Fa, Fb):
    """first = 1 from softmax(7 one-hot(random labels)); first = 0 from the truth's responsibilities (non-uniform
    priors, rho / G reused from the workspace); first = 0 with a dead speaker (an exactly-zero column: Nk = 0, pi = 0
    -> log(1e-8), invL = 1, alpha = 0) and a one-hot row."""
    seed = 100 * VBX_SHAPES.index((N, S, D)) + FA_FB.index((Fa, Fb)) + SEED_OFFSET
    fea, Phi, steps = vbx_steps(N, S, D, Fa, Fb, seed)
    _run_steps(f"vbx[{N},{S},{D}|Fa={Fa},Fb={Fb}", _Iteration(fea, Phi, S, gpu_device), steps, Fa, Fb)


def test_vbx_iteration_large_scores(gpu_device):
    """Fa G < -700 for every frame (D = 300, features times 6, Fa = 0.5; asserted by tests/test_vbx_truth_cpu.py, where
    float64 numpy is measured at 8e-4 of the contract): exp() of a raw score underflows for EVERY speaker, and only
    the subtraction of the row maximum keeps gamma from 0 / 0."""
    k = LARGE_SCORE
    fea, Phi, steps = vbx_steps(k["N"], k["S"], k["D"], k["Fa"], k["Fb"], 77 + SEED_OFFSET, k["scale"])
    G = -0.5 * ((fea ** 2).sum(axis=1) + k["D"] * np.log(2 * np.pi))
    assert (k["Fa"] * G).max() < -700.0
    _run_steps("vbx[large scores", _Iteration(fea, Phi, k["S"], gpu_device), steps, k["Fa"], k["Fb"])


@pytest.mark.parametrize("N,S,D", [(4100, 12, 128), (600, 300, 128)])
def test_vbx_iteration_is_bit_reproducible(gpu_device, N, S, D):
    """fixed reduction trees, no atomics: the same first = 1 / first = 0 pair from identical inputs, in fresh buffers,
    gives the same bits"""
    fea, Phi, gamma0 = vbx_inputs(N, S, D, 5 + SEED_OFFSET)
    runs = []
    for _ in range(2):
        it, out = _Iteration(fea, Phi, S, gpu_device), []
        it.set_gamma(gamma0)
        for first in (1, 0):
            it.ffi.check(it.call(0.07, 0.8, first), "pa_vbx_iteration")
            it.result(f"vbx reproducibility [{N},{S},{D}] first={first}")
            out += [it.gamma.buf.clone(), it.elbo.buf.clone()]
        runs.append(out)
    for a, b in zip(*runs):
        assert not torch.isnan(a[GUARD:-GUARD]).any() and torch.equal(a[GUARD:-GUARD], b[GUARD:-GUARD])


# ---------------------------------------------------------------------------------------------------------------------
# pa_plda_transform

def _plda_inputs(n, DIN, DMID, DOUT, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, DIN)).astype(np.float32)
    lda = rng.standard_normal((DIN, DMID)) / np.sqrt(DIN)
    mean1, mean2, mu = (0.05 * rng.standard_normal(k) for k in (DIN, DMID, DMID))
    trT = np.ascontiguousarray((rng.standard_normal((DMID, DMID)) / np.sqrt(DMID) + np.eye(DMID))[:, :DOUT])
    return X, mean1, lda, mean2, mu, trT


def _plda_numpy(X, mean1, lda, mean2, mu, trT):
    """oracle.vbx.PLDA.__call__ on these parameters (the object is filled in without the .npz files)"""
    from oracle.vbx import PLDA
    ref = object.__new__(PLDA)
    ref.mean1, ref.lda, ref.mean2, ref.plda_mu = mean1, lda, mean2, mu
    ref.plda_tr, ref.lda_dimension = trT.T, trT.shape[1]
    return ref(X)


def _plda_kernel(device, X, mean1, lda, mean2, mu, trT, dims=None):
    """-> (return code, Guarded output); `dims` = (n, DIN, DMID, DOUT) overrides what the arrays say"""
    import pyannote_audio_amd.ffi as ffi
    n, DIN, DMID, DOUT = dims or (X.shape[0], lda.shape[0], lda.shape[1], trT.shape[1])
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (X, mean1, lda, mean2, mu, trT)]
    out = Guarded(max(n, X.shape[0]) * DOUT, device, dtype=torch.float64)
    rc = ffi.load().pa_plda_transform(dptr(dev[0]), n, DIN, DMID, DOUT, dptr(dev[1]), dptr(dev[2]), dptr(dev[3]),
                                      dptr(dev[4]), dptr(dev[5]), out.ptr, ffi.stream())
    torch.cuda.synchronize()
    return rc, out


PLDA_SHAPES = [(700, 256, 128, 128),    # the production shape
               (5, 256, 128, 64),       # DOUT < DMID
               (3, 300, 130, 130),      # strides past 256 (DIN) and 128 (DMID, DOUT)
               (1, 8, 4, 2),            # DIN below a wavefront
               (9, 512, 300, 7)]        # DMID past 256


@pytest.mark.parametrize("n,DIN,DMID,DOUT", PLDA_SHAPES)
def test_plda_transform_matches_truth(gpu_device, n, DIN, DMID, DOUT):
    import pyannote_audio_amd.ffi as ffi
    args = _plda_inputs(n, DIN, DMID, DOUT, 10 + PLDA_SHAPES.index((n, DIN, DMID, DOUT)) + SEED_OFFSET)
    truth = plda_truth(*args)
    rc, out = _plda_kernel(gpu_device, *args)
    ffi.check(rc, "pa_plda_transform")
    name = f"plda[{n},{DIN},{DMID},{DOUT}]"
    got = out.check(what=name).numpy().reshape(n, DOUT)
    assert_parity64(name, plda_ratio(got, truth), plda_ratio(_plda_numpy(*args), truth))


def test_plda_transform_nan_row_stays_in_its_row(gpu_device):
    """one NaN element of X poisons both L2 norms of ITS row: that row of fea is NaN throughout, and every other row has
    the bits it has without the NaN (one workgroup per embedding, nothing shared)"""
    n, DIN, DMID, DOUT = 6, 256, 128, 64
    args = _plda_inputs(n, DIN, DMID, DOUT, 20 + SEED_OFFSET)
    rc, clean = _plda_kernel(gpu_device, *args)
    assert rc == 0
    X = args[0].copy()
    X[2, 77] = np.nan
    rc, out = _plda_kernel(gpu_device, X, *args[1:])
    assert rc == 0
    written = torch.ones(n, DOUT, dtype=torch.bool)
    written[2] = False
    got = out.check(written=written, what="plda with a NaN row")          # (row 2 all NaN, no NaN elsewhere)
    keep = written.reshape(-1)
    assert torch.equal(got[keep], clean.check(what="plda")[keep])


# ---------------------------------------------------------------------------------------------------------------------
# refusals and empty problems: nothing is written

def test_vbx_iteration_refusals_write_nothing(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    fea, Phi, gamma0 = vbx_inputs(40, 3, 16, 30)
    short = _Iteration(fea, Phi, 3, gpu_device, workspace_bytes=lib.pa_vbx_workspace_bytes(40, 3, 16) - 1)
    assert short.call(0.07, 0.8, 1) != 0, "a workspace one byte short was accepted"
    assert short.gamma.untouched() and short.elbo.untouched() and short.ws.unchanged()
    # D + S doubles of LDS in the E step: (128 + 8200) * 8 > 64 KiB
    S = 8200
    assert (128 + S) * 8 > 64 * 1024
    wide = _Iteration(np.zeros((1, 128)), np.ones(128), S, gpu_device)
    assert wide.call(0.07, 0.8, 1) != 0, "S = 8200 at D = 128 was accepted"
    assert wide.gamma.untouched() and wide.elbo.untouched() and wide.ws.unchanged()
    # n <= 0 or s <= 0: nothing to do, and nothing done
    for n, s in ((0, 3), (-1, 3), (40, 0), (40, -2)):
        it = _Iteration(fea, Phi, 3, gpu_device)
        assert it.call(0.07, 0.8, 1, n=n, s=s) == 0, f"n = {n}, s = {s}"
        assert it.gamma.untouched() and it.elbo.untouched() and it.ws.unchanged(), f"n = {n}, s = {s}"


def test_plda_transform_refusals_write_nothing(gpu_device):
    args = _plda_inputs(4, 32, 8, 8, 40)
    rc, out = _plda_kernel(gpu_device, *args, dims=(4, 32, 8, 9))
    assert rc != 0 and out.untouched(), "dout > dmid"
    big = _plda_inputs(1, 8000, 200, 4, 41)
    assert (8000 + 200) * 8 > 64 * 1024
    rc, out = _plda_kernel(gpu_device, *big)
    assert rc != 0 and out.untouched(), "(din + dmid) * 8 > 64 KiB"
    for n in (0, -3):
        rc, out = _plda_kernel(gpu_device, *args, dims=(n, 32, 8, 8))
        assert rc == 0 and out.untouched(), f"n = {n}"
    rc, out = _plda_kernel(gpu_device, *args)
    assert rc == 0
    out.check(what="plda after the refusals")
