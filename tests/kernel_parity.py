"""Shared pieces of the float64 kernel parity tests (test_gemm_family_gpu, test_lstm_values_gpu, test_classifier_gpu,
test_pooling_family_gpu).

The rules every one of them follows:
  * truth is a float64 evaluation on the CPU, written out in the test;
  * a case counts only if float32 torch, doing the same operation, is itself within HALF the project's contract
    (rtol 1e-4 / atol 1e-5) of that truth -- otherwise the inputs are badly chosen and the test says so;
  * the kernel is then held to the contract, or to twice the distance of float32 torch from the truth where that is
    larger (a different summation order of the same float32 arithmetic);
  * every output lives inside a NaN-filled buffer: one guard block in front, one behind, and NaN in every gap that a
    leading dimension larger than the row leaves.  Guards and gaps are NaN afterwards, nothing written is;
  * where a kernel ends in a max (NaN would be swallowed), its inputs live between blocks of +-1e30 (GuardedInput)."""
import ctypes as C
import os

import torch

from conftest import north_star_ratio

#: PA_FUZZ_SEED_OFFSET=k shifts every seed of these modules, as in tests/test_fuzz_gpu.py
SEED_OFFSET = int(os.environ.get("PA_FUZZ_SEED_OFFSET", "0"))

GUARD = 1024            # elements of one guard block (4 KB of float32: keeps the 16-byte alignment of what follows)
U8_UNTOUCHED = 0xA5     # what an unwritten uint8 element holds (the kernels only ever write 0 / 1)


def ratio(got, want, rtol=1e-4, atol=1e-5) -> float:
    """max |got - want| / (atol + rtol |want|): the north-star ratio without the log line (NaN if anything is NaN)"""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    if got.numel() == 0:
        return 0.0
    r = (got - want).abs() / (atol + rtol * want.abs())
    return float("nan") if torch.isnan(r).any() else r.max().item()


class Guarded:
    """`n` elements of device memory between two guard blocks, everything NaN (0xA5 for integers) before the kernel
    runs.  `fill`: another value for "untouched", for outputs whose correct values include the default one (an int32
    count may be 0xA5, a max over no speaker is NaN); it must be exact in `dtype` and a value no correct result takes."""

    def __init__(self, n: int, device, dtype=torch.float32, fill=None):
        self.n, self.dtype, self.fill = int(n), dtype, fill
        if fill is None:
            fill = float("nan") if dtype.is_floating_point else U8_UNTOUCHED
        self.buf = torch.full((self.n + 2 * GUARD,), fill, dtype=dtype, device=device)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def _untouched(self, t):
        if self.fill is not None:
            return t == self.fill
        return torch.isnan(t) if self.dtype.is_floating_point else t == U8_UNTOUCHED

    def check(self, written=None, what=""):
        """the `n` inner elements on the CPU, after asserting: both guards untouched, every element outside the boolean
        mask `written` (None = all of them) untouched, no NaN (no untouched byte) inside it"""
        torch.cuda.synchronize()
        host = self.buf.cpu()
        inner = host[GUARD:GUARD + self.n]
        assert bool(self._untouched(host[:GUARD]).all()), f"{what}: guard block in front of the output overwritten"
        assert bool(self._untouched(host[GUARD + self.n:]).all()), f"{what}: guard block behind the output overwritten"
        if written is not None:
            written = written.reshape(-1)
            assert bool(self._untouched(inner[~written]).all()), f"{what}: a gap of the output was written"
            assert not bool(self._untouched(inner[written]).any()), f"{what}: NaN / unwritten element in the output"
        else:
            assert not bool(self._untouched(inner).any()), f"{what}: NaN / unwritten element in the output"
        return inner

    def untouched(self) -> bool:
        torch.cuda.synchronize()
        return bool(self._untouched(self.buf.cpu()).all())


class GuardedInput:
    """A kernel INPUT between two blocks of large finite values of alternating sign (+-1e30).  NaN would not do here:
    the front-end kernels end in fmaxf, and fmaxf(NaN, x) is x, so NaN around an input hides an over-read instead of
    showing it; 1e30 of either sign survives |.|, max and a leaky ReLU of either branch.  `behind`: elements of poison
    behind the data (at least one guard block; more where a kernel is told of samples that lie behind the end of the
    buffer and must take them as zeros -- the poison stays inside the allocation)."""
    POISON = 1e30

    def __init__(self, data, device, behind: int = GUARD):
        data = data.reshape(-1).float()
        self.n, behind = data.numel(), max(int(behind), GUARD)
        host = torch.full((GUARD + self.n + behind,), self.POISON)
        host[1::2] = -self.POISON
        host[GUARD:GUARD + self.n] = data
        self.buf = host.to(device)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())


def assert_parity(name, got, truth64, ref32, limit=1.0):
    """admissibility of the case first (float32 torch within half the contract of the float64 truth), then the kernel:
    north-star ratio <= max(limit, 2 x that of float32 torch).  Returns the kernel's ratio."""
    r32 = north_star_ratio(name + "__float32_torch", ref32, truth64)      # (logged next to the kernel's own line)
    assert r32 <= 0.5, (f"{name}: inadmissible case -- float32 torch is itself {r32:.3f} of the contract away from the "
                        "float64 truth: choose other inputs")
    r = north_star_ratio(name, got, truth64)
    assert r <= max(limit, 2.0 * r32), f"{name}: kernel {r:.3f}, float32 torch {r32:.3f} of the contract"
    return r


def dptr(t):
    """device pointer of a tensor, or NULL"""
    return None if t is None else C.c_void_p(t.data_ptr())
