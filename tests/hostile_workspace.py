"""Caller workspaces with hostile contents, for every entry point that takes one (test_hostile_workspace_gpu.py; the
audit the runs confirm is DESIGN.md, "What the launch sequences assume about their workspace").

The contract under test (include/pyannote_amd.h, "Workspaces"): a workspace's contents on entry may be anything, nothing
outside [workspace, workspace + workspace_bytes) is touched, and no output depends on the contents.  So:
  * HostileWorkspace hands out exactly the bytes the matching pa_*_workspace_bytes asked for, between two guard blocks;
  * the same call runs on a zeroed workspace (twice), on one of 0xFF bytes and on one of +-1e30 floats;
  * every output of every run must have the same BYTES, and every guard must be untouched.
Nothing here is a tolerance: the one value assertion of a case is made by the case, on the outputs of the 0xFF run."""
import ctypes as C

import torch

from kernel_parity import Guarded, GUARD as OUT_GUARD

GUARD = 2 * 4096          # bytes of one guard block: a multiple of 4096, so the inner pointer keeps the base's alignment
ALIGN = 256               # what the carvers assume of a workspace pointer (torch's device allocations give 512)
GUARD_BYTE = 0xA5
HUGE = 1e30               # kernel_parity.GuardedInput.POISON: survives |.|, max and either branch of a leaky ReLU

FILLS = ("zeros", "ones", "huge")


def fill_bytes(fill: str, n: int, device) -> torch.Tensor:
    """`n` bytes of the pattern `fill`, the pattern starting at byte 0:
         zeros  0x00
         ones   0xFF: NaN as float32 and float64, -1 at every integer width
         huge   float32 +1e30, -1e30 alternating: no fmaxf swallows it; a large positive index as int32 (1 900 671 690),
                finite nonsense (-6.8e238) as float64"""
    if fill == "zeros":
        return torch.zeros(n, dtype=torch.uint8, device=device)
    if fill == "ones":
        return torch.full((n,), 0xFF, dtype=torch.uint8, device=device)
    if fill == "huge":
        pair = torch.tensor([HUGE, -HUGE], dtype=torch.float32).view(torch.uint8).to(device)
        return pair.repeat((n + 7) // 8)[:n]
    raise ValueError(f"unknown fill {fill!r}")


class HostileWorkspace:
    """`need` bytes set by `fill` between two guard blocks of 0xA5.  `.ptr` is 256-byte aligned, `.nbytes` is `need` and
    nothing else: what the caller got from pa_*_workspace_bytes, not rounded up."""

    def __init__(self, need: int, device, fill: str):
        self.need = int(need)
        assert self.need >= 0 and GUARD % 4096 == 0
        self.device = torch.device(device)
        self.buf = torch.full((GUARD + self.need + GUARD + ALIGN,), GUARD_BYTE, dtype=torch.uint8, device=self.device)
        self.lo = GUARD + (-self.buf.data_ptr()) % ALIGN      # (0 on the device; host allocations are 64-byte aligned)
        self.hi = self.lo + self.need
        if self.need:
            self.buf[self.lo:self.hi] = fill_bytes(fill, self.need, self.device)

    @property
    def address(self) -> int:
        return self.buf.data_ptr() + self.lo

    @property
    def ptr(self):
        return C.c_void_p(self.address)

    @property
    def nbytes(self) -> int:
        return self.need

    def inner(self) -> torch.Tensor:
        return self.buf[self.lo:self.hi]

    def guards_untouched(self):
        """(front, behind) after a synchronisation: every byte in front of / behind the `need` bytes still 0xA5"""
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        return (bool((self.buf[:self.lo] == GUARD_BYTE).all()), bool((self.buf[self.hi:] == GUARD_BYTE).all()))

    def check(self, what: str = ""):
        front, behind = self.guards_untouched()
        assert front, f"{what}: bytes in front of the workspace were overwritten"
        assert behind, f"{what}: bytes behind the {self.need} workspace bytes were overwritten"


def _output_guards_untouched(g: Guarded) -> bool:
    host = g.buf.cpu()
    return bool(g._untouched(host[:OUT_GUARD]).all()) and bool(g._untouched(host[OUT_GUARD + g.n:]).all())


def _numel(shape) -> int:
    n = 1
    for s in shape:
        n *= int(s)
    return n


def run_under_fills(call, need: int, outputs, device, what: str = "", initial=None):
    """call(ws_ptr, ws_bytes, *output_ptrs) -> return code, run on a workspace of `need` bytes filled with zeros, ones,
    huge and zeros again.  `outputs`: (shape, dtype) or (shape, dtype, untouched_value) each, every one a
    kernel_parity.Guarded buffer of its own per run.  Asserts, in this order: every return code 0; the two zeros runs
    agree byte for byte; ones and huge agree with zeros byte for byte; no guard of a workspace or an output was
    written.  `initial`: {output index: tensor} for outputs the call reads as well (copied in before every run).
    Returns the outputs of the ones run (host tensors of the given shapes)."""
    need = int(need)
    assert need > 0, f"{what}: the workspace query returned {need}"
    runs = []
    for fill in ("zeros", "ones", "huge", "zeros"):
        ws = HostileWorkspace(need, device, fill)
        outs = [Guarded(_numel(o[0]), device, o[1], o[2] if len(o) > 2 else None) for o in outputs]
        for i, value in (initial or {}).items():
            outs[i].buf[OUT_GUARD:OUT_GUARD + outs[i].n] = value.reshape(-1).to(outs[i].buf.device, outs[i].dtype)
        rc = call(ws.ptr, ws.nbytes, *[g.ptr for g in outs])
        ws_ok = ws.guards_untouched()                              # (synchronises)
        runs.append({"fill": fill, "rc": rc, "ws": ws_ok, "out_guards": [_output_guards_untouched(g) for g in outs],
                     "values": [g.buf.cpu()[OUT_GUARD:OUT_GUARD + g.n].reshape(o[0]) for g, o in zip(outs, outputs)]})
        del ws, outs

    def same_bytes(a, b):
        return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))

    def differing(a, b):
        d = (a.contiguous().view(-1).view(torch.uint8) != b.contiguous().view(-1).view(torch.uint8))
        d = d.view(a.numel(), -1).any(1).nonzero().view(-1)
        return f"{d.numel()} of {a.numel()} elements differ, the first at flat index {int(d[0])}"

    for r in runs:
        assert r["rc"] == 0, f"{what}: return code {r['rc']} on a workspace of {r['fill']}"
    base = runs[0]
    for i in range(len(outputs)):
        assert same_bytes(base["values"][i], runs[3]["values"][i]), (
            f"{what}: output {i} differs between two runs on a zeroed workspace: "
            + differing(base["values"][i], runs[3]["values"][i]))
    for r in runs[1:3]:
        for i in range(len(outputs)):
            assert same_bytes(base["values"][i], r["values"][i]), (
                f"{what}: output {i} depends on the workspace's contents ({r['fill']} against zeros): "
                + differing(base["values"][i], r["values"][i]))
    for r in runs:
        assert r["ws"][0], f"{what}: bytes in front of the workspace were overwritten ({r['fill']})"
        assert r["ws"][1], f"{what}: bytes behind the {need} workspace bytes were overwritten ({r['fill']})"
        for i, ok in enumerate(r["out_guards"]):
            assert ok, f"{what}: a guard block of output {i} was overwritten ({r['fill']})"
    return runs[1]["values"]
