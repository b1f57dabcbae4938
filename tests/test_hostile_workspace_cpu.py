"""The check of the checker: tests/hostile_workspace.py on host tensors (no GPU).  What the GPU cases rely on -- the inner
pointer's alignment, the exact size, each fill's bit pattern at the widths the kernels read, and a guard check that is
off by one in neither direction -- is held here."""
import ctypes as C
import math
import struct

import numpy as np
import pytest
import torch

import hostile_workspace as hw
from hostile_workspace import FILLS, GUARD, GUARD_BYTE, HostileWorkspace

NEEDS = [1, 7, 256, 4096, 4099, 70001]


def _poke(address: int, value: int = 0x00):
    C.memset(C.c_void_p(address), value, 1)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("need", NEEDS)
def test_pointer_and_size(need, fill):
    ws = HostileWorkspace(need, "cpu", fill)
    assert GUARD % 4096 == 0 and GUARD >= 4096
    assert ws.ptr.value % 256 == 0, "the carvers assume a 256-byte aligned workspace"
    assert ws.nbytes == need, "nbytes is the value of the workspace query, not rounded up"
    base, end = ws.buf.data_ptr(), ws.buf.data_ptr() + ws.buf.numel()
    assert ws.ptr.value - base >= GUARD and end - (ws.ptr.value + need) >= GUARD
    raw = np.ctypeslib.as_array(C.cast(base, C.POINTER(C.c_uint8)), shape=(ws.buf.numel(),))
    lo = ws.ptr.value - base
    assert (raw[:lo] == GUARD_BYTE).all() and (raw[lo + need:] == GUARD_BYTE).all()
    assert np.array_equal(raw[lo:lo + need], hw.fill_bytes(fill, need, "cpu").numpy())
    ws.check("fresh")


def test_fill_patterns():
    """what each fill reads as, at the widths the kernels read workspaces at"""
    n = 4096
    z = hw.fill_bytes("zeros", n, "cpu")
    assert (z == 0).all()
    o = hw.fill_bytes("ones", n, "cpu")
    assert (o == 0xFF).all()
    assert torch.isnan(o.view(torch.float32)).all() and torch.isnan(o.view(torch.float64)).all()
    assert (o.view(torch.int32) == -1).all() and (o.view(torch.int64) == -1).all() and (o.view(torch.int16) == -1).all()
    h = hw.fill_bytes("huge", n, "cpu")
    f = h.view(torch.float32)
    assert (f[0::2] == np.float32(1e30)).all() and (f[1::2] == -np.float32(1e30)).all()
    i = h.view(torch.int32)
    plus = struct.unpack("<i", struct.pack("<f", 1e30))[0]
    assert plus > 1_000_000_000 and (i[0::2] == plus).all(), "+1e30 reads as a large positive int32 index"
    assert (i[1::2] < 0).all()
    d = h.view(torch.float64)
    assert torch.isfinite(d).all() and (d.abs() > 1e200).all(), "finite nonsense as float64"
    assert len(set(d.tolist())) == 1
    # an odd size keeps the pattern from byte 0 on
    assert torch.equal(hw.fill_bytes("huge", 13, "cpu"), h[:13])
    with pytest.raises(ValueError):
        hw.fill_bytes("sevens", 4, "cpu")


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("need", NEEDS)
def test_guard_check_is_exact(need, fill):
    """one byte in front of the workspace or one behind it fails the check; the last byte inside does not"""
    ws = HostileWorkspace(need, "cpu", fill)
    _poke(ws.ptr.value + need - 1)
    _poke(ws.ptr.value)
    ws.check("last and first byte inside")
    assert ws.guards_untouched() == (True, True)

    ws = HostileWorkspace(need, "cpu", fill)
    _poke(ws.ptr.value - 1)
    assert ws.guards_untouched() == (False, True)
    with pytest.raises(AssertionError, match="in front of the workspace"):
        ws.check("one byte in front")

    ws = HostileWorkspace(need, "cpu", fill)
    _poke(ws.ptr.value + need)
    assert ws.guards_untouched() == (True, False)
    with pytest.raises(AssertionError, match="behind the"):
        ws.check("one byte behind")

    # the far ends of both guards are watched too
    ws = HostileWorkspace(need, "cpu", fill)
    _poke(ws.ptr.value - GUARD)
    assert ws.guards_untouched() == (False, True)
    ws = HostileWorkspace(need, "cpu", fill)
    _poke(ws.ptr.value + need + GUARD - 1)
    assert ws.guards_untouched() == (True, False)


def _as_array(ptr, n, dtype):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * np.dtype(dtype).itemsize,)).view(dtype)


def test_run_under_fills_on_host_calls():
    """the four assertions of run_under_fills, each provoked by a host-side stand-in for a launch sequence"""
    need, n = 1000, 10
    outs = [((n,), torch.float32), ((2, 3), torch.int32)]

    def good(ws, nbytes, a, b):
        assert nbytes == need
        scratch = _as_array(ws, nbytes, np.uint8)
        scratch[:] = 7                                   # written before read
        _as_array(a, n, np.float32)[:] = np.arange(n) + float(scratch[5])
        _as_array(b, 6, np.int32)[:] = 0xA5             # (the "untouched" value itself is a legal result)
        return 0

    got = hw.run_under_fills(good, need, outs, "cpu", "good")
    assert got[0].tolist() == [i + 7.0 for i in range(n)] and got[1].shape == (2, 3)

    def refuses(ws, nbytes, a, b):
        return 3
    with pytest.raises(AssertionError, match="return code 3"):
        hw.run_under_fills(refuses, need, outs, "cpu", "refuses")

    state = {"calls": 0}

    def unstable(ws, nbytes, a, b):
        good(ws, nbytes, a, b)
        state["calls"] += 1
        _as_array(a, n, np.float32)[3] = state["calls"]
        return 0
    with pytest.raises(AssertionError, match="two runs on a zeroed workspace"):
        hw.run_under_fills(unstable, need, outs, "cpu", "unstable")

    def reads_scratch(ws, nbytes, a, b):
        first = float(_as_array(ws, nbytes // 4, np.float32)[1])
        good(ws, nbytes, a, b)
        _as_array(a, n, np.float32)[0] = max(first, 0.0)    # NaN and -1e30 vanish in the max ...
        _as_array(a, n, np.float32)[1] = first if math.isnan(first) else 0.0    # ... the NaN does not here
        return 0
    with pytest.raises(AssertionError, match=r"depends on the workspace's contents \(ones against zeros\)"):
        hw.run_under_fills(reads_scratch, need, outs, "cpu", "reads_scratch")

    def signed_zero(ws, nbytes, a, b):
        first = float(_as_array(ws, nbytes // 4, np.float32)[1])      # 0, NaN, -1e30
        good(ws, nbytes, a, b)
        _as_array(a, n, np.float32)[0] = -0.0 if first < 0 else 0.0   # equal as values, not as bytes
        return 0
    with pytest.raises(AssertionError, match=r"\(huge against zeros\)"):
        hw.run_under_fills(signed_zero, need, outs, "cpu", "signed_zero")

    def past_the_end(ws, nbytes, a, b):
        good(ws, nbytes, a, b)
        _poke(ws.value + nbytes)
        return 0
    with pytest.raises(AssertionError, match="behind the 1000 workspace bytes"):
        hw.run_under_fills(past_the_end, need, outs, "cpu", "past_the_end")

    def past_the_output(ws, nbytes, a, b):
        good(ws, nbytes, a, b)
        _as_array(b, 7, np.int32)[6] = 1
        return 0
    with pytest.raises(AssertionError, match="guard block of output 1"):
        hw.run_under_fills(past_the_output, need, outs, "cpu", "past_the_output")
