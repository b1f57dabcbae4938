"""Every stream-taking entry point held to the stream contract of include/pyannote_amd.h (tests/stream_contract.py).

The instrument is stream capture, not timing.  While a stream is captured in `global` mode, a synchronising call, an
allocation or work sent to the legacy stream from this thread is an ERROR, and work sent to the capturing stream becomes
a graph node that does not run.  So, for an `async` row:

  1. eager      one call on the default stream: the reference bytes R (and the warm-up: code objects are loaded and the
                tile-counter pool takes its first-use path outside any capture);
  2. capture    outputs poisoned again, workspace refilled with 0xFF, the call made inside
                torch.cuda.graph(stream=side, capture_error_mode="global"): return code 0, the capture ends clean, and
                afterwards every output element and every guard still holds its poison -- nothing escaped `side`;
  3. replay     the outputs equal R byte for byte, guards intact -- the captured nodes are the whole operation;
  4. replay     outputs poisoned, workspace refilled with +-1e30, again R: the same tile-counter block and the same
                workspace pointers as in 3, so a counter that does not return to zero, or state kept between launches,
                shows here and nowhere else;
  5. the inputs still have their bits.

A `waits` row is called under torch.cuda.stream(side) and must give the default-stream bytes, with its host-side results
valid on return and the stream idle: the call waited, the test does not.  Every comparison is on bytes.  The profiler
stays off (it records events of its own), and nothing here sets an environment variable or touches the queues."""
import os
import subprocess
import sys

import pytest
import torch

import stream_contract as sc
from hostile_workspace import HostileWorkspace, fill_bytes
from kernel_parity import GUARD, Guarded

pytestmark = pytest.mark.gpu


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


class Live:
    """an Entry with its output buffers and its workspace in place"""

    def __init__(self, entry, device):
        self.entry, self.device = entry, device
        self.outs = [Guarded(_numel(o[0]), device, o[1], o[2] if len(o) > 2 else None) for o in entry.outputs]
        self.ws = HostileWorkspace(entry.need, device, "ones") if entry.need is not None else None
        self.dtypes = [g.dtype for g in self.outs]
        self.poison_of = [g.buf.clone() for g in self.outs]
        for i, value in entry.initial.items():
            self.poison_of[i][GUARD:GUARD + self.outs[i].n] = value.reshape(-1).to(device, self.outs[i].dtype)

    def poison(self, fill=None):
        """every output back to its untouched state (in / out operands: to their input), the workspace to `fill`"""
        for g, state in zip(self.outs, self.poison_of):
            g.buf.copy_(state)
        if self.ws is not None and fill is not None and self.ws.need:
            self.ws.inner().copy_(fill_bytes(fill, self.ws.need, self.device))
        torch.cuda.synchronize()

    def run(self):
        ws = (self.ws.ptr, self.ws.nbytes) if self.ws is not None else (None, 0)
        return self.entry.call(*ws, *[g.ptr for g in self.outs])

    def snapshot(self):
        """the bytes of every output buffer, guards included (after a device-wide synchronisation)"""
        torch.cuda.synchronize()
        return [g.buf.cpu().contiguous().view(-1).view(torch.uint8) for g in self.outs]

    def untouched(self):
        return [s.cpu().contiguous().view(-1).view(torch.uint8) for s in self.poison_of]

    def guards_intact(self, snap, what):
        for i, (g, got, clean) in enumerate(zip(self.outs, snap, self.untouched())):
            lo, hi = GUARD * g.buf.element_size(), (GUARD + g.n) * g.buf.element_size()
            assert torch.equal(got[:lo], clean[:lo]) and torch.equal(got[hi:], clean[hi:]), \
                f"{what}: a guard block of output {i} was overwritten"
        if self.ws is not None:
            self.ws.check(what)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _first_difference(a, b, dtypes=None):
    for i, (x, y) in enumerate(zip(a, b)):
        d = (x != y).nonzero()
        if d.numel():
            text = f"output {i}: {d.numel()} of {x.numel()} bytes differ, the first at byte {int(d[0])} of its buffer"
            if dtypes is not None:
                xv, yv = x.view(dtypes[i]), y.view(dtypes[i])
                size = x.numel() // xv.numel()
                elements = sorted({int(k) // size for k in d.view(-1)[:4096]})[:4]
                text += "; elements (guard block included) " + ", ".join(
                    f"[{k - GUARD}] {xv[k].item()!r} for {yv[k].item()!r}" for k in elements)
            return text
    return "no difference"


def _error(lib):
    return lib.pa_last_error().decode(errors="replace")


def _input_bits(entry):
    return [t.detach().cpu().contiguous().view(-1).view(torch.uint8).clone() for t in entry.inputs]


ASYNC_ROWS = [r for r in sc.ROWS if r.cls == sc.ASYNC]
WAITS_ROWS = [r for r in sc.ROWS if r.cls == sc.WAITS]


@pytest.fixture(scope="module")
def lib(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    lib.pa_prof_enable(0)
    return lib


@pytest.mark.parametrize("row", ASYNC_ROWS, ids=sc.row_id)
def test_async_entry_point_is_captured_whole(gpu_device, lib, row):
    who = sc.row_id(row)
    with torch.cuda.device(gpu_device):
        entry = row.build(gpu_device)
        live = Live(entry, gpu_device)
        inputs = _input_bits(entry)
        clean = live.untouched()

        # 1. eager reference (and warm-up)
        live.poison("ones")
        rc = live.run()
        assert rc == 0, f"{who}: return code {rc} on the default stream: {_error(lib)}"
        R = live.snapshot()
        live.guards_intact(R, f"{who} (eager)")
        assert entry.outputs == [] or not _same(R, clean), f"{who}: the eager call wrote nothing"

        # 2. capture on a side stream: nothing may run, nothing may escape the stream
        live.poison("ones")
        side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        rc, failure = None, None
        try:
            with torch.cuda.graph(graph, stream=side, capture_error_mode="global"):      # (ends the capture on any exit)
                rc = live.run()
        except Exception as e:                                                           # noqa: BLE001
            failure = e
        assert failure is None, (f"{who}: the capture did not end clean (a synchronisation, an allocation or work on "
                                 f"another stream inside the launcher?): {failure!r}; return code {rc}; "
                                 f"pa_last_error: {_error(lib)}")
        assert rc == 0, f"{who}: return code {rc} while its stream was being captured: {_error(lib)}"
        after = live.snapshot()
        assert _same(after, clean), (f"{who}: something ran while the call was only being captured -- work that did not "
                                     f"go to the caller's stream: {_first_difference(after, clean, live.dtypes)}")
        if live.ws is not None:
            live.ws.check(f"{who} (capture)")

        # 3. replay: the captured sequence is the whole operation
        graph.replay()
        got = live.snapshot()
        live.guards_intact(got, f"{who} (replay)")
        assert _same(got, R), f"{who}: the replayed graph does not give the eager bytes: {_first_difference(got, R, live.dtypes)}"

        # 4. second replay, on the same counter block and the same workspace pointers, from other workspace contents
        live.poison("huge")
        graph.replay()
        got = live.snapshot()
        live.guards_intact(got, f"{who} (second replay)")
        assert _same(got, R), f"{who}: the second replay does not give the eager bytes: {_first_difference(got, R, live.dtypes)}"

        # 5. the inputs are inputs
        assert _same(_input_bits(entry), inputs), f"{who}: an input was modified"
        del graph


@pytest.mark.parametrize("row", WAITS_ROWS, ids=sc.row_id)
def test_waiting_entry_point_on_a_side_stream(gpu_device, lib, row):
    who = sc.row_id(row)
    with torch.cuda.device(gpu_device):
        entry = row.build(gpu_device)
        live = Live(entry, gpu_device)
        inputs = _input_bits(entry)
        live.poison("ones")
        rc = live.run()
        assert rc == 0, f"{who}: return code {rc} on the default stream: {_error(lib)}"
        host_default = [a.copy() for a in entry.host]
        R = live.snapshot()
        live.guards_intact(R, f"{who} (default stream)")

        live.poison("huge")
        for a in entry.host:
            a[...] = -9
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            rc = live.run()
            host_side = [a.copy() for a in entry.host]               # valid on return: the test has not synchronised
            idle = side.query()
        assert rc == 0, f"{who}: return code {rc} on a side stream: {_error(lib)}"
        for k, (a, b) in enumerate(zip(host_default, host_side)):
            assert a.tobytes() == b.tobytes(), f"{who}: host result {k} on return from the side-stream call: {b} vs {a}"
        if entry.host:
            assert idle, f"{who}: work was still pending on the stream when the call returned"
        got = live.snapshot()
        live.guards_intact(got, f"{who} (side stream)")
        assert _same(got, R), f"{who}: other bytes on a side stream: {_first_difference(got, R, live.dtypes)}"
        assert _same(_input_bits(entry), inputs), f"{who}: an input was modified"


# ------------------------------------------------------------------------------------------------------ cold start
def test_first_persistent_convolution_of_a_process_on_a_side_stream(gpu_device):
    """A fresh process whose FIRST call into the library is a persistent convolution on a non-blocking side stream, every
    claiming workgroup taking at least two tiles: the first-use path of the tile-counter pool (csrc/pa_core.cpp).  The
    result must be the integer convolution bit for bit -- a counter block that is not zero when the kernel reads it skips
    or repeats tiles."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stream_cold_start_child.py")
    done = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, f"exit status {done.returncode}\n{done.stdout[-2000:]}\n{done.stderr[-2000:]}"
    assert "COLD START OK" in done.stdout, done.stdout[-2000:]


# ------------------------------------------------------------------------------------------------- the Python side
def test_ffi_stream_follows_torch(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    with torch.cuda.device(gpu_device):
        default = torch.cuda.current_stream().cuda_stream
        assert (ffi.stream().value or 0) == default
        side = torch.cuda.Stream()
        assert side.cuda_stream != default
        with torch.cuda.stream(side):
            assert ffi.stream().value == side.cuda_stream
        assert (ffi.stream().value or 0) == default
        x = torch.zeros(8, device=gpu_device)
        torch.cuda.synchronize()
        graph, seen = torch.cuda.CUDAGraph(), None
        with torch.cuda.graph(graph, stream=side, capture_error_mode="global"):
            seen = ffi.stream().value
            x.add_(1.0)
        assert seen == side.cuda_stream
        assert (ffi.stream().value or 0) == default


def _bytes(t):
    t = torch.as_tensor(t)
    return t.detach().cpu().contiguous().view(-1).view(torch.uint8)


def _default_then_side(fn):
    """fn() on the default stream, then under a side stream -> both results"""
    torch.cuda.synchronize()
    first = fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        second = fn()
        side.synchronize()
    torch.cuda.synchronize()
    return first, second


def test_segmentation_engine_under_a_side_stream(gpu_device):
    """A smoke test: the engine reaches the library with torch's current stream, and a side stream gives the default
    stream's bytes.  It cannot prove ordering -- the capture tests above do that."""
    import entry_cases as ec
    from pyannote_audio_amd.segmentation import SegmentationEngine
    _, pack = ec.seg_models(gpu_device)["h128"]
    wav = ec.wave(16 * 1600 + ec.N1, seed=1).to(gpu_device)
    a, b = _default_then_side(lambda: SegmentationEngine(pack).forward_strided(wav, 1600, 17, ec.N1))
    assert torch.equal(_bytes(a[0]), _bytes(b[0])) and torch.equal(_bytes(a[1]), _bytes(b[1]))
    assert not torch.isnan(a[0]).any()


def test_embedding_engine_under_a_side_stream(gpu_device):
    """A smoke test: same bytes under a side stream.  It cannot prove ordering -- the capture tests above do that."""
    import entry_cases as ec
    from pyannote_audio_amd.embedding import EmbeddingEngine
    _, eng = ec.emb_models(gpu_device)["basic"]
    waveforms = ec.wave(3 * 32160, seed=4).view(3, 1, 32160).to(gpu_device)
    weights = ec.masks_01(3, 3, 115, seed=6).to(gpu_device)
    a, b = _default_then_side(lambda: EmbeddingEngine(eng.pack).forward(waveforms, weights))
    assert a.shape == (3, 3, 256) and torch.equal(_bytes(a), _bytes(b))
    assert not torch.isnan(a).any()


def test_linkage_centroid_under_a_side_stream(gpu_device):
    """A smoke test: same bytes under a side stream.  It cannot prove ordering -- the capture tests above do that."""
    import entry_cases as ec
    from pyannote_audio_amd import distance
    X = ec.clustered_unit(130, 16, seed=3, dup=20)
    a, b = _default_then_side(lambda: distance.linkage_centroid(X, gpu_device))
    assert a.shape == (129, 4) and a.tobytes() == b.tobytes()


def test_aggregate_under_a_side_stream(gpu_device):
    """A smoke test: same bytes under a side stream.  It cannot prove ordering -- the capture tests above do that."""
    import numpy as np
    import entry_cases as ec
    from pyannote_audio_amd import frames
    from pyannote_audio_amd.core import SlidingWindow
    scores = ec.rand("cpu", 6, 293, 3, seed=8).numpy()
    scores[2, :, 1] = np.nan
    chunks, grid = SlidingWindow(start=0.0, duration=5.0, step=0.5), SlidingWindow(start=0.0, duration=0.0619375,
                                                                                    step=0.016875)
    a, b = _default_then_side(lambda: frames.aggregate(scores, chunks, grid, gpu_device, hamming=True,
                                                       warm_up=(0.1, 0.1)))
    assert a.data.shape[1] == 3 and a.data.tobytes() == b.data.tobytes()
