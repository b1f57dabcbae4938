"""`pao_cluster_step` and `pao_emit` (include/pyannote_amd_online.h) held to the two contracts of the main header, as
tests/test_stream_contract_gpu.py holds the `pa_*` entry points to them:

  1. eager      one call on the default stream: the reference bytes R of every output and of the in / out state;
  2. capture    everything back to its untouched state, the call made inside torch.cuda.graph(stream=side,
                capture_error_mode="global"): return code 0, the capture ends clean, and afterwards outputs and state
                still hold what they held -- their `kernel_parity.Guarded` fill or their input -- guards included;
  3. replay     gives R byte for byte, guards intact; a second replay from the untouched state gives R again;
  4. the inputs still have their bits.

Neither entry point takes a workspace, so there is nothing to run under `hostile_workspace.run_under_fills`; outputs
start from the Guarded fill, which is the "contents on entry may be anything" of an output.  Plain torch.cuda.graph
capture; no runtime setting is touched."""
import numpy as np
import pytest
import torch

from kernel_parity import GUARD, Guarded

pytestmark = pytest.mark.gpu


class Case:
    """call(*pointers of `outs`) -> return code; `outs`: Guarded buffers, `initial[i]`: the input of in / out operand i"""

    def __init__(self, device, call, outs, initial, inputs):
        self.call, self.outs, self.inputs = call, outs, inputs
        for i, value in initial.items():
            outs[i].buf[GUARD:GUARD + outs[i].n] = value.reshape(-1).to(device, outs[i].dtype)
        self.clean = [g.buf.clone() for g in outs]

    def reset(self):
        for g, state in zip(self.outs, self.clean):
            g.buf.copy_(state)
        torch.cuda.synchronize()

    def run(self):
        return self.call(*[g.ptr for g in self.outs])

    def snapshot(self):
        torch.cuda.synchronize()
        return [g.buf.cpu().contiguous().view(-1).view(torch.uint8) for g in self.outs]

    def guards_intact(self, snap):
        for g, got, clean in zip(self.outs, snap, self.clean):
            clean = clean.cpu().contiguous().view(-1).view(torch.uint8)
            lo, hi = GUARD * g.buf.element_size(), (GUARD + g.n) * g.buf.element_size()
            assert torch.equal(got[:lo], clean[:lo]) and torch.equal(got[hi:], clean[hi:]), "a guard block was overwritten"


def _bits(tensors):
    return [t.detach().cpu().contiguous().view(-1).view(torch.uint8).clone() for t in tensors]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _cluster_step_case(device):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    rng = np.random.default_rng(3)
    M, N, S, D, K = 5, 7, 3, 33, 6
    slots = np.array([6, 0, 3, 2, 5], dtype=np.int32)
    emb = torch.from_numpy(rng.standard_normal((M, S, D)).astype(np.float32)).to(device)
    active = torch.from_numpy(rng.integers(0, 20, size=(M, S)).astype(np.int32)).to(device)
    clean = torch.from_numpy(rng.integers(0, 20, size=(M, S)).astype(np.int32)).to(device)
    d_slots = torch.from_numpy(slots).to(device)
    csum = torch.from_numpy(rng.standard_normal((N, K, D)))
    cn = torch.from_numpy(rng.integers(0, 3, size=(N, K)).astype(np.int32))
    outs = [Guarded(M * S, device, torch.int32), Guarded(N * K * D, device, torch.float64),
            Guarded(N * K, device, torch.int32)]

    def call(map_ptr, csum_ptr, cn_ptr):
        return lib.pao_cluster_step(ffi.ptr(d_slots), slots.ctypes.data, M, N, ffi.ptr(emb), ffi.ptr(active),
                                    ffi.ptr(clean), S, D, K, 5, 8, 0.9, csum_ptr, cn_ptr, map_ptr, ffi.stream())

    return Case(device, call, outs, {1: csum, 2: cn}, [emb, active, clean, d_slots])


def _emit_case(device):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    rng = np.random.default_rng(4)
    M, N, F, S, K, E = 4, 6, 37, 3, 5, 11
    R = F + E
    slots = np.array([5, 1, 0, 3], dtype=np.int32)
    frames = np.array([[100, 0, 60, -1], [110, 0, 60, 70], [121, 11, 60, 75]], dtype=np.int64)
    seg = torch.from_numpy((rng.random((M, F, S)) < 0.6).astype(np.uint8)).to(device)
    mp = torch.from_numpy(rng.integers(-1, K, size=(M, S)).astype(np.int32)).to(device)
    d_slots, d_frames = torch.from_numpy(slots).to(device), torch.from_numpy(frames).to(device)
    acc_sum = torch.from_numpy(rng.integers(0, 3, size=(N, R, K)).astype(np.int32))
    acc_cnt = torch.from_numpy(rng.integers(3, 6, size=(N, R)).astype(np.int32))
    outs = [Guarded(M * E * K, device, torch.uint8), Guarded(N * R * K, device, torch.int32),
            Guarded(N * R, device, torch.int32)]

    def call(out_ptr, sum_ptr, cnt_ptr):
        return lib.pao_emit(ffi.ptr(d_slots), slots.ctypes.data, M, N, ffi.ptr(seg), F, S, ffi.ptr(mp),
                            ffi.ptr(d_frames[0]), ffi.ptr(d_frames[1]), ffi.ptr(d_frames[2]), frames.ctypes.data, R, K,
                            E, sum_ptr, cnt_ptr, out_ptr, ffi.stream())

    return Case(device, call, outs, {1: acc_sum, 2: acc_cnt}, [seg, mp, d_slots, d_frames])


@pytest.mark.parametrize("build", [_cluster_step_case, _emit_case], ids=["pao_cluster_step", "pao_emit"])
def test_online_entry_point_is_captured_whole(gpu_device, build):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    lib.pa_prof_enable(0)
    with torch.cuda.device(gpu_device):
        case = build(gpu_device)
        inputs = _bits(case.inputs)
        case.reset()
        clean = case.snapshot()

        rc = case.run()
        assert rc == 0, lib.pa_last_error().decode()
        R = case.snapshot()
        case.guards_intact(R)
        assert all(not torch.equal(r, c) for r, c in zip(R, clean)), "the eager call left an output or the state alone"

        case.reset()
        side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        rc, failure = None, None
        try:
            with torch.cuda.graph(graph, stream=side, capture_error_mode="global"):
                rc = case.run()
        except Exception as e:                                                           # noqa: BLE001
            failure = e
        assert failure is None, f"the capture did not end clean: {failure!r}; pa_last_error: {lib.pa_last_error().decode()}"
        assert rc == 0, lib.pa_last_error().decode()
        assert _same(case.snapshot(), clean), "something ran while the call was only being captured"

        graph.replay()
        got = case.snapshot()
        case.guards_intact(got)
        assert _same(got, R), "the replayed graph does not give the eager bytes"

        case.reset()
        graph.replay()
        got = case.snapshot()
        case.guards_intact(got)
        assert _same(got, R), "the second replay does not give the eager bytes"
        assert _same(_bits(case.inputs), inputs), "an input was modified"
        del graph
