"""`pao_detect_step` (include/pyannote_amd_online.h) held to the two contracts of the main header, exactly as
tests/test_online_contract_gpu.py holds `pao_cluster_step` and `pao_emit` to them:

  1. eager      one call on the default stream: the reference bytes R of every output and of the in / out state;
  2. capture    everything back to its untouched state, the call made inside torch.cuda.graph(stream=side,
                capture_error_mode="global"): return code 0, the capture ends clean, and afterwards outputs and state
                still hold what they held -- their `kernel_parity.Guarded` fill or their input -- guards included;
  3. replay     gives R byte for byte, guards intact; a second replay from the untouched state gives R again;
  4. the inputs still have their bits.

The entry point takes no workspace; outputs start from the Guarded fill, which is the "contents on entry may be
anything" of an output.  Plain torch.cuda.graph capture; no runtime setting is touched."""
import numpy as np
import pytest
import torch

from kernel_parity import Guarded
from test_online_contract_gpu import Case, _bits, _same

pytestmark = pytest.mark.gpu


def _numbers(uint8):
    """the case on the host: sizes, tables, scores, parameters and the state on entry (in the header's order)"""
    rng = np.random.default_rng(6)
    M, N, F, S, E = 4, 6, 37, 3, 11
    any = int(uint8)
    K = 1 if any else S
    R, cap = F + E, E // 2 + 2
    slots = np.array([5, 1, 0, 3], dtype=np.int32)
    # a chunk that emits all of E, one that emits a part, one that closes, and a closing flush
    rows = np.array([[100, 110, 121, -1], [100, 105, 116, 60], [111, 111, 127, 71], [0, 0, 1, 1]], dtype=np.int64)
    if uint8:
        scores = (rng.random((M, F, S)) < 0.3).astype(np.uint8) * 7
    else:
        scores = rng.random((M, F, S)).astype(np.float32)
    weights = np.stack([np.hamming(F), np.ones(F)])
    onset, offset = np.full(K, 0.55, np.float32), np.full(K, 0.45, np.float32)
    min_on, min_off = np.full(K, 0.02, np.float64), np.full(K, 0.03, np.float64)
    # a state in mid-stream: partial sums in the ring, every class active; a region pending in the slots that close
    weight = rng.random((N, R, K)).astype(np.float32) + 0.5
    pending = np.zeros((N, K), dtype=np.uint8)
    pending[[0, 3]] = 1
    state = {"acc": weight * rng.random((N, R, K)).astype(np.float32), "cnt": weight,
             "msk": np.ones((N, R, K), dtype=np.uint8), "on": np.ones((N, K), dtype=np.uint8),
             "open_start": np.full((N, K), 0.4), "pend": np.tile(np.array([0.1, 0.39]), (N, K, 1)),
             "has_pend": pending, "n_merged": np.full((N, K), 3, dtype=np.int32)}
    return dict(M=M, N=N, F=F, S=S, E=E, any=any, K=K, R=R, cap=cap, slots=slots, rows=rows, scores=scores,
                weights=weights, onset=onset, offset=offset, min_on=min_on, min_off=min_off, state=state)


def _detect_step_case(device, uint8):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    c = _numbers(uint8)
    M, N, F, S, E, any, K, R, cap = (c[n] for n in ("M", "N", "F", "S", "E", "any", "K", "R", "cap"))
    slots, rows, onset, offset, min_on, min_off = (c[n] for n in ("slots", "rows", "onset", "offset", "min_on", "min_off"))
    scores, weights = torch.from_numpy(c["scores"]).to(device), torch.from_numpy(c["weights"]).to(device)
    d_slots, d_rows = torch.from_numpy(slots).to(device), torch.from_numpy(rows).to(device)
    names = ("acc", "cnt", "msk", "on", "open_start", "pend", "has_pend", "n_merged")
    initial = {5 + i: torch.from_numpy(np.ascontiguousarray(c["state"][name])) for i, name in enumerate(names)}
    outs = [Guarded(M * E * K, device, torch.float32), Guarded(M * E * K, device, torch.uint8),
            Guarded(M * K, device, torch.int32), Guarded(M * K * cap * 2, device, torch.float64),
            Guarded(M * K * cap, device, torch.int32),
            Guarded(N * R * K, device, torch.float32), Guarded(N * R * K, device, torch.float32),
            Guarded(N * R * K, device, torch.uint8), Guarded(N * K, device, torch.uint8),
            Guarded(N * K, device, torch.float64), Guarded(N * K * 2, device, torch.float64),
            Guarded(N * K, device, torch.uint8), Guarded(N * K, device, torch.int32)]

    def call(values, active, counts, regions, tracks, acc, cnt, msk, on, open_start, pend, has_pend, n_merged):
        return lib.pao_detect_step(
            ffi.ptr(d_slots), slots.ctypes.data, M, N, ffi.ptr(scores), int(uint8), F, S, any, ffi.ptr(weights[0]),
            ffi.ptr(weights[1]), 1e-12, 0.0, ffi.ptr(d_rows[0]), ffi.ptr(d_rows[1]), ffi.ptr(d_rows[2]),
            ffi.ptr(d_rows[3]), rows.ctypes.data, 0.0, 0.0619375, 0.016875, onset.ctypes.data, offset.ctypes.data,
            min_on.ctypes.data, min_off.ctypes.data, R, E, cap, acc, cnt, msk, on, open_start, pend, has_pend,
            n_merged, values, active, counts, regions, tracks, ffi.stream())

    return Case(device, call, outs, initial, [scores, weights, d_slots, d_rows])


@pytest.mark.parametrize("uint8", [False, True], ids=["float32", "uint8-any"])
def test_detect_step_is_captured_whole(gpu_device, uint8):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    lib.pa_prof_enable(0)
    with torch.cuda.device(gpu_device):
        case = _detect_step_case(gpu_device, uint8)
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
