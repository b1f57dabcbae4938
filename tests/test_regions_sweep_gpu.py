"""pa_regions_sweep_count / pa_regions_sweep_emit (csrc/regions_sweep.hip) through `frames.binarize_regions_sweep`:
every job's rows and track positions against the frame-by-frame oracle and against the single-call kernel, BIT FOR
BIT (rows are compared as int64 views)."""
import numpy as np
import pytest
import torch

import regions_sweep_cases as rs
from pyannote_audio_amd import frames as frame_ops

pytestmark = pytest.mark.gpu


def sweep(device, scores, *tables, **kwargs):
    return frame_ops.binarize_regions_sweep(torch.from_numpy(scores).to(device), rs.window(), *tables,
                                            return_tracks=True, **kwargs)


@pytest.mark.parametrize("K", [1, 3, 16])
def test_regions_equal_the_oracle_on_the_grid(gpu_device, K):
    for key in rs.grid(K):
        (scores, *tables), want = rs.case_with_truth(*key)
        rs.assert_same(sweep(gpu_device, scores, *tables), want, key)


def test_every_job_equals_the_single_call_kernel(gpu_device):
    rng = np.random.default_rng(11)
    T, K, L = 20000, 4, 64
    scores = rs.mo.smooth_scores(rng, T, K, width=25, nan_fraction=0.01)
    x = torch.from_numpy(scores).to(gpu_device)
    lane_class = rng.integers(0, K, L).astype(np.int32)
    onset, offset = rng.uniform(0.3, 0.7, L).astype(np.float32), rng.uniform(0.3, 0.7, L).astype(np.float32)
    job_lane = rng.permutation(np.repeat(np.arange(L, dtype=np.int32), 2))
    d_on, d_off = rng.choice([0.0, 0.05, 0.2], 2 * L), rng.choice([0.0, 0.04, 0.3], 2 * L)
    regions, positions = frame_ops.binarize_regions_sweep(x, rs.window(), lane_class, onset, offset, job_lane, d_on,
                                                          d_off, return_tracks=True)
    assert sum(len(r) for r in regions) > 1000
    for j, lane in enumerate(job_lane):
        # the single-call kernel takes one detector per class: the job's parameters on every column, its column read
        one, tracks = frame_ops.binarize_regions(x, rs.window(), float(onset[lane]), float(offset[lane]),
                                                 float(d_on[j]), float(d_off[j]), return_tracks=True)
        k = lane_class[lane]
        assert np.array_equal(one[k].view(np.int64), regions[j].view(np.int64)), j
        assert tracks[k].tolist() == positions[j].tolist(), j


def test_the_raw_list_survives_its_readers(gpu_device):
    (scores, lane_class, onset, offset, *_), _ = rs.case_with_truth(77, 3073, 3, 17, 0.02)
    lane = 4
    job_lane = np.array([lane, lane, lane], dtype=np.int32)
    d_on, d_off = np.array([0.05, 0.3, 0.05]), np.array([0.1, 0.5, 0.1])
    want = rs.truth(scores, lane_class, onset, offset, job_lane, d_on, d_off)
    assert len(want[0][0]) > len(want[1][0]) > 0
    got = sweep(gpu_device, scores, lane_class, onset, offset, job_lane, d_on, d_off)
    rs.assert_same(got, want, "three readers")
    assert np.array_equal(got[0][0].view(np.int64), got[0][2].view(np.int64)) and \
        got[1][0].tolist() == got[1][2].tolist()


def group_bytes(T):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    return int(lib.pa_regions_sweep_workspace_bytes(T, 5, 1, 35, 0, 0, 0)) - \
        int(lib.pa_regions_sweep_workspace_bytes(T, 5, 0, 35, 0, 0, 0))


def same_tensors(a, b):
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1], b[1])
    assert np.array_equal(a[2], b[2])


def test_results_do_not_depend_on_the_split(gpu_device):
    T = 3073
    (_, *tables), _ = rs.case_with_truth(78, T, 3, 33, 0.0)                   # 35 lanes: 3 + 1 + 1 groups
    tables[2] = np.minimum(tables[1], tables[2])      # (offset above onset flips the state on every frame in between)
    # slow scores, three regions a lane: the row buffers of all lanes are smaller than one group's event words
    t, k = np.arange(T, dtype=np.float64)[:, None], np.arange(3, dtype=np.float64)[None, :]
    scores = (0.5 + 0.4 * np.sin(2.0 * np.pi * (t / 1000.0 + k / 3.0))).astype(np.float32)
    want = rs.truth(scores, *tables)
    x = torch.from_numpy(scores).to(gpu_device)
    whole_stats, split_stats, calls_stats = {}, {}, {}
    whole = frame_ops.binarize_regions_sweep(x, rs.window(), *tables, return_tracks=True, to_host=False,
                                             stats=whole_stats)
    assert whole_stats == {"count_launches": 1, "emit_launches": 1, "calls": 1}
    rows, tracks, offsets = whole
    got = ([rows.cpu().numpy()[a:b] for a, b in zip(offsets[:-1], offsets[1:])],
           [tracks.cpu().numpy()[a:b] for a, b in zip(offsets[:-1], offsets[1:])])
    rs.assert_same(got, want, "whole")
    # a budget of one group's event words and chunk tables: one call, every group in a launch sequence of its own
    split = frame_ops.binarize_regions_sweep(x, rs.window(), *tables, return_tracks=True, to_host=False,
                                             workspace_bytes=group_bytes(T), stats=split_stats)
    assert split_stats == {"count_launches": 5, "emit_launches": 5, "calls": 1}
    same_tensors(whole, split)
    # a budget below the row buffers as well: the lanes go in several calls, some of them with several groups
    calls = frame_ops.binarize_regions_sweep(x, rs.window(), *tables, return_tracks=True, to_host=False,
                                             workspace_bytes=2048, stats=calls_stats)
    assert calls_stats["calls"] >= 3 and calls_stats["emit_launches"] > calls_stats["calls"]
    same_tensors(whole, calls)


def test_degenerate_cases(gpu_device):
    for T in (0, 1):
        regions, positions = sweep(gpu_device, np.full((T, 2), 0.9, dtype=np.float32), [0, 1], 0.5, 0.5, [0, 1, 1])
        assert [len(r) for r in regions] == [0, 0, 0] and [len(p) for p in positions] == [0, 0, 0]
    x = np.full((40, 2), 0.9, dtype=np.float32)
    assert sweep(gpu_device, x, [], [], [], []) == ([], [])
    assert sweep(gpu_device, x, [0], 0.5, 0.5, []) == ([], [])
    (never, always, again), _ = sweep(gpu_device, x, [0, 1, 1], [0.95, 0.5, 0.5], [0.95, 0.5, 0.5], [0, 1, 2])
    first, last = rs.mo.frame_middle(0, *rs.FRAMES), rs.mo.frame_middle(39, *rs.FRAMES)
    assert len(never) == 0 and always.tolist() == [[first, last]] and again.tolist() == always.tolist()


def test_every_refusal_returns_an_error_and_launches_nothing(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    T = 100
    x = torch.full((T, 2), 0.9, dtype=torch.float32, device=gpu_device)
    nan = float("nan")
    cases = [dict(K=17), dict(K=0), dict(lane_class=[2]), dict(lane_class=[-1]), dict(onset=[nan]), dict(offset=[nan]),
             dict(job_lane=[1]), dict(job_lane=[-1]), dict(d_on=[nan]), dict(d_off=[nan])]
    for case in cases:
        a = dict(K=2, lane_class=[0], onset=[0.5], offset=[0.5], job_lane=[0], d_on=[0.0], d_off=[0.0])
        a.update(case)
        lane_class, job_lane = np.array(a["lane_class"], dtype=np.int32), np.array(a["job_lane"], dtype=np.int32)
        onset, offset = np.array(a["onset"], dtype=np.float32), np.array(a["offset"], dtype=np.float32)
        d_on, d_off = np.array(a["d_on"]), np.array(a["d_off"])
        n_raw, launches = np.full(1, 50, dtype=np.int32), np.full(1, -1, dtype=np.int32)
        nbytes = 1 << 20
        ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=gpu_device)
        out = torch.full((50, 2), -1.5, dtype=torch.float64, device=gpu_device)
        job_off = torch.full((2,), -7, dtype=torch.int32, device=gpu_device)
        lane_fault = not set(case) & {"job_lane", "d_on", "d_off"}
        if lane_fault:
            rc = lib.pa_regions_sweep_count(ffi.ptr(x), T, a["K"], 1, lane_class.ctypes.data, onset.ctypes.data,
                                            offset.ctypes.data, n_raw.ctypes.data, launches.ctypes.data, ffi.ptr(ws),
                                            nbytes, ffi.stream())
            assert rc == 3 and launches[0] == 0 and lib.pa_last_error().decode(), case
            assert int(lib.pa_regions_sweep_groups(a["K"], 1, lane_class.ctypes.data)) == -1 or "onset" in case \
                or "offset" in case
        n_raw[0] = 50
        rc = lib.pa_regions_sweep_emit(ffi.ptr(x), T, a["K"], 1, lane_class.ctypes.data, onset.ctypes.data,
                                       offset.ctypes.data, n_raw.ctypes.data, 1, job_lane.ctypes.data,
                                       d_on.ctypes.data, d_off.ctypes.data, *rs.FRAMES, 50, ffi.ptr(out), None,
                                       ffi.ptr(job_off), launches.ctypes.data, ffi.ptr(ws), nbytes, ffi.stream())
        torch.cuda.synchronize()
        assert rc == 3 and launches[0] == 0, case
        with pytest.raises(ValueError):
            ffi.check(rc, "pa_regions_sweep_emit")
        assert (ws == 0xA5).all() and (out == -1.5).all() and (job_off == -7).all(), case
