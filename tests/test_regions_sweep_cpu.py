"""The numpy form of the region sweep (`frames.binarize_regions_sweep` on CPU scores) against the frame-by-frame
oracle, bit for bit, on the grid the GPU test uses; and its refusals."""
import numpy as np
import pytest
import torch

import regions_sweep_cases as rs
from pyannote_audio_amd import frames as frame_ops


@pytest.mark.parametrize("K", [1, 3, 16])
def test_numpy_form_equals_the_oracle_on_the_grid(K):
    for key in rs.grid(K):
        (scores, *tables), want = rs.case_with_truth(*key)
        got = frame_ops.binarize_regions_sweep(scores, rs.window(), *tables, return_tracks=True)
        rs.assert_same(got, want, key)


def test_packed_form_and_tensor_input():
    (scores, *tables), want = rs.case_with_truth(5, 1025, 3, 17, 0.02)
    rows, tracks, offsets = frame_ops.binarize_regions_sweep(torch.from_numpy(scores), rs.window(), *tables,
                                                             return_tracks=True, to_host=False)
    assert rows.dtype == torch.float64 and tracks.dtype == torch.int32 and len(offsets) == len(want) + 1
    got = ([rows.numpy()[a:b] for a, b in zip(offsets[:-1], offsets[1:])],
           [tracks.numpy()[a:b] for a, b in zip(offsets[:-1], offsets[1:])])
    rs.assert_same(got, want, "packed")


def test_degenerate_cases():
    w = rs.window()
    for T in (0, 1):
        out = frame_ops.binarize_regions_sweep(np.full((T, 2), 0.9, dtype=np.float32), w, [0, 1], 0.5, 0.5, [0, 1, 1])
        assert [len(r) for r in out] == [0, 0, 0]
    x = np.full((40, 2), 0.9, dtype=np.float32)
    assert frame_ops.binarize_regions_sweep(x, w, [], [], [], []) == []
    assert frame_ops.binarize_regions_sweep(x, w, [0], 0.5, 0.5, []) == []
    never, always, again = frame_ops.binarize_regions_sweep(x, w, [0, 1, 1], [0.95, 0.5, 0.5], [0.95, 0.5, 0.5],
                                                            [0, 1, 2])
    assert len(never) == 0
    first, last = rs.mo.frame_middle(0, *rs.FRAMES), rs.mo.frame_middle(39, *rs.FRAMES)
    assert always.tolist() == [[first, last]] and again.tolist() == always.tolist()


@pytest.mark.parametrize("kwargs", [dict(lane_class=[2]), dict(lane_class=[-1]), dict(job_lane=[1]),
                                    dict(onset=[float("nan")]), dict(offset=[float("nan")]),
                                    dict(min_duration_on=[float("nan")]), dict(min_duration_off=[float("nan")])])
def test_refusals(kwargs):
    args = dict(lane_class=[0], onset=[0.5], offset=[0.5], job_lane=[0], min_duration_on=[0.0], min_duration_off=[0.0])
    args.update(kwargs)
    with pytest.raises(ValueError):
        frame_ops.binarize_regions_sweep(np.zeros((10, 2), dtype=np.float32), rs.window(), **args)
    with pytest.raises(ValueError):
        frame_ops.binarize_regions_sweep(np.zeros((10, 17), dtype=np.float32), rs.window(), [0], 0.5, 0.5, [0])
