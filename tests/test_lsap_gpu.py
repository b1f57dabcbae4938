"""GPU: `pa_lsap_batch` (csrc/lsap.hip) directly and through `distance.linear_sum_assignment_batch`, held to SciPy with
`==`: to the recorded assignments of tests/golden/lsap_v1.npz, where nearly every problem has several optima and only
SciPy's own order of operations returns SciPy's one, and to the installed SciPy on problems made here.  The installed
SciPy is held to the golden file by tests/test_lsap_model_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from lsap_model import golden_problems

pytestmark = pytest.mark.gpu

GUARD = -77


def c_lsap(cost, maximize=False, row_mask=None, col_mask=None, want_total=True):
    """one `pa_lsap_batch` call on the device tensor `cost` (B, R, C) as it lies, guard rows around every output
    -> (col4row, total, status) as numpy arrays"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    B, R, C = cost.shape
    dev = cost.device
    col4row = torch.full((B + 2, max(R, 1)), GUARD, dtype=torch.int32, device=dev)
    total = torch.full((B + 2,), float(GUARD), dtype=torch.float64, device=dev)
    status = torch.full((B + 2,), 99, dtype=torch.uint8, device=dev)
    masks = [None if m is None else torch.from_numpy(np.asarray(m, dtype=np.uint64).view(np.int64)).to(dev)
             for m in (row_mask, col_mask)]
    rc = lib.pa_lsap_batch(ctypes.c_void_p(cost.data_ptr()), *cost.stride(), B, R, C, ffi.ptr(masks[0]),
                           ffi.ptr(masks[1]), int(maximize), ffi.ptr(col4row[1:]) if R else None,
                           ffi.ptr(total[1:]) if want_total else None, ffi.ptr(status[1:]), ffi.stream())
    ffi.check(rc, "pa_lsap_batch")
    col4row, total, status = col4row.cpu().numpy(), total.cpu().numpy(), status.cpu().numpy()
    if R:
        flat = col4row.reshape(-1)
        assert (flat[:R] == GUARD).all() and (flat[R * (B + 1):] == GUARD).all()
        col4row = flat[R:R * (B + 1)].reshape(B, R)
    else:
        assert (col4row == GUARD).all()
        col4row = np.zeros((B, 0), dtype=np.int32)
    assert total[0] == GUARD and total[-1] == GUARD and status[0] == 99 and status[-1] == 99
    assert want_total or (total == GUARD).all()
    return col4row, total[1:-1], status[1:-1]


def expected(rows: int, row_ind, col_ind, row_of=None, col_of=None) -> np.ndarray:
    out = np.full(rows, -1, dtype=np.int32)
    row_ind, col_ind = np.asarray(row_ind, dtype=np.int64), np.asarray(col_ind, dtype=np.int64)
    out[row_ind if row_of is None else row_of[row_ind]] = col_ind if col_of is None else col_of[col_ind]
    return out


def python_total(cost: np.ndarray, col4row: np.ndarray) -> float:
    total = 0.0
    for r in range(len(col4row)):
        if col4row[r] >= 0:
            total += float(cost[r, col4row[r]])
    return total


@pytest.fixture(scope="module")
def golden():
    return golden_problems()


@pytest.mark.parametrize("slot,which", [(12, "small"), (64, "large")])
def test_golden_problems_in_masked_slots(gpu_device, golden, slot, which):
    """every problem sits in the corner of a slot of NaNs and is cut out by the masks, one launch for all of them,
    through the C entry point and through the Python function"""
    from pyannote_audio_amd.distance import linear_sum_assignment_batch
    problems = [p for p in golden if (max(p[0].shape) <= 12) == (which == "small")]
    assert len(problems) == (2000 if which == "small" else 40)
    for maximize in (False, True):
        chosen = [p for p in problems if p[1] == maximize]
        batch = np.full((len(chosen), slot, slot), np.nan)
        want = np.full((len(chosen), slot), -1, dtype=np.int32)
        row_mask, col_mask = np.zeros(len(chosen), dtype=np.uint64), np.zeros(len(chosen), dtype=np.uint64)
        for n, (cost, _, r, c) in enumerate(chosen):
            nr, nc = cost.shape
            batch[n, :nr, :nc] = cost
            want[n] = expected(slot, r, c)
            row_mask[n], col_mask[n] = (1 << nr) - 1 if nr < 64 else 2 ** 64 - 1, (1 << nc) - 1 if nc < 64 else 2 ** 64 - 1
        device_batch = torch.from_numpy(batch).to(gpu_device)
        col4row, total, status = c_lsap(device_batch, maximize, row_mask, col_mask)
        assert not status.any()
        wrong = np.flatnonzero((col4row != want).any(axis=1))
        assert wrong.size == 0, f"{wrong.size} of {len(chosen)} problems differ, the first is {wrong[0]}"
        assert total.tolist() == [python_total(np.nan_to_num(batch[n]), want[n]) for n in range(len(chosen))]
        tables = [(np.arange(slot)[None, :] < np.array([p[0].shape[k] for p in chosen])[:, None]) for k in (0, 1)]
        got = linear_sum_assignment_batch(device_batch, maximize=maximize, row_mask=torch.from_numpy(tables[0]),
                                          col_mask=torch.from_numpy(tables[1]))
        assert got.dtype == torch.int32 and got.device == device_batch.device and np.array_equal(got.cpu().numpy(), want)


def test_golden_problems_unmasked_by_shape(gpu_device, golden):
    """the same problems without masks: one launch per shape and direction, wide and tall"""
    from pyannote_audio_amd.distance import linear_sum_assignment_batch
    groups = {}
    for cost, maximize, r, c in golden:
        groups.setdefault((cost.shape, maximize), []).append((cost, r, c))
    assert len(groups) > 150
    for (shape, maximize), members in groups.items():
        batch = torch.from_numpy(np.stack([m[0] for m in members])).to(gpu_device)
        got = linear_sum_assignment_batch(batch, maximize=maximize).cpu().numpy()
        want = np.stack([expected(shape[0], r, c) for _, r, c in members])
        assert np.array_equal(got, want), (shape, maximize)


@pytest.mark.parametrize("shape", [(1, 1), (1, 64), (64, 1), (64, 64), (5, 9), (9, 5), (63, 64), (33, 17)])
def test_continuous_costs_equal_live_scipy(gpu_device, shape):
    """a unique optimum; `maximize`; `total` equals the Python sum in ascending row order on doubles that are not
    dyadic; a transposed view through the strides equals the solve of the materialised transpose"""
    from pyannote_audio_amd.distance import linear_sum_assignment_batch
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    batch = rng.standard_normal((9, *shape)) / 3.0 + 0.1
    device_batch = torch.from_numpy(batch).to(gpu_device)
    for maximize in (False, True):
        want = np.stack([expected(shape[0], *linear_sum_assignment(m, maximize=maximize)) for m in batch])
        col4row, total, status = c_lsap(device_batch, maximize)
        assert not status.any() and np.array_equal(col4row, want)
        assert total.tolist() == [python_total(m, w) for m, w in zip(batch, want)]
        assert np.array_equal(c_lsap(device_batch, maximize, want_total=False)[0], want)
        got, got_total = linear_sum_assignment_batch(device_batch, maximize=maximize, return_total=True)
        assert np.array_equal(got.cpu().numpy(), want) and got_total.cpu().numpy().tolist() == total.tolist()
        # the transposed problem: a view, and its copy
        want_t = np.stack([expected(shape[1], *linear_sum_assignment(m.T, maximize=maximize)) for m in batch])
        view = device_batch.transpose(1, 2)
        assert not view.is_contiguous() or 1 in shape
        by_view, total_view, _ = c_lsap(view, maximize)
        by_copy, total_copy, _ = c_lsap(view.contiguous(), maximize)
        assert np.array_equal(by_view, want_t) and np.array_equal(by_copy, want_t)
        assert total_view.tolist() == total_copy.tolist() == [python_total(m.T, w) for m, w in zip(batch, want_t)]
    # the host route of the Python function: the same shapes and values
    host, host_total = linear_sum_assignment_batch(batch, maximize=True, return_total=True)
    assert host.dtype == np.int32 and np.array_equal(host, want) and host_total.tolist() == total.tolist()


def test_three_thousand_masked_problems_in_one_launch(gpu_device):
    """16 x 16 slots, every problem with its own row and column mask -- empty masks and single bits among them --
    tie-rich integers and continuous costs by turns; SciPy sees the compacted matrix"""
    rng = np.random.default_rng(16)
    B, slot = 3000, 16
    batch = np.where(np.arange(B)[:, None, None] % 2 == 0, rng.integers(0, 3, (B, slot, slot)).astype(np.float64),
                     rng.standard_normal((B, slot, slot)))
    bits = rng.random((2, B, slot)) < rng.random((2, B, 1))
    bits[:, 0] = False                                   # no row and no column
    bits[0, 1], bits[1, 2] = False, False                # no row; no column
    bits[:, 3:40] = False
    bits[0, np.arange(3, 40), rng.integers(0, slot, 37)] = True       # single bits
    bits[1, np.arange(3, 40), rng.integers(0, slot, 37)] = True
    bits[:, 40] = True                                   # everything
    masks = (bits.astype(np.uint64) << np.arange(slot, dtype=np.uint64)).sum(axis=2).astype(np.uint64)
    # bits above the slot are ignored
    masks[:, 41:60] |= np.uint64(0xFFFF) << np.uint64(16)
    for maximize in (False, True):
        want = np.full((B, slot), -1, dtype=np.int32)
        for n in range(B):
            row_of, col_of = np.flatnonzero(bits[0, n]), np.flatnonzero(bits[1, n])
            r, c = linear_sum_assignment(batch[n][row_of][:, col_of], maximize=maximize)
            want[n] = expected(slot, r, c, row_of, col_of)
        col4row, total, status = c_lsap(torch.from_numpy(batch).to(gpu_device), maximize, masks[0], masks[1])
        assert not status.any()
        wrong = np.flatnonzero((col4row != want).any(axis=1))
        assert wrong.size == 0, f"{wrong.size} problems differ, the first is {wrong[0]}"
        assert total.tolist() == [python_total(batch[n], want[n]) for n in range(B)]
        assert (want[:3] == -1).all() and not total[:3].any()


def test_forbidden_pairs_and_refused_problems(gpu_device):
    """+inf forbids a pair, as in SciPy; a NaN, a -inf and an infeasible problem among good ones get status 1, 1 and
    2 and leave their neighbours alone; the Python function raises SciPy's texts"""
    from pyannote_audio_amd.distance import linear_sum_assignment_batch
    rng = np.random.default_rng(5)
    batch = rng.integers(0, 4, (12, 7, 9)).astype(np.float64)
    batch[rng.random(batch.shape) < 0.3] = np.inf
    batch[:, np.arange(7), np.arange(7)] = 1.0                     # (a finite diagonal: feasible)
    good = batch.copy()
    batch[2, 3, 4] = np.nan
    batch[5, 0, 8] = -np.inf
    batch[9, :, 1:] = np.inf                                       # seven rows want column 0
    want = np.stack([expected(7, *linear_sum_assignment(m)) for m in good])
    for n in (2, 5, 9):
        want[n] = -1
    device_batch = torch.from_numpy(batch).to(gpu_device)
    col4row, total, status = c_lsap(device_batch)
    assert status.tolist() == [0, 0, 1, 0, 0, 1, 0, 0, 0, 2, 0, 0]
    assert np.array_equal(col4row, want)
    assert total.tolist() == [python_total(m, w) for m, w in zip(batch, want)] and not total[[2, 5, 9]].any()
    # tall: the transposed view has more rows than columns
    tall = np.stack([expected(9, *linear_sum_assignment(m.T)) for m in good])
    for n in (2, 5, 9):
        tall[n] = -1
    col4row, _, status = c_lsap(device_batch.transpose(1, 2))
    assert status.tolist() == [0, 0, 1, 0, 0, 1, 0, 0, 0, 2, 0, 0] and np.array_equal(col4row, tall)
    # maximised, +inf is what SciPy refuses and -inf what it avoids
    col4row, _, status = c_lsap(torch.from_numpy(-batch).to(gpu_device), maximize=True)
    assert status.tolist() == [0, 0, 1, 0, 0, 1, 0, 0, 0, 2, 0, 0] and np.array_equal(col4row, want)
    # the Python function
    got, flags = linear_sum_assignment_batch(device_batch, check=False)
    assert flags.dtype == torch.uint8 and flags.cpu().tolist() == status.tolist()
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match=r"matrix contains invalid numeric entries \(problem 2 "):
        linear_sum_assignment_batch(device_batch)
    with pytest.raises(ValueError, match=r"cost matrix is infeasible \(problem 0 "):
        linear_sum_assignment_batch(device_batch[9:])
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        linear_sum_assignment(batch[9])
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        linear_sum_assignment(batch[5])
    assert np.array_equal(linear_sum_assignment_batch(torch.from_numpy(good).to(gpu_device)).cpu().numpy(),
                          np.stack([expected(7, *linear_sum_assignment(m)) for m in good]))


def test_limits_and_empty_batches(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd.distance import linear_sum_assignment_batch
    lib = ffi.load()
    assert lib.pa_lsap_max_size() == 64
    # batch == 0: nothing is launched and nothing is needed
    assert lib.pa_lsap_batch(None, 0, 0, 0, 0, 5, 5, None, None, 0, None, None, None, ffi.stream()) == 0
    empty = linear_sum_assignment_batch(torch.zeros((0, 5, 6), dtype=torch.float64, device=gpu_device),
                                        return_total=True)
    assert empty[0].shape == (0, 5) and empty[1].shape == (0,)
    # a problem without columns or without rows is solved
    col4row, total, status = c_lsap(torch.zeros((3, 4, 0), dtype=torch.float64, device=gpu_device))
    assert (col4row == -1).all() and not total.any() and not status.any()
    col4row, total, status = c_lsap(torch.zeros((3, 0, 4), dtype=torch.float64, device=gpu_device))
    assert col4row.shape == (3, 0) and not total.any() and not status.any()
    # 65 a side
    wide = torch.zeros((2, 3, 65), dtype=torch.float64, device=gpu_device)
    with pytest.raises(ValueError, match="at most 64 rows and columns"):
        linear_sum_assignment_batch(wide)
    with pytest.raises(ValueError, match="at most 64 rows and 64 columns"):
        c_lsap(wide)
    with pytest.raises(ValueError, match="at most 64 rows and 64 columns"):
        c_lsap(wide.transpose(1, 2))
    with pytest.raises(ValueError, match="float64"):
        linear_sum_assignment_batch(wide[:, :, :3].float())
