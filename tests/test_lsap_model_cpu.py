"""tests/lsap_model.py, the restatement `pa_lsap_batch` and `pa_pair_costs` (csrc/lsap.hip) are held to, against the
installed SciPy and numpy with `==`: seeded families of tie-rich problems, every problem of tests/golden/lsap_v1.npz,
and the cost matrices of `permutation._pair_costs`."""
import numpy as np
import pytest
import scipy
from scipy.optimize import linear_sum_assignment

import lsap_model

GOLDEN = lsap_model.GOLDEN
golden_problems = lsap_model.golden_problems


def _same(cost, maximize):
    want = linear_sum_assignment(cost, maximize=maximize)
    got = lsap_model.solve(cost, maximize=maximize)
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_model_equals_scipy_on_small_problems():
    rng = np.random.default_rng(7)
    wrong = sum(not _same(lsap_model.small_problem(rng, n % 4), bool(n // 4 % 2)) for n in range(6000))
    assert wrong == 0


def test_model_equals_scipy_on_large_problems():
    rng = np.random.default_rng(11)
    wrong = sum(not _same(lsap_model.large_problem(rng), bool(n % 2)) for n in range(300))
    assert wrong == 0


def test_installed_scipy_agrees_with_the_golden_file():
    wrong = [n for n, (cost, mx, r, c) in enumerate(golden_problems())
             if not all(map(np.array_equal, linear_sum_assignment(cost, maximize=mx), (r, c)))]
    recorded = str(np.load(GOLDEN)["scipy_version"])
    assert not wrong, (f"scipy {scipy.__version__} breaks ties differently from scipy {recorded}, which recorded "
                       f"tests/golden/lsap_v1.npz: {len(wrong)} problems, the first is number {wrong[0]}")


def test_model_equals_the_golden_file():
    problems = golden_problems()
    assert len(problems) == 2040
    shapes = {(c.shape[0] < c.shape[1], c.shape[0] > c.shape[1], mx) for c, mx, _, _ in problems}
    assert {(True, False, False), (True, False, True), (False, True, False), (False, True, True)} <= shapes
    for n, (cost, mx, r, c) in enumerate(problems):
        got = lsap_model.solve(cost, maximize=mx)
        assert np.array_equal(got[0], r) and np.array_equal(got[1], c), n


def test_model_refusals_and_forbidden_pairs():
    with pytest.raises(ValueError, match="invalid numeric entries"):
        lsap_model.solve([[0.0, np.nan], [1.0, 2.0]])
    with pytest.raises(ValueError, match="invalid numeric entries"):
        lsap_model.solve([[0.0, np.inf], [1.0, 2.0]], maximize=True)
    with pytest.raises(ValueError, match="infeasible"):
        lsap_model.solve([[np.inf, 1.0], [np.inf, 2.0]])
    cost = np.array([[np.inf, 1.0, 2.0], [3.0, np.inf, 1.0], [1.0, 1.0, np.inf]])
    assert _same(cost, False) and _same(-cost, True) and _same(cost[:2], False) and _same(cost[:, :2], False)
    assert all(len(x) == 0 for x in lsap_model.solve(np.zeros((0, 3))))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("cost_func", ["mse", "mae"])
@pytest.mark.parametrize("shape", [(589, 3, 3), (293, 4, 7), (64, 1, 5), (17, 7, 2), (1, 2, 2), (100, 5, 1),
                                   (2000, 8, 8)])
def test_pair_cost_model_equals_pair_costs(dtype, cost_func, shape):
    from pyannote_audio_amd.permutation import _pair_costs
    frames, c1, c2 = shape
    rng = np.random.default_rng(frames + c1)
    a = rng.standard_normal((frames, c1)).astype(dtype)
    b = rng.standard_normal((frames, c2)).astype(dtype)
    a[:, 0] = 0
    want = _pair_costs(a, b, cost_func)
    got = lsap_model.pair_costs(a, b, cost_func)
    assert got.dtype == want.dtype == dtype and np.array_equal(got, want)
    padded = lsap_model.padded_costs(a, b, cost_func)
    assert padded.dtype == np.float64 and padded.shape == (max(c1, c2), c2)
    assert np.array_equal(padded[:c1], want.astype(np.float64))
    if c2 > c1:
        assert (padded[c1:] == np.float64(want.max() + 1)).all()


def test_host_route_of_linear_sum_assignment_batch():
    """host arrays and host tensors take a SciPy loop with the outputs of the device route: masks, totals, status"""
    import torch
    from pyannote_audio_amd.distance import linear_sum_assignment_batch
    rng = np.random.default_rng(3)
    batch = rng.integers(0, 3, (6, 5, 7)).astype(np.float64) + 0.1
    rows, cols = rng.random((6, 5)) < 0.7, rng.random((6, 7)) < 0.7
    rows[0], cols[1] = False, False
    for maximize in (False, True):
        col4row, total = linear_sum_assignment_batch(batch, maximize=maximize, row_mask=rows, col_mask=cols,
                                                     return_total=True)
        assert col4row.dtype == np.int32 and col4row.shape == (6, 5) and total.shape == (6,)
        for b in range(6):
            row_of, col_of = np.flatnonzero(rows[b]), np.flatnonzero(cols[b])
            r, c = linear_sum_assignment(batch[b][row_of][:, col_of], maximize=maximize)
            want = np.full(5, -1)
            want[row_of[r]] = col_of[c]
            assert np.array_equal(col4row[b], want)
            assert total[b] == sum((batch[b, i, j] for i, j in zip(row_of[r], col_of[c])), 0.0)
        assert (col4row[0] == -1).all() and (col4row[1] == -1).all() and total[0] == total[1] == 0.0
    as_tensor = linear_sum_assignment_batch(torch.from_numpy(batch))
    assert isinstance(as_tensor, torch.Tensor) and as_tensor.dtype == torch.int32
    assert np.array_equal(as_tensor.numpy(), np.stack([linear_sum_assignment(m)[1] for m in batch]))
    batch[2, 0, 0], batch[4, :, 1:] = np.nan, np.inf
    col4row, status = linear_sum_assignment_batch(batch, check=False)
    assert status.tolist() == [0, 0, 1, 0, 2, 0] and (col4row[[2, 4]] == -1).all() and (col4row[3] >= 0).all()
    with pytest.raises(ValueError, match=r"matrix contains invalid numeric entries \(problem 2 "):
        linear_sum_assignment_batch(batch)
    with pytest.raises(ValueError, match=r"cost matrix is infeasible \(problem 1 "):
        linear_sum_assignment_batch(batch[3:])
