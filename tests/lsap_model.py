"""Restatement of `scipy.optimize.linear_sum_assignment` (the shortest-augmenting-path solver of Crouse, 2016), step
for step and tie for tie, and of the cost matrix `permutation._pair_costs` builds: what `pa_lsap_batch` and
`pa_pair_costs` (csrc/lsap.hip) are held to.  tests/test_lsap_model_cpu.py holds this file to the installed SciPy and
numpy with `==`; the GPU tests hold the kernels to SciPy, to the golden file and to this model.

Only additions, subtractions and comparisons of doubles occur in `solve`, in the order written, so a kernel that does
the same operations returns the same bits.  Two properties of the inner scan decide every tie:
  * among the columns at the minimum it picks the unassigned one with the LARGEST scan position if any is unassigned,
    otherwise the one with the SMALLEST scan position;
  * `remaining` is permuted by the swap-removal, so the scan position of a column is state that is carried."""
import os

import numpy as np

INF = float("inf")


class Infeasible(ValueError):
    pass


def solve(cost, maximize: bool = False):
    """-> (row_ind, col_ind) int64 arrays, as `linear_sum_assignment(cost, maximize)` returns them"""
    cost = np.asarray(cost, dtype=np.float64)
    if cost.ndim != 2:
        raise ValueError("expected a matrix")
    nr, nc = cost.shape
    if nr == 0 or nc == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    transposed = nc < nr
    if transposed:
        cost = cost.T
        nr, nc = nc, nr
    if maximize:
        cost = -cost
    if np.isnan(cost).any() or (cost == -INF).any():
        raise ValueError("matrix contains invalid numeric entries")
    c = cost.tolist()
    u, v = [0.0] * nr, [0.0] * nc
    col4row, row4col = [-1] * nr, [-1] * nc
    path = [-1] * nc
    for cur in range(nr):
        min_val, i = 0.0, cur
        remaining = [nc - 1 - it for it in range(nc)]
        num = nc
        SR, SC = [False] * nr, [False] * nc
        spc = [INF] * nc
        sink = -1
        while sink == -1:
            index, lowest = -1, INF
            SR[i] = True
            row, ui = c[i], u[i]
            for it in range(num):
                j = remaining[it]
                r = ((min_val + row[j]) - ui) - v[j]
                if r < spc[j]:
                    path[j] = i
                    spc[j] = r
                if spc[j] < lowest or (spc[j] == lowest and row4col[j] == -1):
                    lowest = spc[j]
                    index = it
            min_val = lowest
            if min_val == INF:
                raise Infeasible("cost matrix is infeasible")
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            num -= 1
            remaining[index] = remaining[num]
        u[cur] += min_val
        for i in range(nr):
            if SR[i] and i != cur:
                u[i] += min_val - spc[col4row[i]]
        for j in range(nc):
            if SC[j]:
                v[j] -= min_val - spc[j]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if transposed:
        order = np.argsort(np.array(col4row), kind="stable")
        return np.array(col4row, dtype=np.int64)[order], np.arange(nr, dtype=np.int64)[order]
    return np.arange(nr, dtype=np.int64), np.array(col4row, dtype=np.int64)


def pair_costs(a, b, cost_func: str = "mse"):
    """(frames, C1), (frames, C2) of one float dtype -> (C1, C2) in that dtype: the frames are added one after the
    other from frame 0, in the input dtype, the product rounded before the addition, then ONE division by the number
    of frames in that dtype.  Equals `np.mean(diff * diff, axis=0)` bit for bit except for C1 * C2 == 1, where numpy
    adds pairwise."""
    a, b = np.asarray(a), np.asarray(b)
    dtype = np.result_type(a.dtype, b.dtype)
    acc = np.zeros((a.shape[1], b.shape[1]), dtype=dtype)
    for f in range(a.shape[0]):
        diff = (a[f][:, None] - b[f][None, :]).astype(dtype)
        acc = acc + (np.abs(diff) if cost_func == "mae" else diff * diff)
    return acc / dtype.type(a.shape[0])


def padded_costs(a, b, cost_func: str = "mse"):
    """the float64 (max(C1, C2), C2) matrix `permutate` hands to the solver: `pair_costs`, and for C2 > C1 the dummy
    rows of `cost.max() + 1`, maximum and sum taken in the input dtype"""
    cost = pair_costs(a, b, cost_func)
    c1, c2 = cost.shape
    if c2 > c1:
        cost = np.concatenate([cost, np.full((c2 - c1, c2), cost.max() + 1, dtype=cost.dtype)], axis=0)
    return cost.astype(np.float64)


# ------------------------------------------------------------------------------------------- seeded families
def small_problem(rng, kind: int):
    """one rectangular problem of 1..12 x 1..12 of family `kind` (0..3): heavy-tie integers 0..2, sparse non-negative,
    continuous, duplicated rows with zero columns"""
    nr, nc = int(rng.integers(1, 13)), int(rng.integers(1, 13))
    if kind == 0:
        return rng.integers(0, 3, (nr, nc)).astype(np.float64)
    if kind == 1:
        return np.where(rng.random((nr, nc)) < 0.6, 0.0, rng.integers(1, 6, (nr, nc)) * 0.25)
    if kind == 2:
        return rng.standard_normal((nr, nc))
    base = rng.integers(0, 4, (nr, nc)).astype(np.float64)
    base[rng.integers(0, nr, nr)] = base[rng.integers(0, nr, nr)]
    base[:, rng.random(nc) < 0.3] = 0.0
    return base


def large_problem(rng):
    """20..64 x 20..64, integer costs 0..4"""
    nr, nc = int(rng.integers(20, 65)), int(rng.integers(20, 65))
    return rng.integers(0, 5, (nr, nc)).astype(np.float64)


# ------------------------------------------------------------------------------------------- the golden file
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lsap_v1.npz")


def golden_problems():
    """[(float64 cost, maximize, row_ind, col_ind)] of the golden file"""
    z = np.load(GOLDEN)
    out = []
    for n, (nr, nc) in enumerate(z["shape"].astype(int)):
        cost = z["cost"][z["cost_offset"][n]:z["cost_offset"][n + 1]].reshape(nr, nc).astype(np.float64)
        lo, hi = z["pair_offset"][n], z["pair_offset"][n + 1]
        out.append((cost, bool(z["maximize"][n]), z["row_ind"][lo:hi].astype(np.int64),
                    z["col_ind"][lo:hi].astype(np.int64)))
    return out
