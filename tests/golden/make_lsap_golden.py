"""Generator of tests/golden/lsap_v1.npz: tie-rich assignment problems as int8 costs with the assignments that the
installed `scipy.optimize.linear_sum_assignment` returns for them (results only).  2 000 problems of 1..12 x 1..12 and 40
of up to 64 x 64, wide and tall, minimised and maximised.

    python tests/golden/make_lsap_golden.py

Arrays: `shape` (N, 2) uint8; `maximize` (N) uint8; `cost` int8, the matrices row-major one after the other,
`cost_offset` (N + 1) int64; `row_ind`, `col_ind` uint8, the assignments one after the other, `pair_offset` (N + 1)
int64; `scipy_version`."""
import os

import numpy as np
import scipy
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL, LARGE = 2000, 40


def problems():
    rng = np.random.default_rng(20161)
    for n in range(SMALL):
        nr, nc = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        kind = n % 4
        if kind == 0:      # three values: ties everywhere
            cost = rng.integers(0, 3, (nr, nc))
        elif kind == 1:    # mostly zero
            cost = np.where(rng.random((nr, nc)) < 0.6, 0, rng.integers(1, 6, (nr, nc)))
        elif kind == 2:    # duplicated rows, constant columns (silent speakers)
            cost = rng.integers(0, 4, (nr, nc))
            cost[rng.integers(0, nr, nr)] = cost[rng.integers(0, nr, nr)]
            cost[:, rng.random(nc) < 0.3] = int(rng.integers(0, 3))
        else:              # signed
            cost = rng.integers(-3, 4, (nr, nc))
        yield cost.astype(np.int8), bool(rng.integers(0, 2))
    corners = [(64, 64), (64, 20), (20, 64), (1, 64), (64, 1), (63, 64), (64, 63), (33, 32)]
    for n in range(LARGE):
        nr, nc = corners[n] if n < len(corners) else (int(rng.integers(13, 65)), int(rng.integers(13, 65)))
        yield rng.integers(0, 5 if n % 2 else 2, (nr, nc)).astype(np.int8), bool(n // 2 % 2)


def main():
    shapes, maximize, costs, rows, cols = [], [], [], [], []
    for cost, mx in problems():
        r, c = linear_sum_assignment(cost.astype(np.float64), maximize=mx)
        shapes.append(cost.shape)
        maximize.append(mx)
        costs.append(cost.ravel())
        rows.append(r.astype(np.uint8))
        cols.append(c.astype(np.uint8))
    out = os.path.join(HERE, "lsap_v1.npz")
    np.savez_compressed(
        out, shape=np.array(shapes, dtype=np.uint8), maximize=np.array(maximize, dtype=np.uint8),
        cost=np.concatenate(costs), cost_offset=np.cumsum([0] + [len(c) for c in costs]).astype(np.int64),
        row_ind=np.concatenate(rows), col_ind=np.concatenate(cols),
        pair_offset=np.cumsum([0] + [len(r) for r in rows]).astype(np.int64), scipy_version=np.array(scipy.__version__))
    print(f"{out}: {len(shapes)} problems, {os.path.getsize(out)} bytes, scipy {scipy.__version__}")


if __name__ == "__main__":
    main()
