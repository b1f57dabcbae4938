"""Plain Python restatement of the two SciPy algorithms that csrc/linkage_chain.hip replays on the device:
`_hierarchy.nn_chain` (complete, average, weighted, ward) and `_hierarchy.mst_single_linkage` (single), both up to --
and not including -- the stable sort by height and `label()`, which are `distance.linkage_finish`.  They return the
unsorted merge list that `pa_linkage_chain_f64` returns: (n - 1, 4) float64 rows [x, y, height, size].

Python floats are IEEE doubles and every operator rounds on its own, so the update expressions below are SciPy's
arithmetic as written: left to right, integer sizes converted to double."""
import math

import numpy as np

INF = float("inf")


def square(y, n):
    """condensed -> list of rows (Python floats)"""
    S = np.zeros((n, n))
    S[np.triu_indices(n, 1)] = y
    return (S + S.T).tolist()


def update(method, a, b, c, nx, ny, ni):
    if method == "complete":
        return max(a, b)
    if method == "average":
        return (nx * a + ny * b) / (nx + ny)
    if method == "weighted":
        return 0.5 * (a + b)
    if method == "ward":
        t = 1.0 / (nx + ny + ni)
        return math.sqrt((ni + nx) * t * a * a + (ni + ny) * t * b * b - ni * t * c * c)
    raise ValueError(method)


def nn_chain(y, n, method):
    D = square(y, n)
    size = [1] * n
    chain = []
    raw = np.zeros((n - 1, 4))
    for k in range(n - 1):
        if not chain:
            chain.append(next(i for i in range(n) if size[i] > 0))
        while True:
            x = chain[-1]
            if len(chain) > 1:
                nearest, cur = chain[-2], D[x][chain[-2]]
            else:
                nearest, cur = None, INF
            row = D[x]
            for i in range(n):
                if size[i] == 0 or i == x:
                    continue
                if row[i] < cur:
                    cur, nearest = row[i], i
            if len(chain) > 1 and nearest == chain[-2]:
                break
            chain.append(nearest)
        y_ = nearest
        del chain[-2:]
        if x > y_:
            x, y_ = y_, x
        nx, ny = size[x], size[y_]
        raw[k] = (x, y_, cur, nx + ny)
        size[x], size[y_] = 0, nx + ny
        for i in range(n):
            if size[i] == 0 or i == y_:
                continue
            D[i][y_] = D[y_][i] = update(method, D[i][x], D[i][y_], cur, nx, ny, size[i])
    return raw


def mst_single(y, n):
    D = square(y, n)
    dmin = [INF] * n
    merged = [False] * n
    raw = np.zeros((n - 1, 4))
    x = 0
    for k in range(n - 1):
        merged[x] = True
        cur, nearest = INF, None
        row = D[x]
        for i in range(n):
            if merged[i]:
                continue
            if dmin[i] > row[i]:
                dmin[i] = row[i]
            if dmin[i] < cur:
                nearest, cur = i, dmin[i]
        raw[k] = (x, nearest, cur, 0.0)
        x = nearest
    return raw


def raw_merges(y, n, method):
    return mst_single(y, n) if method == "single" else nn_chain(y, n, method)
