"""float64 numpy restatement of scikit-learn 1.7.2's dense `KMeans(init="k-means++", algorithm="lloyd")` with unit
sample weights, laid out like `pa_kmeans_f64` (csrc/kmeans.hip): the random draws are taken on the host before
anything else (they do not depend on the data), every initialisation is a job with its own labels, centres, inertia,
k-means++ picks and status, and the selection across initialisations runs afterwards.

Where the device sums in another order than numpy (per-block partial sums, butterflies) the VALUES differ in the last
bits; labels, picks, iteration counts and stop kinds are integers that only a knife edge could move, and
`knife_edges` measures how far an input stays from one.  No test compares floating-point bits with this model: the
centres are held to `math.fsum` means and the inertia to a relative bound (tests/test_kmeans_gpu.py)."""
import numpy as np

STRICT, TOL, MAX_ITER = 0, 1, 2      # status[1], the stop kinds of pa_kmeans_f64


def data(n, d, g, noise, seed, dtype):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((g, d))
    X = C[rng.integers(0, g, n)] + noise * rng.standard_normal((n, d))
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(dtype)


#: (n, d, g, k, noise), each with seeds 0..3 in float32 and float64
TABLE = [(97, 16, 3, 2, 1.2), (257, 24, 4, 3, 0.6), (300, 32, 4, 4, 0.6), (500, 24, 5, 8, 0.7),
         (1000, 64, 6, 5, 0.9), (640, 256, 4, 4, 0.8), (130, 256, 3, 5, 0.8)]
SEEDS = (0, 1, 2, 3)


def duplicate_points(dtype=np.float32):
    """60 rows taken from 3 distinct unit vectors: with k = 5 a cluster comes up empty"""
    rng = np.random.default_rng(7)
    P = rng.standard_normal((3, 16))
    P /= np.linalg.norm(P, axis=1, keepdims=True)
    return P[rng.integers(0, 3, 60)].astype(dtype)


def draws(n, k, n_init, seed):
    """(first (n_init) int32, uniforms (n_init, k - 1, T) float64) in sklearn's order of consumption"""
    rs = np.random.RandomState(seed)
    T = 2 + int(np.log(k))
    first = np.empty(n_init, dtype=np.int32)
    uniforms = np.empty((n_init, k - 1, T))
    for i in range(n_init):
        first[i] = rs.choice(n, p=np.ones(n) / n)
        for c in range(1, k):
            uniforms[i, c - 1] = rs.uniform(size=T)
    return first, uniforms


def _sqdist(X, rows):
    """(len(rows), n): |X - X[r]|^2 for every row r, as the sum of squared differences"""
    return np.stack([((X - X[r]) ** 2).sum(axis=1) for r in rows])


def plusplus(X, k, first, uniforms):
    """the k rows k-means++ picks (`_kmeans_plusplus`)"""
    n = len(X)
    picks = np.empty(k, dtype=np.int32)
    picks[0] = first
    closest = _sqdist(X, [first])[0]
    pot = closest.sum()
    for c in range(1, k):
        cand = np.minimum(np.searchsorted(np.cumsum(closest), uniforms[c - 1] * pot), n - 1)
        d = np.minimum(closest, _sqdist(X, cand))
        pots = d.sum(axis=1)
        best = int(np.argmin(pots))
        picks[c], closest, pot = cand[best], d[best], pots[best]
    return picks


def _assign(X, C):
    return np.argmin((C ** 2).sum(axis=1)[None, :] - 2.0 * (X @ C.T), axis=1).astype(np.int32)


def lloyd(X, C, max_iter, tolv):
    """-> labels, centres, inertia, iterations, stop kind, empty flag, the shifts of every iteration"""
    k = len(C)
    old = np.full(len(X), -1, dtype=np.int32)
    shifts, kind, empty = [], MAX_ITER, False
    labels = old
    for it in range(max_iter):
        labels = _assign(X, C)
        counts = np.bincount(labels, minlength=k)
        if (counts == 0).any():
            empty = True
            break
        new = np.stack([X[labels == j].sum(axis=0) / counts[j] for j in range(k)])
        shift = ((new - C) ** 2).sum()
        C = new
        if np.array_equal(labels, old):
            kind = STRICT
            break
        shifts.append(shift)
        if shift <= tolv:
            kind = TOL
            break
        old = labels
    if kind != STRICT and not empty:
        labels = _assign(X, C)
    inertia = ((X - C[labels]) ** 2).sum()
    return labels, C, inertia, it + 1, kind, empty, shifts


def same_clustering(a, b, k):
    """sklearn's `_is_same_clustering`: the same partition under a renaming"""
    mapping = np.full(k, -1, dtype=np.int64)
    for x, y in zip(a, b):
        if mapping[x] == -1:
            mapping[x] = y
        elif mapping[x] != y:
            return False
    return True


def select(labels, inertia, k):
    """index of the initialisation `KMeans.fit` keeps"""
    best = 0
    for i in range(1, len(labels)):
        if inertia[i] < inertia[best] and not same_clustering(labels[i], labels[best], k):
            best = i
    return best


def kmeans(X, k, n_init=3, seed=42, max_iter=300, tol=1e-4):
    """dict of per-initialisation arrays (labels, centers, inertia, picks, status (n_init, 4): iterations, stop kind,
    empty flag, non-finite flag), `best`, `tolv`, `shifts` per iteration, the centred rows `Xc` and their `mean`;
    centres in the caller's coordinates"""
    X64 = np.asarray(X, dtype=np.float64)
    n, d = X64.shape
    first, uniforms = draws(n, k, n_init, seed)
    mean = X64.mean(axis=0)
    Xc = X64 - mean
    tolv = tol * np.mean(np.var(Xc, axis=0))
    out = {"labels": np.empty((n_init, n), dtype=np.int32), "centers": np.empty((n_init, k, d)),
           "inertia": np.empty(n_init), "picks": np.empty((n_init, k), dtype=np.int32),
           "status": np.zeros((n_init, 4), dtype=np.int32), "tolv": tolv, "shifts": [], "Xc": Xc, "mean": mean}
    for i in range(n_init):
        picks = plusplus(Xc, k, first[i], uniforms[i])
        labels, C, inertia, iters, kind, empty, shifts = lloyd(Xc, Xc[picks].copy(), max_iter, tolv)
        out["labels"][i], out["centers"][i], out["inertia"][i], out["picks"][i] = labels, C + mean, inertia, picks
        out["status"][i] = (iters, kind, int(empty), 0)
        out["shifts"].append(shifts)
    out["empty"] = bool(out["status"][:, 2].any())
    out["best"] = None if out["empty"] else select(out["labels"], out["inertia"], k)
    return out


def knife_edges(model):
    """(smallest gap between a point's nearest and second-nearest final centre (squared distances) over all
    initialisations, smallest |shift / tolv - 1| over all iterations)"""
    Xc, gap = model["Xc"], np.inf
    for C in model["centers"]:
        d = ((Xc[:, None, :] - (C - model["mean"])[None]) ** 2).sum(axis=2)
        d.sort(axis=1)
        gap = min(gap, float((d[:, 1] - d[:, 0]).min()))
    ratio = min((abs(s / model["tolv"] - 1.0) for shifts in model["shifts"] for s in shifts), default=np.inf)
    return gap, ratio


#: shapes at the edges of the kernel's tiling (a workgroup owns 64 rows, a lane the columns lane, lane + 64, ...; the
#: block partial sums take the columns in chunks of 6144 // k): an odd D, N one below and one above the row block,
#: N == K, more than 256 columns, K = 64 with N = 200 and three column chunks.  Seed 0 each, in float32 and float64
#: (with N == K every potential of the last k-means++ steps is a sum of a few terms, and seed 1 in float64 draws a
#: candidate on which scikit-learn's |x|^2 - 2 x.y + |y|^2 and the plain squared difference part: another seed)
EXTRA = [(150, 19, 3, 3, 0.7), (63, 8, 2, 2, 0.8), (65, 8, 2, 2, 0.8), (12, 8, 3, 12, 0.8), (100, 300, 3, 3, 0.8),
         (200, 256, 8, 64, 0.8)]
EXTRA_SEEDS = (0,)
