"""float64 distance kernels for clustering: GPU (`pa_pdist_f64`, `pa_pdist_cosine_f64`, `pa_cdist_cosine_f64`) with
results bit-identical to SciPy's `pdist(X, "euclidean")` / `pdist(X, "cosine")` / `cdist(A, B, "cosine")`, and the
dendrograms on top of them (`linkage_centroid`, `linkage_chain`), bit-identical to SciPy's `linkage`.

SciPy computes Euclidean distances as a sequential-k sum of (u_k - v_k)^2 in double without FMA
contraction, then sqrt; cosine as 1 - <u,v> / (|u| |v|) with sequential dot products.  The kernels
reproduce that summation order with explicit `__dmul_rn/__dadd_rn` (see csrc/cluster.hip).  Small
problems stay in SciPy: the launch + copy overhead exceeds the work."""
from __future__ import annotations

import os
import time

import numpy as np
import torch
from scipy.spatial.distance import cdist as _scipy_cdist
from scipy.spatial.distance import pdist as _scipy_pdist

from . import ffi

def _use_gpu(device, n: int) -> bool:
    """GPU kernels whenever the clustering object lives on a GPU (`pipeline.to(cuda)`); a missing library on a GPU
    device raises -- no silent downgrade there.  A clustering object that was never placed (device None) or that
    its user put on the host is the reference's stand-alone use (`AgglomerativeClustering().instantiate(...)(
    embeddings, ...)`, pipelines/clustering.py:214-289) and calls SciPy, i.e. the reference's own implementation
    of these two functions; the PIPELINE never gets there: SpeakerDiarization._require_device refuses to run
    anywhere but on a GPU."""
    kind = getattr(device, "type", None)
    if kind == "cuda":
        ffi.require_gpu()
        return n >= 2
    return False


@ffi.on_device(lambda X, device=None: device)
def pdist_euclidean(X: np.ndarray, device=None) -> np.ndarray:
    """condensed float64 Euclidean distance matrix of the rows of X (any float dtype)."""
    n = X.shape[0]
    if not _use_gpu(device, n):
        return _scipy_pdist(X, metric="euclidean")
    lib = ffi.load()
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(device)
    out = torch.empty(n * (n - 1) // 2, dtype=torch.float64, device=device)
    ffi.check(lib.pa_pdist_f64(ffi.ptr(Xd), n, X.shape[1], ffi.ptr(out), ffi.stream()), "pa_pdist_f64")
    return out.cpu().numpy()


@ffi.on_device(lambda X, rows, labels, num_segments, device: device)
def centroid_means(X: torch.Tensor, rows: np.ndarray, labels: np.ndarray, num_segments: int, device) -> np.ndarray:
    """means of the rows X[rows] per label 0..num_segments-1 on the GPU (`pa_centroid_means`), bit-identical to
    `np.vstack([np.mean(X[rows][labels == k], axis=0) for k in range(num_segments)])` (pipelines/clustering.py:
    182-187): ONE stable sort groups the row numbers (original order kept inside a cluster), the kernel adds the
    rows of a cluster top to bottom in float32 and divides in float32.  `X`: (., D) float32 tensor on `device`
    (the embeddings never leave HBM for this); an empty cluster yields NaN."""
    ffi.require_gpu()
    lib = ffi.load()
    if X.dtype != torch.float32 or not X.is_contiguous():
        raise ValueError("centroid_means: X must be a contiguous float32 tensor")
    order = np.argsort(labels, kind="stable")
    counts = np.bincount(labels, minlength=num_segments)[:num_segments]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    grouped = np.ascontiguousarray(np.asarray(rows)[order], dtype=np.int32)
    D = X.shape[1]
    rows_d = torch.from_numpy(grouped).to(device)
    offs_d = torch.from_numpy(offsets).to(device)
    out = torch.empty((num_segments, D), dtype=torch.float32, device=device)
    ffi.check(lib.pa_centroid_means(ffi.ptr(X), D, ffi.ptr(rows_d), ffi.ptr(offs_d), num_segments, ffi.ptr(out),
                                    ffi.stream()), "pa_centroid_means")
    return out.cpu().numpy()


@ffi.on_device(lambda X, device: device)
def linkage_centroid(X: np.ndarray, device) -> np.ndarray:
    """scipy.cluster.hierarchy.linkage(X, method="centroid", metric="euclidean") entirely on the GPU:
    float64 pdist (`pa_pdist_f64`) feeds the persistent merge kernels (`pa_linkage_centroid_f64`: the heap-free
    merge of csrc/linkage_fast.hip, then -- only if two rows ever tied for the smallest lower bound -- the exact
    heap replay of csrc/linkage.hip) without leaving HBM; only the (n-1, 4) dendrogram comes back.  Bit-identical
    to SciPy."""
    n = X.shape[0]
    ffi.require_gpu()
    lib = ffi.load()
    global last_linkage_stats, last_linkage_phases
    timed = os.environ.get("PA_LINKAGE_TIMING") == "1"   # development: where the wall time of a call goes
    marks = [("start", time.perf_counter())]

    host_only = os.environ.get("PA_LINKAGE_EVENTS") == "1"   # host clock at every step WITHOUT synchronising

    def mark(name):
        if timed:
            torch.cuda.synchronize(device)
        if timed or host_only:
            marks.append((name, time.perf_counter()))

    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(device)
    cond = torch.empty(n * (n - 1) // 2, dtype=torch.float64, device=device)
    mark("upload + allocate condensed")
    ffi.check(lib.pa_pdist_f64(ffi.ptr(Xd), n, X.shape[1], ffi.ptr(cond), ffi.stream()), "pa_pdist_f64")
    mark("pdist")
    Z = torch.empty((n - 1, 4), dtype=torch.float64, device=device)
    ws = torch.empty(lib.pa_linkage_workspace_bytes(n), dtype=torch.uint8, device=device)
    mark("allocate workspace")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if os.environ.get("PA_LINKAGE_EVENTS") == "1" else None
    if ev:
        ev[0].record()
    ffi.check(lib.pa_linkage_centroid_f64(ffi.ptr(cond), n, ffi.ptr(Z), ffi.ptr(ws), ws.numel(), ffi.stream()),
              "pa_linkage_centroid_f64")
    if ev:
        ev[1].record()
    mark("merge kernels")
    if ev:   # development: device time of the merge kernels without changing what the host does around them
        ev[1].synchronize()
        last_linkage_phases = [("host: " + b[0], b[1] - a[1]) for a, b in zip(marks, marks[1:])] + [
            ("whole call until the events are done", time.perf_counter() - marks[0][1]),
            ("merge kernels (events)", ev[0].elapsed_time(ev[1]) / 1e3)]
    if timed:
        last_linkage_phases = [(b[0], b[1] - a[1]) for a, b in zip(marks, marks[1:])]
    # development counters: [0:8] heap kernel (csrc/linkage.hip; all zero when the heap-free merge completed the
    # dendrogram), [8:16] heap-free merge (csrc/linkage_fast.hip): status (0 = complete, 1 = tie -> heap, 2 =
    # degenerate input -> heap, 3 = a workgroup
    # never showed up -> heap), lower-bound repairs, cycles in pop / pass, n, workgroups, re-publishes, merges done
    last_linkage_stats = ws[-128:].view(torch.int64).cpu().numpy()
    return Z.cpu().numpy()


last_linkage_stats = None
last_linkage_phases = None


# PA_LINKAGE_* of include/pyannote_amd.h: the methods of csrc/linkage_chain.hip
# (all five beat the former pdist + download + SciPy path at n = 7 176: profiles/linkage_methods_timing.txt)
CHAIN_METHODS = {"single": 0, "complete": 1, "average": 2, "weighted": 3, "ward": 4}



def linkage_finish(raw: np.ndarray, n: int, single: bool = False) -> np.ndarray:
    """SciPy's dendrogram from the unsorted merge list of `nn_chain` / `mst_single_linkage` (`pa_linkage_chain_f64`):
    the stable sort of the rows by height, then `_hierarchy.label` -- a union-find over the sorted rows that names
    every merge by the two current roots of its entries (smaller first), joins them under the new id n + i and
    recomputes the size column.  `single`: the rows come from the single-linkage kernel, which leaves the fourth
    column unused and writes 0 there -- anything else means the rows are not what the caller says they are.
    Host work: O(n log n) plus n - 1 union-find steps."""
    raw = np.asarray(raw, dtype=np.float64).reshape(n - 1, 4)
    if single and raw[:, 3].any():
        raise ValueError("linkage_finish: single-linkage merges carry 0 in their fourth column")
    Z = raw[np.argsort(raw[:, 2], kind="mergesort")]
    parent = list(range(2 * n - 1))
    size = [1] * (2 * n - 1)
    left, right = Z[:, 0].astype(np.int64).tolist(), Z[:, 1].astype(np.int64).tolist()
    ids = np.empty((n - 1, 2), dtype=np.float64)
    sizes = np.empty(n - 1, dtype=np.float64)

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:      # path compression
            parent[x], x = root, parent[x]
        return root

    for i in range(n - 1):
        a, b = find(left[i]), find(right[i])
        if a > b:
            a, b = b, a
        ids[i, 0], ids[i, 1] = a, b
        parent[a] = parent[b] = n + i
        size[n + i] = size[a] + size[b]
        sizes[i] = size[n + i]
    Z[:, :2] = ids
    Z[:, 3] = sizes
    return Z


@ffi.on_device(lambda X, method, metric, device, raw=None: device)
def linkage_chain(X: np.ndarray, method: str, metric: str, device, raw: torch.Tensor = None):
    """scipy.cluster.hierarchy.linkage(pdist(X, metric), method) for method in CHAIN_METHODS and metric "euclidean" or
    "cosine", on the GPU: float64 pdist (`pa_pdist_f64` / `pa_pdist_cosine_f64`), SciPy's finite check
    (`pa_nonfinite_flag_f64`) and the persistent merge kernel (`pa_linkage_chain_f64`) without leaving HBM; the
    32 (n - 1) bytes of the unsorted merge list come back and `linkage_finish` sorts and labels them.  Bit-identical
    to SciPy.  Returns None when the square copy of the matrix exceeds PA_LINKAGE_FAST_MAX_GB (the caller keeps the
    host path).  `raw`: see `linkage_chain_condensed`."""
    n = X.shape[0]
    if method not in CHAIN_METHODS or metric not in ("euclidean", "cosine") or n < 2:
        raise ValueError(f"linkage_chain: method {method!r}, metric {metric!r}, {n} points")
    ffi.require_gpu()
    lib = ffi.load()
    ws_bytes = lib.pa_linkage_chain_workspace_bytes(n)
    if ws_bytes == 0:
        return None
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(device)
    cond = torch.empty(n * (n - 1) // 2, dtype=torch.float64, device=device)
    if metric == "cosine":
        norms = torch.empty(n, dtype=torch.float64, device=device)
        ffi.check(lib.pa_pdist_cosine_f64(ffi.ptr(Xd), n, X.shape[1], ffi.ptr(cond), ffi.ptr(norms), ffi.stream()),
                  "pa_pdist_cosine_f64")
    else:
        ffi.check(lib.pa_pdist_f64(ffi.ptr(Xd), n, X.shape[1], ffi.ptr(cond), ffi.stream()), "pa_pdist_f64")
    flag = torch.empty(1, dtype=torch.int32, device=device)
    ffi.check(lib.pa_nonfinite_flag_f64(ffi.ptr(cond), cond.numel(), ffi.ptr(flag), ffi.stream()),
              "pa_nonfinite_flag_f64")
    if int(flag.item()) != 0:
        # scipy.cluster.hierarchy.linkage validates its condensed input the same way
        raise ValueError("The condensed distance matrix must contain only finite values.")
    return linkage_chain_condensed(cond, n, method, device, raw)


def linkage_chain_condensed(cond: torch.Tensor, n: int, method: str, device, raw: torch.Tensor = None) -> np.ndarray:
    """the merge of `linkage_chain` for a finite condensed float64 matrix that already lives on `device` (left
    intact); `raw`: where the (n - 1, 4) merge list goes on the device (allocated when None)."""
    lib = ffi.load()
    if raw is None:
        raw = torch.empty((n - 1, 4), dtype=torch.float64, device=device)
    ws = torch.empty(lib.pa_linkage_chain_workspace_bytes(n), dtype=torch.uint8, device=device)
    ffi.check(lib.pa_linkage_chain_f64(ffi.ptr(cond), n, CHAIN_METHODS[method], ffi.ptr(raw), ffi.ptr(ws), ws.numel(),
                                       ffi.stream()), "pa_linkage_chain_f64")
    # the merge list and the status word (first int of the workspace) in ONE synchronising copy
    packed = torch.cat([raw.reshape(-1), ws[:8].view(torch.float64)]).cpu().numpy()
    merges, status = packed[:-1], int(packed[-1:].view(np.int32)[0])
    if status != 0:
        raise RuntimeError(f"pa_linkage_chain_f64: the merge kernel ended with status {status} "
                           "(1: chain bound exceeded, 2: no neighbour found, -1: it did not run to its end)")
    return linkage_finish(merges, n, single=method == "single")


@ffi.on_device(lambda A, B, metric="cosine", device=None: device)
def cdist(A, B: np.ndarray, metric: str = "cosine", device=None) -> np.ndarray:
    """`A`: host array, or a tensor that already lives on `device` (converted to float64 there)."""
    on_device = isinstance(A, torch.Tensor)
    if metric != "cosine" or not _use_gpu(device, A.shape[0]):
        return _scipy_cdist(A.cpu().numpy() if on_device else A, B, metric=metric)
    lib = ffi.load()
    if on_device:
        Ad = A.to(device=device, dtype=torch.float64).contiguous()
    else:
        Ad = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64)).to(device)
    Bd = torch.from_numpy(np.ascontiguousarray(B, dtype=np.float64)).to(device)
    out = torch.empty((A.shape[0], B.shape[0]), dtype=torch.float64, device=device)
    norms = torch.empty(A.shape[0] + B.shape[0], dtype=torch.float64, device=device)
    ffi.check(lib.pa_cdist_cosine_f64(ffi.ptr(Ad), A.shape[0], ffi.ptr(Bd), B.shape[0], A.shape[1],
                                      ffi.ptr(out), ffi.ptr(norms), ffi.stream()), "pa_cdist_cosine_f64")
    return out.cpu().numpy()


#: what SciPy says when it refuses a matrix, by status of `pa_lsap_batch`
LSAP_REFUSALS = {1: "matrix contains invalid numeric entries", 2: "cost matrix is infeasible"}


def _bit_masks(mask, batch: int, size: int, device):
    """None or a (batch, size) boolean table -> None or the (batch,) 64-bit masks of `pa_lsap_batch`, as an int64
    device tensor"""
    if mask is None:
        return None
    mask = torch.as_tensor(mask).to(device)
    if mask.dtype != torch.bool or mask.shape != (batch, size):
        raise ValueError(f"expected a boolean mask of shape {(batch, size)}, got {mask.dtype} {tuple(mask.shape)}")
    weights = torch.ones(size, dtype=torch.int64, device=device) << torch.arange(size, device=device)
    return (mask.to(torch.int64) * weights).sum(dim=1).contiguous()     # (bit 63 wraps to the sign: the same bits)


def _lsap_host(cost: np.ndarray, maximize: bool, row_mask, col_mask):
    """the SciPy loop with the outputs of `pa_lsap_batch`"""
    from scipy.optimize import linear_sum_assignment
    B, R, Cn = cost.shape
    col4row = np.full((B, R), -1, dtype=np.int32)
    total, status = np.zeros(B), np.zeros(B, dtype=np.uint8)
    for b in range(B):
        rows = np.flatnonzero(row_mask[b]) if row_mask is not None else np.arange(R)
        cols = np.flatnonzero(col_mask[b]) if col_mask is not None else np.arange(Cn)
        try:
            r, c = linear_sum_assignment(cost[b][rows][:, cols], maximize=maximize)
        except ValueError as error:
            status[b] = 2 if "infeasible" in str(error) else 1
            continue
        col4row[b, rows[r]] = cols[c]
        total[b] = sum((float(cost[b, i, j]) for i, j in zip(rows[r], cols[c])), 0.0)
    return col4row, total, status


@ffi.on_device(lambda cost, *args, **kwargs: getattr(cost, "device", None))
def linear_sum_assignment_batch(cost, maximize: bool = False, row_mask=None, col_mask=None,
                                return_total: bool = False, check: bool = True):
    """`scipy.optimize.linear_sum_assignment(cost[b], maximize)` for every matrix of a (B, R, C) float64 batch, with
    SciPy's own choice among equal optima (`pa_lsap_batch`, csrc/lsap.hip).
    `cost`: a `cuda` tensor of any strides (a transposed view costs nothing) runs ONE launch and returns device tensors;
    R, C <= 64 there.  `row_mask`, `col_mask`: (B, R) / (B, C) boolean tables: problem b is the submatrix of the
    rows and columns that are set.  -> `col4row` (B, R) int32, the column of every row, -1 for a row that is
    masked out or left unassigned; with `return_total` also `total` (B,) float64, cost[r][col4row[r]] added in
    ascending r.  `check=True` downloads the B status bytes and raises SciPy's `ValueError` for the first problem it
    would refuse; `check=False` appends the (B,) uint8 status (0 solved, 1 invalid entry, 2 infeasible) instead.
    A host array or host tensor takes a SciPy loop and returns arrays of its own kind."""
    on_device = isinstance(cost, torch.Tensor) and cost.is_cuda
    if cost.ndim != 3:
        raise ValueError(f"expected a (B, R, C) batch of matrices, got shape {tuple(cost.shape)}")
    B, R, Cn = cost.shape
    if on_device:
        if cost.dtype != torch.float64:
            raise ValueError(f"expected float64 costs, got {cost.dtype}")
        lib = ffi.load()
        limit = int(lib.pa_lsap_max_size())
        if R > limit or Cn > limit:
            raise ValueError(f"at most {limit} rows and columns on the device, got {R} x {Cn}")
        dev = cost.device
        rm, cm = _bit_masks(row_mask, B, R, dev), _bit_masks(col_mask, B, Cn, dev)
        col4row = torch.empty((B, R), dtype=torch.int32, device=dev)
        total = torch.empty(B, dtype=torch.float64, device=dev) if return_total else None
        status = torch.empty(B, dtype=torch.uint8, device=dev)
        sb, sr, sc = cost.stride()
        ffi.check(lib.pa_lsap_batch(ffi.C.c_void_p(cost.data_ptr()), sb, sr, sc, B, R, Cn, ffi.ptr(rm), ffi.ptr(cm),
                                    int(bool(maximize)), ffi.ptr(col4row), ffi.ptr(total), ffi.ptr(status),
                                    ffi.stream()), "pa_lsap_batch")
        host_status = status.cpu().numpy() if check else None
    else:
        as_torch = isinstance(cost, torch.Tensor)
        array = cost.detach().numpy() if as_torch else np.asarray(cost)

        tables = [None if mask is None else np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask, dtype=bool)
                  for mask in (row_mask, col_mask)]
        col4row, total, status = _lsap_host(array.astype(np.float64, copy=False), bool(maximize), *tables)
        host_status = status
        if as_torch:
            col4row, total, status = (torch.from_numpy(x) for x in (col4row, total, status))
    if check and host_status.any():
        first = int(np.flatnonzero(host_status)[0])
        raise ValueError(f"{LSAP_REFUSALS[int(host_status[first])]} (problem {first} of the batch)")
    out = (col4row,) + ((total,) if return_total else ()) + (() if check else (status,))
    return out[0] if len(out) == 1 else out


#: Lloyd iterations enqueued between two reads of the done flags (`pa_kmeans_f64`; 0: all `max_iter` at once, no
#: read-back).  The choice is measured in profiles/kmeans_timing.txt.
KMEANS_ROUND_ITERATIONS = 8


def kmeans_draws(n: int, num_clusters: int, n_init: int, random_state: int):
    """the random draws of sklearn's k-means++ for `n_init` initialisations, in its order of consumption from one
    `RandomState(random_state)`: first (n_init) int32 = the first centre's row, uniforms (n_init, K - 1, T) float64 with
    T = 2 + int(log(K)).  None of them depends on the data."""
    rs = np.random.RandomState(random_state)
    T = 2 + int(np.log(num_clusters))
    first = np.empty(n_init, dtype=np.int32)
    uniforms = np.empty((n_init, num_clusters - 1, T), dtype=np.float64)
    weights = np.ones(n) / n
    for i in range(n_init):
        first[i] = rs.choice(n, p=weights)
        for c in range(num_clusters - 1):
            uniforms[i, c] = rs.uniform(size=T)
    return first, uniforms


def kmeans_select(labels: np.ndarray, inertia: np.ndarray, num_clusters: int) -> int:
    """the initialisation `KMeans.fit` keeps: the first, replaced by a later one only if its inertia is smaller AND its
    labelling is not the same partition under a renaming (sklearn's `_is_same_clustering`)"""
    best = 0
    for i in range(1, len(labels)):
        if not inertia[i] < inertia[best]:
            continue
        # the same partition <=> the pairs (label here, label there) pair every label with exactly one other
        pairs = np.unique(labels[i].astype(np.int64) * num_clusters + labels[best])
        if len(np.unique(pairs // num_clusters)) != len(pairs):
            best = i
    return best


@ffi.on_device(lambda X, num_clusters, device, **kw: device)
def kmeans(X: np.ndarray, num_clusters: int, device, n_init: int = 3, random_state: int = 42, max_iter: int = 300,
           tol: float = 1e-4, details: bool = False):
    """labels (N) int32 of `sklearn.cluster.KMeans(n_clusters=num_clusters, n_init=n_init, random_state=random_state,
    max_iter=max_iter, tol=tol).fit_predict` FOR THE SAME VALUES IN FLOAT64, numbering included, computed on the GPU
    (`pa_kmeans_f64`, csrc/kmeans.hip): the random draws are taken on the host (they do not depend on the data) and
    uploaded once, all initialisations run as jobs of one set of launches, and the choice among them is made here from
    ONE download.  float64 throughout with a fixed order of additions: bit-reproducible from call to call.  For float32
    rows scikit-learn computes in float32; where k-means over-splits a homogeneous cloud that rounding can move a
    few boundary points (KMeans section).
    None when the device route does not apply or gave up -- no CUDA device, a size outside the kernel's limits,
    non-finite rows, a cluster that comes up empty (sklearn then relocates points; not built here): the caller makes
    the sklearn call.  `details=True`: (labels, dict of the per-initialisation outputs `labels`, `centers`, `inertia`,
    `picks`, `status` and the winner's index `best`)."""
    X = np.asarray(X)
    n, dim = X.shape
    K, J = int(num_clusters), int(n_init)
    if getattr(device, "type", None) != "cuda" or not torch.cuda.is_available():
        return None
    if K == 1:
        labels = np.zeros(n, dtype=np.int32)
        return (labels, None) if details else labels
    lib = ffi.load()
    if J < 1 or max_iter < 1 or lib.pa_kmeans_workspace_bytes(n, dim, K, J) == 0 or not np.isfinite(X).all():
        return None
    first, uniforms = kmeans_draws(n, K, J, random_state)
    try:
        ws = torch.empty(lib.pa_kmeans_workspace_bytes(n, dim, K, J), dtype=torch.uint8, device=device)
    except torch.cuda.OutOfMemoryError:
        return None
    Xd = torch.from_numpy(np.ascontiguousarray(X)).to(device).to(torch.float64)
    first_d, uniforms_d = torch.from_numpy(first).to(device), torch.from_numpy(uniforms).to(device)
    # one buffer, one download: centres (J, K, D) and inertia (J) as doubles, then labels (J, n), picks (J, K) and
    # status (J, 4) as int32
    doubles, ints = J * K * dim + J, J * n + J * K + J * 4
    buffer = torch.zeros(doubles + (ints + 1) // 2, dtype=torch.float64, device=device)
    centers, inertia = buffer[:J * K * dim], buffer[J * K * dim:doubles]
    tail = buffer[doubles:].view(torch.int32)
    labels, picks, status = tail[:J * n], tail[J * n:J * n + J * K], tail[J * n + J * K:ints]
    ffi.check(lib.pa_kmeans_f64(ffi.ptr(Xd), n, dim, K, J, ffi.ptr(first_d), ffi.ptr(uniforms_d), int(max_iter),
                                float(tol), KMEANS_ROUND_ITERATIONS, ffi.ptr(labels), ffi.ptr(centers),
                                ffi.ptr(inertia), ffi.ptr(picks), ffi.ptr(status), ffi.ptr(ws), ws.numel(),
                                ffi.stream()), "pa_kmeans_f64")
    host = buffer.cpu().numpy()
    host_ints = host[doubles:].view(np.int32)
    out = {"centers": host[:J * K * dim].reshape(J, K, dim), "inertia": host[J * K * dim:doubles],
           "labels": host_ints[:J * n].reshape(J, n), "picks": host_ints[J * n:J * n + J * K].reshape(J, K),
           "status": host_ints[J * n + J * K:ints].reshape(J, 4)}
    if out["status"][:, 2:].any():      # an empty cluster or non-finite values: sklearn's call
        return None
    out["best"] = kmeans_select(out["labels"], out["inertia"], K)
    labels = out["labels"][out["best"]].copy()
    return (labels, out) if details else labels
