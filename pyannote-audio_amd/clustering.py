"""Embedding clustering back ends of the diarization pipeline (the b4 interface of SURVEY.md section 8b:
`Clustering[name].value(metric=...)(embeddings, segmentations, num_clusters, min_clusters,
max_clusters) -> (hard (C,S), soft (C,S,K), centroids (K,D))`, pipelines/clustering.py:44-763).

What runs where
  GPU (libpyannote_amd.so)   float64 pdist + the whole centroid-linkage merge (`distance.linkage_centroid`,
                             bit-identical to SciPy incl. ties), cosine cdist of every embedding to the
                             centroids, the PLDA projection and the VB iterations of VBx (one file: `_vbx`; the
                             candidates of a tuning sweep: `vbx_batch`), the constrained assignment of all chunks
                             for such a sweep (`constrained_argmax_device`), KMeans (`distance.kmeans`,
                             csrc/kmeans.hip: KMeansClustering and the forced speaker counts of VBx; scikit-learn's
                             labels for the same values in float64 -- float32 rows of an over-split cloud can differ
                             from the reference's float32 run in a few boundary points)
  host, SciPy / sklearn      `fcluster` on the (GPU-built) dendrogram, Hungarian assignment -- the very library
                             calls the reference makes, O(N) or tiny; KMeans only with `kmeans_on_device = False`,
                             off the GPU, or when the device route gives up (an empty cluster, sizes beyond its limits)
  host, this file            everything between those calls, organised around array operations instead
                             of the reference's per-cluster / per-iteration Python loops:
                               * `segment_means`: all cluster centroids from one stable sort (contiguous
                                 slices instead of K boolean masks), bit-identical to
                                 `np.mean(X[labels == k], axis=0)`; on a GPU the centroids of the final
                                 assignment come from `distance.centroid_means` (`pa_centroid_means`: the
                                 same sums in the same order on the embeddings that are still in HBM)
                               * `Dendrogram.large_cluster_counts`: the number of large clusters after
                                 EVERY merge from one O(N) scan of the merge sizes, which turns the
                                 reference's forced-number search (one `fcluster` per candidate cut,
                                 clustering.py:405-451) into a lookup + ONE `fcluster`
                               * `Dendrogram.cuts`: every candidate cut of one tree from one plan (built on
                                 the host by `pa_dendrogram_plan`), on a GPU by `pa_dendrogram_cuts` -- what
                                 tuning the threshold on a corpus asks for (tuning.py)
Arithmetic contract: embeddings are float32; the AHC training copy is
L2-normalised in float32; distances are float64 with SciPy's summation order; centroids are float32 row
sums in row order divided in float32.  Cluster ids are bit-identical to the reference's given identical
embeddings (oracle: oracle/pipeline.py, oracle/vbx.py hold the loop-for-loop restatement)."""
from __future__ import annotations

import time
import warnings
from enum import Enum
from typing import Callable, Optional, Tuple

import numpy as np
import torch
from scipy.cluster.hierarchy import fcluster, linkage
from scipy.spatial.distance import cdist as scipy_cdist

from . import distance
from .core import SlidingWindowFeature
from .pipeline import Categorical, Integer, Pipeline, Uniform


# ---------------------------------------------------------------------------------------------------
# array helpers
# ---------------------------------------------------------------------------------------------------
def segment_means(X: np.ndarray, labels: np.ndarray, num_segments: int) -> np.ndarray:
    """row means of X per label 0..num_segments-1, bit-identical to
    `np.vstack([np.mean(X[labels == k], axis=0) for k in range(num_segments)])`: ONE stable sort groups
    the rows (original order kept inside a segment), then each segment is a contiguous slice reduced by
    `np.add.reduce(axis=0)` -- numpy adds the rows of a C-contiguous block top to bottom in X's dtype,
    which is what `np.mean` does (`np.add.reduceat` and `np.add.at` do NOT keep that order) -- and divided
    in X's dtype.  An empty segment yields NaN."""
    order = np.argsort(labels, kind="stable")
    counts = np.bincount(labels, minlength=num_segments)[:num_segments]
    ends = np.cumsum(counts)
    grouped = X[order]
    out = np.full((num_segments, X.shape[1]), np.nan, dtype=X.dtype)
    for k in np.nonzero(counts)[0]:
        out[k] = np.add.reduce(grouped[ends[k] - counts[k]:ends[k]], axis=0) / X.dtype.type(counts[k])
    return out


def clamp_cluster_bounds(num_items: int, num_clusters, min_clusters, max_clusters
                         ) -> Tuple[Optional[int], int, int]:
    """resolve (num, min, max) against the number of items (clustering.py:54-75): an explicit number
    pins both bounds, both are clipped to [1, num_items], and equal bounds become an explicit number."""
    lo = min(num_items, num_clusters or min_clusters or 1)
    hi = min(num_items, num_clusters or max_clusters or num_items)
    lo, hi = max(1, lo), max(1, hi)
    if lo > hi:
        raise ValueError(f"min_clusters must be smaller than (or equal to) max_clusters "
                         f"(here: min_clusters={lo:g} and max_clusters={hi:g}).")
    return (lo if lo == hi else num_clusters), lo, hi


class Dendrogram:
    """(N-1, 4) SciPy linkage matrix with the two queries the pipeline needs."""

    def __init__(self, Z: np.ndarray):
        self.Z = Z
        self.num_leaves = Z.shape[0] + 1

    def cut(self, height: float) -> np.ndarray:
        """flat clusters at `height`, numbered like fcluster(..., "distance") - 1"""
        return fcluster(self.Z, height, criterion="distance") - 1

    def cut_after_merge(self, index: int) -> np.ndarray:
        """flat clusters once merges 0..index have been applied (heights replaced by their rank, which
        also removes the inversions centroid linkage can produce: clustering.py:407-410)"""
        ranked = self.Z.copy()
        ranked[:, 2] = np.arange(self.num_leaves - 1)
        return fcluster(ranked, index, criterion="distance") - 1

    def plan(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """what every cut of this tree shares (`pa_dendrogram_plan`, csrc/dendrogram_plan.h; built once): the nodes
        in the order in which SciPy hands out cluster numbers, each with the largest height of its subtree (-inf for a
        leaf), that of its parent (+inf for the root) and the first position of its leaves in left-first leaf order;
        and the position of every leaf."""
        cached = self.__dict__.get("_plan")
        if cached is None:
            from . import ffi
            n = self.num_leaves
            Z = np.ascontiguousarray(self.Z, dtype=np.float64)
            own, parent = np.empty(2 * n - 1), np.empty(2 * n - 1)
            lo, leaf_lo = np.empty(2 * n - 1, dtype=np.int32), np.empty(n, dtype=np.int32)
            ffi.check(ffi.load().pa_dendrogram_plan(Z.ctypes.data, n, own.ctypes.data, parent.ctypes.data,
                                                    lo.ctypes.data, leaf_lo.ctypes.data), "pa_dendrogram_plan")
            cached = self._plan = (own, parent, lo, leaf_lo)
        return cached

    def cuts(self, heights, device=None) -> np.ndarray:
        """(T, n) int32: row k = `fcluster(Z, heights[k], "distance") - 1`, numbering included, for all heights at
        once.  On a GPU `device`: `pa_dendrogram_cuts` (csrc/dendrogram.hip; the plan is uploaded once per tree and
        device); `device` None or the host: the same plan through numpy.  `last_num_clusters` (T) = clusters per row."""
        heights = np.ascontiguousarray(np.atleast_1d(np.asarray(heights, dtype=np.float64)).reshape(-1))
        if np.isnan(heights).any():
            raise ValueError("Dendrogram.cuts: a threshold is NaN")
        # (the root has no parent: its `parent_md` is +inf, which a threshold of +inf must still lie under)
        heights = np.minimum(heights, np.finfo(np.float64).max)
        T, n = len(heights), self.num_leaves
        if n == 1 or T == 0:
            self.last_num_clusters = np.ones(T, dtype=np.int32)
            return np.zeros((T, n), dtype=np.int32)
        if getattr(device, "type", None) == "cuda":
            return self._cuts_on_device(heights, device)
        own, parent, lo, leaf_lo = self.plan()
        labels = np.empty((T, n), dtype=np.int32)
        counts = np.empty(T, dtype=np.int32)
        positions = np.arange(n)
        for k, t in enumerate(heights):
            starts = np.nonzero((own <= t) & (t < parent))[0]          # in timeline order: cluster k + 1 is starts[k]
            numbers = np.zeros(n, dtype=np.int32)
            numbers[lo[starts]] = np.arange(1, len(starts) + 1)
            # "last non-zero wins" prefix scan: every position takes the number at the latest start before it
            latest = np.maximum.accumulate(np.where(numbers > 0, positions, 0))
            labels[k] = numbers[latest][leaf_lo] - 1
            counts[k] = len(starts)
        self.last_num_clusters = counts
        return labels

    def _cuts_on_device(self, heights: np.ndarray, device) -> np.ndarray:
        from . import ffi
        ffi.require_gpu()
        lib = ffi.load()
        T, n = len(heights), self.num_leaves
        with torch.cuda.device(device):
            key = (device.type, torch.cuda.current_device() if device.index is None else device.index)
            cache = self.__dict__.setdefault("_device_plans", {})
            if key not in cache:
                cache[key] = tuple(torch.from_numpy(a).to(device) for a in self.plan())
            own, parent, lo, leaf_lo = cache[key]
            t_dev = torch.from_numpy(heights).to(device)
            labels = torch.empty((T, n), dtype=torch.int32, device=device)
            counts = torch.empty(T, dtype=torch.int32, device=device)
            ws = torch.empty(lib.pa_dendrogram_cuts_workspace_bytes(n, T), dtype=torch.uint8, device=device)
            ffi.check(lib.pa_dendrogram_cuts(ffi.ptr(own), ffi.ptr(parent), ffi.ptr(lo), ffi.ptr(leaf_lo), n,
                                             ffi.ptr(t_dev), T, ffi.ptr(labels), ffi.ptr(counts), ffi.ptr(ws),
                                             ws.numel(), ffi.stream()), "pa_dendrogram_cuts")
            self.last_num_clusters = counts.cpu().numpy()
            return labels.cpu().numpy()

    def large_cluster_counts(self, min_size: int) -> np.ndarray:
        """counts[i] = number of clusters with >= min_size members after merges 0..i."""
        Z, n = self.Z, self.num_leaves
        child_size = np.ones((n - 1, 2))
        for side in (0, 1):
            ids = Z[:, side].astype(np.int64)
            inner = ids >= n
            child_size[inner, side] = Z[ids[inner] - n, 3]
        delta = (Z[:, 3] >= min_size).astype(np.int64) - (child_size >= min_size).sum(axis=1)
        return (n if min_size <= 1 else 0) + np.cumsum(delta)


# ---------------------------------------------------------------------------------------------------
class BaseClustering(Pipeline):
    def __init__(self, metric: str = "cosine", constrained_assignment: bool = False):
        super().__init__()
        self.metric = metric
        self.constrained_assignment = constrained_assignment
        self.device = None
        object.__setattr__(self, "timings", {})   # wall seconds of the last call, per sub-step

    def to(self, device):
        self.device = device
        return self

    def set_num_clusters(self, num_embeddings: int, num_clusters: Optional[int] = None,
                         min_clusters: Optional[int] = None, max_clusters: Optional[int] = None):
        return clamp_cluster_bounds(num_embeddings, num_clusters, min_clusters, max_clusters)

    def filter_embeddings(self, embeddings: np.ndarray, segmentations: SlidingWindowFeature,
                          min_active_ratio: float = 0.2, num_clean_frames: Optional[np.ndarray] = None):
        """training set = (chunk, speaker) pairs that speak ALONE for at least 20 % of the chunk and
        whose embedding has no NaN (clustering.py:77-125).  `num_clean_frames` (C, S): those frame
        counts when the caller already has them (pa_seg_chunk_stats on the GPU)."""
        num_frames = segmentations.data.shape[1]
        if num_clean_frames is None:
            seg = segmentations.data
            alone = seg.sum(axis=2, keepdims=True) == 1
            num_clean_frames = (seg * alone).sum(axis=1)
        keep = (num_clean_frames >= min_active_ratio * num_frames) & ~np.isnan(embeddings).any(axis=2)
        chunk_idx, speaker_idx = np.nonzero(keep)
        return embeddings[chunk_idx, speaker_idx], chunk_idx, speaker_idx

    def constrained_argmax(self, soft_clusters: np.ndarray) -> np.ndarray:
        """one cluster per local speaker and chunk, no cluster twice (Hungarian, clustering.py:127-140)"""
        from scipy.optimize import linear_sum_assignment
        scores = np.nan_to_num(soft_clusters, nan=np.nanmin(soft_clusters))
        hard = np.full(scores.shape[:2], -2, dtype=np.int8)
        for c, cost in enumerate(scores):
            speakers, clusters = linear_sum_assignment(cost, maximize=True)
            hard[c, speakers] = clusters
        return hard

    #: chunks of the last `constrained_argmax_device` call that went back to the host solver
    last_flagged_chunks: int = 0

    def constrained_argmax_device(self, soft_clusters: np.ndarray, silent: np.ndarray) -> np.ndarray:
        """`np.where(silent, -2, self.constrained_argmax(soft_clusters))` with all chunks assigned in one launch
        (`pa_constrained_assign`, csrc/assign.hip).  `silent` (C, S): local speakers that never speak; the caller has
        pushed their rows below every other value (`soft[silent] = soft.min() - 1`), so they only ever take what the
        others leave and the kernel searches over the other rows alone.  A chunk whose optimum is not safely unique
        (an active row of NaN, which `nan_to_num` turns into a constant; a runner-up within 1e-9; a row whose last
        kept and first dropped column lie within 1e-9, where the kernel's pruned search could miss such a runner-up;
        silent rows that do not lie below every active value) is solved by
        `constrained_argmax` on the rows the host path would have seen, as is every chunk beyond the kernel's
        limits (4 local speakers, 64 clusters) or without a GPU."""
        silent = np.asarray(silent, dtype=bool)
        C, S, K = soft_clusters.shape
        on_gpu = getattr(self.device, "type", None) == "cuda"
        if not on_gpu or C == 0 or K == 0 or S > 4 or K > 64:
            self.last_flagged_chunks = C
            return np.where(silent, -2, self.constrained_argmax(soft_clusters)).astype(np.int8)
        from . import ffi
        device = self.device
        with torch.cuda.device(device):
            soft = torch.from_numpy(np.ascontiguousarray(soft_clusters, dtype=np.float64)).to(device)
            mask = torch.from_numpy(np.ascontiguousarray(silent, dtype=np.uint8)).to(device)
            out = torch.empty(C * (S + 1), dtype=torch.int8, device=device)     # hard (C, S), then flagged (C)
            ffi.check(ffi.load().pa_constrained_assign(ffi.ptr(soft), ffi.ptr(mask), C, S, K, ffi.ptr(out[:C * S]),
                                                       ffi.ptr(out[C * S:]), ffi.stream()), "pa_constrained_assign")
            host = out.cpu().numpy()
        hard = host[:C * S].reshape(C, S).copy()
        # the kernel leaves the silent rows out, which is the host's answer only while they lie below every value of
        # an active row.  They do not when a NaN embedding makes `soft.min()` NaN: the silent rows then become the
        # smallest finite value, like the NaN row itself.  A chunk where they come within the margin goes to the host.
        scores = np.nan_to_num(soft_clusters, nan=np.nanmin(soft_clusters))
        mask = silent[:, :, None]
        unsafe = np.where(mask, scores, -np.inf).max(axis=(1, 2)) > np.where(mask, np.inf, scores).min(axis=(1, 2)) - 1e-9
        flagged = np.nonzero((host[C * S:] != 0) | unsafe)[0]
        self.last_flagged_chunks = len(flagged)
        if len(flagged):
            hard[flagged] = np.where(silent[flagged], -2, self.constrained_argmax(scores[flagged]))
        return hard

    def _similarities(self, embeddings: np.ndarray, centroids: np.ndarray, device_embeddings=None) -> np.ndarray:
        """soft (C, S, K) = 2 - distance of every (chunk, speaker) embedding to every centroid.
        `device_embeddings`: the same (C, S, D) values as a device tensor, when the caller still has them there
        (saves the float64 conversion on the host and the upload)."""
        C, S, D = embeddings.shape
        A = embeddings.reshape(C * S, D)
        if device_embeddings is not None and tuple(device_embeddings.shape) == (C, S, D):
            A = device_embeddings.reshape(C * S, D)
        d = distance.cdist(A, centroids, metric=self.metric, device=self.device)
        return 2 - d.reshape(C, S, -1)

    def assign_embeddings(self, embeddings: np.ndarray, train_chunk_idx: np.ndarray,
                          train_speaker_idx: np.ndarray, train_clusters: np.ndarray,
                          constrained: bool = False, device_embeddings=None):
        """centroid of every cluster from the (un-normalised) training embeddings, then every
        (chunk, speaker) goes to its most similar centroid (clustering.py:142-212)"""
        K = int(np.max(train_clusters)) + 1
        C, S, D = embeddings.shape
        on_gpu = getattr(self.device, "type", None) == "cuda"
        if (on_gpu and device_embeddings is not None and tuple(device_embeddings.shape) == (C, S, D)
                and device_embeddings.dtype == torch.float32):
            # the embeddings are still in HBM: centroids there (pa_centroid_means), only (K, D) comes back
            centroids = distance.centroid_means(device_embeddings.reshape(C * S, D).contiguous(),
                                                train_chunk_idx * S + train_speaker_idx, train_clusters, K,
                                                self.device)
        else:
            centroids = segment_means(embeddings[train_chunk_idx, train_speaker_idx], train_clusters, K)
        soft = self._similarities(embeddings, centroids, device_embeddings)
        hard = self.constrained_argmax(soft) if constrained else np.argmax(soft, axis=2)
        return hard, soft, centroids

    #: KMeans on the device (`distance.kmeans`) when the object lives on a GPU; False: always scikit-learn's call
    kmeans_on_device: bool = True

    def kmeans_labels(self, vectors: np.ndarray, num_clusters: int) -> np.ndarray:
        """`KMeans(n_clusters=num_clusters, n_init=3, random_state=42, copy_x=False).fit_predict(vectors)`
        (clustering.py:545-547, 635-637).  On a GPU with `kmeans_on_device`: `distance.kmeans`, scikit-learn's labels
        for the same values in float64; where that route does not apply or gives up (None), and on the host, the
        scikit-learn call itself.  `timings["kmeans"]`: seconds, `timings["kmeans_route"]`: "device" or "host"."""
        t0 = time.perf_counter()
        labels = None
        if self.kmeans_on_device and getattr(self.device, "type", None) == "cuda":
            labels = distance.kmeans(vectors, num_clusters, self.device, n_init=3, random_state=42)
        route = "host" if labels is None else "device"
        if labels is None:
            from sklearn.cluster import KMeans
            labels = KMeans(n_clusters=num_clusters, n_init=3, random_state=42, copy_x=False).fit_predict(vectors)
        self.timings.update(kmeans=time.perf_counter() - t0, kmeans_route=route)
        return labels

    def _single_cluster(self, embeddings: np.ndarray, train_embeddings: np.ndarray):
        C, S, _ = embeddings.shape
        return (np.zeros((C, S), dtype=np.int8), np.ones((C, S, 1)),
                np.mean(train_embeddings, axis=0, keepdims=True))

    def __call__(self, embeddings: np.ndarray, segmentations: Optional[SlidingWindowFeature] = None,
                 num_clusters: Optional[int] = None, min_clusters: Optional[int] = None,
                 max_clusters: Optional[int] = None, **kwargs):
        """clustering.py:214-289"""
        self.timings.clear()
        t0 = time.perf_counter()
        train, chunk_idx, speaker_idx = self.filter_embeddings(
            embeddings, segmentations=segmentations, num_clean_frames=kwargs.get("num_clean_frames"))
        self.timings["filter"] = time.perf_counter() - t0
        num_clusters, min_clusters, max_clusters = self.set_num_clusters(
            train.shape[0], num_clusters=num_clusters, min_clusters=min_clusters, max_clusters=max_clusters)
        if max_clusters < 2:
            return self._single_cluster(embeddings, train)
        t0 = time.perf_counter()
        labels = self.cluster(train, min_clusters=min_clusters, max_clusters=max_clusters,
                              num_clusters=num_clusters)
        t1 = time.perf_counter()
        out = self.assign_embeddings(embeddings, chunk_idx, speaker_idx, labels,
                                     constrained=self.constrained_assignment,
                                     device_embeddings=kwargs.get("device_embeddings"))
        self.timings.update(cluster=t1 - t0, assign=time.perf_counter() - t1)
        return out


class AgglomerativeClustering(BaseClustering):
    """clustering.py:292-480.  Hyper-parameters: method, threshold, min_cluster_size."""

    expects_num_clusters: bool = False

    def __init__(self, metric: str = "cosine", constrained_assignment: bool = False):
        super().__init__(metric=metric, constrained_assignment=constrained_assignment)
        self.threshold = Uniform(0.0, 2.0)
        self.method = Categorical(["average", "centroid", "complete", "median", "single", "ward",
                                   "weighted"])
        self.min_cluster_size = Integer(1, 20)

    def dendrogram(self, embeddings: np.ndarray) -> np.ndarray:
        """linkage matrix (:368-382).  Geometric methods on cosine embeddings are run as Euclidean
        linkage of the unit-normalised vectors -- normalised IN PLACE, like the reference, because the
        small-cluster centroids below are means of the normalised copy."""
        geometric = self.metric == "cosine" and self.method in ("centroid", "median", "ward")
        if geometric:
            with np.errstate(divide="ignore", invalid="ignore"):
                embeddings /= np.linalg.norm(embeddings, axis=-1, keepdims=True)
        t0 = time.perf_counter()
        on_gpu = self.device is not None and getattr(self.device, "type", None) == "cuda"
        if geometric and self.method == "centroid" and on_gpu and len(embeddings) >= 2:
            if not np.isfinite(embeddings).all():
                # scipy.cluster.hierarchy.linkage validates its input the same way; a zero-norm / inf
                # embedding (NaN after the normalisation) must not reach the merge kernel
                raise ValueError("The condensed distance matrix must contain only finite values.")
            Z = distance.linkage_centroid(embeddings, self.device)
            self.timings.update(pdist=0.0, linkage=time.perf_counter() - t0, num_embeddings=len(embeddings))
            return Z
        if (self.method in distance.CHAIN_METHODS and self.metric in ("cosine", "euclidean") and on_gpu
                and len(embeddings) >= 2):
            # single / complete / average / weighted / ward: pdist, SciPy's finite check and the merge loop on the
            # device (csrc/linkage_chain.hip); ward on cosine embeddings is geometric (normalised above)
            metric = "euclidean" if geometric else self.metric
            Z = distance.linkage_chain(embeddings, self.method, metric, self.device)
            if Z is not None:    # (None: the square matrix exceeds the cap -> the host path below)
                self.timings.update(pdist=0.0, linkage=time.perf_counter() - t0, num_embeddings=len(embeddings))
                return Z
        if geometric or self.metric == "euclidean":
            condensed = distance.pdist_euclidean(embeddings, device=self.device)
            t1 = time.perf_counter()
            Z = linkage(condensed, method=self.method)
            self.timings.update(pdist=t1 - t0, linkage=time.perf_counter() - t1,
                                num_embeddings=len(embeddings))
            return Z
        return linkage(embeddings, method=self.method, metric=self.metric)

    def _cut_for_target(self, tree: Dendrogram, target: int, min_size: int) -> Tuple[np.ndarray, bool]:
        """flat clusters with `target` large clusters, examining cuts by increasing |height - threshold|
        (clustering.py:405-451).  Returns (labels, exact)."""
        Z = tree.Z
        order = np.argsort(np.abs(Z[:, 2] - self.threshold))      # same call as the reference: ties
        order = order[Z[order, 3] >= min_size]                    # merges that create a large cluster
        large = tree.large_cluster_counts(min_size)[order]
        hits = np.nonzero(large == target)[0]
        if len(hits):
            return tree.cut_after_merge(int(order[hits[0]])), True
        # no cut gives the target: the first cut that comes closest, if it beats "everything in one"
        gap = np.abs(large - target)
        if len(gap) and gap.min() < abs(1 - target):
            return tree.cut_after_merge(int(order[int(np.argmin(gap))])), False
        return tree.cut_after_merge(tree.num_leaves - 1), False

    def cluster(self, embeddings: np.ndarray, min_clusters: Optional[int] = None,
                max_clusters: Optional[int] = None, num_clusters: Optional[int] = None):
        n = embeddings.shape[0]
        if n == 1:
            return np.zeros((1,), dtype=np.uint8)
        tree = Dendrogram(self.dendrogram(embeddings))
        return self.cluster_from_cut(embeddings, tree, tree.cut(self.threshold), min_clusters=min_clusters,
                                     max_clusters=max_clusters, num_clusters=num_clusters)

    def cluster_from_cut(self, embeddings: np.ndarray, tree: Dendrogram, labels: np.ndarray,
                         min_clusters: Optional[int] = None, max_clusters: Optional[int] = None,
                         num_clusters: Optional[int] = None):
        """the rest of `cluster` once `tree` = the dendrogram of `embeddings` and `labels` = its cut at
        `self.threshold` are known (:390-476): the size test, the forced-number walk and the reassignment of the small
        clusters.  `embeddings` is the copy the tree was built from (normalised by `dendrogram` for the geometric
        methods: the small-cluster centroids are its means)."""
        n = embeddings.shape[0]
        min_size = min(self.min_cluster_size, max(1, round(0.1 * n)))
        sizes = np.bincount(labels)
        num_large = int((sizes >= min_size).sum())
        # a bound that the threshold cut violates becomes the target (:394-403)
        if num_large < min_clusters:
            num_clusters = min_clusters
        elif num_large > max_clusters:
            num_clusters = max_clusters
        if num_clusters is not None and num_large != num_clusters:
            labels, exact = self._cut_for_target(tree, num_clusters, min_size)
            sizes = np.bincount(labels)
            num_large = int((sizes >= min_size).sum())
            if not exact:
                warnings.warn(f"hierarchical clustering yields {num_large} clusters of at least "
                              f"{min_size} embeddings where {num_clusters} were requested; a smaller "
                              "`min_cluster_size` may help")
        if num_large == 0:
            return np.zeros_like(labels)
        is_large = sizes >= min_size
        if is_large[np.unique(labels)].all():
            return labels
        # every small cluster joins the large cluster with the nearest centroid (:457-476); centroids
        # are means of the (normalised) training copy
        ids = np.nonzero(sizes > 0)[0]
        means = segment_means(embeddings, labels, len(sizes))
        large_ids, small_ids = ids[is_large[ids]], ids[~is_large[ids]]
        nearest = np.argmin(scipy_cdist(means[large_ids], means[small_ids], metric=self.metric), axis=0)
        relabel = np.arange(len(sizes))
        relabel[small_ids] = large_ids[nearest]
        return np.unique(relabel[labels], return_inverse=True)[1]


class KMeansClustering(BaseClustering):
    """clustering.py:483-547.  KMeans with an explicit number of speakers: on a GPU `distance.kmeans` (csrc/kmeans.hip),
    scikit-learn's labels for the same values in float64; unplaced, on the host or with `kmeans_on_device = False`
    scikit-learn's KMeans, the reference's own call (`kmeans_labels`)."""

    expects_num_clusters: bool = True

    def __init__(self, metric: str = "cosine"):
        if metric not in ("cosine", "euclidean"):
            raise ValueError(f"Unsupported metric: {metric}. Must be 'cosine' or 'euclidean'.")
        super().__init__(metric=metric)

    def cluster(self, embeddings: np.ndarray, min_clusters: Optional[int] = None,
                max_clusters: Optional[int] = None, num_clusters: Optional[int] = None):
        if num_clusters is None:
            raise ValueError("`num_clusters` must be provided.")
        if embeddings.shape[0] < num_clusters:
            return np.arange(embeddings.shape[0], dtype=np.int32)
        if self.metric == "cosine":
            with np.errstate(divide="ignore", invalid="ignore"):
                embeddings /= np.linalg.norm(embeddings, axis=-1, keepdims=True)
        return self.kmeans_labels(embeddings, num_clusters)


class VBxClustering(BaseClustering):
    """clustering.py:550-669: AHC initialisation (GPU linkage) -> PLDA projection (GPU) -> VBx (GPU,
    csrc/vbx.hip) -> centroids of the surviving speakers -> constrained assignment.
    Hyper-parameters: threshold (AHC cut), Fa, Fb."""

    expects_num_clusters: bool = False
    max_iterations = 20          # cluster_vbx(maxIters=20), utils/vbx.py:143
    init_smoothing = 7.0         # softmax temperature of the one-hot AHC labels, utils/vbx.py:143-147
    elbo_epsilon = 1e-4          # VBx(epsilon=1e-4), utils/vbx.py:36
    prune_below = 1e-7           # speakers whose prior collapsed (clustering.py:621)

    def __init__(self, plda=None, metric: str = "cosine", constrained_assignment: bool = True):
        super().__init__(metric=metric, constrained_assignment=constrained_assignment)
        from .plda import get_plda
        self.plda = get_plda(plda)
        self.threshold = Uniform(0.5, 0.8)
        self.Fa = Uniform(0.01, 0.5)
        self.Fb = Uniform(0.01, 15.0)

    def to(self, device):
        super().to(device)
        if self.plda is not None:
            self.plda.to(device)
        return self

    def _unit_linkage(self, train: np.ndarray):
        """the centroid linkage of the unit vectors (it depends on no hyper-parameter) and those vectors"""
        unit = train / np.linalg.norm(train, axis=1, keepdims=True)
        if not np.isfinite(unit).all():
            raise ValueError("The condensed distance matrix must contain only finite values.")
        return distance.linkage_centroid(unit, self.device), unit

    def _ahc_labels(self, train: np.ndarray) -> np.ndarray:
        Z, unit = self._unit_linkage(train)
        labels = fcluster(Z, self.threshold, criterion="distance") - 1
        return np.unique(labels, return_inverse=True)[1], unit

    def initial_responsibilities(self, labels: np.ndarray) -> np.ndarray:
        """(N, S) float64: the smoothed one-hot AHC labels VB starts from (utils/vbx.py:143-147)"""
        from scipy.special import softmax
        n, s = len(labels), int(labels.max()) + 1
        onehot = np.zeros((n, s))
        onehot[np.arange(n), labels] = 1.0
        return onehot if self.init_smoothing < 0 else softmax(onehot * self.init_smoothing, axis=1)

    def _vbx(self, fea, labels: np.ndarray):
        """responsibilities (N, S) and speaker priors (S,) after VB inference on the device"""
        import torch
        from . import ffi
        lib = ffi.load()
        device = self.device
        n, d = fea.shape
        q0 = self.initial_responsibilities(labels)
        s = q0.shape[1]
        gamma = torch.from_numpy(q0).to(device)
        phi = torch.from_numpy(np.ascontiguousarray(self.plda.phi, dtype=np.float64)).to(device)
        elbo = torch.zeros(self.max_iterations, dtype=torch.float64, device=device)
        ws = torch.empty(lib.pa_vbx_workspace_bytes(n, s, d), dtype=torch.uint8, device=device)
        history = []
        with torch.cuda.device(device):
            for it in range(self.max_iterations):
                ffi.check(lib.pa_vbx_iteration(ffi.ptr(fea), ffi.ptr(phi), n, s, d, float(self.Fa),
                                               float(self.Fb), int(it == 0), ffi.ptr(gamma),
                                               ffi.ptr(elbo[it:]), ffi.ptr(ws), ws.numel(), ffi.stream()),
                          "pa_vbx_iteration")
                history.append(float(elbo[it].item()))     # the convergence test of utils/vbx.py:129-133
                if it > 0 and history[-1] - history[-2] < self.elbo_epsilon:
                    break
        q = gamma.cpu().numpy()
        pi = q.sum(axis=0)
        self.timings["vbx_iterations"] = len(history)
        self.last_elbo_history = history
        return q, pi / pi.sum()

    def vbx_batch(self, fea, inits: list, jobs: list, workspace_bytes: Optional[int] = None):
        """Whole VB inferences for many (initialisation, Fa, Fb) jobs over the same features, without a read-back per
        iteration (`pa_vbx_run_batch`, csrc/vbx.hip).  `fea` (N, 128) device tensor; `inits`: (N, S_i) float64 arrays
        (`initial_responsibilities`), uploaded once; `jobs`: (index into `inits`, Fa, Fb).  Returns per job
        (q (N, S), ELBO history): bit for bit what `_vbx` gives with those hyper-parameters.  `workspace_bytes`
        bounds what one call allocates beyond the shared inputs -- the kernels' workspace plus the result buffer
        (J N Smax doubles, the larger of the two); a batch over the budget is run in several calls
        (`last_vbx_calls`), one download each."""
        from . import ffi
        lib = ffi.load()
        device = self.device
        n, d = fea.shape
        if not jobs:
            self.last_vbx_calls = 0
            return []
        sizes = [int(q0.shape[1]) for q0 in inits]
        offsets = np.concatenate([[0], np.cumsum([n * s for s in sizes])]).astype(np.int64)
        job_s = [sizes[i] for i, _, _ in jobs]
        iters = self.max_iterations

        def call_bytes(count, smax):      # the kernels' workspace and the buffer the results come back in
            return int(lib.pa_vbx_batch_workspace_bytes(count, n, smax, d)) \
                + 8 * (count * n * smax + count * iters + (count + 1) // 2)
        calls = split_vbx_jobs(job_s, call_bytes, workspace_bytes)
        out = [None] * len(jobs)
        with torch.cuda.device(device):
            gamma0 = torch.from_numpy(np.concatenate([np.ascontiguousarray(q0, dtype=np.float64).reshape(-1)
                                                      for q0 in inits])).to(device)
            phi = torch.from_numpy(np.ascontiguousarray(self.plda.phi, dtype=np.float64)).to(device)
            for call in calls:
                J, smax = len(call), max(job_s[j] for j in call)
                table = np.array([[offsets[jobs[j][0]], job_s[j]] for j in call], dtype=np.int64)
                factors = np.array([[float(jobs[j][1]), float(jobs[j][2])] for j in call], dtype=np.float64)
                job_init, job_f = torch.from_numpy(table).to(device), torch.from_numpy(factors).to(device)
                # one buffer, one download: gamma (J, n smax), the ELBO histories (J, iters), the iteration counts
                buffer = torch.zeros(J * n * smax + J * iters + (J + 1) // 2, dtype=torch.float64, device=device)
                gamma, elbo = buffer[:J * n * smax], buffer[J * n * smax:J * n * smax + J * iters]
                counts = buffer[J * n * smax + J * iters:].view(torch.int32)
                ws = torch.empty(lib.pa_vbx_batch_workspace_bytes(J, n, smax, d), dtype=torch.uint8, device=device)
                ffi.check(lib.pa_vbx_run_batch(ffi.ptr(fea), ffi.ptr(phi), n, d, J, ffi.ptr(gamma0), gamma0.numel(),
                                               ffi.ptr(job_init), ffi.ptr(job_f), smax, iters,
                                               float(self.elbo_epsilon), ffi.ptr(gamma), ffi.ptr(elbo),
                                               ffi.ptr(counts), ffi.ptr(ws), ws.numel(), ffi.stream()),
                          "pa_vbx_run_batch")
                host = buffer.cpu().numpy()
                done = host[J * n * smax + J * iters:].view(np.int32)
                for k, j in enumerate(call):
                    if done[k] < 1:
                        raise RuntimeError("pa_vbx_run_batch left a job untouched: its table entry is out of range")
                    q = host[k * n * smax:k * n * smax + n * job_s[j]].reshape(n, job_s[j]).copy()
                    history = host[J * n * smax + k * iters:J * n * smax + k * iters + done[k]].tolist()
                    out[j] = (q, history)
        self.last_vbx_calls = len(calls)
        return out

    def before_cut(self, embeddings: np.ndarray, segmentations: SlidingWindowFeature, num_clean_frames=None):
        """what a file needs before the AHC cut, none of it a function of threshold, Fa or Fb: the training
        embeddings, their unit vectors, the centroid linkage of those and the PLDA features (kept on the device).
        None with fewer than two training embeddings."""
        train, _, _ = self.filter_embeddings(embeddings, segmentations=segmentations,
                                             num_clean_frames=num_clean_frames)
        if train.shape[0] < 2:
            return None
        Z, unit = self._unit_linkage(train)
        return train, unit, Z, self.plda.transform_device(train, self.device)

    def after_vbx(self, embeddings: np.ndarray, segmentations: SlidingWindowFeature, train: np.ndarray,
                  unit: np.ndarray, q: np.ndarray, num_clusters: Optional[int] = None, min_clusters=1,
                  max_clusters=np.inf, active_frames=None, assign_on_device: bool = False):
        """from the responsibilities `q` to (hard, soft, centroids): speakers whose prior collapsed are pruned, the
        centroids are `W.T @ train` on the host, a violated bound falls back to KMeans, silent local speakers are
        pushed out of the assignment.  `assign_on_device`: the constrained assignment through
        `constrained_argmax_device`, whose silent rows are -2 (the pipeline masks them to -2 anyway)."""
        pi = q.sum(axis=0)
        priors = pi / pi.sum()
        W = q[:, priors > self.prune_below]
        centroids = W.T @ train / W.sum(axis=0, keepdims=True).T
        constrained = self.constrained_assignment
        found = centroids.shape[0]
        self.timings["vbx_speakers"] = found
        # a violated bound (or an explicit number that VBx did not find) falls back to KMeans on the
        # unit vectors, without the assignment constraint (clustering.py:624-645)
        if found < min_clusters:
            num_clusters = min_clusters
        elif found > max_clusters:
            num_clusters = max_clusters
        if num_clusters and num_clusters != found:
            constrained = False
            km = self.kmeans_labels(unit, num_clusters)
            centroids = segment_means(train, km, num_clusters)
        soft = self._similarities(embeddings, centroids)
        if constrained:
            # silent local speakers must never win a cluster in the assignment (:658-660)
            silent = (segmentations.data.sum(axis=1) == 0) if active_frames is None else (active_frames == 0)
            soft[silent] = soft.min() - 1.0
            hard = self.constrained_argmax_device(soft, silent) if assign_on_device else self.constrained_argmax(soft)
        else:
            hard = np.argmax(soft, axis=2)
        return hard.reshape(embeddings.shape[:2]), soft, centroids

    def __call__(self, embeddings: np.ndarray, segmentations: Optional[SlidingWindowFeature] = None,
                 num_clusters: Optional[int] = None, min_clusters: Optional[int] = None,
                 max_clusters: Optional[int] = None, **kwargs):
        if self.plda is None:
            raise ValueError("VBxClustering needs a PLDA model (`plda=` of SpeakerDiarization)")
        if self.device is None or getattr(self.device, "type", None) != "cuda":
            raise RuntimeError("VBxClustering runs on the GPU: pipeline.to(torch.device('cuda')) first")
        self.timings.clear()
        min_clusters = 1 if min_clusters is None else min_clusters
        max_clusters = np.inf if max_clusters is None else max_clusters
        train, _, _ = self.filter_embeddings(embeddings, segmentations=segmentations,
                                             num_clean_frames=kwargs.get("num_clean_frames"))
        if train.shape[0] < 2:
            return self._single_cluster(embeddings, train)
        t0 = time.perf_counter()
        labels, unit = self._ahc_labels(train)
        t1 = time.perf_counter()
        fea = self.plda.transform_device(train, self.device)
        q, _ = self._vbx(fea, labels)
        t2 = time.perf_counter()
        out = self.after_vbx(embeddings, segmentations, train, unit, q, num_clusters=num_clusters,
                             min_clusters=min_clusters, max_clusters=max_clusters,
                             active_frames=kwargs.get("active_frames"))
        self.timings.update(ahc=t1 - t0, vbx=t2 - t1, assign=time.perf_counter() - t2,
                            num_embeddings=train.shape[0])
        return out


def split_vbx_jobs(job_sizes: list, bytes_of: Callable, budget: Optional[int] = None) -> list:
    """the jobs of one `VBxClustering.vbx_batch`, in order, as consecutive runs of job indices: a run is as long as
    `bytes_of(jobs in it, largest S in it)` stays within `budget` (None: one run); a single job over the budget
    still gets a run of its own.  Runs are also cut at the 65 535 jobs one launch takes."""
    runs, run, largest = [], [], 0
    for j, s in enumerate(job_sizes):
        if run and (len(run) >= 65535 or (budget is not None and bytes_of(len(run) + 1, max(s, largest)) > budget)):
            runs.append(run)
            run, largest = [], 0
        run.append(j)
        largest = max(largest, s)
    if run:
        runs.append(run)
    return runs


class OracleClustering(BaseClustering):
    """Clusters with the answer sheet (clustering.py:672-756): every chunk's local speakers are mapped onto
    the reference speakers by the cost-minimising permutation between the model's segmentation and the
    reference annotation discretised on the same chunk / frame grid.  Needs `file["annotation"]`; no
    embeddings are involved in the assignment (centroids are computed when they are given)."""

    expects_num_clusters = True

    def __call__(self, embeddings: Optional[np.ndarray] = None,
                 segmentations: Optional[SlidingWindowFeature] = None, file=None, frames=None, **kwargs):
        from .annotation_frames import oracle_segmentation
        from .permutation import permutate
        num_chunks, num_frames, num_speakers = segmentations.data.shape
        oracle = oracle_segmentation(file, segmentations.sliding_window, frames=frames)
        file["oracle_segmentations"] = oracle
        num_clusters = oracle.data.shape[2]
        common = min(num_frames, oracle.data.shape[1])
        seg, ref = segmentations.data[:, :common], oracle.data[:, :common]
        hard = np.full((num_chunks, num_speakers), -2, dtype=np.int8)
        soft = np.zeros((num_chunks, num_speakers, num_clusters))
        for c in range(min(num_chunks, ref.shape[0])):     # the zero-padded last chunk has no reference chunk
            _, (permutation,) = permutate(ref[c][np.newaxis], seg[c])
            for cluster, speaker in enumerate(permutation):
                if speaker is not None:
                    hard[c, speaker] = cluster
                    soft[c, speaker, cluster] = 1.0
        if embeddings is None:
            return hard, soft, None
        train, chunk_idx, speaker_idx = self.filter_embeddings(
            embeddings, segmentations=SlidingWindowFeature(seg, segmentations.sliding_window))
        train_clusters = hard[chunk_idx, speaker_idx]
        centroids = np.vstack([np.mean(train[train_clusters == k], axis=0) for k in range(num_clusters)])
        return hard, soft, centroids


class Clustering(Enum):
    """clustering.py:759-763"""
    AgglomerativeClustering = AgglomerativeClustering
    KMeansClustering = KMeansClustering
    VBxClustering = VBxClustering
    OracleClustering = OracleClustering
