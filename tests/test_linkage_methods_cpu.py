"""Host side of the single / complete / average / weighted / Ward linkage on the device (csrc/linkage_chain.hip):
`distance.linkage_finish` -- the stable sort by height plus SciPy's `label()` -- against SciPy on the raw merges of
the plain Python model of the two algorithms (tests/linkage_chain_model.py), which is the model the GPU tests'
reasoning rests on; and the dispatch of `AgglomerativeClustering.dendrogram`."""
import numpy as np
import pytest
import torch
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import pdist

import pyannote_audio_amd as pa
from pyannote_audio_amd import distance
from linkage_chain_model import raw_merges

METHODS = ("single", "complete", "average", "weighted", "ward")


def clustered(n, d, seed, dup_fraction=0.2):
    """five-cluster float32 rows, about `dup_fraction` of them copies of other rows (exact ties)"""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((5, d))
    X = (centers[rng.integers(0, 5, n)] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)
    dup = int(round(dup_fraction * n))
    if dup:
        X[rng.integers(0, n, dup)] = X[rng.integers(0, n, dup)]
    return X


def assert_same_dendrogram(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float64, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: first differing merge {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("n", [2, 3, 40, 150])
def test_linkage_finish_of_the_model_equals_scipy(n, metric):
    y = pdist(clustered(n, 16, seed=n), metric)
    for method in METHODS:
        raw = raw_merges(y, n, method)
        got = distance.linkage_finish(raw, n, single=method == "single")
        assert_same_dendrogram(got, linkage(y, method), f"{method}, n = {n}, {metric}")


def test_linkage_finish_all_points_identical():
    """every distance 0: the chain's prefer-the-previous rule and the smallest-index rule decide every merge"""
    n = 30
    X = np.tile(np.random.default_rng(0).standard_normal((1, 8)), (n, 1))
    for metric in ("cosine", "euclidean"):
        y = pdist(X, metric)
        for method in METHODS:
            got = distance.linkage_finish(raw_merges(y, n, method), n, single=method == "single")
            assert_same_dendrogram(got, linkage(y, method), f"{method}, identical points, {metric}")


def test_linkage_finish_leaves_its_input_alone():
    y = pdist(clustered(20, 8, seed=1), "euclidean")
    raw = raw_merges(y, 20, "average")
    before = raw.copy()
    distance.linkage_finish(raw, 20)
    assert np.array_equal(raw, before)


ALL_METHODS = ("average", "centroid", "complete", "median", "single", "ward", "weighted")


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_unplaced_dendrogram_is_scipy_for_all_seven_methods(metric, monkeypatch):
    def sentinel(*args, **kwargs):
        raise AssertionError("linkage_chain called without a GPU device")
    monkeypatch.setattr(distance, "linkage_chain", sentinel)
    X = clustered(60, 12, seed=5, dup_fraction=0.1)
    for method in ALL_METHODS:
        clu = pa.AgglomerativeClustering(metric=metric).instantiate(
            {"method": method, "min_cluster_size": 2, "threshold": 0.7})
        assert clu.device is None
        got = clu.dendrogram(X.copy())
        if metric == "cosine" and method in ("centroid", "median", "ward"):
            unit = X.copy()
            unit /= np.linalg.norm(unit, axis=-1, keepdims=True)
            want = linkage(pdist(unit, "euclidean"), method)
        else:
            want = linkage(X.copy(), method=method, metric=metric)
        assert_same_dendrogram(got, want, f"{method}, {metric}")


@pytest.mark.parametrize("device", [None, torch.device("cpu"), torch.device("cuda", 0)])
def test_median_never_reaches_linkage_chain(device, monkeypatch):
    """median is the heap algorithm with non-monotone heights: it keeps the host path on every device"""
    def sentinel(*args, **kwargs):
        raise AssertionError("linkage_chain called for method median")
    monkeypatch.setattr(distance, "linkage_chain", sentinel)
    # (on a cuda device the Euclidean pdist would run on the GPU: the host's stands in, this test is about dispatch)
    monkeypatch.setattr(distance, "pdist_euclidean", lambda X, device=None: pdist(X, "euclidean"))
    X = clustered(40, 8, seed=7)
    for metric in ("cosine", "euclidean"):
        clu = pa.AgglomerativeClustering(metric=metric).instantiate(
            {"method": "median", "min_cluster_size": 2, "threshold": 0.7})
        clu.device = device
        unit = X.copy()
        if metric == "cosine":
            unit /= np.linalg.norm(unit, axis=-1, keepdims=True)
        assert_same_dendrogram(clu.dendrogram(X.copy()), linkage(pdist(unit, "euclidean"), "median"), metric)


def test_chain_methods_on_a_gpu_device_go_to_linkage_chain(monkeypatch):
    """the five methods reach `linkage_chain` with the pdist the reference would take: Euclidean on the in-place
    normalised rows for ward on cosine embeddings, cosine on the raw rows for the other four, Euclidean for
    metric="euclidean"; a None answer (square matrix above the cap) falls through to the host path."""
    calls = []
    X = clustered(30, 8, seed=3)

    def recorder(emb, method, metric, device):
        calls.append((method, metric, emb.copy()))
        return None
    monkeypatch.setattr(distance, "linkage_chain", recorder)
    monkeypatch.setattr(distance, "pdist_euclidean", lambda X, device=None: pdist(X, "euclidean"))
    unit = X / np.linalg.norm(X, axis=-1, keepdims=True)
    for metric in ("cosine", "euclidean"):
        for method in METHODS:
            clu = pa.AgglomerativeClustering(metric=metric).instantiate(
                {"method": method, "min_cluster_size": 2, "threshold": 0.7})
            clu.device = torch.device("cuda", 0)
            got = clu.dendrogram(X.copy())
            geometric = metric == "cosine" and method == "ward"
            assert calls[-1][:2] == (method, "euclidean" if geometric else metric)
            assert np.array_equal(calls[-1][2], unit if geometric else X)
            want = linkage(pdist(unit, "euclidean"), method) if geometric else linkage(X, method=method, metric=metric)
            assert_same_dendrogram(got, want, f"{method}, {metric}")
    assert len(calls) == 10

