"""`pa_dendrogram_cuts` (csrc/dendrogram.hip) against `scipy.cluster.hierarchy.fcluster(Z, t, "distance") - 1`: labels and
cluster counts equal for every threshold, on trees that cross a wave, a workgroup and several scan tiles, for more
thresholds than one launch takes, at the size of one audio-hour, and whatever was cut before in the same process."""
import numpy as np
import pytest
from scipy.cluster.hierarchy import fcluster, linkage

from test_dendrogram_cuts_cpu import points, thresholds_for

pytestmark = pytest.mark.gpu

METHODS = ("centroid", "single", "average")
SIZES = (2, 3, 64, 65, 257, 1000, 1025, 4097)
KINDS = ("random", "tied", "chain")
COUNTS = (1, 7, 64)


def many_thresholds(Z: np.ndarray, count: int, seed: int) -> np.ndarray:
    """`count` thresholds: the special ones of the host test first, then merge heights, their lower neighbours and
    uniform draws over the range"""
    rng = np.random.default_rng(seed)
    heights = Z[:, 2]
    some = heights[rng.integers(0, len(heights), size=count)]
    pool = np.concatenate([thresholds_for(Z, seed), some, np.nextafter(some, -np.inf),
                           rng.uniform(heights.min() - 0.1, heights.max() + 0.1, size=count)])
    return pool[:count] if count <= 5 else np.concatenate([pool[:5], rng.permutation(pool[5:])[:count - 5]])


def assert_device_cuts(tree, Z, thresholds, device):
    got = tree.cuts(thresholds, device=device)
    assert got.shape == (len(thresholds), Z.shape[0] + 1) and got.dtype == np.int32
    for k, t in enumerate(thresholds):
        want = fcluster(Z, t, criterion="distance") - 1
        assert (got[k] == want).all(), f"threshold {t!r} (row {k})"
        assert tree.last_num_clusters[k] == want.max() + 1
    return got


@pytest.fixture(scope="module")
def trees():
    """every (method, kind, n) dendrogram once (SciPy on the host)"""
    return {(method, kind, n): linkage(points(kind, n, seed=n), method=method)
            for method in METHODS for kind in KINDS for n in SIZES}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", METHODS)
def test_device_cuts_equal_fcluster(trees, method, kind, gpu_device):
    from pyannote_audio_amd.clustering import Dendrogram
    for n in SIZES:
        Z = trees[method, kind, n]
        tree = Dendrogram(Z)
        for count in COUNTS:
            if count == 64 and n > 1025:      # (64 SciPy cuts of the largest tree add nothing the 7 do not)
                continue
            assert_device_cuts(tree, Z, many_thresholds(Z, count, seed=n + count), gpu_device)


def test_more_thresholds_than_one_launch(trees, gpu_device):
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd.clustering import Dendrogram
    chunk = ffi.load().pa_dendrogram_cuts_chunk()
    for key in (("centroid", "random", 65), ("single", "chain", 257)):
        Z = trees[key]
        assert_device_cuts(Dendrogram(Z), Z, many_thresholds(Z, 2 * chunk + 3, seed=9), gpu_device)


def test_workspace_smaller_than_asked_for_means_more_launches(trees, gpu_device):
    """the C entry point with room for three rows only"""
    import torch
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd.clustering import Dendrogram
    lib = ffi.load()
    Z = trees["average", "random", 257]
    n, tree = 257, Dendrogram(Z)
    thresholds = many_thresholds(Z, 10, seed=4)
    plan = [torch.from_numpy(a).to(gpu_device) for a in tree.plan()]
    t_dev = torch.from_numpy(thresholds).to(gpu_device)
    labels = torch.full((10, n), -7, dtype=torch.int32, device=gpu_device)
    counts = torch.full((10,), -7, dtype=torch.int32, device=gpu_device)
    ws = torch.empty(3 * n * 4 + 5, dtype=torch.uint8, device=gpu_device)
    ffi.check(lib.pa_dendrogram_cuts(*(ffi.ptr(a) for a in plan), n, ffi.ptr(t_dev), 10, ffi.ptr(labels),
                                     ffi.ptr(counts), ffi.ptr(ws), ws.numel(), ffi.stream()), "pa_dendrogram_cuts")
    want = np.stack([fcluster(Z, t, criterion="distance") - 1 for t in thresholds])
    assert (labels.cpu().numpy() == want).all()
    assert (counts.cpu().numpy() == want.max(axis=1) + 1).all()
    with pytest.raises(ValueError):
        ffi.check(lib.pa_dendrogram_cuts(*(ffi.ptr(a) for a in plan), n, ffi.ptr(t_dev), 10, ffi.ptr(labels),
                                         ffi.ptr(counts), ffi.ptr(ws), n * 4 - 1, ffi.stream()), "pa_dendrogram_cuts")


@pytest.fixture(scope="module")
def hour(gpu_device):
    """the training set of one audio-hour: 7 176 unit-norm 256-d points around twelve directions, their centroid
    dendrogram from the device (held bit-identical to SciPy by the linkage tests) and 32 thresholds over its heights"""
    from pyannote_audio_amd import distance
    rng = np.random.default_rng(11)
    centres = rng.normal(size=(12, 256))
    X = centres[rng.integers(0, 12, size=7176)] + 0.6 * rng.normal(size=(7176, 256))
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    Z = distance.linkage_centroid(X, gpu_device)
    heights = np.sort(Z[:, 2])
    thresholds = np.concatenate([[heights[0] - 1e-3], np.quantile(heights, np.linspace(0.02, 0.999, 29)),
                                 [heights[-1], heights[-1] + 1e-3]])
    return Z, thresholds


def test_hour_sized_tree(hour, gpu_device):
    from pyannote_audio_amd.clustering import Dendrogram
    Z, thresholds = hour
    assert Z.shape == (7175, 4) and len(thresholds) == 32
    assert (np.diff(Z[:, 2]) < 0).any()          # centroid linkage: inversions at this size too
    got = assert_device_cuts(Dendrogram(Z), Z, thresholds, gpu_device)
    # n clusters under every height, one above every height, and something in between
    assert len({int(row.max()) for row in got}) >= 3


def test_small_call_after_a_large_one(hour, trees, gpu_device):
    """nothing of an earlier call (scratch rows, cached plans) leaks into a later one"""
    from pyannote_audio_amd.clustering import Dendrogram
    Z, thresholds = hour
    small = trees["centroid", "tied", 65]
    small_thresholds = many_thresholds(small, 7, seed=2)
    before = assert_device_cuts(Dendrogram(small), small, small_thresholds, gpu_device)
    big = Dendrogram(Z)
    big.cuts(thresholds, device=gpu_device)
    tree = Dendrogram(small)
    after = assert_device_cuts(tree, small, small_thresholds, gpu_device)
    assert (before == after).all()
    assert (assert_device_cuts(tree, small, small_thresholds[:1], gpu_device) == after[:1]).all()   # the cached plan


def test_host_and_device_rows_are_the_same(trees, gpu_device):
    from pyannote_audio_amd.clustering import Dendrogram
    Z = trees["centroid", "random", 1025]
    tree = Dendrogram(Z)
    thresholds = many_thresholds(Z, 7, seed=3)
    assert (tree.cuts(thresholds, device=gpu_device) == tree.cuts(thresholds)).all()
    with pytest.raises(ValueError):
        tree.cuts([np.nan], device=gpu_device)
