"""Single, complete, average, weighted and Ward linkage on the GPU (csrc/linkage_chain.hip) against SciPy with `==`:
the cosine pdist, the dendrograms of `distance.linkage_chain` for every method and both metrics at the sizes where the
kernels change shape, the raw merge list against the plain Python model (tests/linkage_chain_model.py, itself pinned
to SciPy in tests/test_linkage_methods_cpu.py), the refusals, the finite check and the clustering object.  Everything
is float64 arithmetic in SciPy's order, so there is no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import pdist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from linkage_chain_model import raw_merges  # noqa: E402
from refusals import GUARD, check_refusal  # noqa: E402

pytestmark = pytest.mark.gpu

METHODS = ("single", "complete", "average", "weighted", "ward")


def clustered(n, d, seed, dup=0):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((5, d))
    X = (centers[rng.integers(0, 5, n)] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)
    if dup:
        X[rng.integers(0, n, dup)] = X[rng.integers(0, n, dup)]
    return X


def identical(n, d, seed):
    return np.tile(np.random.default_rng(seed).standard_normal((1, d)).astype(np.float32), (n, 1))


def assert_same_dendrogram(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float64, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: first differing merge {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


def guarded(count, device, fill=float("nan")):
    """`count` float64 between two guard bands of GUARD elements, everything set to `fill` -> (whole, inner view)"""
    whole = torch.full((count + 2 * GUARD,), fill, dtype=torch.float64, device=device)
    return whole, whole[GUARD:GUARD + count]


def untouched(whole, count):
    return bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[GUARD + count:]).all())


@pytest.mark.parametrize("n,d", [(2, 8), (65, 16), (1025, 256), (33, 17)])
def test_pdist_cosine_equals_scipy(gpu_device, n, d):
    """pa_pdist_cosine_f64 == pdist(X, "cosine") with duplicated rows (distance 0 or one rounding away from it) and a
    pair of antiparallel rows (the clip at -1); (33, 17) adds dot2way's odd tail element.  The condensed output sits
    between NaN guard bands."""
    import pyannote_audio_amd.ffi as ffi
    rng = np.random.default_rng(n)
    X = clustered(n, d, seed=n).astype(np.float64)
    if n > 2:
        X[rng.integers(0, n, n // 8)] = X[rng.integers(0, n, n // 8)]
    X[n - 1] = -3.0 * X[0]
    want = pdist(X, "cosine")
    pairs = n * (n - 1) // 2
    whole, out = guarded(pairs, gpu_device)
    Xd = torch.from_numpy(X).to(gpu_device)
    norms = torch.empty(n, dtype=torch.float64, device=gpu_device)
    ffi.check(ffi.load().pa_pdist_cosine_f64(ffi.ptr(Xd), n, d, ffi.ptr(out), ffi.ptr(norms), ffi.stream()),
              "pa_pdist_cosine_f64")
    torch.cuda.synchronize()
    assert untouched(whole, pairs)
    got = out.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} of {pairs} pairs differ, first {bad[0]}: {got[bad[0]]!r} vs {want[bad[0]]!r}"


CASES = {
    "n2": lambda: clustered(2, 16, 2),                      # the degenerate chain
    "n3": lambda: clustered(3, 16, 3),
    "n63": lambda: clustered(63, 16, 63, dup=6),            # one short of a 64 x 64 tile of the square copy
    "n65": lambda: clustered(65, 16, 65, dup=6),            # crosses a wave, and a tile edge of the square copy
    "n129": lambda: clustered(129, 16, 129, dup=12),        # 3 x 3 tiles, the last one a single row and column
    "n1025": lambda: clustered(1025, 32, 1025, dup=40),     # one element more than the workgroup
    "n2500": lambda: clustered(2500, 32, 2500, dup=25),     # several elements per thread, ties across threads and waves
    "identical70": lambda: identical(70, 16, 70),           # every distance equal: only the tie rules decide
    "n1025-global": lambda: clustered(1025, 32, 1025, dup=40),   # sizes and chain in global memory
}


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("case", list(CASES))
def test_linkage_chain_equals_scipy(gpu_device, case, metric, monkeypatch):
    """distance.linkage_chain(X, method, metric) == scipy linkage(pdist(X, metric), method) row for row, all five
    methods; the host pdist is shared among them."""
    from pyannote_audio_amd import distance
    if case.endswith("-global"):
        monkeypatch.setenv("PA_LINKAGE_CHAIN_LDS", "0")
    X = CASES[case]()
    y = pdist(X, metric)
    for method in METHODS:
        got = distance.linkage_chain(X.copy(), method, metric, gpu_device)
        assert_same_dendrogram(got, linkage(y, method), f"{case}, {method}, {metric}")


def test_two_methods_above_the_default_lds_in_one_process(gpu_device):
    """n = 8200: the nn-chain kernels keep 8 n = 65 600 bytes in dynamic LDS, above the 64 KB a launch gets without
    asking.  The grant is remembered per kernel and device (csrc/launch_state.h), and the kernels of the four methods
    have one signature: every method's own kernel must have been granted its LDS, whichever ran first in the process.
    complete, then average, each equal to SciPy row for row (about 2 s of SciPy each)."""
    from pyannote_audio_amd import distance
    X = clustered(8200, 8, 8200)
    y = pdist(X, "euclidean")
    for method in ("complete", "average"):
        got = distance.linkage_chain(X.copy(), method, "euclidean", gpu_device)
        assert_same_dendrogram(got, linkage(y, method), f"n8200, {method}")


@pytest.mark.parametrize("lds", ["1", "0"])
@pytest.mark.parametrize("method", METHODS)
def test_raw_merges_equal_the_model_and_stay_in_bounds(gpu_device, method, lds, monkeypatch):
    """pa_linkage_chain_f64 on a condensed matrix with ties: `raw` equals the unsorted merge list of the Python model
    (for single: fourth column 0), exactly (n - 1) * 4 doubles are written between intact guard bands, D keeps its
    bits and the status word of the workspace is 0."""
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd import distance
    monkeypatch.setenv("PA_LINKAGE_CHAIN_LDS", lds)
    n = 65
    y = pdist(clustered(n, 8, seed=9, dup=10), "euclidean")
    lib = ffi.load()
    D = torch.from_numpy(y).to(gpu_device)
    before = D.clone()
    whole, raw = guarded((n - 1) * 4, gpu_device)
    ws = torch.empty(lib.pa_linkage_chain_workspace_bytes(n), dtype=torch.uint8, device=gpu_device)
    ffi.check(lib.pa_linkage_chain_f64(ffi.ptr(D), n, distance.CHAIN_METHODS[method], ffi.ptr(raw), ffi.ptr(ws),
                                       ws.numel(), ffi.stream()), "pa_linkage_chain_f64")
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 0
    assert untouched(whole, (n - 1) * 4)
    assert not bool(torch.isnan(raw).any()), "fewer than (n - 1) * 4 doubles were written"
    assert torch.equal(D.view(torch.int64), before.view(torch.int64))
    got, want = raw.cpu().numpy().reshape(n - 1, 4), raw_merges(y, n, method)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"first differing raw merge {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


@pytest.mark.parametrize("what", ["n = 1", "unknown method", "workspace one byte too small"])
def test_linkage_chain_refusals(gpu_device, what):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    n = 65
    D = torch.from_numpy(pdist(clustered(n, 8, seed=1), "euclidean")).to(gpu_device)
    ws_bytes = lib.pa_linkage_chain_workspace_bytes(n)
    n_arg, method, ws_arg, message = {
        "n = 1": (1, 2, ws_bytes, "pa_linkage_chain_f64: n = 1, at least 2 points needed"),
        "unknown method": (n, 5, ws_bytes, "pa_linkage_chain_f64: unknown method 5"),
        "workspace one byte too small": (n, 2, ws_bytes - 1, "pa_linkage_chain_f64: workspace too small"),
    }[what]
    # raw and the workspace travel as bytes: full-size, between guard bands
    check_refusal(lambda raw, ws: lib.pa_linkage_chain_f64(ffi.ptr(D), n_arg, method, raw, ws, ws_arg, ffi.stream()),
                  [(((n - 1) * 32,), torch.uint8), ((ws_bytes,), torch.uint8)], message, gpu_device)
    assert lib.pa_linkage_chain_workspace_bytes(1) == 0


def test_non_finite_matrix_raises_before_the_merge(gpu_device):
    """a zero row makes its cosine distances NaN: SciPy's ValueError, and the merge kernel is never launched (`raw`
    keeps its fill pattern)"""
    from pyannote_audio_amd import distance
    X = clustered(40, 8, seed=4)
    X[17] = 0.0
    with np.errstate(invalid="ignore"), pytest.raises(ValueError) as scipy_error:
        linkage(X, method="average", metric="cosine")
    for method in METHODS:
        whole, raw = guarded(39 * 4, gpu_device)
        with pytest.raises(ValueError) as ours:
            distance.linkage_chain(X.copy(), method, "cosine", gpu_device, raw=raw.view(39, 4))
        assert str(ours.value) == str(scipy_error.value) == "The condensed distance matrix must contain only finite values."
        torch.cuda.synchronize()
        assert bool(torch.isnan(whole).all()), "the merge kernel ran on a non-finite matrix"
    # the same rows are fine under the Euclidean metric
    assert_same_dendrogram(distance.linkage_chain(X.copy(), "average", "euclidean", gpu_device),
                           linkage(pdist(X, "euclidean"), "average"), "zero row, euclidean")


@pytest.fixture(scope="module")
def conversation():
    """300 chunks x 3 speakers: embeddings around three centres and a binary segmentation cut from the activity of
    oracle.synthetic.synth_conversation (10 s chunks every second, 40 frames each; 200 Hz is enough for activity)."""
    from oracle.synthetic import synth_conversation
    from pyannote_audio_amd.core import SlidingWindow, SlidingWindowFeature
    C, S, F, sr = 300, 3, 40, 200
    _, act = synth_conversation(C + 9.0, sr=sr, num_speakers=S, seed=3)
    frames = (np.arange(F) * (10 * sr // F) + 5 * sr // F)
    seg = np.stack([act[:, c * sr + frames].T for c in range(C)]).astype(np.float32)      # (C, F, S)
    rng = np.random.default_rng(8)
    centers = rng.standard_normal((S, 32))
    emb = (centers[None] + 0.35 * rng.standard_normal((C, S, 32))).astype(np.float32)
    return emb, SlidingWindowFeature(seg, SlidingWindow(start=0.0, duration=10.0, step=1.0))


@pytest.mark.parametrize("method", METHODS + ("centroid", "median"))
def test_clustering_object_on_gpu_equals_unplaced(gpu_device, conversation, method):
    """AgglomerativeClustering with the 3.1 threshold and min_cluster_size: hard clusters, soft scores and centroids
    of the object on the GPU equal those of the unplaced (SciPy) object, for the five methods that now run on the
    device and for centroid and median, which keep their paths."""
    import pyannote_audio_amd as pa
    emb, seg = conversation
    params = {"method": method, "min_cluster_size": 12, "threshold": 0.7045654963945799}
    on_gpu = pa.AgglomerativeClustering(metric="cosine").instantiate(params).to(gpu_device)
    unplaced = pa.AgglomerativeClustering(metric="cosine").instantiate(params)
    got = on_gpu(embeddings=emb.copy(), segmentations=seg)
    want = unplaced(embeddings=emb.copy(), segmentations=seg)
    assert on_gpu.timings["num_embeddings"] > 100
    if method != "median":
        # the device branches report no separate pdist time; the host path (median, or a None from linkage_chain) does
        assert on_gpu.timings["pdist"] == 0.0, f"{method} did not take the device branch"
    for name, g, w in zip(("hard clusters", "soft scores", "centroids"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w, equal_nan=True), f"{method}: {name} differ"


def test_size_above_the_cap_keeps_the_host_path(gpu_device, monkeypatch):
    """PA_LINKAGE_FAST_MAX_GB caps the square copy: above it `linkage_chain` answers None and the dendrogram is
    SciPy's, computed on the host as before"""
    import pyannote_audio_amd as pa
    from pyannote_audio_amd import distance
    monkeypatch.setenv("PA_LINKAGE_FAST_MAX_GB", "0.000001")      # 1 kB: n = 65 needs 37 kB
    X = clustered(65, 16, 65, dup=6)
    assert distance.linkage_chain(X.copy(), "average", "cosine", gpu_device) is None
    clu = pa.AgglomerativeClustering(metric="cosine").instantiate(
        {"method": "average", "min_cluster_size": 2, "threshold": 0.7}).to(gpu_device)
    assert_same_dendrogram(clu.dendrogram(X.copy()), linkage(X, method="average", metric="cosine"), "above the cap")
