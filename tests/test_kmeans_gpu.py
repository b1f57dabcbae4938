"""GPU: KMeans on the device (`distance.kmeans`, `pa_kmeans_f64`, csrc/kmeans.hip) against the float64 restatement of
scikit-learn's algorithm (tests/kmeans_model.py, which tests/test_kmeans_model_cpu.py holds to scikit-learn) and
against scikit-learn itself, and the two places of clustering.py that call it.

Contract: scikit-learn's labels FOR THE SAME VALUES IN FLOAT64, numbering included; float64 with a fixed order of
additions, so a second call returns the same bits.  Integers (labels, picks, iteration counts, stop kinds) are compared
with `==`; the centres with `math.fsum` means and the inertia with the model within bounds worked out below."""
import functools
import math
import os
import warnings

import numpy as np
import pytest
import torch

import kmeans_model as km

pytestmark = pytest.mark.gpu

CASES = [(row, km.SEEDS) for row in km.TABLE] + [(row, km.EXTRA_SEEDS) for row in km.EXTRA]


def sklearn_fit(X, k, **kw):
    from sklearn.cluster import KMeans
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return KMeans(n_clusters=k, n_init=3, random_state=42, **kw).fit(X.copy())


@functools.lru_cache(maxsize=None)
def reference(row, seed, dtype_name):
    """(X, model, sklearn fit on the float64 values), computed once per input and left alone"""
    n, d, g, k, noise = row
    X = km.data(n, d, g, noise, seed, np.dtype(dtype_name).type)
    return X, km.kmeans(X, k), sklearn_fit(X.astype(np.float64), k)


def log(line):
    """the measured figures go to the test's output (`pytest -s` shows them)"""
    print(line)


@pytest.mark.parametrize("row,seeds", CASES)
def test_every_initialisation_equals_the_model_and_the_winner_sklearn(gpu_device, row, seeds):
    import pyannote_audio_amd.distance as distance
    n, d, g, k, noise = row
    worst_centre = worst_inertia = 0.0
    for seed in seeds:
        for dtype_name in ("float32", "float64"):
            X, model, fit = reference(row, seed, dtype_name)
            labels, out = distance.kmeans(X, k, gpu_device, details=True)
            assert labels.dtype == np.int32
            # every initialisation: labels, k-means++ picks, iterations and stop kind of the model; no flag
            assert np.array_equal(out["picks"], model["picks"])
            assert np.array_equal(out["status"], model["status"])
            assert np.array_equal(out["labels"], model["labels"])
            # the winner: scikit-learn's labels, numbering included, and its iteration count
            assert out["best"] == model["best"]
            assert np.array_equal(labels, fit.labels_)
            assert out["status"][out["best"], 0] == fit.n_iter_
            # winning centres against exactly rounded means of the float64 rows under those labels.  The kernel
            # subtracts the column mean (one rounding, |x - mean| <= 2 max|X|), adds at most n - 1 such terms one
            # after the other (recursive summation: relative error below (n - 1) 2^-53 of the sum of magnitudes),
            # divides and adds the mean back (one rounding): 2 n 2^-53 max|X| per coordinate
            X64 = X.astype(np.float64)
            bound = 2.0 * n * 2.0 ** -53 * np.abs(X64).max()
            centres = out["centers"][out["best"]]
            for j in range(k):
                members = X64[labels == j]
                want = np.array([math.fsum(col) for col in members.T]) / len(members)
                err = np.abs(centres[j] - want).max()
                worst_centre = max(worst_centre, err / bound)
                assert err <= bound
            # inertia: n D squared differences, each a few roundings, summed in another order than the model's
            rel = np.abs(out["inertia"] - model["inertia"]) / np.maximum(model["inertia"], 1e-300)
            worst_inertia = max(worst_inertia, rel.max() / (4.0 * n * d * 2.0 ** -53))
            assert (rel <= 4.0 * n * d * 2.0 ** -53).all()
    log(f"kmeans[n={n},d={d},k={k}]: centre error / bound = {worst_centre:.3f}, "
        f"inertia error / bound = {worst_inertia:.3f}")


# ---- the entry point itself -------------------------------------------------------------------------------------------
GUARD = 64      # elements in front of and behind every output


class LowLevel:
    """one `pa_kmeans_f64` call with guard bands around every output"""

    def __init__(self, X, k, device, n_init=3, max_iter=300, tol=1e-4, round_iterations=8, seed=42):
        import pyannote_audio_amd.distance as distance
        import pyannote_audio_amd.ffi as ffi
        lib = ffi.load()
        n, d = X.shape
        first, uniforms = distance.kmeans_draws(n, k, n_init, seed)
        self.shapes = {"labels": ((n_init, n), torch.int32), "centers": ((n_init, k, d), torch.float64),
                       "inertia": ((n_init,), torch.float64), "picks": ((n_init, k), torch.int32),
                       "status": ((n_init, 4), torch.int32)}
        self.fill = {torch.int32: -77, torch.float64: 1234.5}
        self.whole = {name: torch.full((math.prod(shape) + 2 * GUARD,), self.fill[dtype], dtype=dtype, device=device)
                      for name, (shape, dtype) in self.shapes.items()}
        Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(device)
        first_d, uniforms_d = torch.from_numpy(first).to(device), torch.from_numpy(uniforms).to(device)
        ws = torch.empty(lib.pa_kmeans_workspace_bytes(n, d, k, n_init), dtype=torch.uint8, device=device)
        p = {name: ffi.ptr(w[GUARD:]) for name, w in self.whole.items()}
        with torch.cuda.device(device):
            self.rc = lib.pa_kmeans_f64(ffi.ptr(Xd), n, d, k, n_init, ffi.ptr(first_d), ffi.ptr(uniforms_d), max_iter,
                                        tol, round_iterations, p["labels"], p["centers"], p["inertia"], p["picks"],
                                        p["status"], ffi.ptr(ws), ws.numel(), ffi.stream())
            torch.cuda.synchronize()
        self.host = {name: w.cpu().numpy() for name, w in self.whole.items()}

    def __getitem__(self, name):
        shape, _ = self.shapes[name]
        return self.host[name][GUARD:-GUARD].reshape(shape)

    def guards_untouched(self):
        return all((h[:GUARD] == self.fill[self.shapes[name][1]]).all()
                   and (h[-GUARD:] == self.fill[self.shapes[name][1]]).all() for name, h in self.host.items())


@pytest.mark.parametrize("kw", [{"tol": 0.05}, {"tol": 0.0}, {"max_iter": 1}, {"max_iter": 2}])
def test_tolerance_and_iteration_limit_through_the_entry_point(gpu_device, kw):
    """the tol stop and the iteration limit both end in one more assignment with the final centres; every output stays
    between its guard bands"""
    kinds = set()
    for row in (km.TABLE[3], km.TABLE[4], km.TABLE[1]):
        n, d, g, k, noise = row
        X = km.data(n, d, g, noise, 0, np.float64)
        model = km.kmeans(X, k, **kw)
        got = LowLevel(X, k, gpu_device, **kw)
        assert got.rc == 0 and got.guards_untouched()
        assert np.array_equal(got["status"], model["status"])
        assert np.array_equal(got["picks"], model["picks"])
        assert np.array_equal(got["labels"], model["labels"])
        assert np.allclose(got["centers"], model["centers"], rtol=0, atol=2.0 * n * 2.0 ** -53)   # (max|X| <= 1)
        kinds |= set(got["status"][:, 1].tolist())
    if "max_iter" in kw:
        assert km.MAX_ITER in kinds
    if kw.get("tol") == 0.05:
        assert km.TOL in kinds
    if kw.get("tol") == 0.0:
        assert kinds == {km.STRICT}


@pytest.mark.parametrize("row", [km.TABLE[4], km.TABLE[5], km.EXTRA[5]])
def test_a_second_call_returns_the_same_bits(gpu_device, row):
    """... in every output, guard bands included, whether the iterations are enqueued in rounds or all at once"""
    n, d, g, k, noise = row
    X = km.data(n, d, g, noise, 1 if row in km.TABLE else 0, np.float32)
    a, b = LowLevel(X, k, gpu_device), LowLevel(X, k, gpu_device)
    c = LowLevel(X, k, gpu_device, round_iterations=0, max_iter=40)
    assert a.rc == b.rc == c.rc == 0 and a.guards_untouched()
    for name in a.shapes:
        assert a.host[name].tobytes() == b.host[name].tobytes()
        assert a.host[name].tobytes() == c.host[name].tobytes()


REFUSALS = [
    (dict(k=1), "pa_kmeans_f64: fewer than 2 clusters"),
    (dict(k=65), "pa_kmeans_f64: more clusters than pa_kmeans_max_clusters()"),
    (dict(d=513), "pa_kmeans_f64: dimension outside 1..pa_kmeans_max_dim()"),
    (dict(n=4), "pa_kmeans_f64: fewer rows than clusters"),
    (dict(n=1 << 24), "pa_kmeans_f64: 2^24 rows or more"),
    (dict(n_init=0), "pa_kmeans_f64: n_init outside 1..65535"),
    (dict(max_iter=0), "pa_kmeans_f64: max_iter below 1"),
    (dict(ws_short=1), "pa_kmeans_f64: workspace too small"),
]


@pytest.mark.parametrize("change,message", REFUSALS)
def test_refusals(gpu_device, change, message):
    """return code 3 and the message before any launch; nobody writes to the outputs.  The buffers have the size of
    the accepted call (70 rows, 16 columns, 5 clusters): a refused size is only ever NAMED, and were the call wrongly
    accepted with the short workspace it would compute in bounds of the full one that is passed."""
    import pyannote_audio_amd.ffi as ffi
    from refusals import check_refusal
    lib = ffi.load()
    assert lib.pa_kmeans_max_clusters() == 64 and lib.pa_kmeans_max_dim() >= 512
    n, d, k, n_init, max_iter = 70, 16, 5, 3, 300
    X = torch.from_numpy(km.data(n, d, 3, 0.8, 0, np.float64)).to(gpu_device)
    first = torch.zeros(n_init, dtype=torch.int32, device=gpu_device)
    uniforms = torch.full((n_init, k - 1, 3), 0.5, dtype=torch.float64, device=gpu_device)
    ws = torch.empty(lib.pa_kmeans_workspace_bytes(n, d, k, n_init), dtype=torch.uint8, device=gpu_device)
    assert ws.numel() > 0
    named = dict(n=n, d=d, k=k, n_init=n_init, max_iter=max_iter)
    named.update({key: value for key, value in change.items() if key in named})
    ws_bytes = ws.numel() - change.get("ws_short", 0)
    if "ws_short" not in change and set(change) & {"n", "d", "k", "n_init"}:
        assert lib.pa_kmeans_workspace_bytes(named["n"], named["d"], named["k"], named["n_init"]) == 0

    def launch(labels, centers, inertia, picks, status):
        return lib.pa_kmeans_f64(ffi.ptr(X), named["n"], named["d"], named["k"], named["n_init"], ffi.ptr(first),
                                 ffi.ptr(uniforms), named["max_iter"], 1e-4, 8, labels, centers, inertia, picks, status,
                                 ffi.ptr(ws), ws_bytes, ffi.stream())
    outputs = [((4 * n_init * n,), torch.uint8), ((8 * n_init * k * d,), torch.uint8), ((8 * n_init,), torch.uint8),
               ((4 * n_init * k,), torch.uint8), ((4 * n_init * 4,), torch.uint8)]
    check_refusal(launch, outputs, message, gpu_device)


def test_what_the_device_route_gives_up_on(gpu_device):
    import pyannote_audio_amd.distance as distance
    X = km.data(97, 16, 3, 1.2, 0, np.float32)
    bad = X.copy()
    bad[5, 3] = np.nan
    assert distance.kmeans(bad, 2, gpu_device) is None
    assert distance.kmeans(km.duplicate_points(), 5, gpu_device) is None      # a cluster comes up empty
    assert distance.kmeans(X, 65, gpu_device) is None                         # beyond pa_kmeans_max_clusters()
    assert distance.kmeans(X, 98, gpu_device) is None                         # more clusters than rows
    assert np.array_equal(distance.kmeans(X, 1, gpu_device), np.zeros(97, dtype=np.int32))
    # the flags themselves: the duplicate points raise the empty-cluster flag of every job, NaN the non-finite one
    dup = LowLevel(km.duplicate_points(np.float64), 5, gpu_device)
    assert dup.rc == 0 and dup.guards_untouched() and dup["status"][:, 2].all() and not dup["status"][:, 3].any()
    nan = LowLevel(bad.astype(np.float64), 2, gpu_device)
    assert nan.rc == 0 and nan.guards_untouched() and nan["status"][:, 3].all()


# ---- the two callers ---------------------------------------------------------------------------------------------------
def _embeddings(C, K, noise, seed, D_=256, F=60, S=3):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((K, D_))
    who = rng.integers(0, K, size=(C, S))
    emb = (centers[who] + noise * rng.standard_normal((C, S, D_))).astype(np.float32)
    seg = (rng.uniform(size=(C, F, S)) < 0.45).astype(np.float32)
    seg[rng.integers(0, C, C // 8), :, rng.integers(0, S, C // 8)] = 0.0
    return emb, seg


class _Patched(RuntimeError):
    pass


def _raise(*args, **kwargs):
    raise _Patched("sklearn.cluster.KMeans was called")


def test_kmeans_clustering_on_the_gpu_equals_the_unplaced_object(gpu_device, monkeypatch):
    import pyannote_audio_amd as pa
    import pyannote_audio_amd.distance as distance
    from pyannote_audio_amd.core import SlidingWindow, SlidingWindowFeature
    emb, seg = _embeddings(200, 3, 0.8, 21)
    chunks = SlidingWindow(start=0.0, duration=10.0, step=1.0)

    def run(clu):
        return clu(embeddings=emb.copy(), segmentations=SlidingWindowFeature(seg, chunks), num_clusters=3)
    want = run(pa.KMeansClustering().instantiate({}))
    assert want[2].shape == (3, 256)
    device_route = distance.kmeans
    with monkeypatch.context() as m:
        m.setattr("sklearn.cluster.KMeans", _raise)
        clu = pa.KMeansClustering().instantiate({}).to(gpu_device)
        got = run(clu)                                   # the device computed it: scikit-learn is not there
        assert clu.timings["kmeans_route"] == "device" and clu.timings["kmeans"] > 0
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        clu.kmeans_on_device = False
        with pytest.raises(_Patched):
            run(clu)
    with monkeypatch.context() as m:
        m.setattr(distance, "kmeans", lambda *args, **kwargs: None)
        clu = pa.KMeansClustering().instantiate({}).to(gpu_device)
        got = run(clu)
        assert clu.timings["kmeans_route"] == "host"
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    assert distance.kmeans is device_route


@pytest.fixture(scope="module")
def plda_dir(tmp_path_factory):
    from oracle.vbx import synth_plda
    return synth_plda(str(tmp_path_factory.mktemp("plda")))


#: (chunks, speakers, noise, seed, bounds): more clusters asked for than VBx finds, and fewer allowed.  Checked on the
#: CPU with the oracle: VBx keeps 2 and 3 speakers, and on these training sets (136 and 149 rows) scikit-learn's float32
#: run and the float64 model give the same labels
@pytest.mark.parametrize("C,K,noise,seed,kw", [(280, 3, 0.8, 12, {"num_clusters": 5}),
                                               (330, 5, 0.9, 16, {"max_clusters": 2})])
def test_vbx_forced_counts_take_the_device_route(plda_dir, gpu_device, C, K, noise, seed, kw):
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.core import SlidingWindow, SlidingWindowFeature
    from oracle.vbx import PLDA as OraclePLDA, vbx_clustering
    emb, seg = _embeddings(C, K, noise, seed)
    params = {"threshold": 0.6, "Fa": 0.07, "Fb": 0.8}
    clu = pa.VBxClustering(plda=plda_dir).instantiate(params).to(gpu_device)
    chunks = SlidingWindow(start=0.0, duration=10.0, step=1.0)
    hard, soft, cen = clu(embeddings=emb.copy(), segmentations=SlidingWindowFeature(seg, chunks),
                          min_clusters=kw.get("num_clusters", 1), max_clusters=kw.get("num_clusters",
                                                                                      kw.get("max_clusters", np.inf)),
                          num_clusters=kw.get("num_clusters"))
    assert clu.timings["vbx_speakers"] != kw.get("num_clusters", kw.get("max_clusters"))
    assert clu.timings["kmeans_route"] == "device"
    ref = OraclePLDA(os.path.join(plda_dir, "xvec_transform.npz"), os.path.join(plda_dir, "plda.npz"))
    rh, rs, rc = vbx_clustering(emb.copy(), seg, ref, num_clusters=kw.get("num_clusters"),
                                min_clusters=kw.get("num_clusters"), max_clusters=kw.get("num_clusters",
                                                                                         kw.get("max_clusters")),
                                **params)
    assert cen.shape == rc.shape
    assert np.array_equal(hard, rh)
    assert np.allclose(cen, rc, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("seed,k", [(100, 9), (101, 9), (100, 4)])
def test_hour_sized_training_set(gpu_device, seed, k):
    """7 176 unit vectors of 256 dimensions in 6 groups: the device labels are scikit-learn's on the float64 values;
    how many differ from its float32 run is printed, not asserted (k = 9 cuts homogeneous clouds, whose boundaries
    move with the rounding: DESIGN.md section 27 records the counts)"""
    import pyannote_audio_amd.distance as distance
    X = km.data(7176, 256, 6, 0.8, seed, np.float32)
    labels, out = distance.kmeans(X, k, gpu_device, details=True)
    fit64 = sklearn_fit(X.astype(np.float64), k)
    fit32 = sklearn_fit(X, k)
    log(f"kmeans hour-sized[seed={seed},k={k}]: {int((labels != fit64.labels_).sum())} labels differ from "
        f"scikit-learn on float64, {int((labels != fit32.labels_).sum())} from scikit-learn on float32; "
        f"iterations {out['status'][:, 0].tolist()}, winner {out['best']}")
    assert np.array_equal(labels, fit64.labels_)
    assert out["status"][out["best"], 0] == fit64.n_iter_
