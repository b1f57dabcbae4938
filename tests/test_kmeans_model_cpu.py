"""The float64 restatement of scikit-learn's KMeans that the GPU tests hold `pa_kmeans_f64` to
(tests/kmeans_model.py) equals scikit-learn itself: labels, iteration count, winning initialisation, k-means++ picks,
under the default settings and with other tolerances and iteration limits; and no input of the tables sits on a knife
edge, where the device's other order of additions could move an integer."""
import warnings

import numpy as np
import pytest

import kmeans_model as km

CASES = [(row, km.SEEDS) for row in km.TABLE] + [(row, km.EXTRA_SEEDS) for row in km.EXTRA]


def sklearn_fit(X64, k, n_init=3, **kw):
    from sklearn.cluster import KMeans
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # ConvergenceWarning of max_iter = 1, 2
        return KMeans(n_clusters=k, n_init=n_init, random_state=42, **kw).fit(X64.copy())


def sklearn_winner(X64, k, **kw):
    """(fit with 3 initialisations, index of the one it kept): a later initialisation replaces the best only with
    another labelling, so the winner is the last m at which the labels of `n_init = m + 1` changed"""
    fits = [sklearn_fit(X64, k, n_init=m, **kw) for m in (1, 2, 3)]
    winner = 0
    for m in (1, 2):
        if not np.array_equal(fits[m].labels_, fits[m - 1].labels_):
            winner = m
    return fits[2], winner


@pytest.mark.parametrize("row,seeds", CASES)
def test_model_equals_sklearn(row, seeds):
    n, d, g, k, noise = row
    for seed in seeds:
        for dtype in (np.float32, np.float64):
            X = km.data(n, d, g, noise, seed, dtype)
            model = km.kmeans(X, k)
            fit, winner = sklearn_winner(X.astype(np.float64), k)
            best = model["best"]
            assert best == winner
            assert np.array_equal(model["labels"][best], fit.labels_)
            assert model["status"][best, 0] == fit.n_iter_
            # off the knife edges: a point's two nearest final centres, every iteration's shift against tolv
            gap, ratio = km.knife_edges(model)
            assert gap > 1e-5 and ratio > 1e-6


def test_every_initialisation_wins_somewhere():
    wins = {km.kmeans(km.data(n, d, g, noise, seed, np.float32), k)["best"]
            for n, d, g, k, noise in km.TABLE for seed in km.SEEDS}
    assert wins == {0, 1, 2}


@pytest.mark.parametrize("kw", [{"tol": 0.05}, {"tol": 0.0}, {"max_iter": 1}, {"max_iter": 2}])
@pytest.mark.parametrize("row", [km.TABLE[3], km.TABLE[4], km.TABLE[1]])
def test_model_equals_sklearn_with_other_settings(row, kw):
    n, d, g, k, noise = row
    kinds = set()
    for seed in km.SEEDS:
        X = km.data(n, d, g, noise, seed, np.float64)
        model = km.kmeans(X, k, **kw)
        fit, winner = sklearn_winner(X, k, **kw)
        best = model["best"]
        assert best == winner
        assert np.array_equal(model["labels"][best], fit.labels_)
        assert model["status"][best, 0] == fit.n_iter_
        kinds |= set(model["status"][:, 1].tolist())
    if "max_iter" in kw:        # (two iterations can also end in a strict stop)
        assert km.MAX_ITER in kinds
    if kw.get("tol") == 0.05:
        assert km.TOL in kinds
    if kw.get("tol") == 0.0:
        assert kinds == {km.STRICT}


@pytest.mark.parametrize("row", km.TABLE)
def test_picks_equal_sklearn_kmeans_plusplus(row):
    from sklearn.cluster import kmeans_plusplus
    n, d, g, k, noise = row
    for seed in km.SEEDS:
        model = km.kmeans(km.data(n, d, g, noise, seed, np.float32), k)
        rs = np.random.RandomState(42)
        for i in range(3):
            _, picks = kmeans_plusplus(model["Xc"], k, random_state=rs)
            assert np.array_equal(picks, model["picks"][i])
            # (the Lloyd iterations in between draw nothing)


def test_duplicate_points_raise_the_empty_flag():
    model = km.kmeans(km.duplicate_points(), 5)
    assert model["empty"] and model["best"] is None and model["status"][:, 2].all()


def test_host_helpers_of_the_device_route():
    """`distance.kmeans_draws` and `distance.kmeans_select` are the model's `draws` and `select`"""
    import pyannote_audio_amd.distance as distance
    first, uniforms = distance.kmeans_draws(257, 8, 3, 42)
    want_first, want_uniforms = km.draws(257, 8, 3, 42)
    assert np.array_equal(first, want_first) and np.array_equal(uniforms, want_uniforms)
    assert uniforms.shape == (3, 7, 2 + int(np.log(8)))
    rng = np.random.default_rng(0)
    for _ in range(200):
        k = int(rng.integers(2, 6))
        a = rng.integers(0, k, 40)
        labels = np.array([a, rng.permutation(k)[a] if rng.random() < 0.5 else rng.integers(0, k, 40),
                           rng.integers(0, k, 40)], dtype=np.int32)
        inertia = rng.random(3)
        assert distance.kmeans_select(labels, inertia, k) == km.select(labels, inertia, k)


def test_no_device_means_none_and_the_host_route():
    """without a CUDA device `distance.kmeans` answers None, and an unplaced KMeansClustering makes scikit-learn's call"""
    import torch
    import pyannote_audio_amd as pa
    import pyannote_audio_amd.distance as distance
    X = km.data(97, 16, 3, 1.2, 0, np.float32)
    assert distance.kmeans(X, 2, None) is None
    assert distance.kmeans(X, 2, torch.device("cpu")) is None
    clu = pa.KMeansClustering().instantiate({})
    assert clu.kmeans_on_device is True
    labels = clu.cluster(X.copy(), num_clusters=2)
    assert np.array_equal(labels, sklearn_fit(X, 2).labels_)
    assert clu.timings["kmeans_route"] == "host" and clu.timings["kmeans"] > 0
