"""Host side of `pyannote_audio_amd.verification`: the numpy truth that the GPU tests hold the kernels to equals
sklearn's roc_curve + det_curve's lines and the committed golden with `==`; the checks that run before anything is
launched refuse bad input; without a GPU the device parts raise."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from verification_truth import B, CHUNK, det_curve_truth, large_zero_mix_case, scan_case, small_cases  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "verification_v1.npz")


def _same(got, want):
    """(fpr, fnr, thresholds, eer, k) equal with ==, the thresholds' sign of zero included"""
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    assert np.array_equal(np.signbit(got[2]), np.signbit(want[2]))
    assert got[3] == want[3] and got[4] == want[4]


@pytest.fixture(scope="module")
def cases():
    return small_cases()


@pytest.mark.parametrize("distances", [False, True])
def test_truth_equals_sklearn(cases, distances):
    pytest.importorskip("sklearn")
    from make_verification_golden import sklearn_det_curve
    for name, (y_true, scores) in list(cases.items()) + [("scan", scan_case()), ("zeros", large_zero_mix_case())]:
        _same(det_curve_truth(y_true, scores, distances), sklearn_det_curve(y_true, scores, distances))


@pytest.mark.parametrize("distances", [False, True])
def test_truth_equals_golden(cases, distances):
    golden = np.load(GOLDEN)
    names = {key.split("/")[0] for key in golden.files if "/" in key}
    assert names == set(cases)
    for name, (y_true, scores) in cases.items():
        assert np.array_equal(golden[f"{name}/y_true"], y_true) and golden[f"{name}/y_true"].dtype == y_true.dtype
        assert np.array_equal(golden[f"{name}/scores"], scores) and golden[f"{name}/scores"].dtype == scores.dtype
        assert np.array_equal(np.signbit(golden[f"{name}/scores"]), np.signbit(scores))
        tag = f"{name}/{'distances' if distances else 'scores'}"
        want = (golden[f"{tag}/fpr"], golden[f"{tag}/fnr"], golden[f"{tag}/thresholds"], float(golden[f"{tag}/eer"]),
                int(golden[f"{tag}/k"]))
        _same(det_curve_truth(y_true, scores, distances), want)


def test_cases_are_what_they_claim(cases):
    """the shapes the kernels can go wrong at are really in the cases"""
    fpr, fnr, thresholds, _, k = det_curve_truth(*cases["all_equal"])
    assert len(fpr) == 2 and k == 1
    assert len(det_curve_truth(*cases["two_groups"])[0]) == 3
    # no error at the best threshold: the crossing is the jump from (0, 0) to (1, 0) in (fpr, fnr), or its mirror
    assert det_curve_truth(*cases["separated"])[3] == 0.25 and det_curve_truth(*cases["inverted"])[3] == 0.75
    assert det_curve_truth(*cases["first_point_crosses"])[4] == 1
    # the zero group's threshold is the sign of the element that ends it, and both signs occur
    zeros = [det_curve_truth(*cases[name], distances)[2] for name in ("signed_zeros", "signed_zeros_ends_positive")
             for distances in (False, True)]
    signs = {bool(np.signbit(t[t == 0][0])) for t in zeros}
    assert signs == {False, True}
    # a tie group on both sides of the first workgroup boundary
    y_true, scores = cases[f"block_{B + 1}"]
    ranked = np.sort(scores)[::-1]
    assert ranked[B - 3] == ranked[B] and ranked[B - 4] != ranked[B - 3]
    # the crossing's predecessor lies more than two workgroups back
    y_true, scores = cases["long_negative_run"]
    fpr, fnr, _, _, k = det_curve_truth(y_true, scores)
    negatives = int((~y_true).sum())
    assert round((fpr[k] - fpr[k - 1]) * negatives) > 2 * B and fnr[k] == fnr[k - 1]
    assert cases["float32_bool"][1].dtype == np.float32 and cases["float32_int64"][0].dtype == np.int64


def test_truth_refuses_what_the_module_refuses():
    for scores in ([0.1, np.nan, 0.3], [0.1, np.inf, 0.3], [0.1, -np.inf, 0.3]):
        with pytest.raises(ValueError):
            det_curve_truth([1, 0, 1], scores)
    for y_true in ([1, 1, 1], [0, 0, 0]):
        with pytest.raises(ValueError):
            det_curve_truth(y_true, [0.1, 0.2, 0.3])


def test_host_side_refusals():
    """raised before any device is asked for, so they are the same with and without a GPU"""
    from pyannote_audio_amd import verification as v
    table = np.arange(12, dtype=np.float64).reshape(4, 3)
    for index1, index2 in (([0, 4], [1, 2]), ([0, 1], [-1, 2]), (torch.tensor([0, 7]), torch.tensor([1, 2]))):
        with pytest.raises(ValueError, match=r"must lie in 0\.\.3"):
            v.trial_distances(table, index1, index2)
    with pytest.raises(ValueError, match="one entry per trial"):
        v.trial_distances(table, [0, 1, 2], [1, 2])
    with pytest.raises(ValueError, match="integers"):
        v.trial_distances(table, [0.0, 1.0], [1, 2])
    with pytest.raises(ValueError, match="one-dimensional"):
        v.trial_distances(table, [[0, 1]], [[1, 2]])
    with pytest.raises(ValueError, match="num_embeddings, dimension"):
        v.trial_distances(table[0], [0], [0])
    for metric in ("euclidean", "angular", None):
        with pytest.raises(ValueError, match="cosine"):
            v.trial_distances(table, [0, 1], [1, 2], metric=metric)
    for entry in (v.det_curve, v.equal_error_rate):
        with pytest.raises(ValueError, match="one length"):
            entry([True, False, True], [0.5, 0.25])
        with pytest.raises(ValueError, match="target and a non-target"):
            entry([True], [0.5])
    metric = v.EqualErrorRate()
    with pytest.raises(ValueError, match="one length"):
        metric.update(torch.zeros(3), torch.zeros(2))
    with pytest.raises(ValueError, match="before any update"):
        metric.compute()
    with pytest.raises(ValueError, match="'audio' entry"):
        v.evaluate_trials(None, [{"file1": {"uri": "a"}, "file2": {"audio": "b.wav"}, "reference": True}])
    with pytest.raises(ValueError, match="no trials"):
        v.evaluate_trials(None, [])


def test_public_names():
    import pyannote_audio_amd as pkg
    from pyannote_audio_amd import metrics, verification
    assert pkg.verification is verification
    assert metrics.EqualErrorRate is verification.EqualErrorRate
    assert verification.EqualErrorRate().distances is True


def test_cases_sit_on_the_kernels_boundaries():
    """the block and scan-level cases are built from B and CHUNK: both are the constants the library was compiled with"""
    from pyannote_audio_amd import verification
    assert verification.det_geometry() == (B, CHUNK)
    assert len(scan_case()[1]) == B * CHUNK + 1 <= 2 ** 21


def test_raises_without_a_gpu(cases):
    from pyannote_audio_amd import verification as v
    if torch.cuda.is_available():
        return                                   # (the device parts run: tests/test_verification_gpu.py)
    y_true, scores = cases["t3"]
    table = np.eye(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.trial_distances(table, [0, 1], [1, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.det_curve(y_true, scores)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.equal_error_rate(y_true, scores, distances=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.EqualErrorRate().update(torch.from_numpy(scores), torch.from_numpy(y_true))
    trial = {"file1": {"audio": "a.wav"}, "file2": {"audio": "b.wav"}, "reference": True}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.evaluate_trials(None, [trial])
