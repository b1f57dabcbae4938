"""`pyannote_audio_amd.verification` on the GPU, held to the numpy truth (tests/verification_truth.py, itself equal to
sklearn's roc_curve + det_curve's lines: tests/test_verification_cpu.py) and to SciPy's cdist with `==`: everything
here is integer counting and single float64 divisions, so there is no tolerance.  `np.array_equal` treats -0.0 and
0.0 as equal, so the thresholds' sign of zero is compared with `np.signbit` as well.  Every entry point is called
twice and the two results must have the same bits."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from verification_truth import B, CHUNK, det_curve_truth, large_zero_mix_case, scan_case, small_cases  # noqa: E402
# the seeded-checkpoint helpers of the embedding interface tests (fixtures included)
from test_embedding_inference_gpu import SR, _file, _wave, models, segmentation  # noqa: E402,F401

pytestmark = pytest.mark.gpu

CASES = small_cases()


def _bits(curve):
    fpr, fnr, thresholds, eer = curve
    return fpr.tobytes(), fnr.tobytes(), thresholds.tobytes(), np.float64(eer).tobytes()


def _check_curve(y_true, scores, distances, want=None):
    from pyannote_audio_amd import verification as v
    want = det_curve_truth(y_true, scores, distances) if want is None else want
    first, second = v.det_curve(y_true, scores, distances=distances), v.det_curve(y_true, scores, distances=distances)
    assert _bits(first) == _bits(second)
    fpr, fnr, thresholds, eer = first
    assert fpr.dtype == fnr.dtype == thresholds.dtype == np.float64 and isinstance(eer, float)
    assert np.array_equal(fpr, want[0]) and np.array_equal(fnr, want[1]) and np.array_equal(thresholds, want[2])
    assert np.array_equal(np.signbit(thresholds), np.signbit(want[2]))
    assert eer == want[3]
    assert fpr[want[4]] > fnr[want[4]] and not (fpr[:want[4]] > fnr[:want[4]]).any()
    alone = [v.equal_error_rate(y_true, scores, distances=distances) for _ in range(2)]
    assert alone[0] == alone[1] == want[3]


@pytest.mark.parametrize("distances", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_det_curve_case(gpu_device, name, distances):
    _check_curve(*CASES[name], distances)


@pytest.fixture(scope="module")
def scan():
    y_true, scores = scan_case()
    assert len(scores) == B * CHUNK + 1 <= 2 ** 21
    return y_true, scores, {d: det_curve_truth(y_true, scores, d) for d in (False, True)}


@pytest.mark.parametrize("distances", [False, True])
def test_det_curve_fills_every_scan_level(gpu_device, scan, distances):
    y_true, scores, want = scan
    assert len(want[distances][0]) > B * CHUNK // 4          # the kept points run into the second chunk too
    _check_curve(y_true, scores, distances, want=want[distances])


@pytest.mark.parametrize("distances", [False, True])
def test_signed_zeros_through_the_large_sort(gpu_device, distances):
    """the ±0 rule at a size where torch's sort takes its radix path: -0.0 and 0.0 stay one key in input order, so
    the zero group's counts and its threshold's sign (compared with np.signbit in _check_curve) equal numpy's"""
    from pyannote_audio_amd import verification as v
    y_true, scores = large_zero_mix_case()
    zeros = scores == 0
    assert len(scores) == 40000 and np.signbit(scores[zeros]).any() and not np.signbit(scores[zeros]).all()
    want = det_curve_truth(y_true, scores, distances)
    at = np.flatnonzero(want[2] == 0)
    assert len(at) == 1 and np.signbit(want[2][at[0]])       # the first zero of the input is -0.0, the second 0.0
    assert v.det_geometry() == (B, CHUNK)
    _check_curve(y_true, scores, distances, want=want)


def test_det_curve_takes_device_tensors_where_they_lie(gpu_device):
    from pyannote_audio_amd import verification as v
    y_true, scores = CASES["rounded"]
    want = det_curve_truth(y_true, scores, True)
    s, y = torch.from_numpy(scores).to(gpu_device), torch.from_numpy(y_true).to(gpu_device)
    fpr, fnr, thresholds, eer = v.det_curve(y, s, distances=True)
    assert np.array_equal(fpr, want[0]) and np.array_equal(fnr, want[1]) and np.array_equal(thresholds, want[2])
    assert eer == want[3] == v.equal_error_rate(y.to(torch.int64), s, distances=True)
    assert torch.equal(s.cpu(), torch.from_numpy(scores))   # (the caller's tensor is not sorted or negated in place)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_refuses_non_finite_scores_then_works(gpu_device, bad):
    from pyannote_audio_amd import verification as v
    y_true, scores = CASES["rounded"]
    broken = scores.copy()
    broken[[3, 400]] = bad
    for distances in (False, True):
        with pytest.raises(ValueError, match="2 of the 500 scores are NaN or infinite"):
            v.det_curve(y_true, broken, distances=distances)
        with pytest.raises(ValueError, match="NaN or infinite"):
            v.equal_error_rate(y_true, broken, distances=distances)
        _check_curve(y_true, scores, distances)


def test_refuses_a_single_class_then_works(gpu_device):
    from pyannote_audio_amd import verification as v
    y_true, scores = CASES["rounded"]
    for labels in (np.zeros_like(y_true), np.ones_like(y_true)):
        with pytest.raises(ValueError, match="target and a non-target"):
            v.det_curve(labels, scores)
        with pytest.raises(ValueError, match="target and a non-target"):
            v.equal_error_rate(labels, scores, distances=True)
    _check_curve(y_true, scores, False)


# ------------------------------------------------------------------------------------------------ trial distances
def _cdist_kernel(table, device):
    """pa_cdist_cosine_f64(E, E) -> (N, N) numpy"""
    import pyannote_audio_amd.ffi as ffi
    E = torch.from_numpy(table).to(device)
    n, d = table.shape
    out = torch.empty((n, n), dtype=torch.float64, device=device)
    norms = torch.empty(2 * n, dtype=torch.float64, device=device)
    ffi.check(ffi.load().pa_cdist_cosine_f64(ffi.ptr(E), n, ffi.ptr(E), n, d, ffi.ptr(out), ffi.ptr(norms),
                                             ffi.stream()), "pa_cdist_cosine_f64")
    return out.cpu().numpy()


@pytest.mark.parametrize("D", [1, 2, 3, 255, 256])
def test_trial_distances(gpu_device, D):
    from scipy.spatial.distance import cdist
    from pyannote_audio_amd import verification as v
    rng = np.random.default_rng(D)
    for N in (1, 2, 100):
        table = rng.normal(size=(N, D))
        full = _cdist_kernel(table, gpu_device)
        for T in (1, 129):
            index1, index2 = rng.integers(0, N, size=T), rng.integers(0, N, size=T)
            index1[0] = index2[0] = N - 1                       # i == j
            if T > 4:
                index1[3:5], index2[3:5] = index1[1], index2[1]     # a pair three times over
                index1[5], index2[5] = index2[1], index1[1]         # ... and the other way round
            got = [v.trial_distances(table, index1, index2) for _ in range(2)]
            assert got[0].dtype == torch.float64 and got[0].device == gpu_device and got[0].shape == (T,)
            first, second = (g.cpu().numpy() for g in got)
            assert first.tobytes() == second.tobytes()
            want = np.array([cdist(table[i:i + 1], table[j:j + 1], "cosine")[0, 0] for i, j in zip(index1, index2)])
            assert np.array_equal(first, want) and np.array_equal(np.signbit(first), np.signbit(want))
            assert np.array_equal(first, full[index1, index2])
            # a device table and int32 device indices are used where they lie
            there = v.trial_distances(torch.from_numpy(table).to(gpu_device),
                                      torch.from_numpy(index1).to(gpu_device, torch.int32),
                                      torch.from_numpy(index2).to(gpu_device))
            assert there.cpu().numpy().tobytes() == first.tobytes()


def test_trial_distances_float32_table_is_scored_in_float64(gpu_device):
    from scipy.spatial.distance import cdist
    from pyannote_audio_amd import verification as v
    table = np.random.default_rng(1).normal(size=(7, 256)).astype(np.float32)
    index1, index2 = np.array([0, 1, 2, 6, 6]), np.array([3, 4, 5, 0, 6])
    got = v.trial_distances(table, index1, index2).cpu().numpy()
    want = np.array([cdist(table[i:i + 1], table[j:j + 1], "cosine")[0, 0] for i, j in zip(index1, index2)])
    assert np.array_equal(got, want)


def test_zero_embedding_gives_nan_which_the_curve_refuses(gpu_device):
    from pyannote_audio_amd import verification as v
    table = np.random.default_rng(2).normal(size=(4, 3))
    table[2] = 0.0
    dist = v.trial_distances(table, [0, 1, 2, 2], [1, 2, 3, 2])
    assert torch.isnan(dist).tolist() == [False, True, True, True]
    with pytest.raises(ValueError, match="3 of the 4 scores are NaN or infinite"):
        v.det_curve([True, False, True, False], dist, distances=True)
    with pytest.raises(ValueError, match="must lie in 0..3"):
        v.trial_distances(torch.from_numpy(table).to(gpu_device), torch.tensor([0, 4], device=gpu_device), [1, 2])


# ------------------------------------------------------------------------------------------------ EqualErrorRate
def test_equal_error_rate_metric(gpu_device):
    from pyannote_audio_amd import metrics, verification as v
    y_true, scores = CASES["rounded"]
    assert metrics.EqualErrorRate is v.EqualErrorRate
    for distances in (True, False):
        metric = v.EqualErrorRate(distances=distances)
        for first, stop in ((0, 7), (7, 300), (300, 500)):
            s, y = torch.from_numpy(scores[first:stop]), torch.from_numpy(y_true[first:stop])
            metric.update(s.to(gpu_device) if first else s, y)
        assert [t.shape[0] for t in metric.scores] == [7, 293, 200] and all(t.is_cuda for t in metric.scores)
        got = [metric.compute() for _ in range(2)]
        assert got[0].dtype == torch.float64 and got[0].ndim == 0 and torch.equal(got[0], got[1])
        assert got[0].item() == v.det_curve(y_true, scores, distances=distances)[3]
        assert got[0].item() == det_curve_truth(y_true, scores, distances)[3]
        metric.reset()
        assert metric.scores == [] and metric.y_true == []
        with pytest.raises(ValueError, match="before any update"):
            metric.compute()


# ------------------------------------------------------------------------------------------------ end to end
SECONDS = (2.1, 3.0, 2.5, 4.2, 3.3, 2.8)
PAIRS = ((0, 1, True), (2, 3, False), (0, 2, False), (1, 4, True), (5, 5, True), (3, 0, False), (4, 2, True),
         (1, 0, True), (5, 3, False), (2, 4, False))


@pytest.mark.parametrize("with_segmentation", [False, True])
def test_evaluate_trials(models, segmentation, gpu_device, with_segmentation):
    """With and without a segmentation model.  The voice-activity weights change the pooled embeddings, so the two
    runs do not share distances; what is the same in both, and asserted for each, is the contract: the result equals
    the truth on `scipy.cdist` of that pipeline's own `apply_batch(files)`, every file is embedded once, and the
    files, their order and the labels do not depend on the segmentation model."""
    from scipy.spatial.distance import cdist
    from pyannote_audio_amd import SpeakerEmbedding
    from pyannote_audio_amd import verification as v
    _, model = models["wespeaker"]
    files = [dict(_file(_wave(int(s * SR), seed=40 + i)), audio=f"utt{i}.wav") for i, s in enumerate(SECONDS)]
    trials = [{"file1": dict(files[a]), "file2": files[b], "reference": same} for a, b, same in PAIRS]
    first_seen = [0, 1, 2, 3, 4, 5]
    assert len(trials) == 10 and len({len(f["waveform"][0]) for f in files}) == 6
    pipeline = SpeakerEmbedding(embedding=model, segmentation=segmentation if with_segmentation else None)
    y_true = np.array([same for _, _, same in PAIRS])

    def truth(table):
        return np.array([cdist(table[a:a + 1], table[b:b + 1], "cosine")[0, 0] for a, b, _ in PAIRS])

    want_eer = det_curve_truth(y_true, truth(np.concatenate(pipeline.apply_batch(files))), True)[3]

    seen, returned = [], []
    inner = pipeline.apply_batch

    def counting(batch):
        batch = list(batch)
        seen.extend(f["audio"] for f in batch)
        out = inner(batch)
        returned.extend(out)
        return out

    pipeline.apply_batch = counting
    result = v.evaluate_trials(pipeline, trials)
    assert seen == [f"utt{i}.wav" for i in first_seen]                 # each file once, in order of appearance
    assert result["num_files"] == 6 and isinstance(result["eer"], float)
    assert result["eer"] == want_eer
    assert result["distances"].device == gpu_device and result["distances"].dtype == torch.float64
    assert np.array_equal(result["distances"].cpu().numpy(), truth(np.concatenate(returned)))
    assert result["y_true"].cpu().numpy().tolist() == y_true.tolist()

    del seen[:], returned[:]
    batched = v.evaluate_trials(pipeline, iter(trials), batch_size=4)    # 4 + 2 files
    assert sorted(seen) == sorted(f["audio"] for f in files) and batched["num_files"] == 6
    assert np.array_equal(batched["distances"].cpu().numpy(), truth(np.concatenate(returned)))
    assert batched["eer"] == det_curve_truth(y_true, batched["distances"].cpu().numpy(), True)[3]
