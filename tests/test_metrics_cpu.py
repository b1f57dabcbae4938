"""pyannote_audio_amd.metrics without a GPU: the truth (tests/metrics_truth.py) equals the reference's own outputs
(tests/golden/metrics_v1.npz, regenerated and compared when the reference is present), and the host side of the metric
classes -- dispatch, accumulation, speaker padding, `uem` handling, argument errors -- with the truth standing in for
the counting kernel (there is no host implementation of the counting in the product: it raises without a GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import metrics_truth  # noqa: E402

KEYS = ("false alarm", "missed detection", "confusion", "total")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "metrics_v1.npz")))


def chunk_case(golden, name):
    """-> preds float32, target uint8 (both padded to the common number of speakers), thresholds (Q,) float32,
    scalar?, near_tie (B,)"""
    preds = golden[f"chunk/{name}/preds"].astype(np.float32)
    target = golden[f"chunk/{name}/target"]
    S = max(preds.shape[1], target.shape[1])
    preds = np.pad(preds, ((0, 0), (0, S - preds.shape[1]), (0, 0)))
    target = np.pad(target, ((0, 0), (0, S - target.shape[1]), (0, 0)))
    thresholds = golden[f"chunk/{name}/thresholds"]
    scalar = thresholds.ndim == 0
    return preds, target, thresholds.astype(np.float32).reshape(-1), scalar, golden[f"chunk/{name}/near_tie"]


def test_truth_equals_reference_file_mode(golden):
    assert len(golden["file_cases"]) >= 15
    for name in golden["file_cases"]:
        reference, hypothesis = golden[f"file/{name}/reference"], golden[f"file/{name}/hypothesis"]
        want = dict(zip(KEYS, (int(v) for v in golden[f"file/{name}/components"])))
        assert metrics_truth.file_components(reference, hypothesis) == want, name
        # ... and the counts the kernel takes give the same components: confusion = both - correct
        from pyannote_audio_amd.metrics import _rate, components_from_counts
        got = components_from_counts(metrics_truth.der_counts(reference, hypothesis))
        assert got == want, name
        if f"file/{name}/der" in golden:
            # the reference's rate is ONE half-precision division of exactly represented sums: relative 2^-11
            ref_der, ours = float(golden[f"file/{name}/der"]), _rate(got)
            if np.isfinite(ours):
                assert abs(ref_der - ours) <= 2.0 ** -11 * abs(ours), name
            else:
                assert np.isnan(ref_der) == np.isnan(ours) and np.isinf(ref_der) == np.isinf(ours), name


def test_truth_equals_reference_chunk_mode(golden):
    assert len(golden["chunk_cases"]) >= 12
    left_out = total = 0
    for name in golden["chunk_cases"]:
        preds, target, thresholds, scalar, near = chunk_case(golden, name)
        counts, speech = metrics_truth.chunk_components(preds, target, thresholds)
        keep = ~near
        left_out += int(near.sum())
        total += len(near)
        for k, key in enumerate(("false_alarm", "missed_detection", "confusion")):
            want = golden[f"chunk/{name}/chunk_{key}"].reshape(len(near), -1)
            assert np.array_equal(counts[keep][:, :, k], want[keep]), (name, key)
            if not near.any():
                assert np.array_equal(counts[:, :, k].sum(axis=0), golden[f"chunk/{name}/batch_{key}"].reshape(-1))
        assert np.array_equal(speech, golden[f"chunk/{name}/chunk_total"]), name
        assert speech.sum() == golden[f"chunk/{name}/batch_total"], name
    assert left_out <= 0.01 * total


def test_golden_regenerates_from_the_reference(golden):
    import refharness
    if not refharness.available():
        pytest.skip("the reference tree is not on this machine")
    import make_metrics_golden
    fresh = make_metrics_golden.generate()
    assert set(fresh) == set(golden)
    for key, value in fresh.items():
        assert np.array_equal(np.asarray(value), golden[key], equal_nan=np.asarray(value).dtype.kind == "f"), key


def test_permutation_margin_is_the_written_bound():
    # 2 S (F + 2) u with u = 2^-24
    assert metrics_truth.permutation_margin(3, 589) == 2 * 3 * 591 * 2.0 ** -24


# ------------------------------------------------------------------------------------ the classes' host side
@pytest.fixture
def M(monkeypatch):
    import pyannote_audio_amd.metrics as metrics
    monkeypatch.setattr(metrics, "der_counts", metrics_truth.der_counts)
    return metrics


def random_pair(seed, T=400, Sr=3, Sh=3):
    rng = np.random.default_rng(seed)
    return (rng.random((T, Sr)) < 0.3).astype(np.uint8), (rng.random((T, Sh)) < 0.3).astype(np.uint8)


def test_exported_from_the_package():
    import pyannote_audio_amd as pa
    assert pa.DiscreteDiarizationErrorRate is pa.metrics.DiscreteDiarizationErrorRate
    assert pa.diarization_error_rate is pa.metrics.diarization_error_rate
    assert pa.optimal_diarization_error_rate is pa.metrics.optimal_diarization_error_rate
    assert pa.discrete_diarization_error_rate is pa.metrics.discrete_diarization_error_rate


def test_accumulation_and_reset(M):
    metric = M.DiscreteDiarizationErrorRate()
    assert metric.metric_name() == "discrete diarization error rate"
    assert metric.metric_components() == ["total", "false alarm", "missed detection", "confusion"]
    files = [random_pair(1), random_pair(2, T=77), random_pair(3, Sr=2, Sh=5)]
    want = {k: 0 for k in KEYS}
    for reference, hypothesis in files:
        value = metric(reference, hypothesis)
        one = metrics_truth.file_components(reference, hypothesis)
        assert value == (one["false alarm"] + one["missed detection"] + one["confusion"]) / one["total"]
        for k in KEYS:
            want[k] += one[k]
    assert metric[:] == want and all(type(v) is int for v in metric[:].values())
    assert metric["confusion"] == want["confusion"]
    assert abs(metric) == (want["false alarm"] + want["missed detection"] + want["confusion"]) / want["total"]
    assert abs(metric) == metric.compute_metric(want)
    assert len(list(metric)) == 3
    detailed = metric(*files[0], detailed=True)
    assert {k: detailed[k] for k in KEYS} == metrics_truth.file_components(*files[0])
    assert detailed["discrete diarization error rate"] == metric.compute_metric(detailed)
    metric.reset()
    assert metric[:] == {k: 0 for k in KEYS} and list(metric) == []
    assert np.isnan(abs(metric))


def test_padding_equals_the_reference_class(M, golden):
    metric = M.DiscreteDiarizationErrorRate()
    padded = [n for n in golden["file_cases"] if n.startswith("padded")]
    assert len(padded) == 4
    for name in padded:
        got = metric.compute_components(golden[f"file/{name}/reference"], golden[f"file/{name}/hypothesis"])
        assert [got[k] for k in KEYS] == golden[f"file/{name}/components"].tolist(), name
        # torch tensors take the same road
        got = metric.compute_components(torch.from_numpy(golden[f"file/{name}/reference"]),
                                        torch.from_numpy(golden[f"file/{name}/hypothesis"]))
        assert [got[k] for k in KEYS] == golden[f"file/{name}/components"].tolist(), name


def conversation(seed=0, duration=60.0, speakers=3):
    from pyannote_audio_amd.core import Annotation, Segment
    rng = np.random.default_rng(seed)
    reference = Annotation(uri="conv")
    t, n = 0.3, 0
    while t < duration - 3:
        d = float(rng.uniform(0.5, 3.0))
        reference[Segment(t, t + d), n] = f"spk{int(rng.integers(speakers))}"
        t += d * float(rng.uniform(0.5, 1.2))
        n += 1
    return reference


def test_uem_becomes_the_frame_mask(M):
    from pyannote_audio_amd.core import Segment, SlidingWindow, SlidingWindowFeature
    frames = SlidingWindow(start=0.0, duration=0.0619375, step=0.016875)
    reference = conversation()
    T = 3500
    rng = np.random.default_rng(5)
    extent = SlidingWindowFeature(np.zeros((T, 1)), frames).extent
    truth = reference.discretize(extent, resolution=frames).data
    hyp = np.where(rng.random((T, 3)) < 0.85, truth[:T], rng.random((T, 3)) < 0.3).astype(np.float32)[:, [2, 0, 1]]
    hypothesis = SlidingWindowFeature(hyp, frames)
    metric = M.DiscreteDiarizationErrorRate()
    # without uem: the whole file, on the frames both sides have
    assert truth.shape[0] >= T
    assert metric.compute_components(reference, hypothesis) == metrics_truth.file_components(truth[:T], hyp)
    # with uem: the frames that the segments touch ("loose"), once each, under ONE mapping
    uem = M.Timeline([Segment(2.0, 11.5), Segment(30.0, 41.25), Segment(41.0, 45.0)])
    keep = np.zeros(T, dtype=bool)
    starts = frames.start + np.arange(T) * frames.step
    for segment in uem:
        keep |= (starts + frames.duration >= segment.start - 1e-9) & (starts <= segment.end + 1e-9)
    got = metric.compute_components(reference, hypothesis, uem=uem)
    assert got == metrics_truth.file_components(truth[:T], hyp, keep=keep)
    assert 0 < got["total"] < metrics_truth.file_components(truth[:T], hyp)["total"]
    # a plain list of segments serves as a uem; one that leaves the hypothesis' extent is refused
    assert metric.compute_components(reference, hypothesis, uem=list(uem)) == got
    with pytest.raises(ValueError, match="`uem` must fully cover hypothesis extent."):
        metric.compute_components(reference, hypothesis, uem=M.Timeline([Segment(50.0, 70.0)]))
    # through the accumulating call
    assert metric(reference, hypothesis, uem=uem, detailed=True)["total"] == got["total"]


def test_chunked_hypothesis_skips_windows_the_uem_does_not_cover(M):
    from pyannote_audio_amd.core import Segment, SlidingWindow, SlidingWindowFeature
    chunks = SlidingWindow(start=0.0, duration=5.0, step=2.5)
    C, F, K = 20, 293, 3
    reference = conversation(seed=3)
    rng = np.random.default_rng(9)
    data = (rng.random((C, F, K)) < 0.3).astype(np.uint8)
    hypothesis = SlidingWindowFeature(data, chunks)
    support = Segment(chunks[0].start, chunks[C - 1].end)
    discrete = reference.discretize(support, resolution=chunks.duration / F)

    def expected(covered):
        out = {k: 0 for k in KEYS}
        for i in range(C):
            if not covered(chunks[i]):
                continue
            window = discrete.crop(chunks[i], mode="center")
            n = min(F, window.shape[0])
            one = metrics_truth.file_components(window[:n], data[i][:n])
            for k in KEYS:
                out[k] += one[k]
        return out

    metric = M.DiscreteDiarizationErrorRate()
    everything = metric.compute_components(reference, hypothesis)
    assert everything == expected(lambda w: True)
    uem = M.Timeline([Segment(2.5, 20.0), Segment(30.0, 36.0)])
    inside = lambda w: any(s.start <= w.start and w.end <= s.end for s in uem)      # noqa: E731
    assert sum(inside(chunks[i]) for i in range(C)) == 7
    got = metric.compute_components(reference, hypothesis, uem=uem)
    assert got == expected(inside)
    assert 0 < got["total"] < everything["total"]


def test_argument_errors_are_the_references(M):
    metric = M.DiscreteDiarizationErrorRate()
    reference, hypothesis = random_pair(0)
    with pytest.raises(NotImplementedError, match="Providing hypothesis as list instances is not supported."):
        metric(reference, hypothesis.tolist())
    with pytest.raises(NotImplementedError, match="shaped reference is supported"):
        metric(reference[None], hypothesis)
    with pytest.raises(NotImplementedError, match="shaped hypothesis is supported"):
        metric(reference, hypothesis[:, 0])
    with pytest.raises(ValueError, match="same number of frames"):
        metric(reference[:-1], hypothesis)
    with pytest.raises(ValueError, match="`uem` is not supported with numpy arrays."):
        metric(reference, hypothesis, uem=M.Timeline([]))
    from pyannote_audio_amd.core import SlidingWindow, SlidingWindowFeature
    with pytest.raises(NotImplementedError, match="shaped"):
        metric(conversation(), SlidingWindowFeature(np.zeros((2, 3, 4, 5)), SlidingWindow()))
    assert metric[:] == {k: 0 for k in KEYS}       # nothing was accumulated by the refused calls


def test_chunk_mode_argument_errors():
    from pyannote_audio_amd import metrics
    preds, target = torch.rand(4, 3, 50), torch.zeros(4, 3, 50)
    with pytest.raises(NotImplementedError, match="frame"):
        metrics.diarization_error_rate(preds, target, reduce="frame")
    with pytest.raises(ValueError, match="Batch size mismatch: 4 != 3."):
        metrics.diarization_error_rate(preds, target[:3])
    with pytest.raises(ValueError, match="Number of frames mismatch: 50 != 49."):
        metrics.diarization_error_rate(preds, target[:, :, :49])
    with pytest.raises(ValueError, match="reduce"):
        metrics.diarization_error_rate(preds, target, reduce="file")


def test_no_host_counting():
    """the counting has no CPU implementation: host arrays without a GPU are an error, never a slow answer"""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: host arrays are moved to it")
    from pyannote_audio_amd import metrics
    reference, hypothesis = random_pair(0)
    with pytest.raises(RuntimeError):
        metrics.discrete_diarization_error_rate(reference, hypothesis)
    with pytest.raises(RuntimeError):
        metrics.diarization_error_rate(torch.rand(2, 3, 50), torch.zeros(2, 3, 50))
    with pytest.raises(RuntimeError):
        metrics.DiarizationErrorRate().update(torch.rand(2, 3, 50), torch.zeros(2, 3, 50))
