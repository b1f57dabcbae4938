"""`tuning.DetectionTuner` on the GPU: the counts of all candidates from one `pa_annot_corpus_counts` call equal
`pa_annot_counts` entry by entry, and the sweeps of VoiceActivityDetection and MultiLabelSegmentation give, candidate
by candidate and with `==`, the loss, the best entry and the hypothesis rows of the literal loop --
`pipeline.instantiate(params)`, `pipeline(file)`, `metric(reference, hypothesis, uem=annotated)` with a metric on the
same device."""
import numpy as np
import pytest
import torch

import detection_tuning_cases as dt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """three named classes with the calibrated read-out of oracle.synthetic: scores that cross their thresholds"""
    from conftest import PYANNET_HPARAMS
    from oracle.synthetic import calibrated_multilabel_pyannet
    from pyannote_audio_amd.model import Problem, PyanNet, Resolution, Specifications, save_checkpoint
    path = tmp_path_factory.mktemp("detection") / "seg.bin"
    spec = Specifications(problem=Problem.MULTI_LABEL_CLASSIFICATION, resolution=Resolution.FRAME, duration=10.0,
                          min_duration=None, warm_up=(0.0, 0.0), classes=list(dt.CLASSES), permutation_invariant=False)
    save_checkpoint(str(path), calibrated_multilabel_pyannet(calib_seconds=40.0).state_dict(), PYANNET_HPARAMS,
                    PyanNet.ARCHITECTURE, spec)
    return str(path)


def losses_of(result):
    return [entry["loss"] for entry in result["entries"]]


def same_hypotheses(got, want):
    for a, b in zip(got, want):
        assert [dt.rows(x) for x in a] == [dt.rows(x) for x in b]


@pytest.mark.parametrize("fscore", [False, True])
def test_vad_sweep_equals_the_literal_loop(checkpoint, gpu_device, fscore):
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.tuning import DetectionTuner
    pipeline = pa.VoiceActivityDetection(segmentation=checkpoint, fscore=fscore).to(gpu_device)
    files = dt.audio_corpus(["alice", "bob"], seed=31)
    tuner = DetectionTuner(pipeline, keep_hypotheses=True).prepare(files)
    assert all(item.scores.is_cuda for item in tuner.prepared) and pipeline.training is False
    assert all(pipeline.CACHED_SEGMENTATION in file for file in files)
    scores = np.concatenate([file[pipeline.CACHED_SEGMENTATION].data.ravel() for file in files])
    onsets = [float(q) for q in np.quantile(scores, [0.35, 0.5, 0.7])]
    offsets = [float(q) for q in np.quantile(scores, [0.25, 0.5, 0.6])]
    result = tuner.sweep(onsets, offsets, [0.0, 0.2], [0.0, 0.3])
    candidates = [entry["params"] for entry in result["entries"]]
    assert len(candidates) == 6 * 4 and result["skipped_offset_above_onset"] == 3 * 4
    metric = pipeline.get_metric
    assert metric().device == gpu_device
    losses, hypotheses = dt.literal_loop(pipeline, files, candidates, metric)
    assert losses_of(result) == losses and len(set(losses)) > 6
    best = max(losses) if fscore else min(losses)
    assert result["best"] is result["entries"][losses.index(best)]
    same_hypotheses(tuner.hypotheses, hypotheses)
    assert sum(len(dt.rows(h)) for h in hypotheses[0]) > 10
    assert result["shared"]["lanes"] == 6 and result["shared"]["jobs"] == 24
    # the best candidate through the pipeline as a user runs it: fresh files, no training mode, the network runs
    pipeline.instantiate(result["best"]["params"])
    fresh = metric()
    for file in dt.audio_corpus(["alice", "bob"], seed=31):
        fresh(file["annotation"], pipeline(file), uem=file["annotated"])
    assert abs(fresh) == result["best"]["loss"]


@pytest.mark.parametrize("shared", [False, True])
def test_multilabel_equals_the_literal_loop(checkpoint, gpu_device, shared):
    import pyannote_audio_amd as pa
    from pyannote_audio_amd import annotation_metrics as am
    from pyannote_audio_amd.tuning import DetectionTuner
    pipeline = pa.MultiLabelSegmentation(segmentation=checkpoint, share_min_duration=shared).to(gpu_device)
    files = dt.audio_corpus(dt.CLASSES + ["other"], seed=31)
    tuner = DetectionTuner(pipeline, keep_hypotheses=True).prepare(files)
    assert all(item.scores.is_cuda for item in tuner.prepared)
    # (sigmoid scores are above 0: the last candidate has speech and music on throughout, min_duration_off = 0)
    candidates = dt.multilabel_candidates(shared, always_on_at=1e-30)
    result = tuner.evaluate(candidates)
    metric = lambda: am.IdentificationErrorRate(device=gpu_device)        # noqa: E731
    losses, hypotheses = dt.literal_loop(pipeline, files, candidates, metric)
    assert losses_of(result) == losses and len(set(losses)) > 4
    assert result["best"] is result["entries"][losses.index(min(losses))]
    same_hypotheses(tuner.hypotheses, hypotheses)
    collided = hypotheses[-1]
    assert all(a.labels() == ["music", "noise"] or a.labels() == ["music"] for a in collided)
    assert result["shared"]["collisions"] >= len(files)
    # the same candidates counted by the default metric of the tuner
    assert losses_of(DetectionTuner(pipeline).prepare(files).evaluate(candidates)) == losses


def test_batched_counts_equal_the_single_call(checkpoint, gpu_device):
    import pyannote_audio_amd as pa
    from pyannote_audio_amd import annotation_metrics as am
    from pyannote_audio_amd import ffi
    from pyannote_audio_amd import frames as frame_ops
    from pyannote_audio_amd.tuning import DetectionTuner, candidate_counts
    pipeline = pa.MultiLabelSegmentation(segmentation=checkpoint).to(gpu_device)
    files = dt.audio_corpus(dt.CLASSES + ["other"], seed=32, durations=(31.0,))
    tuner = DetectionTuner(pipeline).prepare(files)
    item = tuner.prepared[0]
    lane_class = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
    onset = np.array([0.5, 0.45, 0.55, 0.6, 0.4, 5.0], dtype=np.float32)          # lane 5: never on
    job_lane = np.array([0, 1, 2, 3, 4, 5, 0], dtype=np.int32)
    d_off = np.array([0.0, 0.1, 0.0, 0.3, 0.0, 0.0, 0.5])
    rows, _, offsets = frame_ops.binarize_regions_sweep(item.scores, item.frames, lane_class, onset, onset, job_lane,
                                                        0.05, d_off, to_host=False)
    counts = np.diff(offsets)
    assert counts[5] == 0 and counts[:5].min() > 0
    entry_jobs = np.array([[0, 1, 2], [3, 4, 5], [6, 1, 5], [3, 1, 2], [0, 4, 5]])
    host_rows = rows.cpu().numpy()
    everything = list(range(len(entry_jobs)))
    order = sorted(range(3), key=lambda k: dt.CLASSES[k])
    for collar, skip_overlap in ((0.0, False), (0.25, True)):
        singles = []
        for picked in entry_jobs:
            runs = [picked[k] for k in order if counts[picked[k]]]
            seg = np.concatenate([host_rows[offsets[j]:offsets[j + 1]] for j in runs])
            lab = np.repeat(np.arange(len(runs), dtype=np.int32), counts[runs])
            singles.append(am.device_counts(item.ref_seg, item.ref_lab, len(item.ref_labels), seg, lab, len(runs),
                                            item.uem_seg, collar, skip_overlap, gpu_device).cpu().numpy())
        # the default budget takes the five entries in one call; at 1 byte every entry is a call of its own
        for budget, calls in ((DetectionTuner.workspace_bytes, 1), (1, len(entry_jobs))):
            ffi.prof_enable(True)
            try:
                ffi.prof_report()
                batched = candidate_counts(item, rows, offsets, counts, entry_jobs, everything, tuner.classes, collar,
                                           skip_overlap, gpu_device, budget)
                torch.cuda.synchronize()
                report = ffi.prof_report()
            finally:
                ffi.prof_enable(False)
            assert report["k_annot_corpus_counts"]["launches"] == calls
            for e, picked in enumerate(entry_jobs):
                labels, values = batched[e]
                assert labels == [dt.CLASSES[k] for k in order if counts[picked[k]]]
                assert values.shape == singles[e].shape and values.sum() > 0
                assert np.array_equal(values.view(np.int64), singles[e].view(np.int64)), (collar, budget, e)
