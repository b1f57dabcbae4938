"""`tuning.DetectionTuner` without a GPU: the numpy forms of the sweep and of the counts give, candidate by candidate
and with `==`, the loss of the literal loop; shared work is reported; refusals raise; VoiceActivityDetection keeps its
aggregated scores in training mode."""
import numpy as np
import pytest

import detection_tuning_cases as dt

SPEAKERS = ["s1", "s2", "s3"]


@pytest.fixture(scope="module")
def vad(tmp_path_factory):
    import pyannote_audio_amd as pa
    ckpt = dt.checkpoint(tmp_path_factory.mktemp("vad") / "seg.bin", SPEAKERS)
    return pa.VoiceActivityDetection(segmentation=ckpt)


@pytest.fixture(scope="module")
def vad_files(vad):
    return dt.corpus(vad.CACHED_SEGMENTATION, 1, ["alice", "bob"], seed=3)


def multilabel(tmp_path, **kwargs):
    import pyannote_audio_amd as pa
    return pa.MultiLabelSegmentation(segmentation=dt.checkpoint(tmp_path / "ml.bin", dt.CLASSES), **kwargs)


@pytest.mark.parametrize("fscore", [False, True])
def test_vad_sweep_equals_the_literal_loop(tmp_path, vad_files, fscore):
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.tuning import DetectionTuner
    pipeline = pa.VoiceActivityDetection(segmentation=dt.checkpoint(tmp_path / "seg.bin", SPEAKERS), fscore=fscore)
    tuner = DetectionTuner(pipeline, keep_hypotheses=True).prepare(vad_files)
    assert pipeline.training is False
    result = tuner.sweep([0.4, 0.5, 0.6], [0.35, 0.5, 0.6], [0.0, 0.15], [0.0, 0.2])
    candidates = [entry["params"] for entry in result["entries"]]
    # 0.4 / 0.5, 0.4 / 0.6 and 0.5 / 0.6 have the offset above the onset
    assert len(candidates) == 6 * 4 and result["skipped_offset_above_onset"] == 3 * 4
    assert candidates[0] == {"onset": 0.4, "offset": 0.35, "min_duration_on": 0.0, "min_duration_off": 0.0}
    assert candidates[1]["min_duration_off"] == 0.2 and candidates[4]["offset"] == 0.35 and candidates[4]["onset"] == 0.5
    losses, hypotheses = dt.literal_loop(pipeline, vad_files, candidates, pipeline.get_metric)
    assert [entry["loss"] for entry in result["entries"]] == losses
    assert len(set(losses)) > 6
    best = max(losses) if fscore else min(losses)
    assert result["best"] is result["entries"][losses.index(best)]
    for got, want in zip(tuner.hypotheses, hypotheses):
        assert [dt.rows(a) for a in got] == [dt.rows(a) for a in want]
    assert result["shared"] == {"candidates": 24, "detectors": 24, "lanes": 6, "jobs": 24, "counted": 24,
                                "collisions": 0}


def test_vad_shared_work_and_float32_thresholds(vad, vad_files):
    from pyannote_audio_amd.tuning import DetectionTuner
    tuner = DetectionTuner(vad).prepare(vad_files)
    near = float(np.nextafter(np.float32(0.5), np.float32(1.0)))          # the next float32: another lane
    same = 0.5 + 1e-12                                                    # rounds to the same float32: the same lane
    candidates = [{"onset": a, "offset": 0.0, "min_duration_on": d, "min_duration_off": 0.1}
                  for a in (0.5, same, near) for d in (0.0, 0.2, 0.0)]
    result = tuner.evaluate(candidates)
    assert result["shared"]["lanes"] == 2 and result["shared"]["jobs"] == 4 and result["shared"]["counted"] == 4
    losses, _ = dt.literal_loop(vad, vad_files, candidates, vad.get_metric)
    assert [entry["loss"] for entry in result["entries"]] == losses
    assert tuner.hypotheses == []


def test_vad_refusals(tmp_path, vad, vad_files):
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.tuning import DetectionTuner
    tuner = DetectionTuner(vad)
    with pytest.raises(RuntimeError, match="prepare"):
        tuner.evaluate([{"onset": 0.5, "offset": 0.5, "min_duration_on": 0.0, "min_duration_off": 0.0}])
    without = {k: v for k, v in vad_files[0].items() if k != "annotated"}
    with pytest.raises(ValueError, match="annotated"):
        tuner.prepare([without])
    tuner.prepare(vad_files)
    with pytest.raises(ValueError, match="offset"):
        tuner.evaluate([{"onset": 0.4, "offset": 0.6, "min_duration_on": 0.0, "min_duration_off": 0.0}])
    with pytest.raises(ValueError, match="NaN"):
        tuner.evaluate([{"onset": 0.4, "offset": 0.3, "min_duration_on": float("nan"), "min_duration_off": 0.0}])
    with pytest.raises(TypeError):
        DetectionTuner(object())
    powerset = pa.VoiceActivityDetection(segmentation=dt.checkpoint(tmp_path / "ps.bin", None, powerset=True))
    fixed = DetectionTuner(powerset).prepare(vad_files)
    with pytest.raises(ValueError, match="fixed"):
        fixed.sweep([0.5], None, [0.0], [0.0])
    with pytest.raises(ValueError, match="fixed"):
        fixed.evaluate([{"onset": 0.5, "offset": 0.5, "min_duration_on": 0.0, "min_duration_off": 0.0}])
    result = fixed.sweep(min_duration_ons=[0.0, 0.1], min_duration_offs=[0.0, 0.3])
    candidates = [entry["params"] for entry in result["entries"]]
    assert candidates[1] == {"min_duration_on": 0.0, "min_duration_off": 0.3}
    assert result["shared"]["lanes"] == 1 and result["shared"]["jobs"] == 4
    losses, _ = dt.literal_loop(powerset, vad_files, candidates, powerset.get_metric)
    assert [entry["loss"] for entry in result["entries"]] == losses


def test_vad_keeps_and_reuses_its_scores_in_training_mode(vad, vad_files, monkeypatch):
    calls = []
    scores = vad_files[0][vad.CACHED_SEGMENTATION]

    def inference(file, hook=None):
        calls.append(file["uri"])
        return scores

    monkeypatch.setattr(vad._segmentation, "__call__", inference, raising=False)
    monkeypatch.setattr(type(vad._segmentation), "__call__", lambda self, file, hook=None: inference(file, hook))
    vad.instantiate({"onset": 0.5, "offset": 0.4, "min_duration_on": 0.0, "min_duration_off": 0.0})
    file = {k: v for k, v in vad_files[0].items() if k != vad.CACHED_SEGMENTATION}
    assert vad.CACHED_SEGMENTATION == "cache/segmentation/inference" and vad.training is False
    plain = vad.apply(file)
    assert calls == ["file0"] and vad.CACHED_SEGMENTATION not in file        # unchanged without `training`
    vad.training = True
    try:
        first = vad.apply(file)
        assert calls == ["file0"] * 2 and file[vad.CACHED_SEGMENTATION] is scores
        second = vad.apply(file)
        assert calls == ["file0"] * 2
    finally:
        vad.training = False
    assert dt.rows(first) == dt.rows(plain) == dt.rows(second) and len(dt.rows(plain)) > 3
    vad.apply(file)
    assert calls == ["file0"] * 3                                            # the cache is not read without `training`


@pytest.mark.parametrize("shared", [False, True])
def test_multilabel_equals_the_oracle_loop(tmp_path, shared):
    from pyannote_audio_amd import annotation_metrics as am
    from pyannote_audio_amd.tuning import DetectionTuner
    pipeline = multilabel(tmp_path, share_min_duration=shared)
    files = dt.corpus(pipeline.CACHED_SEGMENTATION, 3, dt.CLASSES + ["other"], seed=8)
    tuner = DetectionTuner(pipeline, keep_hypotheses=True).prepare(files)
    candidates = dt.multilabel_candidates(shared)
    result = tuner.evaluate(candidates)
    metric = lambda: am.IdentificationErrorRate()          # noqa: E731
    losses, hypotheses = dt.oracle_loop(pipeline, files, candidates, metric)
    assert [entry["loss"] for entry in result["entries"]] == losses
    assert result["best"] is result["entries"][losses.index(min(losses))] and len(set(losses)) > 4
    for got, want in zip(tuner.hypotheses, hypotheses):
        assert [dt.rows(a) for a in got] == [dt.rows(a) for a in want]
    assert result["shared"]["lanes"] < result["shared"]["detectors"] == 3 * len(candidates)


@pytest.mark.parametrize("shared", [False, True])
def test_multilabel_collision_and_other_metrics(tmp_path, shared):
    """two classes on throughout with min_duration_off = 0 hold the same (segment, track): the later class's row
    replaces the earlier one's in the pipeline's Annotation, and in the tuner's loss"""
    from pyannote_audio_amd import annotation_metrics as am
    from pyannote_audio_amd.tuning import DetectionTuner
    pipeline = multilabel(tmp_path, share_min_duration=shared, fscore=True)
    files = dt.corpus(pipeline.CACHED_SEGMENTATION, 3, dt.CLASSES, seed=9, always_on=(0, 1))
    candidates = dt.multilabel_candidates(shared)
    ier = lambda: am.IdentificationErrorRate()             # noqa: E731
    result = DetectionTuner(pipeline, metric=ier).prepare(files).evaluate(candidates)
    losses, hypotheses = dt.oracle_loop(pipeline, files, candidates, ier)
    assert [entry["loss"] for entry in result["entries"]] == losses
    collided = [len(h[0].labels()) < 3 and any(r[3] == "music" for r in dt.rows(h[0])) for h in hypotheses]
    assert result["shared"]["collisions"] >= sum(collided) * len(files) > 0
    # a metric without `add_counts`: Annotations are built and the metric is called as usual; the default with fscore
    tuner = DetectionTuner(pipeline).prepare(files)
    result = tuner.evaluate(candidates)
    macro = lambda: am.MacroAverageFMeasure(classes=dt.CLASSES)           # noqa: E731
    losses, _ = dt.oracle_loop(pipeline, files, candidates, macro)
    assert [entry["loss"] for entry in result["entries"]] == losses
    assert result["best"] is result["entries"][losses.index(max(losses))]


def test_multilabel_sweep_grid_and_write_config(tmp_path):
    import yaml
    from pyannote_audio_amd.tuning import DetectionTuner, write_config
    for shared in (False, True):
        pipeline = multilabel(tmp_path, share_min_duration=shared)
        files = dt.corpus(pipeline.CACHED_SEGMENTATION, 3, dt.CLASSES, seed=4, durations=(12.0,))
        result = DetectionTuner(pipeline).prepare(files).sweep([0.4, 0.6], [0.5], [0.0, 0.1], [0.2])
        assert "skipped_offset_above_onset" in result and result["skipped_offset_above_onset"] == 0
        params = [entry["params"] for entry in result["entries"]]
        assert len(params) == 4
        if shared:
            assert params[1] == {"thresholds": {c: {"onset": 0.4, "offset": 0.5} for c in dt.CLASSES},
                                 "min_duration_on": 0.1, "min_duration_off": 0.2}
        else:
            assert params[2]["thresholds"]["music"] == {"onset": 0.6, "offset": 0.5, "min_duration_on": 0.0,
                                                        "min_duration_off": 0.2}
    config = tmp_path / "config.yaml"
    with open(config, "w") as fp:
        yaml.safe_dump({"pipeline": {"name": "pyannote.audio.pipelines.MultiLabelSegmentation"}, "params": {}}, fp)
    out = write_config(config, result, "dev")
    with open(out) as fp:
        written = yaml.safe_load(fp)
    assert written["params"] == result["best"]["params"]
    assert written["optimization"]["status"]["best_loss"] == result["best"]["loss"]
    pipeline.instantiate(written["params"])
