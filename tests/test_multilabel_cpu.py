"""MultiLabelSegmentation without a GPU: the tests' frame-by-frame helper (tests/multilabel_oracle.py) against the
reference's recorded output (tests/golden/multilabel_v1.npz) and, where the reference lies beside the repository,
against its live code; and the pipeline class's public surface (constructor, parameter tree, loading)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import multilabel_oracle as mo  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multilabel_v1.npz")
CLASSES = ["speech", "music", "noise"]


def golden_cases():
    g = np.load(GOLDEN)
    return g, [str(c) for c in g["cases"]]


def helper_on_case(g, name):
    start, duration, step = g[f"{name}/frames"]
    return mo.all_regions(g[f"{name}/scores"], start, duration, step, g[f"{name}/onset"], g[f"{name}/offset"],
                          g[f"{name}/min_duration_on"], g[f"{name}/min_duration_off"])


def golden_rows(g, name):
    return [(float(a), float(b), str(t), str(l)) for (a, b), t, l in
            zip(g[f"{name}/apply_times"], g[f"{name}/apply_tracks"], g[f"{name}/apply_labels"])]


def test_golden_file_holds_the_cases_the_kernel_must_survive():
    g, names = golden_cases()
    assert [str(c) for c in g["classes"]] == CLASSES
    above = g["offset_above_onset/offset"] > g["offset_above_onset/onset"]
    assert above.all()
    assert np.isnan(g["nan/scores"][0]).any() and np.isnan(g["all_nan/scores"]).all()
    T = len(g["alternating/scores"])
    assert [len(g[f"alternating/binarize{k}_times"]) for k in range(3)] == [T // 2] * 3      # the T / 2 bound
    assert len(g["opens_on_last_frame/binarize0_times"]) == 0
    assert bool(g["shared_min_duration/shared"]) and len(set(g["per_class_min_duration/min_duration_on"])) == 3
    # float32 comparisons: a score equal to float32(0.4) is NOT above the threshold 0.4
    assert np.float32(0.4) in g["threshold_neighbours/scores"][:, 0]
    assert {"offset_below_onset", "offset_equals_onset", "all_on", "all_off", "two_frames"} <= set(names)


@pytest.mark.parametrize("name", golden_cases()[1])
def test_helper_reproduces_the_reference_recording(name):
    g, _ = golden_cases()
    per_class = helper_on_case(g, name)
    for k, (regions, positions) in enumerate(per_class):
        want = g[f"{name}/binarize{k}_times"]
        got = np.array(regions, dtype=np.float64).reshape(-1, 2)
        assert got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))
        assert [mo.track_name(p) for p in positions] == [str(t) for t in g[f"{name}/binarize{k}_tracks"]]
    assert mo.triples(per_class, CLASSES) == golden_rows(g, name)


def test_float32_threshold_rule_is_what_the_recording_pins():
    """evaluating the comparisons in float64 changes the regions of the threshold-neighbour case"""
    g, _ = golden_cases()
    name = "threshold_neighbours"
    start, duration, step = g[f"{name}/frames"]
    y = g[f"{name}/scores"][:, 0].astype(np.float64)
    on, off = float(g[f"{name}/onset"][0]), float(g[f"{name}/offset"][0])
    state, flips = y[0] > on, 0
    for v in y[1:]:
        if state and v < off:
            state, flips = False, flips + 1
        elif not state and v > on:
            state = True
    assert flips != len(g[f"{name}/binarize0_times"])


def test_helper_matches_the_live_reference_on_fresh_cases():
    import refharness
    if not refharness.available():
        pytest.skip("the reference is not beside the repository")
    os.environ.setdefault("PYANNOTE_SKIP_DEPENDENCY_CHECK", "1")
    rng = np.random.default_rng(77)
    with refharness.reference_modules(third_party=True) as ref:
        ref.load_pipelines()
        signal = ref.load("pyannote.audio.utils.signal")
        core = sys.modules["pyannote.core"]
        for trial in range(12):
            T = int(rng.integers(2, 900))
            frames = (float(rng.uniform(0, 2)), 0.0619375, 0.016875)
            scores = mo.smooth_scores(rng, T, 2, width=int(rng.integers(1, 20)),
                                      nan_fraction=[0.0, 0.03][trial % 2])
            onset, offset = rng.uniform(0.2, 0.8, 2), rng.uniform(0.2, 0.8, 2)
            d_on = rng.choice([0.0, 0.05, 0.2], 2)
            d_off = rng.choice([0.0, 0.05, 0.2], 2)
            per_class = mo.all_regions(scores, *frames, onset, offset, d_on, d_off)
            window = core.SlidingWindow(start=frames[0], duration=frames[1], step=frames[2])
            for k in range(2):
                active = signal.Binarize(onset=onset[k], offset=offset[k], min_duration_on=d_on[k],
                                         min_duration_off=d_off[k])(
                    core.SlidingWindowFeature(scores[:, k:k + 1], window))
                want = [(s.start, s.end, t) for s, t in active.itertracks()]
                got = [(a, b, mo.track_name(p)) for (a, b), p in zip(*per_class[k])]
                assert got == want, (trial, k)


# ------------------------------------------------------------------------------------------------ the class
def multilabel_checkpoint(path, classes=CLASSES, powerset=False):
    import torch
    from conftest import PYANNET_HPARAMS
    from oracle import seeded_pyannet
    from pyannote_audio_amd.model import (Problem, PyanNet, Resolution, Specifications, save_checkpoint,
                                          segmentation_specifications)
    state = seeded_pyannet(seed=5, num_layers=4).state_dict()
    if powerset:
        spec = segmentation_specifications(10.0, powerset=True)
    else:
        g = torch.Generator().manual_seed(1)
        state["classifier.weight"] = 0.1 * torch.randn(len(classes), 128, generator=g)
        state["classifier.bias"] = torch.zeros(len(classes))
        spec = Specifications(problem=Problem.MULTI_LABEL_CLASSIFICATION, resolution=Resolution.FRAME,
                              duration=10.0, min_duration=None, warm_up=(0.0, 0.0), classes=list(classes),
                              permutation_invariant=False)
    save_checkpoint(str(path), state, PYANNET_HPARAMS, PyanNet.ARCHITECTURE, spec)
    return str(path)


def test_constructor_needs_a_multilabel_model(tmp_path):
    import pyannote_audio_amd as pa
    with pytest.raises(ValueError, match="segmentation"):
        pa.MultiLabelSegmentation()
    bad = multilabel_checkpoint(tmp_path / "powerset.bin", powerset=True)
    with pytest.raises(ValueError, match="powerset"):
        pa.MultiLabelSegmentation(segmentation=bad)


@pytest.mark.parametrize("shared", [False, True])
def test_parameter_tree_and_initialize(tmp_path, shared):
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.pipeline import ParamDict, Uniform
    ckpt = multilabel_checkpoint(tmp_path / "ml.bin")
    pipeline = pa.MultiLabelSegmentation(segmentation=ckpt, share_min_duration=shared)
    assert pipeline.classes() == CLASSES
    tree = pipeline.parameters()
    assert isinstance(tree["thresholds"], ParamDict) and list(tree["thresholds"].params) == CLASSES
    leaf = tree["thresholds"].params["music"]
    assert isinstance(leaf, ParamDict)
    if shared:
        assert sorted(leaf.params) == ["offset", "onset"]
        assert isinstance(tree["min_duration_on"], Uniform) and tree["min_duration_off"].high == 2.0
    else:
        assert sorted(leaf.params) == ["min_duration_off", "min_duration_on", "offset", "onset"]
        assert "min_duration_on" not in tree and leaf.params["min_duration_on"].high == 2.0
    assert (leaf.params["onset"].low, leaf.params["onset"].high) == (0.0, 1.0)
    assert not pipeline.instantiated
    thresholds = {c: {"onset": 0.4 + 0.1 * k, "offset": 0.6 - 0.1 * k} for k, c in enumerate(CLASSES)}
    thresholds["noise"]["offset"] = 0.0               # Binarize: `offset or onset`
    if shared:
        params = {"thresholds": thresholds, "min_duration_on": 0.1, "min_duration_off": 0.2}
    else:
        for k, c in enumerate(CLASSES):
            thresholds[c].update(min_duration_on=0.1 * k, min_duration_off=0.2 * k)
        params = {"thresholds": thresholds}
    assert pipeline.instantiate(params) is pipeline and pipeline.instantiated
    assert np.allclose(pipeline._onset, [0.4, 0.5, 0.6]) and np.allclose(pipeline._offset, [0.6, 0.5, 0.6])
    want_on = [0.1] * 3 if shared else [0.0, 0.1, 0.2]
    want_off = [0.2] * 3 if shared else [0.0, 0.2, 0.4]
    assert np.allclose(pipeline._min_duration_on, want_on) and np.allclose(pipeline._min_duration_off, want_off)
    assert pipeline.get_direction() == "minimize"
    assert pa.MultiLabelSegmentation(segmentation=ckpt, fscore=True).get_direction() == "maximize"
    with pytest.raises(NotImplementedError, match="pyannote.metrics"):
        pipeline.get_metric()


def test_from_pretrained_resolves_the_reference_class_path(tmp_path):
    import yaml
    import pyannote_audio_amd as pa
    os.makedirs(tmp_path / "segmentation")
    multilabel_checkpoint(tmp_path / "segmentation" / "pytorch_model.bin")
    thresholds = {c: {"onset": 0.6, "offset": 0.4, "min_duration_on": 0.0, "min_duration_off": 0.1} for c in CLASSES}
    config = {"version": "3.1.0",
              "pipeline": {"name": "pyannote.audio.pipelines.MultiLabelSegmentation",
                           "params": {"segmentation": "$model/segmentation"}},
              "params": {"thresholds": thresholds}}
    with open(tmp_path / "config.yaml", "w") as fp:
        yaml.safe_dump(config, fp)
    pipeline = pa.Pipeline.from_pretrained(str(tmp_path))
    assert type(pipeline) is pa.MultiLabelSegmentation and pipeline.instantiated
    assert pipeline.classes() == CLASSES and not pipeline.share_min_duration
    assert np.array_equal(pipeline._min_duration_off, [0.1] * 3)
    assert pipeline.CACHED_SEGMENTATION == "cache/segmentation"
    from pyannote_audio_amd.pipeline import get_class_by_name
    assert get_class_by_name("pyannote.audio.pipelines.multilabel.MultiLabelSegmentation") is pa.MultiLabelSegmentation


def test_annotation_update_overwrites_equal_segment_and_track():
    from pyannote_audio_amd.core import Annotation, Segment
    a, b = Annotation(uri="u"), Annotation()
    a[Segment(0, 1), "A"] = "speech"
    a[Segment(2, 3), "A"] = "speech"
    b[Segment(0, 1), "A"] = "music"
    b[Segment(0, 1), "B"] = "music"
    assert a.update(b) is a
    rows = [(s.start, s.end, t, l) for s, t, l in a.itertracks(yield_label=True)]
    assert rows == [(0, 1, "A", "music"), (0, 1, "B", "music"), (2, 3, "A", "speech")]
