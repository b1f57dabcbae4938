"""Host side of `pyannote_audio_amd.identification`: the candidate restriction of the numpy truth (tests/identify_model.py)
keeps SciPy's optimum over the whole gallery; a gallery survives its file; what cannot be scored is refused before
anything is launched; the renaming of a diarization output from hand-made matches; without a GPU the device parts raise."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import identify_model as model  # noqa: E402


def _problems(seed, count, integer):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        S = int(rng.integers(1, 10))
        G = int(rng.integers(1, 41))
        if integer:
            yield rng.integers(0, 4, size=(S, G)).astype(np.float64)     # tie-rich, sums exact
        else:
            yield rng.random((S, G))


def test_candidate_restriction_keeps_the_optimum_on_continuous_costs():
    """continuous costs have one optimum: the same pairs, and therefore the same sum"""
    for cost in _problems(0, 400, integer=False):
        col4row, columns = model.restricted_assignment(cost)
        rows, cols = linear_sum_assignment(cost)
        want = np.full(cost.shape[0], -1, dtype=np.int64)
        want[rows] = cols
        assert np.array_equal(col4row, want), cost.shape
        assert len(columns) <= min(cost.shape) * cost.shape[0]


def test_candidate_restriction_keeps_the_optimum_on_tied_costs():
    """small integers: many optima, every sum exact -- the restricted optimum costs what the full one costs, it assigns
    as many rows, and nothing twice"""
    for cost in _problems(1, 600, integer=True):
        col4row, _ = model.restricted_assignment(cost)
        rows, cols = linear_sum_assignment(cost)
        assigned = np.flatnonzero(col4row >= 0)
        assert len(assigned) == len(rows) == min(cost.shape)
        assert len(set(col4row[assigned].tolist())) == len(assigned)
        assert cost[assigned, col4row[assigned]].sum() == cost[rows, cols].sum(), cost.shape


def test_model_statistics_add_in_ascending_order():
    """the truth itself: cumsum's last element is the left-to-right sum, on a case where np.sum gives other bits"""
    rng = np.random.default_rng(2)
    X, C = rng.standard_normal((3, 16)), rng.standard_normal((300, 16))
    mean, std, status = model.cohort_stats(X, C, 257)
    s = np.sort(model.distances(X, C), axis=1)[:, :257]
    for i in range(3):
        acc = s[i, 0]
        for v in s[i, 1:]:
            acc = acc + v
        assert mean[i] == acc / 257
        acc = (s[i, 0] - mean[i]) * (s[i, 0] - mean[i])
        for v in s[i, 1:]:
            acc = acc + (v - mean[i]) * (v - mean[i])
        assert std[i] == np.sqrt(acc / 257)
    assert not status.any()
    mean, std, status = model.cohort_stats(np.zeros((1, 16)), C, 5)
    assert np.isnan(mean[0]) and np.isnan(std[0]) and status[0] == 1


def test_gallery_round_trip(tmp_path):
    from pyannote_audio_amd.identification import Gallery
    rng = np.random.default_rng(3)
    table = rng.standard_normal((5, 7)).astype(np.float32)
    gallery = Gallery([f"speaker {i}" for i in range(4)] + ["Zoë"], table)
    assert gallery.voiceprints.dtype == np.float64 and np.array_equal(gallery.voiceprints, table.astype(np.float64))
    path = tmp_path / "gallery.safetensors"
    gallery.save(path)
    again = Gallery.load(path)
    assert again.names == gallery.names and np.array_equal(again.voiceprints, gallery.voiceprints)
    assert not again.normalised and again.g_mean is None
    # with its side of the normalisation (set by hand: taking it needs the device)
    gallery.g_mean, gallery.g_std = rng.random(5), rng.random(5) + 0.5
    gallery.cohort_rows, gallery.top = 1000, 300
    gallery.save(path)
    again = Gallery.load(path)
    assert again.normalised and np.array_equal(again.g_mean, gallery.g_mean) and np.array_equal(again.g_std, gallery.g_std)
    assert (again.cohort_rows, again.top) == (1000, 300)
    other = tmp_path / "other.safetensors"
    from safetensors.numpy import save_file
    save_file({"voiceprints": gallery.voiceprints}, str(other))
    with pytest.raises(ValueError, match="not a gallery file"):
        Gallery.load(other)


def test_gallery_refuses_bad_names_and_rows():
    from pyannote_audio_amd.identification import Gallery
    good = np.eye(3, 4)
    with pytest.raises(ValueError, match="unique"):
        Gallery(["a", "b", "a"], good)
    with pytest.raises(ValueError, match="non-empty strings"):
        Gallery(["a", "", "c"], good)
    with pytest.raises(ValueError, match="non-empty strings"):
        Gallery(["a", 3, "c"], good)
    with pytest.raises(ValueError, match="3 names for 2 voiceprints"):
        Gallery(["a", "b", "c"], good[:2])
    with pytest.raises(ValueError, match="row 1 is zero or not finite"):
        Gallery(["a", "b", "c"], np.array([[1.0, 0], [0, 0], [0, 1]]))
    for poison in (np.nan, np.inf):
        with pytest.raises(ValueError, match="row 2 is zero or not finite"):
            Gallery(["a", "b", "c"], np.array([[1.0, 0], [0, 1], [poison, 1]]))
    with pytest.raises(ValueError, match="rows, dimension"):
        Gallery(["a"], np.ones(4))
    with pytest.raises(ValueError, match="empty"):
        Gallery([], np.ones((0, 4)))


def test_cohort_and_statistics_are_checked_before_any_launch():
    from pyannote_audio_amd import identification
    from pyannote_audio_amd.identification import Gallery, identify
    gallery = Gallery(["a", "b"], np.eye(2, 4))
    cohort = np.ones((6, 4))
    cohort[4] = 0.0
    with pytest.raises(ValueError, match="the cohort: row 4 is zero or not finite"):
        gallery.normalise(cohort)
    cohort[4] = np.nan
    with pytest.raises(ValueError, match="the cohort: row 4"):
        gallery.normalise(cohort)
    with pytest.raises(ValueError, match="cohort of dimension 3"):
        gallery.normalise(np.ones((6, 3)))
    with pytest.raises(ValueError, match="cohort: row 4"):
        identify([np.eye(2, 4)], gallery, cohort=cohort)
    # a cohort for a gallery that has no statistics over it
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="not normalised over this cohort"):
            identify([np.eye(2, 4)], gallery, cohort=np.ones((6, 4)) + np.eye(6, 4))
    with pytest.raises(ValueError, match="dimension 5"):
        identify([np.eye(2, 5)], gallery)
    with pytest.raises(ValueError, match="`top` must be positive"):
        identification._clipped_top(0, 10)
    _, max_top, max_k = identification.identify_geometry()
    assert max_top >= 512 and max_k >= 8
    with pytest.raises(ValueError, match="at most"):
        identification._clipped_top(max_top + 1, 10 * max_top)
    with pytest.warns(UserWarning, match="every cohort row is used"):
        assert identification._clipped_top(300, 10) == 10
    with pytest.raises(ValueError, match="at most .* per file"):
        identify([np.ones((max_k + 1, 4)) + np.eye(max_k + 1, 4)], Gallery([str(i) for i in range(max_k + 1)],
                                                                          np.ones((max_k + 1, 4))))
    # the statistics a call brings back: std == 0, a row without direction, a value that is not finite
    mean, std, status = torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32)
    identification._host_statistics(mean, std, status, "x")
    bad = std.clone()
    bad[1] = 0.0
    with pytest.raises(ValueError, match="row 1 has std == 0"):
        identification._host_statistics(mean, bad, status, "x")
    flagged = status.clone()
    flagged[2] = 1
    with pytest.raises(ValueError, match="row 2 has no direction"):
        identification._host_statistics(mean, std, flagged, "x")
    with pytest.raises(ValueError, match="not finite"):
        identification._host_statistics(mean * float("nan"), std, status, "x")


def test_rows_without_direction_stay_anonymous_without_a_launch():
    """a file of padded centroids only: nothing to score, so nothing is launched and no GPU is needed"""
    from pyannote_audio_amd.identification import Gallery, identify
    gallery = Gallery(["a", "b"], np.eye(2, 4))
    E = np.zeros((3, 4))
    E[1, 2] = np.nan
    (index, value), (index2, value2) = identify([E, np.zeros((0, 4))], gallery)
    assert index.tolist() == [-1, -1, -1] and np.isnan(value).all()
    assert index2.shape == (0,) and value2.shape == (0,)


def test_valid_rows_follow_the_norm_the_kernels_take():
    """finite is not enough: a row whose squares overflow or underflow has a norm of inf or 0 and NaN distances"""
    from pyannote_audio_amd.identification import Gallery, valid_rows
    E = np.ones((7, 3))
    E[1] = 0.0
    E[2, 1] = np.nan
    E[3, 0] = np.inf
    E[4] = 1e200
    E[5] = 1e-200
    E[6] = [1e-150, 0.0, -1e150]
    assert valid_rows(E).tolist() == [True, False, False, False, False, False, True]
    assert model.valid_rows(E).tolist() == valid_rows(E).tolist()
    assert valid_rows(np.zeros((0, 3))).shape == (0,)
    with pytest.raises(ValueError, match="row 0 is zero or not finite"):
        Gallery(["a"], E[4:5])


def _output(labels, uri="file"):
    from pyannote_audio_amd import Annotation, DiarizeOutput, Segment
    regular, exclusive = Annotation(uri=uri), Annotation(uri=uri)
    for i, label in enumerate(labels):
        regular[Segment(i, i + 1.5), "_"] = label
        exclusive[Segment(i, i + 1.0), "_"] = label
    return DiarizeOutput(regular, exclusive, np.arange(len(labels) * 2, dtype=np.float32).reshape(len(labels), 2))


def _turns(annotation):
    return [(s.start, s.end, label) for s, _, label in annotation.itertracks(yield_label=True)]


def test_rename_speakers():
    from pyannote_audio_amd.identification import IdentifiedOutput, rename_speakers
    names = ["alice", "bob", "carol"]
    output = _output(["SPEAKER_00", "SPEAKER_01", "SPEAKER_02", "SPEAKER_03"])
    # 00 accepted as carol, 01 rejected (a value but no index), 02 accepted as alice, 03 never scored
    named = rename_speakers(output, names, np.array([2, -1, 0, -1]), np.array([0.25, 0.9, 0.5, np.nan]))
    assert isinstance(named, IdentifiedOutput)
    assert _turns(named.speaker_diarization) == [(0, 1.5, "carol"), (1, 2.5, "SPEAKER_01"), (2, 3.5, "alice"),
                                                 (3, 4.5, "SPEAKER_03")]
    assert _turns(named.exclusive_speaker_diarization) == [(0, 1.0, "carol"), (1, 2.0, "SPEAKER_01"), (2, 3.0, "alice"),
                                                           (3, 4.0, "SPEAKER_03")]
    assert named.matches == {"SPEAKER_00": ("carol", 0.25), "SPEAKER_01": (None, 0.9), "SPEAKER_02": ("alice", 0.5)}
    assert named.speaker_embeddings is output.speaker_embeddings and named.speaker_diarization.uri == "file"
    # the input is left as it was
    assert _turns(output.speaker_diarization)[0] == (0, 1.5, "SPEAKER_00")
    assert set(named.serialize()) == {"diarization", "exclusive_diarization"}
    # a gallery name that collides with a label that stays
    with pytest.raises(ValueError, match="SPEAKER_01"):
        rename_speakers(output, ["SPEAKER_01", "bob"], np.array([0, -1, -1, -1]), np.array([0.1, np.nan, np.nan, np.nan]))
    # ... but not with a label that goes away
    swapped = rename_speakers(output, ["SPEAKER_01", "SPEAKER_00"], np.array([0, 1, -1, -1]),
                              np.array([0.1, 0.2, np.nan, np.nan]))
    assert [label for _, _, label in _turns(swapped.speaker_diarization)][:2] == ["SPEAKER_01", "SPEAKER_00"]
    with pytest.raises(ValueError, match="3 identification rows for 4 speakers"):
        rename_speakers(output, names, np.array([0, 1, 2]), np.zeros(3))


def test_pipeline_interface():
    from pyannote_audio_amd import Pipeline, annotation_metrics
    from pyannote_audio_amd.identification import Gallery, SpeakerIdentification
    from pyannote_audio_amd.pipeline import Uniform

    class Diarizer(Pipeline):
        legacy = False

        def apply(self, file, **kwargs):
            return _output(["SPEAKER_00"])

    gallery = Gallery(["a", "b"], np.eye(2, 2))
    pipeline = SpeakerIdentification(Diarizer(), gallery)
    threshold = pipeline.parameters()["threshold"]
    assert isinstance(threshold, Uniform) and (threshold.low, threshold.high) == (0.0, 2.0)
    assert isinstance(pipeline.get_metric(), annotation_metrics.IdentificationErrorRate)
    assert pipeline.get_direction() == "minimize"
    pipeline.instantiate({"threshold": 0.5})
    assert pipeline.threshold == 0.5
    with pytest.raises(TypeError):
        SpeakerIdentification(Diarizer(), np.eye(2))
    legacy = Diarizer()
    legacy.legacy = True
    with pytest.raises(ValueError, match="legacy"):
        SpeakerIdentification(legacy, gallery)
    with pytest.raises(ValueError, match="the cohort: row 0"):
        SpeakerIdentification(Diarizer(), gallery, cohort=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="joint_clustering"):
        list(pipeline.apply_batch([{"uri": "x"}], joint_clustering=True))


def test_device_parts_raise_without_a_gpu():
    if torch.cuda.is_available():
        return
    from pyannote_audio_amd.identification import Gallery, SpeakerIdentification, identify
    gallery = Gallery(["a", "b"], np.eye(2, 4))
    with pytest.raises(RuntimeError, match="needs an AMD GPU"):
        identify([np.eye(2, 4)], gallery)
    with pytest.raises(RuntimeError, match="needs an AMD GPU"):
        gallery.normalise(np.ones((3, 4)), top=2)
    with pytest.raises(RuntimeError, match="needs an AMD GPU"):
        Gallery.enroll(None, {"a": [{"audio": "a.wav"}]})

    class Diarizer:
        legacy = False

    with pytest.raises(RuntimeError, match="needs an AMD GPU"):
        SpeakerIdentification(Diarizer(), gallery).instantiate({"threshold": 1.0}).apply({"uri": "x"})
