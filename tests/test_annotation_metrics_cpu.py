"""Host path of `pyannote_audio_amd.annotation_metrics` (the numpy sweep and everything above the counts) against
tests/annotation_metrics_truth.py and against cases worked out by hand.  No GPU."""
import os
import warnings
from fractions import Fraction

import numpy as np
import pytest

import pyannote_audio_amd as pa
from pyannote_audio_amd import annotation_metrics as am
from pyannote_audio_amd.core import Segment

import annotation_metrics_truth as truth


def _annotation(rows, uri=None):
    a = pa.Annotation(uri=uri)
    for n, (start, end, label) in enumerate(rows):
        a[Segment(start, end), n] = label
    return a


def _host_logic_example():
    ref = _annotation([(0, 10, "alice"), (10, 20, "bob")], uri="r")
    hyp = _annotation([(0, 9, 0), (9, 12, 1), (12, 20, 2), (30, 31, 3)], uri="h")
    return ref, hyp


def _assert_counts_equal_truth(counts, want):
    got = list(counts["cooc"].ravel()) + list(counts["ref_dur"]) + list(counts["hyp_dur"]) + \
        [counts[name] for name in truth.SCALARS]
    assert [Fraction(float(v)) for v in got] == truth.flat(want)


def test_host_logic_example_by_hand():
    """ref: alice 0-10, bob 10-20; hyp: 0 on 0-9, 1 on 9-12, 2 on 12-20, 3 on 30-31.  Inside the reference extent
    [0, 20] one speaker is on on each side everywhere: total 20, no false alarm, no miss.  The optimal mapping is
    0 -> alice (9 s), 2 -> bob (8 s); speaker 1 stays unmapped, so all of its 3 s (one second of alice, two of bob)
    are confusion: correct 17, confusion 3.  (Mapping 1 -> bob instead of 2 -> bob would match 2 s, not 8.)"""
    ref, hyp = _host_logic_example()
    metric = am.DiarizationErrorRate()
    detail = metric(ref, hyp, uem=[Segment(0, 20)], detailed=True)
    assert detail == {"total": 20.0, "correct": 17.0, "false alarm": 0.0, "missed detection": 0.0, "confusion": 3.0,
                      "diarization error rate": 3.0 / 20.0}
    assert metric.optimal_mapping(ref, hyp, uem=[Segment(0, 20)]) == {0: "alice", 2: "bob"}
    # without a uem the evaluated region is approximated by the extent [0, 31] of both: the turn at 30-31 lies
    # outside the reference, inside that region, and becomes one second of false alarm
    with pytest.warns(UserWarning, match="approximated"):
        detail = am.DiarizationErrorRate()(ref, hyp, detailed=True)
    assert detail["false alarm"] == 1.0 and detail["total"] == 20.0 and detail["confusion"] == 3.0
    assert detail["diarization error rate"] == 4.0 / 20.0
    # ... and the same through a file mapping, with and without "annotated"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert am.DiarizationErrorRate()({"annotation": ref, "annotated": [Segment(0, 20)]}, hyp) == 3.0 / 20.0
    labels_r, rows_r = truth.rows_of(ref)
    labels_h, rows_h = truth.rows_of(hyp)
    _assert_counts_equal_truth(am.annotation_counts(ref, hyp, uem=[Segment(0, 31)]),
                               truth.truth_counts(rows_r, rows_h, [(0, 31)], 2, 4))


def test_collar_by_hand():
    """collar 0.5 removes (-0.25, 0.25), (9.75, 10.25) -- the collars of alice's end and bob's start coincide and
    are removed once -- and (19.75, 20.25).  Reference speech left: 20 - 0.25 - 0.5 - 0.25 = 19.  Speaker 0 keeps
    0.25-9 = 8.75 s of alice, speaker 2 keeps 12-19.75 = 7.75 s of bob: correct 16.5; speaker 1 keeps 9-9.75 and
    10.25-12 = 2.5 s, all confusion.  The turn at 30-31 stays one second of false alarm."""
    ref, hyp = _host_logic_example()
    detail = am.DiarizationErrorRate(collar=0.5)(ref, hyp, uem=[Segment(0, 31)], detailed=True)
    assert detail["total"] == 19.0 and detail["correct"] == 16.5 and detail["confusion"] == 2.5
    assert detail["false alarm"] == 1.0 and detail["missed detection"] == 0.0
    counts = am.annotation_counts(ref, hyp, uem=[Segment(0, 31)], collar=0.5)
    assert counts["ref_speech"] == 19.0 and counts["hyp_speech"] == 20.0 and counts["both_speech"] == 19.0
    _assert_counts_equal_truth(counts, truth.truth_counts(truth.rows_of(ref)[1], truth.rows_of(hyp)[1], [(0, 31)],
                                                          2, 4, collar=0.5))


def test_skip_overlap_three_reference_speakers():
    """a on 0-6, b on 2-8, c on 4-10: pairs overlap on 2-4 (a b) and 6-8 (b c), all three on 4-6.  Only 0-2 (a) and
    8-10 (c) are evaluated."""
    ref = _annotation([(0, 6, "a"), (2, 8, "b"), (4, 10, "c")])
    hyp = _annotation([(0, 10, "x")])
    counts = am.annotation_counts(ref, hyp, uem=[Segment(0, 10)], skip_overlap=True)
    assert counts["total"] == 4.0 and counts["both"] == 4.0 and counts["hyp_speech"] == 4.0
    assert counts["cooc"].ravel().tolist() == [2.0, 0.0, 2.0] and counts["ref_dur"].tolist() == [2.0, 0.0, 2.0]
    full = am.annotation_counts(ref, hyp, uem=[Segment(0, 10)])
    assert full["total"] == 18.0 and full["missed"] == 8.0 and full["both"] == 10.0 and full["ref_speech"] == 10.0
    for skip in (False, True):
        _assert_counts_equal_truth(
            am.annotation_counts(ref, hyp, uem=[Segment(0, 10)], skip_overlap=skip),
            truth.truth_counts(truth.rows_of(ref)[1], truth.rows_of(hyp)[1], [(0, 10)], 3, 1, skip_overlap=skip))


def test_same_label_overlap_counts_once_and_zero_length_pieces_count_nothing():
    ref = _annotation([(0, 4, "a"), (2, 6, "a")])
    hyp = _annotation([(0, 6, "x"), (6, 6.0000005, "y")])
    counts = am.annotation_counts(ref, hyp, uem=[Segment(0, 6), Segment(3, 3)])
    assert counts["total"] == 6.0 and counts["ref_dur"].tolist() == [6.0] and counts["false_alarm"] == 0.0


def test_greedy_against_hungarian():
    """rows are hypothesis labels, columns reference labels: [[5, 4, 0], [4, 0, 0], [0, 0, 1]].  Greedy takes (0, 0)
    = 5 first, which leaves hypothesis 1 nothing, then (2, 2): {0: 0, 2: 2}, correct 6.  Hungarian takes (0, 1),
    (1, 0), (2, 2): {0: 1, 1: 0, 2: 2}, correct 9."""
    together = np.array([[5.0, 4.0, 0.0], [4.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    cooc = together.T                                  # (reference, hypothesis), as `annotation_counts` returns it
    assert am.greedy_mapping(cooc) == {0: 0, 2: 2}
    assert am.optimal_mapping(cooc) == {0: 1, 1: 0, 2: 2}
    # the same through annotations: reference r0 r1 r2, hypothesis h0 h1 h2, durations as in the matrix
    ref = _annotation([(0, 5, "r0"), (10, 14, "r0"), (5, 9, "r1"), (20, 21, "r2")])
    hyp = _annotation([(0, 9, "h0"), (10, 14, "h1"), (20, 21, "h2")])
    uem = [Segment(0, 21)]
    assert np.array_equal(am.annotation_counts(ref, hyp, uem=uem)["cooc"].T, together)
    greedy, optimal = am.GreedyDiarizationErrorRate(), am.DiarizationErrorRate()
    assert greedy.greedy_mapping(ref, hyp, uem=uem) == {"h0": "r0", "h2": "r2"}
    assert greedy.optimal_mapping(ref, hyp, uem=uem) == {"h0": "r1", "h1": "r0", "h2": "r2"}
    g, o = greedy(ref, hyp, uem=uem, detailed=True), optimal(ref, hyp, uem=uem, detailed=True)
    assert (g["correct"], g["confusion"], g["total"]) == (6.0, 8.0, 14.0)
    assert (o["correct"], o["confusion"], o["total"]) == (9.0, 5.0, 14.0)


def test_greedy_row_major_tie():
    """all four entries equal: the first maximum in row-major order is (hypothesis 0, reference 0), then (1, 1)"""
    assert am.greedy_mapping(np.full((2, 2), 3.0)) == {0: 0, 1: 1}
    # [[2, 7], [7, 7]] as (hypothesis, reference): first 7 in row-major order is (0, 1); then only (1, 0) is left
    assert am.greedy_mapping(np.array([[2.0, 7.0], [7.0, 7.0]]).T) == {0: 1, 1: 0}
    assert am.greedy_mapping(np.zeros((2, 3))) == {} and am.greedy_mapping(np.zeros((0, 3))) == {}


def test_names_that_collide_across_sides():
    """the hypothesis calls its speakers "alice" and "bob" the wrong way round, and a third one "carol" who never
    overlaps the reference's carol.  The mapping works on indices: hypothesis "alice" -> reference "bob"; the
    unmapped hypothesis "carol" is not taken for the reference's."""
    ref = _annotation([(0, 10, "alice"), (10, 20, "bob"), (20, 22, "carol")])
    hyp = _annotation([(0, 10, "bob"), (10, 20, "alice"), (30, 31, "carol")])
    uem = [Segment(0, 31)]
    metric = am.DiarizationErrorRate()
    assert metric.optimal_mapping(ref, hyp, uem=uem) == {"bob": "alice", "alice": "bob"}
    detail = metric(ref, hyp, uem=uem, detailed=True)
    assert (detail["correct"], detail["confusion"], detail["missed detection"], detail["false alarm"]) == \
        (20.0, 0.0, 2.0, 1.0)
    # matched by name instead, everything that was said is confusion
    ier = am.IdentificationErrorRate()(ref, hyp, uem=uem, detailed=True)
    assert (ier["correct"], ier["confusion"], ier["missed detection"], ier["false alarm"], ier["total"]) == \
        (0.0, 20.0, 2.0, 1.0, 22.0)
    assert am.IdentificationErrorRate()(ref, ref, uem=uem) == 0.0


def test_empty_sides():
    empty = pa.Annotation()
    hyp = _annotation([(0, 3, "x")])
    for cls in (am.DiarizationErrorRate, am.GreedyDiarizationErrorRate, am.IdentificationErrorRate,
                am.DetectionErrorRate):
        assert cls()(empty, hyp, uem=[Segment(0, 5)]) == 1.0
        assert cls()(empty, empty, uem=[Segment(0, 5)]) == 0.0
        with pytest.warns(UserWarning, match="approximated"):
            assert cls()(empty, empty) == 0.0
    f = am.DetectionPrecisionRecallFMeasure()
    assert f(empty, empty, uem=[Segment(0, 5)]) == 1.0
    assert f(empty, hyp, uem=[Segment(0, 5)]) == 0.0 and f.compute_metrics() == (0.0, 1.0, 0.0)


def test_detection_metrics_by_hand():
    """reference speech 0-10 (two speakers overlapping on 4-6), hypothesis speech 2-12: both 8, false alarm 2, miss 2"""
    ref = _annotation([(0, 6, "a"), (4, 10, "b")])
    hyp = _annotation([(2, 12, "SPEECH")])
    uem = [Segment(0, 20)]
    detail = am.DetectionErrorRate()(ref, hyp, uem=uem, detailed=True)
    assert detail == {"total": 10.0, "false alarm": 2.0, "miss": 2.0, "detection error rate": 0.4}
    f = am.DetectionPrecisionRecallFMeasure(beta=2.0)
    detail = f(ref, hyp, uem=uem, detailed=True)
    assert (detail["retrieved"], detail["relevant"], detail["relevant retrieved"]) == (10.0, 10.0, 8.0)
    precision, recall, fscore = f.compute_metrics()
    assert (precision, recall) == (0.8, 0.8) and fscore == pytest.approx(0.8)
    assert detail["F[precision|recall]"] == fscore


def test_accumulation_over_two_files():
    ref, hyp = _host_logic_example()
    ref2 = _annotation([(0, 4, "a")], uri="second")
    hyp2 = _annotation([(1, 6, "x")])
    metric = am.GreedyDiarizationErrorRate()
    first = metric(ref, hyp, uem=[Segment(0, 31)], detailed=True)
    second = metric(ref2, hyp2, uem=[Segment(0, 10)], detailed=True)
    assert (second["total"], second["correct"], second["false alarm"], second["missed detection"]) == (4.0, 3.0, 2.0, 1.0)
    for name in am.GreedyDiarizationErrorRate.metric_components():
        assert metric[name] == first[name] + second[name]
    assert metric[:] == {name: first[name] + second[name] for name in metric.metric_components()}
    assert abs(metric) == (1.0 + 3.0 + 2.0 + 1.0) / 24.0
    assert [uri for uri, _ in metric] == ["r", "second"]
    assert metric(ref2, hyp2, uem=[Segment(0, 10)], uri="again") == 0.75 and metric.results_[-1][0] == "again"
    metric.reset()
    assert metric["total"] == 0 and list(metric) == []


def test_refuses_nan_and_reversed_segments():
    good = _annotation([(0, 1, "a")])
    with pytest.raises(ValueError, match="NaN"):
        am.annotation_counts(good, good, uem=[Segment(0.0, float("nan"))])
    with pytest.raises(ValueError, match="ends before"):
        am.annotation_counts(good, good, uem=[Segment(2.0, 1.0)])
    with pytest.raises(ValueError, match="collar"):
        am.annotation_counts(good, good, uem=[Segment(0.0, 1.0)], collar=-1.0)


def test_macro_average_f_measure():
    """three classes, "noise" absent from the reference.  speech: reference 0-10, hypothesis 0-8 -> P 1, R 0.8,
    F 8/9.  music: reference 10-14, hypothesis 12-16 -> P 0.5, R 0.5, F 0.5.  noise: reference nothing, hypothesis
    18-19 -> P 0, R 1 (nothing relevant), F 0."""
    ref = _annotation([(0, 10, "speech"), (10, 14, "music")], uri="f")
    hyp = _annotation([(0, 8, "speech"), (12, 16, "music"), (18, 19, "noise")])
    metric = am.MacroAverageFMeasure(classes=["speech", "music", "noise"])
    detail = metric(ref, hyp, uem=[Segment(0, 20)], detailed=True)
    assert detail["speech"] == pytest.approx(8.0 / 9.0) and detail["music"] == 0.5 and detail["noise"] == 0.0
    assert detail["Macro F-measure"] == pytest.approx((8.0 / 9.0 + 0.5) / 3.0)
    assert abs(metric) == pytest.approx((8.0 / 9.0 + 0.5) / 3.0)
    report = metric.report()
    assert report["f"]["music"] == 0.5 and report["TOTAL"]["speech"] == pytest.approx(8.0 / 9.0)
    # a class that neither side has is a perfect score, as DetectionPrecisionRecallFMeasure has it
    assert am.MacroAverageFMeasure(classes=["speech", "laugh"])(ref, hyp, uem=[Segment(0, 20)]) == \
        pytest.approx((8.0 / 9.0 + 1.0) / 2.0)


@pytest.mark.parametrize("Kr,Kh", [(65, 3), (3, 65)])
def test_more_than_64_labels_take_the_host_path(Kr, Kh):
    """also with a `cuda` device asked for (this test has no GPU: reaching for one would raise)"""
    case = truth.random_dyadic_case(5, Nr=Kr + 20, Nh=Kh + 20, Nu=3, Kr=Kr, Kh=Kh, collar=0.25, span=32.0, shortest_ticks=1)
    ref = _annotation([(a, b, f"r{l:02d}") for a, b, l in case["ref"]])
    hyp = _annotation([(a, b, f"h{l:02d}") for a, b, l in case["hyp"]])
    assert len(ref.labels()) == Kr and len(hyp.labels()) == Kh
    counts = am.annotation_counts(ref, hyp, uem=[Segment(a, b) for a, b in case["uem"]], collar=0.25, device="cuda")
    _assert_counts_equal_truth(counts, truth.case_truth(case))


@pytest.mark.parametrize("seed,collar,skip", [(0, 0.0, False), (1, 0.5, False), (2, 0.0, True), (3, 0.125, True)])
def test_host_sweep_equals_truth_on_random_dyadic_cases(seed, collar, skip):
    case = truth.random_dyadic_case(seed, Nr=60, Nh=70, Nu=4, Kr=5, Kh=6, collar=collar, skip_overlap=skip,
                                    span=48.0, shortest_ticks=1)
    ref = _annotation([(a, b, l) for a, b, l in case["ref"]])
    hyp = _annotation([(a, b, l) for a, b, l in case["hyp"]])
    counts = am.annotation_counts(ref, hyp, uem=[Segment(a, b) for a, b in case["uem"]], collar=collar,
                                  skip_overlap=skip)
    _assert_counts_equal_truth(counts, truth.case_truth(case))


def test_get_metric_of_the_pipelines(pipeline_dir):
    assert not hasattr(pa, "GreedyDiarizationErrorRate")        # the classes are not re-exported at top level
    pipeline = pa.Pipeline.from_pretrained(pipeline_dir)
    metric = pipeline.get_metric()
    assert type(metric) is am.GreedyDiarizationErrorRate
    assert (metric.collar, metric.skip_overlap) == (0.0, False) and pipeline.get_direction() == "minimize"
    custom = pa.SpeakerDiarization(segmentation=os.path.join(pipeline_dir, "segmentation"),
                                   embedding=os.path.join(pipeline_dir, "embedding"),
                                   clustering="AgglomerativeClustering",
                                   der_variant={"collar": 0.25, "skip_overlap": True})
    metric = custom.get_metric()
    assert type(metric) is am.GreedyDiarizationErrorRate and (metric.collar, metric.skip_overlap) == (0.25, True)
    vad = pa.VoiceActivityDetection(segmentation=os.path.join(pipeline_dir, "segmentation"))
    metric = vad.get_metric()
    assert type(metric) is am.DetectionErrorRate and (metric.collar, metric.skip_overlap) == (0.0, False)
    assert vad.get_direction() == "minimize"
    vad = pa.VoiceActivityDetection(segmentation=os.path.join(pipeline_dir, "segmentation"), fscore=True)
    metric = vad.get_metric()
    assert type(metric) is am.DetectionPrecisionRecallFMeasure and (metric.collar, metric.skip_overlap) == (0.0, False)
    assert vad.get_direction() == "maximize"
