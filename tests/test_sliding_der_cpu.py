"""No GPU: the numpy form of `annotation_metrics.window_counts` against the exact truth (the cases of
tests/test_window_counts_gpu.py that need no device: `==` on dyadic cases, the derived bound otherwise),
`SlidingDiarizationErrorRate` against the literal loop of the reference class, and the two `pyannote.core` stand-ins
the loop needs (`SlidingWindow.__call__`, `Annotation.crop`)."""
from fractions import Fraction

import numpy as np
import pytest

import pyannote_audio_amd as pa
from pyannote_audio_amd import annotation_metrics as am
from pyannote_audio_amd.core import Segment, SlidingWindow
from pyannote_audio_amd.metrics import Timeline

import annotation_metrics_truth as truth
import window_counts_cases as cases


def _host(case) -> np.ndarray:
    """the numpy form on a case of the truth module -> (W, Kr*Kh + Kr + Kh + 7)"""
    seg = lambda rows: np.array([(r[0], r[1]) for r in rows], dtype=np.float64).reshape(-1, 2)  # noqa: E731
    lab = lambda rows: np.array([r[2] for r in rows], dtype=np.int32)  # noqa: E731
    return am._host_window_counts(seg(case["ref"]), lab(case["ref"]), case["Kr"], seg(case["hyp"]), lab(case["hyp"]),
                                  case["Kh"], seg(case["uem"]), seg(case["windows"]), float(case["collar"]),
                                  bool(case["skip_overlap"]))


def _exact(case) -> np.ndarray:
    cases.assert_dyadic(case)
    out = _host(case)
    assert out.shape == (len(case["windows"]), case["Kr"] * case["Kh"] + case["Kr"] + case["Kh"] + 7)
    for w, (row, want) in enumerate(zip(out.tolist(), cases.window_truths(case))):
        assert [Fraction(v) for v in row] == truth.flat(want), (w, case["windows"][w])
    return out


@pytest.mark.parametrize("collar", [0.0, 0.25, 0.5, 1.0])
@pytest.mark.parametrize("skip", [False, True])
def test_hand_built_edges(collar, skip):
    case = cases.hand_case(collar, skip)
    out = _exact(case)
    assert not out[list(cases.HAND_ZERO_ROWS)].any()
    down = sorted(case["windows"], reverse=True)
    flipped = _exact(cases.hand_case(collar, skip, down))
    for w, window in enumerate(down):
        assert np.array_equal(flipped[w], out[case["windows"].index(window)])


@pytest.mark.parametrize("windows", [[(3.0, 7.5)], [(5.0, 5.0)], [(50.0, 60.0)], []])
def test_one_window_and_none(windows):
    _exact(cases.hand_case(0.25, False, windows))


def test_empty_sides():
    for Nr, Nh, Nu in ((0, 9, 2), (9, 0, 2), (9, 9, 0), (0, 0, 0), (0, 0, 3)):
        case = truth.random_dyadic_case(11, Nr, Nh, Nu, Kr=3 if Nr else 0, Kh=2 if Nh else 0, collar=0.5, span=8.0)
        out = _exact(cases.with_windows(case, cases.random_windows(Nr + Nh, 5, span=8.0, longest=4.0)))
        if Nu == 0 or (Nr == 0 and Nh == 0):
            assert not out.any()


@pytest.mark.parametrize("seed,collar,skip", [(0, 0.0, False), (1, 0.5, False), (2, 0.0, True), (3, 0.125, True)])
def test_random_dyadic_cases(seed, collar, skip):
    case = truth.random_dyadic_case(seed, Nr=60, Nh=70, Nu=4, Kr=5, Kh=6, collar=collar, skip_overlap=skip, span=48.0)
    out = _exact(cases.with_windows(case, cases.random_windows(seed, 25, span=48.0, longest=12.0)))
    assert out[:, -7].any()


@pytest.mark.parametrize("name,Nr,Nh,Nu,W,collar", cases.SHAPES)
@pytest.mark.parametrize("skip", [False, True])
def test_sizes_where_the_kernels_change_shape(name, Nr, Nh, Nu, W, collar, skip):
    _exact(cases.shape_case(name, Nr, Nh, Nu, W, collar, skip))


def test_64_labels_with_bit_63_inside_one_window_only():
    case = cases.labels64_case()
    _exact(dict(case, skip_overlap=True))
    out = _exact(case)
    assert out[1, 63 * 64 + 63] > 0.0 and not out[[0, 2, 3, 4], 63 * 64 + 63].any()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_intervals_in_a_window(n):
    _exact(cases.range_case(n))


@pytest.mark.parametrize("collar,skip", [(0.0, False), (2.0 ** -6, True)])
def test_non_dyadic_within_the_derived_bound(collar, skip):
    case, truths, n = cases.non_dyadic(collar, skip)
    worst = cases.check_within_bound(_host(case).tolist(), case, truths, n)
    print(f"non-dyadic windows, numpy (collar {collar}, skip_overlap {skip}): n = {n}, worst relative error "
          f"{worst:.3e}, bound {n * 2.0 ** -52:.3e}")


def _annotation(rows):
    a = pa.Annotation()
    for n, (start, end, label) in enumerate(rows):
        a[Segment(start, end), n] = label
    return a


def test_window_counts_through_annotations():
    """the public function: labels in `labels()` order, the shapes, a file mapping, more than 64 labels on a side
    (the numpy form also with a `cuda` device asked for: this test has no GPU, reaching for one would raise)"""
    case = truth.random_dyadic_case(5, Nr=85, Nh=30, Nu=3, Kr=65, Kh=4, collar=0.25, span=32.0, shortest_ticks=1)
    case = cases.with_windows(case, cases.random_windows(2, 12, span=32.0, longest=8.0))
    ref = _annotation([(a, b, f"r{l:02d}") for a, b, l in case["ref"]])
    hyp = _annotation([(a, b, f"h{l}") for a, b, l in case["hyp"]])
    uem = [Segment(a, b) for a, b in case["uem"]]
    counts = am.window_counts({"annotation": ref, "annotated": uem}, hyp, [Segment(a, b) for a, b in case["windows"]],
                              collar=0.25, device="cuda")
    assert counts["ref_labels"] == ref.labels() and counts["hyp_labels"] == hyp.labels()
    assert counts["cooc"].shape == (12, 65, 4) and counts["ref_dur"].shape == (12, 65)
    assert counts["hyp_dur"].shape == (12, 4) and all(counts[name].shape == (12,) for name in truth.SCALARS)
    for w, want in enumerate(cases.window_truths(case)):
        got = list(counts["cooc"][w].ravel()) + list(counts["ref_dur"][w]) + list(counts["hyp_dur"][w]) + \
            [counts[name][w] for name in truth.SCALARS]
        assert [Fraction(float(v)) for v in got] == truth.flat(want)
    again = am.window_counts(ref, hyp, np.array(case["windows"]), uem=uem, collar=0.25)
    assert all(np.array_equal(again[key], counts[key]) for key in ("cooc", "ref_dur", "hyp_dur") + truth.SCALARS)
    with pytest.raises(ValueError, match="NaN"):
        am.window_counts(ref, hyp, [(1.0, float("nan"))], uem=uem)
    with pytest.raises(ValueError, match="ends before"):
        am.window_counts(ref, hyp, [Segment(3.0, 2.0)], uem=uem)
    with pytest.raises(ValueError, match=r"\(W, 2\)"):
        am.window_counts(ref, hyp, np.zeros((4, 3)), uem=uem)
    with pytest.warns(UserWarning, match="approximated"):
        am.window_counts(ref, hyp, [Segment(1.0, 9.0)])


def test_window_error_rates_by_hand():
    """ref: alice 0-10, bob 10-20; hyp: 0 on 0-9, 1 on 9-12, 2 on 12-20.  Window 0-10: alice alone, 0 -> alice 9 s,
    the last second is speaker 1's: confusion 1.  Window 5-15: alice 5-10, bob 10-15; 0 -> alice matches 4 s and
    2 -> bob 3 s (1 -> bob would match 2 s): correct 7, confusion 3.  Window 8-12: alice 8-10, bob 10-12; speaker 2 is
    not in the window, and its own best mapping is 0 -> alice (1 s), 1 -> bob (2 s): correct 3, confusion 1 -- a
    mapping the whole file would not choose (there 2 -> bob).  Window 30-40 lies outside the uem."""
    ref = _annotation([(0, 10, "alice"), (10, 20, "bob")])
    hyp = _annotation([(0, 9, 0), (9, 12, 1), (12, 20, 2)])
    table = am.window_error_rates(ref, hyp, [Segment(0, 10), Segment(5, 15), Segment(8, 12), Segment(30, 40)],
                                  uem=[Segment(0, 20)])
    assert table["total"].tolist() == [10.0, 10.0, 4.0, 0.0]
    assert table["correct"].tolist() == [9.0, 7.0, 3.0, 0.0]
    assert table["confusion"].tolist() == [1.0, 3.0, 1.0, 0.0]
    assert table["false alarm"].tolist() == [0.0] * 4 and table["missed detection"].tolist() == [0.0] * 4
    assert table["diarization error rate"].tolist() == [0.1, 0.3, 0.25, 0.0]


@pytest.mark.parametrize("speakers", [3, 5])
def test_sliding_der_equals_the_literal_loop(speakers):
    cases.check_sliding(am, speakers)


def test_sliding_der_interface():
    metric = am.SlidingDiarizationErrorRate()
    assert metric.window == 10.0 and metric.device is None
    assert metric.metric_name() == "window diarization error rate" == metric.name
    assert metric.metric_components() == ["total", "false alarm", "missed detection", "confusion"]
    assert metric.compute_metric({"total": 8.0, "false alarm": 1.0, "missed detection": 2.0, "confusion": 1.0}) == 0.5
    ref = _annotation([(0, 10, "alice"), (10, 20, "bob")])
    hyp = _annotation([(0, 9, 0), (9, 12, 1), (12, 20, 2)])
    with pytest.raises(ValueError, match="SlidingDiarizationErrorRate expects `uem` to be provided."):
        metric(ref, hyp)
    with pytest.raises(ValueError, match="expects `uem`"):
        metric.windows(ref, hyp)
    # windows 0-10, 5-15, 10-20: (1 + 3 + 2) s of confusion in 30 s
    assert metric(ref, hyp, uem=[Segment(0, 20)]) == 6.0 / 30.0
    assert metric.windows(ref, hyp, uem=Timeline([Segment(0, 20)]))["windows"] == \
        [Segment(0, 10), Segment(5, 15), Segment(10, 20)]


# ------------------------------------------------------------------------------- the pyannote.core stand-ins

def test_sliding_window_over_a_support():
    window = SlidingWindow(duration=4.0, step=2.0)
    assert list(window(Segment(1.0, 4.5))) == []                                   # shorter than the window
    assert list(window(Segment(1.0, 9.0))) == [Segment(1, 5), Segment(3, 7), Segment(5, 9)]      # a multiple
    assert list(window(Segment(1.0, 5.0))) == [Segment(1, 5)]
    assert list(window(Segment(1.0, 10.5))) == [Segment(1, 5), Segment(3, 7), Segment(5, 9)]     # a remainder
    assert list(window(Segment(1.0, 10.5), align_last=True)) == \
        [Segment(1, 5), Segment(3, 7), Segment(5, 9), Segment(6.5, 10.5)]
    assert list(window(Segment(1.0, 9.0), align_last=True)) == [Segment(1, 5), Segment(3, 7), Segment(5, 9)]
    both = Timeline([Segment(20.0, 26.5), Segment(1.0, 5.0), Segment(30.0, 31.0)])
    assert list(window(both)) == [Segment(1, 5), Segment(20, 24), Segment(22, 26)]
    assert list(window(both, align_last=True)) == [Segment(1, 5), Segment(20, 24), Segment(22, 26), Segment(22.5, 26.5)]
    # iteration: the windows that start before `end`; endless without one
    assert list(SlidingWindow(duration=4.0, step=2.0, start=1.0, end=6.0)) == [Segment(1, 5), Segment(3, 7), Segment(5, 9)]
    endless = iter(SlidingWindow(duration=4.0, step=2.0))
    assert [next(endless) for _ in range(3)] == [Segment(0, 4), Segment(2, 6), Segment(4, 8)]


def test_annotation_crop():
    a = pa.Annotation(uri="file")
    a[Segment(0.0, 10.0), "x"] = "alice"
    a[Segment(2.0, 3.0), "y"] = "bob"
    a[Segment(20.0, 30.0), "z"] = "carol"
    cropped = a.crop(Segment(1.0, 2.5))
    assert cropped.uri == "file"
    assert list(cropped.itertracks(yield_label=True)) == [(Segment(1.0, 2.5), "x", "alice"),
                                                          (Segment(2.0, 2.5), "y", "bob")]             # cut at both ends
    assert list(a.crop(Segment(12.0, 18.0)).itertracks(yield_label=True)) == []                       # wholly outside
    assert list(a.crop(Segment(10.0, 20.0)).itertracks(yield_label=True)) == []                       # touching
    support = Timeline([Segment(25.0, 40.0), Segment(2.5, 4.0)])
    assert list(a.crop(support).itertracks(yield_label=True)) == \
        [(Segment(2.5, 3.0), "y", "bob"), (Segment(2.5, 4.0), "x", "alice"), (Segment(25.0, 30.0), "z", "carol")]
    assert a.crop(support, mode="intersection") == a.crop(support)
    # two tracks of one name that land on the same piece: the second gets a fresh name
    b = pa.Annotation()
    b[Segment(0.0, 10.0), "x"] = "alice"
    b[Segment(1.0, 9.0), "x"] = "bob"
    assert sorted(b.crop(Segment(2.0, 3.0)).itertracks(yield_label=True), key=lambda t: t[2]) == \
        [(Segment(2.0, 3.0), "x", "alice"), (Segment(2.0, 3.0), 0, "bob")]
    assert len(a) == 3                                                                                 # (not edited)
