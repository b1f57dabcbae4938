"""GPU: `window_error_rates(device=cuda)` finds the optimal mapping of every window on the device (`pa_lsap_batch`,
one launch) and downloads five numbers a window; the table equals `window_rates_from_counts` on the host counts with
`==`.  The files are dyadic (tests/window_counts_cases.conversation), so the counts of both routes are exact."""
import numpy as np
import pytest

import window_counts_cases as cases

pytestmark = pytest.mark.gpu

COLUMNS = ("total", "correct", "false alarm", "missed detection", "confusion", "diarization error rate")


def _file(speakers: int):
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.core import Segment, SlidingWindow
    from pyannote_audio_amd.metrics import Timeline
    ref_rows, hyp_rows, uem_rows = cases.conversation(speakers, speakers)
    reference, hypothesis = pa.Annotation(), pa.Annotation()
    for annotation, rows in ((reference, ref_rows), (hypothesis, hyp_rows)):
        for n, (start, end, label) in enumerate(rows):
            annotation[Segment(start, end), n] = label
    uem = Timeline([Segment(a, b) for a, b in uem_rows])
    windows = list(SlidingWindow(duration=8.0, step=4.0)(uem))
    return reference, hypothesis, uem, windows


@pytest.mark.parametrize("speakers", [3, 4, 5])
def test_device_mapping_equals_the_host_table(gpu_device, speakers, monkeypatch):
    from pyannote_audio_amd import annotation_metrics as am
    reference, hypothesis, uem, windows = _file(speakers)
    assert len(windows) > 40
    counts = am.window_counts(reference, hypothesis, windows, uem=uem, device=None)
    want = am.window_rates_from_counts(counts)
    # windows in which a label of the file is absent are there: the masks matter
    assert (counts["ref_dur"] == 0).any() and (counts["hyp_dur"] == 0).any() and (want["confusion"] > 0).any()

    def refuse(*args, **kwargs):
        raise AssertionError("the host solver was called")

    monkeypatch.setattr(am, "linear_sum_assignment", refuse)
    got = am.window_error_rates(reference, hypothesis, windows, uem=uem, device=gpu_device)
    assert set(got) == set(want) == set(COLUMNS)
    for name in COLUMNS:
        assert got[name].dtype == np.float64 and got[name].tolist() == want[name].tolist(), name
    # and through the metric class
    table = am.SlidingDiarizationErrorRate(window=8.0, device=gpu_device).windows(reference, hypothesis, uem=uem)
    for name in COLUMNS:
        assert table[name].tolist() == want[name].tolist(), name


def test_windows_without_a_label_on_one_side(gpu_device):
    """a window in which only the reference speaks, one in which only the hypothesis does, one in which nobody does
    and one without length: `correct` is 0, the rate is the host's"""
    import pyannote_audio_amd as pa
    from pyannote_audio_amd import annotation_metrics as am
    from pyannote_audio_amd.core import Segment
    reference, hypothesis = pa.Annotation(), pa.Annotation()
    for n, (a, b, label) in enumerate([(1.0, 3.0, "A"), (2.0, 5.0, "B"), (20.0, 22.0, "A"), (30.0, 31.0, "B")]):
        reference[Segment(a, b), n] = label
    for n, (a, b, label) in enumerate([(1.5, 3.5, "x"), (2.5, 4.5, "y"), (10.0, 12.0, "x"), (30.0, 31.5, "y")]):
        hypothesis[Segment(a, b), n] = label
    uem = [Segment(0.0, 40.0)]
    windows = [Segment(0.0, 8.0), Segment(18.0, 24.0), Segment(8.0, 16.0), Segment(14.0, 18.0), Segment(6.0, 6.0),
               Segment(28.0, 32.0), Segment(0.0, 40.0)]
    want = am.window_rates_from_counts(am.window_counts(reference, hypothesis, windows, uem=uem))
    got = am.window_error_rates(reference, hypothesis, windows, uem=uem, device=gpu_device)
    for name in COLUMNS:
        assert got[name].tolist() == want[name].tolist(), name
    assert got["correct"][1:5].tolist() == [0.0] * 4 and got["correct"][0] > 0 and got["correct"][6] > 0
    assert got["diarization error rate"][1:5].tolist() == [1.0, 1.0, 0.0, 0.0]
    empty = am.window_error_rates(reference, hypothesis, [], uem=uem, device=gpu_device)
    assert all(empty[name].shape == (0,) for name in COLUMNS)
