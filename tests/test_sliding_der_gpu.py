"""GPU: `SlidingDiarizationErrorRate(device=cuda)` -- every window of a file counted in one `pa_annot_window_counts`
call -- against the literal loop of the reference class (utils/metric.py:258-279) written with the package's
`DiarizationErrorRate` on `crop`ped annotations.  The file is dyadic (tests/window_counts_cases.conversation), so the
sums of both routes are exact and `==` is the right comparison."""
import pytest

import window_counts_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("speakers", [3, 4, 5])
def test_sliding_der_equals_the_literal_loop(gpu_device, speakers):
    from pyannote_audio_amd import annotation_metrics as am
    cases.check_sliding(am, speakers, device=gpu_device)


def test_window_counts_on_the_device_equal_the_numpy_form(gpu_device):
    """the public function: one upload, one call, one download; the dict of arrays, bit for bit the host's on a
    dyadic file, windows as `Segment`s or as an array"""
    import numpy as np
    import pyannote_audio_amd as pa
    from pyannote_audio_amd import annotation_metrics as am
    from pyannote_audio_amd.core import Segment
    ref_rows, hyp_rows, uem_rows = cases.conversation(9, 4, turns=60, span=64.0)
    reference, hypothesis = pa.Annotation(), pa.Annotation()
    for annotation, rows in ((reference, ref_rows), (hypothesis, hyp_rows)):
        for n, (start, end, label) in enumerate(rows):
            annotation[Segment(start, end), n] = label
    uem = [Segment(a, b) for a, b in uem_rows]
    windows = cases.random_windows(5, 30, span=64.0, longest=8.0)
    for collar, skip in ((0.0, False), (0.25, True)):
        kw = dict(uem=uem, collar=collar, skip_overlap=skip)
        dev = am.window_counts(reference, hypothesis, [Segment(a, b) for a, b in windows], device=gpu_device, **kw)
        host = am.window_counts(reference, hypothesis, np.array(windows), **kw)
        assert dev["ref_labels"] == host["ref_labels"] and dev["hyp_labels"] == host["hyp_labels"]
        assert dev["cooc"].shape == (30, 4, 4) and dev["ref_dur"].shape == (30, 4) and dev["total"].shape == (30,)
        for key in ("cooc", "ref_dur", "hyp_dur", "total", "false_alarm", "missed", "both", "ref_speech",
                    "hyp_speech", "both_speech"):
            assert np.array_equal(dev[key], host[key]), key
        assert dev["total"].any() and dev["cooc"].any()
    empty = am.window_counts(reference, hypothesis, [], uem=uem, device=gpu_device)
    assert empty["cooc"].shape == (0, 4, 4) and empty["total"].shape == (0,)
    with pytest.raises(ValueError, match="ends before"):
        am.window_counts(reference, hypothesis, [Segment(3.0, 2.0)], uem=uem, device=gpu_device)
