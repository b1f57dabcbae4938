"""The streaming formulation of detection (tests/online_detect_model.py, the numpy statement of `pao_detect_step`) pinned
to the offline one without a device: at full latency a streamed recording gives `frames_model.aggregate` on all its
chunks followed by `multilabel_oracle.all_regions` (the host model of `pa_binarize_regions`), values, regions and
tracks compared with `==`; at the shortest latency every emission is the aggregate of the chunks seen so far."""
import itertools

import numpy as np
import pytest

import frames_model as fm
import multilabel_oracle as mo
import online_detect_model as dm

SAMPLE_RATE, DURATION, STEP = 16000, 5.0, 0.5
WINDOW, STEP_SAMPLES = 80000, 8000
FRAME_STEP, FRAME_DURATION = 270 / 16000, 991 / 16000        # PyanNet's receptive field (SincNet stride 10)
#: shorter than a chunk, a whole number of steps, a ragged tail
LENGTHS = {"short": 30000, "whole-steps": WINDOW + 3 * STEP_SAMPLES, "ragged": 116800}
DURATIONS = [(0.0, 0.0), (0.0, 0.12), (0.1, 0.0), (0.15, 0.1)]           # (min_duration_on, min_duration_off)
THRESHOLDS = [(0.6, 0.4), (0.5, 0.5), (0.4, 0.6)]                       # offset <, = and > onset
EPSILON, MISSING = 1e-12, 0.0
S = 3


def _geometry():
    from pyannote_audio_amd.core import SlidingWindow
    from pyannote_audio_amd.segmentation import num_frames
    return SlidingWindow(start=0.0, duration=FRAME_DURATION, step=FRAME_STEP), num_frames(WINDOW)


def _schedule(num_samples, latency):
    from pyannote_audio_amd.online import file_schedule
    frames, F = _geometry()
    return file_schedule(num_samples, window=WINDOW, step_samples=STEP_SAMPLES, sample_rate=SAMPLE_RATE,
                         duration=DURATION, step=STEP, latency=latency, frames=frames, F=F)


def _offline_grid(C):
    """start frame of every chunk and the frames they cover, as offline inference lays them out"""
    from pyannote_audio_amd.core import SlidingWindow
    from pyannote_audio_amd.frames import frame_geometry
    frames, _ = _geometry()
    starts, T, _ = frame_geometry(SlidingWindow(start=0.0, duration=DURATION, step=STEP), frames, C)
    return starts, T


def _chunk_scores(seed, starts, F, T):
    """(C, F, S) float32: every chunk sees one slowly wandering signal per class through noise of its own, so the
    aggregate crosses the thresholds a few times; NaN frames in single classes, one frame NaN in every chunk"""
    rng = np.random.default_rng(seed)
    signal = mo.smooth_scores(rng, T, S, width=15)
    scores = np.stack([signal[a:a + F] for a in starts]) + rng.normal(0, 0.03, (len(starts), F, S)).astype(np.float32)
    scores = scores.astype(np.float32)
    scores.reshape(-1)[rng.integers(0, scores.size, size=scores.size // 40)] = np.nan
    for c, a in enumerate(starts):                       # global frame 60 is NaN in class 1 of every chunk covering it
        if a <= 60 < a + F:
            scores[c, 60 - a, 1] = np.nan
    return scores


def _window(F, warm_up=0):
    warm = np.ones(F)
    if warm_up:
        warm[:warm_up] = EPSILON
        warm[F - warm_up:] = EPSILON
    return np.hamming(F), warm


@pytest.fixture(scope="module")
def recordings():
    """per length: (scores, starts, T covered, total kept, full-latency schedule)"""
    out = {}
    for seed, (name, n) in enumerate(LENGTHS.items()):
        C, rows, total = _schedule(n, DURATION)
        starts, T = _offline_grid(C)
        _, F = _geometry()
        assert (rows[:C, 0] == starts).all() and total <= T and starts[-1] + F <= T
        out[name] = (_chunk_scores(100 + seed, starts, F, T), starts, T, total, rows)
    return out


@pytest.mark.parametrize("length", list(LENGTHS))
@pytest.mark.parametrize("any", [False, True], ids=["classes", "any"])
def test_full_latency_is_the_offline_pipeline(recordings, length, any):
    scores, starts, T, total, rows = recordings[length]
    frames, F = _geometry()
    grid = (0.0, frames.duration, frames.step)
    window, warm = _window(F, warm_up=0 if length == "short" else 7)
    K = 1 if any else S
    collapsed = np.max(scores, axis=-1, keepdims=True) if any else scores
    offline = fm.aggregate(collapsed, starts, T, window, warm, EPSILON, MISSING, 0)[:total]
    assert np.isnan(collapsed[:, :, -1 if any else 1]).any() and (offline[60] == MISSING).any()    # nobody voted there
    seen = set()
    for (onset, offset), (min_on, min_off) in itertools.product(THRESHOLDS, DURATIONS):
        spread = lambda v: [v + 0.01 * k for k in range(K)]                       # noqa: E731  (per-class parameters)
        values, active, per_class, calls = dm.stream_file(
            scores, rows, any, window, warm, EPSILON, MISSING, grid, spread(onset), spread(offset),
            [min_on] * K, [min_off] * K)
        assert values.shape == (total, K) and fm.same_bits(values, offline)
        assert calls[0][0] == 0 and calls[-1][1] == total
        want = mo.all_regions(offline, *grid, spread(onset), spread(offset), min_on, min_off)
        for k in range(K):
            assert per_class[k][0] == want[k][0], (length, any, onset, offset, min_on, min_off, k)
            assert per_class[k][1] == want[k][1], (length, any, onset, offset, min_on, min_off, k)
            # (a track list with a hole: a merged region was dropped by min_duration_on and still counted)
            seen.add((len(want[k][0]) > 0, min_off > 0 and want[k][1] != list(range(len(want[k][1])))))
        # the states are those of the plain rule on the offline values
        state = np.zeros(K, dtype=bool)                                            # frame 0 finds the stream inactive
        for t in range(total):
            v = offline[t]
            with np.errstate(invalid="ignore"):
                state = np.where(state, ~(v < np.asarray(spread(offset), dtype=np.float32)),
                                 v > np.asarray(spread(onset), dtype=np.float32))
            assert (active[t] == state).all()
    assert (True, False) in seen                                                   # regions were found ...
    if length != "short" and not any:
        assert (True, True) in seen                         # ... and a merged region was dropped by min_duration_on


@pytest.mark.parametrize("length", list(LENGTHS))
def test_hard_decisions_any_give_the_bits_of_their_float_image(recordings, length):
    """uint8 hard decisions with `any`: the values and regions of the same decisions as float32 0 / 1"""
    scores, _, _, total, rows = recordings[length]
    frames, F = _geometry()
    grid = (0.0, frames.duration, frames.step)
    window, warm = _window(F)
    hard = (np.nan_to_num(scores, nan=0.0) > 0.55).astype(np.uint8)
    hard[hard == 1] = np.random.default_rng(3).integers(1, 256, size=int(hard.sum()))       # any non-zero byte is 1
    args = (rows, True, window, warm, EPSILON, MISSING, grid, [0.5], [0.5], [0.05], [0.1])
    a = dm.stream_file(hard, *args)
    b = dm.stream_file((hard != 0).astype(np.float32), *args)
    assert fm.same_bits(a[0], b[0]) and (a[1] == b[1]).all() and a[2] == b[2] and a[0].shape == (total, 1)
    assert len(a[2][0][0]) >= (1 if length != "short" else 0)


@pytest.mark.parametrize("length", list(LENGTHS))
def test_shortest_latency_is_the_aggregate_of_the_chunks_seen_so_far(recordings, length):
    scores, starts, T, total, _ = recordings[length]
    frames, F = _geometry()
    grid = (0.0, frames.duration, frames.step)
    window, warm = _window(F, warm_up=5)
    C, rows, total_again = _schedule(LENGTHS[length], STEP)
    assert total_again == total and C == len(scores)
    values, _, _, calls = dm.stream_file(scores, rows, False, window, warm, EPSILON, MISSING, grid, [0.5] * S,
                                         [0.5] * S, [0.0] * S, [0.0] * S)
    emitted_early = 0
    for c, (ga, gb) in enumerate(calls):
        seen = min(c + 1, C)
        covered = int(starts[seen - 1]) + F
        so_far = fm.aggregate(scores[:seen], starts[:seen], max(covered, gb), window, warm, EPSILON, MISSING, 0)
        assert fm.same_bits(values[ga:gb], so_far[ga:gb]), (length, c)
        emitted_early += (gb - ga) if c < C - 1 else 0
    if C > 1:                  # frames left before later chunks covered them: not the offline values any more
        offline = fm.aggregate(scores, starts, T, window, warm, EPSILON, MISSING, 0)[:total]
        assert emitted_early > 0 and not fm.same_bits(values, offline)


# ------------------------------------------------------------------------------------------ the rule, frame by frame
def _frame_by_frame(values, onset, offset, min_on, min_off, grid=(0.0, 0.0619375, 0.016875)):
    """one class, one frame per call (F = 1, unit weights: the emitted value is the score, NaN where it is NaN), the
    last call closing -> [(call, start, end, track)]"""
    state = dm.fresh_state(1, 2, 1)
    out = []
    T = len(values)
    for g, v in enumerate(values):
        _, _, n, regions, tracks = dm.detect_step_one(
            state, 0, np.array([[v]], dtype=np.float32), False, [1.0], [1.0], EPSILON, np.nan, g, g, g + 1,
            g == T - 1, grid, [onset], [offset], [min_on], [min_off], 1, 2)
        out += [(g, float(regions[0, i, 0]), float(regions[0, i, 1]), int(tracks[0, i])) for i in range(n[0])]
    return out


def _t(g):
    return dm.frame_time(g, 0.0, 0.0619375, 0.016875)


def test_when_a_region_becomes_final():
    hi, lo = 0.9, 0.1
    # without min_duration_off a region is final the moment it closes
    assert _frame_by_frame([lo, hi, hi, lo, lo, hi, lo], 0.5, 0.5, 0.0, 0.0) == \
        [(3, _t(1), _t(3), 0), (6, _t(5), _t(6), 0)]
    # with it, a region waits: a gap of 2 frames (0.03375 s) < 0.05 merges, the merged region leaves at the close
    assert _frame_by_frame([lo, hi, hi, lo, lo, hi, lo], 0.5, 0.5, 0.0, 0.05) == [(6, _t(1), _t(6), 0)]
    # a gap that is not smaller finalises the pending region at the on-event, before the next region closes
    assert _frame_by_frame([lo, hi, lo, lo, lo, lo, hi, hi, lo, lo], 0.5, 0.5, 0.0, 0.05) == \
        [(6, _t(1), _t(2), 0), (9, _t(6), _t(8), 1)]
    # a merged region dropped by min_duration_on still counts: the next one is track 1
    assert _frame_by_frame([lo, hi, lo, lo, lo, lo, hi, hi, hi, lo], 0.5, 0.5, 0.03, 0.02) == [(9, _t(6), _t(9), 1)]
    # open at the end: closes on the last frame; an on-event ON the last frame is empty; one frame gives nothing
    assert _frame_by_frame([lo, hi, hi, hi], 0.5, 0.5, 0.0, 0.0) == [(3, _t(1), _t(3), 0)]
    assert _frame_by_frame([lo, lo, lo, hi], 0.5, 0.5, 0.0, 0.0) == []
    assert _frame_by_frame([hi], 0.5, 0.5, 0.0, 0.0) == []
    assert _frame_by_frame([hi, hi], 0.5, 0.5, 0.0, 0.0) == [(1, _t(0), _t(1), 0)]
    # values exactly on the thresholds change nothing; NaN changes nothing; offset > onset swaps every frame in between
    on, off = float(np.float32(0.6)), float(np.float32(0.4))
    assert _frame_by_frame([on, hi, off, np.nan, lo, lo], 0.6, 0.4, 0.0, 0.0) == [(4, _t(1), _t(4), 0)]
    assert _frame_by_frame([0.5, 0.5, 0.5, 0.5, 0.5], 0.4, 0.6, 0.0, 0.0) == \
        [(1, _t(0), _t(1), 0), (3, _t(2), _t(3), 0)]
    for values in ([lo, hi, hi, lo, lo, hi, lo], [hi, lo, hi, np.nan, hi], [0.5] * 6):
        for onset, offset, min_on, min_off in ((0.5, 0.5, 0.0, 0.0), (0.4, 0.6, 0.0, 0.05), (0.6, 0.4, 0.03, 0.02)):
            got = _frame_by_frame(values, onset, offset, min_on, min_off)
            want = mo.class_regions(np.asarray(values, dtype=np.float32), 0.0, 0.0619375, 0.016875, onset, offset,
                                    min_on, min_off)
            assert [(s, e) for _, s, e, _ in got] == want[0] and [t for _, _, _, t in got] == want[1]
