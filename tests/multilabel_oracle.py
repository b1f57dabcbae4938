"""Frame-by-frame restatement of what MultiLabelSegmentation computes after the model, for the tests
(TEST INFRASTRUCTURE ONLY; written from the rule, one frame and one region at a time, no vectorisation):

  * hysteresis with a state-dependent rule: inactive -> active iff y > onset, active -> inactive iff y < offset;
    float32 scores against float32-rounded thresholds (NumPy 2 compares a float32 scalar with a Python float in
    float32); NaN compares false both ways and changes nothing; the state of frame 0 is y[0] > onset;
  * a region runs from the middle of the frame that switched on to the middle of the frame that switched off, or of
    the last frame when still open; frame middles in float64: 0.5 * (s + (s + duration)), s = start + i * step;
  * regions not longer than 1e-6 do not exist;
  * min_duration_off > 0: neighbours are merged when the gap's duration (0 when not longer than 1e-6) is smaller;
    the merged regions are numbered in time order (their track names); otherwise every region has number 0;
  * min_duration_on > 0: regions whose duration is smaller are removed (numbers stay);
  * fewer than two frames: nothing.

`triples` lists what the pipeline's Annotation must iterate as: (start, end, track name, class name)."""
import itertools
import string

import numpy as np

PRECISION = 1e-6


def track_name(position: int) -> str:
    """A..Z, AA..ZZ, AAA.. -- the generated track names, by position"""
    length, block = 1, 26
    while position >= block:
        position -= block
        length += 1
        block = 26 ** length
    letters = []
    for _ in range(length):
        letters.append(string.ascii_uppercase[position % 26])
        position //= 26
    return "".join(reversed(letters))


def frame_middle(i: int, start: float, duration: float, step: float) -> float:
    s = float(start) + i * float(step)
    return 0.5 * (s + (s + float(duration)))


def class_regions(y, start, duration, step, onset, offset, min_duration_on=0.0, min_duration_off=0.0):
    """one class: y (T,) float32 -> ([(start, end)], [track position])"""
    y = np.asarray(y, dtype=np.float32)
    T = len(y)
    if T < 2:
        return [], []
    on_threshold, off_threshold = np.float32(onset), np.float32(offset)
    regions = []
    active = bool(y[0] > on_threshold)
    opened = frame_middle(0, start, duration, step)
    for i in range(1, T):
        if active:
            if y[i] < off_threshold:
                regions.append((opened, frame_middle(i, start, duration, step)))
                active = False
        elif y[i] > on_threshold:
            opened = frame_middle(i, start, duration, step)
            active = True
    if active:
        regions.append((opened, frame_middle(T - 1, start, duration, step)))
    regions = [(a, b) for a, b in regions if (b - a) > PRECISION]
    positions = [0] * len(regions)
    if min_duration_off > 0.0:
        merged = []
        for a, b in regions:
            if merged:
                gap = a - merged[-1][1]
                gap = gap if gap > PRECISION else 0.0
                if gap < min_duration_off:
                    merged[-1] = (merged[-1][0], b)
                    continue
            merged.append((a, b))
        regions = merged
        positions = list(range(len(regions)))
    if min_duration_on > 0.0:
        kept = [n for n, (a, b) in enumerate(regions) if not ((b - a if (b - a) > PRECISION else 0.0) < min_duration_on)]
        regions = [regions[n] for n in kept]
        positions = [positions[n] for n in kept]
    return regions, positions


def all_regions(scores, start, duration, step, onset, offset, min_duration_on, min_duration_off):
    """scores (T, K) -> per class ([(start, end)], [track position]); scalars are shared between classes"""
    scores = np.asarray(scores, dtype=np.float32)
    K = scores.shape[1]
    spread = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (K,))
    onset, offset, d_on, d_off = spread(onset), spread(offset), spread(min_duration_on), spread(min_duration_off)
    return [class_regions(scores[:, k], start, duration, step, onset[k], offset[k], d_on[k], d_off[k])
            for k in range(K)]


def triples(per_class, class_names):
    """(start, end, track, label) in the order an Annotation iterates: classes are added one after the other, a later
    class overwrites an earlier one on the same (segment, track); segments by (start, end), tracks by name"""
    table = {}
    for (regions, positions), label in zip(per_class, class_names):
        for (a, b), position in zip(regions, positions):
            table[(a, b, track_name(position))] = label
    return sorted(((a, b, t, l) for (a, b, t), l in table.items()), key=lambda r: (r[0], r[1], str(r[2]), str(r[3])))


def annotation_rows(annotation):
    return [(s.start, s.end, t, l) for s, t, l in annotation.itertracks(yield_label=True)]


def smooth_scores(rng, T, K, width=25, nan_fraction=0.0):
    """random scores in (0, 1) that wander slowly enough to make regions of many frames"""
    x = rng.standard_normal((T + width, K))
    kernel = np.ones(width) / np.sqrt(width)
    y = np.stack([np.convolve(x[:, k], kernel, mode="valid")[:T] for k in range(K)], axis=1)
    y = (1.0 / (1.0 + np.exp(-1.5 * y))).astype(np.float32)
    if nan_fraction >= 1.0:
        y[:] = np.nan
    elif nan_fraction > 0.0:
        y[rng.random((T, K)) < nan_fraction] = np.nan
    return y


assert [track_name(n) for n in (0, 25, 26, 27, 701, 702)] == \
    [n for i, n in enumerate(map("".join, itertools.chain(
        itertools.product(string.ascii_uppercase, repeat=1), itertools.product(string.ascii_uppercase, repeat=2),
        itertools.product(string.ascii_uppercase, repeat=3)))) if i in (0, 25, 26, 27, 701, 702)]
