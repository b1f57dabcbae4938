"""Cases and truths shared by the tests of the windowed error counts (`pa_annot_window_counts`,
`annotation_metrics.window_counts`): tests/test_window_counts_gpu.py and tests/test_sliding_der_cpu.py.

The truth of window w is `annotation_metrics_truth.truth_counts(ref, hyp, uem clipped to the window, ...)`: the exact
rational computation of the one-file counts, untouched; the clipping of the uem rows is `clip` below.  A case is a
dict of the truth module plus "windows": [(start, end)]."""
import functools
import random

import numpy as np

import annotation_metrics_truth as truth

TILE = 256            # threads per workgroup, LDS tile of the rank sort and of the sweep, stride of the reduction


def clip(uem, start, end) -> list:
    """the uem rows inside [start, end]; rows left without length are dropped (they evaluate nothing)"""
    rows = [(max(a, start), min(b, end)) for a, b in uem]
    return [(a, b) for a, b in rows if a < b]


def window_truths(case: dict) -> list:
    """per window the dict of `truth_counts`"""
    return [truth.truth_counts(case["ref"], case["hyp"], clip(case["uem"], a, b), case["Kr"], case["Kh"],
                               collar=case["collar"], skip_overlap=case["skip_overlap"]) for a, b in case["windows"]]


def assert_dyadic(case: dict):
    """`annotation_metrics_truth.assert_dyadic`, and the window boundaries on the same grid: the extra cuts split
    intervals into pieces that are again whole multiples of GRID, so every sum stays exact"""
    truth.assert_dyadic(case)
    for a, b in case["windows"]:
        assert truth.is_dyadic(a) and truth.is_dyadic(b) and a <= b


def total_cuts(case: dict) -> int:
    """the cuts the device sorts: the file's, and two per window"""
    Nr, Nh, Nu, W = len(case["ref"]), len(case["hyp"]), len(case["uem"]), len(case["windows"])
    return 2 * (Nr + Nh + Nu + W) + (4 * Nr if case["collar"] else 0)


def rank_ranges(case: dict) -> list:
    """per window (a, b): the ranks of its start and end cut, by the documented layout of the cut list ([ref start]
    [ref end][hyp start][hyp end][uem start][uem end][collar lo][collar hi][window start][window end]) and the
    documented order (by value, equal values by position): the window reduces the intervals a <= k < b"""
    half = case["collar"] / 2
    ref, hyp, uem, win = case["ref"], case["hyp"], case["uem"], case["windows"]
    cuts = [r[0] for r in ref] + [r[1] for r in ref] + [h[0] for h in hyp] + [h[1] for h in hyp] + \
        [u[0] for u in uem] + [u[1] for u in uem]
    if case["collar"]:
        bounds = [r[0] for r in ref] + [r[1] for r in ref]
        cuts += [t - half for t in bounds] + [t + half for t in bounds]
    first = len(cuts)
    cuts += [w[0] for w in win] + [w[1] for w in win]
    assert len(cuts) == total_cuts(case)
    rank = {i: r for r, i in enumerate(sorted(range(len(cuts)), key=lambda i: (cuts[i], i)))}
    return [(rank[first + w], rank[first + len(win) + w]) for w in range(len(win))]


def with_windows(case: dict, windows) -> dict:
    return dict(case, windows=[(float(a), float(b)) for a, b in windows])


def random_windows(seed: int, W: int, span: float = 64.0, longest: float = 16.0) -> list:
    """W windows on the GRID inside [0.5, 1.5 + span] (the generator's segments lie in [1, 1 + span]), unsorted,
    overlapping, some of zero length"""
    rng = random.Random(seed)
    ticks = int((span + 1.0) / truth.GRID)
    out = []
    for _ in range(W):
        a = rng.randrange(0, ticks)
        b = min(ticks, a + rng.randrange(0, int(longest / truth.GRID) + 1))
        out.append((0.5 + a * truth.GRID, 0.5 + b * truth.GRID))
    return out


# the file of test_annotation_metrics_gpu.test_hand_built_edges: touching segments, shared boundaries, a uem of several
# regions, same-label overlap, zero-length segments
HAND_REF = [(2.0, 4.0, 0), (4.0, 6.0, 0), (4.0, 8.0, 1), (8.0, 8.25, 2), (8.25, 8.5, 2), (20.0, 22.0, 1),
            (3.0, 5.0, 0), (7.0, 7.0, 2)]
HAND_HYP = [(2.0, 4.0, 1), (4.0, 9.0, 0), (6.0, 8.0, 1), (20.0, 22.0, 0), (30.0, 31.0, 1), (8.5, 8.5, 0)]
HAND_UEM = [(2.0, 5.0), (4.5, 7.0), (7.5, 8.5), (12.0, 12.0), (21.0, 40.0)]
HAND_WINDOWS = [
    (2.0, 4.0), (4.0, 8.25),          # edges on segment boundaries
    (4.5, 7.0), (5.0, 7.5),           # on uem boundaries: a region's own, the end of one and the start of the next
    (1.75, 2.25), (3.875, 8.125),     # on the collar boundaries of collar 0.5 (2 -/+ 0.25) and 0.25 (4 - 0.125, 8 + 0.125)
    (0.0, 4.0), (2.0, 6.0), (4.0, 8.0), (6.0, 10.0), (8.0, 12.0),   # sliding: the end of w is the start of w + 2
    (9.0, 11.5),                      # outside the uem: all zeros
    (6.0, 8.0), (3.0, 30.0),          # across two uem regions; across all of them
    (5.0, 5.0), (12.0, 12.0),         # zero length
    (0.0, 64.0),                      # the whole file
]
HAND_ZERO_ROWS = (11, 14, 15)         # windows of HAND_WINDOWS that evaluate nothing


def hand_case(collar=0.0, skip_overlap=False, windows=HAND_WINDOWS) -> dict:
    return {"ref": HAND_REF, "hyp": HAND_HYP, "uem": HAND_UEM, "Kr": 3, "Kh": 2, "collar": collar,
            "skip_overlap": skip_overlap, "windows": list(windows)}


# the sizes at which the kernels change shape (256 threads per workgroup, LDS tiles of 256 cuts in the rank sort), the
# cuts counted WITH the two of every window: name, Nr, Nh, Nu, W, collar
SHAPES = [
    ("254 cuts: one workgroup, one tile, two cuts short", 60, 55, 4, 8, 0.0),
    ("256 cuts: exactly one workgroup and one tile; 255 intervals", 60, 55, 4, 9, 0.0),
    ("258 cuts: a second workgroup and a second tile of two; 257 intervals", 60, 55, 4, 10, 0.0),
    ("254 cuts with collars", 30, 30, 4, 3, 0.25),
    ("256 cuts with collars", 30, 30, 4, 4, 0.25),
    ("258 cuts with collars", 30, 30, 4, 5, 0.25),
    ("510 cuts", 120, 120, 5, 10, 0.0),
    ("512 cuts: two full cut tiles", 120, 120, 5, 11, 0.0),
    ("514 cuts", 120, 120, 5, 12, 0.0),
    ("510 cuts with collars", 60, 64, 5, 6, 0.25),
    ("512 cuts with collars", 60, 64, 5, 7, 0.25),
    ("514 cuts with collars", 60, 64, 5, 8, 0.25),
    ("792 cuts: four workgroups, more windows than segments on a side", 130, 120, 6, 140, 0.0),
    ("852 cuts with collars: four workgroups", 100, 100, 6, 20, 0.25),
]


def shape_case(name, Nr, Nh, Nu, W, collar, skip) -> dict:
    """the random dyadic case of a row of SHAPES; asserts the cut count its name states"""
    case = truth.random_dyadic_case(len(name) + Nu, Nr, Nh, Nu, Kr=4, Kh=5, collar=collar, skip_overlap=skip, span=32.0)
    case = with_windows(case, random_windows(W, W, span=32.0, longest=4.0))
    cuts = total_cuts(case)
    assert cuts == 2 * (Nr + Nh + Nu + W) + (4 * Nr if collar else 0)
    assert cuts == int(name.split()[0])
    assert abs(cuts - TILE) <= 2 or abs(cuts - 2 * TILE) <= 2 or cuts > 3 * TILE
    return case


def labels64_case() -> dict:
    """64 labels a side; label 63 of both sides is on inside window 1 only (and the reference's in window 4)"""
    case = truth.random_dyadic_case(3, Nr=150, Nh=140, Nu=3, Kr=63, Kh=63, collar=0.125, span=16.0)
    case = dict(case, Kr=64, Kh=64)
    case["ref"] = [r for r in case["ref"] if r[1] <= 2.0 or r[0] >= 4.0] + [(2.0, 3.0, l) for l in range(64)]
    case["hyp"] = [h for h in case["hyp"] if h[1] <= 2.0 or h[0] >= 4.0] + [(2.5, 3.5, l) for l in range(64)]
    case["uem"] = case["uem"] + [(1.0, 4.0)]
    return with_windows(case, [(0.5, 2.0), (1.5, 4.0), (4.0, 9.0), (3.5, 17.0), (2.0, 2.5)])


def range_case(n: int) -> dict:
    """one window (8, 40) whose rank range holds exactly n >= 1 intervals, all of non-zero length: n - 1 distinct
    cuts strictly inside it (segment starts; the ends lie behind the window, distinct too), no cut tied with its
    edges; one more turn a side covers the whole window"""
    inside = n - 1
    ref = [(8.0 + (2 * i + 1) * 16 * truth.GRID, 41.0 + i * truth.GRID, i % 3) for i in range((inside + 1) // 2)]
    hyp = [(8.0 + (2 * i + 2) * 16 * truth.GRID, 45.0 + i * truth.GRID, i % 2) for i in range(inside // 2)]
    assert len(ref) + len(hyp) == inside and 8.0 + (inside + 1) * 16 * truth.GRID < 40.0
    return {"ref": ref + [(6.0, 60.0, 2)], "hyp": hyp + [(5.0, 61.0, 1)], "uem": [(7.0, 50.0)], "Kr": 3, "Kh": 2,
            "collar": 0.0, "skip_overlap": False, "windows": [(8.0, 40.0)]}


@functools.lru_cache(maxsize=None)
def non_dyadic(collar=0.0, skip=False):
    """The file of test_annotation_metrics_gpu._non_dyadic (uniform random float64 boundaries, 300 segments per side,
    8 labels; with a collar the boundaries lie in [16, 31.5), where t -/+ collar / 2 is exact) and 40 windows of
    irregular length with uniform random float64 boundaries.  -> (case, per-window truths, the file's elementary
    intervals n)"""
    rng = np.random.default_rng(7)
    lo, hi = (16.0, 31.5) if collar else (0.0, 3600.0)

    def side():
        a = rng.uniform(lo, hi, 300)
        b = np.minimum(a + rng.uniform(0.0, (hi - lo) / (400.0 if collar else 40.0), 300), np.nextafter(hi, 0.0))
        return [(float(x), float(y), int(l)) for x, y, l in zip(a, b, rng.integers(0, 8, 300))]

    ref, hyp = side(), side()
    uem = [(lo + (hi - lo) * 0.01, lo + (hi - lo) * 0.6), (lo + (hi - lo) * 0.7, hi)]
    start = rng.uniform(lo, lo + (hi - lo) * 0.95, 40)
    length = rng.uniform((hi - lo) / 400.0, (hi - lo) / 20.0, 40)
    windows = [(float(a), float(min(a + l, hi))) for a, l in zip(start, length)]
    windows[3] = (lo + (hi - lo) * 0.55, lo + (hi - lo) * 0.75)          # across the gap of the uem
    case = {"ref": ref, "hyp": hyp, "uem": uem, "Kr": 8, "Kh": 8, "collar": collar, "skip_overlap": skip,
            "windows": windows}
    n = truth.truth_counts(ref, hyp, uem, 8, 8, collar=collar, skip_overlap=skip)["intervals"]
    return case, window_truths(case), n


def check_within_bound(rows, case, truths, n) -> float:
    """Every field of every window within n * 2^-52 * truth, n = the file's elementary intervals: the derivation of
    test_annotation_metrics_gpu.test_non_dyadic_within_the_derived_bound.  A window's sum has at most n + 2 W terms
    (the window boundaries, inputs like the others, split intervals further), each with a relative error below
    2 * 2^-53, and at most as many roundings of partial sums that never exceed the rounded total: altogether
    (n + 2 W + 1) * 2^-53 * truth * (1 + tiny) <= n * 2^-52 * truth because 2 W + 2 <= n.  -> the worst
    |got - truth| / truth."""
    from fractions import Fraction
    assert 2 * len(case["windows"]) + 2 <= n
    worst = Fraction(0)
    for row, want in zip(rows, truths):
        for got, t in zip(row, truth.flat(want)):
            bound = n * Fraction(1, 2 ** 52) * t
            error = abs(Fraction(float(got)) - t)
            assert error <= bound, (float(got), float(t), float(error), float(bound))
            if t:
                worst = max(worst, error / t)
    return float(worst)


# ------------------------------------------------------------------------------------------ a file for sliding windows
def conversation(seed: int, speakers: int, turns: int = 200, span: float = 256.0):
    """A dyadic synthetic file: `turns` reference turns of `speakers` speakers on the GRID inside [1, 1 + span]; the
    hypothesis is the reference with every boundary moved by up to a quarter of a second, one turn in ten dropped, as
    many invented, its speakers renamed and one turn in eight given to the wrong one; a uem of two regions.
    -> (reference rows, hypothesis rows, uem rows), rows (start, end, label name)"""
    rng = random.Random(seed)
    tick = truth.GRID
    ticks = int(span / tick)

    def turn():
        a = rng.randrange(0, ticks - 1)
        return a, min(ticks, a + rng.randrange(int(0.5 / tick), int(4.0 / tick)))

    ref = [turn() + (rng.randrange(speakers),) for _ in range(turns)]
    hyp = []
    for a, b, s in ref:
        if rng.random() < 0.1:
            a, b = turn()
        a, b = max(0, a + rng.randrange(-256, 257)), min(ticks, b + rng.randrange(-256, 257))
        if b <= a:
            continue
        hyp.append((a, b, (s + 1) % speakers if rng.random() > 0.125 else rng.randrange(speakers)))
    seconds = lambda rows, name: [(1.0 + a * tick, 1.0 + b * tick, f"{name}{s}") for a, b, s in rows]  # noqa: E731
    uem = [(2.0, 1.0 + span * 0.4375), (1.0 + span * 0.5 + 3 * tick, span - 1.0)]
    case = {"ref": seconds(ref, "r"), "hyp": seconds(hyp, "h"), "uem": uem, "collar": 0.0}
    truth.assert_dyadic(case)
    return case["ref"], case["hyp"], uem


def literal_loop(am, reference, hypothesis, uem, window: float):
    """the loop of the reference's SlidingDiarizationErrorRate.compute_components (utils/metric.py:258-279), with the
    package's `DiarizationErrorRate` on cropped annotations -> (the accumulated components, the windows, the
    per-window components)"""
    from pyannote_audio_amd.core import SlidingWindow
    from pyannote_audio_amd.metrics import Timeline
    der = am.DiarizationErrorRate()
    chunks, rows = [], []
    for chunk in SlidingWindow(duration=window, step=0.5 * window)(uem):
        rows.append(der(reference.crop(chunk), hypothesis.crop(chunk), uem=Timeline([chunk]), detailed=True))
        chunks.append(chunk)
    return der[:], chunks, rows


def check_sliding(am, speakers: int, device=None, window: float = 8.0):
    """`SlidingDiarizationErrorRate(device=device)` on a `conversation` equals the literal loop with `==`: all
    boundaries, the windows' included (uem starts and multiples of window / 2 on the GRID), are dyadic, so every sum
    on either route is exact"""
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.core import Segment
    from pyannote_audio_amd.metrics import Timeline
    ref_rows, hyp_rows, uem_rows = conversation(speakers, speakers)

    def annotation(rows):
        a = pa.Annotation()
        for n, (start, end, label) in enumerate(rows):
            a[Segment(start, end), n] = label
        return a

    reference, hypothesis = annotation(ref_rows), annotation(hyp_rows)
    assert len(reference.labels()) == speakers and len(hypothesis.labels()) == speakers
    uem = Timeline([Segment(a, b) for a, b in uem_rows])
    want, chunks, rows = literal_loop(am, reference, hypothesis, uem, window)
    assert len(chunks) > 40 and all(truth.is_dyadic(c.start) and truth.is_dyadic(c.end) for c in chunks)
    assert want["confusion"] > 0 and want["false alarm"] > 0 and want["missed detection"] > 0
    metric = am.SlidingDiarizationErrorRate(window=window, device=device)
    detail = metric(reference, hypothesis, uem=uem, detailed=True)
    name = "window diarization error rate"
    assert {k: v for k, v in detail.items() if k != name} == want
    assert detail[name] == (want["false alarm"] + want["missed detection"] + want["confusion"]) / want["total"]
    assert metric[:] == {k: want[k] for k in metric.metric_components()} and abs(metric) == detail[name]
    table = metric.windows(reference, hypothesis, uem=uem)
    assert table["windows"] == chunks
    for key in ("total", "correct", "false alarm", "missed detection", "confusion", "diarization error rate"):
        assert table[key].tolist() == [row[key] for row in rows], key
    assert len({row["diarization error rate"] for row in rows}) > 10          # (the windows differ)
