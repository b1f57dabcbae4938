"""Exact truth of the time-based error counts (`pa_annot_counts`, `annotation_metrics.annotation_counts`): a brute
force in rational arithmetic that shares no code with the package.

Every float is taken as the rational it is (`fractions.Fraction(float)` is exact).  The time axis is cut at every
segment, uem and collar boundary; inside an elementary interval nothing changes, so everything is decided at its
MIDPOINT by plain membership tests: a label is on when a segment of that label contains the midpoint, the interval is
evaluated when a uem segment contains it, no collar (t - collar/2, t + collar/2) around a reference boundary does,
and, with `skip_overlap`, fewer than two distinct reference labels are on.  The sums are exact.

(All boundaries are floats, so their denominators are powers of two: the helper scales everything to Python integers
by the largest denominator first, which is the same arithmetic as Fractions, only faster.)"""
from __future__ import annotations

import random
from fractions import Fraction

SCALARS = ("total", "false_alarm", "missed", "both", "ref_speech", "hyp_speech", "both_speech")


def truth_counts(ref, hyp, uem, Kr, Kh, collar=0.0, skip_overlap=False) -> dict:
    """ref, hyp: [(start, end, label index)], uem: [(start, end)], floats in any order.
    -> Fractions: `cooc` [Kr][Kh], `ref_dur` [Kr], `hyp_dur` [Kh], the seven SCALARS, and the int `intervals`
    (elementary intervals of non-zero length)."""
    half = Fraction(collar) / 2
    fr = lambda x: Fraction(x)  # noqa: E731
    R = [(fr(a), fr(b), int(l)) for a, b, l in ref]
    H = [(fr(a), fr(b), int(l)) for a, b, l in hyp]
    U = [(fr(a), fr(b)) for a, b in uem]
    C = [(t - half, t + half) for a, b, _ in R for t in (a, b)] if collar > 0 else []
    values = [v for a, b, _ in R + H for v in (a, b)] + [v for pair in U + C for v in pair]
    scale = max([v.denominator for v in values] + [1])
    # doubled integer coordinates: boundaries are even, midpoints are whole
    z = lambda v: int(v * scale) * 2  # noqa: E731
    assert all((v * scale).denominator == 1 for v in values)
    R = [(z(a), z(b), l) for a, b, l in R]
    H = [(z(a), z(b), l) for a, b, l in H]
    U = [(z(a), z(b)) for a, b in U]
    C = [(z(a), z(b)) for a, b in C]
    cuts = sorted({v for a, b, _ in R + H for v in (a, b)} | {v for pair in U + C for v in pair})

    cooc = [[0] * Kh for _ in range(Kr)]
    ref_dur, hyp_dur = [0] * Kr, [0] * Kh
    scalars = dict.fromkeys(SCALARS, 0)
    for a, b in zip(cuts[:-1], cuts[1:]):
        m = (a + b) // 2
        if not any(s < m < e for s, e in U):
            continue
        if any(s < m < e for s, e in C):
            continue
        on_r = sorted({l for s, e, l in R if s < m < e})
        if skip_overlap and len(on_r) >= 2:
            continue
        on_h = sorted({l for s, e, l in H if s < m < e})
        d, nr, nh = b - a, len(on_r), len(on_h)
        for i in on_r:
            ref_dur[i] += d
            for j in on_h:
                cooc[i][j] += d
        for j in on_h:
            hyp_dur[j] += d
        scalars["total"] += nr * d
        scalars["false_alarm"] += max(0, nh - nr) * d
        scalars["missed"] += max(0, nr - nh) * d
        scalars["both"] += min(nr, nh) * d
        scalars["ref_speech"] += d if nr else 0
        scalars["hyp_speech"] += d if nh else 0
        scalars["both_speech"] += d if nr and nh else 0
    q = lambda v: Fraction(v, 2 * scale)  # noqa: E731
    out = {"cooc": [[q(v) for v in row] for row in cooc], "ref_dur": [q(v) for v in ref_dur],
           "hyp_dur": [q(v) for v in hyp_dur], "intervals": max(len(cuts) - 1, 0)}
    out.update({name: q(v) for name, v in scalars.items()})
    return out


def flat(truth: dict) -> list:
    """the Fractions in the order of the kernel's output: cooc row-major, ref_dur, hyp_dur, the scalars"""
    return [v for row in truth["cooc"] for v in row] + truth["ref_dur"] + truth["hyp_dur"] + \
        [truth[name] for name in SCALARS]


def rows_of(annotation) -> tuple:
    """(labels, [(start, end, label index)]) of an Annotation, labels indexed in `labels()` order"""
    labels = annotation.labels()
    index = {label: i for i, label in enumerate(labels)}
    return labels, [(s.start, s.end, index[l]) for s, _, l in annotation.itertracks(yield_label=True)]


# ------------------------------------------------------------------------------------------------ generators
GRID = 2.0 ** -10         # dyadic cases: every boundary is an integer multiple of this, below LIMIT seconds
LIMIT = 4096.0


def is_dyadic(x: float) -> bool:
    return 0.0 <= x < LIMIT and (x / GRID) == int(x / GRID)


def assert_dyadic(case: dict):
    """every boundary of the case, and every collar boundary, is a multiple of GRID in [0, LIMIT): then every
    product (labels on) * (length) is an integer < 2^6 * 2^22 multiples of GRID and every partial sum of at most
    2^20 of them stays below 2^53 multiples: exactly representable in float64 whatever the order of addition"""
    half = case["collar"] / 2
    assert half == 0 or (half / GRID) == int(half / GRID)
    for a, b, _ in case["ref"] + case["hyp"]:
        assert is_dyadic(a) and is_dyadic(b) and a <= b
    for a, b in case["uem"]:
        assert is_dyadic(a) and is_dyadic(b) and a <= b
    for a, b, _ in case["ref"]:
        for t in (a, b):
            assert t - half >= -LIMIT and t + half < 2 * LIMIT and ((t - half) / GRID) == int((t - half) / GRID)


def random_dyadic_case(seed: int, Nr: int, Nh: int, Nu: int, Kr: int, Kh: int, collar: float = 0.0,
                       skip_overlap: bool = False, span: float = 64.0, longest: float = 4.0,
                       shortest_ticks: int = 0) -> dict:
    """segments on the GRID inside [1, 1 + span], in shuffled (unsorted) order; labels cover 0..K-1 when there are
    enough segments.  `shortest_ticks=1` keeps zero-length segments out (an `Annotation` drops them on insertion)"""
    rng = random.Random(seed)
    ticks = int(span / GRID)

    def segment(longest_ticks):
        a = rng.randrange(0, ticks - 1)
        b = min(ticks, a + rng.randrange(shortest_ticks, longest_ticks + 1))   # zero-length segments happen
        return 1.0 + a * GRID, 1.0 + b * GRID

    def side(N, K):
        rows = [segment(int(longest / GRID)) + ((n % K) if n < K else rng.randrange(K),) for n in range(N)]
        rng.shuffle(rows)
        return rows

    case = {"ref": side(Nr, max(Kr, 1)) if Kr else [], "hyp": side(Nh, max(Kh, 1)) if Kh else [],
            "uem": [segment(int(span / 2 / GRID)) for _ in range(Nu)], "Kr": Kr, "Kh": Kh, "collar": collar,
            "skip_overlap": skip_overlap}
    assert len(case["ref"]) == (Nr if Kr else 0) and len(case["hyp"]) == (Nh if Kh else 0)
    assert_dyadic(case)
    return case


def case_truth(case: dict) -> dict:
    return truth_counts(case["ref"], case["hyp"], case["uem"], case["Kr"], case["Kh"], collar=case["collar"],
                        skip_overlap=case["skip_overlap"])
