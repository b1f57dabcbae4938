"""Truths and inputs of the corpus evaluation tests (tests/test_evaluation_cpu.py, tests/test_corpus_counts_gpu.py):
restatements that share no code with the package (only the builders at the end make the package's objects).

* `support_rows`: the gap-filling rule of `Annotation.support` on plain (start, end, label) rows, in the number type
  of the caller (`float`: the operations the package and the kernel do; `Fraction`: exact -- on the dyadic grid of
  `annotation_metrics_truth` both agree because every difference is exact).
* `jaccard_truth`: the Jaccard error rate from the exact counts of `annotation_metrics_truth.truth_counts`, with the
  speaker mapping found by trying every assignment.
* the corpora and the support edge cases the CPU and the GPU tests share."""
from __future__ import annotations

import itertools
import random
from fractions import Fraction

import annotation_metrics_truth as truth

GRID = truth.GRID
PRECISION = 1e-6


# ------------------------------------------------------------------------------------------------- support
def support_rows(rows, fill, num=float) -> list:
    """rows [(start, end, label)] in any order -> the rows of `support(fill)`: per label, rows sorted by
    (start, end); the current turn (a, E) takes in the next row (c, d) when they overlap by more than PRECISION or
    the gap between them -- 0 when it is not more than PRECISION -- is < fill; a turn that is not longer than
    PRECISION is no segment and is not kept."""
    precision, fill = num(PRECISION), num(fill)
    out = []
    for label in sorted({l for _, _, l in rows}, key=str):
        turns = sorted((num(a), num(b)) for a, b, l in rows if l == label)
        (a, E), rest = turns[0], turns[1:]
        for c, d in rest:
            lo = min(E, d)
            overlap, gap = lo - c, c - lo
            if not gap > precision:
                gap = num(0)
            if overlap > precision or gap < fill:
                E = max(E, d)
            else:
                if E - a > precision:
                    out.append((a, E, label))
                a, E = c, d
        if E - a > precision:
            out.append((a, E, label))
    return out


FILL = 0.25          # the fill the edge cases are written for (a multiple of GRID)

#: name -> (hypothesis rows of ONE label, {fill: number of turns after support(fill)})
SUPPORT_EDGES = {
    "gap equal to fill": ([(1.0, 2.0), (2.0 + FILL, 3.0)], {FILL: 2, FILL + GRID: 1}),
    "gap one step below fill": ([(1.0, 2.0), (2.0 + FILL - GRID, 3.0)], {FILL: 1, FILL - GRID: 2}),
    "gap one step above fill": ([(1.0, 2.0), (2.0 + FILL + GRID, 3.0)], {FILL: 2, 0.0: 2}),
    "touching": ([(1.0, 2.0), (2.0, 3.0)], {0.0: 2, GRID: 1, FILL: 1}),
    "nested": ([(1.0, 5.0), (2.0, 3.0), (5.0 + GRID, 6.0)], {0.0: 2, FILL: 1}),
    # the turn that starts at 1 reaches 10: the last row is 0.125 from ITS end, not 5.125 from the previous row's
    "running maximum": ([(1.0, 10.0), (2.0, 3.0), (4.0, 5.0), (10.125, 11.0)], {0.0: 2, GRID: 2, FILL: 1}),
    "overlapping tracks": ([(1.0, 3.0), (1.0, 3.0), (2.0, 4.0), (3.5, 3.75), (8.0, 9.0)], {0.0: 2, FILL: 2, 4.5: 1}),
    # after a break the running maximum starts again: (6, 7) is compared with (5.5, 5.75), not with the end 5 of the
    # first turn or any earlier maximum
    "maximum of the run": ([(1.0, 5.0), (5.5, 5.75), (6.0, 7.0)], {0.0: 3, FILL: 3, 0.5: 2, 0.5 + GRID: 1}),
}

#: off the grid: a row no longer than PRECISION inside a longer turn.  It does not overlap the turn by MORE than
#: PRECISION and the gap is 0: with fill = 0 it ends the turn it lies in, (3, 6) is then compared with the short row
#: and starts a third turn, and the short row itself is no segment: 2 turns.  Any fill > 0 merges all three.
SHORT_ROW_INSIDE = ([(1.0, 5.0), (2.0, 2.0 + 5e-7), (3.0, 6.0)], {0.0: 2, FILL: 1})


# ------------------------------------------------------------------------------------------------- jaccard
def jaccard_truth(ref, hyp, uem, Kr, Kh, collar=0.0, skip_overlap=False) -> tuple:
    """-> (speaker count, [error of every counted reference label, a Fraction, in label order]).  The mapping is the
    one-to-one assignment of hypothesis to reference labels with the largest matched duration, pairs without common
    time left out; found by trying every assignment (small K only), and it must be the only best one."""
    t = truth.truth_counts(ref, hyp, uem, Kr, Kh, collar=collar, skip_overlap=skip_overlap)
    cooc, ref_dur, hyp_dur = t["cooc"], t["ref_dur"], t["hyp_dur"]
    assert Kr <= 6 and Kh <= 6
    columns = list(range(Kh)) + [None] * Kr                  # None: the reference label stays unmapped
    best, best_value, ties = None, -1, 0
    for choice in set(itertools.permutations(columns, Kr)):
        value = sum(cooc[i][j] for i, j in enumerate(choice) if j is not None)
        pairs = {i: j for i, j in enumerate(choice) if j is not None and cooc[i][j] > 0}
        if value > best_value:
            best, best_value, ties = pairs, value, 0
        elif value == best_value and pairs != best:
            ties += 1
    assert ties == 0, "the case has several best mappings: the truth is not unique"
    errors = []
    for i in range(Kr):
        if ref_dur[i] == 0:
            continue
        if i not in best:
            errors.append(Fraction(1))
            continue
        j = best[i]
        errors.append((hyp_dur[j] + ref_dur[i] - 2 * cooc[i][j]) / (ref_dur[i] + hyp_dur[j] - cooc[i][j]))
    return len(errors), errors


def float_sum(fractions) -> float:
    """the floats nearest to the Fractions, added in order (a quotient of two exact floats IS the float nearest to
    the exact quotient, so this is what a float64 computation of the same terms gives)"""
    total = 0.0
    for value in fractions:
        total += float(value)
    return total


# ------------------------------------------------------------------------------------------------- corpora
def split_gap_turns(seed: int, turns: int = 12, speakers: int = 2, gap: float = 0.25) -> tuple:
    """-> (reference rows, hypothesis rows) on the grid: the hypothesis is the reference with every turn split in
    two by a `gap`, and speaker names of its own.  Filling gaps of `gap` removes all missed detection."""
    rng = random.Random(seed)
    ref, hyp, t = [], [], 1.0
    for n in range(turns):
        length = 2.0 + rng.randrange(0, 2048) * GRID
        cut = 0.5 + rng.randrange(0, 512) * GRID
        s = n % speakers
        ref.append((t, t + length, f"spk{s}"))
        hyp += [(t, t + cut, f"h{s}"), (t + cut + gap, t + length, f"h{s}")]
        t += length + 1.0 + rng.randrange(0, 1024) * GRID
    return ref, hyp


def zero_wins_turns(seed: int, turns: int = 10) -> tuple:
    """the hypothesis has two turns of one speaker where the reference has silence between them (0.125 to 0.5 s):
    filling any gap only adds false alarm, so min_duration_off = 0 is best"""
    rng = random.Random(seed)
    ref, hyp, t = [], [], 1.0
    for n in range(turns):
        a = 1.0 + rng.randrange(0, 1024) * GRID
        silence = 0.125 + rng.randrange(0, 384) * GRID
        b = 1.0 + rng.randrange(0, 1024) * GRID
        for rows, names in ((ref, "spk"), (hyp, "h")):
            rows += [(t, t + a, f"{names}{n % 2}"), (t + a + silence, t + a + silence + b, f"{names}{n % 2}")]
        t += a + silence + b + 2.0
    return ref, hyp


def random_rows(rng, n: int, labels: list, span: float, dyadic: bool) -> list:
    rows = []
    for _ in range(n):
        if dyadic:
            a = 1.0 + rng.randrange(0, int(span / GRID)) * GRID
            b = a + rng.randrange(1, int(3.0 / GRID)) * GRID
        else:
            a = 1.0 + rng.uniform(0.0, span)
            b = a + rng.uniform(0.01, 3.0)
        rows.append((a, b, rng.choice(labels)))
    return rows


# ------------------------------------------------------------------------------------------------ builders
def annotation(rows, uri=None):
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.core import Segment
    out = pa.Annotation(uri=uri)
    for track, (a, b, label) in enumerate(rows):
        out[Segment(a, b), track] = label
    return out


def timeline(pairs):
    from pyannote_audio_amd.core import Segment
    from pyannote_audio_amd.metrics import Timeline
    return Timeline([Segment(a, b) for a, b in pairs])


def indexed(rows):
    """[(start, end, name)] -> (K, [(start, end, index in sorted-name order)]): the labels as `labels()` orders them"""
    names = sorted({l for _, _, l in rows}, key=str)
    return len(names), [(a, b, names.index(l)) for a, b, l in rows]


def bare_annotation(rows):
    """an Annotation holding `rows` as they are, rows too short to be segments included (`annotation[segment] =`
    would drop them): what `support` does with such a row is part of the rule"""
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.core import Segment
    out = pa.Annotation()
    for track, (a, b, label) in enumerate(rows):
        out._tracks.setdefault(Segment(a, b), {})[track] = label
    return out


def corpus_files(maker, seeds=(0, 1, 2), uem=True):
    files = []
    for seed in seeds:
        ref, hyp = maker(seed)
        file = {"uri": f"file{seed}", "annotation": annotation(ref, uri=f"file{seed}"),
                "speaker_diarization": annotation(hyp, uri=f"file{seed}"), "duration": 120.0}
        if uem:
            file["annotated"] = timeline([(0.0, 120.0)])
        files.append(file)
    return files
