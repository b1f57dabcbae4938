"""Plain-numpy truth of `pyannote_audio_amd.verification`: the detection-error-tradeoff curve and its equal error
rate in int64 counts and float64 quotients, written from the steps of sklearn.metrics.roc_curve
(drop_intermediate=True) and det_curve without calling either, plus the seeded cases that the CPU tests, the GPU
tests and tests/golden/make_verification_golden.py share."""
import numpy as np

#: elements per workgroup of the curve kernels and workgroup sums per scan chunk (csrc/verification.hip)
B = 1024
CHUNK = 1024


def det_curve_truth(y_true, scores, distances=False):
    """-> (fpr, fnr, thresholds, eer, k).  ValueError for a non-finite score or a single-class list."""
    s = np.asarray(scores)
    y = np.asarray(y_true) != 0
    if s.ndim != 1 or s.shape != y.shape:
        raise ValueError("one score per label")
    if not np.isfinite(s).all():
        raise ValueError("non-finite score")
    if y.all() or not y.any():
        raise ValueError("both classes are needed")
    if distances:
        s = -s
    order = np.argsort(s, kind="stable")[::-1]            # descending; ties in reverse input order
    s, y = s[order], y[order]
    ends = np.flatnonzero(np.r_[s[1:] != s[:-1], True])   # last element of every run of equal VALUES (-0.0 == 0.0)
    tps = np.cumsum(y, dtype=np.int64)[ends]
    fps = 1 + ends.astype(np.int64) - tps
    thresholds = s[ends]
    if len(ends) > 2:
        keep = np.ones(len(ends), dtype=bool)
        towards_next = np.stack([fps[2:] - fps[1:-1], tps[2:] - tps[1:-1]])
        from_previous = np.stack([fps[1:-1] - fps[:-2], tps[1:-1] - tps[:-2]])
        keep[1:-1] = (towards_next != from_previous).any(axis=0)
        fps, tps, thresholds = fps[keep], tps[keep], thresholds[keep]
    fps, tps = np.r_[np.int64(0), fps], np.r_[np.int64(0), tps]
    thresholds = np.r_[np.inf, thresholds.astype(np.float64)]
    fpr = fps.astype(np.float64) / np.float64(fps[-1])
    fnr = 1.0 - tps.astype(np.float64) / np.float64(tps[-1])
    if distances:
        thresholds = -thresholds
    k = int(np.flatnonzero(fpr > fnr)[0])
    eer = 0.25 * (((fpr[k - 1] + fpr[k]) + fnr[k - 1]) + fnr[k])
    return fpr, fnr, thresholds, float(eer), k


def _mixed(rng, n, shift=1.0):
    """n labels and unit-variance scores whose targets sit `shift` higher"""
    y = rng.random(n) < 0.4
    y[:2] = (True, False)
    return y, rng.normal(size=n) + shift * y


def _tie_across(rng, T, first, stop):
    """T distinct scores, those at descending ranks first..stop-1 (cut to the list) made equal, in random order"""
    y, s = _mixed(rng, T)
    order = np.argsort(-s, kind="stable")
    s[order[max(first, 0):min(stop, T)]] = s[order[max(first, 0)]]
    return y, s


def _long_negative_run(rng):
    """300 mixed trials (mostly targets), more than 2 B distinct pure non-targets, 200 mixed trials, by falling
    score: the run crosses two workgroup boundaries, every point inside it is collinear, and the first point with
    fpr > fnr is the run's far corner, whose predecessor on the curve is the corner 2 B + 100 elements earlier"""
    run = 2 * B + 100
    head_y = rng.random(300) < 0.9
    tail_y = rng.random(200) < 0.5
    y = np.r_[head_y, np.zeros(run, dtype=bool), tail_y]
    s = np.sort(rng.random(len(y)))[::-1].copy()          # distinct with probability 1
    shuffle = rng.permutation(len(y))
    return y[shuffle], s[shuffle]


def small_cases():
    """name -> (y_true, scores): the cases small enough for the golden file"""
    rng = np.random.default_rng(20240611)
    cases = {}
    cases["t2"] = (np.array([True, False]), np.array([0.9, 0.1]))
    cases["t3"] = (np.array([False, True, False]), np.array([0.2, 0.7, 0.5]))
    cases["all_equal"] = (np.array([True, False, False, True, False, True, False]), np.full(7, 0.5))
    cases["two_groups"] = (np.array([1, 1, 0, 1, 0, 0, 1, 0, 0, 0], dtype=bool),
                           np.array([.75, .75, .75, .25, .25, .75, .75, .25, .25, .25]))
    y = np.r_[np.ones(8, dtype=bool), np.zeros(12, dtype=bool)]
    s = np.r_[2.0 + rng.random(8), rng.random(12)]
    shuffle = rng.permutation(20)
    cases["separated"] = (y[shuffle], s[shuffle])
    cases["inverted"] = (y[shuffle], -s[shuffle])
    # one tie group holds most of the list: the first point after (0, 0) already has fpr > fnr (k = 1)
    cases["first_point_crosses"] = (np.array([1, 0, 1, 0, 1, 0, 0], dtype=bool),
                                    np.array([1.0, 1.0, 1.0, 1.0, 0.5, 1.0, 0.25]))
    y, s = _mixed(rng, 500)
    cases["rounded"] = (y, np.round(s, 2))
    cases["signed_zeros"] = (np.array([1, 0, 0, 1, 1, 0, 1, 0, 0, 1], dtype=bool),
                             np.array([-0.0, 0.0, 0.0, -0.0, 0.5, -0.5, 0.0, -0.0, 0.25, -0.25]))
    cases["signed_zeros_ends_positive"] = (np.array([0, 1, 0, 1], dtype=bool), np.array([0.0, -0.0, 1.0, -1.0]))
    for T in (B - 1, B, B + 1):
        cases[f"block_{T}"] = _tie_across(rng, T, B - 3, B + 2)
    cases["long_negative_run"] = _long_negative_run(rng)
    y, s = _mixed(rng, 300)
    cases["float32_bool"] = (y, np.round(s, 1).astype(np.float32))
    cases["float32_int64"] = (y.astype(np.int64), s.astype(np.float32))
    return cases


def scan_case():
    """The smallest list that fills more than one chunk of the workgroup-sum scan: B * CHUNK + 1 elements, so a
    second chunk exists and the single top-level workgroup has two sums to scan.  Distinct scores: the groups, and
    about half of them as kept points, run into the second chunk as well."""
    rng = np.random.default_rng(7)
    return _mixed(rng, B * CHUNK + 1)


def large_zero_mix_case():
    """40 000 scores of which about a third are zeros of both signs, the rest rounded to two decimals: large enough
    for the device sort's radix path, where -0.0 and 0.0 must still be one key and keep their input order.  The zero
    group's threshold is the zero that comes first in the input; its sign is made negative here, so a sort that
    orders -0.0 before 0.0 by bits, or is not stable across them, changes the threshold's sign or the counts."""
    rng = np.random.default_rng(11)
    y, s = _mixed(rng, 40000, shift=0.5)
    s = np.round(s, 2)
    zero = rng.random(len(s)) < 0.33
    s[zero] = np.where(rng.random(int(zero.sum())) < 0.5, -0.0, 0.0)
    first = np.flatnonzero(s == 0)[0]
    s[first] = -0.0
    s[np.flatnonzero(s == 0)[1]] = 0.0
    return y, s
