"""Cases and truths of the region sweep (`frames.binarize_regions_sweep`), shared by the CPU and GPU tests
(TEST INFRASTRUCTURE ONLY).  The truth of every job is tests/multilabel_oracle.py `class_regions` on the job's column
with the job's four parameters; it is computed once per case and kept."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import multilabel_oracle as mo  # noqa: E402

FRAMES = (0.0, 0.0619375, 0.016875)             # start, duration, step
TILE_EDGES = (2, 3, 1023, 1024, 1025, 3073)     # frames per workgroup in csrc/regions.h: 1024
WORD_EDGES = (1, 15, 16, 17, 33)                # lanes of one class per map word: 16
NAN_FRACTIONS = (0.0, 0.02, 1.0)
DURATIONS = ((0.0, 0.0), (0.05, 0.1), (0.12, 0.04))      # (min_duration_on, min_duration_off)


def window():
    from pyannote_audio_amd.core import SlidingWindow
    return SlidingWindow(start=FRAMES[0], duration=FRAMES[1], step=FRAMES[2])


def make_case(seed: int, T: int, K: int, many: int, nan_fraction: float):
    """class `many % K` gets `many` lanes, every other class one; thresholds below and above each other; every lane
    but each class's last gets the three duration pairs (that one has no job); jobs in shuffled order"""
    rng = np.random.default_rng(seed)
    scores = mo.smooth_scores(rng, T, K, width=int(rng.integers(1, 12)), nan_fraction=nan_fraction)
    lane_class = np.concatenate([np.full(many if k == many % K else 1, k) for k in range(K)]).astype(np.int32)
    lane_class = lane_class[rng.permutation(len(lane_class))]
    L = len(lane_class)
    onset = rng.uniform(0.3, 0.7, L).astype(np.float32)
    offset = rng.uniform(0.3, 0.7, L).astype(np.float32)
    offset[::5] = onset[::5]
    jobless = set()
    if many > 1:
        jobless.add(int(np.flatnonzero(lane_class == many % K)[-1]))
    jobs = [(l, a, b) for l in range(L) if l not in jobless for a, b in DURATIONS]
    jobs = [jobs[i] for i in rng.permutation(len(jobs))]
    job_lane = np.array([j[0] for j in jobs], dtype=np.int32)
    d_on = np.array([j[1] for j in jobs], dtype=np.float64)
    d_off = np.array([j[2] for j in jobs], dtype=np.float64)
    return scores, lane_class, onset, offset, job_lane, d_on, d_off


@functools.lru_cache(maxsize=None)
def case_with_truth(seed: int, T: int, K: int, many: int, nan_fraction: float):
    case = make_case(seed, T, K, many, nan_fraction)
    return case, truth(*case)


def truth(scores, lane_class, onset, offset, job_lane, d_on, d_off):
    out = []
    for lane, a, b in zip(job_lane.tolist(), d_on.tolist(), d_off.tolist()):
        regions, positions = mo.class_regions(scores[:, lane_class[lane]], *FRAMES, onset[lane], offset[lane], a, b)
        out.append((np.array(regions, dtype=np.float64).reshape(-1, 2), list(positions)))
    return out


def grid(K: int):
    """(seed, T, K, many, nan_fraction) of the grid: every tile edge with every NaN fraction, the word edges in turn"""
    cases, n = [], 0
    for T in TILE_EDGES:
        for nan_fraction in NAN_FRACTIONS:
            for many in (WORD_EDGES if T in (3, 1025) else (WORD_EDGES[n % len(WORD_EDGES)],)):
                cases.append((1000 * K + n, T, K, many, nan_fraction))
                n += 1
    return cases


def assert_same(got, want, where):
    regions, positions = got
    assert len(regions) == len(want) == len(positions), where
    for j, (rows, tracks) in enumerate(want):
        assert regions[j].dtype == np.float64 and regions[j].shape == rows.shape, (where, j, regions[j].shape, rows.shape)
        assert np.array_equal(np.ascontiguousarray(regions[j]).view(np.int64), rows.view(np.int64)), (where, j)
        assert np.asarray(positions[j]).tolist() == tracks, (where, j)
