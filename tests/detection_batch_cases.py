"""The cases of tests/test_detection_batch_cpu.py and tests/test_detection_batch_gpu.py (TEST INFRASTRUCTURE ONLY):
ragged lists of files for `binarize_regions_files` and `aggregate_files`, built once per process from fixed seeds and
never modified by their users."""
import functools

import numpy as np

import multilabel_oracle as mo

FRAMES = (0.0, 0.0619375, 0.016875)
#: frames per file: chunk (64) and tile (1024) boundaries of the region kernels, and fewer than two frames
REGION_T = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2500]
#: (name, onset, offset, min_duration_on, min_duration_off) of class 0; class k adds 0.01 k to both thresholds
REGION_PARAMETERS = [
    ("offset_below_onset", 0.6, 0.4, 0.0, 0.0),
    ("offset_is_onset", 0.5, 0.5, 0.1, 0.08),
    ("offset_above_onset", 0.4, 0.6, 0.05, 0.1),
]


def region_parameters(name, K):
    _, onset, offset, d_on, d_off = next(p for p in REGION_PARAMETERS if p[0] == name)
    k = np.arange(K)
    return onset + 0.01 * k, offset + 0.01 * k, np.full(K, d_on), np.full(K, d_off)


@functools.lru_cache(maxsize=None)
def region_files(K):
    """-> per file a (T, K) float32 array: a smoothed random walk per class, with these deliberate neighbours
      file 2 (63 frames)      column 0 is all NaN
      file 3 -> file 4        3 is active to its last frame, 4 from its first one: neither merged nor leaked
      file 5, 6, 7            an all-inactive file between one that ends active and one that starts active"""
    rng = np.random.default_rng(4000 + K)
    files = [mo.smooth_scores(rng, T, K, width=9) for T in REGION_T]
    files[2][:, 0] = np.nan
    files[3][-10:] = 0.95
    files[4][:10] = 0.95
    files[5][-20:] = 0.95
    files[6][:] = 0.05
    files[7][:20] = 0.95
    for x in files:
        x.setflags(write=False)
    return files


def oracle_per_file(files, onset, offset, d_on, d_off):
    """multilabel_oracle.all_regions of every file alone"""
    return [mo.all_regions(x, *FRAMES, onset, offset, d_on, d_off) for x in files]


def assert_same_lists(got, want, where):
    """got: (regions, positions) per file as frames.binarize_regions_files returns them, or the model's per-file
    [(rows, positions)]; want: per file, per class ([(start, end)], [position]).  Times bit for bit."""
    regions, positions = got
    assert len(regions) == len(want) and len(positions) == len(want), where
    for f, per_class in enumerate(want):
        for k, (want_rows, want_positions) in enumerate(per_class):
            w = np.array(want_rows, dtype=np.float64).reshape(-1, 2)
            g = np.ascontiguousarray(np.array(regions[f][k], dtype=np.float64).reshape(-1, 2))
            assert g.shape == w.shape, (where, f, k, g.shape, w.shape)
            assert np.array_equal(g.view(np.int64), w.view(np.int64)), (where, f, k)
            assert list(np.asarray(positions[f][k]).tolist()) == list(want_positions), (where, f, k)


# ------------------------------------------------------------------------------------------------ aggregate_files
AGG_F, AGG_S = 293, 3
AGG_COUNTS = [1, 4, 13, 2]
AGG_CHUNKS = (0.0, 5.0, 0.5)          # start, duration, step of the chunk grid
AGG_WARM_UP = (0.1, 0.1)


@functools.lru_cache(maxsize=None)
def aggregate_scores(kind):
    """chunk scores (sum of AGG_COUNTS, F, S) of the three modes:
      "classes"  float32, about 20 % NaN, the first two chunks of file 2 all NaN (rows nobody voted on)
      "any"      the same: a NaN in a column makes the frame's maximum NaN
      "hard"     uint8 {0, 1}"""
    rng = np.random.default_rng(77)
    total = sum(AGG_COUNTS)
    if kind == "hard":
        x = (rng.uniform(size=(total, AGG_F, AGG_S)) < 0.3).astype(np.uint8)
    else:
        x = rng.uniform(size=(total, AGG_F, AGG_S)).astype(np.float32)
        x[rng.uniform(size=x.shape) < 0.2] = np.nan
        first = sum(AGG_COUNTS[:2])
        x[first:first + 2] = np.nan
    x.setflags(write=False)
    return x
