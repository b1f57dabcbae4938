"""tests/frames_model.py is what the frame-domain kernels are held to (tests/test_frames_kernels_gpu.py), so it is held
to something itself, here, without a GPU:

  * on regular chunk grids (the geometries of tests/test_frames_gpu.py with fewer chunks) every model function equals
    the oracle's restatement of the reference (oracle.pipeline), bit for bit;
  * every deliberately wrong variant of a model function (frames_model.WRONG) gives a different output on at least one
    listed case of its operation: the case lists can tell such a kernel from a right one.

The initial state of the hysteresis deserves a word.  oracle.pipeline.hysteresis compares the float32 scores of frame 0
with the Python float 0.5 * (onset + offset) as numpy does -- rounded once to float32 -- which is the reference's own
expression (utils/signal.py:111).  The model states that rounding explicitly, and the two must agree on EVERY
hysteresis case, the knife-edge ones included, where the first score is that float32 midpoint or a neighbour of it:
this agreement is what makes the model the reference's statement rather than the kernel's."""
import numpy as np
import pytest

import frames_model as fm
from oracle import pipeline as op

FRAMES = (0.0, 0.0619375, 0.016875)
#: C, F, S, chunk duration, chunk step, seed: tests/test_frames_gpu.py's geometries with fewer chunks
GEOMETRIES = [(7, 589, 3, 10.0, 1.0, 0), (9, 293, 3, 5.0, 0.5, 1), (1, 589, 3, 10.0, 1.0, 2), (5, 589, 4, 10.0, 2.5, 3)]


def _geometry(C, F, dur, step):
    """chunk and frame windows, the start frame of every chunk and the number of global frames, as
    oracle.pipeline.aggregate computes them"""
    chunks, frames = op.SW(0.0, dur, step), op.SW(*FRAMES)
    out = op.SW(chunks.start, frames.duration, frames.step)
    T = out.closest_frame(chunks.start + chunks.duration + (C - 1) * chunks.step + 0.5 * out.duration) + 1
    start = np.array([out.closest_frame(chunks.segment(c)[0] + 0.5 * out.duration) for c in range(C)], dtype=np.int32)
    return chunks, frames, start, T


def _random_segmentation(C, F, S, seed):
    rng = np.random.default_rng(seed)
    seg = np.zeros((C, F, S), dtype=np.float32)
    for c in range(C):
        for s in range(S):
            if rng.uniform() < 0.75:
                for _ in range(rng.integers(1, 4)):
                    a = rng.integers(0, F)
                    seg[c, a:min(F, a + rng.integers(1, F)), s] = 1
    return seg


def _assert_selection(got, tie, want, act, what):
    """frames without a flagged tie: equal.  Flagged frames: the oracle's np.argsort may order equal activations in any
    way, so there the two select equally many clusters, all of those above the boundary value and none below it."""
    assert got.shape == want.shape, what
    plain = tie == 0
    assert np.array_equal(got[plain].astype(want.dtype), want[plain]), what
    for t in np.flatnonzero(tie):
        boundary = act[t][got[t] == 1].min()
        assert got[t].sum() == want[t].sum(), (what, t)
        assert np.array_equal(want[t][act[t] > boundary], np.ones((act[t] > boundary).sum())), (what, t)
        assert not want[t][act[t] < boundary].any(), (what, t)


@pytest.mark.parametrize("C,F,S,dur,step,seed", GEOMETRIES)
def test_count_and_hard_reconstruction_equal_the_oracle(C, F, S, dur, step, seed):
    seg = _random_segmentation(C, F, S, seed)
    seg8 = seg.astype(np.uint8)
    chunks, frames, start, T = _geometry(C, F, dur, step)
    want_count, count_frames = op.speaker_count(seg, chunks, frames)
    count = fm.speaker_count(seg8, start, T)
    assert want_count.shape == (T, 1) and np.array_equal(count, want_count[:, 0])

    rng = np.random.default_rng(100 + seed)
    for K in (1, 2, 5):
        hard = rng.integers(0, K, size=(C, S))
        hard[rng.uniform(size=(C, S)) < 0.2] = -2
        hard[0, 0] = K - 1
        for cap in (255, 1):
            capped = np.minimum(want_count, cap).astype(np.int8)
            want = op.reconstruct(seg, chunks, hard, capped, count_frames)
            width = max(K, int(capped.max()))
            act = fm.cluster_activations(seg8, start, hard.astype(np.int32), width, T)
            # the same activations by the oracle's own overlap-add of the model's per-chunk maxima, and by the model's
            clustered = fm.cluster_max(seg, hard, width)
            by_oracle, _ = op.aggregate(clustered, chunks, frames, missing=0.0, skip_average=True)
            assert np.array_equal(act.astype(np.float32), by_oracle), (K, cap)
            by_model = fm.aggregate(clustered, start, T, np.ones(F), np.ones(F), 1e-12, 0.0, 1)
            assert fm.same_bits(by_model, by_oracle), (K, cap)
            got, tie = fm.topk(act, capped[:, 0].astype(np.uint8), 255)
            _assert_selection(got, tie, want, act, (K, cap))
            # a cap inside topk is the cap on the counts
            got_cap, tie_cap = fm.topk(act, want_count[:, 0], cap)
            assert np.array_equal(got_cap, got) and np.array_equal(tie_cap, tie)


def test_soft_reconstruction_equals_the_oracle():
    rng = np.random.default_rng(3)
    C, F, S = 7, 589, 3
    scores = rng.uniform(size=(C, F, S)).astype(np.float32)
    scores[:, ::5, :] = np.round(scores[:, ::5, :] * 4) / 4                 # equal activations do occur
    hard = rng.integers(-2, 4, size=(C, S))
    hard[hard == -1] = 0
    hard[0, 0] = 3
    hard[4] = -2
    chunks, frames, start, T = _geometry(C, F, 10.0, 1.0)
    count, count_frames = op.speaker_count((scores > 0.5).astype(np.float32), chunks, frames)
    for cap in (255, 1):
        capped = np.minimum(count, cap).astype(np.int8)
        want = op.reconstruct(scores, chunks, hard.copy(), capped, count_frames)
        width = max(4, int(capped.max()))
        clustered = fm.cluster_max(scores, hard, width)
        act = fm.aggregate(clustered, start, T, np.ones(F), np.ones(F), 1e-12, 0.0, 1)
        by_oracle, _ = op.aggregate(clustered, chunks, frames, missing=0.0, skip_average=True)
        assert fm.same_bits(act, by_oracle)
        got, tie = fm.topk(act, capped[:, 0].astype(np.uint8), 255)
        _assert_selection(got, tie, want, act, cap)


@pytest.mark.parametrize("C,F,S,dur,step,seed", GEOMETRIES)
def test_aggregate_equals_the_oracle(C, F, S, dur, step, seed):
    rng = np.random.default_rng(40 + seed)
    scores = rng.uniform(size=(C, F, S)).astype(np.float32)
    scores.reshape(-1)[rng.integers(0, scores.size, size=scores.size // 9)] = np.nan
    scores[::2, :, 0] = np.nan
    scores[:, :, 1] = np.nan
    chunks, frames, start, T = _geometry(C, F, dur, step)
    for hamming in (False, True):
        for warm_up in ((0.0, 0.0), (0.1 * dur, 0.05 * dur)):
            for skip in (False, True):
                for missing in (np.nan, 0.0):
                    want, _ = op.aggregate(scores, chunks, frames, warm_up=warm_up, hamming=hamming, missing=missing,
                                           skip_average=skip)
                    warm = np.ones(F)
                    left, right = round(warm_up[0] / dur * F), round(warm_up[1] / dur * F)
                    warm[:left] = 1e-12
                    warm[F - right:] = 1e-12
                    got = fm.aggregate(scores, start, T, np.hamming(F) if hamming else np.ones(F), warm, 1e-12,
                                       missing, int(skip))
                    assert got.dtype == np.float32 and fm.same_bits(got, want), (hamming, warm_up, skip, missing)


def test_hysteresis_equals_the_oracle_on_every_case():
    """(see the module docstring: the knife-edge cases are among these)"""
    edge = 0
    for case in fm.hysteresis_cases():
        initial = {-1: None, 0: False, 1: True}[case["initial_state"]]
        want = op.hysteresis(case["scores"], onset=case["onset"], offset=case["offset"], initial_state=initial)
        got = fm.hysteresis(case["scores"], case["onset"], case["offset"], case["initial_state"])
        assert got.dtype == np.uint8 and np.array_equal(got.astype(np.float64), want), case["id"]
        edge += (case["onset"], case["offset"]) in fm.KNIFE_EDGE_PAIRS
    assert edge >= 3 * 18


def test_knife_edge_pairs_are_knife_edges():
    """the float32 product of the float32 thresholds is a neighbour of the reference's midpoint, not the midpoint"""
    for onset, offset in fm.KNIFE_EDGE_PAIRS:
        mid = fm.hysteresis_midpoint(onset, offset)
        assert np.float32(0.5) * (np.float32(onset) + np.float32(offset)) in (np.nextafter(mid, np.float32(1)),
                                                                              np.nextafter(mid, np.float32(-1)))


def test_chunk_stats_and_masks_equal_the_numpy_expressions():
    """the expressions of test_frames_gpu.test_chunk_stats_and_masks, on every listed case"""
    for case in fm.embedding_masks_cases():
        seg = case["seg"].astype(np.float32)
        C, F, S = seg.shape
        single = seg.sum(axis=2, keepdims=True) == 1
        active, clean = fm.chunk_stats(case["seg"])
        assert active.dtype == clean.dtype == np.int32
        assert np.array_equal(active, seg.sum(axis=1).astype(np.int32)), case["id"]
        assert np.array_equal(clean, (seg * single).sum(axis=1).astype(np.int32)), case["id"]
        clean_seg = seg * (seg.sum(axis=2, keepdims=True) < 2)
        want = np.empty((C, S, F), dtype=np.float32)
        for c in range(C):
            for s in range(S):
                use_clean = case["exclude_overlap"] and clean_seg[c, :, s].sum() > case["min_num_frames"]
                want[c, s] = clean_seg[c, :, s] if use_clean else seg[c, :, s]
        got = fm.embedding_masks(case["seg"], clean, case["exclude_overlap"], case["min_num_frames"])
        assert got.dtype == np.float32 and np.array_equal(got, want), case["id"]


def test_distinct_activations_have_no_tie():
    for cases in (fm.topk_i32_cases(), fm.topk_f32_cases()):
        for case in cases[:24]:
            if case["distinct"]:
                assert not fm.topk(case["act"], case["count"], case["cap"])[1].any(), case["id"]


def _differs(a, b):
    if a.dtype == np.float32:
        return not fm.same_bits(a, b)
    return not np.array_equal(a, b)


@pytest.mark.parametrize("operation,wrong", [(o, w) for o, names in fm.WRONG.items() for w in names])
def test_cases_catch_a_wrong_kernel(operation, wrong):
    """at least one listed case of the operation separates the wrong variant from the model"""
    cases, run = fm.OPERATIONS[operation]
    caught = next((case["id"] for case in cases()
                   if any(_differs(a, b) for a, b in zip(run(case, wrong=wrong), run(case)))), None)
    assert caught is not None, f"no {operation} case tells `{wrong}` from the model: the case list is too weak"
