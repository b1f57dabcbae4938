"""The host side of the replay route (pyannote_audio_amd.online.file_schedule) and the numpy model the device tests
hold `pao_replay` to (tests/online_replay_model.py), without a device."""
import numpy as np
import pytest

import online_model as om
import online_replay_model as rm

SAMPLE_RATE, DURATION, STEP = 16000, 5.0, 0.5
WINDOW, STEP_SAMPLES = 80000, 8000
FRAME_STEP, FRAME_DURATION = 270 / 16000, 991 / 16000        # PyanNet's receptive field (SincNet stride 10)
LATENCIES = [0.5 * i for i in range(1, 11)]                   # every multiple of the step in [step, duration]
LENGTHS = [0, 1, STEP_SAMPLES - 1, STEP_SAMPLES, WINDOW - 1, WINDOW, WINDOW + 1, WINDOW + STEP_SAMPLES - 1,
           WINDOW + STEP_SAMPLES, 116800]


def _geometry():
    from pyannote_audio_amd.core import SlidingWindow
    from pyannote_audio_amd.segmentation import num_frames
    return SlidingWindow(start=0.0, duration=FRAME_DURATION, step=FRAME_STEP), num_frames(WINDOW)


def _bookkeeping(num_samples, latency, frames, F):
    """the bookkeeping of `ModelBank` (tests/test_online_gpu.py) for one stream of `num_samples` samples, pushed in
    whole steps and closed with its tail, without the device calls -> (rows of the chunks, flush row or None, total)"""
    from pyannote_audio_amd.online import stream_num_frames
    state = dict(have=0, chunks=0, emitted=0)
    rows = []

    def step(limit=None):
        c = state["chunks"]
        start = om.start_frame(c, STEP, FRAME_STEP, FRAME_DURATION)
        bound = om.emit_bound(c, STEP, DURATION, latency, FRAME_STEP, FRAME_DURATION)
        to = max(min(bound, start + F, limit if limit is not None else bound), state["emitted"])
        rows.append((start, state["emitted"], to))
        state["emitted"], state["chunks"] = to, c + 1

    tail = num_samples % STEP_SAMPLES
    for _ in range(num_samples // STEP_SAMPLES):                                   # push
        state["have"] += STEP_SAMPLES
        if state["have"] >= WINDOW:
            step()
    state["have"] += tail                                                          # close
    total = stream_num_frames(state["have"], WINDOW, STEP_SAMPLES, SAMPLE_RATE, DURATION, STEP, frames)
    if state["have"] < WINDOW:
        if state["have"] > 0:
            step(limit=total)
    elif tail:
        step(limit=total)
    flush = (-1, state["emitted"], total) if state["emitted"] < total else None
    return rows, flush, total


@pytest.mark.parametrize("latency", LATENCIES)
def test_file_schedule_is_the_streaming_bookkeeping(latency):
    from pyannote_audio_amd.online import file_schedule, stream_num_frames
    frames, F = _geometry()
    assert F == 293
    R = 2 * F + 16
    for n in LENGTHS:
        C, rows, total = file_schedule(n, window=WINDOW, step_samples=STEP_SAMPLES, sample_rate=SAMPLE_RATE,
                                       duration=DURATION, step=STEP, latency=latency, frames=frames, F=F)
        assert rows.shape == (C + 1, 3) and rows.dtype == np.int64
        assert total == stream_num_frames(n, WINDOW, STEP_SAMPLES, SAMPLE_RATE, DURATION, STEP, frames)
        if n == 0:
            assert (C, total) == (0, 0)
        # the rows tile [0, total)
        assert rows[0, 1] == 0 and rows[-1, 2] == total
        assert (rows[1:, 1] == rows[:-1, 2]).all() and (rows[:, 1] <= rows[:, 2]).all()
        # the ring condition of every row, with the ring a bank allocates
        assert all(g0 < 0 or g0 + F - ga <= R for g0, ga, _ in rows.tolist())
        assert rows[-1, 0] < 0 and (rows[:-1, 0] >= 0).all()
        want, flush, want_total = _bookkeeping(n, latency, frames, F)
        assert total == want_total and C == len(want), f"{n} samples: {C} chunks for {len(want)}"
        assert rows[:C].tolist() == [list(r) for r in want], f"{n} samples at latency {latency}"
        assert tuple(rows[C].tolist()) == (flush if flush is not None else (-1, want[-1][2] if want else 0, total)), \
            f"{n} samples at latency {latency}: the flush row"
        # chunks come from whole steps, the tail padded to one; a short file gets one chunk
        blocks = -(-n // STEP_SAMPLES)
        assert C == (0 if n == 0 else max(1, blocks - WINDOW // STEP_SAMPLES + 1))


def test_the_model_agrees_with_online_model_on_a_hand_case():
    """two steps written out with `online_model` directly, D = 2, K = 2, F = 3, one frame per step"""
    emb = np.array([[[1, 0], [0, 1]], [[1, 0.1], [-1, 0]]], dtype=np.float32)
    active = np.array([[9, 9], [9, 9]], dtype=np.int32)
    clean = np.array([[9, 2], [9, 9]], dtype=np.int32)
    seg = np.array([[[1, 0], [1, 1], [0, 1]], [[1, 1], [0, 1], [1, 0]]], dtype=np.uint8)
    sched = np.array([[0, 0, 1], [1, 1, 2], [-1, 2, 6]], dtype=np.int64)
    total, R, K = 6, 5, 2
    csum, cn = np.zeros((K, 2)), np.zeros(K, dtype=np.int32)
    acc_sum, acc_cnt = np.zeros((R, K), dtype=np.int32), np.zeros(R, dtype=np.int32)
    rows, maps = [], []
    for c in range(2):
        maps.append(om.cluster_step_one(emb[c], active[c], clean[c], csum, cn, 5, 8, 0.5))
        rows.append(om.emit_one(seg[c], maps[c], *sched[c].tolist(), acc_sum, acc_cnt, 1))
    rows.append(om.emit_one(np.zeros((3, 2), np.uint8), np.full(2, -1), -1, 2, 6, acc_sum, acc_cnt, 4))
    # step 0: speaker 0 founds centroid 0, speaker 1 is present but short and finds nothing; step 1: speaker 0
    # matches and updates, speaker 1 is long, too far from centroid 0's holder, and founds centroid 1
    assert [m.tolist() for m in maps] == [[0, -1], [0, 1]] and cn.tolist() == [2, 1]
    assert (csum == np.array([[2.0, np.float64(np.float32(0.1))], [-1.0, 0.0]])).all()
    want = np.concatenate(rows)
    assert want.tolist() == [[1, 0], [1, 0], [0, 0], [1, 0], [0, 0], [0, 0]]      # frame 5 is covered by no chunk
    for run in (rm.replay_one, rm.interleaved):
        state = np.zeros((K, 2)), np.zeros(K, dtype=np.int32), np.zeros((R, K), np.int32), np.zeros(R, np.int32)
        got = run(emb, active, clean, seg, sched, total, 5, 8, 0.5, *state)
        assert (got[0] == np.array(maps)).all() and (got[1] == want).all()
        assert state[0].tobytes() == csum.tobytes() and (state[1] == cn).all()
        assert (state[2] == acc_sum).all() and (state[3] == acc_cnt).all()
    events = rm.replay_one(emb, active, clean, seg, sched, total, 5, 8, 0.5, np.zeros((K, 2)), np.zeros(K, np.int32),
                           np.zeros((R, K), np.int32), np.zeros(R, np.int32))[2]
    assert dict(events) == {"found": 2, "nothing_can_take": 1, "update": 1}


def test_the_generated_cases_reach_every_branch_of_the_rule():
    """the six cases of tests/test_online_replay_gpu.py: found, updated, forced, un-mapped and absent speakers in
    every one of them (the counts the cases were chosen for)"""
    for seed, C, S, D, K, V, sigma, delta_new in rm.CASES:
        emb, active, clean, _ = rm.generate(seed, C, S, D, V, sigma, 1)
        _, events = rm.cluster_file(emb, active, clean, np.zeros((K, D)), np.zeros(K, np.int32), 10, 15, delta_new)
        assert events["found"] >= 1 and events["update"] >= 6 and events["forced"] >= 3, (seed, dict(events))
        assert events["unmapped"] >= 3 and events["absent"] >= 10, (seed, dict(events))
        assert seed == 2 or events["nothing_can_take"] >= 1, (seed, dict(events))
