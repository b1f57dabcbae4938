"""numpy model of `pao_replay` (include/pyannote_amd_online.h): the literal loop over the chunks of one file --
`online_model.cluster_step_one`, then `online_model.emit_one` with the chunk's schedule row -- and the flush.  It also
classifies what happened to every local speaker of every step (found / update / forced / un-mapped / absent / nothing
can take it), so that a test can assert its inputs reach every branch of the rule."""
from collections import Counter

import numpy as np
from scipy.spatial.distance import cdist

import online_model as om


def step_events(emb, active, csum, cn, mp, cn_after, min_active, delta_new):
    """the events of one step, from the state BEFORE it (csum, cn), its map and centroid_n AFTER it -> Counter"""
    S = emb.shape[0]
    K = cn.shape[0]
    e64 = emb.astype(np.float64)
    with np.errstate(all="ignore"):
        present = [bool(active[s] >= min_active and np.isfinite(emb[s]).all() and np.any(emb[s] != 0)) for s in range(S)]
    occupied = [bool(cn[k] > 0) for k in range(K)]
    ps, oc = [s for s in range(S) if present[s]], [k for k in range(K) if occupied[k]]
    d = np.full((S, K), np.nan)
    if ps and oc:
        with np.errstate(all="ignore"):
            d[np.ix_(ps, oc)] = cdist(e64[ps], csum[oc], "cosine")
    tup = om.optimal_map(d, present, occupied, K)
    events = Counter()
    for s in range(S):
        if not present[s]:
            events["absent"] += 1
            continue
        assigned = tup[s] < K
        matched = assigned and not d[s][tup[s]] > delta_new
        if assigned and not matched:
            events["unmapped"] += 1
        if matched:
            if cn_after[mp[s]] == cn[mp[s]] + 1:
                events["update"] += 1
        elif mp[s] >= 0 and not occupied[mp[s]]:
            events["found"] += 1
        elif mp[s] >= 0:
            events["forced"] += 1
        else:
            events["nothing_can_take"] += 1
    return events


def cluster_file(emb, active, clean, csum, cn, min_active, min_update, delta_new):
    """the clustering steps of one file in turn: emb (C, S, D), active / clean (C, S); csum (K, D) and cn (K) updated
    in place -> (maps (C, S) int32, Counter of events)"""
    C, S, _ = emb.shape
    maps = np.empty((C, S), dtype=np.int32)
    events = Counter()
    for c in range(C):
        before_sum, before_n = csum.copy(), cn.copy()
        maps[c] = om.cluster_step_one(emb[c], active[c], clean[c], csum, cn, min_active, min_update, delta_new)
        events += step_events(emb[c], active[c], before_sum, before_n, maps[c], cn, min_active, delta_new)
    return maps, events


def emit_file(seg, maps, sched, total, acc_sum, acc_cnt):
    """the emissions of one file in turn, the flush row last: seg (C, F, S), maps (C, S), sched (C + 1, 3); acc_sum
    (R, K) and acc_cnt (R) updated in place -> out (total, K) uint8, row g - sched[0][1] holding frame g"""
    C, F, S = seg.shape
    K = acc_sum.shape[1]
    out = np.zeros((total, K), dtype=np.uint8)
    first = int(sched[0][1])
    for c in range(C + 1):
        g0, ga, gb = (int(v) for v in sched[c])
        if c < C:
            rows = om.emit_one(seg[c], maps[c], g0, ga, gb, acc_sum, acc_cnt, gb - ga)
        else:
            rows = om.emit_one(np.zeros((F, S), np.uint8), np.full(S, -1), -1, ga, gb, acc_sum, acc_cnt, gb - ga)
        out[ga - first:gb - first] = rows
    return out


def replay_one(emb, active, clean, seg, sched, total, min_active, min_update, delta_new, csum, cn, acc_sum, acc_cnt):
    """one job: cluster step then emission per chunk, then the flush; the state is updated in place
    -> (maps (C, S), out (total, K), events).  The two loops are run one after the other: a clustering step reads
    nothing an emission writes, so the interleaved loop of the kernel gives the same."""
    maps, events = cluster_file(emb, active, clean, csum, cn, min_active, min_update, delta_new)
    return maps, emit_file(seg, maps, sched, total, acc_sum, acc_cnt), events


def interleaved(emb, active, clean, seg, sched, total, min_active, min_update, delta_new, csum, cn, acc_sum, acc_cnt):
    """the same written as the kernel walks it: step c, emission c, ..., flush -> (maps, out)"""
    C, F, S = seg.shape
    K = cn.shape[0]
    maps = np.empty((C, S), dtype=np.int32)
    out = np.zeros((total, K), dtype=np.uint8)
    first = int(sched[0][1])
    for c in range(C):
        g0, ga, gb = (int(v) for v in sched[c])
        maps[c] = om.cluster_step_one(emb[c], active[c], clean[c], csum, cn, min_active, min_update, delta_new)
        out[ga - first:gb - first] = om.emit_one(seg[c], maps[c], g0, ga, gb, acc_sum, acc_cnt, gb - ga)
    _, ga, gb = (int(v) for v in sched[C])
    out[ga - first:gb - first] = om.emit_one(np.zeros((F, S), np.uint8), np.full(S, -1), -1, ga, gb, acc_sum, acc_cnt,
                                             gb - ga)
    return maps, out


# ------------------------------------------------------------------------------------------------ inputs of the tests
#: (seed, C, S, D, K, V, sigma, delta_new) with min_active_frames = 10 and min_update_frames = 15: every case founds,
#: updates, forces, un-maps and leaves absent; every case but seed 2 has a present speaker nothing can take
CASES = [(0, 40, 3, 8, 3, 5, 0.5, 0.5), (1, 40, 4, 16, 5, 4, 0.4, 0.6), (2, 24, 1, 1, 1, 2, 0.5, 0.5),
         (3, 30, 4, 255, 32, 6, 0.6, 0.9), (4, 40, 3, 2, 2, 4, 0.3, 0.3), (5, 12, 4, 256, 4, 8, 0.5, 0.4)]
MIN_ACTIVE, MIN_UPDATE = 10, 15


def generate(seed, C, S, D, V, sigma, F):
    """the inputs of one file: -> emb (C, S, D) float32, active, clean (C, S) int32, seg (C, F, S) uint8"""
    rng = np.random.default_rng(seed)
    proto = rng.standard_normal((V, D))
    voice = rng.integers(0, V, (C, S))
    emb = np.float32(proto[voice] + sigma * rng.standard_normal((C, S, D)))
    active = rng.integers(0, 40, (C, S))
    clean = np.minimum(active, rng.integers(0, 40, (C, S)))
    emb[rng.random((C, S)) < 0.05] = 0
    emb[rng.random((C, S)) < 0.03, 0] = np.nan
    seg = rng.random((C, F, S)) < 0.6
    return emb, active.astype(np.int32), clean.astype(np.int32), seg.astype(np.uint8)


def synthetic_schedule(C, F, per_step, latency_steps, behind=2):
    """chunk c starts on frame c per_step; frames below start + F - (latency_steps - 1) per_step are due once it is in;
    the file has `behind` frames no chunk covers after its last chunk -> (schedule (C + 1, 3) int64, total)"""
    rows = np.empty((C + 1, 3), dtype=np.int64)
    emitted = 0
    for c in range(C):
        start = c * per_step
        bound = min(start + F, max(start + F - (latency_steps - 1) * per_step, 0))
        rows[c] = (start, emitted, max(bound, emitted))
        emitted = int(rows[c, 2])
    total = ((C - 1) * per_step + F if C else 0) + behind
    rows[C] = (-1, emitted, total)
    return rows, total


def streamed_schedule(C, F, duration, step, latency, frame_step, frame_duration, behind=2):
    """the same with the float64 frame arithmetic of a bank (`online_model.start_frame` / `emit_bound`)"""
    rows = np.empty((C + 1, 3), dtype=np.int64)
    emitted = 0
    for c in range(C):
        start = om.start_frame(c, step, frame_step, frame_duration)
        bound = min(om.emit_bound(c, step, duration, latency, frame_step, frame_duration), start + F)
        rows[c] = (start, emitted, max(bound, emitted))
        emitted = int(rows[c, 2])
    total = (int(rows[C - 1, 0]) + F if C else 0) + behind
    rows[C] = (-1, emitted, total)
    return rows, total


def smallest_ring(sched, F):
    """the smallest R the schedule's ring condition allows"""
    need = [int(g0) + F - int(ga) for g0, ga, _ in sched if g0 >= 0]
    return max([F] + need)
