"""numpy model of the online diarization step (include/pyannote_amd_online.h): `cluster_step` and `emit` written from
their definition, one stream at a time.  Distances come from scipy.spatial.distance.cdist, the optimal map is a literal
enumeration of every tuple with float64 sums in the stated order and a plain min over (total, tuple).  The kernels are
held to these with `==`."""
import itertools

import numpy as np
from scipy.spatial.distance import cdist


def optimal_map(d, present, occupied, K):
    """d: (S, K) float64 (entries of present rows / occupied columns are read); -> tuple of S entries in [0, K], K =
    unmapped: exactly min(P, K_occ) present speakers mapped injectively to occupied centroids, smallest total (added in
    increasing s), ties -> the lexicographically smallest tuple."""
    S = len(present)
    occ = [k for k in range(K) if occupied[k]]
    need = min(int(np.sum(present)), len(occ))
    choices = [occ + [K] if present[s] else [K] for s in range(S)]
    best = None
    for tup in itertools.product(*choices):
        mapped = [k for k in tup if k < K]
        if len(mapped) != need or len(set(mapped)) != len(mapped):
            continue
        total = np.float64(0.0)
        for s in range(S):
            if tup[s] < K:
                total = total + d[s][tup[s]]
        if not total == total:   # a NaN total (a centroid of norm zero) never wins
            continue
        key = (float(total), tup)
        if best is None or key < best:
            best = key
    return best[1] if best is not None else tuple([K] * S)


def cluster_step_one(emb, active, clean, csum, cn, min_active, min_update, delta_new):
    """one stream: emb (S, D) float32, active / clean (S), csum (K, D) float64 and cn (K) int32 updated IN PLACE
    -> map (S) int32"""
    S, D = emb.shape
    K = cn.shape[0]
    e64 = emb.astype(np.float64)
    with np.errstate(all="ignore"):
        present = [bool(active[s] >= min_active and np.isfinite(emb[s]).all() and np.any(emb[s] != 0)) for s in range(S)]
    long_ = [present[s] and bool(clean[s] >= min_update) for s in range(S)]
    occupied = [bool(cn[k] > 0) for k in range(K)]
    d = np.full((S, K), np.nan)
    ps = [s for s in range(S) if present[s]]
    oc = [k for k in range(K) if occupied[k]]
    if ps and oc:
        with np.errstate(all="ignore"):
            d[np.ix_(ps, oc)] = cdist(e64[ps], csum[oc], "cosine")
    tup = optimal_map(d, present, occupied, K)
    out = np.full(S, -1, dtype=np.int32)
    matched = [False] * S
    held = set()
    for s in range(S):
        if tup[s] < K and not d[s][tup[s]] > delta_new:
            out[s], matched[s] = tup[s], True
            held.add(tup[s])
    taken = set(oc)
    founded, updates = [], []
    for s in ps:
        if matched[s]:
            if long_[s]:
                updates.append(s)
            continue
        free = [k for k in range(K) if k not in taken]
        if long_[s] and free:
            k = free[0]
            out[s] = k
            taken.add(k)
            held.add(k)
            founded.append(s)
            continue
        cands = [(d[s][k], k) for k in oc if k not in held]
        if cands:
            k = cands[0][1]
            for dk, kk in cands[1:]:
                if dk < d[s][k]:
                    k = kk
            out[s] = k
            held.add(k)
    for s in founded:
        csum[out[s]] = e64[s]
        cn[out[s]] = 1
    for s in updates:
        csum[out[s]] = csum[out[s]] + e64[s]
        cn[out[s]] = cn[out[s]] + 1
    return out


def cluster_step(slots, emb, active, clean, centroid_sum, centroid_n, min_active, min_update, delta_new):
    """the listed slots of a bank, state updated in place -> map (M, S) int32"""
    M, S, _ = emb.shape
    out = np.empty((M, S), dtype=np.int32)
    for m, slot in enumerate(slots):
        out[m] = cluster_step_one(emb[m], active[m], clean[m], centroid_sum[slot], centroid_n[slot], min_active,
                                  min_update, delta_new)
    return out


def emit_one(seg, mp, start, emit_from, emit_to, acc_sum, acc_cnt, E):
    """one stream: seg (F, S) uint8, mp (S), acc_sum (R, K) / acc_cnt (R) int32 updated in place -> out (E, K) uint8"""
    F, S = seg.shape
    R, K = acc_sum.shape
    for f in range(F if start >= 0 else 0):   # (start < 0: a flush, nothing is added)
        g = start + f
        if g < emit_from:      # emitted by an earlier call: its ring row belongs to frame g + R now
            continue
        acc_cnt[g % R] += 1
        for s in range(S):
            if 0 <= mp[s] < K and seg[f][s]:
                acc_sum[g % R][mp[s]] += 1
    out = np.zeros((E, K), dtype=np.uint8)
    for g in range(emit_from, emit_to):
        out[g - emit_from] = 2 * acc_sum[g % R] > acc_cnt[g % R]
        acc_sum[g % R] = 0
        acc_cnt[g % R] = 0
    return out


def emit(slots, seg, mp, start, emit_from, emit_to, acc_sum, acc_cnt, E):
    M = seg.shape[0]
    K = acc_sum.shape[2]
    out = np.empty((M, E, K), dtype=np.uint8)
    for m, slot in enumerate(slots):
        out[m] = emit_one(seg[m], mp[m], int(start[m]), int(emit_from[m]), int(emit_to[m]), acc_sum[slot],
                          acc_cnt[slot], E)
    return out


# ---------------------------------------------------------------------------------------------- geometry of a stream
def frame_of_time(t, frame_step, frame_duration):
    """frames.frame_geometry's float64 formula for the frame a chunk starting at time t starts on (chunks and frames
    start at 0; the half frame is added and taken off again as there, roundings included)"""
    half = 0.5 * np.float64(frame_duration)
    return int(np.rint((((0.0 + np.float64(t)) + half) - 0.0 - half) / np.float64(frame_step)))


def start_frame(c, step, frame_step, frame_duration):
    """global frame of frame 0 of chunk c"""
    return frame_of_time(np.float64(c) * np.float64(step), frame_step, frame_duration)


def emit_bound(c, step, duration, latency, frame_step, frame_duration):
    """frames below this one are emitted once chunk c is in: the start frame of time c step + duration - latency + step"""
    return frame_of_time(np.float64(c) * np.float64(step) + duration - latency + step, frame_step, frame_duration)
