"""Truth for pyannote_audio_amd.metrics: the definitions of csrc/metrics.hip's counts in plain numpy int64, with
scipy's Hungarian assignment for the speaker mappings.  Every comparison against this file is `==`.

The `torch_*` functions at the end restate the same definitions as plain torch ops; tools/bench_metrics.py times
them on the GPU beside the fused kernels."""
import itertools

import numpy as np
from scipy.optimize import linear_sum_assignment


# ------------------------------------------------------------------------------------------------ file mode
def der_counts(reference, hypothesis, keep=None) -> dict:
    """(T, Sr), (T, Sh) 0/1 arrays (+ optional (T,) mask of the frames that count) -> the counts of `pa_der_counts`
    under the keys of `pyannote_audio_amd.metrics.der_counts`"""
    r = (np.asarray(reference) != 0).astype(np.int64)
    h = (np.asarray(hypothesis) != 0).astype(np.int64)
    if r.shape[1] == 0:
        r = np.zeros((r.shape[0], 1), dtype=np.int64)
    if h.shape[1] == 0:
        h = np.zeros((h.shape[0], 1), dtype=np.int64)
    if keep is not None:
        on = np.asarray(keep).reshape(-1) != 0
        r, h = r[on], h[on]
    nr, nh = r.sum(axis=1), h.sum(axis=1)
    return {"cooc": r.T @ h, "ref_frames": r.sum(axis=0), "hyp_frames": h.sum(axis=0),
            "total": int(nr.sum()), "false_alarm": int(np.maximum(0, nh - nr).sum()),
            "missed": int(np.maximum(0, nr - nh).sum()), "both": int(np.minimum(nr, nh).sum())}


def file_components(reference, hypothesis, keep=None) -> dict:
    """the reference's four components (Python ints) by its own formula: pad to a common number of speakers, map the
    hypothesis one-to-one onto the reference so that the matched co-occurrence is maximal, then
    confusion = sum((h != r) * h) - false_alarm"""
    r = (np.asarray(reference) != 0).astype(np.int64)
    h = (np.asarray(hypothesis) != 0).astype(np.int64)
    if keep is not None:
        on = np.asarray(keep).reshape(-1) != 0
        r, h = r[on], h[on]
    S = max(r.shape[1], h.shape[1], 1)
    r = np.pad(r, ((0, 0), (0, S - r.shape[1])))
    h = np.pad(h, ((0, 0), (0, S - h.shape[1])))
    rows, cols = linear_sum_assignment(-(r.T @ h))
    mapped = np.zeros_like(h)
    mapped[:, rows] = h[:, cols]
    detection_error = mapped.sum(axis=1) - r.sum(axis=1)
    false_alarm = np.maximum(0, detection_error)
    missed = np.maximum(0, -detection_error)
    confusion = ((mapped != r) * mapped).sum(axis=1) - false_alarm
    return {"false alarm": int(false_alarm.sum()), "missed detection": int(missed.sum()),
            "confusion": int(confusion.sum()), "total": int(r.sum())}


# ----------------------------------------------------------------------------------------------- chunk mode
def chunk_costs(preds, target) -> np.ndarray:
    """(B, S, F) scores and 0/1 targets -> (B, S, S) float64: cost[b, i, j] = mean_f (target_i - preds_j)^2"""
    p = np.asarray(preds, dtype=np.float64)
    t = (np.asarray(target) != 0).astype(np.float64)
    out = np.empty((p.shape[0], p.shape[1], p.shape[1]), dtype=np.float64)
    for i in range(p.shape[1]):
        d = t[:, i:i + 1, :] - p
        out[:, i, :] = np.mean(d * d, axis=2)
    return out


TIE = 1e-12      # permutation costs (<= S) closer than this are equal up to the rounding of a float64 sum


def chunk_permutations(preds, target):
    """-> perm (B, S) int32 (score row perm[b, i] plays target speaker i: the cheapest assignment on the float64
    cost), gap (B,) float64 = the cost of the cheapest permutation that is NOT tied with the best one, minus the
    best (inf when there is none), and tied (B,) = how many other permutations tie with the best (within `TIE`:
    duplicated rows).  Enumerated, so S <= 6."""
    cost = chunk_costs(preds, target)
    B, S, _ = cost.shape
    perm = np.empty((B, S), dtype=np.int32)
    for b in range(B):
        rows, cols = linear_sum_assignment(cost[b])
        perm[b, rows] = cols
    sums = np.stack([cost[:, np.arange(S), list(sigma)].sum(axis=1) for sigma in itertools.permutations(range(S))],
                    axis=1)
    excess = sums - sums.min(axis=1, keepdims=True)
    tied = (excess <= TIE).sum(axis=1) - 1
    gap = np.where(excess > TIE, excess, np.inf).min(axis=1)
    return perm, gap, tied


def chunk_components(preds, target, thresholds, perm=None):
    """-> counts (B, Q, 3) int64 = false alarm, missed detection, confusion per chunk and threshold, total (B,)
    int64.  Hypothesis at threshold q = mapped score > float32(threshold q), compared in float32; confusion by
    the reference's formula sum((h != t) * h) - false_alarm."""
    p = np.asarray(preds, dtype=np.float32)
    t = (np.asarray(target) != 0).astype(np.int64)
    thresholds = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    B, S, F = p.shape
    if perm is None:
        perm = chunk_permutations(p, t)[0]
    perm = np.asarray(perm)
    mapped = np.take_along_axis(p, np.maximum(perm, 0)[:, :, None].astype(np.int64), axis=1)
    mapped = np.where((perm >= 0)[:, :, None], mapped, np.float32(0))
    nr = t.sum(axis=1)
    counts = np.empty((B, len(thresholds), 3), dtype=np.int64)
    for q, thr in enumerate(thresholds):
        h = (mapped > thr).astype(np.int64)
        detection_error = h.sum(axis=1) - nr
        false_alarm = np.maximum(0, detection_error)
        counts[:, q, 0] = false_alarm.sum(axis=1)
        counts[:, q, 1] = np.maximum(0, -detection_error).sum(axis=1)
        counts[:, q, 2] = (((h != t) * h).sum(axis=1) - false_alarm).sum(axis=1)
    return counts, nr.sum(axis=1)


def permutation_margin(num_speakers: int, num_frames: int) -> float:
    """Below this float64 gap between the two cheapest permutations of a chunk, a float32 cost (the reference's) may
    rank them the other way round.  With u = 2^-24 and scores in [0, 1] (every squared difference <= 1): a float32
    term fl(fl(t - p)^2) carries a relative error <= 2 u, summing F of them in any order adds <= (F - 1) u, the
    division by F one more u, so a cost entry (<= 1) is off by <= (F + 2) u.  A permutation's cost is S entries
    (added in float64 by scipy), and two permutations are compared: 2 S (F + 2) u."""
    return 2.0 * num_speakers * (num_frames + 2) * 2.0 ** -24


# ------------------------------------------------------------------ the same definitions as plain torch ops
def torch_file_counts(reference, hypothesis):
    """`der_counts` as torch ops on the tensors' device: (cooc, total, false_alarm, missed, both) int64 tensors"""
    import torch
    r, h = (reference != 0).to(torch.int64), (hypothesis != 0).to(torch.int64)
    nr, nh = r.sum(dim=1), h.sum(dim=1)
    cooc = (r.to(torch.float64).T @ h.to(torch.float64)).to(torch.int64)    # (exact: counts < 2^53)
    return (cooc, nr.sum(), torch.clamp(nh - nr, min=0).sum(), torch.clamp(nr - nh, min=0).sum(),
            torch.minimum(nr, nh).sum())


def torch_chunk_counts(preds, target, thresholds, perm):
    """`chunk_components` as torch ops, the way the definition reads: a (B, S, F, Q) hypothesis.  `perm` (B, S)
    int64 is given (the assignment itself is host work in every formulation)."""
    import torch
    mapped = torch.gather(preds, 1, perm[:, :, None].expand(-1, -1, preds.shape[2]))
    h = (mapped.unsqueeze(-1) > thresholds).to(torch.int32)
    t = (target != 0).to(torch.int32).unsqueeze(-1)
    detection_error = h.sum(dim=1) - t.sum(dim=1)
    false_alarm = torch.clamp(detection_error, min=0)
    missed = torch.clamp(-detection_error, min=0)
    confusion = ((h != t).to(torch.int32) * h).sum(dim=1) - false_alarm
    counts = torch.stack([false_alarm.sum(dim=1), missed.sum(dim=1), confusion.sum(dim=1)], dim=-1)
    return counts.to(torch.int64), t.sum(dim=(1, 2, 3)).to(torch.int64)
