"""numpy model of `pa_constrained_assign` (csrc/assign.hip), rule for rule: the rows that take part, the kept columns,
the order of the search, the totals (row order, float64) and the three reasons for a flag (a non-finite active row, a
runner-up within the margin, a gap within the margin between a row's last kept and first dropped column).  Shared by
tests/test_vbx_tuning_cpu.py (the model against SciPy; how many chunks the GPU test's inputs flag) and
tests/test_vbx_batch_gpu.py (the inputs themselves)."""
import itertools

import numpy as np

MARGIN = 1e-9
MAX_SPEAKERS, MAX_CLUSTERS = 4, 64
#: (chunks, local speakers, clusters) of the GPU test
SHAPES = ((1, 3, 1), (7, 3, 2), (64, 3, 3), (257, 3, 8), (33, 4, 5), (50, 2, 40))
#: share of the chunks of a random case that may go back to the host
FLAGGED_CAP = 0.05
#: the cases in which the two planted chunks (one NaN row, one exact tie) are themselves within the cap: there the cap
#: holds for ALL flagged chunks; in the smaller cases two chunks alone exceed 5 % and the cap is taken beyond them
CAP_COUNTS_PLANTED = ((64, 3, 3), (257, 3, 8))


def assign_model(soft: np.ndarray, silent: np.ndarray):
    """(hard (C, S) int8 with -2 for silent, unassigned and flagged rows; flagged (C) bool)"""
    C, S, K = soft.shape
    hard = np.full((C, S), -2, dtype=np.int8)
    flagged = np.zeros(C, dtype=bool)
    for c in range(C):
        rows = [s for s in range(S) if not silent[c, s]]
        A = len(rows)
        if A == 0:
            continue
        if not np.isfinite(soft[c, rows]).all():
            flagged[c] = True
            continue
        L = min(A, K)
        cols, vals, flag = [], [], False
        for r in rows:
            row = soft[c, r]
            taken = []
            for _ in range(L):
                best = -1
                for k in range(K):
                    if k not in taken and (best < 0 or row[k] > row[best]):
                        best = k
                taken.append(best)
            cols.append(taken)
            vals.append([row[k] for k in taken])
            if K > L:
                rest = max(row[k] for k in range(K) if k not in taken)
                flag |= bool(row[taken[-1]] - rest < MARGIN)
        best_total, second_total, best_choice = -np.inf, -np.inf, None
        # (the first row's choice runs fastest, as in the kernel's mixed-radix counter)
        for reverse in itertools.product(range(L + 1), repeat=A):
            choice = reverse[::-1]
            picked = [cols[a][l] for a, l in enumerate(choice) if l < L]
            if len(picked) != L or len(set(picked)) != len(picked):
                continue
            total = 0.0
            for a, l in enumerate(choice):
                if l < L:
                    total += vals[a][l]
            if total > best_total:
                best_total, second_total, best_choice = total, best_total, choice
            elif total > second_total:
                second_total = total
        flag |= bool(best_total - second_total < MARGIN)
        flagged[c] = flag
        if not flag:
            for a, l in enumerate(best_choice):
                if l < L:
                    hard[c, rows[a]] = cols[a][l]
    return hard, flagged


def host_assign(soft_after_silencing: np.ndarray, silent: np.ndarray) -> np.ndarray:
    """the contract's right-hand side: `constrained_argmax` (clustering.py) on the silenced scores, silent rows -2"""
    from scipy.optimize import linear_sum_assignment
    scores = np.nan_to_num(soft_after_silencing, nan=np.nanmin(soft_after_silencing))
    hard = np.full(scores.shape[:2], -2, dtype=np.int8)
    for c, cost in enumerate(scores):
        speakers, clusters = linear_sum_assignment(cost, maximize=True)
        hard[c, speakers] = clusters
    return np.where(silent, -2, hard).astype(np.int8)


def random_case(C: int, S: int, K: int, seed: int, planted: bool = True):
    """(soft after silencing (C, S, K), silent (C, S), chunks that must be flagged): cosine-like scores in [0, 2]
    with about a quarter of the rows silent and, where the case has room, a fully silent chunk, one active row of
    NaN and one exact tie (two active rows equal in their two best columns)"""
    rng = np.random.default_rng(seed)
    soft = rng.uniform(0.0, 2.0, size=(C, S, K))
    silent = rng.uniform(size=(C, S)) < 0.25
    must = []
    if planted and C >= 7:
        silent[0] = True                                  # a fully silent chunk
        silent[1] = False
        soft[1, 0] = np.nan                               # an active speaker whose embedding is NaN
        must.append(1)
        if K >= 2:
            silent[2] = False                             # rows 0 and 1 tie: swapping their columns changes nothing
            soft[2, :2] = 0.25
            soft[2, :2, :2] = 1.75
            must.append(2)
    silenced = soft.copy()
    silenced[silent] = np.nanmin(soft) - 1.0
    return silenced, silent, must
