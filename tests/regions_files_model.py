"""Numpy model of csrc/regions_files.hip: the region lists of every (file, class) from ONE scan over the concatenation
of the files' rows (TEST INFRASTRUCTURE ONLY; tests/test_detection_batch_cpu.py holds it to multilabel_oracle per file,
which shows that the scan-over-everything formulation is the per-file rule before any kernel runs).

What the model keeps of the kernels' formulation, and the per-file oracle does not have:
  * every row is a map on {inactive, active}, (image of inactive, image of active); padding rows are the identity, a
    file's frame 0 is a constant map; the state is carried through ALL rows and never reset;
  * a first frame is told that nothing comes before it, a last kept frame closes what is open;
  * per class the n-th on-event pairs with the n-th off-event over the whole concatenation, and the list of a file is
    found by counting the on-events in front of its first row;
  * times are those of the row's index in its own file.
`wrong` names one deliberate error (WRONG): the CPU test shows that its cases tell each from the right model."""
import numpy as np

PRECISION = 1e-6
ALIGN = 64
WRONG = ("no_first_frame", "no_last_frame", "global_times")


def layout(T):
    """row0 of files of T[f] frames: every file starts at the next multiple of 64"""
    owned = (np.asarray(T, dtype=np.int64) + ALIGN - 1) // ALIGN * ALIGN
    return np.concatenate([[0], np.cumsum(owned)]).astype(np.int32)


def pack(per_file, row0, fill=np.nan):
    """[(T[f], K)] -> (row0[-1], K) float32, `fill` in the padding rows"""
    K = per_file[0].shape[1]
    out = np.full((int(row0[-1]), K), fill, dtype=np.float32)
    for a, x in zip(row0[:-1], per_file):
        out[a:a + len(x)] = x
    return out


def _clean(rows, min_on, min_off):
    rows = [(a, b) for a, b in rows if (b - a) > PRECISION]
    positions = [0] * len(rows)
    if min_off > 0.0:
        merged = []
        for a, b in rows:
            gap = a - merged[-1][1] if merged else None
            if merged and (gap if gap > PRECISION else 0.0) < min_off:
                merged[-1] = (merged[-1][0], b)
            else:
                merged.append((a, b))
        rows, positions = merged, list(range(len(merged)))
    if min_on > 0.0:
        keep = [n for n, (a, b) in enumerate(rows) if not ((b - a if (b - a) > PRECISION else 0.0) < min_on)]
        rows, positions = [rows[n] for n in keep], [positions[n] for n in keep]
    return rows, positions


def regions_files(scores, row0, T, start, duration, step, onset, offset, min_duration_on, min_duration_off,
                  wrong=None):
    """scores (row0[-1], K) float32 -> per file, per class ([(start, end)], [track position])"""
    scores = np.asarray(scores, dtype=np.float32)
    rows, K = scores.shape
    N = len(T)
    spread = lambda v, t: np.broadcast_to(np.asarray(v, dtype=t), (K,))
    onset, offset = spread(onset, np.float32), spread(offset, np.float32)
    d_on, d_off = spread(min_duration_on, np.float64), spread(min_duration_off, np.float64)
    # where every row lies: (file, index in the file), -1 for padding
    file_of = np.full(rows, -1)
    local = np.zeros(rows, dtype=np.int64)
    for f in range(N):
        file_of[row0[f]:row0[f] + T[f]] = f
        local[row0[f]:row0[f + 1]] = np.arange(row0[f + 1] - row0[f])
    with np.errstate(invalid="ignore"):
        m0 = scores > onset                  # image of "inactive"
        m1 = ~(scores < offset)              # image of "active"
    first = (file_of >= 0) & (local == 0)
    if wrong != "no_first_frame":
        m1[first] = m0[first]
    pad = file_of < 0
    m0[pad], m1[pad] = False, True
    last = np.zeros(rows, dtype=bool)
    for f in range(N):
        if T[f] > 0 and wrong != "no_last_frame":
            last[row0[f] + T[f] - 1] = True
    middle = lambda i: 0.5 * ((float(start) + i * float(step)) + ((float(start) + i * float(step)) + float(duration)))
    out = [[None] * K for _ in range(N)]
    for k in range(K):
        state = False
        on_rows, off_rows = [], []
        for i in range(rows):
            before = state
            if first[i] and wrong != "no_first_frame":
                before = False
            after = m1[i, k] if before else m0[i, k]
            on, off = (not before) and after, before and not after
            if last[i]:
                on, off = False, before
            if pad[i]:
                on = off = False
            if on:
                on_rows.append(i)
            if off:
                off_rows.append(i)
            state = m1[i, k] if state else m0[i, k]          # the scan itself knows nothing of files
        assert len(on_rows) == len(off_rows) or wrong in ("no_last_frame", "no_first_frame")
        on_rows = np.asarray(on_rows, dtype=np.int64)
        index = (lambda i: i) if wrong == "global_times" else (lambda i: int(local[i]))
        pairs = [(middle(index(a)), middle(index(b))) for a, b in zip(on_rows, off_rows)]
        for f in range(N):
            lo = int(np.searchsorted(on_rows, row0[f]))          # on-events in front of the file's first row
            hi = int(np.searchsorted(on_rows, row0[f + 1]))
            out[f][k] = _clean(pairs[lo:hi], d_on[k], d_off[k])
    return out
