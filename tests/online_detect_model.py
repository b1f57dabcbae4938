"""numpy model of the online detection step (`pao_detect_step`, include/pyannote_amd_online.h): rule items 1 - 5 written
from their statement, one stream, one class and one frame at a time (TEST INFRASTRUCTURE ONLY).

tests/test_online_detect_model_cpu.py pins the streaming formulation to the offline one -- `frames_model.aggregate`
on all chunks followed by `multilabel_oracle.all_regions` -- before any kernel runs; tests/test_online_detect_gpu.py
holds the kernel to this model with `==`."""
import numpy as np

PRECISION = 1e-6
STATE = (("acc", np.float32, "RK"), ("cnt", np.float32, "RK"), ("msk", np.uint8, "RK"), ("on", np.uint8, "K"),
         ("open_start", np.float64, "K"), ("pend", np.float64, "K2"), ("has_pend", np.uint8, "K"),
         ("n_merged", np.int32, "K"))


def fresh_state(N, R, K):
    """the state of a bank of N fresh streams: zeros"""
    dims = {"RK": (N, R, K), "K": (N, K), "K2": (N, K, 2)}
    return {name: np.zeros(dims[shape], dtype=dtype) for name, dtype, shape in STATE}


def copy_state(state):
    return {name: a.copy() for name, a in state.items()}


def same_state(a, b):
    """bit for bit (NaN included)"""
    return all(a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes() for name, _, _ in STATE)


def frame_time(g, start, duration, step):
    """the middle of frame g, in the host's float64 expression"""
    s = float(start) + g * float(step)
    return 0.5 * (s + (s + float(duration)))


def duration_of(a, b):
    """pyannote.core's Segment.duration: 0 for segments not longer than the precision"""
    return (b - a) if (b - a) > PRECISION else 0.0


def chunk_values(scores, any):
    """scores (F, S) float32 or uint8 -> (F, K) float32: hard decisions count as 0 / 1; with `any` the np.max over the
    columns (NaN if one of them is)"""
    scores = np.asarray(scores)
    x = (scores != 0).astype(np.float32) if scores.dtype == np.uint8 else scores.astype(np.float32)
    return np.max(x, axis=-1, keepdims=True) if any else x


class _Class:
    """items 3 - 5 for one class of one stream: the state it carries and the regions one call finalises"""

    def __init__(self, state, slot, k, min_on, min_off):
        self.state, self.slot, self.k, self.min_on, self.min_off = state, slot, k, float(min_on), float(min_off)
        self.regions, self.tracks = [], []

    def get(self, name):
        return self.state[name][self.slot, self.k]

    def put(self, name, value):
        self.state[name][self.slot, self.k] = value

    def finalise(self):
        s, e = (float(v) for v in self.get("pend"))
        if not (self.min_on > 0.0 and duration_of(s, e) < self.min_on):
            self.regions.append((s, e))
            self.tracks.append(int(self.get("n_merged")) - 1 if self.min_off > 0.0 else 0)
        self.put("has_pend", 0)

    def opens(self, t):
        self.put("open_start", t)
        if self.get("has_pend") and not (self.min_off > 0.0 and duration_of(float(self.get("pend")[1]), t) < self.min_off):
            self.finalise()

    def closes(self, e):
        s = float(self.get("open_start"))
        if not (e - s > PRECISION):
            return
        if self.get("has_pend") and self.min_off > 0.0 and duration_of(float(self.get("pend")[1]), s) < self.min_off:
            self.state["pend"][self.slot, self.k, 1] = e
        else:
            if self.get("has_pend"):
                self.finalise()
            self.put("pend", (s, e))
            self.put("has_pend", 1)
            self.put("n_merged", self.get("n_merged") + 1)
        if not self.min_off > 0.0:
            self.finalise()


def detect_step_one(state, slot, scores, any, window, warm, epsilon, missing, start_frame, emit_from, emit_to, closing,
                    grid, onset, offset, min_on, min_off, E, cap):
    """one stream: scores (F, S), state[...][slot] updated IN PLACE -> values (E, K) float32, active (E, K) uint8,
    counts (K) int32, regions (K, cap, 2) float64, tracks (K, cap) int32"""
    x = chunk_values(scores, any)
    F, K = x.shape
    R = state["acc"].shape[1]
    g0, ga, gb = int(start_frame), int(emit_from), int(emit_to)
    assert 0 <= ga <= gb and gb - ga <= E and R >= F + E and (g0 < 0 or g0 + F - ga <= R) and cap >= E // 2 + 2
    acc, cnt, msk = state["acc"][slot], state["cnt"][slot], state["msk"][slot]
    # 1. overlap-add: float32 accumulators, every addition in float64 (numpy's `float32_array += float64_array`)
    for f in range(F if g0 >= 0 else 0):
        g = g0 + f
        if g < ga:
            continue
        r = g % R
        for k in range(K):
            nan = bool(np.isnan(x[f, k]))
            m = 0.0 if nan else 1.0
            score = np.float64(0.0 if nan else x[f, k])
            acc[r, k] = np.float32(np.float64(acc[r, k]) + ((score * m) * np.float64(window[f])) * np.float64(warm[f]))
            cnt[r, k] = np.float32(np.float64(cnt[r, k]) + (m * np.float64(window[f])) * np.float64(warm[f]))
            msk[r, k] = max(msk[r, k], 0 if nan else 1)
    # 2. emission
    values = np.full((E, K), np.nan, dtype=np.float32)
    for g in range(ga, gb):
        r = g % R
        for k in range(K):
            v = acc[r, k] / np.maximum(cnt[r, k], np.float32(epsilon))
            values[g - ga, k] = np.float32(missing) if msk[r, k] == 0 else v
        acc[r], cnt[r], msk[r] = 0, 0, 0
    # 3 - 5. per class
    active = np.zeros((E, K), dtype=np.uint8)
    counts = np.zeros(K, dtype=np.int32)
    regions = np.full((K, cap, 2), np.nan, dtype=np.float64)
    tracks = np.full((K, cap), -1, dtype=np.int32)
    for k in range(K):
        c = _Class(state, slot, k, min_on[k], min_off[k])
        on32, off32 = np.float32(onset[k]), np.float32(offset[k])
        on = bool(state["on"][slot, k])
        for g in range(ga, gb):
            v = values[g - ga, k]
            before = False if g == 0 else on
            after = (not v < off32) if before else bool(v > on32)
            if not before and after:
                c.opens(frame_time(g, *grid))
            if before and not after:
                c.closes(frame_time(g, *grid))
            on = after
            active[g - ga, k] = on
        if closing:
            if on:
                c.closes(frame_time(gb - 1, *grid))
            on = False
            if c.get("has_pend"):
                c.finalise()
        state["on"][slot, k] = on
        assert len(c.regions) <= cap
        counts[k] = len(c.regions)
        regions[k, :len(c.regions)] = np.asarray(c.regions, dtype=np.float64).reshape(-1, 2)
        tracks[k, :len(c.tracks)] = c.tracks
    return values, active, counts, regions, tracks


def detect_step(state, slots, scores, any, window, warm, epsilon, missing, start_frame, emit_from, emit_to, closing, grid,
                onset, offset, min_on, min_off, E, cap):
    """the listed slots of a bank -> values (M, E, K), active (M, E, K), counts (M, K), regions (M, K, cap, 2),
    tracks (M, K, cap)"""
    outs = [detect_step_one(state, int(slot), scores[m], any, window, warm, epsilon, missing, start_frame[m],
                            emit_from[m], emit_to[m], closing[m], grid, onset, offset, min_on, min_off, E, cap)
            for m, slot in enumerate(slots)]
    return tuple(np.stack(part) for part in zip(*outs))


def stream_file(scores, schedule, any, window, warm, epsilon, missing, grid, onset, offset, min_on, min_off, R=None):
    """A whole recording through a fresh slot: scores (C, F, S), schedule (C + 1, 3) as `online.file_schedule` gives it
    (the flush row last); the last row that emits or adds something carries `closing`.  -> (values (total, K),
    active (total, K), per class ([(start, end)], [track]), per call (emit_from, emit_to))"""
    C, F, _ = scores.shape
    K = 1 if any else scores.shape[2]
    schedule = np.asarray(schedule, dtype=np.int64)
    E = max(1, int((schedule[:, 2] - schedule[:, 1]).max()))
    R = F + E if R is None else R
    state = fresh_state(1, R, K)
    values, active, calls = [], [], []
    per_class = [([], []) for _ in range(K)]
    for c in range(C + 1):
        g0, ga, gb = (int(v) for v in schedule[c])
        chunk = scores[c] if c < C else np.zeros((F, scores.shape[2]), dtype=scores.dtype)
        v, a, n, regions, tracks = detect_step_one(state, 0, chunk, any, window, warm, epsilon, missing, g0, ga, gb,
                                                   c == C, grid, onset, offset, min_on, min_off, E, E // 2 + 2)
        values.append(v[:gb - ga])
        active.append(a[:gb - ga])
        calls.append((ga, gb))
        for k in range(K):
            per_class[k][0].extend((float(s), float(e)) for s, e in regions[k, :n[k]])
            per_class[k][1].extend(int(t) for t in tracks[k, :n[k]])
    # (the ring may still hold the padding of a zero-padded last chunk: frames past the stream's total)
    assert not state["has_pend"].any() and not state["on"].any()
    return np.concatenate(values), np.concatenate(active), per_class, calls
