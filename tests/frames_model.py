"""Plain restatements of the frame-domain kernels (csrc/frames.hip) and the cases they are held to.

Each function states one entry point's contract (include/pyannote_amd.h) as the obvious loops over (chunk, frame,
speaker) in numpy / Python, following the reference lines that frames.hip cites.  tests/test_frames_model_cpu.py pins
them to oracle.pipeline on regular chunk grids; tests/test_frames_kernels_gpu.py holds the kernels to them, bit for bit,
through the C ABI.  Nothing here touches the GPU or the product package.

Every function takes `wrong`: the name of one deliberate error (WRONG lists them per operation).  It exists for
test_frames_model_cpu alone, which shows that the case lists below tell each of these wrong kernels from a right one;
the GPU tests never pass it.

The case lists are data: `*_cases()` return lists of dicts (an "id" and the arguments), built once per process from
fixed seeds and never modified by their users."""
import functools
import itertools

import numpy as np

#: the deliberate errors each model function knows (see the module docstring)
WRONG = {
    "chunk_stats": ("clean_counts_overlap",),
    "embedding_masks": ("use_clean_ge",),
    "speaker_count": ("half_away", "clamp_frames"),
    "cluster_activations": ("count_every_speaker", "wrap_hard", "clamp_frames"),
    "topk_i32": ("highest_index", "tie_never", "tie_when_full"),
    "topk_f32": ("highest_index", "tie_never", "tie_when_full"),
    "hysteresis": ("midpoint_f32", "nan_first_kept"),
    "cluster_max": ("ignore_nan",),
    "aggregate": ("accumulate_f64", "missing_zero"),
}


# ------------------------------------------------------------------------------------------------- the models
def chunk_stats(seg, wrong=None):
    """seg (C, F, S) uint8 -> active (C, S) int32 = frames speaker s is on, clean (C, S) int32 = frames it is on
    alone (pipelines/clustering.py:109-116)"""
    C, F, S = seg.shape
    active = np.zeros((C, S), dtype=np.int32)
    clean = np.zeros((C, S), dtype=np.int32)
    for c in range(C):
        for f in range(F):
            tot = int(seg[c, f].sum())
            alone = tot >= 1 if wrong == "clean_counts_overlap" else tot == 1
            for s in range(S):
                active[c, s] += seg[c, f, s]
                if alone:
                    clean[c, s] += seg[c, f, s]
    return active, clean


def embedding_masks(seg, clean, exclude_overlap, min_num_frames, wrong=None):
    """-> masks (C, S, F) float32: the speaker's frames without those where two or more speak, where exclude_overlap
    and clean[c][s] > min_num_frames (strictly); all its frames otherwise (pipelines/speaker_diarization.py:375-427)"""
    C, F, S = seg.shape
    masks = np.zeros((C, S, F), dtype=np.float32)
    for c in range(C):
        for s in range(S):
            enough = clean[c, s] >= min_num_frames if wrong == "use_clean_ge" else clean[c, s] > min_num_frames
            use_clean = bool(exclude_overlap) and enough
            for f in range(F):
                overlapped = int(seg[c, f].sum()) >= 2
                masks[c, s, f] = 0.0 if (use_clean and overlapped) else float(seg[c, f, s])
    return masks


def _global_frame(t, T, wrong):
    """the global frame a chunk frame lands on, None where it is dropped"""
    if wrong == "clamp_frames":
        return min(max(t, 0), T - 1)
    return t if 0 <= t < T else None


def speaker_count(seg, start, T, wrong=None):
    """-> count (T) uint8 = rint(float32 sum of active speakers / float32 number of covering chunks), 0 where no chunk
    covers the frame; chunk frames outside [0, T) are dropped (pipelines/utils/diarization.py:150-185)"""
    C, F, S = seg.shape
    total = np.zeros(T, dtype=np.int64)
    covering = np.zeros(T, dtype=np.int64)
    for c in range(C):
        for f in range(F):
            t = _global_frame(int(start[c]) + f, T, wrong)
            if t is None:
                continue
            total[t] += int(seg[c, f].sum())
            covering[t] += 1
    count = np.zeros(T, dtype=np.uint8)
    for t in range(T):
        if covering[t] > 0:
            average = np.float32(total[t]) / np.float32(covering[t])
            if wrong == "half_away":
                count[t] = np.uint8(np.floor(np.float64(average) + 0.5))
            else:
                count[t] = np.uint8(np.rint(average))
    return count


def cluster_activations(seg, start, hard, K, T, wrong=None):
    """-> act (T, K) int32: per global frame and cluster the number of chunks in which a local speaker of that cluster
    is active -- ONE per (chunk, frame, cluster) however many of its speakers are; hard outside [0, K) is no cluster
    (pipelines/speaker_diarization.py:480-528 + the overlap SUM of to_diarization)"""
    C, F, S = seg.shape
    act = np.zeros((T, K), dtype=np.int32)
    for c in range(C):
        for f in range(F):
            t = _global_frame(int(start[c]) + f, T, wrong)
            if t is None:
                continue
            seen = set()
            for s in range(S):
                k = int(hard[c, s])
                if wrong == "wrap_hard" and k >= K:
                    k %= K
                if k < 0 or k >= K or not seg[c, f, s]:
                    continue
                if k in seen and wrong != "count_every_speaker":
                    continue
                seen.add(k)
                act[t, k] += 1
    return act


def topk(act, count, cap, wrong=None):
    """act (T, K) int32 or float32 (>= 0, no NaN), count (T) uint8 -> out (T, K) uint8, tie (T) uint8.
    n = min(count, cap, K) clusters are selected, largest first, equal values by lowest index; tie = 1 iff 0 < n < K
    and an unselected cluster equals the last selected value (pipelines/utils/diarization.py:250-266)"""
    T, K = act.shape
    out = np.zeros((T, K), dtype=np.uint8)
    tie = np.zeros(T, dtype=np.uint8)
    sign = -1 if wrong == "highest_index" else 1
    for t in range(T):
        row = act[t].tolist()
        n = min(int(count[t]), int(cap), K)
        order = sorted(range(K), key=lambda k: (-row[k], sign * k))
        for k in order[:n]:
            out[t, k] = 1
        if n == 0 or wrong == "tie_never":
            continue
        last = row[order[n - 1]]
        if n < K:
            tie[t] = any(row[k] == last for k in order[n:])
        elif wrong == "tie_when_full":          # looks for the last value among the selected clusters too
            tie[t] = any(row[k] == last for k in order[:n - 1])
    return out, tie


def hysteresis_midpoint(onset, offset):
    """the reference's threshold for the initial state (utils/signal.py:111): 0.5 * (onset + offset) on Python
    doubles, which numpy rounds ONCE to float32 when it compares float32 scores with it"""
    return np.float32(0.5 * (float(onset) + float(offset)))


def hysteresis(scores, onset, offset, initial_state, wrong=None):
    """scores (C, F, K) float32, onset / offset Python floats, initial_state 0 / 1 / -1 -> (C, F, K) uint8: per
    (chunk, class) on where score > onset, off where score < offset, unchanged in between (float32 comparisons); NaN
    counts as 0; -1 starts from scores[:, 0] >= midpoint (utils/signal.py:78-140).
    (The frame loop is the state machine; the rows, which do not interact, are taken together.)"""
    C, F, K = scores.shape
    on32, off32 = np.float32(onset), np.float32(offset)
    mid32 = hysteresis_midpoint(onset, offset)
    if wrong == "midpoint_f32":
        mid32 = np.float32(0.5) * (on32 + off32)
    data = np.where(np.isnan(scores), np.float32(0.0), scores).astype(np.float32)
    first = scores[:, 0, :] if wrong == "nan_first_kept" else data[:, 0, :]
    if initial_state < 0:
        with np.errstate(invalid="ignore"):
            state = first >= mid32
    else:
        state = np.full((C, K), initial_state != 0)
    out = np.zeros((C, F, K), dtype=np.uint8)
    for f in range(F):
        s = data[:, f, :]
        state = np.where(s > on32, True, np.where(s < off32, False, state))
        out[:, f, :] = state
    return out


def cluster_max(scores, hard, K, wrong=None):
    """scores (C, F, S) float32 -> (C, F, K) float32: np.max over the local speakers of cluster k (NaN propagates),
    NaN where the chunk has none (pipelines/speaker_diarization.py:506-522)"""
    C, F, S = scores.shape
    out = np.full((C, F, K), np.nan, dtype=np.float32)
    for c in range(C):
        for k in range(K):
            members = [s for s in range(S) if int(hard[c, s]) == k]
            if not members:
                continue
            for f in range(F):
                values = scores[c, f, members]
                if wrong == "ignore_nan" and not np.isnan(values).all():
                    out[c, f, k] = np.nanmax(values)
                else:
                    out[c, f, k] = np.max(values)
    return out


def aggregate(scores, start, T, window, warm, epsilon, missing, skip_average, wrong=None):
    """Inference.aggregate's chunk loop (core/inference.py:498-620) on a table of start frames: scores (C, F, K)
    float32 (NaN = missing), window / warm (F) float64, every chunk inside [0, T) -> (T, K) float32.  float32
    accumulators, `+=` of the float64 products ((score * mask) * window) * warm."""
    C, F, K = scores.shape
    acc = np.float64 if wrong == "accumulate_f64" else np.float32
    aggregated = np.zeros((T, K), dtype=acc)
    weight = np.zeros((T, K), dtype=acc)
    voted = np.zeros((T, K), dtype=np.float32)
    window, warm = np.asarray(window, dtype=np.float64).reshape(F, 1), np.asarray(warm, dtype=np.float64).reshape(F, 1)
    for c in range(C):
        assert 0 <= start[c] and start[c] + F <= T
        score = np.array(scores[c])
        mask = 1 - np.isnan(score)
        np.nan_to_num(score, copy=False, nan=0.0)
        frames = slice(int(start[c]), int(start[c]) + F)
        aggregated[frames] += score * mask * window * warm
        weight[frames] += mask * window * warm
        voted[frames] = np.maximum(voted[frames], mask)
    aggregated, weight = aggregated.astype(np.float32), weight.astype(np.float32)
    average = aggregated if skip_average else aggregated / np.maximum(weight, np.float32(epsilon))
    average[voted == 0.0] = 0.0 if wrong == "missing_zero" else missing
    return average


# ------------------------------------------------------------------------------------------------- the cases
def _segmentation(rng, C, F, S, density=0.45):
    """(C, F, S) uint8 {0, 1}: runs of activity, so that frames with none, one and several speakers all occur"""
    seg = (rng.uniform(size=(C, F, S)) < density).astype(np.uint8)
    for c in range(C):
        for s in range(S):
            if F > 4 and rng.uniform() < 0.5:
                a = int(rng.integers(0, F))
                seg[c, a:a + int(rng.integers(1, F)), s] = rng.integers(0, 2)
    return seg


@functools.lru_cache(maxsize=None)
def chunk_stats_cases():
    """S = 1..8, F on both sides of the block size and its multiples, one chunk and several"""
    cases = []
    for S, F, C in itertools.product(range(1, 9), (1, 63, 255, 256, 257, 589), (1, 3)):
        rng = np.random.default_rng(1000 * S + 10 * F + C)
        cases.append({"id": f"S{S}-F{F}-C{C}", "seg": _segmentation(rng, C, F, S)})
    return cases


@functools.lru_cache(maxsize=None)
def embedding_masks_cases():
    """every chunk_stats case with exclude_overlap 0 / 1 and min_num_frames -1, 0 and the exact `clean` of one pair
    -- a pair that also has overlapped frames where there is one, so that `>` and `>=` give different masks"""
    cases = []
    for base in chunk_stats_cases():
        seg = base["seg"]
        active, clean = chunk_stats(seg)
        C, F, S = seg.shape
        pairs = [(c, s) for c in range(C) for s in range(S) if clean[c, s] < active[c, s]]
        c, s = pairs[0] if pairs else (C - 1, S - 1)
        for exclude, min_num_frames in itertools.product((0, 1), (-1, 0, int(clean[c, s]))):
            cases.append({"id": f"{base['id']}-ex{exclude}-min{min_num_frames}", "seg": seg, "clean": clean,
                          "exclude_overlap": exclude, "min_num_frames": min_num_frames})
    return cases


#: (name, T, F, start frames): a negative first start, two chunks with the same start, a gap no chunk covers and a last
#: chunk that runs past T in every irregular table; F = 300 takes two blocks of 256 frames per chunk
START_TABLES = (
    ("T1", 1, 3, (-1, -1, 0, 0)),
    ("T255", 255, 63, (-10, 20, 20, 60, 150, 230)),
    ("T257", 257, 300, (-290, -290, 40)),
    ("T700", 700, 100, (-30, 40, 40, 110, 400, 650)),
    ("T700-regular", 700, 589, (0, 59, 111)),
)


def _sums_segmentation(sums, S):
    """(C, F, S) uint8 whose frame (c, f) has sums[c][f] active speakers"""
    sums = np.asarray(sums)
    seg = np.zeros(sums.shape + (S,), dtype=np.uint8)
    for c, f in np.ndindex(*sums.shape):
        seg[c, f, :sums[c, f]] = 1
    return seg


@functools.lru_cache(maxsize=None)
def speaker_count_cases():
    cases = []
    for name, T, F, starts in START_TABLES:
        for S in (1, 3, 8):
            rng = np.random.default_rng(7 * T + F + S)
            cases.append({"id": f"{name}-S{S}", "seg": _segmentation(rng, len(starts), F, S),
                          "start": np.array(starts, dtype=np.int32), "T": T})
    cases.append({"id": "no-chunk", "seg": np.zeros((0, 63, 3), dtype=np.uint8), "start": np.zeros(0, dtype=np.int32),
                  "T": 255})
    # averages on the rounding knife edge: n = 2 chunks give 0.5 1.5 2.5 3.5 (and 0 1 2 3), n = 4 the same halves and
    # the quarters, n = 3 the thirds
    halves2 = [[0, 1, 2, 3, 0, 1, 2, 3], [1, 2, 3, 4, 0, 1, 2, 3]]
    halves4 = [[0, 1, 2, 3, 0, 0, 1, 1], [0, 1, 2, 3, 0, 1, 1, 2], [1, 2, 3, 4, 0, 1, 1, 2], [1, 2, 3, 4, 1, 1, 2, 2]]
    thirds = [[0, 0, 1, 1, 2, 2, 3, 4], [0, 1, 1, 2, 2, 3, 3, 4], [1, 1, 2, 2, 3, 3, 4, 4]]
    for name, sums in (("halves-n2", halves2), ("halves-n4", halves4), ("thirds-n3", thirds)):
        cases.append({"id": name, "seg": _sums_segmentation(sums, 4), "start": np.zeros(len(sums), dtype=np.int32),
                      "T": 8})
    return cases


@functools.lru_cache(maxsize=None)
def cluster_activations_cases():
    """the start tables of speaker_count, S up to 8, K = 1, 2, 7, 20; `hard` holds -2, -1, K and K + 3 next to valid
    clusters, and with S = 8 several active local speakers share a cluster (at least three of them for K <= 2)"""
    cases = []
    for (name, T, F, starts), S, K in itertools.product(START_TABLES, (1, 3, 8), (1, 2, 7, 20)):
        rng = np.random.default_rng(31 * T + 7 * F + 3 * S + K)
        C = len(starts)
        hard = rng.integers(0, K, size=(C, S)).astype(np.int32)
        outside = np.array([-2, K, -1, K + 3], dtype=np.int32)
        where = rng.permutation(C * S)[:min(4, C * S - 1)]
        hard.reshape(-1)[where] = outside[:len(where)]
        cases.append({"id": f"{name}-S{S}-K{K}", "seg": _segmentation(rng, C, F, S, density=0.6),
                      "start": np.array(starts, dtype=np.int32), "hard": hard, "K": K, "T": T})
    return cases


def _topk_cases(dtype):
    cases = []
    scale = 1 if dtype == np.int32 else 0.25
    for T, K, cap, kind in itertools.product((1, 255, 257, 1000), (1, 2, 3, 7, 20, 64), (1, 2, 255),
                                             ("tied", "distinct")):
        rng = np.random.default_rng(100000 + 97 * T + 13 * K + cap)
        if kind == "tied":          # four distinct values, 0 among them; every seventh row all zero
            act = rng.integers(0, 4, size=(T, K))
            act[::7] = 0
        else:                       # every row a permutation of 0 .. K - 1
            act = np.stack([rng.permutation(K) for _ in range(T)])
        count = rng.integers(0, K + 4, size=T)
        count[:K + 4] = np.arange(K + 4)[:T]            # every count from 0 to K + 3 where T allows
        cases.append({"id": f"T{T}-K{K}-cap{cap}-{kind}", "act": (act * scale).astype(dtype),
                      "count": count.astype(np.uint8), "cap": cap, "distinct": kind == "distinct"})
    return cases


@functools.lru_cache(maxsize=None)
def topk_i32_cases():
    return _topk_cases(np.int32)


@functools.lru_cache(maxsize=None)
def topk_f32_cases():
    return _topk_cases(np.float32)


#: (onset, offset) pairs for which 0.5f * (onset + offset) in float32 is one ulp off the reference's midpoint (above
#: it for the first and the last, below it for the second)
KNIFE_EDGE_PAIRS = ((0.4, 0.3), (0.45, 0.35), (0.6, 0.3))
#: ... ordinary pairs, and one whose midpoint is 0: there a NaN in frame 0 starts the row ON only if it counts as 0
HYSTERESIS_PAIRS = ((0.5, 0.5), (0.6, 0.4)) + KNIFE_EDGE_PAIRS + ((0.25, -0.25),)


def _hysteresis_scores(rng, C, F, K, onset, offset):
    scores = rng.uniform(size=(C, F, K)).astype(np.float32)
    flat = scores.reshape(-1)
    flat[rng.integers(0, flat.size, size=max(1, flat.size // 11))] = np.float32(onset)      # exactly on a threshold
    flat[rng.integers(0, flat.size, size=max(1, flat.size // 11))] = np.float32(offset)
    flat[rng.integers(0, flat.size, size=max(1, flat.size // 13))] = np.nan
    scores[::3, 0, :] = np.nan                                                              # NaN in frame 0 ...
    band = np.float32(0.5 * (onset + offset))
    scores[::3, 1:, 0] = band                               # ... followed, in class 0, by scores that change nothing
    mid = hysteresis_midpoint(onset, offset)
    rows = [mid, np.nextafter(mid, np.float32(1)), np.nextafter(mid, np.float32(-1))]
    for c, first in zip((1, 2, 4), rows):                   # first score on the midpoint and on its two neighbours,
        k = K - 1                                           # then in-band scores for the whole row
        scores[c, :, k] = rng.uniform(offset, onset, size=F).astype(np.float32) if offset < onset else band
        scores[c, 0, k] = first
    return scores


@functools.lru_cache(maxsize=None)
def hysteresis_cases():
    """K = 1, 3, 7; F = 1, 2, 589; C * K on both sides of 256; every pair with initial_state -1, one pair with 0 and 1"""
    cases = []
    shapes = [(C, F, K) for K, Cs in ((1, (255, 257)), (3, (85, 86)), (7, (36, 37))) for C in Cs for F in (1, 2, 589)]
    for (C, F, K), (onset, offset) in itertools.product(shapes, HYSTERESIS_PAIRS):
        rng = np.random.default_rng(500000 + 1000 * C + 10 * F + K)
        scores = _hysteresis_scores(rng, C, F, K, onset, offset)
        for initial in (-1, 0, 1) if (onset, offset) == (0.6, 0.4) else (-1,):
            cases.append({"id": f"C{C}-F{F}-K{K}-on{onset}-off{offset}-init{initial}", "scores": scores,
                          "onset": onset, "offset": offset, "initial_state": initial})
    return cases


@functools.lru_cache(maxsize=None)
def cluster_max_cases():
    """S = 1, 3, 8; K = 1, 4; C * F = 255 and 258; chunk 1 has no assigned speaker; NaN in one and in all speakers of a
    cluster"""
    cases = []
    for S, K, (C, F) in itertools.product((1, 3, 8), (1, 4), ((3, 85), (3, 86))):
        rng = np.random.default_rng(700000 + 100 * S + 10 * K + F)
        scores = rng.uniform(size=(C, F, S)).astype(np.float32)
        hard = rng.integers(0, K, size=(C, S)).astype(np.int32)
        hard[1] = -2
        if S > 1:
            hard[0, :2] = 0                     # two speakers of cluster 0 in chunk 0 ...
            hard[2, -1] = K + 1                 # ... and a speaker of no cluster
        scores[0, 3, 0] = np.nan                # NaN in one speaker of the cluster (the only one when S = 1)
        scores[0, 5, -1] = np.nan
        scores[0, 7, :] = np.nan                # NaN in all of them
        scores[2, 11, :] = np.nan
        cases.append({"id": f"S{S}-K{K}-C{C}-F{F}", "scores": scores, "hard": hard, "K": K})
    return cases


@functools.lru_cache(maxsize=None)
def aggregate_cases():
    """C <= 6, F <= 40, K = 1, 3, 7, T * K no multiple of 256; uncovered frames in front of the first chunk and
    between chunks, two chunks with the same start; class 0 NaN in some chunks, class 1 (K > 1) NaN in every chunk"""
    cases = []
    geometries = (("F40", 145, 40, (5, 15, 15, 30, 90, 100)), ("F7", 33, 7, (2, 2, 6, 20)))
    for (name, T, F, starts), K in itertools.product(geometries, (1, 3, 7)):
        assert (T * K) % 256
        rng = np.random.default_rng(900000 + 10 * F + K)
        C = len(starts)
        scores = rng.uniform(size=(C, F, K)).astype(np.float32)
        scores.reshape(-1)[rng.integers(0, scores.size, size=scores.size // 9)] = np.nan
        scores[1::2, :, 0] = np.nan
        if K > 1:
            scores[:, :, 1] = np.nan
        for hamming, warm_up, skip, missing in itertools.product((0, 1), (0, 3), (0, 1), (np.nan, 0.0)):
            epsilon = 1e-12
            warm = np.ones(F)
            if warm_up:
                warm[:warm_up] = epsilon
                warm[F - warm_up:] = epsilon
            cases.append({"id": f"{name}-K{K}-ham{hamming}-warm{warm_up}-skip{skip}-missing{missing}",
                          "scores": scores, "start": np.array(starts, dtype=np.int32), "T": T,
                          "window": np.hamming(F) if hamming else np.ones(F), "warm": warm, "epsilon": epsilon,
                          "missing": missing, "skip_average": skip})
    return cases


#: operation -> (its case list, the model's outputs for one case as a tuple)
OPERATIONS = {
    "chunk_stats": (chunk_stats_cases, lambda c, wrong=None: chunk_stats(c["seg"], wrong=wrong)),
    "embedding_masks": (embedding_masks_cases, lambda c, wrong=None: (embedding_masks(
        c["seg"], c["clean"], c["exclude_overlap"], c["min_num_frames"], wrong=wrong),)),
    "speaker_count": (speaker_count_cases, lambda c, wrong=None: (speaker_count(c["seg"], c["start"], c["T"],
                                                                                wrong=wrong),)),
    "cluster_activations": (cluster_activations_cases, lambda c, wrong=None: (cluster_activations(
        c["seg"], c["start"], c["hard"], c["K"], c["T"], wrong=wrong),)),
    "topk_i32": (topk_i32_cases, lambda c, wrong=None: topk(c["act"], c["count"], c["cap"], wrong=wrong)),
    "topk_f32": (topk_f32_cases, lambda c, wrong=None: topk(c["act"], c["count"], c["cap"], wrong=wrong)),
    "hysteresis": (hysteresis_cases, lambda c, wrong=None: (hysteresis(
        c["scores"], c["onset"], c["offset"], c["initial_state"], wrong=wrong),)),
    "cluster_max": (cluster_max_cases, lambda c, wrong=None: (cluster_max(c["scores"], c["hard"], c["K"],
                                                                          wrong=wrong),)),
    "aggregate": (aggregate_cases, lambda c, wrong=None: (aggregate(
        c["scores"], c["start"], c["T"], c["window"], c["warm"], c["epsilon"], c["missing"], c["skip_average"],
        wrong=wrong),)),
}


def same_bits(got, want) -> bool:
    """float32 arrays equal bit for bit, NaN compared as positions (any NaN is the same NaN)"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(got[ok].view(np.int32), want[ok].view(np.int32))
