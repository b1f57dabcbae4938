"""`pao_replay` (include/pyannote_amd_online.h, csrc/online_replay.hip) against its numpy model
(tests/online_replay_model.py) and against the per-chunk device calls; `StreamBank.front_end` / `replay`, the
`replay=True` route of the pipeline and `tuning.OnlineTuner` end to end on the seeded synthetic models against the
streaming route.  Every comparison is `==`; float64 state is compared as bits."""

import numpy as np
import pytest
import torch

import online_model as om
import online_replay_model as rm
from kernel_parity import GUARD, Guarded

pytestmark = pytest.mark.gpu

#: (F, frames per step, latency in steps); None: PyanNet's receptive field with 5-s chunks and 0.5-s steps
GEOMETRIES = [(1, 1, 1), (7, 2, 1), (7, 3, 2), (293, None, 4)]
FRAME_STEP, FRAME_DURATION = 270 / 16000, 991 / 16000


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _schedule(C, geometry):
    F, per_step, latency_steps = geometry
    if per_step is None:
        return rm.streamed_schedule(C, F, 5.0, 0.5, 0.5 * latency_steps, FRAME_STEP, FRAME_DURATION)
    return rm.synthetic_schedule(C, F, per_step, latency_steps)


_clustered = {}


def _model_clustering(case):
    """the clustering steps of a case through the model, once: they do not depend on the emission geometry
    -> (maps, centroid_sum, centroid_n, events)"""
    if case not in _clustered:
        seed, C, S, D, K, V, sigma, delta_new = case
        emb, active, clean, _ = rm.generate(seed, C, S, D, V, sigma, 1)
        csum, cn = np.zeros((K, D)), np.zeros(K, dtype=np.int32)
        maps, events = rm.cluster_file(emb, active, clean, csum, cn, rm.MIN_ACTIVE, rm.MIN_UPDATE, delta_new)
        _clustered[case] = (maps, csum, cn, events)
    return _clustered[case]


class Job:
    """one file as one job, on the host"""

    def __init__(self, case, geometry, C=None):
        seed, C0, self.S, self.D, self.K, V, sigma, self.delta_new = case
        self.F = geometry[0]
        self.C = C0 if C is None else C
        self.emb, self.active, self.clean, self.seg = (a[:self.C] for a in rm.generate(seed, C0, self.S, self.D, V,
                                                                                       sigma, self.F))
        self.sched, self.total = _schedule(self.C, geometry)


def _zeros(J, K, D, R, device):
    return (torch.zeros((J, K, D), dtype=torch.float64, device=device),
            torch.zeros((J, K), dtype=torch.int32, device=device),
            torch.zeros((J, R, K), dtype=torch.int32, device=device),
            torch.zeros((J, R), dtype=torch.int32, device=device))


def _replay_single(job, R, device, state=None, chunks=None, sched=None, total=None, delta_new=None):
    """one job through `online.replay_jobs` -> (maps, out, state tensors)"""
    from pyannote_audio_amd import online
    a, b = chunks if chunks is not None else (0, job.C)
    sched = job.sched if sched is None else sched
    total = job.total if total is None else total
    state = _zeros(1, job.K, job.D, R, device) if state is None else state
    mp, out = online.replay_jobs(
        _dev(job.emb[a:b], device), _dev(job.active[a:b], device), _dev(job.clean[a:b], device),
        _dev(job.seg[a:b], device), [[0, b - a, 0, total]], sched, [[0, rm.MIN_ACTIVE, rm.MIN_UPDATE]],
        [job.delta_new if delta_new is None else delta_new], [[0, 0]], *state)
    return mp.cpu().numpy(), out.cpu().numpy(), state


def _same_state(state, csum, cn, acc_sum, acc_cnt):
    got = [t.cpu().numpy() for t in state]
    assert got[0][0].tobytes() == csum.tobytes(), "centroid_sum (bits)"
    assert (got[1][0] == cn).all(), "centroid_n"
    assert (got[2][0] == acc_sum).all() and (got[3][0] == acc_cnt).all(), "the ring"


# ------------------------------------------------------------------------------------------- 1. kernel == model
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: f"F{g[0]}-{g[1]}-{g[2]}")
@pytest.mark.parametrize("case", rm.CASES, ids=lambda c: f"seed{c[0]}")
def test_replay_equals_the_model(gpu_device, case, geometry):
    """every case at every emission geometry, with the smallest ring the schedule allows and with the bank's 2F + 16"""
    job = Job(case, geometry)
    maps, csum, cn, events = _model_clustering(case)
    # the condition the cases were chosen for, from the model's own run
    assert events["found"] >= 1 and events["update"] >= 6 and events["forced"] >= 3, dict(events)
    assert events["unmapped"] >= 3 and events["absent"] >= 10, dict(events)
    assert case[0] == 2 or events["nothing_can_take"] >= 1, dict(events)
    assert (maps == -1).any() and (maps >= 0).any()
    said = False
    for R in (rm.smallest_ring(job.sched, job.F), 2 * job.F + 16):
        acc_sum, acc_cnt = np.zeros((R, job.K), dtype=np.int32), np.zeros(R, dtype=np.int32)
        want = rm.emit_file(job.seg, maps, job.sched, job.total, acc_sum, acc_cnt)
        got_maps, got, state = _replay_single(job, R, gpu_device)
        assert (got_maps == maps).all(), f"R = {R}: maps"
        assert got.shape == want.shape and (got == want).all(), f"R = {R}: emitted rows"
        _same_state(state, csum, cn, acc_sum, acc_cnt)
        said = said or bool(want.any())
    assert said


def test_the_interleaved_model_is_the_two_loops(gpu_device):
    """the kernel interleaves step and emission; the model of test 1 runs the two loops one after the other"""
    job = Job(rm.CASES[1], GEOMETRIES[2])
    R = rm.smallest_ring(job.sched, job.F)
    args = (job.emb, job.active, job.clean, job.seg, job.sched, job.total, rm.MIN_ACTIVE, rm.MIN_UPDATE, job.delta_new)
    new = lambda: (np.zeros((job.K, job.D)), np.zeros(job.K, np.int32), np.zeros((R, job.K), np.int32),  # noqa: E731
                   np.zeros(R, np.int32))
    a, b = new(), new()
    m1, o1, _ = rm.replay_one(*args, *a)
    m2, o2 = rm.interleaved(*args, *b)
    assert (m1 == m2).all() and (o1 == o2).all() and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    got_maps, got, state = _replay_single(job, R, gpu_device)
    assert (got_maps == m2).all() and (got == o2).all()
    _same_state(state, *b)


# ------------------------------------------------------------------------- 2. kernel == the existing device calls
@pytest.mark.parametrize("case,geometry", [(rm.CASES[1], GEOMETRIES[2]), (rm.CASES[3], GEOMETRIES[3]),
                                           (rm.CASES[2], GEOMETRIES[0])], ids=["seed1", "seed3", "seed2"])
def test_replay_equals_the_per_chunk_calls(gpu_device, case, geometry):
    from pyannote_audio_amd import online
    job = Job(case, geometry)
    R = 2 * job.F + 16
    dev = gpu_device
    got_maps, got, state = _replay_single(job, R, dev)
    csum, cn, acc_sum, acc_cnt = _zeros(1, job.K, job.D, R, dev)
    emb, active, clean, seg = (_dev(a, dev) for a in (job.emb, job.active, job.clean, job.seg))
    rows, maps = [], []
    for c in range(job.C + 1):
        g0, ga, gb = job.sched[c].tolist()
        if c < job.C:
            mp = online.cluster_step([0], emb[c:c + 1], active[c:c + 1], clean[c:c + 1], csum, cn, rm.MIN_ACTIVE,
                                     rm.MIN_UPDATE, job.delta_new)
            maps.append(mp)
            chunk = seg[c:c + 1]
        else:
            mp = torch.full((1, job.S), -1, dtype=torch.int32, device=dev)
            chunk = torch.zeros((1, job.F, job.S), dtype=torch.uint8, device=dev)
        rows.append(online.emit([0], chunk, mp, [g0], [ga], [gb], acc_sum, acc_cnt, max(1, gb - ga))[0, :gb - ga])
    assert (got_maps == torch.cat(maps).cpu().numpy()).all()
    assert (got == torch.cat(rows).cpu().numpy()).all() and got.any()
    for a, b in zip(state, (csum, cn, acc_sum, acc_cnt)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------- 3. many jobs, ragged
def _call(lib, dev_in, tables, host, J, sizes, ptrs):
    """`pao_replay` through the C ABI.  dev_in: emb, active, clean, seg; tables: device files, sched, jobs, delta,
    offsets; host: numpy files, sched, jobs, offsets (None -> NULL); sizes: num_chunks, F, S, D, num_files, num_sched,
    map_rows, out_rows, K, R; ptrs: centroid_sum, centroid_n, acc_sum, acc_cnt, map, out"""
    import pyannote_audio_amd.ffi as ffi
    num_chunks, F, S, D, num_files, num_sched, map_rows, out_rows, K, R = sizes
    h = [None if a is None else a.ctypes.data for a in host]
    return lib.pao_replay(*[ffi.ptr(t) for t in dev_in], num_chunks, F, S, D, ffi.ptr(tables[0]), h[0], num_files,
                          ffi.ptr(tables[1]), h[1], num_sched, ffi.ptr(tables[2]), h[2], ffi.ptr(tables[3]),
                          ffi.ptr(tables[4]), h[3], J, map_rows, out_rows, K, R, *ptrs, ffi.stream())


def _guards_intact(g, what):
    host = g.buf.cpu()
    assert bool(g._untouched(host[:GUARD]).all()) and bool(g._untouched(host[GUARD + g.n:]).all()), \
        f"{what}: a guard block was overwritten"
    return host[GUARD:GUARD + g.n]


def _boundary_delta(job):
    """a distance that occurs in the job's step 1: that of the first long speaker the optimal map assigns there (step 0 of
    an empty bank only founds, so the state after it does not depend on delta_new)"""
    from scipy.spatial.distance import cdist
    csum, cn = np.zeros((job.K, job.D)), np.zeros(job.K, dtype=np.int32)
    om.cluster_step_one(job.emb[0], job.active[0], job.clean[0], csum, cn, rm.MIN_ACTIVE, rm.MIN_UPDATE, 0.5)
    e = job.emb[1]
    present = [bool(job.active[1][s] >= rm.MIN_ACTIVE and np.isfinite(e[s]).all() and np.any(e[s] != 0))
               for s in range(job.S)]
    occupied = [bool(n > 0) for n in cn]
    d = np.full((job.S, job.K), np.nan)
    ps, oc = [s for s in range(job.S) if present[s]], [k for k in range(job.K) if occupied[k]]
    assert ps and oc
    d[np.ix_(ps, oc)] = cdist(e[ps].astype(np.float64), csum[oc], "cosine")
    tup = om.optimal_map(d, present, occupied, job.K)
    # a LONG one: mapped it moves its centroid, un-mapped it does not (or founds another), so the two sides differ
    s = next(s for s in range(job.S) if tup[s] < job.K and job.clean[1][s] >= rm.MIN_UPDATE)
    return float(d[s][tup[s]])


def test_many_ragged_jobs_in_one_launch(gpu_device):
    """files of 0, 1 and 17 chunks, two to three threshold triples each, jobs interleaved, rows of `map` and `out`
    with gaps no job owns: every job equals its own launch and the model, and nothing else is written"""
    import pyannote_audio_amd.ffi as ffi
    lib, dev = ffi.load(), gpu_device
    case, geometry = (9, 17, 3, 8, 4, 3, 0.4, 0.5), GEOMETRIES[2]
    fs = [Job(case, geometry, C=c) for c in (0, 1, 17)]
    S, D, K, F = fs[0].S, fs[0].D, fs[0].K, fs[0].F
    R = max(rm.smallest_ring(f.sched, F) for f in fs)
    d = _boundary_delta(fs[2])
    assert 0.0 < d < 2.0
    below = float(np.nextafter(d, -np.inf))
    # (file, min_active_frames, min_update_frames, delta_new), interleaved
    plan = [(2, 10, 15, d), (0, 10, 15, 0.5), (1, 10, 15, 0.5), (2, 10, 15, below), (1, 3, 4, 0.9), (0, 3, 4, 0.1),
            (2, 3, 4, 0.9), (1, 10, 15, 1e-3)]
    J = len(plan)
    counts = np.array([f.C for f in fs], dtype=np.int64)
    files = np.stack([np.concatenate([[0], np.cumsum(counts)[:-1]]), counts,
                      np.concatenate([[0], np.cumsum(counts + 1)[:-1]]), [f.total for f in fs]], axis=1).astype(np.int64)
    sched = np.concatenate([f.sched for f in fs])
    jobs = np.array([[f, a, u] for f, a, u, _ in plan], dtype=np.int32)
    delta = np.array([p[3] for p in plan])
    offsets = np.zeros((J, 2), dtype=np.int64)
    map_rows = out_rows = 3                                                   # a gap in front of the first job
    for j in (5, 0, 3, 1, 7, 2, 6, 4):                                        # offsets in another order than the jobs
        offsets[j] = (map_rows, out_rows)
        map_rows += fs[plan[j][0]].C + 2                                      # ... and gaps between the jobs
        out_rows += fs[plan[j][0]].total + 5
    dev_in = [_dev(np.concatenate([getattr(f, name) for f in fs]), dev) for name in ("emb", "active", "clean", "seg")]
    tables = [_dev(a, dev) for a in (files, sched, jobs, delta, offsets)]
    sizes = (int(counts.sum()), F, S, D, len(fs), len(sched), map_rows, out_rows, K, R)
    state_n = (J * K * D, J * K, J * R * K, J * R)
    outs = [Guarded(state_n[0], dev, torch.float64), Guarded(state_n[1], dev, torch.int32),
            Guarded(state_n[2], dev, torch.int32), Guarded(state_n[3], dev, torch.int32),
            Guarded(map_rows * S, dev, torch.int32), Guarded(out_rows * K, dev, torch.uint8)]
    for g in outs[:4]:                                                        # the state on entry: zeros
        g.buf[GUARD:GUARD + g.n] = 0
    rc = _call(lib, dev_in, tables, (files, sched, jobs, offsets), J, sizes, [g.ptr for g in outs])
    assert rc == 0, lib.pa_last_error().decode()
    torch.cuda.synchronize()
    csum, cn, acc_sum, acc_cnt = (_guards_intact(g, "state").numpy() for g in outs[:4])
    csum, cn = csum.reshape(J, K, D), cn.reshape(J, K)
    acc_sum, acc_cnt = acc_sum.reshape(J, R, K), acc_cnt.reshape(J, R)
    owned_map = torch.zeros(map_rows * S, dtype=torch.bool)
    owned_out = torch.zeros(out_rows * K, dtype=torch.bool)
    for j, (f, _, _, _) in enumerate(plan):
        owned_map[offsets[j, 0] * S:(offsets[j, 0] + fs[f].C) * S] = True
        owned_out[offsets[j, 1] * K:(offsets[j, 1] + fs[f].total) * K] = True
    got_map = outs[4].check(owned_map, "map").numpy().reshape(map_rows, S)   # (gaps untouched, owned rows written)
    got_out = outs[5].check(owned_out, "out").numpy().reshape(out_rows, K)
    results = []
    for j, (f, min_active, min_update, delta_new) in enumerate(plan):
        job = fs[f]
        m_state = np.zeros((K, D)), np.zeros(K, np.int32), np.zeros((R, K), np.int32), np.zeros(R, np.int32)
        want_maps, want, _ = rm.replay_one(job.emb, job.active, job.clean, job.seg, job.sched, job.total, min_active,
                                           min_update, delta_new, *m_state)
        mine_map = got_map[offsets[j, 0]:offsets[j, 0] + job.C]
        mine_out = got_out[offsets[j, 1]:offsets[j, 1] + job.total]
        assert (mine_map == want_maps).all() and (mine_out == want).all(), f"job {j} against the model"
        assert csum[j].tobytes() == m_state[0].tobytes() and (cn[j] == m_state[1]).all(), f"job {j}: centroids"
        assert (acc_sum[j] == m_state[2]).all() and (acc_cnt[j] == m_state[3]).all(), f"job {j}: ring"
        # ... and against its own launch
        from pyannote_audio_amd import online
        state = _zeros(1, K, D, R, dev)
        mp, out = online.replay_jobs(*(_dev(getattr(job, n), dev) for n in ("emb", "active", "clean", "seg")),
                                     [[0, job.C, 0, job.total]], job.sched, [[0, min_active, min_update]], [delta_new],
                                     [[0, 0]], *state)
        assert (mp.cpu().numpy() == mine_map).all() and (out.cpu().numpy() == mine_out).all(), f"job {j} alone"
        assert state[0].cpu().numpy()[0].tobytes() == csum[j].tobytes()
        results.append((want_maps, want, m_state[0].tobytes() + m_state[1].tobytes()))
    # the > boundary: at delta_new = d the pair stays mapped, one ulp below it is un-mapped (it founds or is forced:
    # another map, or the same map and no update)
    assert not (results[0][0] == results[3][0]).all() or results[0][2] != results[3][2]
    assert results[2][1].any() or results[0][1].any()
    assert fs[0].total > 0 and not results[1][1].any()                        # no chunk: rows of zeros, written


# ------------------------------------------------------------------------------------------- 4. state is complete
def test_a_replay_can_be_continued(gpu_device):
    """chunks [0, c0) and then [c0, C) with the carried state give one replay of [0, C)"""
    job = Job(rm.CASES[0], GEOMETRIES[2])
    R = rm.smallest_ring(job.sched, job.F) + 3
    maps, out, state = _replay_single(job, R, gpu_device)
    whole = [t.cpu().numpy().tobytes() for t in state]
    assert out.any()
    for c0 in (1, job.C // 2, job.C - 1):
        done = int(job.sched[c0, 1])                                          # emitted before chunk c0
        first = np.concatenate([job.sched[:c0], [[-1, done, done]]])          # a flush that emits nothing
        m1, o1, carried = _replay_single(job, R, gpu_device, chunks=(0, c0), sched=first, total=done)
        m2, o2, carried = _replay_single(job, R, gpu_device, state=carried, chunks=(c0, job.C), sched=job.sched[c0:],
                                         total=job.total - done)
        assert (np.concatenate([m1, m2]) == maps).all() and (np.concatenate([o1, o2]) == out).all(), f"c0 = {c0}"
        assert [t.cpu().numpy().tobytes() for t in carried] == whole, f"c0 = {c0}: final state"


# ---------------------------------------------------------------------------------------------------- 5. refusals
def _refusal_case(dev, S=3, K=5, D=6, F=7, R=30):
    """two files of 2 and 1 chunks, three jobs -> (device inputs, host tables, sizes)"""
    counts = [2, 1]
    scheds = [rm.synthetic_schedule(c, F, 3, 2) for c in counts]
    files = np.array([[0, 2, 0, scheds[0][1]], [2, 1, 3, scheds[1][1]]], dtype=np.int64)
    sched = np.concatenate([s for s, _ in scheds])
    jobs = np.array([[0, 1, 1], [1, 1, 1], [0, 2, 2]], dtype=np.int32)
    totals = [int(files[f, 3]) for f in jobs[:, 0]]
    offsets = np.array([[0, 0], [2, totals[0]], [3, totals[0] + totals[1]]], dtype=np.int64)
    dev_in = [torch.ones((3, S, max(D, 1)), device=dev), torch.full((3, S), 9, dtype=torch.int32, device=dev),
              torch.full((3, S), 9, dtype=torch.int32, device=dev), torch.ones((3, F, S), dtype=torch.uint8, device=dev)]
    sizes = dict(num_chunks=3, F=F, S=S, D=D, num_files=2, num_sched=5, map_rows=5, out_rows=sum(totals), K=K, R=R)
    return dev_in, dict(files=files, sched=sched, jobs=jobs, offsets=offsets), sizes


REQUIRED = ("pao_replay: the host copies of the file table, the schedule, the job table and the offsets are required: "
            "the loop bounds come from them")


def _refusals():
    """(name, keyword arguments of the case, edit of tables and sizes, message)"""
    def table(name, index, value):
        def edit(tables, sizes):
            tables[name][index] = value
        return edit

    def size(name, value):
        def edit(tables, sizes):
            sizes[name] = value
        return edit

    def null(name):
        def edit(tables, sizes):
            tables["null"] = name
        return edit

    # the base schedule of file 0 (F = 7, 3 frames per step, latency 2 steps): (0, 0, 4), (3, 4, 7), (-1, 7, 12)
    return [
        ("S", dict(S=5), None, "pao_replay: 5 local speakers per chunk, the kernel handles 1..4"),
        ("K", dict(K=33), None, "pao_replay: 33 global speakers per stream, the kernel handles 1..32"),
        ("D", dict(D=0), None, "pao_replay: needs D >= 1, F >= 1, R >= F and counts >= 0 (got D = 0, F = 7, R = 30)"),
        ("files_host", {}, null("files"), REQUIRED), ("sched_host", {}, null("sched"), REQUIRED),
        ("jobs_host", {}, null("jobs"), REQUIRED), ("offsets_host", {}, null("offsets"), REQUIRED),
        ("job_file", {}, table("jobs", (1, 0), 2), "pao_replay: job 1 names file 2 of 2"),
        ("job_file_negative", {}, table("jobs", (2, 0), -1), "pao_replay: job 2 names file -1 of 2"),
        ("file_chunks", {}, table("files", (1, 1), 2),
         "pao_replay: file 1 (chunks [2, +2), schedule rows from 3, 9 frames) runs past the 3 chunks or the 5 schedule "
         "rows"),
        ("map_past", {}, size("map_rows", 4),
         "pao_replay: job 2 writes map rows [3, +2) of 4 and out rows [21, +12) of 33"),
        ("out_past", {}, table("offsets", (2, 1), 22),
         "pao_replay: job 2 writes map rows [3, +2) of 5 and out rows [22, +12) of 33"),
        ("map_overlap", {}, table("offsets", (1, 0), 1), "pao_replay: two jobs share map rows [1, 2)"),
        ("out_overlap", {}, table("offsets", (1, 1), 11), "pao_replay: two jobs share out rows [11, 12)"),
        ("from_above_to", {}, table("sched", (1, 2), 3),
         "pao_replay: inconsistent schedule of file 0, row 1: chunk at 3 (F = 7), emission [4, 3), R = 30"),
        ("not_chained", {}, table("sched", (1, 1), 3),
         "pao_replay: inconsistent schedule of file 0, row 1: chunk at 3 (F = 7), emission [3, 7), R = 30"),
        ("total", {}, table("files", (0, 3), 11), "pao_replay: the schedule of file 0 emits 12 frames, its frame total "
         "is 11"),
        # a ring of 7 rows holds chunk 0 (0 + 7 - 0); chunk 1 moved to frame 5 with frame 4 still due needs 8
        ("ring", dict(R=7), table("sched", (1, 0), 5),
         "pao_replay: inconsistent schedule of file 0, row 1: chunk at 5 (F = 7), emission [4, 7), R = 7"),
        ("flush", {}, table("sched", (2, 0), 6),
         "pao_replay: inconsistent schedule of file 0, row 2: chunk at 6 (F = 7), emission [7, 12), R = 30 (the last "
         "row is the flush: start_frame < 0)"),
    ]


@pytest.mark.parametrize("name,kwargs,edit,message", _refusals(), ids=[r[0] for r in _refusals()])
def test_a_refused_replay_writes_nothing(gpu_device, name, kwargs, edit, message):
    import pyannote_audio_amd.ffi as ffi
    from refusals import check_refusal
    lib, dev = ffi.load(), gpu_device
    dev_in, tables, sizes = _refusal_case(dev, **kwargs)
    if edit is not None:
        edit(tables, sizes)
    null = tables.pop("null", None)
    S, K, D, R = sizes["S"], sizes["K"], max(sizes["D"], 1), sizes["R"]
    J = 3
    d_tables = [_dev(tables[n], dev) for n in ("files", "sched", "jobs")] + \
        [torch.full((J,), 0.5, dtype=torch.float64, device=dev), _dev(tables["offsets"], dev)]
    host = tuple(None if n == null else tables[n] for n in ("files", "sched", "jobs", "offsets"))
    csum = torch.full((J, K, D), 0.25, dtype=torch.float64, device=dev)
    order = tuple(sizes[n] for n in ("num_chunks", "F", "S", "D", "num_files", "num_sched", "map_rows", "out_rows", "K",
                                     "R"))
    check_refusal(lambda mp, out, cn, acc_sum, acc_cnt: _call(
        lib, dev_in, d_tables, host, J, order, [ffi.ptr(csum), cn, acc_sum, acc_cnt, mp, out]),
        [((sizes["map_rows"] + 2, S), torch.int32), ((sizes["out_rows"] + 12, K), torch.uint8), ((J, K), torch.int32),
         ((J, R, K), torch.int32), ((J, R), torch.int32)], message, dev)
    assert bool((csum == 0.25).all())


def test_the_refusal_case_is_accepted_as_it_stands(gpu_device):
    """the base case of the refusals runs: every refusal above is due to its one edit"""
    import pyannote_audio_amd.ffi as ffi
    lib, dev = ffi.load(), gpu_device
    dev_in, tables, sizes = _refusal_case(dev)
    J, S, K, D, R = 3, sizes["S"], sizes["K"], sizes["D"], sizes["R"]
    d_tables = [_dev(tables[n], dev) for n in ("files", "sched", "jobs")] + \
        [torch.full((J,), 0.5, dtype=torch.float64, device=dev), _dev(tables["offsets"], dev)]
    state = _zeros(J, K, D, R, dev)
    mp = torch.full((sizes["map_rows"], S), 77, dtype=torch.int32, device=dev)
    out = torch.full((sizes["out_rows"], K), 77, dtype=torch.uint8, device=dev)
    order = tuple(sizes[n] for n in ("num_chunks", "F", "S", "D", "num_files", "num_sched", "map_rows", "out_rows", "K",
                                     "R"))
    rc = _call(lib, dev_in, d_tables, tuple(tables[n] for n in ("files", "sched", "jobs", "offsets")), J, order,
               [ffi.ptr(t) for t in state] + [ffi.ptr(mp), ffi.ptr(out)])
    assert rc == 0, lib.pa_last_error().decode()
    torch.cuda.synchronize()
    assert not bool((mp == 77).any()) and not bool((out == 77).any()) and bool(out.any())


# --------------------------------------------------------------------------------------------- 6. stream contract
def test_replay_is_captured_whole(gpu_device):
    """the four steps of tests/test_online_contract_gpu.py for one `pao_replay` case of three jobs on two files"""
    import pyannote_audio_amd.ffi as ffi
    from test_online_contract_gpu import Case, _bits, _same
    lib, dev = ffi.load(), gpu_device
    lib.pa_prof_enable(0)
    with torch.cuda.device(dev):
        fs = [Job(rm.CASES[1], GEOMETRIES[2], C=c) for c in (9, 4)]
        S, D, K, F = fs[0].S, fs[0].D, fs[0].K, fs[0].F
        R = 2 * F + 16
        plan = [(0, 10, 15, 0.6), (1, 10, 15, 0.6), (0, 3, 4, 0.3)]
        J = len(plan)
        files = np.array([[0, 9, 0, fs[0].total], [9, 4, 10, fs[1].total]], dtype=np.int64)
        sched = np.concatenate([f.sched for f in fs])
        jobs = np.array([p[:3] for p in plan], dtype=np.int32)
        rows = np.array([[fs[f].C, fs[f].total] for f, _, _, _ in plan], dtype=np.int64)
        offsets = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(rows, axis=0)])
        map_rows, out_rows = (int(v) for v in offsets[-1])
        offsets = np.ascontiguousarray(offsets[:-1])
        dev_in = [_dev(np.concatenate([getattr(f, n) for f in fs]), dev) for n in ("emb", "active", "clean", "seg")]
        tables = [_dev(a, dev) for a in (files, sched, jobs, np.array([p[3] for p in plan]), offsets)]
        sizes = (13, F, S, D, 2, len(sched), map_rows, out_rows, K, R)
        rng = np.random.default_rng(6)
        outs = [Guarded(J * K * D, dev, torch.float64), Guarded(J * K, dev, torch.int32),
                Guarded(J * R * K, dev, torch.int32), Guarded(J * R, dev, torch.int32),
                Guarded(map_rows * S, dev, torch.int32), Guarded(out_rows * K, dev, torch.uint8)]
        initial = {0: torch.from_numpy(rng.standard_normal((J, K, D))),
                   1: torch.from_numpy(rng.integers(0, 3, size=(J, K)).astype(np.int32)),
                   2: torch.zeros((J, R, K), dtype=torch.int32), 3: torch.zeros((J, R), dtype=torch.int32)}
        case = Case(dev, lambda *ptrs: _call(lib, dev_in, tables, (files, sched, jobs, offsets), J, sizes, list(ptrs)),
                    outs, initial, dev_in + tables)
        inputs = _bits(case.inputs)
        case.reset()
        clean = case.snapshot()

        rc = case.run()
        assert rc == 0, lib.pa_last_error().decode()
        eager = case.snapshot()
        case.guards_intact(eager)
        changed = [not torch.equal(r, c) for r, c in zip(eager, clean)]
        assert all(changed[i] for i in (0, 1, 4, 5)), "the eager call left an output or the centroids alone"

        case.reset()
        side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        rc, failure = None, None
        try:
            with torch.cuda.graph(graph, stream=side, capture_error_mode="global"):
                rc = case.run()
        except Exception as e:                                                           # noqa: BLE001
            failure = e
        assert failure is None, f"the capture did not end clean: {failure!r}; pa_last_error: {lib.pa_last_error().decode()}"
        assert rc == 0, lib.pa_last_error().decode()
        assert _same(case.snapshot(), clean), "something ran while the call was only being captured"
        for _ in range(2):
            graph.replay()
            got = case.snapshot()
            case.guards_intact(got)
            assert _same(got, eager), "a replayed graph does not give the eager bytes"
            case.reset()
        assert _same(_bits(case.inputs), inputs), "an input was modified"
        del graph


# ------------------------------------------------------------------------ 7. end to end, seeded synthetic models
@pytest.fixture(scope="module")
def models(gpu_device, synthetic_models):
    import pyannote_audio_amd.model as pm
    from conftest import PYANNET_HPARAMS, WESPEAKER_HPARAMS
    seg_o, emb_o = synthetic_models
    seg = pm.PyanNet(seg_o.state_dict(), PYANNET_HPARAMS, pm.segmentation_specifications(5.0, True)).to(gpu_device)
    emb = pm.WeSpeakerResNet34(emb_o.state_dict(), WESPEAKER_HPARAMS, pm.embedding_specifications()).to(gpu_device)
    return seg, emb


@pytest.fixture(scope="module")
def waves():
    from oracle.synthetic import synth_conversation
    return {seconds: synth_conversation(seconds, seed=seed)[0].view(-1)
            for seed, seconds in enumerate((7.3, 12.0, 5.0, 6.0, 2.0))}


OPTIONS = dict(max_speakers=6, delta_new=0.7, min_active=0.2, min_update=0.5)


def _streamed(bank, wav):
    """the wave through a fresh slot of the bank, one step per push -> (decisions, centroids)"""
    slot = bank.open()
    step, at = bank.step_samples, 0
    while wav.numel() - at >= step:
        bank.push(wav[at:at + step][None], [slot])
        at += step
    bank.close(slot, wav[at:] if wav.numel() > at else None)
    return bank.decisions(slot), bank.centroids(slot)


def _turns(annotation):
    return sorted((float(seg.start), float(seg.end), str(label))
                  for seg, _, label in annotation.itertracks(yield_label=True))


@pytest.mark.parametrize("latency", [0.5, 2.0, 5.0])
def test_replaying_a_wave_equals_streaming_it(gpu_device, models, waves, latency):
    from pyannote_audio_amd.online import StreamBank
    bank = StreamBank(*models, 1, latency=latency, device=gpu_device, **OPTIONS)
    said = 0
    for seconds, wav in waves.items():
        rows, centroids = _streamed(bank, wav)
        front = bank.front_end(wav)
        assert front.num_chunks == max(1, -(-wav.numel() // bank.step_samples) - bank.steps_per_window + 1)
        got = bank.replay(front)
        assert got.decisions.shape == rows.shape and (got.decisions == rows).all(), f"{seconds}-s wave: decisions"
        assert got.centroids.tobytes() == centroids.tobytes(), f"{seconds}-s wave: centroids"
        assert got.maps.shape == (front.num_chunks, bank.S)
        said += int(rows.any())
    assert said >= 1
    # all of them as the files of one replay, a small front-end group: the same again
    bank.front_end_bytes = 3 * 4 * bank.window
    fronts = bank.front_ends(list(waves.values()))
    for got, one in zip(bank.replay(fronts), (bank.replay(bank.front_end(w)) for w in waves.values())):
        assert (got.decisions == one.decisions).all() and got.centroids.tobytes() == one.centroids.tobytes()
        assert (got.maps == one.maps).all()


@pytest.mark.parametrize("latency", [0.5, 2.0, 5.0])
def test_pipeline_replay_gives_the_streamed_turns(gpu_device, models, waves, latency):
    from pyannote_audio_amd.online import OnlineSpeakerDiarization
    pipeline = OnlineSpeakerDiarization(segmentation=models[0], embedding=models[1], latency=latency,
                                        **OPTIONS).to(gpu_device)
    files = [{"waveform": w.view(1, -1), "sample_rate": 16000, "uri": f"file{i}"} for i, w in enumerate(waves.values())]
    streamed = pipeline.apply_batch(files)
    replayed = pipeline.apply_batch(files, replay=True)
    assert [a.uri for a in replayed] == [f["uri"] for f in files]
    for a, b in zip(replayed, streamed):
        assert _turns(a) == _turns(b)
    assert any(_turns(a) for a in replayed)
    assert _turns(pipeline.apply(files[0], replay=True)) == _turns(streamed[0])


# ----------------------------------------------------------------------------------------------------- 8. tuner
def test_online_tuner_equals_the_literal_loop(gpu_device, models, waves):
    from oracle.synthetic import synth_conversation
    from pyannote_audio_amd.core import Annotation, Segment
    from pyannote_audio_amd.online import OnlineSpeakerDiarization
    from pyannote_audio_amd.tuning import OnlineTuner
    files = []
    for seed, seconds in ((0, 7.3), (1, 12.0), (3, 6.0)):
        activity = synth_conversation(seconds, seed=seed)[1]
        reference = Annotation(uri=f"file{seed}")
        for s, row in enumerate(np.asarray(activity)):
            edges = np.flatnonzero(np.diff(np.concatenate([[0], row.astype(np.int8), [0]])))
            for a, b in zip(edges[::2], edges[1::2]):
                reference[Segment(a / 16000, b / 16000), s] = f"ref{s}"
        files.append({"waveform": waves[seconds].view(1, -1), "sample_rate": 16000, "uri": f"file{seed}",
                      "annotation": reference})
    options = dict(latency=2.0, max_speakers=6)
    pipeline = OnlineSpeakerDiarization(segmentation=models[0], embedding=models[1], **options).to(gpu_device)
    tuner = OnlineTuner(pipeline).prepare(files)
    frame = tuner.bank.frames.step
    grid = ([0.3, 0.9], [12.2 * frame, 11.8 * frame], [0.5, 1.5])            # both min_active values are 12 frames
    assert tuner.bank.threshold_frames(grid[1][0], 0.5)[0] == tuner.bank.threshold_frames(grid[1][1], 0.5)[0] == 12
    result = tuner.sweep(*grid)
    assert len(result["entries"]) == 8 and result["evaluations"] == 24 and tuner.jobs == 12
    losses = []
    for entry in result["entries"]:
        params = entry["params"]
        literal = OnlineSpeakerDiarization(segmentation=models[0], embedding=models[1], **options,
                                           **params).to(gpu_device)
        metric = literal.get_metric()
        for file in files:
            metric(file["annotation"], literal.apply(file), uem=file.get("annotated"))
        losses.append(abs(metric))
        assert entry["loss"] == losses[-1], f"{params}: {entry['loss']!r} for {losses[-1]!r}"
    assert [e["params"] for e in result["entries"]] == [
        {"delta_new": d, "min_active": a, "min_update": u} for d in grid[0] for a in grid[1] for u in grid[2]]
    assert result["best"] is result["entries"][int(np.argmin(losses))]
    assert result["shared_evaluations"] >= 12                                 # the rounding-equal candidates, at least
    assert len(set(losses)) > 1, "every candidate scored the same: the grid decides nothing"
    assert tuner.apply_best(result) == result["best"]["params"] and \
        all(pipeline.bank_options[n] == v for n, v in result["best"]["params"].items())
