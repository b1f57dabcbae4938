"""The online step on the device against its numpy model (tests/online_model.py): `cluster_step`, `emit`, the
`StreamBank` end to end on the synthetic models, batch independence and the pipeline.  Every comparison is `==`."""
import numpy as np
import pytest
import torch

import online_model as om

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _same_f64(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _step_both(slots, emb, active, clean, csum, cn, d_csum, d_cn, min_active, min_update, delta_new):
    """one step on the model state (csum, cn: numpy, in place) and on the device state (d_csum, d_cn) -> both maps"""
    from pyannote_audio_amd import online
    dev = d_csum.device
    want = om.cluster_step(slots, emb, active, clean, csum, cn, min_active, min_update, delta_new)
    got = online.cluster_step(slots, _dev(emb, dev), _dev(active, dev), _dev(clean, dev), d_csum, d_cn, min_active,
                              min_update, delta_new)
    return got.cpu().numpy(), want


# ------------------------------------------------------------------------------------------------------ cluster_step
@pytest.mark.parametrize("M,S,K,D", [(1, 1, 1, 1), (3, 3, 2, 2), (65, 3, 5, 255), (3, 4, 32, 256), (1, 4, 5, 2),
                                     (65, 1, 2, 256), (3, 4, 1, 255), (3, 3, 32, 1)])
def test_cluster_step_equals_the_model_over_a_sequence(gpu_device, M, S, K, D):
    rng = np.random.default_rng(M * 1000 + S * 100 + K + D)
    N = M + 2
    slots = rng.permutation(N)[:M].astype(np.int32)
    proto = rng.standard_normal((6, D)).astype(np.float32)
    csum, cn = np.zeros((N, K, D)), np.zeros((N, K), dtype=np.int32)
    if K == 32:                       # a few centroids far apart in the table, so that high indices are reached
        for k in (7, 31):
            csum[:, k], cn[:, k] = proto[k % 6].astype(np.float64) * 3, 3
    d_csum, d_cn = _dev(csum, gpu_device), _dev(cn, gpu_device)
    for step in range(6):
        emb = (proto[rng.integers(0, 6, size=(M, S))] + 0.15 * rng.standard_normal((M, S, D))).astype(np.float32)
        bad = rng.random((M, S))
        emb[bad < 0.04] = 0.0
        emb[(bad > 0.04) & (bad < 0.07), 0] = np.nan
        emb[(bad > 0.07) & (bad < 0.10), -1] = np.inf
        active = rng.integers(0, 20, size=(M, S)).astype(np.int32)
        clean = np.minimum(active, rng.integers(0, 20, size=(M, S))).astype(np.int32)
        got, want = _step_both(slots, emb, active, clean, csum, cn, d_csum, d_cn, 5, 8, 0.5)
        assert (got == want).all(), f"step {step}: map {got.tolist()} for {want.tolist()}"
        assert (d_cn.cpu().numpy() == cn).all(), f"step {step}: centroid_n"
        assert _same_f64(d_csum.cpu().numpy(), csum), f"step {step}: centroid_sum"
    if M * S > 1:                                                             # centroids were founded and updated
        assert cn.max() > 1 and (cn > 0).sum() > (2 * M if K == 32 else 0)


def _one(gpu_device, emb, active, clean, csum, cn, delta_new=0.5, min_active=5, min_update=8):
    """a bank of one stream: kernel == model on map and state -> (map, centroid_sum, centroid_n)"""
    emb = np.asarray(emb, dtype=np.float32)[None]
    active, clean = np.asarray(active, dtype=np.int32)[None], np.asarray(clean, dtype=np.int32)[None]
    csum, cn = np.array(csum, dtype=np.float64)[None], np.array(cn, dtype=np.int32)[None]
    d_csum, d_cn = _dev(csum, gpu_device), _dev(cn, gpu_device)
    got, want = _step_both(np.zeros(1, np.int32), emb, active, clean, csum, cn, d_csum, d_cn, min_active, min_update,
                           delta_new)
    assert (got == want).all(), f"map {got.tolist()} for {want.tolist()}"
    assert (d_cn.cpu().numpy() == cn).all() and _same_f64(d_csum.cpu().numpy(), csum)
    return want[0].tolist(), csum[0], cn[0].tolist()


E3 = np.eye(3, 4, dtype=np.float32)          # three orthogonal embeddings, D = 4


def test_cluster_step_constructed_cases(gpu_device):
    zero = np.zeros((3, 4))
    # empty bank: every long speaker founds the next free slot; a present but short one has nowhere to go
    mp, csum, cn = _one(gpu_device, E3, [9, 9, 9], [9, 2, 9], zero, [0, 0, 0])
    assert (mp, cn) == ([0, -1, 1], [1, 1, 0]) and (csum[1] == E3[2]).all()
    # full bank, P > K_occ: two are mapped, the third finds both centroids held
    mp, _, cn = _one(gpu_device, E3, [9, 9, 9], [9, 9, 9], E3[:2].astype(np.float64), [1, 1], delta_new=0.5)
    assert (mp, cn) == ([0, 1, -1], [2, 2])
    # full bank, everybody too far: nobody matches, all are forced, nothing moves
    far = np.array([[1, 1, 0, 0], [1, -1, 0, 0]], dtype=np.float32)
    mp, csum, cn = _one(gpu_device, far, [9, 9], [9, 9], E3[:2].astype(np.float64), [4, 4], delta_new=0.1)
    assert (mp, cn) == ([0, 1], [4, 4]) and (csum == E3[:2]).all()
    # nobody present
    mp, csum, cn = _one(gpu_device, E3, [4, 0, 1], [4, 0, 1], E3.astype(np.float64), [1, 0, 2])
    assert (mp, cn) == ([-1, -1, -1], [1, 0, 2])
    # NaN, Inf and all-zero rows are not present, whatever their activity
    bad = np.array([[np.nan, 1, 0, 0], [np.inf, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0]], dtype=np.float32)
    mp, _, cn = _one(gpu_device, bad, [9] * 4, [9] * 4, zero, [0, 0, 0])
    assert (mp, cn) == ([-1, -1, -1, 0], [1, 0, 0])
    # duplicated centroids and duplicated embeddings: every total ties, the smallest tuple wins
    same = np.tile(E3[:1], (3, 1))
    mp, _, cn = _one(gpu_device, same, [9] * 3, [9] * 3, np.tile(E3[:1].astype(np.float64), (4, 1)), [1, 0, 1, 1])
    assert (mp, cn) == ([0, 2, 3], [2, 0, 2, 2])
    mp, _, _ = _one(gpu_device, same, [9, 9, 0], [9, 9, 0], np.tile(E3[:1].astype(np.float64), (4, 1)), [0, 0, 0, 1])
    assert mp == [3, 0, -1]          # one centroid for two: speaker 0 takes it ((3, unmapped) < (unmapped, 3))
    # two unmatched long speakers and one free slot: the first founds it, the second is forced
    mp, _, cn = _one(gpu_device, far, [9, 9], [9, 9], E3[:2].astype(np.float64), [1, 0], delta_new=0.1)
    assert (mp, cn) == ([1, 0], [1, 1])
    # a forced speaker whose nearest centroid was founded in this step: its founder holds it
    twins = np.array([[0, 0, 1, 0], [0, 0, 1, 0]], dtype=np.float32)
    mp, _, cn = _one(gpu_device, twins, [9, 9], [9, 2], np.array([[1.0, 0, 0, 0], [0, 0, 0, 0]]), [1, 0], delta_new=0.5)
    assert (mp, cn) == ([1, 0], [1, 1])


def test_cluster_step_delta_new_boundary(gpu_device):
    """delta_new set to a distance the model computed: d > delta_new un-maps, d == delta_new does not"""
    from scipy.spatial.distance import cdist
    rng = np.random.default_rng(5)
    emb = rng.standard_normal((1, 7)).astype(np.float32)
    centre = rng.standard_normal((2, 7))
    centre[1] = 0.0
    d = float(cdist(emb.astype(np.float64), centre[:1], "cosine")[0, 0])
    assert 0.0 < d < 2.0
    mp, _, cn = _one(gpu_device, emb, [9], [9], centre, [1, 0], delta_new=d)
    assert (mp, cn) == ([0], [2, 0])
    mp, _, cn = _one(gpu_device, emb, [9], [9], centre, [1, 0], delta_new=float(np.nextafter(d, -np.inf)))
    assert (mp, cn) == ([1], [1, 1])
    mp, _, cn = _one(gpu_device, emb, [9], [9], centre, [1, 0], delta_new=float(np.nextafter(d, np.inf)))
    assert (mp, cn) == ([0], [2, 0])


def test_cluster_step_leaves_unlisted_slots_alone(gpu_device):
    rng = np.random.default_rng(11)
    N, K, D, S = 6, 3, 5, 2
    csum = rng.standard_normal((N, K, D))
    cn = rng.integers(0, 3, size=(N, K)).astype(np.int32)
    before_sum, before_n = csum.copy(), cn.copy()
    d_csum, d_cn = _dev(csum, gpu_device), _dev(cn, gpu_device)
    slots = np.array([4, 2, 0], dtype=np.int32)                      # descending
    emb = rng.standard_normal((3, S, D)).astype(np.float32)
    got, want = _step_both(slots, emb, np.full((3, S), 9, np.int32), np.full((3, S), 9, np.int32), csum, cn, d_csum,
                           d_cn, 5, 8, 0.8)
    assert (got == want).all() and (d_cn.cpu().numpy() == cn).all() and _same_f64(d_csum.cpu().numpy(), csum)
    for slot in (1, 3, 5):
        assert _same_f64(csum[slot], before_sum[slot]) and (cn[slot] == before_n[slot]).all()
    assert not _same_f64(csum[[0, 2, 4]], before_sum[[0, 2, 4]])


# -------------------------------------------------------------------------------------------------------------- emit
def _emit_both(slots, seg, mp, start, frm, to, acc_sum, acc_cnt, d_sum, d_cnt, E):
    from pyannote_audio_amd import online
    dev = d_sum.device
    want = om.emit(slots, seg, mp, start, frm, to, acc_sum, acc_cnt, E)
    got = online.emit(slots, _dev(seg, dev), _dev(mp, dev), start, frm, to, d_sum, d_cnt, E).cpu().numpy()
    assert (got == want).all(), "emitted rows"
    assert (d_sum.cpu().numpy() == acc_sum).all() and (d_cnt.cpu().numpy() == acc_cnt).all(), "ring state"
    return want


@pytest.mark.parametrize("F,advances", [(1, (1,)), (7, (2, 3)), (293, (30, 29))])
def test_emit_equals_the_model(gpu_device, F, advances):
    """Four streams in one call at different phases: latency = one step (everything the chunk reaches is emitted),
    latency = the chunk (only what the next chunk will not cover), one whose map rows are all -1, one that emits
    nothing until its last call.  F = 7: R = F + E and 40 steps of alternating advances wrap the ring several times."""
    rng = np.random.default_rng(F)
    S, K, N, steps = 3, 4, 6, (40 if F == 7 else 8)
    E = F
    R = F + E
    slots = np.array([5, 0, 3, 2], dtype=np.int32)
    acc_sum, acc_cnt = np.zeros((N, R, K), dtype=np.int32), np.zeros((N, R), dtype=np.int32)
    d_sum, d_cnt = _dev(acc_sum, gpu_device), _dev(acc_cnt, gpu_device)
    start = np.array([0, 3, 2 * F + 1, 0], dtype=np.int64)          # different phases of the ring in one call
    emitted = start.copy()
    wrapped = 0
    for step in range(steps):
        adv = advances[step % len(advances)]
        seg = (rng.random((4, F, S)) < 0.6).astype(np.uint8)
        mp = rng.integers(-1, K, size=(4, S)).astype(np.int32)
        mp[2] = -1
        last = step == steps - 1
        to = np.array([start[0] + F, start[1] + adv, start[2] + F, start[3] + F if last else emitted[3]])
        to = np.minimum(np.maximum(to, emitted), emitted + E)
        out = _emit_both(slots, seg, mp, start.copy(), emitted.copy(), to, acc_sum, acc_cnt, d_sum, d_cnt, E)
        assert not out[2].any() and (last or not out[3].any())
        wrapped = max(wrapped, int(to[0]) // R)
        emitted = to
        # the stream that holds everything back advances only while its ring has room
        start = start + np.array([adv, adv, adv, adv if start[3] + adv + F - emitted[3] <= R else 0])
    assert wrapped >= (3 if F == 7 else 0)
    assert not acc_sum[[1, 4]].any() and not acc_cnt[[1, 4]].any()             # unlisted slots
    # a flush (start_frame < 0) adds nothing and empties what is left
    to = start + F
    to[3] = emitted[3]
    _emit_both(slots, seg, mp, np.full(4, -1, np.int64), emitted.copy(), np.minimum(to, emitted + E), acc_sum, acc_cnt,
               d_sum, d_cnt, E)


def test_refusals(gpu_device):
    from pyannote_audio_amd import online
    dev = gpu_device
    assert online.cluster_step_limits() == (4, 32)

    def step(S=3, K=5, slots=(0, 1)):
        M, N, D = len(slots), 4, 6
        state = torch.zeros((N, K, D), dtype=torch.float64, device=dev), torch.zeros((N, K), dtype=torch.int32, device=dev)
        ints = torch.full((M, S), 9, dtype=torch.int32, device=dev)
        online.cluster_step(slots, torch.ones((M, S, D), device=dev), ints, ints, *state, 1, 1, 0.5)
        return state

    def emission(S=3, K=5, R=20, E=6, F=7, slots=(0, 1), frm=(0, 0), to=(3, 3)):
        M, N = len(slots), 4
        state = torch.zeros((N, R, K), dtype=torch.int32, device=dev), torch.zeros((N, R), dtype=torch.int32, device=dev)
        online.emit(slots, torch.ones((M, F, S), dtype=torch.uint8, device=dev),
                    torch.zeros((M, S), dtype=torch.int32, device=dev), [0] * M, frm, to, *state, E)
        return state

    step(), emission()
    with pytest.raises(ValueError, match="5 local speakers per chunk, the kernel handles 1..4"):
        step(S=5)
    with pytest.raises(ValueError, match="33 global speakers per stream, the kernel handles 1..32"):
        step(K=33)
    with pytest.raises(ValueError, match=r"duplicate slot 1 \(entries 0 and 2\)"):
        step(slots=(1, 0, 1))
    with pytest.raises(ValueError, match="slot 4 .* outside the bank of 4"):
        step(slots=(0, 4))
    with pytest.raises(ValueError, match="a ring of 12 frames is shorter than F \\+ E = 7 \\+ 6"):
        emission(R=12)
    with pytest.raises(ValueError, match="5 local speakers"):
        emission(S=5)
    with pytest.raises(ValueError, match="33 global speakers"):
        emission(K=33)
    with pytest.raises(ValueError, match="duplicate slot 2"):
        emission(slots=(2, 2))
    with pytest.raises(ValueError, match="inconsistent frames of entry 1"):
        emission(frm=(0, 4), to=(3, 3))
    with pytest.raises(ValueError, match="inconsistent frames of entry 0"):
        emission(to=(7, 3))                                      # more than E frames
    torch.cuda.synchronize()


def test_a_refused_call_writes_nothing(gpu_device):
    """through the C ABI with full-size buffers (tests/refusals.py): return code 3, the message, outputs and state as
    they were"""
    import pyannote_audio_amd.ffi as ffi
    from refusals import check_refusal
    lib, dev = ffi.load(), gpu_device
    M, N, D, K, F, E = 2, 4, 6, 5, 7, 6
    slots = np.array([0, 1], dtype=np.int32)
    d_slots = torch.from_numpy(slots).to(dev)
    frames = np.array([[0, 0], [0, 0], [3, 3]], dtype=np.int64)
    d_frames = torch.from_numpy(frames).to(dev)
    emb = torch.ones((M, 5, D), device=dev)
    ints = torch.full((M, 5), 9, dtype=torch.int32, device=dev)
    csum = torch.full((N, K, D), 0.25, dtype=torch.float64, device=dev)
    seg = torch.ones((M, F, 3), dtype=torch.uint8, device=dev)
    mp = torch.zeros((M, 3), dtype=torch.int32, device=dev)
    check_refusal(lambda out, cn: lib.pao_cluster_step(
        ffi.ptr(d_slots), slots.ctypes.data, M, N, ffi.ptr(emb), ffi.ptr(ints), ffi.ptr(ints), 5, D, K, 1, 1, 0.5,
        ffi.ptr(csum), cn, out, ffi.stream()), [((M, 5), torch.int32), ((N, K), torch.int32)],
        "pao_cluster_step: 5 local speakers per chunk, the kernel handles 1..4", dev)
    assert bool((csum == 0.25).all())
    check_refusal(lambda out, acc_sum, acc_cnt: lib.pao_emit(
        ffi.ptr(d_slots), slots.ctypes.data, M, N, ffi.ptr(seg), F, 3, ffi.ptr(mp), ffi.ptr(d_frames[0]),
        ffi.ptr(d_frames[1]), ffi.ptr(d_frames[2]), frames.ctypes.data, 12, K, E, acc_sum, acc_cnt, out, ffi.stream()),
        [((M, E, K), torch.uint8), ((N, 12, K), torch.int32), ((N, 12), torch.int32)],
        "pao_emit: a ring of 12 frames is shorter than F + E = 7 + 6", dev)


# -------------------------------------------------------------------------------------------------- the bank, end to end
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
            for seed, seconds in enumerate((7.3, 12.0, 5.0, 6.0))}


class ModelBank:
    """the bank written again for the test: host buffers, the same engine calls with the same batch composition, then
    the numpy model of the two kernels"""

    def __init__(self, bank):
        self.b = bank
        N = bank.num_slots
        self.csum, self.cn = np.zeros((N, bank.K, bank.D)), np.zeros((N, bank.K), dtype=np.int32)
        self.acc_sum = np.zeros((N, bank.R, bank.K), dtype=np.int32)
        self.acc_cnt = np.zeros((N, bank.R), dtype=np.int32)
        self.audio = {}                                 # slot -> samples received

    def centroids(self, slot):
        with np.errstate(all="ignore"):                 # (0 / 0 = NaN for the speakers not founded yet)
            return self.csum[slot] / self.cn[slot][:, None].astype(np.float64)

    def open(self, slot):
        self.csum[slot], self.cn[slot], self.acc_sum[slot], self.acc_cnt[slot] = 0, 0, 0, 0
        self.audio[slot] = dict(wav=np.zeros(0, dtype=np.float32), chunks=0, emitted=0, rows=[])

    def _geometry(self, c):
        b = self.b
        args = (b.frames.step, b.frames.duration)
        return om.start_frame(c, b.step, *args), om.emit_bound(c, b.step, b.duration, b.latency, *args)

    def step(self, ready, windows, limit=None):
        """ready slots and their windows (M, window) -> {slot: (first, rows)}"""
        from pyannote_audio_amd import frames as frame_ops
        b = self.b
        M = len(ready)
        flat = _dev(windows, b.device).view(-1)
        _, seg = b.seg_model.engine.forward_strided(flat, b.window, M, b.window, want_logp=False, want_multilabel=True)
        active, clean = frame_ops.chunk_stats(seg)
        masks = frame_ops.embedding_masks(seg, clean, b.exclude_overlap, b._min_num_frames())
        emb = b.emb_model.engine.forward_strided(flat, b.window, M, b.window, masks).cpu().numpy()
        seg, active, clean = seg.cpu().numpy(), active.cpu().numpy(), clean.cpu().numpy()
        mp = om.cluster_step(ready, emb, active, clean, self.csum, self.cn, b.min_active_frames, b.min_update_frames,
                             b.delta_new)
        out = {}
        for i, slot in enumerate(ready):
            st = self.audio[slot]
            start, bound = self._geometry(st["chunks"])
            to = max(min(bound, start + b.F, limit if limit is not None else bound), st["emitted"])
            rows = om.emit_one(seg[i], mp[i], start, st["emitted"], to, self.acc_sum[slot], self.acc_cnt[slot],
                               max(1, to - st["emitted"]))[:to - st["emitted"]]
            out[slot] = (st["emitted"], rows)
            st["rows"].append(rows)
            st["emitted"], st["chunks"] = to, st["chunks"] + 1
        return out

    def push(self, blocks, slots):
        b, ready = self.b, []
        for block, slot in zip(blocks, slots):
            st = self.audio[slot]
            st["wav"] = np.concatenate([st["wav"], block])
            if len(st["wav"]) >= b.window:
                ready.append(slot)
        if not ready:
            return {}
        return self.step(ready, np.stack([self.audio[s]["wav"][-b.window:] for s in ready]))

    def close(self, slot, tail):
        """-> every row of the stream"""
        from pyannote_audio_amd.online import stream_num_frames
        b, st = self.b, self.audio[slot]
        wav = st["wav"] if tail is None else np.concatenate([st["wav"], tail])
        total = stream_num_frames(len(wav), b.window, b.step_samples, b.sample_rate, b.duration, b.step, b.frames)
        padded = np.concatenate([wav, np.zeros((-len(wav)) % b.step_samples, dtype=np.float32)])
        if len(wav) < b.window:
            window = np.concatenate([wav, np.zeros(b.window - len(wav), dtype=np.float32)])
            self.step([slot], window[None], limit=total)
        elif tail is not None and len(tail):
            self.step([slot], padded[-b.window:][None], limit=total)
        if st["emitted"] < total:
            rows = om.emit_one(np.zeros((b.F, b.S), np.uint8), np.full(b.S, -1), -1, st["emitted"], total,
                               self.acc_sum[slot], self.acc_cnt[slot], total - st["emitted"])
            st["rows"].append(rows)
            st["emitted"] = total
        return np.concatenate(st["rows"])


def _run_length(rows, frames):
    """[(start, end, label)] of the runs of every column, with the frame middles as times"""
    turns = []
    middle = lambda i: 0.5 * ((frames.start + i * frames.step) + ((frames.start + i * frames.step) + frames.duration))  # noqa: E731
    for k in range(rows.shape[1]):
        on, begin = False, 0
        for i in range(rows.shape[0]):
            if rows[i, k] and not on:
                on, begin = True, i
            elif not rows[i, k] and on:
                on = False
                turns.append((middle(begin), middle(i), f"SPEAKER_{k:02d}"))
        if on:
            turns.append((middle(begin), middle(rows.shape[0] - 1), f"SPEAKER_{k:02d}"))
    return sorted(turns)


def _turns(annotation):
    return sorted((float(seg.start), float(seg.end), str(label))
                  for seg, _, label in annotation.itertracks(yield_label=True))


def test_bank_end_to_end_equals_the_model_loop(gpu_device, models, waves):
    """streams of 7.3 s, 5 s and 12 s, opened at different pushes, the 5-s one closed and its slot reused by a 6-s one"""
    from pyannote_audio_amd.core import SlidingWindow
    from pyannote_audio_amd.online import StreamBank
    bank = StreamBank(*models, 3, latency=2.0, max_speakers=6, delta_new=0.7, min_active=0.2, min_update=0.5,
                      device=gpu_device)
    ref = ModelBank(bank)
    step = bank.step_samples
    plan = {0: [(7.3, 0)], 1: [(5.0, 1), (6.0, 13)], 2: [(12.0, 3)]}         # slot -> (stream, push it opens at)
    live, done = {}, []
    matched_rows = 0
    for push in range(40):
        for slot, streams in plan.items():
            if slot not in live and streams and streams[0][1] <= push:
                seconds, _ = streams.pop(0)
                assert bank.open() == slot
                ref.open(slot)
                live[slot] = [waves[seconds].numpy(), 0, seconds]
        for slot in [s for s, (wav, at, _) in live.items() if len(wav) - at < step]:
            wav, at, seconds = live.pop(slot)
            tail = wav[at:] if len(wav) > at else None
            bank.close(slot, None if tail is None else torch.from_numpy(tail))
            want = ref.close(slot, tail)
            got = bank.decisions(slot)
            assert got.shape == want.shape and (got == want).all(), f"{seconds}-s stream at close"
            frames = SlidingWindow(start=0.0, duration=bank.frames.duration, step=bank.frames.step)
            assert _turns(bank.annotation(slot)) == _run_length(got, frames)
            assert _same_f64(bank.centroids(slot), ref.centroids(slot))
            done.append((seconds, got))
        slots = sorted(live, reverse=push % 2 == 1)
        if not slots:
            continue
        blocks = np.stack([live[s][0][live[s][1]:live[s][1] + step] for s in slots])
        for s in slots:
            live[s][1] += step
        got = bank.push(torch.from_numpy(blocks) if push % 3 else torch.from_numpy(blocks).to(gpu_device), slots)
        want = ref.push(blocks, slots)
        assert list(got) == list(want), f"push {push}: slots {list(got)} for {list(want)}"
        for s in got:
            assert got[s][0] == want[s][0] and got[s][1].shape == want[s][1].shape and (got[s][1] == want[s][1]).all()
            assert _same_f64(bank.centroids(s), ref.centroids(s))
            matched_rows += int(got[s][1].sum())
    assert not live and sorted(s for s, _ in done) == [5.0, 6.0, 7.3, 12.0]
    assert matched_rows > 0 and all(rows.any() for _, rows in done)      # the streams said something


def _stream_through(bank, slot, wav, others):
    """stream `wav` through `slot`, the other open slots fed with their own audio -> (rows, centroids)"""
    step = bank.step_samples
    at = 0
    while len(wav) - at >= step:
        slots = [slot] + [s for s, w in others.items() if len(w) - at >= step]
        bank.push(torch.stack([torch.from_numpy((wav if s == slot else others[s])[at:at + step]) for s in slots]), slots)
        at += step
    bank.close(slot, torch.from_numpy(wav[at:]) if len(wav) > at else None)
    return bank.decisions(slot), bank.centroids(slot)


def test_a_stream_does_not_depend_on_its_neighbours(gpu_device, models, waves):
    """stream 0 alone, in a bank of 3 and in a bank of 17: the same rows and the same centroids, bit for bit"""
    from pyannote_audio_amd.online import StreamBank
    wav = waves[7.3].numpy()
    results = []
    for n in (1, 3, 17):
        bank = StreamBank(*models, n, max_speakers=6, delta_new=0.7, min_active=0.2, min_update=0.5, device=gpu_device)
        slots = [bank.open() for _ in range(n)]
        mine = slots[n // 2]
        others = {s: np.roll(waves[12.0].numpy(), 1000 * s)[:16000 * (6 + s % 3)] for s in slots if s != mine}
        results.append(_stream_through(bank, mine, wav, others))
    for rows, centroids in results[1:]:
        assert rows.shape == results[0][0].shape and (rows == results[0][0]).all()
        assert _same_f64(centroids, results[0][1])
    assert results[0][0].any()


def test_pipeline_batch_equals_one_by_one(gpu_device, models, waves):
    from pyannote_audio_amd.online import OnlineSpeakerDiarization
    pipeline = OnlineSpeakerDiarization(segmentation=models[0], embedding=models[1], latency=1.0, max_speakers=6,
                                        delta_new=0.7, min_active=0.2, min_update=0.5).to(gpu_device)
    files = [{"waveform": waves[s].view(1, -1), "sample_rate": 16000, "uri": f"file{i}"}
             for i, s in enumerate((7.3, 5.0, 6.0))]
    batch = pipeline.apply_batch(files, num_slots=2)
    single = [pipeline.apply(f) for f in files]
    assert [a.uri for a in batch] == ["file0", "file1", "file2"]
    for a, b in zip(batch, single):
        assert _turns(a) == _turns(b)
    assert any(_turns(a) for a in batch)
    assert [(f["uri"], _turns(a)) for f, a in pipeline(files, num_slots=2)] == [(a.uri, _turns(a)) for a in batch]
