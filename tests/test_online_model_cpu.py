"""The numpy model of the online step (tests/online_model.py) against independent statements of the same things, and
the host side of `pyannote_audio_amd.online`: frame arithmetic and `StreamBank`'s scheduling.  No GPU; every comparison
is `==`."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import online_model as om

FRAME_DURATION, FRAME_STEP = 0.0619375, 0.016875     # PyanNet's receptive field at 16 kHz


# ---------------------------------------------------------------------------------------- the optimal map
def _map_case(seed):
    rng = np.random.default_rng(1000 + seed)
    S, K = 4, 8
    P, Kocc = 1 + seed % 4, (seed // 4) % 7
    present = np.zeros(S, dtype=bool)
    present[rng.permutation(S)[:P]] = True
    occupied = np.zeros(K, dtype=bool)
    occupied[rng.permutation(K)[:Kocc]] = True
    return rng.random((S, K)) * 2.0, present, occupied, K


def test_model_map_is_the_linear_assignment_optimum():
    """400 seeded cases, P in 1..4, K_occ in 0..6: continuous random costs have one optimum, and the enumeration finds
    the one scipy.optimize.linear_sum_assignment finds.  No case is left out (0 exact ties among the 400)."""
    seen = set()
    for seed in range(400):
        d, present, occupied, K = _map_case(seed)
        seen.add((int(present.sum()), int(occupied.sum())))
        tup = om.optimal_map(d, list(present), list(occupied), K)
        ps, oc = np.nonzero(present)[0], np.nonzero(occupied)[0]
        want = np.full(len(present), K)
        if len(oc):
            rows, cols = linear_sum_assignment(d[np.ix_(ps, oc)])
            want[ps[rows]] = oc[cols]
        assert tuple(int(k) for k in want) == tuple(tup), f"seed {seed}: {tup} for {want}"
        assert sum(k < K for k in tup) == min(len(ps), len(oc))
    assert seen == {(p, k) for p in range(1, 5) for k in range(7)}


def test_model_map_ties_go_to_the_lexicographically_smallest_tuple():
    d = np.ones((3, 4))
    assert om.optimal_map(d, [True] * 3, [True] * 4, 4) == (0, 1, 2)
    assert om.optimal_map(d, [True] * 3, [False, True, False, True], 4) == (1, 3, 4)     # "unmapped" is last
    assert om.optimal_map(d, [False, True, True], [False, False, True, False], 4) == (4, 2, 4)


# ------------------------------------------------------------------------------------------- the emission
def _stream_geometry(C, duration, step, latency, frame_step, frame_duration, F):
    """(start, emit_from, emit_to) of C chunks by the bank's rule, then the flush to the end of the last chunk"""
    rows, emitted = [], 0
    for c in range(C):
        start = om.start_frame(c, step, frame_step, frame_duration)
        bound = min(om.emit_bound(c, step, duration, latency, frame_step, frame_duration), start + F)
        rows.append((start, emitted, max(bound, emitted)))
        emitted = rows[-1][2]
    return rows, rows[-1][0] + F


@pytest.mark.parametrize("latency_steps", [1, 2, 4])
def test_emission_model_is_the_average_of_the_covering_chunks(latency_steps):
    """ring model, step by step == over whole arrays: a frame is the majority of the chunks that covered it by the time
    it was emitted (every chunk that covers it when the latency is the chunk duration)"""
    rng = np.random.default_rng(7 + latency_steps)
    duration, step, frame_step, frame_duration, F, S, K, C = 1.0, 0.25, 0.137, 0.21, 7, 3, 5, 60
    rows, last = _stream_geometry(C, duration, step, latency_steps * step, frame_step, frame_duration, F)
    seg = (rng.random((C, F, S)) < 0.5).astype(np.uint8)
    maps = rng.integers(-1, K, size=(C, S)).astype(np.int32)
    E, R = F + 2, 2 * F + 2
    acc_sum, acc_cnt = np.zeros((R, K), dtype=np.int32), np.zeros(R, dtype=np.int32)
    got = [om.emit_one(seg[c], maps[c], start, a, b, acc_sum, acc_cnt, E)[:b - a] for c, (start, a, b) in enumerate(rows)]
    got.append(om.emit_one(seg[0], maps[0], -1, rows[-1][2], last, acc_sum, acc_cnt, E)[:last - rows[-1][2]])
    got = np.concatenate(got)
    assert got.shape == (last, K) and not acc_sum.any() and not acc_cnt.any()

    # whole arrays: contribution of every chunk to every frame, then the chunks that were in when the frame left
    on = np.zeros((C, last, K), dtype=np.int64)
    covers = np.zeros((C, last), dtype=np.int64)
    for c, (start, _, _) in enumerate(rows):
        covers[c, start:start + F] = 1
        for s in range(S):
            if maps[c, s] >= 0:
                on[c, start:start + F, maps[c, s]] += seg[c, :, s]
    emitted_after = np.full(last, C - 1)
    for c, (_, a, b) in reversed(list(enumerate(rows))):
        emitted_after[a:b] = c
    seen = np.arange(C)[:, None] <= emitted_after[None, :]
    want = 2 * (on * seen[:, :, None]).sum(0) > (covers * seen).sum(0)[:, None]
    assert (got == want.astype(np.uint8)).all()
    if latency_steps == 4:
        assert seen[covers.astype(bool)].all()      # latency = duration: every covering chunk was in


def _tiles(duration, step, frame_step, frame_duration, F, C):
    from pyannote_audio_amd import online
    from pyannote_audio_amd.core import SlidingWindow
    frames = SlidingWindow(start=0.0, duration=frame_duration, step=frame_step)
    for multiple in range(1, round(duration / step) + 1):
        latency = multiple * step
        emitted = 0
        for c in range(C):
            start = online.start_frame(c, step, frames)
            assert start == om.start_frame(c, step, frame_step, frame_duration)
            bound = online.emit_bound(c, step, duration, latency, frames)
            assert bound == om.emit_bound(c, step, duration, latency, frame_step, frame_duration)
            to = min(bound, start + F)
            # no gap, no overlap: the range starts where the last one ended, inside the chunk that just came in, and
            # never runs backwards; what is due is emitted unless the chunk does not reach that far
            assert start <= emitted <= to <= start + F, (latency, c, start, emitted, to)
            if multiple == round(duration / step):
                assert (emitted, to) == (start, online.start_frame(c + 1, step, frames)) or to == start + F
            emitted = to
        assert emitted > online.start_frame(C - 1, step, frames)


def test_emitted_ranges_tile_the_stream():
    """every latency in {step, ..., duration}: consecutive ranges tile [0, last) in PyanNet's non-integral geometry
    (5-s chunks, 0.5-s steps, 16.875-ms frames, F = 293) and in a synthetic one with F = 7"""
    _tiles(5.0, 0.5, FRAME_STEP, FRAME_DURATION, 293, 200)
    _tiles(1.0, 0.25, 0.137, 0.21, 7, 200)


def test_start_frame_is_frame_geometry():
    from pyannote_audio_amd import online
    from pyannote_audio_amd.core import SlidingWindow
    from pyannote_audio_amd.frames import frame_geometry
    frames = SlidingWindow(start=0.0, duration=FRAME_DURATION, step=FRAME_STEP)
    for duration, step in ((5.0, 0.5), (10.0, 1.0), (5.0, 0.1)):
        starts, _, _ = frame_geometry(SlidingWindow(start=0.0, duration=duration, step=step), frames, 5000)
        assert [online.start_frame(c, step, frames) for c in range(5000)] == starts.tolist()


# ---------------------------------------------------------------------------------------- the bank's host side
def _fake_models(dimension=8):
    import pyannote_audio_amd.model as pm

    class FakeResNet(pm.Model):
        ARCHITECTURE = pm.WeSpeakerResNet34.ARCHITECTURE
        dimension = 8

    seg = pm.PyanNet({}, {"sincnet": {"stride": 10, "sample_rate": 16000}, "sample_rate": 16000},
                     pm.segmentation_specifications(5.0, True))
    return seg, FakeResNet({}, {"sample_rate": 16000}, pm.embedding_specifications())


def _recording_bank(num_slots, **options):
    """a StreamBank on the host whose device step is replaced by a recorder: the engines are never reached"""
    from pyannote_audio_amd.online import StreamBank

    class Recording(StreamBank):
        def _advance(self, slots, start, emit_from, emit_to, flush=False):
            self.calls.append((slots.tolist(), start.tolist(), emit_from.tolist(), emit_to.tolist(), flush,
                               self.buffer[torch.as_tensor(slots, dtype=torch.long)].clone()))
            E = max(1, int((emit_to - emit_from).max()))
            return np.ones((len(slots), E, self.K), dtype=np.uint8)

    bank = Recording(*_fake_models(), num_slots, device=torch.device("cpu"), **options)
    bank.calls = []
    return bank


def test_bank_schedules_ready_slots_and_reuses_closed_ones():
    bank = _recording_bank(3, latency=2.0)
    assert (bank.window, bank.step_samples, bank.F, bank.S, bank.steps_per_window) == (80000, 8000, 293, 3, 10)
    assert bank.min_active_frames == round(0.25 / FRAME_STEP) and bank.min_update_frames == round(1.0 / FRAME_STEP)
    a, b = bank.open(), bank.open()
    assert (a, b) == (0, 1)
    block = lambda v, n=1: torch.full((n, 8000), float(v))      # noqa: E731
    for i in range(9):
        assert bank.push(block(i + 1, 2), [a, b]) == {}
    c = bank.open()
    assert c == 2
    out = bank.push(torch.stack([block(10)[0], block(1)[0]]), [a, c])         # a is ready, b lags, c just began
    assert list(out) == [a] and len(bank.calls) == 1
    slots, start, frm, to, flush, windows = bank.calls[0]
    bound = om.emit_bound(0, 0.5, 5.0, 2.0, FRAME_STEP, FRAME_DURATION)
    assert (slots, start, frm, to, flush) == ([a], [0], [0], [bound], False)
    assert windows[0].view(10, 8000)[:, 0].tolist() == [float(i + 1) for i in range(10)]
    assert out[a][0] == 0 and out[a][1].shape == (bound, bank.K)
    out = bank.push(block(11, 2), [b, a])                                      # both ready, in the order given
    assert list(out) == [b, a]
    slots, start, frm, to, flush, windows = bank.calls[1]
    assert slots == [b, a] and start == [0, om.start_frame(1, 0.5, FRAME_STEP, FRAME_DURATION)] and frm == [0, bound]
    assert windows[1].view(10, 8000)[:, 0].tolist() == [float(i + 2) for i in range(9)] + [11.0]
    with pytest.raises(ValueError):
        bank.push(block(0, 2), [a, a])
    with pytest.raises(RuntimeError):
        bank.open()

    # close: b has had exactly 10 steps and no tail -> no further chunk, one flush to the file's last frame
    n_calls = len(bank.calls)
    first, rows = bank.close(b)
    total = bank.calls[-1][3][0]
    assert len(bank.calls) == n_calls + 1 and bank.calls[-1][4] and bank.calls[-1][1] == [-1]
    assert first == bound and rows.shape[0] == total - bound
    from pyannote_audio_amd.core import SlidingWindow
    from pyannote_audio_amd.frames import frame_geometry
    _, num_frames, _ = frame_geometry(SlidingWindow(start=0.0, duration=5.0, step=0.5),
                                      SlidingWindow(start=0.0, duration=FRAME_DURATION, step=FRAME_STEP), 1)
    assert total == num_frames and bank.decisions(b).shape[0] == total
    with pytest.raises(ValueError):
        bank.push(block(0), [b])
    # the freed slot is handed out again, zeroed
    again = bank.open()
    assert again == b and not bank.buffer[b].any() and bank.decisions(b).shape[0] == 0
    assert bank.push(block(5), [again]) == {}


def test_bank_tail_rule():
    """a partial last block is zero-padded to one step and run; a stream shorter than a chunk gets one zero-padded
    chunk with its samples in front; the emission ends at the frames offline inference gives the file"""
    from pyannote_audio_amd.online import stream_num_frames
    bank = _recording_bank(2)
    a = bank.open()
    for i in range(10):
        bank.push(torch.full((1, 8000), float(i + 1)), [a])
    first, rows = bank.close(a, torch.full((3000,), 99.0))
    slots, start, frm, to, flush, windows = bank.calls[-2]
    total = stream_num_frames(83000, 80000, 8000, 16000, 5.0, 0.5, bank.frames)
    assert not flush and start == [om.start_frame(1, 0.5, FRAME_STEP, FRAME_DURATION)]
    w = windows[0]
    assert w[:72000].view(9, 8000)[:, 0].tolist() == [float(i + 2) for i in range(9)]
    assert (w[72000:75000] == 99.0).all() and not w[75000:].any()
    assert bank.calls[-1][4] and bank.calls[-1][3] == [total] and first + rows.shape[0] == total
    assert bank.decisions(a).shape[0] == total

    b = bank.open()
    bank.push(torch.full((1, 8000), 7.0), [b])
    first, rows = bank.close(b, torch.full((10,), 3.0))
    total = stream_num_frames(8010, 80000, 8000, 16000, 5.0, 0.5, bank.frames)
    chunk = [c for c in bank.calls if not c[4]][-1]
    assert chunk[1] == [0] and (chunk[5][0][:8000] == 7.0).all() and (chunk[5][0][8000:8010] == 3.0).all()
    assert not chunk[5][0][8010:].any()
    assert (first, rows.shape[0]) == (0, total) and 0 < total < 293

    c = bank.open()
    assert bank.close(c)[1].shape == (0, bank.K)          # nothing arrived: nothing to say


def test_bank_refuses_what_the_online_step_does_not_run():
    import pyannote_audio_amd.model as pm
    from pyannote_audio_amd.online import StreamBank
    seg, emb = _fake_models()
    cpu = torch.device("cpu")
    multilabel = pm.PyanNet({}, {"sample_rate": 16000}, pm.segmentation_specifications(5.0, False))
    with pytest.raises(NotImplementedError, match="powerset PyanNet"):
        StreamBank(multilabel, emb, 1, device=cpu)

    class FakeSSeRiouSS(pm.Model):
        ARCHITECTURE = pm.SSeRiouSS.ARCHITECTURE

    with pytest.raises(NotImplementedError, match="powerset PyanNet"):
        StreamBank(FakeSSeRiouSS({}, {}, pm.segmentation_specifications(5.0, True)), emb, 1, device=cpu)

    class FakeXVector(pm.Model):
        ARCHITECTURE = pm.XVectorSincNet.ARCHITECTURE

    with pytest.raises(NotImplementedError, match="WeSpeaker ResNet"):
        StreamBank(seg, FakeXVector({}, {}, pm.embedding_specifications()), 1, device=cpu)
    for latency in (0.25, 0.7, 5.5):
        with pytest.raises(ValueError, match="latency"):
            StreamBank(seg, emb, 1, latency=latency, device=cpu)
    with pytest.raises(ValueError, match="whole number"):
        StreamBank(seg, emb, 1, step=0.3, device=cpu)


def test_pipeline_is_registered():
    import pyannote_audio_amd
    from pyannote_audio_amd.online import OnlineSpeakerDiarization
    from pyannote_audio_amd.pipeline import get_class_by_name
    assert get_class_by_name("pyannote.audio.pipelines.OnlineSpeakerDiarization") is OnlineSpeakerDiarization
    assert pyannote_audio_amd.OnlineSpeakerDiarization is OnlineSpeakerDiarization
    seg, emb = _fake_models()
    pipeline = OnlineSpeakerDiarization(segmentation=seg, embedding=emb)
    assert type(pipeline.get_metric()).__name__ == "DiarizationErrorRate" and pipeline.get_direction() == "minimize"
    with pytest.raises(RuntimeError, match="GPU"):
        pipeline.bank(1)
