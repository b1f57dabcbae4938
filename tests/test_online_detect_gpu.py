"""`pao_detect_step` on the device against its numpy model (tests/online_detect_model.py), then `DetectionBank` and
`OnlineVoiceActivityDetection` end to end: against the model on the synthetic checkpoints and, at full latency, against
the offline pipelines.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import online_detect_model as dm

pytestmark = pytest.mark.gpu

F, S, N, ADV, E = 9, 3, 5, 3, 9
GRID = (0.0, 0.0619375, 0.016875)                 # the frame grid of a real model: the bits of the times matter
HI, LO = 0.9, 0.1
EPSILON = 1e-12
TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.uint8): torch.uint8,
            np.dtype(np.int32): torch.int32}


def _t(g):
    return dm.frame_time(g, *GRID)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _same(got, want):
    """arrays equal in dtype, shape and value, NaN in the same places"""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


class DeviceBank:
    """the state of a bank on the device and `pao_detect_step` through the C ABI, every output pre-filled with 0xA5"""

    def __init__(self, state, device):
        self.device = device
        self.state = {name: _dev(a, device) for name, a in state.items()}
        self.N, self.R, self.K = state["acc"].shape

    def host_state(self):
        return {name: t.cpu().numpy() for name, t in self.state.items()}

    def outputs(self, M, cap, E=E):
        shapes = (("values", (M, E, self.K), torch.float32), ("active", (M, E, self.K), torch.uint8),
                  ("counts", (M, self.K), torch.int32), ("regions", (M, self.K, cap, 2), torch.float64),
                  ("tracks", (M, self.K, cap), torch.int32))
        return {name: torch.full((int(np.prod(shape)) * dtype.itemsize,), 0xA5, dtype=torch.uint8,
                                 device=self.device).view(dtype).view(shape) for name, shape, dtype in shapes}

    def step(self, slots, scores, any, window, warm, missing, rows, onset, offset, min_on, min_off, cap, E=E,
             host_tables=True, grid=GRID, S=None):
        """rows (4, M) int64: start_frame, emit_from, emit_to, closing -> (return code, outputs on the host)"""
        import pyannote_audio_amd.ffi as ffi
        lib = ffi.load()
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        M = len(slots)
        d_scores, d_rows, d_slots = _dev(scores, self.device), _dev(rows, self.device), _dev(slots, self.device)
        d_window, d_warm = _dev(np.asarray(window, np.float64), self.device), _dev(np.asarray(warm, np.float64), self.device)
        on, off = np.ascontiguousarray(onset, np.float32), np.ascontiguousarray(offset, np.float32)
        d_on, d_off = np.ascontiguousarray(min_on, np.float64), np.ascontiguousarray(min_off, np.float64)
        outs = self.outputs(M, cap, E)
        st = self.state
        rc = lib.pao_detect_step(
            ffi.ptr(d_slots), slots.ctypes.data if host_tables else None, M, self.N, ffi.ptr(d_scores),
            int(scores.dtype == np.uint8), scores.shape[1], scores.shape[2] if S is None else S, int(any),
            ffi.ptr(d_window), ffi.ptr(d_warm), EPSILON, float(missing), ffi.ptr(d_rows[0]), ffi.ptr(d_rows[1]),
            ffi.ptr(d_rows[2]), ffi.ptr(d_rows[3]), rows.ctypes.data if host_tables else None, *grid, on.ctypes.data,
            off.ctypes.data, d_on.ctypes.data, d_off.ctypes.data, self.R, E, cap,
            *(ffi.ptr(st[name]) for name, _, _ in dm.STATE),
            *(ffi.ptr(outs[name]) for name in ("values", "active", "counts", "regions", "tracks")), ffi.stream())
        torch.cuda.synchronize()
        return rc, {name: t.cpu().numpy() for name, t in outs.items()}


# ------------------------------------------------------------------------------------------------------ the scenario
def _targets():
    """what the three streams are meant to look like, per global frame and class.  Stream "full" (48 frames), class 0:
    a region over pushes 0 - 5 with a 2-frame gap across a push boundary inside (merged), a value equal to the onset
    while inactive, a 2-frame region 4 frames later (final at its on-event; dropped by min_duration_on, its track
    counted), a region with a value equal to the offset inside, a region open at the close."""
    full = np.full((48, S), LO, dtype=np.float32)
    full[1:11, 0] = full[13:17, 0] = full[21:23, 0] = full[28:34, 0] = full[44:48, 0] = HI
    full[19, 0], full[30, 0] = 0.52, 0.48
    full[3:9, 1] = full[20:40, 1] = HI
    full[::5, 2] = full[1::5, 2] = HI
    second = np.full((30, S), LO, dtype=np.float32)
    second[3:9] = HI
    second[29] = HI                                   # an on-event on the last frame
    return full, second


def _chunks(rng, target, C):
    """(C, F, S): chunk c sees frames [3c, 3c + F) of the target through noise of its own"""
    return np.stack([target[ADV * c:ADV * c + F] for c in range(C)]) + \
        rng.normal(0, 0.01, (C, F, S)).astype(np.float32)


def _scenario():
    """per call: [(slot, scores (F, S), start_frame, emit_from, emit_to, closing)], slots 4, 0, 2 in that order"""
    rng = np.random.default_rng(77)
    full, second = _targets()
    a = _chunks(rng, full, 14)                                     # slot 4: full latency, 48 frames
    for c in range(14):                                            # frames 5, 6 of class 1: NaN in every chunk ...
        for g in (5, 6):
            if 0 <= g - ADV * c < F:
                a[c, g - ADV * c, 1] = np.nan
    a[3, 4, 0] = a[5, 2, 2] = a[9, 8, 1] = np.nan                  # ... and NaN in single chunks
    b = _chunks(rng, full, 14)                                     # slot 0: latency = step
    b[2, :, 2] = np.nan
    d = _chunks(rng, second, 8)                                    # slot 2, second stream: 30 frames
    zero = np.zeros((F, S), dtype=np.float32)
    calls = [[] for _ in range(15)]
    for c in range(14):
        calls[c].append((4, a[c], ADV * c, ADV * c, ADV * c + ADV, 0))
    calls[14].append((4, zero, -1, 42, 48, 1))                     # the flush closes with a region open
    emitted = 0
    for c in range(14):
        calls[c].append((0, b[c], ADV * c, emitted, ADV * c + F, 0))
        emitted = ADV * c + F
    calls[14].append((0, zero, -1, 48, 48, 1))                     # a flush row that emits nothing
    calls[0].append((2, np.full((F, S), HI, dtype=np.float32), 0, 0, 1, 0))      # a stream of one frame
    calls[1].append((2, zero, -1, 1, 1, 1))
    calls[2].append(("reset", 2))
    for c in range(8):
        calls[3 + c].append((2, d[c], ADV * c, ADV * c, ADV * c + ADV, 0))
    calls[11].append((2, zero, -1, 24, 30, 1))
    return calls


def _garbage_state(rng, R, K):
    """unlisted slots hold arbitrary bytes"""
    state = dm.fresh_state(N, R, K)
    for slot in (1, 3):
        for name, a in state.items():
            a[slot] = rng.integers(0, 256, size=a[slot].nbytes, dtype=np.uint8).view(a.dtype).reshape(a[slot].shape)
    return state


def _thresholds(mode, any, window, warm, R):
    """"lt": onset / offset of class 0 are VALUES the full-latency stream emits (frames 19 and 30), found with the
    model; "gt": offset > onset"""
    K = 1 if any else S
    if mode == "gt":
        return [0.4 + 0.01 * k for k in range(K)], [0.6 + 0.01 * k for k in range(K)]
    state = dm.fresh_state(N, R, K)
    values = {}
    for call in _scenario():
        for entry in call:
            if entry[0] == 4:
                _, scores, g0, ga, gb, closing = entry
                out = dm.detect_step_one(state, 4, scores, any, window, warm, EPSILON, 0.0, g0, ga, gb, closing, GRID,
                                         [0.5] * K, [0.5] * K, [0.0] * K, [0.0] * K, E, E // 2 + 2)
                for g in range(ga, gb):
                    values[g] = out[0][g - ga]
    onset, offset = [0.55] * K, [0.45] * K
    if not any:
        onset[0], offset[0] = float(values[19][0]), float(values[30][0])
        assert 0.5 < onset[0] < 0.54 and 0.46 < offset[0] < 0.5
    return onset, offset


@pytest.mark.parametrize("mode", ["lt", "gt"])
@pytest.mark.parametrize("ring", ["roomy", "minimal"])
@pytest.mark.parametrize("any", [False, True], ids=["classes", "any"])
def test_detect_step_equals_the_model_over_a_sequence(gpu_device, any, ring, mode):
    K = 1 if any else S
    R = 2 * F + 16 if ring == "roomy" else F + E
    cap = E // 2 + 2
    window, warm = np.hamming(F), np.ones(F)
    warm[:1] = warm[F - 1:] = EPSILON
    missing = 0.0 if mode == "lt" else np.nan
    onset, offset = _thresholds(mode, any, window, warm, R)
    min_on, min_off = ([0.04, 0.0, 0.04], [0.045, 0.045, 0.0]) if not any else ([0.04], [0.045])
    state = _garbage_state(np.random.default_rng(5), R, K)
    before = dm.copy_state(state)
    bank = DeviceBank(state, gpu_device)
    finals = {4: [], 0: [], 2: []}                     # slot -> [(call, class, start, end, track)]
    wrapped = 0
    for index, call in enumerate(_scenario()):
        for entry in [e for e in call if e[0] == "reset"]:
            for name in state:
                state[name][entry[1]] = 0
                bank.state[name][entry[1]].zero_()
        entries = [e for e in call if e[0] != "reset"]
        slots = [e[0] for e in entries]
        scores = np.stack([e[1] for e in entries])
        rows = np.array([[e[i] for e in entries] for i in (2, 3, 4, 5)], dtype=np.int64)
        want = dm.detect_step(state, slots, scores, any, window, warm, EPSILON, missing, *rows, GRID, onset, offset,
                              min_on, min_off, E, cap)
        rc, got = bank.step(slots, scores, any, window, warm, missing, rows, onset, offset, min_on, min_off, cap)
        assert rc == 0
        for name, w in zip(("values", "active", "counts", "regions", "tracks"), want):
            assert _same(got[name], w), f"call {index}: {name}"
        assert dm.same_state(bank.host_state(), state), f"call {index}: state"
        for m, slot in enumerate(slots):
            finals[slot] += [(index, k, *want[3][m, k, i], int(want[4][m, k, i]))
                             for k in range(K) for i in range(want[2][m, k])]
        wrapped = max(wrapped, int(rows[2].max()) // R)
    assert wrapped >= 1                                                        # the ring wrapped
    for slot in (1, 3):                                                        # unlisted slots: not a bit changed
        assert all(state[name][slot].tobytes() == before[name][slot].tobytes() for name in state)
    assert all(len(v) >= 1 for v in finals.values()) or any
    if mode == "lt" and not any:
        class0 = [r for r in finals[4] if r[1] == 0]
        # merged over the push boundary and final at the on-event of frame 21 (call 7); the 2-frame region is dropped
        # and counted; the value equal to the onset (frame 19) opened nothing, the one equal to the offset (frame 30)
        # closed nothing; the last region was open at the close
        assert class0 == [(7, 0, _t(1), _t(17), 0), (14, 0, _t(28), _t(34), 2), (14, 0, _t(44), _t(47), 3)]
        # the one-frame stream and the on-event on the last frame (frame 29, in the flush of call 11) gave nothing; that
        # on-event made the region pending since call 6 final
        assert [r[:1] + r[2:4] for r in finals[2] if r[1] == 0] == [(11, _t(3), _t(9))]
        assert not [r for r in finals[2] if r[0] <= 2]
    if mode == "gt":
        assert all(on < off for on, off in zip(onset, offset))


@pytest.mark.parametrize("S_", [1, 3, 16])
def test_hard_decisions_give_the_bits_of_their_float_image(gpu_device, S_):
    """`any` on uint8 hard decisions (any non-zero byte counts as 1) and on the same decisions as float32"""
    rng = np.random.default_rng(S_)
    R, cap, M = F + E, E // 2 + 2, 2
    window, warm = np.hamming(F), np.ones(F)
    speech = np.zeros(6 * ADV + F, dtype=bool)                       # per global frame: somebody speaks
    speech[2:8] = speech[12:14] = speech[17:22] = True
    hard = np.zeros((6, M, F, S_), dtype=np.uint8)
    for c, m, f in np.ndindex(6, M, F):
        if speech[ADV * c + f] != (rng.random() < 0.1):             # (a chunk in ten disagrees)
            hard[c, m, f, rng.integers(0, S_)] = rng.integers(1, 256)
    banks = [DeviceBank(dm.fresh_state(3, R, 1), gpu_device) for _ in range(2)]
    state = dm.fresh_state(3, R, 1)
    regions = 0
    for c in range(7):
        last = c == 6
        rows = np.array([[-1 if last else ADV * c] * M, [ADV * c] * M, [ADV * c + (F - ADV if last else ADV)] * M,
                         [int(last)] * M])
        x = hard[min(c, 5)]
        args = (True, window, warm, 0.0, rows, [0.5], [0.5], [0.02], [0.03], cap)
        rc_u, got_u = banks[0].step([2, 0], x, *args)
        rc_f, got_f = banks[1].step([2, 0], (x != 0).astype(np.float32), *args)
        want = dm.detect_step(state, [2, 0], x, True, window, warm, EPSILON, 0.0, *rows, GRID, [0.5], [0.5], [0.02],
                              [0.03], E, cap)
        assert rc_u == 0 and rc_f == 0
        for name, w in zip(("values", "active", "counts", "regions", "tracks"), want):
            assert got_u[name].tobytes() == got_f[name].tobytes() and _same(got_u[name], w), (c, name)
        assert dm.same_state(banks[0].host_state(), state) and dm.same_state(banks[1].host_state(), state)
        regions += int(want[2].sum())
    assert regions >= 2


def test_an_inconsistent_stream_on_the_device_keeps_its_state(gpu_device):
    """without host tables the device checks alone: the stream whose frames are inconsistent gets NaN / 0 / -1 rows
    and keeps its state, its neighbour is served"""
    rng = np.random.default_rng(9)
    R, cap, K = F + E, E // 2 + 2, S
    state = dm.fresh_state(3, R, K)
    state["acc"][:] = rng.random(state["acc"].shape).astype(np.float32)
    state["cnt"][:] = 1.0
    state["msk"][:] = 1
    state["on"][:] = 1
    state["open_start"][:] = _t(2)
    before = dm.copy_state(state)
    bank = DeviceBank(state, gpu_device)
    scores = rng.random((2, F, S)).astype(np.float32)
    rows = np.array([[12, 12], [12, 9], [10, 15], [0, 1]])                      # entry 0: emit_from > emit_to
    window, warm = np.ones(F), np.ones(F)
    rc, got = bank.step([1, 2], scores, False, window, warm, 0.0, rows, [0.5] * K, [0.5] * K, [0.0] * K, [0.0] * K, cap,
                        host_tables=False)
    assert rc == 0
    want = dm.detect_step(state, [2], scores[1:], False, window, warm, EPSILON, 0.0, *rows[:, 1:], GRID, [0.5] * K,
                          [0.5] * K, [0.0] * K, [0.0] * K, E, cap)
    for name, w in zip(("values", "active", "counts", "regions", "tracks"), want):
        assert _same(got[name][1:], w), name
    assert np.isnan(got["values"][0]).all() and not got["active"][0].any() and not got["counts"][0].any()
    assert np.isnan(got["regions"][0]).all() and (got["tracks"][0] == -1).all()
    assert dm.same_state(bank.host_state(), state)
    assert all(state[name][1].tobytes() == before[name][1].tobytes() for name in state)
    assert want[2].sum() >= 1


def test_the_largest_emission_the_limits_allow(gpu_device):
    """E K = 12 288 values, what `pao_detect_limits` exports: 60 KB of LDS per workgroup, launched and equal to the
    model (16 classes, 768 frames, the minimal ring; a chunk that emits all of E and a closing flush)"""
    rng = np.random.default_rng(12)
    S_, E_ = 16, 768
    R, cap = F + E_, E_ // 2 + 2
    state = dm.fresh_state(2, R, S_)
    state["cnt"][:] = rng.random(state["cnt"].shape).astype(np.float32) + 0.5
    state["acc"][:] = state["cnt"] * np.repeat(rng.random((2, R // 3, S_)) < 0.5, 3, axis=1).astype(np.float32)
    state["msk"][:] = rng.random(state["msk"].shape) < 0.97
    state["on"][:] = rng.integers(0, 2, state["on"].shape)
    state["open_start"][:] = _t(990)
    bank = DeviceBank(state, gpu_device)
    scores = rng.random((2, F, S_)).astype(np.float32)
    rows = np.array([[1760, -1], [1000, 1005], [1768, 1773], [0, 1]], dtype=np.int64)
    window, warm = np.hamming(F), np.ones(F)
    params = ([0.5] * S_, [0.5] * S_, [0.03] * S_, [0.0] * 8 + [0.04] * 8)
    want = dm.detect_step(state, [1, 0], scores, False, window, warm, EPSILON, 0.0, *rows, GRID, *params, E_, cap)
    rc, got = bank.step([1, 0], scores, False, window, warm, 0.0, rows, *params, cap, E=E_)
    assert rc == 0
    for name, w in zip(("values", "active", "counts", "regions", "tracks"), want):
        assert _same(got[name], w), name
    assert dm.same_state(bank.host_state(), state)
    assert want[2].min() >= 20 and E_ * S_ == 12288


def test_every_refusal_returns_3_and_writes_nothing(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    from refusals import check_refusal
    lib, dev = ffi.load(), gpu_device
    limits = (ffi.C.c_int(0), ffi.C.c_int(0))
    assert lib.pao_detect_limits(ffi.C.byref(limits[0]), ffi.C.byref(limits[1])) == 0
    assert (limits[0].value, limits[1].value) == (16, 12288)

    def refused(message, M=2, S=S, any=0, uint8=False, R=F + E, E=E, cap=E // 2 + 2, slots=(0, 1), rows=None,
                onset=0.5, offset=0.5, min_on=0.0, min_off=0.0, grid=GRID, columns=None):
        """a call with full-size buffers (`columns`: what the score buffer really has when S is not to be believed)"""
        K = 1 if any else max(S, 1)
        width = S if columns is None else columns
        scores = torch.zeros((M, F, width), dtype=torch.uint8 if uint8 else torch.float32, device=dev)
        weights = torch.ones((2, F), dtype=torch.float64, device=dev)
        slots = np.array(slots, dtype=np.int32)
        rows = np.array([[0] * M, [0] * M, [3] * M, [0] * M] if rows is None else rows, dtype=np.int64)
        d_slots, d_rows = _dev(slots, dev), _dev(rows, dev)
        on, off = np.full(16, onset, np.float32), np.full(16, offset, np.float32)
        d_on, d_off = np.full(16, min_on, np.float64), np.full(16, min_off, np.float64)
        room = max(cap, 1)
        # state and outputs, float64 as pairs of int32 (the pattern of refusals.py has no float64)
        outputs = [((N, R, K), torch.float32), ((N, R, K), torch.float32), ((N, R, K), torch.uint8),
                   ((N, K), torch.uint8), ((N, K, 2), torch.int32), ((N, K, 4), torch.int32), ((N, K), torch.uint8),
                   ((N, K), torch.int32), ((M, E, K), torch.float32), ((M, E, K), torch.uint8), ((M, K), torch.int32),
                   ((M, K, room, 4), torch.int32), ((M, K, room), torch.int32)]
        check_refusal(lambda *p: lib.pao_detect_step(
            ffi.ptr(d_slots), slots.ctypes.data, M, N, ffi.ptr(scores), int(uint8), F, S, any, ffi.ptr(weights[0]),
            ffi.ptr(weights[1]), EPSILON, 0.0, ffi.ptr(d_rows[0]), ffi.ptr(d_rows[1]), ffi.ptr(d_rows[2]),
            ffi.ptr(d_rows[3]), rows.ctypes.data, *grid, on.ctypes.data, off.ctypes.data, d_on.ctypes.data,
            d_off.ctypes.data, R, E, cap, *p, ffi.stream()), outputs, "pao_detect_step: " + message, dev)

    nan = float("nan")
    refused("0 score columns per frame, the kernel handles 1..16", S=0, columns=1)
    refused("17 score columns per frame, the kernel handles 1..16", S=17)
    refused("17 score columns per frame, the kernel handles 1..16", S=17, any=1)
    refused("uint8 scores are the hard multilabel output, any = 1 only", uint8=True)
    refused("a ring of 17 frames is shorter than F + E = 9 + 9", R=F + E - 1)
    refused("12289 frames of 1 classes per emission, at most 12288 values fit the workgroup's LDS", any=1, E=12289,
            R=F + 12289, cap=12289 // 2 + 2)
    refused("room for 5 regions per class, an emission of 9 frames can finalise 6", cap=E // 2 + 1)
    refused("a threshold or a duration of class 0 is NaN", onset=nan)
    refused("a threshold or a duration of class 0 is NaN", offset=nan)
    refused("a threshold or a duration of class 0 is NaN", min_on=nan)
    refused("a threshold or a duration of class 0 is NaN", min_off=nan)
    for i in range(3):
        refused("the frame grid has a NaN", grid=tuple(nan if j == i else v for j, v in enumerate(GRID)))
    refused("duplicate slot 1 (entries 0 and 1): one workgroup owns one stream", slots=(1, 1))
    refused("slot 5 (entry 1) outside the bank of 5", slots=(0, 5))
    refused("slot -1 (entry 0) outside the bank of 5", slots=(-1, 0))
    frames = "inconsistent frames of entry 1: chunk at {} (F = 9), emission [{}, {}), closing {}, E = 9, R = 18"
    refused(frames.format(0, 4, 3, 0), rows=[[0, 0], [0, 4], [3, 3], [0, 0]])            # emit_from > emit_to
    refused(frames.format(0, 0, 10, 0), rows=[[0, 0], [0, 0], [3, 10], [0, 0]])          # more than E frames
    refused(frames.format(10, 0, 3, 0), rows=[[0, 10], [0, 0], [3, 3], [0, 0]])          # the chunk leaves the ring
    refused(frames.format(0, -1, 3, 0), rows=[[0, 0], [0, -1], [3, 3], [0, 0]])          # a negative frame
    refused(frames.format(0, 0, 3, 2), rows=[[0, 0], [0, 0], [3, 3], [0, 2]])            # closing is 0 or 1


def test_the_python_call_is_the_c_call(gpu_device):
    """`online_detection.detect_step`: the outputs are views of one buffer, and they are the model's"""
    from pyannote_audio_amd.core import SlidingWindow
    from pyannote_audio_amd.online_detection import DetectionState, detect_limits, detect_step
    assert detect_limits() == (16, 12288)
    rng = np.random.default_rng(21)
    R, K = F + E, S
    state = dm.fresh_state(N, R, K)
    d_state = DetectionState(N, R, K, gpu_device)
    window, warm = np.hamming(F), np.ones(F)
    frames = SlidingWindow(start=GRID[0], duration=GRID[1], step=GRID[2])
    onset, offset, min_on, min_off = [0.6, 0.5, 0.4], [0.4, 0.5, 0.6], [0.0, 0.02, 0.0], [0.03, 0.0, 0.0]
    found = 0
    for c in range(6):
        last = c == 5
        scores = (rng.random((2, F, S)) < 0.5).astype(np.float32) * 0.8 + 0.1
        rows = np.array([[ADV * c] * 2, [ADV * c] * 2, [ADV * c + (F if last else ADV)] * 2, [int(last)] * 2])
        want = dm.detect_step(state, [3, 1], scores, False, window, warm, EPSILON, 0.0, *rows, GRID, onset, offset,
                              min_on, min_off, E, E // 2 + 2)
        out = detect_step([3, 1], _dev(scores, gpu_device), _dev(window, gpu_device), _dev(warm, gpu_device), *rows,
                          d_state, frames, onset, offset, min_on, min_off, E=E)
        lo, hi = out.buffer.data_ptr(), out.buffer.data_ptr() + out.buffer.numel()
        for t, w in zip(out[1:], want):
            assert lo <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= hi and t.data_ptr() % 8 == 0
            assert _same(t.cpu().numpy(), w)
        assert dm.same_state({name: getattr(d_state, name).cpu().numpy() for name, _, _ in dm.STATE}, state)
        found += int(want[2].sum())
    assert found >= 3
    with pytest.raises(ValueError, match="uint8 scores are the hard multilabel output"):
        detect_step([0], torch.zeros((1, F, S), dtype=torch.uint8, device=gpu_device), _dev(window, gpu_device),
                    _dev(warm, gpu_device), [0], [0], [3], [0], d_state, frames, 0.5, 0.5, E=E)


# -------------------------------------------------------------------------------------------- the bank, end to end
CLASSES = ["speech", "music", "noise"]
THRESHOLDS = {"speech": {"onset": 0.6, "offset": 0.4, "min_duration_on": 0.0, "min_duration_off": 0.0},
              "music": {"onset": 0.4, "offset": 0.6, "min_duration_on": 0.05, "min_duration_off": 0.1},
              "noise": {"onset": 0.5, "offset": 0.5, "min_duration_on": 0.1, "min_duration_off": 0.0}}


@pytest.fixture(scope="module")
def powerset_model(gpu_device, synthetic_models):
    import pyannote_audio_amd.model as pm
    from conftest import PYANNET_HPARAMS
    return pm.PyanNet(synthetic_models[0].state_dict(), PYANNET_HPARAMS,
                      pm.segmentation_specifications(5.0, True)).to(gpu_device)


@pytest.fixture(scope="module")
def multilabel_model(gpu_device):
    import pyannote_audio_amd.model as pm
    from conftest import PYANNET_HPARAMS
    from oracle.synthetic import calibrated_multilabel_pyannet
    spec = pm.Specifications(problem=pm.Problem.MULTI_LABEL_CLASSIFICATION, resolution=pm.Resolution.FRAME,
                             duration=5.0, min_duration=None, warm_up=(0.0, 0.0), classes=list(CLASSES),
                             permutation_invariant=False)
    return pm.PyanNet(calibrated_multilabel_pyannet(calib_seconds=40.0).state_dict(), PYANNET_HPARAMS, spec).to(gpu_device)


@pytest.fixture(scope="module")
def waves():
    from oracle.synthetic import synth_conversation
    return {seconds: synth_conversation(seconds, seed=60 + seed)[0].view(-1)
            for seed, seconds in enumerate((7.3, 12.0, 3.1, 6.0))}


class ModelBank:
    """the bank written again for the test: host audio, the same engine call with the same batch composition, then the
    numpy model of the kernel"""

    def __init__(self, bank):
        self.b = bank
        self.state = dm.fresh_state(bank.num_slots, bank.R, bank.K)
        self.window = bank._window.cpu().numpy()
        self.warm = bank._warm.cpu().numpy()
        self.grid = (bank.grid.start, bank.grid.duration, bank.grid.step)
        self.audio = {}

    def open(self, slot):
        for a in self.state.values():
            a[slot] = 0
        self.audio[slot] = dict(wav=np.zeros(0, dtype=np.float32), chunks=0, emitted=0, values=[], active=[],
                                regions=[[] for _ in range(self.b.K)], tracks=[[] for _ in range(self.b.K)])

    def _step(self, ready, rows, windows=None):
        """ready slots, rows (4, M); windows (M, window) or None for a flush -> the model's outputs"""
        b = self.b
        M = len(ready)
        if windows is None:
            scores = np.zeros((M, b.F, b.S), dtype=np.uint8 if b.hard else np.float32)
        else:
            flat = _dev(windows, b.device).view(-1)
            logp, ml = b.model.engine.forward_strided(flat, b.window, M, b.window, want_logp=not b.hard,
                                                      want_multilabel=b.hard)
            scores = (ml if b.hard else logp).cpu().numpy()
        E_ = max(1, int((rows[2] - rows[1]).max()))
        out = dm.detect_step(self.state, ready, scores, b.any, self.window, self.warm, b.epsilon, b.missing, *rows,
                             self.grid, b.onset, b.offset, b.min_duration_on, b.min_duration_off, E_, E_ // 2 + 2)
        result = {}
        for i, slot in enumerate(ready):
            st, n = self.audio[slot], int(rows[2][i] - rows[1][i])
            st["values"].append(out[0][i, :n])
            st["active"].append(out[1][i, :n])
            final = [out[3][i, k, :out[2][i, k]] for k in range(b.K)]
            for k in range(b.K):
                st["regions"][k].append(final[k])
                st["tracks"][k].append(out[4][i, k, :out[2][i, k]])
            result[slot] = (int(rows[1][i]), out[0][i, :n], out[1][i, :n], final)
            st["emitted"] = int(rows[2][i])
        return result

    def _rows(self, ready, limit=None):
        import online_model as om
        b = self.b
        rows = np.zeros((4, len(ready)), dtype=np.int64)
        for i, slot in enumerate(ready):
            st = self.audio[slot]
            start = om.start_frame(st["chunks"], b.step, b.frames.step, b.frames.duration)
            bound = om.emit_bound(st["chunks"], b.step, b.duration, b.latency, b.frames.step, b.frames.duration)
            to = max(min(bound, start + b.F, limit if limit is not None else bound), st["emitted"])
            rows[:, i] = (start, st["emitted"], to, 0)
            st["chunks"] += 1
        return rows

    def push(self, blocks, slots):
        b, ready = self.b, []
        for block, slot in zip(blocks, slots):
            st = self.audio[slot]
            st["wav"] = np.concatenate([st["wav"], block])
            if len(st["wav"]) >= b.window:
                ready.append(slot)
        if not ready:
            return {}
        return self._step(ready, self._rows(ready), np.stack([self.audio[s]["wav"][-b.window:] for s in ready]))

    def close(self, slot, tail):
        from pyannote_audio_amd.online import stream_num_frames
        b, st = self.b, self.audio[slot]
        wav = st["wav"] if tail is None else np.concatenate([st["wav"], tail])
        total = stream_num_frames(len(wav), b.window, b.step_samples, b.sample_rate, b.duration, b.step, b.frames)
        padded = np.concatenate([wav, np.zeros((-len(wav)) % b.step_samples, dtype=np.float32)])
        if len(wav) < b.window:
            window = np.concatenate([wav, np.zeros(b.window - len(wav), dtype=np.float32)])
            self._step([slot], self._rows([slot], total), window[None])
        elif tail is not None and len(tail):
            self._step([slot], self._rows([slot], total), padded[-b.window:][None])
        self._step([slot], np.array([[-1], [st["emitted"]], [max(total, st["emitted"])], [1]], dtype=np.int64))
        return total


def _cat(parts, empty):
    return np.concatenate(parts) if parts else empty


def _run_bank(bank, waves, plan, pushes, gpu_device):
    """streams opened at different pushes, closed with their tails, a slot reused; every push and every close
    compared with the model -> per stream (seconds, values, regions per class, tracks per class)"""
    ref = ModelBank(bank)
    step = bank.step_samples
    live, done = {}, []
    for push in range(pushes):
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
            total = ref.close(slot, tail)
            st = ref.audio[slot]
            values = _cat(st["values"], np.zeros((0, bank.K), np.float32))
            assert values.shape == (total, bank.K) and _same(bank.values(slot), values), f"{seconds}-s stream: values"
            assert _same(bank.active(slot), _cat(st["active"], np.zeros((0, bank.K), np.uint8)))
            regions, tracks = bank.regions(slot, return_tracks=True)
            for k in range(bank.K):
                assert _same(regions[k], _cat(st["regions"][k], np.zeros((0, 2)))), f"{seconds}-s stream, class {k}"
                assert _same(tracks[k], _cat(st["tracks"][k], np.zeros(0, np.int32)))
            done.append((seconds, values, regions, tracks, bank.annotation(slot, uri=f"stream{seconds}")))
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
            assert got[s][0] == want[s][0] and _same(got[s][1], want[s][1]) and _same(got[s][2], want[s][2])
            assert all(_same(a, b) for a, b in zip(got[s][3], want[s][3])), f"push {push}, slot {s}: final regions"
    assert not live
    return done


def _rows_of(annotation):
    return [(s.start, s.end, t, l) for s, t, l in annotation.itertracks(yield_label=True)]


def test_powerset_bank_end_to_end_equals_the_model_loop(gpu_device, powerset_model, waves):
    """streams of 7.3 s, 3.1 s (shorter than a chunk) and 12 s, the 3.1-s one closed and its slot reused by a 6-s one;
    latency of four steps, so that values leave before every chunk covering them is in"""
    from pyannote_audio_amd.online_detection import DetectionBank
    bank = DetectionBank(powerset_model, 3, latency=2.0, min_duration_on=0.05, min_duration_off=0.08,
                         keep_frames=True, device=gpu_device)
    assert (bank.K, bank.classes, bank.hard) == (1, ["SPEECH"], True)
    plan = {0: [(7.3, 0)], 1: [(3.1, 1), (6.0, 9)], 2: [(12.0, 3)]}
    done = _run_bank(bank, waves, plan, 40, gpu_device)
    assert sorted(s for s, *_ in done) == [3.1, 6.0, 7.3, 12.0]
    assert sum(len(regions[0]) for _, _, regions, _, _ in done) >= 3
    for seconds, _, regions, _, annotation in done:
        assert annotation.uri == f"stream{seconds}" and annotation.labels() in ([], ["SPEECH"])
        assert [r[:2] for r in _rows_of(annotation)] == [tuple(r) for r in regions[0].tolist()]


def _multilabel_bank(model, num_slots, device, **options):
    from pyannote_audio_amd.online_detection import DetectionBank
    per = [THRESHOLDS[c] for c in CLASSES]
    return DetectionBank(model, num_slots, any=False, onset=[t["onset"] for t in per],
                         offset=[t["offset"] for t in per], min_duration_on=[t["min_duration_on"] for t in per],
                         min_duration_off=[t["min_duration_off"] for t in per], device=device, **options)


def test_multilabel_bank_end_to_end_equals_the_model_loop(gpu_device, multilabel_model, waves):
    bank = _multilabel_bank(multilabel_model, 2, gpu_device, latency=0.5, keep_frames=True)
    assert (bank.K, bank.classes, bank.hard) == (3, CLASSES, False)
    done = _run_bank(bank, waves, {0: [(7.3, 0), (6.0, 16)], 1: [(3.1, 2)]}, 40, gpu_device)
    assert sorted(s for s, *_ in done) == [3.1, 6.0, 7.3]
    assert sum(len(r) for _, _, regions, _, _ in done for r in regions) >= 3


def test_the_bank_takes_these_models_only(gpu_device, powerset_model, multilabel_model):
    from pyannote_audio_amd.online_detection import DetectionBank
    with pytest.raises(NotImplementedError, match="powerset = True, any = False"):
        DetectionBank(powerset_model, 1, any=False, device=gpu_device)
    with pytest.raises(NotImplementedError, match="powerset = False, any = True"):
        DetectionBank(multilabel_model, 1, device=gpu_device)
    with pytest.raises(ValueError, match="latency"):
        DetectionBank(powerset_model, 1, latency=0.7, device=gpu_device)


def test_frames_are_kept_on_request_only(gpu_device, powerset_model, waves):
    """a live stream runs for days: without `keep_frames` the bank holds a stream's final regions and nothing per frame"""
    from pyannote_audio_amd.online_detection import DetectionBank
    results = []
    for keep in (False, True):
        bank = DetectionBank(powerset_model, 1, keep_frames=keep, device=gpu_device)
        slot, wav, step = bank.open(), waves[7.3], bank.step_samples
        pushed = [bank.push(wav[at:at + step][None], [slot]) for at in range(0, wav.numel() - step + 1, step)]
        last = bank.close(slot, wav[wav.numel() // step * step:])
        values = np.concatenate([p[slot][1] for p in pushed if p] + [last[1]])
        results.append((values, bank.regions(slot), bank.values(slot), bank.active(slot)))
        assert len(bank._streams[slot].values) == (len([p for p in pushed if p]) + 2 if keep else 0)
    assert _same(results[0][0], results[1][0]) and _same(results[0][1][0], results[1][1][0])
    assert results[0][2].shape == (0, 1) and results[0][3].shape == (0, 1) and _same(results[1][2], results[1][0])
    assert len(results[0][1][0]) >= 1


# ----------------------------------------------------------------------------------- full latency: the offline pipelines
def _clips():
    """tests/golden/sample.wav, a clip shorter than one chunk and a clip with a ragged tail"""
    import wave
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample.wav")
    with wave.open(path) as w:
        assert (w.getframerate(), w.getnchannels(), w.getsampwidth()) == (16000, 1, 2)
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16)
    sample = torch.from_numpy(pcm.astype(np.float32) / 32768.0)[None]
    return [{"waveform": sample, "sample_rate": 16000, "uri": "sample"},
            {"waveform": sample[:, 40000:40000 + 51234], "sample_rate": 16000, "uri": "short"},
            {"waveform": sample[:, 100000:100000 + 116801], "sample_rate": 16000, "uri": "ragged"}]


@pytest.mark.parametrize("durations", [(0.0, 0.0), (0.2, 0.15)])
def test_online_vad_at_full_latency_is_voice_activity_detection(gpu_device, powerset_model, durations):
    import pyannote_audio_amd as pa
    params = {"min_duration_on": durations[0], "min_duration_off": durations[1]}
    offline = pa.VoiceActivityDetection(segmentation=powerset_model, step=0.5).to(gpu_device).instantiate(params)
    online = pa.OnlineVoiceActivityDetection(segmentation=powerset_model, step=0.5).to(gpu_device).instantiate(params)
    assert online.classes() == offline.classes() and online.get_direction() == offline.get_direction()
    assert type(online.get_metric()) is type(offline.get_metric())
    assert online.default_parameters() == offline.default_parameters()
    assert sorted(online.parameters()) == sorted(offline.parameters())
    found = 0
    for file in _clips():
        want = offline.apply(dict(file))
        got = online.apply(dict(file))
        assert _rows_of(got) == _rows_of(want), file["uri"]
        assert got.uri == want.uri == file["uri"]
        found += len(_rows_of(want))
    assert found >= 3


def _stream_clip(bank, file):
    wav = file["waveform"].view(-1)
    slot, at, step = bank.open(), 0, bank.step_samples
    while wav.numel() - at >= step:
        bank.push(wav[at:at + step][None], [slot])
        at += step
    bank.close(slot, wav[at:] if wav.numel() > at else None)
    return bank.annotation(slot, uri=file["uri"])


def _multilabel_offline(model, device):
    import pyannote_audio_amd as pa
    offline = pa.MultiLabelSegmentation(segmentation=model, step=0.5).to(device)
    offline.instantiate({"thresholds": THRESHOLDS})
    assert any(t["offset"] > t["onset"] for t in THRESHOLDS.values())
    return offline


def test_multilabel_bank_at_full_latency_is_multilabel_segmentation(gpu_device, multilabel_model):
    """The multi-label bank at full latency == `MultiLabelSegmentation.apply`, per-class thresholds included, on
    recordings of ONE chunk (shorter than a chunk, and exactly a chunk): there the offline forward and the bank's run
    the same per-chunk sinc layer, so the float32 chunk scores are the same bits.  From two overlapping chunks on the
    offline forward shares one sinc layer over the file's span (`sincnet_plan_span`) and its scores differ from a
    streamed forward's in the last bits (at most 1.13e-4 measured on the 6-chunk clip below, where one aggregated
    value is 0.5000196 offline and 0.4999908 streamed at a threshold of 0.5 and one region start moves by two
    frames); the next test holds those recordings to the contract on the offline scores."""
    offline = _multilabel_offline(multilabel_model, gpu_device)
    bank = _multilabel_bank(multilabel_model, 1, gpu_device)
    sample = _clips()[0]["waveform"]
    found = []
    for uri, lo, n in (("short", 40000, 51234), ("short-2", 200000, 30000), ("one-chunk", 100000, 80000)):
        file = {"waveform": sample[:, lo:lo + n], "sample_rate": 16000, "uri": uri}
        want = offline.apply(dict(file))
        got = _stream_clip(bank, file)
        assert _rows_of(got) == _rows_of(want) and got.uri == uri, uri
        found += _rows_of(want)
    assert len(found) >= 1


@pytest.mark.parametrize("clip", [0, 2], ids=["sample", "ragged"])
def test_multilabel_bank_on_the_offline_chunk_scores_is_multilabel_segmentation(gpu_device, multilabel_model, clip):
    """recordings of many chunks (30 s; a ragged tail): the bank streams the audio, and its forward hands back the
    chunk scores the OFFLINE forward computed for the same chunk.  Given the same chunk scores the streamed regions
    are `MultiLabelSegmentation.apply`'s, per-class thresholds included"""
    offline = _multilabel_offline(multilabel_model, gpu_device)
    file = _clips()[clip]
    want = offline.apply(dict(file))
    chunks = offline._segmentation.last_device_output.clone()              # (C, F, S) float32: what `apply` aggregated
    bank = _multilabel_bank(multilabel_model, 1, gpu_device)
    engine, calls = bank.model.engine, []

    def offline_scores(flat, stride, count, window, **kwargs):
        assert count == 1
        calls.append(len(calls))
        return chunks[calls[-1]:calls[-1] + 1].contiguous(), None

    engine.forward_strided = offline_scores
    try:
        got = _stream_clip(bank, file)
    finally:
        del engine.forward_strided                                         # (the instance attribute: the method is back)
    assert len(calls) == chunks.shape[0] >= (6 if clip else 51)
    assert _rows_of(got) == _rows_of(want) and got.uri == file["uri"]
    assert len(_rows_of(want)) >= 3 and len(set(want.labels())) >= 2


def test_apply_batch_equals_apply_per_file(gpu_device, powerset_model, waves):
    import pyannote_audio_amd as pa
    pipeline = pa.OnlineVoiceActivityDetection(segmentation=powerset_model, latency=1.0).to(gpu_device)
    pipeline.instantiate({"min_duration_on": 0.05, "min_duration_off": 0.1})
    files = [{"waveform": waves[s].view(1, -1), "sample_rate": 16000, "uri": f"file{i}"}
             for i, s in enumerate((7.3, 3.1, 12.0, 6.0))]
    batch = pipeline.apply_batch(files, num_slots=2)
    single = [pipeline.apply(f) for f in files]
    assert [a.uri for a in batch] == ["file0", "file1", "file2", "file3"]
    for a, b in zip(batch, single):
        assert _rows_of(a) == _rows_of(b)
    assert sum(len(_rows_of(a)) for a in batch) >= 3
    assert [(f["uri"], _rows_of(a)) for f, a in pipeline(files, num_slots=2)] == [(a.uri, _rows_of(a)) for a in batch]


def test_the_pipeline_is_resolved_from_a_config(tmp_path, synthetic_models, gpu_device):
    import yaml
    import pyannote_audio_amd as pa
    from conftest import write_pipeline_dir
    write_pipeline_dir(tmp_path, *synthetic_models, config_extra={
        "pipeline": {"name": "pyannote.audio.pipelines.OnlineVoiceActivityDetection",
                     "params": {"segmentation": "$model/segmentation", "step": 1.0, "latency": 2.0}},
        "params": {"min_duration_on": 0.0, "min_duration_off": 0.1}})
    with open(tmp_path / "config.yaml") as fp:
        assert yaml.safe_load(fp)["pipeline"]["name"].endswith("OnlineVoiceActivityDetection")
    pipeline = pa.Pipeline.from_pretrained(str(tmp_path))
    assert isinstance(pipeline, pa.OnlineVoiceActivityDetection) and pipeline.min_duration_off == 0.1
    bank = pipeline.to(gpu_device).bank(2)
    assert (bank.step, bank.latency, bank.duration, bank.num_slots) == (1.0, 2.0, 10.0, 2)
