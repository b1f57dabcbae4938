"""Online (streaming) voice activity and multi-label detection of many concurrent streams (csrc/online_detect.hip,
include/pyannote_amd_online.h).

A `DetectionBank` holds N stream slots.  Every `push` takes one step of audio for some of them; the slots that now hold
a full window go through ONE segmentation forward and ONE `detect_step` launch, and their next values, states and final
regions come back in ONE download.  No embedding network runs.  The overlap-add ring, the hysteresis state and the one
region per class that is not final yet stay on the device between pushes.

The arithmetic is that of the offline detection path carried across pushes (`frames.aggregate_files`,
`frames.binarize_regions`): at full latency (`latency = duration`, the default) and GIVEN THE SAME CHUNK SCORES a
stream's regions are bit for bit those of `VoiceActivityDetection` / `MultiLabelSegmentation` with the same chunk
step.  The chunk scores are the same for a recording of one chunk.  From two overlapping chunks on, the offline forward
shares ONE sinc layer over the file's span (`sincnet_plan_span`) where a stream forwards single windows, and the two
agree to rounding only (float32 scores within 1.2e-4 measured): the hard decisions of a powerset model absorb that on
every clip tried, though nothing guarantees it; a float32 score of a multi-label model that lies that close to its
threshold can fall on the other side, which moves a region boundary.  The host
arithmetic of push / close (chunk grid, tail padding, frame totals) is `online.StreamBank`'s.  There is no host
implementation behind these calls."""
from __future__ import annotations

from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ffi
from .core import Annotation, SlidingWindow
from .online import _architecture, _host_table, _Stream, emit_bound, start_frame, stream_num_frames
from .pipeline import Pipeline, Uniform


def _lib():
    return ffi.load()


def detect_limits() -> Tuple[int, int]:
    """(most classes, most values E * K of one emission) `detect_step` handles"""
    k, v = ffi.C.c_int(0), ffi.C.c_int(0)
    _lib().pao_detect_limits(ffi.C.byref(k), ffi.C.byref(v))
    return k.value, v.value


class DetectionState:
    """the state of a bank of N slots on the device (the header lists it); zeros are fresh streams"""
    FIELDS = (("acc", torch.float32, "RK"), ("cnt", torch.float32, "RK"), ("msk", torch.uint8, "RK"),
              ("on", torch.uint8, "K"), ("open_start", torch.float64, "K"), ("pend", torch.float64, "K2"),
              ("has_pend", torch.uint8, "K"), ("n_merged", torch.int32, "K"))

    def __init__(self, N: int, R: int, K: int, device):
        self.N, self.R, self.K = int(N), int(R), int(K)
        shapes = {"RK": (N, R, K), "K": (N, K), "K2": (N, K, 2)}
        for name, dtype, shape in self.FIELDS:
            setattr(self, name, torch.zeros(shapes[shape], dtype=dtype, device=device))

    def tensors(self) -> List[torch.Tensor]:
        return [getattr(self, name) for name, _, _ in self.FIELDS]

    def reset(self, slot: int):
        for t in self.tensors():
            t[slot].zero_()


class DetectOutputs(NamedTuple):
    """what one `detect_step` wrote: views of ONE byte buffer (`buffer`), so that one copy brings all of it down"""
    buffer: torch.Tensor       # uint8
    values: torch.Tensor       # (M, E, K) float32
    active: torch.Tensor       # (M, E, K) uint8
    counts: torch.Tensor       # (M, K) int32
    regions: torch.Tensor      # (M, K, cap, 2) float64
    tracks: torch.Tensor       # (M, K, cap) int32


def _carve(buffer, M: int, E: int, K: int, cap: int):
    """the five outputs inside a byte buffer (a device tensor or a host array), each at an 8-byte-aligned offset"""
    parts, at = [], 0
    for shape, itemsize in (((M, K, cap, 2), 8), ((M, E, K), 4), ((M, K), 4), ((M, K, cap), 4), ((M, E, K), 1)):
        n = int(np.prod(shape)) * itemsize
        parts.append((at, n, shape))
        at += (n + 7) & ~7
    if buffer is None:
        return at
    torch_types, numpy_types = (torch.float64, torch.float32, torch.int32, torch.int32, torch.uint8), \
        (np.float64, np.float32, np.int32, np.int32, np.uint8)
    views = []
    for (a, n, shape), tt, nt in zip(parts, torch_types, numpy_types):
        piece = buffer[a:a + n]
        views.append(piece.view(tt).view(shape) if isinstance(buffer, torch.Tensor) else piece.view(nt).reshape(shape))
    regions, values, counts, tracks, active = views
    return values, active, counts, regions, tracks


def step_table(slots: np.ndarray, frame_rows: np.ndarray) -> torch.Tensor:
    """the tables of one step as ONE host byte tensor, so that one upload carries them and nothing is cast on the
    device: the (4, M) int64 rows start_frame, emit_from, emit_to, closing, then the M int32 slots"""
    rows = np.ascontiguousarray(frame_rows, dtype=np.int64).reshape(-1)
    return torch.from_numpy(np.concatenate([rows.view(np.uint8), np.ascontiguousarray(slots, dtype=np.int32).view(np.uint8)]))


@ffi.on_device(lambda slots, scores, *a, **k: scores.device)
def detect_step(slots: Sequence[int], scores: torch.Tensor, window: torch.Tensor, warm: torch.Tensor, start_frame,
                emit_from, emit_to, closing, state: DetectionState, frames: SlidingWindow, onset, offset,
                min_duration_on=0.0, min_duration_off=0.0, *, E: int, any: bool = False, epsilon: float = 1e-12,
                missing: float = 0.0, cap: Optional[int] = None, table_device: Optional[torch.Tensor] = None
                ) -> DetectOutputs:
    """One detection step of the streams `slots` (host integers, distinct) of a bank, in one launch
    (`pao_detect_step`; the header states the rule).  scores (M, F, S) float32, or the uint8 hard decisions with `any`;
    window / warm (F) float64 on the device; start_frame / emit_from / emit_to / closing: host integers per stream
    (start_frame < 0: a flush; closing: the stream's last call); `state` is updated in place; `frames`: the frame
    grid; onset / offset / min_duration_on / min_duration_off: per class (K = 1 with `any`, else S), scalars are
    shared.  -> `DetectOutputs` on the device: values and states of up to E frames per stream and the regions the call
    made final, at most `cap` (default E // 2 + 2, the most there can be) per class.  `table_device`: `step_table` of
    the slots and the four frame rows on the device, when the caller uploaded it already."""
    slots = _host_table(slots, np.int32, "detect_step: slots")
    if scores.dim() != 3 or scores.dtype not in (torch.float32, torch.uint8):
        raise ValueError("detect_step: scores (streams, frames, classes) float32 or uint8")
    M, F, S = scores.shape
    K = 1 if any else S
    E = int(E)
    cap = E // 2 + 2 if cap is None else int(cap)
    frame_rows = np.stack([_host_table(start_frame, np.int64, "detect_step: start_frame"),
                           _host_table(emit_from, np.int64, "detect_step: emit_from"),
                           _host_table(emit_to, np.int64, "detect_step: emit_to"),
                           _host_table(np.asarray(closing).astype(np.int64), np.int64, "detect_step: closing")]) \
        if M else np.zeros((4, 0), np.int64)
    if slots.size != M or frame_rows.shape != (4, M):
        raise ValueError("detect_step: one slot and one entry of every frame table per stream")
    if tuple(window.shape) != (F,) or tuple(warm.shape) != (F,) or window.dtype != torch.float64 \
            or warm.dtype != torch.float64:
        raise ValueError("detect_step: window and warm are (frames,) float64 device tensors")
    if state.K != K:
        raise ValueError(f"detect_step: the state holds {state.K} classes per stream, the scores give {K}")

    def per_class(v, dtype):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (K,)))

    on, off = per_class(onset, np.float32), per_class(offset, np.float32)
    d_on, d_off = per_class(min_duration_on, np.float64), per_class(min_duration_off, np.float64)
    dev = scores.device
    x = scores.contiguous()
    if table_device is None:
        table_device = step_table(slots, frame_rows).to(dev)
    rows_device = table_device[:32 * M].view(torch.int64).view(4, M)
    slots_device = table_device[32 * M:].view(torch.int32)
    buffer = torch.empty(max(_carve(None, M, E, K, cap), 8), dtype=torch.uint8, device=dev)
    values, active, counts, regions, tracks = _carve(buffer, M, E, K, cap)
    ffi.check(_lib().pao_detect_step(
        ffi.ptr(slots_device), slots.ctypes.data, M, state.N, ffi.ptr(x), int(x.dtype == torch.uint8), F, S,
        int(bool(any)), ffi.ptr(window), ffi.ptr(warm), float(epsilon), float(missing), ffi.ptr(rows_device[0]),
        ffi.ptr(rows_device[1]), ffi.ptr(rows_device[2]), ffi.ptr(rows_device[3]), frame_rows.ctypes.data,
        float(frames.start), float(frames.duration), float(frames.step), on.ctypes.data, off.ctypes.data,
        d_on.ctypes.data, d_off.ctypes.data, state.R, E, cap, *(ffi.ptr(t) for t in state.tensors()),
        ffi.ptr(values), ffi.ptr(active), ffi.ptr(counts), ffi.ptr(regions), ffi.ptr(tracks), ffi.stream()),
        "pao_detect_step")
    return DetectOutputs(buffer, values, active, counts, regions, tracks)


class _DetectStream(_Stream):
    """host record of one slot: `_Stream` and what the stream has made final so far"""
    __slots__ = ("values", "active", "final", "positions")

    def __init__(self, K: int):
        super().__init__()
        self.values: List[np.ndarray] = []
        self.active: List[np.ndarray] = []
        self.final: List[List[np.ndarray]] = [[] for _ in range(K)]
        self.positions: List[List[np.ndarray]] = [[] for _ in range(K)]


Emission = Tuple[int, np.ndarray, np.ndarray, List[np.ndarray]]


class DetectionBank:
    """N concurrent streams whose speech (or event) regions are detected while their audio arrives.

    segmentation: a `Model` (or what `get_model` loads): a powerset PyanNet, detected as "somebody speaks" (`any`, the
    maximum over the speakers of the hard multilabel output, what `VoiceActivityDetection` aggregates), or a
    multi-label PyanNet with `any=False`, one detector per class on its float32 scores (`MultiLabelSegmentation`).
    Anything else raises NotImplementedError.  The chunk duration is the model's; `step` seconds of audio arrive per
    push; values for a frame leave `latency` seconds (a multiple of `step` in [step, duration], default duration)
    after its audio arrived.  onset / offset / min_duration_on / min_duration_off: per class or shared, `Binarize`'s
    (offset None: onset).  `warm_up`: seconds on either side of a chunk that count epsilon, as `Inference` has them.

    open() -> slot; push(blocks, slots) -> {slot: (first_frame, values (n, K) float32, active (n, K) uint8,
    [K arrays (r, 2) float64 of the regions this push made final])}; close(slot, tail) -> the same tuple for what the
    call emitted; regions(slot), annotation(slot, uri).

    A region is final -- nothing later can change it -- once it can no longer merge with a later one: at once
    without min_duration_off, else when the stream goes active again at least min_duration_off behind it, or at
    close.  At full latency and given the same chunk scores the final regions of a closed stream are the offline
    pipeline's, bit for bit (the module docstring says when the scores are the same).

    A live stream may run for days: the bank keeps a stream's FINAL REGIONS (what `regions` and `annotation` return)
    until its slot is opened again, and its per-frame values and states only with `keep_frames=True` (`values(slot)`,
    `active(slot)`; about 60 frames per second and class) -- `push` returns every emission anyway."""

    def __init__(self, segmentation, num_slots: int, *, step: float = 0.5, latency: Optional[float] = None,
                 any: bool = True, onset=0.5, offset=None, min_duration_on=0.0, min_duration_off=0.0,
                 warm_up: Tuple[float, float] = (0.0, 0.0), keep_frames: bool = False, device: torch.device = None):
        from .speaker_verification import get_model
        self.keep_frames = bool(keep_frames)
        model = get_model(segmentation)
        specifications = model.specifications
        powerset = bool(specifications.powerset)
        if _architecture(model) != "PyanNet" or powerset != bool(any) \
                or (not powerset and getattr(specifications, "permutation_invariant", False)):
            raise NotImplementedError(
                "DetectionBank runs a powerset PyanNet with any=True or a multi-label PyanNet (classes with an "
                f"identity) with any=False (got {_architecture(model)}, powerset = {powerset}, any = {bool(any)})")
        if device is None:
            raise ValueError("DetectionBank: `device` is required (a gfx950 device: there is no CPU fallback)")
        self.device = torch.device(device)
        self.model = model.to(self.device)
        self.num_slots = int(num_slots)
        if self.num_slots < 1:
            raise ValueError("DetectionBank: at least one slot")
        self.sample_rate = int(model.audio.sample_rate)
        self.duration = float(specifications.duration)
        self.step = float(step)
        self.window = int(model.audio.get_num_samples(self.duration))
        self.step_samples = int(round(self.step * self.sample_rate))
        if self.step_samples < 1 or self.window % self.step_samples:
            raise ValueError(f"DetectionBank: a chunk of {self.duration:g} s is not a whole number of {self.step:g}-s "
                             "steps")
        self.steps_per_window = self.window // self.step_samples
        self.latency = self.duration if latency is None else float(latency)
        multiple = round(self.latency / self.step)
        if abs(multiple * self.step - self.latency) > 1e-9 or not 1 <= multiple <= self.steps_per_window:
            raise ValueError(f"DetectionBank: latency {self.latency:g} s is not a multiple of the step {self.step:g} s "
                             f"in [{self.step:g}, {self.duration:g}]")
        self.frames: SlidingWindow = model.receptive_field
        #: the grid the times of the regions are taken on (streams start at 0)
        self.grid = SlidingWindow(start=0.0, duration=self.frames.duration, step=self.frames.step)
        self.F = int(model.num_frames(self.window))
        self.S = len(specifications.classes)
        self.any, self.hard = bool(any), powerset
        self.K = 1 if self.any else self.S
        self.classes = ["SPEECH"] if self.any else list(specifications.classes)
        if not 1 <= self.S <= detect_limits()[0]:
            raise NotImplementedError(f"DetectionBank: {self.S} classes, the step handles 1..{detect_limits()[0]}")

        def per_class(v, dtype):
            return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (self.K,)))

        self.onset = per_class(onset, np.float64)
        self.offset = self.onset.copy() if offset is None else per_class(offset, np.float64)
        self.min_duration_on = per_class(min_duration_on, np.float64)
        self.min_duration_off = per_class(min_duration_off, np.float64)
        self.epsilon, self.missing = 1e-12, 0.0                      # `Inference.slide`'s aggregation
        #: ring length: the frames of a chunk and the longest emission both fit (`StreamBank.R`)
        self.R = 2 * self.F + 16
        window = np.hamming(self.F)
        warm = np.ones(self.F)
        warm[:round(warm_up[0] / self.duration * self.F)] = self.epsilon
        warm[self.F - round(warm_up[1] / self.duration * self.F):] = self.epsilon
        weights = torch.from_numpy(np.stack([window, warm])).to(self.device)
        self._window, self._warm = weights[0], weights[1]
        self._streams = [_DetectStream(self.K) for _ in range(self.num_slots)]
        #: called with the name of every stage of a step once it is queued (tools/time_online_detection.py)
        self.stage_hook = None
        self.buffer = torch.zeros((self.num_slots, self.window), dtype=torch.float32, device=self.device)
        self.state = DetectionState(self.num_slots, self.R, self.K, self.device)

    # ---------------------------------------------------------------------------------------------------------- state
    def open(self) -> int:
        """the free slot of lowest index, its state zeroed"""
        for slot, stream in enumerate(self._streams):
            if not stream.open:
                self._streams[slot] = stream = _DetectStream(self.K)
                stream.open = True
                self.buffer[slot].zero_()
                self.state.reset(slot)
                return slot
        raise RuntimeError(f"DetectionBank: all {self.num_slots} slots are open")

    def _stream(self, slot: int) -> _DetectStream:
        if not 0 <= int(slot) < self.num_slots or not self._streams[int(slot)].open:
            raise ValueError(f"DetectionBank: slot {slot} is not open")
        return self._streams[int(slot)]

    # ---------------------------------------------------------------------------------------------------- device step
    def _advance(self, slots: np.ndarray, start: np.ndarray, emit_from: np.ndarray, emit_to: np.ndarray,
                 closing: np.ndarray, flush: bool = False):
        """the device side of one step for the ready `slots`: segmentation, `detect_step`, ONE download -> the five
        outputs on the host.  `flush`: only the emission (no chunk is added)."""
        ffi.require_gpu()
        M = len(slots)
        E = max(1, int((emit_to - emit_from).max()))
        cap = E // 2 + 2
        stage = self.stage_hook or (lambda name: None)
        with torch.cuda.device(self.device):
            table = step_table(slots, np.stack([start, emit_from, emit_to, closing.astype(np.int64)])).to(self.device)
            if flush:
                scores = torch.zeros((M, self.F, self.S), dtype=torch.uint8 if self.hard else torch.float32,
                                     device=self.device)
            else:
                flat = self.buffer.index_select(0, table[32 * M:].view(torch.int32)).view(-1)
                stage("windows")
                logp, multilabel = self.model.engine.forward_strided(flat, self.window, M, self.window,
                                                                     want_logp=not self.hard, want_multilabel=self.hard)
                scores = multilabel if self.hard else logp
                stage("segmentation")
            out = detect_step(slots, scores, self._window, self._warm, start, emit_from, emit_to, closing, self.state,
                              self.grid, self.onset, self.offset, self.min_duration_on, self.min_duration_off, E=E,
                              any=self.any, epsilon=self.epsilon, missing=self.missing, cap=cap, table_device=table)
            stage("detect_step")
            host = out.buffer.cpu().numpy()
            stage("download")
        return _carve(host, M, E, self.K, cap)

    def _collect(self, ready, outputs, emit_from, emit_to, chunk: bool) -> Dict[int, Emission]:
        values, active, counts, regions, tracks = outputs
        result = {}
        for i, slot in enumerate(ready):
            stream = self._streams[slot]
            n = int(emit_to[i] - emit_from[i])
            v, a = np.ascontiguousarray(values[i, :n]), np.ascontiguousarray(active[i, :n])
            final = [np.ascontiguousarray(regions[i, k, :counts[i, k]]) for k in range(self.K)]
            if self.keep_frames:
                stream.values.append(v)
                stream.active.append(a)
            for k in range(self.K):
                stream.final[k].append(final[k])
                stream.positions[k].append(np.ascontiguousarray(tracks[i, k, :counts[i, k]]))
            stream.emitted = int(emit_to[i])
            stream.chunks += int(chunk)
            result[slot] = (int(emit_from[i]), v, a, final)
        return result

    # ------------------------------------------------------------------------------------------------------ streaming
    def _append(self, blocks: torch.Tensor, slots: Sequence[int]):
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64)).to(self.device)
        rows = self.buffer.index_select(0, idx)
        self.buffer.index_copy_(0, idx, torch.cat([rows[:, self.step_samples:], blocks], dim=1))

    def _run(self, ready: List[int], limit: Optional[Dict[int, int]] = None) -> Dict[int, Emission]:
        """one step of the `ready` slots (their window is in the buffer): `StreamBank._run`'s frame arithmetic"""
        if not ready:
            return {}
        slots = np.asarray(ready, dtype=np.int32)
        start = np.empty(len(ready), dtype=np.int64)
        emit_from = np.empty(len(ready), dtype=np.int64)
        emit_to = np.empty(len(ready), dtype=np.int64)
        for i, slot in enumerate(ready):
            stream = self._streams[slot]
            c = stream.chunks
            start[i] = start_frame(c, self.step, self.frames)
            bound = min(emit_bound(c, self.step, self.duration, self.latency, self.frames), start[i] + self.F)
            if limit is not None and slot in limit:
                bound = min(bound, limit[slot])
            emit_from[i] = stream.emitted
            emit_to[i] = max(bound, stream.emitted)
        out = self._advance(slots, start, emit_from, emit_to, np.zeros(len(ready), dtype=np.int64))
        return self._collect(ready, out, emit_from, emit_to, chunk=True)

    def push(self, blocks, slots: Sequence[int]) -> Dict[int, Emission]:
        """One step of audio for each listed slot: blocks (M, step_samples) float32, on the host or the device.  The
        slots that now hold a full window run one step together -- one segmentation forward, one `detect_step`, one
        download -> {slot: (first_frame, values, active, final regions per class)} for those."""
        slots = [int(s) for s in slots]
        if len(set(slots)) != len(slots):
            raise ValueError("DetectionBank.push: a slot is listed twice")
        streams = [self._stream(s) for s in slots]
        blocks = torch.as_tensor(blocks)
        if tuple(blocks.shape) != (len(slots), self.step_samples) or blocks.dtype != torch.float32:
            raise ValueError(f"DetectionBank.push: blocks must be ({len(slots)}, {self.step_samples}) float32")
        if not slots:
            return {}
        self._append(blocks.to(self.device), slots)
        ready = []
        for slot, stream in zip(slots, streams):
            stream.blocks += 1
            if stream.blocks >= self.steps_per_window:
                ready.append(slot)
        return self._run(ready)

    def close(self, slot: int, tail=None) -> Emission:
        """End of a stream, as `StreamBank.close` ends one: a partial block (`tail`, fewer samples than one step) is
        zero-padded to one step and run, a stream shorter than one chunk gets one zero-padded chunk; then a closing
        flush emits every frame up to the stream's last one (the frames offline inference gives a file of that many
        samples), closes the region still open and makes the pending regions final, and the slot is freed.
        -> (first_frame, values, active, final regions per class) of what this call emitted; `regions(slot)` and
        `annotation(slot)` stay valid until the slot is opened again."""
        stream = self._stream(slot)
        slot = int(slot)
        tail = None if tail is None else torch.as_tensor(tail).reshape(-1)
        n_tail = 0 if tail is None else int(tail.numel())
        if n_tail >= self.step_samples:
            raise ValueError("DetectionBank.close: the tail is shorter than one step; push whole steps")
        num_samples = stream.blocks * self.step_samples + n_tail
        total = stream_num_frames(num_samples, self.window, self.step_samples, self.sample_rate, self.duration,
                                  self.step, self.frames)
        first, parts = stream.emitted, []
        if n_tail:
            block = torch.zeros(self.step_samples, dtype=torch.float32, device=self.device)
            block[:n_tail] = tail.to(self.device, torch.float32)
            self._append(block[None], [slot])
            stream.blocks += 1
        if num_samples > 0 and stream.blocks < self.steps_per_window:
            # shorter than one chunk: the samples lie at the end of the buffer, chunk 0 has them at its start
            have = stream.blocks * self.step_samples
            self.buffer[slot] = torch.roll(self.buffer[slot], shifts=have - self.window)
            stream.blocks = self.steps_per_window
            parts.append(self._run([slot], {slot: total})[slot])
        elif n_tail:
            parts.append(self._run([slot], {slot: total})[slot])
        if num_samples > 0:
            frm = np.array([stream.emitted], dtype=np.int64)
            to = np.array([max(total, stream.emitted)], dtype=np.int64)
            out = self._advance(np.array([slot], dtype=np.int32), np.array([-1], dtype=np.int64), frm, to,
                                np.ones(1, dtype=np.int64), flush=True)
            parts.append(self._collect([slot], out, frm, to, chunk=False)[slot])
        stream.open = False
        if not parts:
            return first, np.zeros((0, self.K), np.float32), np.zeros((0, self.K), np.uint8), \
                [np.zeros((0, 2)) for _ in range(self.K)]
        return first, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), \
            [np.concatenate([p[3][k] for p in parts]) for k in range(self.K)]

    # -------------------------------------------------------------------------------------------------------- results
    def values(self, slot: int) -> np.ndarray:
        """every value emitted so far for the slot's stream, (frames, K) float32 from frame 0"""
        rows = self._streams[int(slot)].values
        return np.concatenate(rows) if rows else np.zeros((0, self.K), dtype=np.float32)

    def active(self, slot: int) -> np.ndarray:
        """the hysteresis state behind every emitted frame, (frames, K) uint8 from frame 0"""
        rows = self._streams[int(slot)].active
        return np.concatenate(rows) if rows else np.zeros((0, self.K), dtype=np.uint8)

    def regions(self, slot: int, return_tracks: bool = False):
        """the regions of the slot's stream that are final so far: K float64 arrays (n_k, 2) in time order; with
        `return_tracks` also K int arrays, the position of every region in the class's track-name sequence"""
        stream = self._streams[int(slot)]
        regions = [np.concatenate(r) if r else np.zeros((0, 2)) for r in stream.final]
        if not return_tracks:
            return regions
        return regions, [np.concatenate(p) if p else np.zeros(0, np.int32) for p in stream.positions]

    def annotation(self, slot: int, uri: Optional[str] = None) -> Annotation:
        """the final regions as the packed detection path builds its Annotation: labels are the class names ("SPEECH"
        with `any`), tracks the generated names by position"""
        from .multilabel import regions_to_annotation
        regions, positions = self.regions(slot, return_tracks=True)
        return regions_to_annotation(regions, positions, self.classes, uri)


class OnlineVoiceActivityDetection(Pipeline):
    """`VoiceActivityDetection` on audio that arrives `step` seconds at a time: every file is streamed through a
    `DetectionBank` and its speech regions are those the bank made final.  `apply(file)` streams one file through a
    bank of one; `apply_batch(files, num_slots=None)` streams many concurrently (files of different lengths end at
    different steps, and waiting files take the freed slots).  A file's Annotation does not depend on the files it
    shared the bank with.  Hyper-parameters, defaults, `classes`, `get_metric` and `get_direction` are
    `VoiceActivityDetection`'s; at full latency (the default) and with offset <= onset so is the Annotation, for an
    offline pipeline whose chunk step is `step`.  At full latency `tuning.DetectionTuner` tunes the same thresholds."""

    def __init__(self, segmentation=None, step: float = 0.5, latency: Optional[float] = None, fscore: bool = False,
                 token=None, cache_dir=None):
        super().__init__()
        if segmentation is None:
            raise ValueError("`segmentation` must be a local checkpoint (or a Model instance): Hugging Face "
                             "defaults cannot be downloaded in this build.")
        from .speaker_verification import get_model
        self.segmentation = segmentation
        self.fscore = fscore
        self.segmentation_model = get_model(segmentation, token=token, cache_dir=cache_dir)
        self.bank_options = dict(step=step, latency=latency)
        if self.segmentation_model.specifications.powerset:
            self.onset = self.offset = 0.5
        else:
            self.onset = Uniform(0.0, 1.0)
            self.offset = Uniform(0.0, 1.0)
        self.min_duration_on = Uniform(0.0, 1.0)
        self.min_duration_off = Uniform(0.0, 1.0)

    def default_parameters(self):
        if self.segmentation_model.specifications.powerset:
            return {"min_duration_on": 0.0, "min_duration_off": 0.0}
        raise NotImplementedError()

    def classes(self):
        return ["SPEECH"]

    def get_metric(self):
        from . import annotation_metrics
        device = getattr(self, "device", None)
        device = device if device is not None and device.type == "cuda" else None
        if self.fscore:
            return annotation_metrics.DetectionPrecisionRecallFMeasure(collar=0.0, skip_overlap=False, device=device)
        return annotation_metrics.DetectionErrorRate(collar=0.0, skip_overlap=False, device=device)

    def get_direction(self) -> str:
        return "maximize" if self.fscore else "minimize"

    def bank(self, num_slots: int) -> DetectionBank:
        ffi.require_gpu()
        device = getattr(self, "device", None)
        if device is None or getattr(device, "type", None) != "cuda":
            raise RuntimeError("OnlineVoiceActivityDetection must be moved to the GPU first: "
                               "pipeline.to(torch.device('cuda')) -- there is no CPU fallback")
        return DetectionBank(self.segmentation_model, num_slots, any=True, onset=self.onset,
                             offset=self.offset or self.onset, min_duration_on=self.min_duration_on,
                             min_duration_off=self.min_duration_off,
                             warm_up=self.segmentation_model.specifications.warm_up, device=device,
                             **self.bank_options)

    def apply(self, file, **kwargs) -> Annotation:
        return self.apply_batch([file], num_slots=1)[0]

    def _apply_batch(self, files: list, **kwargs):
        return zip(files, self.apply_batch(files, **kwargs))

    def apply_batch(self, files: Iterable, num_slots: Optional[int] = None) -> List[Annotation]:
        """the streaming loop of `OnlineSpeakerDiarization.apply_batch`"""
        from .audio import Audio
        files = [Audio.validate_file(f) for f in files]
        if not files:
            return []
        bank = self.bank(min(len(files), 64) if num_slots is None else int(num_slots))
        audio = Audio(sample_rate=bank.sample_rate, mono="downmix")
        step = bank.step_samples
        results: List[Optional[Annotation]] = [None] * len(files)
        waiting = list(range(len(files)))
        live: Dict[int, list] = {}          # slot -> [file index, waveform on the device, samples consumed]
        while waiting or live:
            while waiting and len(live) < bank.num_slots:
                index = waiting.pop(0)
                waveform, _ = audio(files[index])
                live[bank.open()] = [index, waveform.reshape(-1).to(bank.device, torch.float32), 0]
            pushing = [s for s, (_, wav, at) in live.items() if wav.numel() - at >= step]
            for slot in [s for s in live if s not in pushing]:
                index, wav, at = live.pop(slot)
                bank.close(slot, wav[at:] if wav.numel() > at else None)
                results[index] = bank.annotation(slot, uri=files[index]["uri"])
            if pushing:
                bank.push(torch.stack([live[s][1][live[s][2]:live[s][2] + step] for s in pushing]), pushing)
                for s in pushing:
                    live[s][2] += step
        return results
