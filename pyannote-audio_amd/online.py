"""Online (streaming) speaker diarization of many concurrent streams (csrc/online.hip, include/pyannote_amd_online.h).

A `StreamBank` holds N stream slots.  Every `push` takes one step of audio for some of them; the slots that now hold a
full window go through ONE segmentation forward, ONE embedding forward, one incremental clustering launch
(`cluster_step`) and one rolling overlap-add launch (`emit`), and the next decisions of all of them come back in one
download.  Centroids and the overlap-add ring stay on the device between pushes.

The clustering is the incremental rule of Coria et al., "Overlap-aware low-latency online speaker diarization based on
end-to-end local segmentation" (ASRU 2021), stated in full in the header; it is not part of the reference library and
is held to a numpy model of its own definition (tests/online_model.py).  There is no host implementation behind these
calls.

A recorded file does not have to arrive slowly: `StreamBank.front_end` runs the two networks over all its chunks at
once, and `StreamBank.replay` (`replay_jobs`, `pao_replay`, csrc/online_replay.hip) walks the chunks through the same
rule on the device, one workgroup per (file, threshold triple) -- the route of `apply(file, replay=True)` and of
`tuning.OnlineTuner`."""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ffi
from .core import Annotation, Segment, SlidingWindow, SlidingWindowFeature
from .pipeline import Pipeline


def _lib():
    return ffi.load()


def cluster_step_limits() -> Tuple[int, int]:
    """(most local speakers per chunk, most global speakers per stream) `cluster_step` handles"""
    s, k = ffi.C.c_int(0), ffi.C.c_int(0)
    _lib().pao_cluster_step_limits(ffi.C.byref(s), ffi.C.byref(k))
    return s.value, k.value


def _host_table(values, dtype, what) -> np.ndarray:
    a = np.ascontiguousarray(values, dtype=dtype).reshape(-1)
    if a.size and not np.array_equal(a, np.asarray(values).reshape(-1)):
        raise ValueError(f"{what}: values do not fit {np.dtype(dtype).name}")
    return a


@ffi.on_device(lambda slots, emb, *a, **k: emb.device)
def cluster_step(slots: Sequence[int], emb: torch.Tensor, active: torch.Tensor, clean: torch.Tensor,
                 centroid_sum: torch.Tensor, centroid_n: torch.Tensor, min_active_frames: int,
                 min_update_frames: int, delta_new: float, slots_device: Optional[torch.Tensor] = None
                 ) -> torch.Tensor:
    """One incremental clustering step of the streams `slots` (host integers, distinct) of a bank, in one launch
    (`pao_cluster_step`).  emb (M, S, D) float32, active / clean (M, S) int32; centroid_sum (N, K, D) float64 and
    centroid_n (N, K) int32 are updated in place -> map (M, S) int32 in [-1, K), on the device.  `slots_device`: the
    slots as an int32 device tensor, when the caller uploaded them already."""
    slots = _host_table(slots, np.int32, "cluster_step: slots")
    M, S, D = emb.shape
    N, K, _ = centroid_sum.shape
    if not (emb.dtype == torch.float32 and active.dtype == torch.int32 and clean.dtype == torch.int32
            and centroid_sum.dtype == torch.float64 and centroid_n.dtype == torch.int32):
        raise ValueError("cluster_step: emb float32, active / clean / centroid_n int32, centroid_sum float64")
    if slots.size != M or tuple(active.shape) != (M, S) or tuple(clean.shape) != (M, S) \
            or tuple(centroid_n.shape) != (N, K) or centroid_sum.shape[2] != D:
        raise ValueError("cluster_step: one slot, one row of active and of clean per chunk; centroid_n (N, K) and "
                         "centroid_sum (N, K, D) of one bank")
    dev = emb.device
    if slots_device is None:
        slots_device = torch.from_numpy(slots).to(dev)
    out = torch.empty((M, S), dtype=torch.int32, device=dev)
    ffi.check(_lib().pao_cluster_step(
        ffi.ptr(slots_device), slots.ctypes.data, M, N, ffi.ptr(emb), ffi.ptr(active), ffi.ptr(clean), S, D, K,
        int(min_active_frames), int(min_update_frames), float(delta_new), ffi.ptr(centroid_sum), ffi.ptr(centroid_n),
        ffi.ptr(out), ffi.stream()), "pao_cluster_step")
    return out


@ffi.on_device(lambda slots, seg, *a, **k: seg.device)
def emit(slots: Sequence[int], seg: torch.Tensor, map: torch.Tensor, start_frame, emit_from, emit_to,
         acc_sum: torch.Tensor, acc_cnt: torch.Tensor, E: int, table_device: Optional[torch.Tensor] = None
         ) -> torch.Tensor:
    """Rolling overlap-add and emission of the streams `slots` of a bank, in one launch (`pao_emit`).  seg (M, F, S)
    uint8, map (M, S) int32; start_frame / emit_from / emit_to: host integers per stream (start_frame < 0: nothing is
    added, a flush); acc_sum (N, R, K) and acc_cnt (N, R) int32 are updated in place -> out (M, E, K) uint8 on the
    device, rows behind a stream's emit_to - emit_from zero.  `table_device`: (4, M) int64 device tensor of slots and
    the three frame rows, when the caller uploaded them already."""
    slots = _host_table(slots, np.int32, "emit: slots")
    M, F, S = seg.shape
    N, R, K = acc_sum.shape
    frames = np.stack([_host_table(start_frame, np.int64, "emit: start_frame"),
                       _host_table(emit_from, np.int64, "emit: emit_from"),
                       _host_table(emit_to, np.int64, "emit: emit_to")]) if M else np.zeros((3, 0), np.int64)
    if not (seg.dtype == torch.uint8 and map.dtype == torch.int32 and acc_sum.dtype == torch.int32
            and acc_cnt.dtype == torch.int32):
        raise ValueError("emit: seg uint8, map / acc_sum / acc_cnt int32")
    if slots.size != M or frames.shape != (3, M) or tuple(map.shape) != (M, S) or tuple(acc_cnt.shape) != (N, R):
        raise ValueError("emit: one slot, one map row and one entry of every frame table per chunk; acc_cnt (N, R) and "
                         "acc_sum (N, R, K) of one bank")
    dev = seg.device
    if table_device is None:
        table_device = torch.from_numpy(np.concatenate([slots.astype(np.int64)[None], frames])).to(dev)
    slots_device = table_device[0].to(torch.int32)
    out = torch.empty((M, int(E), K), dtype=torch.uint8, device=dev)
    ffi.check(_lib().pao_emit(
        ffi.ptr(slots_device), slots.ctypes.data, M, N, ffi.ptr(seg), F, S, ffi.ptr(map),
        ffi.ptr(table_device[1]), ffi.ptr(table_device[2]), ffi.ptr(table_device[3]), frames.ctypes.data, R, K, int(E),
        ffi.ptr(acc_sum), ffi.ptr(acc_cnt), ffi.ptr(out), ffi.stream()), "pao_emit")
    return out


@ffi.on_device(lambda emb, *a, **k: emb.device)
def replay_jobs(emb: torch.Tensor, active: torch.Tensor, clean: torch.Tensor, seg: torch.Tensor, files, sched, jobs,
                delta_new, offsets, centroid_sum: torch.Tensor, centroid_n: torch.Tensor, acc_sum: torch.Tensor,
                acc_cnt: torch.Tensor, map_rows: Optional[int] = None, out_rows: Optional[int] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Recorded files through the online rule, every job in ONE launch (`pao_replay`; the header has the tables).
    emb (chunks, S, D) float32, active / clean (chunks, S) int32, seg (chunks, F, S) uint8: the concatenated front
    ends; files (files, 4) and sched (rows, 3) int64, jobs (J, 3) int32, delta_new (J) float64, offsets (J, 2) int64:
    host tables; the state -- centroid_sum (J, K, D) float64, centroid_n (J, K), acc_sum (J, R, K), acc_cnt (J, R)
    int32, one row per job -- is updated in place -> (map (map_rows, S) int32, out (out_rows, K) uint8) on the device.
    `map_rows` / `out_rows` default to what the offsets reach; rows no job owns come back zero."""
    files = np.ascontiguousarray(files, dtype=np.int64).reshape(-1, 4)
    sched = np.ascontiguousarray(sched, dtype=np.int64).reshape(-1, 3)
    jobs = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, 3)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1, 2)
    delta_new = np.ascontiguousarray(delta_new, dtype=np.float64).reshape(-1)
    C, S, D = emb.shape
    F = seg.shape[1]
    J, K, _ = centroid_sum.shape
    R = acc_sum.shape[1]
    if not (emb.dtype == torch.float32 and active.dtype == torch.int32 and clean.dtype == torch.int32
            and seg.dtype == torch.uint8 and centroid_sum.dtype == torch.float64 and centroid_n.dtype == torch.int32
            and acc_sum.dtype == torch.int32 and acc_cnt.dtype == torch.int32):
        raise ValueError("replay_jobs: emb float32, seg uint8, centroid_sum float64, everything else int32")
    if tuple(active.shape) != (C, S) or tuple(clean.shape) != (C, S) or seg.shape[0] != C or seg.shape[2] != S \
            or len(jobs) != J or len(delta_new) != J or len(offsets) != J or centroid_sum.shape[2] != D \
            or tuple(centroid_n.shape) != (J, K) or tuple(acc_sum.shape) != (J, R, K) or tuple(acc_cnt.shape) != (J, R):
        raise ValueError("replay_jobs: one row of active, clean and seg per chunk; one row of the job table, of "
                         "delta_new, of the offsets and of every state tensor per job")
    dev = emb.device
    if map_rows is None or out_rows is None:
        inside = (jobs[:, 0] >= 0) & (jobs[:, 0] < len(files))
        rows = files[jobs[inside, 0]] if inside.any() else np.zeros((0, 4), np.int64)
        reach = offsets[inside] + rows[:, [1, 3]] if inside.any() else np.zeros((0, 2), np.int64)
        map_rows = int(reach[:, 0].max(initial=0)) if map_rows is None else map_rows
        out_rows = int(reach[:, 1].max(initial=0)) if out_rows is None else out_rows
    mp = torch.zeros((max(int(map_rows), 0), S), dtype=torch.int32, device=dev)
    out = torch.zeros((max(int(out_rows), 0), K), dtype=torch.uint8, device=dev)
    wide = torch.from_numpy(np.concatenate([files.reshape(-1), sched.reshape(-1), offsets.reshape(-1),
                                            delta_new.view(np.int64)])).to(dev)
    d_files, d_sched, d_offsets, d_delta = torch.split(wide, [files.size, sched.size, offsets.size, delta_new.size])
    d_jobs = torch.from_numpy(jobs.reshape(-1)).to(dev)
    ffi.check(_lib().pao_replay(
        ffi.ptr(emb), ffi.ptr(active), ffi.ptr(clean), ffi.ptr(seg), C, F, S, D, ffi.ptr(d_files), files.ctypes.data,
        len(files), ffi.ptr(d_sched), sched.ctypes.data, len(sched), ffi.ptr(d_jobs), jobs.ctypes.data,
        ffi.ptr(d_delta), ffi.ptr(d_offsets), offsets.ctypes.data, J, int(map_rows), int(out_rows), K, R,
        ffi.ptr(centroid_sum), ffi.ptr(centroid_n), ffi.ptr(acc_sum), ffi.ptr(acc_cnt), ffi.ptr(mp), ffi.ptr(out),
        ffi.stream()), "pao_replay")
    return mp, out


# ------------------------------------------------------------------------------------------------- frame arithmetic
def frame_of_time(t: float, frames: SlidingWindow) -> int:
    """the frame a chunk starting at time t starts on: `frames.frame_geometry`'s float64 formula for one value (chunks
    and frames start at 0; the half frame is added and taken off as there, roundings included)"""
    half = 0.5 * np.float64(frames.duration)
    return int(np.rint((((0.0 + np.float64(t)) + half) - 0.0 - half) / np.float64(frames.step)))


def start_frame(c: int, step: float, frames: SlidingWindow) -> int:
    """global frame of frame 0 of chunk c"""
    return frame_of_time(np.float64(c) * np.float64(step), frames)


def emit_bound(c: int, step: float, duration: float, latency: float, frames: SlidingWindow) -> int:
    """frames below this one are due once chunk c is in: the start frame of time c step + duration - latency + step"""
    return frame_of_time(np.float64(c) * np.float64(step) + duration - latency + step, frames)


def stream_num_frames(num_samples: int, window: int, step_samples: int, sample_rate: int, duration: float, step: float,
                      frames: SlidingWindow) -> int:
    """the frames offline inference gives a file of `num_samples` samples (`frames.files_layout` for one length)"""
    from .frames import frame_geometry
    from .inference import Inference
    if num_samples <= 0:
        return 0
    n, has_last = Inference.num_chunks(int(num_samples), window, step_samples)
    _, num_frames, out_frames = frame_geometry(SlidingWindow(start=0.0, duration=duration, step=step), frames,
                                               n + has_last)
    if has_last:
        (first, stop), = out_frames.crop(Segment(0.0, num_samples / sample_rate), mode="loose", return_ranges=True)
        num_frames = min(stop, num_frames) - max(first, 0)
    return max(int(num_frames), 0)


def file_schedule(num_samples: int, *, window: int, step_samples: int, sample_rate: int, duration: float, step: float,
                  latency: float, frames: SlidingWindow, F: int) -> Tuple[int, np.ndarray, int]:
    """What a recording of `num_samples` samples goes through when it is streamed, without a bank: -> (C chunks,
    schedule (C + 1, 3) int64 of (start_frame, emit_from, emit_to), total frames).  The host arithmetic of `push`,
    `_run` and `close`: chunks come from whole steps, the tail is zero-padded to one step, a file shorter than one chunk
    gets one zero-padded chunk, the `limit = total` clamp applies on a closing chunk only, and the flush row
    (start_frame = -1) comes last.  Chunk c is `padded[c * step_samples : c * step_samples + window]`."""
    num_samples = max(int(num_samples), 0)
    total = stream_num_frames(num_samples, window, step_samples, sample_rate, duration, step, frames)
    steps_per_window = window // step_samples
    blocks = num_samples // step_samples + (1 if num_samples % step_samples else 0)
    if num_samples == 0:
        C, closing = 0, -1
    elif blocks < steps_per_window:
        C, closing = 1, 0
    else:
        C = blocks - steps_per_window + 1
        closing = C - 1 if num_samples % step_samples else -1
    rows = np.empty((C + 1, 3), dtype=np.int64)
    emitted = 0
    for c in range(C):
        start = start_frame(c, step, frames)
        bound = min(emit_bound(c, step, duration, latency, frames), start + F)
        if c == closing:
            bound = min(bound, total)
        rows[c] = (start, emitted, max(bound, emitted))
        emitted = int(rows[c, 2])
    rows[C] = (-1, emitted, max(total, emitted))
    return C, rows, total


class FrontEnd:
    """everything of a recording the online rule reads, on the device: seg (C, F, S) uint8, active / clean (C, S)
    int32, emb (C, S, D) float32; its `schedule` (C + 1, 3) int64 on the host and its `total` frames"""
    __slots__ = ("seg", "active", "clean", "emb", "schedule", "total")

    def __init__(self, seg, active, clean, emb, schedule, total):
        self.seg, self.active, self.clean, self.emb, self.schedule, self.total = seg, active, clean, emb, schedule, total

    @property
    def num_chunks(self) -> int:
        return int(self.seg.shape[0])


class Replayed:
    """one replayed job: `decisions` (total, K) uint8, `maps` (C, S) int32, `centroids` (K, D) float64 -- what
    `decisions(slot)`, the maps of every step and `centroids(slot)` give after streaming"""
    __slots__ = ("decisions", "maps", "centroids")

    def __init__(self, decisions, maps, centroids):
        self.decisions, self.maps, self.centroids = decisions, maps, centroids


def _architecture(model) -> str:
    return str(getattr(type(model), "ARCHITECTURE", ("", type(model).__name__))[1])


class _Stream:
    """host record of one slot"""
    __slots__ = ("open", "blocks", "chunks", "emitted", "rows")

    def __init__(self):
        self.open = False
        self.blocks = 0        # steps of audio received
        self.chunks = 0        # chunks processed
        self.emitted = 0       # frames emitted
        self.rows: List[np.ndarray] = []


class StreamBank:
    """N concurrent streams diarized while their audio arrives.

    segmentation, embedding: `Model`s (or what `get_model` loads).  This version runs powerset PyanNet with WeSpeaker
    ResNet embeddings; anything else raises NotImplementedError.  The chunk duration is the segmentation model's;
    `step` seconds of audio arrive per push; decisions for a frame leave `latency` seconds (a multiple of `step` in
    [step, duration], default duration) after its audio arrived.  `max_speakers` <= 32 global speakers per stream.

    `delta_new` (a local speaker farther than this cosine distance from its centroid founds a new one), `min_active`
    and `min_update` (seconds a local speaker must be on / on alone to count / to move a centroid) are UNTUNED
    defaults: no trained checkpoint is available offline to tune them with.  `tuning.OnlineTuner` tunes the three
    on a corpus.

    open() -> slot; push(blocks, slots) -> {slot: (first_frame, decisions)}; close(slot, tail) -> (first_frame,
    decisions); annotation(slot); centroids(slot).

    A RECORDED file need not be streamed: `front_end(waveform)` computes what the rule reads for every chunk at
    once and `replay(front_ends, params)` walks the chunks on the device, every (file, threshold triple) a job of one
    launch (`pao_replay`) -- the decisions, maps and centroids streaming the file through a fresh slot gives."""

    #: bound on the bytes of the gathered windows of one front-end group
    front_end_bytes: int = 64 << 20
    #: bound on the bytes of the outputs and the state of one replay launch
    replay_bytes: int = 1 << 30

    def __init__(self, segmentation, embedding, num_slots: int, *, step: float = 0.5, latency: Optional[float] = None,
                 max_speakers: int = 20, delta_new: float = 1.0, min_active: float = 0.25, min_update: float = 1.0,
                 exclude_overlap: bool = True, device: torch.device = None):
        from .speaker_verification import get_model
        seg_model, emb_model = get_model(segmentation), get_model(embedding)
        if _architecture(seg_model) != "PyanNet" or not seg_model.specifications.powerset:
            raise NotImplementedError("StreamBank: the online step runs powerset PyanNet segmentation only (got "
                                      f"{_architecture(seg_model)}, powerset = {bool(seg_model.specifications.powerset)})")
        if not _architecture(emb_model).startswith("WeSpeakerResNet"):
            raise NotImplementedError("StreamBank: the online step runs WeSpeaker ResNet embeddings only (got "
                                      f"{_architecture(emb_model)})")
        if device is None:
            raise ValueError("StreamBank: `device` is required (a gfx950 device: there is no CPU fallback)")
        self.device = torch.device(device)
        self.seg_model, self.emb_model = seg_model.to(self.device), emb_model.to(self.device)
        self.num_slots = int(num_slots)
        if self.num_slots < 1:
            raise ValueError("StreamBank: at least one slot")
        self.sample_rate = int(seg_model.audio.sample_rate)
        if int(emb_model.audio.sample_rate) != self.sample_rate:
            raise ValueError("StreamBank: the two models take different sample rates")
        self.duration = float(seg_model.specifications.duration)
        self.step = float(step)
        self.window = int(seg_model.audio.get_num_samples(self.duration))
        self.step_samples = int(round(self.step * self.sample_rate))
        if self.step_samples < 1 or self.window % self.step_samples:
            raise ValueError(f"StreamBank: a chunk of {self.duration:g} s is not a whole number of {self.step:g}-s steps")
        self.steps_per_window = self.window // self.step_samples
        self.latency = self.duration if latency is None else float(latency)
        multiple = round(self.latency / self.step)
        if abs(multiple * self.step - self.latency) > 1e-9 or not 1 <= multiple <= self.steps_per_window:
            raise ValueError(f"StreamBank: latency {self.latency:g} s is not a multiple of the step {self.step:g} s in "
                             f"[{self.step:g}, {self.duration:g}]")
        self.frames: SlidingWindow = seg_model.receptive_field
        self.F = int(seg_model.num_frames(self.window))
        self.S = len(seg_model.specifications.classes)
        self.D = int(emb_model.dimension)
        self.K = int(max_speakers)
        self.delta_new = float(delta_new)
        self.min_active_frames = max(1, int(np.rint(min_active / self.frames.step)))
        self.min_update_frames = int(np.rint(min_update / self.frames.step))
        self.exclude_overlap = bool(exclude_overlap)
        #: ring length: the frames of a chunk and the longest emission (a whole chunk and the frames offline inference
        #: counts behind the last chunk) both fit
        self.R = 2 * self.F + 16
        self._streams = [_Stream() for _ in range(self.num_slots)]
        #: called with the name of every stage of a step once it is queued (tools/time_online.py records events)
        self.stage_hook = None
        self._allocate()

    # ------------------------------------------------------------------------------------------------------ state
    def _allocate(self):
        N, dev = self.num_slots, self.device
        self.buffer = torch.zeros((N, self.window), dtype=torch.float32, device=dev)
        self.centroid_sum = torch.zeros((N, self.K, self.D), dtype=torch.float64, device=dev)
        self.centroid_n = torch.zeros((N, self.K), dtype=torch.int32, device=dev)
        self.acc_sum = torch.zeros((N, self.R, self.K), dtype=torch.int32, device=dev)
        self.acc_cnt = torch.zeros((N, self.R), dtype=torch.int32, device=dev)

    def open(self) -> int:
        """the free slot of lowest index, its state zeroed"""
        for slot, stream in enumerate(self._streams):
            if not stream.open:
                self._streams[slot] = stream = _Stream()
                stream.open = True
                for t in (self.buffer, self.centroid_sum, self.centroid_n, self.acc_sum, self.acc_cnt):
                    t[slot].zero_()
                return slot
        raise RuntimeError(f"StreamBank: all {self.num_slots} slots are open")

    def _stream(self, slot: int) -> _Stream:
        if not 0 <= int(slot) < self.num_slots or not self._streams[int(slot)].open:
            raise ValueError(f"StreamBank: slot {slot} is not open")
        return self._streams[int(slot)]

    # ------------------------------------------------------------------------------------------------ device step
    def _min_num_frames(self) -> int:
        """speaker_diarization.py:375-382: shortest clean mask that still yields an embedding"""
        if not self.exclude_overlap:
            return -1
        from .speaker_verification import first_true
        frames = ffi.load().pa_emb_num_fbank_frames
        if not hasattr(self, "_min_num_samples"):
            self._min_num_samples = first_true(lambda n: frames(n) > 0, 2, round(0.5 * self.sample_rate))
        return math.ceil(self.F * self._min_num_samples / (self.duration * self.sample_rate))

    def _advance(self, slots: np.ndarray, start: np.ndarray, emit_from: np.ndarray, emit_to: np.ndarray,
                 flush: bool = False) -> np.ndarray:
        """the device side of one step for the ready `slots`: segmentation, statistics, masks, embeddings,
        `cluster_step`, `emit`, ONE download -> (M, E, K) uint8.  `flush`: only the emission (no chunk is added)."""
        from . import frames as frame_ops
        ffi.require_gpu()
        M = len(slots)
        E = max(1, int((emit_to - emit_from).max()))
        stage = self.stage_hook or (lambda name: None)
        with torch.cuda.device(self.device):
            table = torch.from_numpy(np.stack([slots.astype(np.int64), start, emit_from, emit_to])).to(self.device)
            slots_device = table[0].to(torch.int32)
            if flush:
                seg = torch.zeros((M, self.F, self.S), dtype=torch.uint8, device=self.device)
                mp = torch.full((M, self.S), -1, dtype=torch.int32, device=self.device)
            else:
                flat = self.buffer.index_select(0, table[0]).view(-1)
                stage("windows")
                _, seg = self.seg_model.engine.forward_strided(flat, self.window, M, self.window, want_logp=False,
                                                               want_multilabel=True)
                stage("segmentation")
                active, clean = frame_ops.chunk_stats(seg)
                masks = frame_ops.embedding_masks(seg, clean, self.exclude_overlap, self._min_num_frames())
                emb = self.emb_model.engine.forward_strided(flat, self.window, M, self.window, masks)
                stage("embeddings")
                mp = cluster_step(slots, emb, active, clean, self.centroid_sum, self.centroid_n,
                                  self.min_active_frames, self.min_update_frames, self.delta_new,
                                  slots_device=slots_device)
                stage("cluster_step")
            out = emit(slots, seg, mp, start, emit_from, emit_to, self.acc_sum, self.acc_cnt, E, table_device=table)
            stage("emit")
            out = out.cpu().numpy()
            stage("download")
            return out

    # -------------------------------------------------------------------------------------------------- streaming
    def _append(self, blocks: torch.Tensor, slots: Sequence[int]):
        idx = torch.as_tensor(np.asarray(slots, dtype=np.int64)).to(self.device)
        rows = self.buffer.index_select(0, idx)
        self.buffer.index_copy_(0, idx, torch.cat([rows[:, self.step_samples:], blocks], dim=1))

    def _run(self, ready: List[int], limit: Optional[Dict[int, int]] = None) -> Dict[int, Tuple[int, np.ndarray]]:
        """one step of the `ready` slots (their window is in the buffer) -> {slot: (first_frame, decisions)}"""
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
        out = self._advance(slots, start, emit_from, emit_to)
        return self._collect(ready, out, emit_from, emit_to, chunk=True)

    def _collect(self, ready, out, emit_from, emit_to, chunk: bool):
        result = {}
        for i, slot in enumerate(ready):
            stream = self._streams[slot]
            rows = np.ascontiguousarray(out[i, :int(emit_to[i] - emit_from[i])])
            stream.rows.append(rows)
            stream.emitted = int(emit_to[i])
            stream.chunks += int(chunk)
            result[slot] = (int(emit_from[i]), rows)
        return result

    def push(self, blocks, slots: Sequence[int]) -> Dict[int, Tuple[int, np.ndarray]]:
        """One step of audio for each listed slot: blocks (M, step_samples) float32, on the host or the device.  The
        slots that now hold a full window run one step together -> {slot: (first_frame, decisions (n, K) uint8)} for
        those; between the upload of the blocks and the one download nothing waits for the device (the row counts
        of the download are host arithmetic, so only the rows cross)."""
        slots = [int(s) for s in slots]
        if len(set(slots)) != len(slots):
            raise ValueError("StreamBank.push: a slot is listed twice")
        streams = [self._stream(s) for s in slots]
        blocks = torch.as_tensor(blocks)
        if tuple(blocks.shape) != (len(slots), self.step_samples) or blocks.dtype != torch.float32:
            raise ValueError(f"StreamBank.push: blocks must be ({len(slots)}, {self.step_samples}) float32")
        if not slots:
            return {}
        self._append(blocks.to(self.device), slots)
        ready = []
        for slot, stream in zip(slots, streams):
            stream.blocks += 1
            if stream.blocks >= self.steps_per_window:
                ready.append(slot)
        return self._run(ready)

    def close(self, slot: int, tail=None) -> Tuple[int, np.ndarray]:
        """End of a stream.  `tail`: its last samples, fewer than one step (1-D float32), or None.  A partial block is
        zero-padded to one step and run; a stream shorter than one chunk gets one zero-padded chunk; then every frame
        up to the stream's last one (the frames offline inference gives a file of that many samples) is emitted and
        the slot is freed.  -> (first_frame, decisions) of what this call emitted; `annotation(slot)` and
        `centroids(slot)` stay valid until the slot is opened again."""
        stream = self._stream(slot)
        slot = int(slot)
        tail = None if tail is None else torch.as_tensor(tail).reshape(-1)
        n_tail = 0 if tail is None else int(tail.numel())
        if n_tail >= self.step_samples:
            raise ValueError("StreamBank.close: the tail is shorter than one step; push whole steps")
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
            parts.append(self._run([slot], {slot: total})[slot][1])
        elif n_tail:
            parts.append(self._run([slot], {slot: total})[slot][1])
        if stream.emitted < total:
            frm, to = np.array([stream.emitted], dtype=np.int64), np.array([total], dtype=np.int64)
            out = self._advance(np.array([slot], dtype=np.int32), np.array([-1], dtype=np.int64), frm, to, flush=True)
            parts.append(self._collect([slot], out, frm, to, chunk=False)[slot][1])
        stream.open = False
        rows = np.concatenate(parts) if parts else np.zeros((0, self.K), dtype=np.uint8)
        return first, rows

    # ---------------------------------------------------------------------------------------------------- results
    def decisions(self, slot: int) -> np.ndarray:
        """every row emitted so far for the slot's stream, (frames, K) uint8 from frame 0"""
        rows = self._streams[int(slot)].rows
        return np.concatenate(rows) if rows else np.zeros((0, self.K), dtype=np.uint8)

    def annotation(self, slot: int, uri: Optional[str] = None) -> Annotation:
        """the turns emitted so far: runs of every column of `decisions(slot)`, labelled SPEAKER_%02d by global
        speaker, with the frame middles `to_annotation` gives them"""
        return self.annotation_of(self.decisions(slot), uri)

    def annotation_of(self, rows: np.ndarray, uri: Optional[str] = None) -> Annotation:
        """the turns of decisions (frames, K) uint8 from frame 0, as `annotation` gives them"""
        from .diarization import to_annotation
        used = [k for k in range(self.K) if rows[:, k].any()]
        feature = SlidingWindowFeature(rows[:, used].astype(np.float32),
                                       SlidingWindow(start=0.0, duration=self.frames.duration, step=self.frames.step))
        feature.labels = [f"SPEAKER_{k:02d}" for k in used]
        out = to_annotation(feature)
        out.uri = uri
        return out

    def centroids(self, slot: int) -> np.ndarray:
        """centroid_sum / centroid_n of the slot: (K, D) float64, NaN rows for the speakers not founded yet -- row k is
        SPEAKER_k, what `identification.identify` takes as `speaker_embeddings`"""
        slot = int(slot)
        n = self.centroid_n[slot].to(torch.float64)[:, None]
        return (self.centroid_sum[slot] / n).cpu().numpy()

    # ---------------------------------------------------------------------------------------------- recorded files
    def schedule(self, num_samples: int) -> Tuple[int, np.ndarray, int]:
        """`file_schedule` with the geometry of this bank"""
        return file_schedule(num_samples, window=self.window, step_samples=self.step_samples,
                             sample_rate=self.sample_rate, duration=self.duration, step=self.step,
                             latency=self.latency, frames=self.frames, F=self.F)

    def threshold_frames(self, min_active: float, min_update: float) -> Tuple[int, int]:
        """(min_active_frames, min_update_frames) of thresholds in seconds, rounded as the constructor rounds them"""
        return max(1, int(np.rint(min_active / self.frames.step))), int(np.rint(min_update / self.frames.step))

    def front_ends(self, waveforms: Sequence[torch.Tensor]) -> List[FrontEnd]:
        """`front_end` of several recordings; consecutive recordings share launch groups"""
        ffi.require_gpu()
        from . import frames as frame_ops
        dev = self.device
        plans, windows = [], []             # per file (C, schedule, total); per file a (C, window) strided view
        for waveform in waveforms:
            wav = torch.as_tensor(waveform).reshape(-1).to(dev, torch.float32)
            C, rows, total = self.schedule(wav.numel())
            padded = torch.zeros(self.window + max(C - 1, 0) * self.step_samples, dtype=torch.float32, device=dev)
            padded[:wav.numel()] = wav
            plans.append((C, rows, total))
            windows.append(padded.unfold(0, self.window, self.step_samples)[:C])
        per_group = max(1, self.front_end_bytes // (4 * self.window))
        parts = {i: [] for i in range(len(plans))}
        group, size = [], 0

        def run(group):
            with torch.cuda.device(dev):
                flat = torch.cat([windows[i][a:b] for i, a, b in group]).contiguous().view(-1)
                M = flat.numel() // self.window
                _, seg = self.seg_model.engine.forward_strided(flat, self.window, M, self.window, want_logp=False,
                                                               want_multilabel=True)
                active, clean = frame_ops.chunk_stats(seg)
                masks = frame_ops.embedding_masks(seg, clean, self.exclude_overlap, self._min_num_frames())
                emb = self.emb_model.engine.forward_strided(flat, self.window, M, self.window, masks)
            at = 0
            for i, a, b in group:
                parts[i].append(tuple(t[at:at + b - a] for t in (seg, active, clean, emb)))
                at += b - a

        for i, (C, _, _) in enumerate(plans):            # greedy: a group takes chunks of consecutive files
            a = 0
            while a < C:
                b = min(C, a + per_group - size)
                group.append((i, a, b))
                size += b - a
                a = b
                if size == per_group:
                    run(group)
                    group, size = [], 0
        if group:
            run(group)
        out = []
        for i, (C, rows, total) in enumerate(plans):
            if C:
                seg, active, clean, emb = (torch.cat(t) if len(t) > 1 else t[0] for t in zip(*parts[i]))
            else:
                seg = torch.zeros((0, self.F, self.S), dtype=torch.uint8, device=dev)
                active = clean = torch.zeros((0, self.S), dtype=torch.int32, device=dev)
                emb = torch.zeros((0, self.S, self.D), dtype=torch.float32, device=dev)
            out.append(FrontEnd(seg.contiguous(), active.contiguous(), clean.contiguous(), emb.contiguous(), rows, total))
        (self.stage_hook or (lambda name: None))("front_end")
        return out

    def front_end(self, waveform: torch.Tensor) -> FrontEnd:
        """Everything the rule reads for a whole recording (1-D float32): the engine calls `push` makes for one chunk,
        made on GATHERED contiguous windows (M, window) -- chunk c is `padded[c step_samples : c step_samples +
        window]` -- in groups of at most `front_end_bytes`.  A window's result does not depend on the M it is batched
        with, so these are the bits streaming gives."""
        return self.front_ends([waveform])[0]

    def replay(self, front_ends, params: Optional[Sequence[Tuple[float, float, float]]] = None):
        """Recorded files through the rule without streaming them.  `front_ends`: a `FrontEnd` or a list of them;
        `params`: a list of (delta_new, min_active, min_update) in seconds, default the bank's own triple.  Every
        (file, triple) is a job; jobs are split over launches by `replay_bytes`.  -> per file (a list input) per triple
        (a `params` input) one `Replayed`: a single FrontEnd without `params` gives one `Replayed`, a list of files
        with `params` gives results[file][triple]."""
        single = isinstance(front_ends, FrontEnd)
        fes = [front_ends] if single else list(front_ends)
        if params is None:
            triples = [(self.delta_new, self.min_active_frames, self.min_update_frames)]
        else:
            triples = [(float(d), *self.threshold_frames(a, u)) for d, a, u in params]
        pairs = [(f, t) for f in range(len(fes)) for t in range(len(triples))]
        flat = self.replay_pairs(fes, triples, pairs)
        nested = [[flat[f * len(triples) + t] for t in range(len(triples))] for f in range(len(fes))]
        if params is None:
            nested = [row[0] for row in nested]
        return nested[0] if single else nested

    def replay_pairs(self, fes: Sequence[FrontEnd], triples: Sequence[Tuple[float, int, int]],
                     pairs: Sequence[Tuple[int, int]]) -> List[Replayed]:
        """the jobs `pairs` = (index into `fes`, index into `triples` of (delta_new, min_active_frames,
        min_update_frames)) -> one `Replayed` each, in order"""
        ffi.require_gpu()
        dev = self.device
        if not pairs:
            return []
        counts = np.array([fe.num_chunks for fe in fes], dtype=np.int64)
        chunk_off = np.concatenate([[0], np.cumsum(counts)])
        sched_off = np.concatenate([[0], np.cumsum(counts + 1)])
        files = np.stack([chunk_off[:-1], counts, sched_off[:-1], [fe.total for fe in fes]], axis=1).astype(np.int64)
        sched = np.concatenate([fe.schedule for fe in fes]).astype(np.int64)
        emb, active, clean, seg = (torch.cat([getattr(fe, name) for fe in fes]) if len(fes) > 1 else getattr(fes[0], name)
                                   for name in ("emb", "active", "clean", "seg"))
        state = 8 * self.K * self.D + 4 * self.K + 4 * self.R * (self.K + 1)
        results: List[Replayed] = []
        stage = self.stage_hook or (lambda name: None)
        at = 0
        while at < len(pairs):
            batch, used = [], 0
            while at + len(batch) < len(pairs) and len(batch) < 65535:
                f = pairs[at + len(batch)][0]
                need = state + int(fes[f].total) * self.K + 4 * int(counts[f]) * self.S
                if batch and used + need > self.replay_bytes:
                    break
                batch.append(pairs[at + len(batch)])
                used += need
            at += len(batch)
            J = len(batch)
            jobs = np.array([[f, triples[t][1], triples[t][2]] for f, t in batch], dtype=np.int32)
            delta = np.array([triples[t][0] for _, t in batch], dtype=np.float64)
            rows = np.array([[counts[f], fes[f].total] for f, _ in batch], dtype=np.int64)
            offsets = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(rows, axis=0)])
            with torch.cuda.device(dev):
                csum = torch.zeros((J, self.K, self.D), dtype=torch.float64, device=dev)
                cn = torch.zeros((J, self.K), dtype=torch.int32, device=dev)
                acc_sum = torch.zeros((J, self.R, self.K), dtype=torch.int32, device=dev)
                acc_cnt = torch.zeros((J, self.R), dtype=torch.int32, device=dev)
                stage("replay_state")
                mp, out = replay_jobs(emb, active, clean, seg, files, sched, jobs, delta, offsets[:-1], csum, cn,
                                      acc_sum, acc_cnt, map_rows=int(offsets[-1, 0]), out_rows=int(offsets[-1, 1]))
                stage("replay")
                centroids = (csum / cn.to(torch.float64)[:, :, None]).cpu().numpy()
                mp, out = mp.cpu().numpy(), out.cpu().numpy()
                stage("download")
            for j in range(J):
                results.append(Replayed(np.ascontiguousarray(out[offsets[j, 1]:offsets[j + 1, 1]]),
                                        np.ascontiguousarray(mp[offsets[j, 0]:offsets[j + 1, 0]]), centroids[j]))
        return results


class OnlineSpeakerDiarization(Pipeline):
    """Diarizes files as if they were streamed: `step` seconds at a time through a `StreamBank`, every decision made
    with the audio up to `latency` seconds later and never revised.  `apply(file)` streams one file through a bank of
    one; `apply_batch(files, num_slots=None)` streams many concurrently (files of different lengths end at different
    steps, and waiting files take the freed slots).  Both return `Annotation`s; a file's Annotation does not depend on
    the files it shared the bank with.  With `replay=True` both skip the streaming loop: the files are recorded, so
    every chunk's front end is computed at once and the rule is replayed on the device (`StreamBank.replay`), with the
    same turns.  The thresholds are the UNTUNED defaults of `StreamBank`; `tuning.OnlineTuner` tunes them on a corpus."""

    def __init__(self, segmentation=None, embedding=None, step: float = 0.5, latency: Optional[float] = None,
                 max_speakers: int = 20, delta_new: float = 1.0, min_active: float = 0.25, min_update: float = 1.0,
                 exclude_overlap: bool = True, token=None, cache_dir=None):
        super().__init__()
        if segmentation is None or embedding is None:
            raise ValueError("`segmentation` and `embedding` must be local checkpoints (or Model instances): Hugging "
                             "Face defaults cannot be downloaded in this build.")
        from .speaker_verification import get_model
        self.segmentation_model = get_model(segmentation, token=token, cache_dir=cache_dir)
        self.embedding_model = get_model(embedding, token=token, cache_dir=cache_dir)
        self.bank_options = dict(step=step, latency=latency, max_speakers=max_speakers, delta_new=delta_new,
                                 min_active=min_active, min_update=min_update, exclude_overlap=exclude_overlap)

    def default_parameters(self):
        return {}

    def classes(self):
        speaker = 0
        while True:
            yield f"SPEAKER_{speaker:02d}"
            speaker += 1

    def get_metric(self):
        from . import annotation_metrics
        device = getattr(self, "device", None)
        return annotation_metrics.DiarizationErrorRate(
            device=device if device is not None and device.type == "cuda" else None)

    def get_direction(self) -> str:
        return "minimize"

    def bank(self, num_slots: int) -> StreamBank:
        ffi.require_gpu()
        device = getattr(self, "device", None)
        if device is None or getattr(device, "type", None) != "cuda":
            raise RuntimeError("OnlineSpeakerDiarization must be moved to the GPU first: "
                               "pipeline.to(torch.device('cuda')) -- there is no CPU fallback")
        return StreamBank(self.segmentation_model, self.embedding_model, num_slots, device=device, **self.bank_options)

    def apply(self, file, replay: bool = False, **kwargs) -> Annotation:
        return self.apply_batch([file], num_slots=1, replay=replay)[0]

    def _apply_batch(self, files: list, **kwargs):
        return zip(files, self.apply_batch(files, **kwargs))

    def apply_batch(self, files: Iterable, num_slots: Optional[int] = None, replay: bool = False) -> List[Annotation]:
        """`replay=True`: the files are recorded, so nothing has to arrive slowly -- the front ends of all files at
        once (`StreamBank.front_ends`), then ONE replay with the files as jobs (`StreamBank.replay`): the same turns
        without one push per step.  The default is the streaming loop."""
        from .audio import Audio
        files = [Audio.validate_file(f) for f in files]
        if not files:
            return []
        if replay:
            bank = self.bank(1)
            audio = Audio(sample_rate=bank.sample_rate, mono="downmix")
            replayed = bank.replay(bank.front_ends([audio(f)[0].reshape(-1) for f in files]))
            return [bank.annotation_of(r.decisions, uri=f["uri"]) for f, r in zip(files, replayed)]
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
