"""Online (streaming) speaker diarization of many concurrent streams (csrc/online.hip, include/pyannote_amd_online.h).

A `StreamBank` holds N stream slots.  Every `push` takes one step of audio for some of them; the slots that now hold a
full window go through ONE segmentation forward, ONE embedding forward, one incremental clustering launch
(`cluster_step`) and one rolling overlap-add launch (`emit`), and the next decisions of all of them come back in one
download.  Centroids and the overlap-add ring stay on the device between pushes.

The clustering is the incremental rule of Coria et al., "Overlap-aware low-latency online speaker diarization based on
end-to-end local segmentation" (ASRU 2021), stated in full in the header; it is not part of the reference library and
is held to a numpy model of its own definition (tests/online_model.py).  There is no host implementation behind these
calls."""
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
    defaults: no trained checkpoint is available offline to tune them with (a `ClusteringTuner` leg is future
    work).

    open() -> slot; push(blocks, slots) -> {slot: (first_frame, decisions)}; close(slot, tail) -> (first_frame,
    decisions); annotation(slot); centroids(slot)."""

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
        from .diarization import to_annotation
        rows = self.decisions(slot)
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


class OnlineSpeakerDiarization(Pipeline):
    """Diarizes files as if they were streamed: `step` seconds at a time through a `StreamBank`, every decision made
    with the audio up to `latency` seconds later and never revised.  `apply(file)` streams one file through a bank of
    one; `apply_batch(files, num_slots=None)` streams many concurrently (files of different lengths end at different
    steps, and waiting files take the freed slots).  Both return `Annotation`s; a file's Annotation does not depend on
    the files it shared the bank with.  The thresholds are the UNTUNED defaults of `StreamBank`."""

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

    def apply(self, file, **kwargs) -> Annotation:
        return self.apply_batch([file], num_slots=1)[0]

    def _apply_batch(self, files: list, **kwargs):
        return zip(files, self.apply_batch(files, **kwargs))

    def apply_batch(self, files: Iterable, num_slots: Optional[int] = None) -> List[Annotation]:
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
