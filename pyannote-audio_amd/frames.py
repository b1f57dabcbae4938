"""Frame-domain stages on the GPU (csrc/frames.hip): speaker counting, overlap-add reconstruction,
top-k discretisation, per-(chunk, speaker) statistics and embedding-mask selection.

Mirrors pipelines/utils/diarization.py:150-268, pipelines/speaker_diarization.py:375-427, 480-528 and
the overlap-add of core/inference.py:498-620 for the case the diarization pipeline uses (hamming=False,
warm_up=(0, 0), hard {0,1} scores).  Results are bit-identical to the reference's float32 arithmetic
(small-integer sums; see the kernel file).  There is no host implementation behind these calls."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import ffi
from .core import SlidingWindow, SlidingWindowFeature


def frame_geometry(chunks: SlidingWindow, frames: SlidingWindow, num_chunks: int
                   ) -> Tuple[np.ndarray, int, SlidingWindow]:
    """start frame of every chunk and the total number of global frames, in the reference's float64
    arithmetic (core/inference.py:529-571, :596)."""
    out_frames = SlidingWindow(start=chunks.start, duration=frames.duration, step=frames.step)
    num_frames = out_frames.closest_frame(
        chunks.start + chunks.duration + (num_chunks - 1) * chunks.step + 0.5 * out_frames.duration) + 1
    c = np.arange(num_chunks, dtype=np.float64)
    t = (chunks.start + c * chunks.step) + 0.5 * out_frames.duration
    starts = np.rint((t - out_frames.start - 0.5 * out_frames.duration) / out_frames.step)
    return starts.astype(np.int32), int(num_frames), out_frames


def as_device_segmentation(seg, device: torch.device) -> torch.Tensor:
    """(C, F, S) uint8 device tensor from a device tensor or a host array of {0,1} (NaN -> 0)."""
    if isinstance(seg, torch.Tensor):
        return seg.to(device=device, dtype=torch.uint8).contiguous()
    return torch.from_numpy(np.nan_to_num(np.asarray(seg), nan=0.0).astype(np.uint8)).to(device)


@ffi.on_device(lambda seg, *a, **k: seg.device)
def chunk_stats(seg: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> active (C,S) int32 = #frames speaker s is on, clean (C,S) int32 = #frames it speaks alone."""
    C, F, S = seg.shape
    active = torch.empty((C, S), dtype=torch.int32, device=seg.device)
    clean = torch.empty((C, S), dtype=torch.int32, device=seg.device)
    ffi.check(ffi.load().pa_seg_chunk_stats(ffi.ptr(seg), C, F, S, ffi.ptr(active), ffi.ptr(clean),
                                            ffi.stream()), "pa_seg_chunk_stats")
    return active, clean


@ffi.on_device(lambda seg, *a, **k: seg.device)
def embedding_masks(seg: torch.Tensor, clean: torch.Tensor, exclude_overlap: bool,
                    min_num_frames: int) -> torch.Tensor:
    C, F, S = seg.shape
    masks = torch.empty((C, S, F), dtype=torch.float32, device=seg.device)
    ffi.check(ffi.load().pa_embedding_masks(ffi.ptr(seg), C, F, S, ffi.ptr(clean), int(exclude_overlap),
                                            int(min_num_frames), ffi.ptr(masks), ffi.stream()),
              "pa_embedding_masks")
    return masks


@ffi.on_device(lambda seg, *a, **k: seg.device)
def speaker_count(seg: torch.Tensor, chunks: SlidingWindow, frames: SlidingWindow
                  ) -> SlidingWindowFeature:
    """pipelines/utils/diarization.py:150-185 with warm_up=(0, 0)."""
    C, F, S = seg.shape
    starts, T, out_frames = frame_geometry(chunks, frames, C)
    dev = seg.device
    st = torch.from_numpy(starts).to(dev)
    count = torch.empty(T, dtype=torch.uint8, device=dev)
    scratch = torch.empty(2 * T, dtype=torch.int32, device=dev)
    ffi.check(ffi.load().pa_speaker_count(ffi.ptr(seg), C, F, S, ffi.ptr(st), T, ffi.ptr(count),
                                          ffi.ptr(scratch), ffi.stream()), "pa_speaker_count")
    return SlidingWindowFeature(count.cpu().numpy().reshape(T, 1), out_frames)


def gather_chunks(wavs, chunk_file, chunk_start, num_samples: int) -> torch.Tensor:
    """Chunks of several device-resident waveforms -> one dense (num_chunks, num_samples) float32 device tensor
    (`pa_gather_chunks`): row c = wavs[chunk_file[c]][chunk_start[c] : chunk_start[c] + num_samples], zeros past that
    waveform's end.  wavs: 1-D float32 tensors on one device; chunk_file / chunk_start: host integer sequences.
    What a launch group of the embedding network reads when its chunks come from several files."""
    chunk_file = np.ascontiguousarray(chunk_file, dtype=np.int32).reshape(-1)
    chunk_start = np.ascontiguousarray(chunk_start, dtype=np.int64).reshape(-1)
    if chunk_file.size != chunk_start.size:
        raise ValueError("gather_chunks: one file index and one start per chunk")
    if not len(wavs) or num_samples < 0:
        raise ValueError("gather_chunks: no waveform, or a negative chunk length")
    dev = wavs[0].device
    for wav in wavs:
        if wav.dim() != 1 or wav.dtype != torch.float32 or wav.device != dev:
            raise ValueError("gather_chunks: waveforms must be 1-D float32 tensors on one device")
    if chunk_file.size and (chunk_file.min() < 0 or chunk_file.max() >= len(wavs) or chunk_start.min() < 0):
        raise ValueError("gather_chunks: a chunk names a waveform that is not there, or starts before its first sample")
    with torch.cuda.device(dev):
        out = torch.empty((chunk_file.size, num_samples), dtype=torch.float32, device=dev)
        if not out.numel():
            return out
        wavs = [w.contiguous() for w in wavs]
        # ONE upload: [base pointers | lengths | starts | file indices] (8-byte entries first)
        table = np.concatenate([np.array([w.data_ptr() for w in wavs], dtype=np.int64),
                                np.array([w.numel() for w in wavs], dtype=np.int64), chunk_start]).view(np.uint8)
        table = torch.from_numpy(np.concatenate([table, chunk_file.view(np.uint8)])).to(dev)
        base = table.data_ptr()
        n, c = 8 * len(wavs), 8 * chunk_file.size
        ffi.check(ffi.load().pa_gather_chunks(ffi.c_fp(base), ffi.c_fp(base + n), ffi.c_fp(base + 2 * n + c),
                                              ffi.c_fp(base + 2 * n), chunk_file.size, num_samples, ffi.ptr(out),
                                              ffi.stream()), "pa_gather_chunks")
        # (`table` and the waveforms are used by a launch that is queued on the current stream: torch's allocator
        #  hands their memory out again to work on that same stream only, i.e. behind the launch)
    return out


def aggregate_device(scores, chunks: SlidingWindow, frames: SlidingWindow, device: torch.device,
                     warm_up: Tuple[float, float] = (0.0, 0.0), epsilon: float = 1e-12, hamming: bool = False,
                     missing: float = np.nan, skip_average: bool = False) -> Tuple[torch.Tensor, SlidingWindow]:
    """`aggregate` whose result stays where the kernel wrote it: (T, K) float32 device tensor and its frame grid.
    Same kernel, same arguments, so bit-identical to `aggregate` (which is this plus one copy)."""
    x = torch.as_tensor(scores).to(device=device, dtype=torch.float32).contiguous()
    C, F, K = x.shape
    starts, T, out_frames = frame_geometry(chunks, frames, C)
    window = np.hamming(F) if hamming else np.ones(F)
    warm = np.ones(F)
    left = round(warm_up[0] / chunks.duration * F)
    right = round(warm_up[1] / chunks.duration * F)
    warm[:left] = epsilon
    warm[F - right:] = epsilon
    with torch.cuda.device(device):
        w = torch.from_numpy(np.ascontiguousarray(window, dtype=np.float64)).to(device)
        wu = torch.from_numpy(warm).to(device)
        st = torch.from_numpy(starts).to(device)
        out = torch.empty((T, K), dtype=torch.float32, device=device)
        ffi.check(ffi.load().pa_aggregate(ffi.ptr(x), C, F, K, ffi.ptr(st), T, ffi.ptr(w), ffi.ptr(wu), float(epsilon),
                                          float(missing), int(skip_average), ffi.ptr(out), ffi.stream()),
                  "pa_aggregate")
    return out, out_frames


def aggregate(scores, chunks: SlidingWindow, frames: SlidingWindow, device: torch.device,
              warm_up: Tuple[float, float] = (0.0, 0.0), epsilon: float = 1e-12, hamming: bool = False,
              missing: float = np.nan, skip_average: bool = False) -> SlidingWindowFeature:
    """`Inference.aggregate` (core/inference.py:498-620) on the GPU: scores (C, F, K) host array or device
    tensor -> SlidingWindowFeature (T, K) float32, bit-identical to the reference's chunk loop."""
    out, out_frames = aggregate_device(scores, chunks, frames, device, warm_up=warm_up, epsilon=epsilon,
                                       hamming=hamming, missing=missing, skip_average=skip_average)
    return SlidingWindowFeature(out.cpu().numpy(), out_frames)


@ffi.on_device(lambda scores, *a, **k: scores.device)
def binarize_regions(scores: torch.Tensor, frames: SlidingWindow, onset, offset, min_duration_on=0.0,
                     min_duration_off=0.0, capacity: Optional[int] = None, return_tracks: bool = False):
    """`Binarize` (utils/signal.py:207-318, no padding) of every column of an aggregated (T, K) float32 device
    tensor at once (`pa_binarize_regions`): per-class thresholds and minimum durations (scalars are shared) ->
    list of K float64 arrays (n_k, 2) of region start / end times in time order, bit-identical to the host's
    frame middles.  With `return_tracks`, also K int arrays: the position of every region in the reference's
    track-name sequence.  Only the region lists cross to the host.  `capacity` (regions per class before
    merging) defaults to the most a class can have, T // 2."""
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError("binarize_regions expects a (frames, classes) float32 tensor")
    x = scores.contiguous()
    T, K = x.shape
    dev = x.device

    def per_class(v, dtype):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (K,)))

    on, off = per_class(onset, np.float32), per_class(offset, np.float32)
    d_on, d_off = per_class(min_duration_on, np.float64), per_class(min_duration_off, np.float64)
    cap = T // 2 if capacity is None else int(capacity)
    lib = ffi.load()
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    regions = torch.empty((K, cap, 2), dtype=torch.float64, device=dev)
    tracks = torch.empty((K, cap), dtype=torch.int32, device=dev)
    nbytes = int(lib.pa_binarize_regions_workspace_bytes(T, K, cap))
    workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    ffi.check(lib.pa_binarize_regions(
        ffi.ptr(x), T, K, on.ctypes.data, off.ctypes.data, d_on.ctypes.data, d_off.ctypes.data,
        float(frames.start), float(frames.duration), float(frames.step), cap, ffi.ptr(counts), ffi.ptr(regions),
        ffi.ptr(tracks), ffi.ptr(workspace), nbytes, ffi.stream()), "pa_binarize_regions")
    n = counts.cpu().numpy()
    # one packed copy of the filled prefixes: rows of class k first, then k + 1, ...
    packed = torch.cat([regions[k, :n[k]] for k in range(K)]).cpu().numpy()
    bounds = np.concatenate([[0], np.cumsum(n)])
    out = [packed[bounds[k]:bounds[k + 1]] for k in range(K)]
    if not return_tracks:
        return out
    packed_tracks = torch.cat([tracks[k, :n[k]] for k in range(K)]).cpu().numpy()
    return out, [packed_tracks[bounds[k]:bounds[k + 1]] for k in range(K)]


# ------------------------------------------------------------------------- a ragged list of files in shared launches
#: rows of a file in the packed aggregate start at a multiple of this (RG_CHUNK of csrc/regions.h: a 64-frame count of
#: the region kernels never straddles two files)
FILES_ROW_ALIGN = 64


def files_layout(num_samples_per_file, inference):
    """Where the chunks and the aggregated rows of several files lie when they share launches (`forward_files`,
    `aggregate_files`, `binarize_regions_files`) -> (chunks_per_file, chunk0, row0, T), int32 arrays of N, N + 1,
    N + 1 and N entries: file f owns chunks chunk0[f]:chunk0[f + 1] and rows row0[f]:row0[f + 1] of the packed
    aggregate, of which the first T[f] are its frames -- the rows `Inference.slide` / `slide_device` return for the
    file (the padding of a zero-padded last chunk cut off by the loose crop).  row0[f] is a multiple of 64.  Host
    arithmetic only, with `Inference.num_chunks`, `frame_geometry` and the crop of `slide_device`."""
    from .core import Segment
    from .inference import Inference
    model = inference.model
    sample_rate = model.audio.sample_rate
    window_size = model.audio.get_num_samples(inference.duration)
    step_size = round(inference.step * sample_rate)
    chunks = SlidingWindow(start=0.0, duration=inference.duration, step=inference.step)
    counts, kept = [], []
    for num_samples in num_samples_per_file:
        num_samples = int(num_samples)
        n, has_last = Inference.num_chunks(num_samples, window_size, step_size)
        _, num_frames, out_frames = frame_geometry(chunks, model.receptive_field, n + has_last)
        if has_last:
            (first, stop), = out_frames.crop(Segment(0.0, num_samples / sample_rate), mode="loose",
                                             return_ranges=True)
            num_frames = min(stop, num_frames) - max(first, 0)
        counts.append(n + has_last)
        kept.append(max(num_frames, 0))
    counts = np.asarray(counts, dtype=np.int32).reshape(-1)
    T = np.asarray(kept, dtype=np.int32).reshape(-1)
    owned = (T.astype(np.int64) + FILES_ROW_ALIGN - 1) // FILES_ROW_ALIGN * FILES_ROW_ALIGN
    chunk0 = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    row0 = np.concatenate([[0], np.cumsum(owned)])
    if chunk0[-1] > np.iinfo(np.int32).max or row0[-1] > np.iinfo(np.int32).max:
        raise ValueError("files_layout: more than 2^31 - 1 chunks or rows in one group")
    return counts, chunk0.astype(np.int32), row0.astype(np.int32), T


def _files_tables(row0, T, what):
    """the row tables of a group of files, checked as the kernels' entry points check them"""
    row0 = np.ascontiguousarray(row0, dtype=np.int32).reshape(-1)
    T = np.ascontiguousarray(T, dtype=np.int32).reshape(-1)
    if len(row0) != len(T) + 1:
        raise ValueError(f"{what}: row0 has one entry more than T")
    if len(T) > 65535:
        raise ValueError(f"{what}: {len(T)} files, at most 65535 share a call")
    owned = np.diff(row0.astype(np.int64))
    if row0[0] != 0 or (owned < 0).any() or (row0 % FILES_ROW_ALIGN).any():
        raise ValueError(f"{what}: row0 starts at 0 and is a non-decreasing table of multiples of {FILES_ROW_ALIGN}")
    if (T < 0).any() or (T > owned).any():
        raise ValueError(f"{what}: a file keeps more frames than it owns rows")
    return row0, T


def aggregate_files(scores: torch.Tensor, chunk0, row0, T, chunks: SlidingWindow, frames: SlidingWindow,
                    any: bool = False, warm_up: Tuple[float, float] = (0.0, 0.0), epsilon: float = 1e-12,
                    hamming: bool = False, missing: float = np.nan, skip_average: bool = False,
                    packed: bool = False):
    """`aggregate_device` of several files in ONE launch (`pa_aggregate_files`).  scores: (sum of chunks, F, S) device
    tensor, the files' chunks in file order as `forward_files` leaves them -- float32, or the uint8 hard multilabel
    output (with `any` only); chunk0, row0, T: as `files_layout` returns them.  `any`: the chunks collapse to one
    class first, the maximum over the S columns (VoiceActivityDetection's `any_speaker`).
    -> ([(T[f], K) float32 device tensors, views of one buffer], frame grid); with `packed`, the buffer itself,
    (row0[-1], K): file f's rows at row0[f], NaN in the padding rows.  Every file's rows are bit for bit those of
    `aggregate_device` on its chunks alone."""
    if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dim() == 3
            and scores.dtype in (torch.float32, torch.uint8)):
        raise ValueError("aggregate_files expects a (chunks, frames, classes) float32 or uint8 device tensor")
    if scores.dtype == torch.uint8 and not any:
        raise ValueError("aggregate_files: uint8 scores are hard decisions, aggregated with any=True only")
    x = scores.contiguous()
    total, F, S = x.shape
    row0, T = _files_tables(row0, T, "aggregate_files")
    chunk0 = np.ascontiguousarray(chunk0, dtype=np.int32).reshape(-1)
    N = len(T)
    counts = np.diff(chunk0.astype(np.int64))
    if len(chunk0) != N + 1 or chunk0[0] != 0 or (counts < 0).any() or chunk0[-1] != total:
        raise ValueError("aggregate_files: chunk0 is a non-decreasing table from 0 to the number of chunks, one entry "
                         "more than there are files")
    most = int(counts.max()) if N else 0
    starts, _, out_frames = frame_geometry(chunks, frames, most)
    covered = {int(c): frame_geometry(chunks, frames, int(c))[1] if c else 0 for c in np.unique(counts)}
    for f in np.flatnonzero(T > 0):
        if T[f] > covered[int(counts[f])]:
            raise ValueError(f"aggregate_files: file {f} keeps {T[f]} frames, its {counts[f]} chunks cover fewer")
    window = np.hamming(F) if hamming else np.ones(F)
    warm = np.ones(F)
    left = round(warm_up[0] / chunks.duration * F)
    right = round(warm_up[1] / chunks.duration * F)
    warm[:left] = epsilon
    warm[F - right:] = epsilon
    dev = x.device
    K = 1 if any else S
    rows = int(row0[-1])
    with torch.cuda.device(dev):
        # ONE upload: [window | warm-up] (8-byte entries), then [chunk0 | row0 | T | start frames]
        table = np.concatenate([np.ascontiguousarray(window, dtype=np.float64), warm]).view(np.uint8)
        ints = np.concatenate([chunk0, row0, T, starts.astype(np.int32)]).astype(np.int32)
        table = torch.from_numpy(np.concatenate([table, ints.view(np.uint8)])).to(dev)
        base = table.data_ptr()
        at = base + 16 * F
        out = torch.empty((rows, K), dtype=torch.float32, device=dev)
        ffi.check(ffi.load().pa_aggregate_files(
            ffi.ptr(x) if x.numel() else None, int(x.dtype == torch.uint8), total, F, S, int(bool(any)), N,
            ffi.c_fp(at), ffi.c_fp(at + 4 * (N + 1)), ffi.c_fp(at + 8 * (N + 1)), ffi.c_fp(at + 8 * (N + 1) + 4 * N),
            most, ffi.c_fp(base), ffi.c_fp(base + 8 * F), float(epsilon), float(missing), int(skip_average), rows,
            ffi.ptr(out) if rows else None, ffi.stream()), "pa_aggregate_files")
    if packed:
        return out, out_frames
    return [out[a:a + t] for a, t in zip(row0[:-1].tolist(), T.tolist())], out_frames


def binarize_regions_files(scores: torch.Tensor, row0, T, frames: SlidingWindow, onset, offset, min_duration_on=0.0,
                           min_duration_off=0.0, return_tracks: bool = False):
    """`binarize_regions` of every file of a packed aggregate at once (`pa_binarize_regions_files_count` / `_emit`,
    csrc/regions_files.hip).  scores: the (row0[-1], K) float32 device tensor `aggregate_files(..., packed=True)`
    returns; row0, T: as `files_layout` returns them; one set of per-class parameters for all files (scalars are
    shared).  -> per file the list of K float64 arrays (n, 2) `binarize_regions` returns for the file's rows alone
    (times from the file's own frame 0), bit for bit; with `return_tracks`, also per file the K arrays of track
    positions.  The whole group crosses to the host in one copy of the packed rows and one of the offset table."""
    if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dim() == 2
            and scores.dtype == torch.float32):
        raise ValueError("binarize_regions_files expects a (rows, classes) float32 device tensor")
    x = scores.contiguous()
    rows, K = x.shape
    row0, T = _files_tables(row0, T, "binarize_regions_files")
    N = len(T)
    if int(row0[-1]) != rows:
        raise ValueError(f"binarize_regions_files: the files own {int(row0[-1])} rows, the scores have {rows}")
    if not 1 <= K <= 16:
        raise ValueError(f"binarize_regions_files: {K} classes, 1..16 supported")

    def per_class(v, dtype):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (K,)))

    on, off = per_class(onset, np.float32), per_class(offset, np.float32)
    d_on, d_off = per_class(min_duration_on, np.float64), per_class(min_duration_off, np.float64)
    if np.isnan(on).any() or np.isnan(off).any() or np.isnan(d_on).any() or np.isnan(d_off).any():
        raise ValueError("binarize_regions_files: a threshold or a duration is NaN")
    lib = ffi.load()
    dev = x.device
    with torch.cuda.device(dev):
        n_raw = np.zeros(K, dtype=np.int32)
        nbytes = int(lib.pa_binarize_regions_files_workspace_bytes(rows, K, N, 0))
        workspace = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
        ffi.check(lib.pa_binarize_regions_files_count(
            ffi.ptr(x) if rows else None, K, N, row0.ctypes.data, T.ctypes.data, on.ctypes.data, off.ctypes.data,
            n_raw.ctypes.data, ffi.ptr(workspace), nbytes, ffi.stream()), "pa_binarize_regions_files_count")
        raw_rows = int(n_raw.sum(dtype=np.int64))
        regions = torch.empty((raw_rows, 2), dtype=torch.float64, device=dev)
        tracks = torch.empty(raw_rows, dtype=torch.int32, device=dev) if return_tracks else None
        list_off = torch.empty(N * K + 1, dtype=torch.int32, device=dev)
        nbytes = int(lib.pa_binarize_regions_files_workspace_bytes(rows, K, N, raw_rows))
        if workspace.numel() < nbytes:
            workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ffi.check(lib.pa_binarize_regions_files_emit(
            ffi.ptr(x) if rows else None, K, N, row0.ctypes.data, T.ctypes.data, on.ctypes.data, off.ctypes.data,
            d_on.ctypes.data, d_off.ctypes.data, float(frames.start), float(frames.duration), float(frames.step),
            n_raw.ctypes.data, raw_rows, ffi.ptr(regions) if raw_rows else None,
            ffi.ptr(tracks) if raw_rows and return_tracks else None, ffi.ptr(list_off), ffi.ptr(workspace), nbytes,
            ffi.stream()), "pa_binarize_regions_files_emit")
        offsets = list_off.cpu().numpy().astype(np.int64)
        total = int(offsets[-1])
        # one copy of the packed rows; the track positions ride along as a third float64 column (exact: they are
        # small integers)
        if return_tracks:
            both = torch.cat([regions[:total], tracks[:total].to(torch.float64)[:, None]], dim=1).cpu().numpy()
            host, host_tracks = np.ascontiguousarray(both[:, :2]), both[:, 2].astype(np.int32)
        else:
            host = regions[:total].cpu().numpy()
    out = [[host[offsets[f * K + k]:offsets[f * K + k + 1]] for k in range(K)] for f in range(N)]
    if not return_tracks:
        return out
    return out, [[host_tracks[offsets[f * K + k]:offsets[f * K + k + 1]] for k in range(K)] for f in range(N)]


#: default budget of `binarize_regions_sweep`'s device workspace (event words, chunk tables and row buffers)
SWEEP_WORKSPACE_BYTES = 1 << 30
_SEGMENT_PRECISION = 1e-6


def _sweep_tables(K, lane_class, onset, offset, job_lane, min_duration_on, min_duration_off):
    """the host arrays of a sweep, checked as the kernel's entry points check them"""
    lane_class = np.ascontiguousarray(lane_class, dtype=np.int32).reshape(-1)
    L = len(lane_class)
    on = np.ascontiguousarray(np.broadcast_to(np.asarray(onset, dtype=np.float32), (L,)))
    off = np.ascontiguousarray(np.broadcast_to(np.asarray(offset, dtype=np.float32), (L,)))
    job_lane = np.ascontiguousarray(job_lane, dtype=np.int32).reshape(-1)
    M = len(job_lane)
    d_on = np.ascontiguousarray(np.broadcast_to(np.asarray(min_duration_on, dtype=np.float64), (M,)))
    d_off = np.ascontiguousarray(np.broadcast_to(np.asarray(min_duration_off, dtype=np.float64), (M,)))
    if not 1 <= K <= 16:
        raise ValueError(f"binarize_regions_sweep: {K} classes, 1..16 supported")
    if L and (lane_class.min() < 0 or lane_class.max() >= K):
        raise ValueError(f"binarize_regions_sweep: a lane names a class outside 0..{K - 1}")
    if M and (job_lane.min() < 0 or job_lane.max() >= L):
        raise ValueError(f"binarize_regions_sweep: a job names a lane outside 0..{L - 1}")
    if np.isnan(on).any() or np.isnan(off).any() or np.isnan(d_on).any() or np.isnan(d_off).any():
        raise ValueError("binarize_regions_sweep: a threshold or a duration is NaN")
    return lane_class, on, off, job_lane, d_on, d_off


def _lane_regions_host(y: np.ndarray, frames: SlidingWindow, onset: np.float32, offset: np.float32) -> np.ndarray:
    """one lane on the host: the regions of column `y` before merging, empty ones dropped -> (n, 2) float64.
    Every frame is one of four maps of the state (keep, set, clear, swap): the state is the value of the last set /
    clear frame, flipped once per swap since."""
    T = len(y)
    if T < 2:
        return np.zeros((0, 2))
    with np.errstate(invalid="ignore"):
        above, below = y > onset, y < offset                 # float32 comparisons; NaN: both false
    turn_on, turn_off = above & ~below, below & ~above
    swap = above & below
    turn_on[0], turn_off[0], swap[0] = above[0], not above[0], False      # frame 0 sets the state
    idx = np.arange(T)
    last = np.maximum.accumulate(np.where(turn_on | turn_off, idx, 0))
    flips = np.cumsum(swap)
    active = turn_on[last] ^ (((flips - flips[last]) & 1) == 1)
    before = np.concatenate([[False], active[:-1]])
    opens = np.flatnonzero(active & ~before)
    closes = np.flatnonzero(~active & before)
    if active[-1]:
        closes = np.append(closes, T - 1)

    def middle(i):
        s = float(frames.start) + i.astype(np.float64) * float(frames.step)
        return 0.5 * (s + (s + float(frames.duration)))

    rows = np.stack([middle(opens), middle(closes)], axis=1)
    return rows[(rows[:, 1] - rows[:, 0]) > _SEGMENT_PRECISION]


def _job_regions_host(rows: np.ndarray, min_duration_on: float, min_duration_off: float):
    """`Annotation.support(min_duration_off)` and the min_duration_on removal on a lane's rows -> rows, positions"""
    positions = np.zeros(len(rows), dtype=np.int32)
    if min_duration_off > 0.0 and len(rows):
        gap = rows[1:, 0] - rows[:-1, 1]
        gap = np.where(gap > _SEGMENT_PRECISION, gap, 0.0)
        head = np.concatenate([[True], ~(gap < min_duration_off)])
        tail = np.concatenate([head[1:], [True]])
        rows = np.stack([rows[head, 0], rows[tail, 1]], axis=1)
        positions = np.arange(len(rows), dtype=np.int32)
    if min_duration_on > 0.0 and len(rows):
        length = rows[:, 1] - rows[:, 0]
        keep = ~(np.where(length > _SEGMENT_PRECISION, length, 0.0) < min_duration_on)
        rows, positions = rows[keep], positions[keep]
    return rows, positions


def _sweep_host(scores: np.ndarray, frames, lane_class, on, off, job_lane, d_on, d_off):
    lanes = {}
    rows, tracks = [], []
    for lane, a, b in zip(job_lane.tolist(), d_on.tolist(), d_off.tolist()):
        if lane not in lanes:                # the hysteresis of a lane runs once, however many jobs read it
            lanes[lane] = _lane_regions_host(scores[:, lane_class[lane]], frames, on[lane], off[lane])
        r, t = _job_regions_host(lanes[lane], a, b)
        rows.append(r)
        tracks.append(t)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    packed = np.concatenate(rows) if rows else np.zeros((0, 2))
    packed_tracks = np.concatenate(tracks) if tracks else np.zeros(0, dtype=np.int32)
    return np.ascontiguousarray(packed, dtype=np.float64).reshape(-1, 2), packed_tracks.astype(np.int32), offsets


def _sweep_workspace(lib, x, groups, L, M, raw_rows, job_rows, budget):
    """the fixed part and as many groups' event words and chunk tables as the budget holds (at least one group's)"""
    T = x.shape[0]
    fixed = int(lib.pa_regions_sweep_workspace_bytes(T, groups, 0, L, M, raw_rows, job_rows))
    each = int(lib.pa_regions_sweep_workspace_bytes(T, groups, 1, L, M, raw_rows, job_rows)) - fixed
    nbytes = fixed + max(1, min(groups, budget // max(each, 1))) * each
    return torch.empty(nbytes, dtype=torch.uint8, device=x.device), nbytes


def _sweep_count(x, lane_class, on, off, budget, stats) -> np.ndarray:
    """the counting phase: regions of every lane before any clean-up (one read-back)"""
    lib = ffi.load()
    T, K = x.shape
    L = len(lane_class)
    n_raw = np.zeros(L, dtype=np.int32)
    if T < 2 or L == 0:
        return n_raw
    groups = int(lib.pa_regions_sweep_groups(K, L, lane_class.ctypes.data))
    launches = np.zeros(1, dtype=np.int32)
    ws, nbytes = _sweep_workspace(lib, x, groups, L, 0, 0, 0, budget)
    ffi.check(lib.pa_regions_sweep_count(ffi.ptr(x), T, K, L, lane_class.ctypes.data, on.ctypes.data,
                                         off.ctypes.data, n_raw.ctypes.data, launches.ctypes.data, ffi.ptr(ws),
                                         nbytes, ffi.stream()), "pa_regions_sweep_count")
    stats["count_launches"] += int(launches[0])
    return n_raw


def _sweep_emit(x, frames, lane_class, on, off, n_raw, job_lane, d_on, d_off, want_tracks, budget, stats):
    """the emitting phase for some lanes and their jobs -> device rows, tracks, host job counts"""
    lib = ffi.load()
    T, K = x.shape
    dev = x.device
    L, M = len(lane_class), len(job_lane)
    n_raw = np.ascontiguousarray(n_raw, dtype=np.int32)
    raw_rows = int(n_raw.sum(dtype=np.int64))
    rows = int(n_raw[job_lane].sum(dtype=np.int64))
    regions = torch.empty((rows, 2), dtype=torch.float64, device=dev)
    tracks = torch.empty(rows, dtype=torch.int32, device=dev) if want_tracks else None
    job_off = torch.empty(M + 1, dtype=torch.int32, device=dev)
    launches = np.zeros(1, dtype=np.int32)
    ws, nbytes = None, 0
    if T >= 2 and L and M:
        groups = int(lib.pa_regions_sweep_groups(K, L, lane_class.ctypes.data))
        ws, nbytes = _sweep_workspace(lib, x, groups, L, M, raw_rows, rows, budget)
    ffi.check(lib.pa_regions_sweep_emit(
        ffi.ptr(x) if x.numel() else None, T, K, L, lane_class.ctypes.data, on.ctypes.data, off.ctypes.data,
        n_raw.ctypes.data, M, job_lane.ctypes.data, d_on.ctypes.data, d_off.ctypes.data, float(frames.start),
        float(frames.duration), float(frames.step), rows, ffi.ptr(regions) if rows else None,
        ffi.ptr(tracks) if rows and want_tracks else None, ffi.ptr(job_off), launches.ctypes.data, ffi.ptr(ws), nbytes,
        ffi.stream()), "pa_regions_sweep_emit")
    stats["emit_launches"] += int(launches[0])
    stats["calls"] += 1
    offsets = job_off.cpu().numpy().astype(np.int64)
    total = int(offsets[-1])
    return regions[:total], (tracks[:total] if want_tracks else None), np.diff(offsets)


def binarize_regions_sweep(scores, frames: SlidingWindow, lane_class, onset, offset, job_lane, min_duration_on=0.0,
                           min_duration_off=0.0, return_tracks: bool = False, to_host: bool = True,
                           workspace_bytes: int = SWEEP_WORKSPACE_BYTES, stats: Optional[dict] = None):
    """The region lists of many detectors on one aggregated (T, K) float32 score array (`pa_regions_sweep_count` /
    `pa_regions_sweep_emit`, csrc/regions_sweep.hip).  A lane is (class, onset, offset) -- float32 thresholds, scalars
    are shared --, a job is (lane, min_duration_on, min_duration_off); job j's rows are bit for bit what
    `binarize_regions` returns for column `lane_class[job_lane[j]]` with the job's four parameters.

    `to_host=True`: a list of M (n_j, 2) float64 arrays (and, with `return_tracks`, M int32 arrays of track
    positions).  `to_host=False`: (rows (N, 2) float64, tracks (N,) int32 or None, offsets (M + 1,) int64 numpy):
    the packed rows stay on the scores' device, job j owns rows offsets[j]:offsets[j + 1].

    `workspace_bytes` bounds the device scratch: lane groups are split over several launch sequences, and lanes over
    several calls, when the event words (4 T bytes per group of 16 lanes) or the row buffers exceed it; results do
    not depend on the split.  `stats`, when given, receives the number of launch sequences and calls.

    Scores on the CPU (tensor or array) go through a numpy form of the same rule."""
    on_gpu = isinstance(scores, torch.Tensor) and scores.is_cuda
    if isinstance(scores, torch.Tensor):
        if scores.dim() != 2 or scores.dtype != torch.float32:
            raise ValueError("binarize_regions_sweep expects a (frames, classes) float32 array")
        x = scores.contiguous() if on_gpu else scores.numpy()
    else:
        x = np.asarray(scores)
        if x.ndim != 2 or x.dtype != np.float32:
            raise ValueError("binarize_regions_sweep expects a (frames, classes) float32 array")
    T, K = x.shape
    lane_class, on, off, job_lane, d_on, d_off = _sweep_tables(K, lane_class, onset, offset, job_lane,
                                                               min_duration_on, min_duration_off)
    L, M = len(lane_class), len(job_lane)
    stats = stats if stats is not None else {}
    stats.update({"count_launches": 0, "emit_launches": 0, "calls": 0})
    if not on_gpu:
        rows, tracks, offsets = _sweep_host(x, frames, lane_class, on, off, job_lane, d_on, d_off)
        if not to_host:
            return torch.from_numpy(rows), (torch.from_numpy(tracks) if return_tracks else None), offsets
    else:
        with torch.cuda.device(x.device):
            budget = int(workspace_bytes)
            n_raw = _sweep_count(x, lane_class, on, off, budget, stats)
            # lanes are taken in order, as many per call as keep the row buffers (raw and cleaned rows of the lane,
            # merged rows and output rows of each of its jobs: 16 bytes a row) under the budget
            per_lane = 16 * n_raw.astype(np.int64) * (2 + 2 * np.bincount(job_lane, minlength=L)[:L])
            parts, lo = [], 0
            while lo < L or not parts:
                hi, used = lo, 0
                while hi < L and (hi == lo or used + per_lane[hi] <= budget):
                    used += per_lane[hi]
                    hi += 1
                picked = np.flatnonzero((job_lane >= lo) & (job_lane < hi))
                r, t, n = _sweep_emit(x, frames, lane_class[lo:hi], on[lo:hi], off[lo:hi], n_raw[lo:hi],
                                      np.ascontiguousarray(job_lane[picked] - lo), d_on[picked], d_off[picked],
                                      return_tracks, budget, stats)
                parts.append((picked, r, t, n))
                lo = max(hi, lo + 1)
            counts = np.zeros(M, dtype=np.int64)
            for picked, _, _, n in parts:
                counts[picked] = n
            offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            if len(parts) == 1 and np.array_equal(parts[0][0], np.arange(M)):
                rows, tracks = parts[0][1], parts[0][2]
            else:       # back into job order: where every row of the calls' outputs goes
                where = np.concatenate([np.concatenate([np.arange(offsets[j], offsets[j + 1]) for j in picked] or
                                                       [np.zeros(0, dtype=np.int64)]) for picked, _, _, _ in parts])
                order = torch.from_numpy(np.argsort(where, kind="stable")).to(x.device)
                rows = torch.cat([r for _, r, _, _ in parts])[order]
                tracks = torch.cat([t for _, _, t, _ in parts])[order] if return_tracks else None
        if not to_host:
            return rows, tracks, offsets
        rows = rows.cpu().numpy()
        tracks = tracks.cpu().numpy() if return_tracks else None
    out = [rows[offsets[j]:offsets[j + 1]] for j in range(M)]
    if not return_tracks:
        return out
    return out, [tracks[offsets[j]:offsets[j + 1]] for j in range(M)]


@ffi.on_device(lambda scores, *a, **k: scores.device)
def binarize(scores: torch.Tensor, onset: float = 0.5, offset: float | None = None,
             initial_state: bool | None = None) -> torch.Tensor:
    """`binarize` (utils/signal.py:78-204) on the device: (C, F, K) float32 scores -> (C, F, K) uint8 by
    hysteresis thresholding per (chunk, class); what SpeakerDiarization.apply does to the segmentations of a
    non-powerset model (pipelines/speaker_diarization.py:599-606)."""
    offset = offset or onset
    x = scores.to(torch.float32).contiguous()
    C, F, K = x.shape
    out = torch.empty((C, F, K), dtype=torch.uint8, device=x.device)
    init = -1 if initial_state is None else int(bool(initial_state))
    # the reference compares the float32 scores of frame 0 with 0.5 * (onset + offset), a Python float that numpy
    # rounds once to float32 (utils/signal.py:111); the same product of the float32 thresholds can be one ulp off
    midpoint = float(np.float32(0.5 * (float(onset) + float(offset))))
    ffi.check(ffi.load().pa_binarize_hysteresis(ffi.ptr(x), C, F, K, float(onset), float(offset), midpoint, init,
                                                ffi.ptr(out), ffi.stream()), "pa_binarize_hysteresis")
    return out


class Reconstructor:
    """speaker_diarization.py:480-528 + diarization.py:221-268: cluster activations are accumulated
    once, then discretised for any per-frame cap (regular and exclusive diarization share them)."""

    @ffi.on_device(lambda self, seg, *a, **k: seg.device)
    def __init__(self, seg: torch.Tensor, chunks: SlidingWindow, frames: SlidingWindow,
                 hard_clusters: np.ndarray, count: np.ndarray):
        """`seg`: (C, F, S) uint8 hard segmentations (powerset models: sums of small integers), or float32
        soft scores (non-powerset models: the reference reconstructs from the RAW segmentations,
        speaker_diarization.py:687-691, so activations are float32 overlap-add sums of sigmoid scores)."""
        C, F, S = seg.shape
        self.soft = seg.dtype != torch.uint8
        dev = seg.device
        starts, T, self.frames = frame_geometry(chunks, frames, C)
        count = np.ascontiguousarray(count.reshape(-1))
        if len(count) != T:
            raise ValueError(f"count has {len(count)} frames, the chunks cover {T}")
        num_clusters = int(np.max(hard_clusters)) + 1
        # to_diarization pads the cluster axis up to max(count) (diarization.py:250-256)
        self.K = max(num_clusters, int(np.max(count)) if len(count) else 0, 1)
        self.T = T
        self.count = torch.from_numpy(count.astype(np.uint8)).to(dev)
        hard = torch.from_numpy(np.ascontiguousarray(hard_clusters, dtype=np.int32)).to(dev)
        st = torch.from_numpy(starts).to(dev)
        if self.soft:
            lib = ffi.load()
            clustered = torch.empty((C, F, self.K), dtype=torch.float32, device=dev)
            ffi.check(lib.pa_cluster_max(ffi.ptr(seg.contiguous()), C, F, S, ffi.ptr(hard), self.K,
                                         ffi.ptr(clustered), ffi.stream()), "pa_cluster_max")
            ones = torch.ones(F, dtype=torch.float64, device=dev)
            self.act = torch.empty((T, self.K), dtype=torch.float32, device=dev)
            # aggregate(hamming=False, missing=0, skip_average=True) (diarization.py:243-249)
            ffi.check(lib.pa_aggregate(ffi.ptr(clustered), C, F, self.K, ffi.ptr(st), T, ffi.ptr(ones),
                                       ffi.ptr(ones), 1e-12, 0.0, 1, ffi.ptr(self.act), ffi.stream()),
                      "pa_aggregate")
            return
        self.act = torch.empty((T, self.K), dtype=torch.int32, device=dev)
        ffi.check(ffi.load().pa_cluster_activations(ffi.ptr(seg), C, F, S, ffi.ptr(st), ffi.ptr(hard),
                                                    self.K, T, ffi.ptr(self.act), ffi.stream()),
                  "pa_cluster_activations")

    @ffi.on_device(lambda self, *a, **k: self.act.device)
    def discretize(self, cap: int = 255) -> SlidingWindowFeature:
        """Top-min(count[t], cap) clusters per frame.  Frames whose selection boundary falls inside a
        group of EQUAL activations are re-decided with `np.argsort(-activations)` -- the reference's
        own call (diarization.py:261), whose order among equals depends on the host's numpy build
        (SIMD sorting networks) -- so the output equals the reference's on this host, not merely up
        to ties.  Every other frame is decided on the GPU."""
        dev = self.act.device
        out = torch.empty((self.T, self.K), dtype=torch.uint8, device=dev)
        tie = torch.empty(self.T, dtype=torch.uint8, device=dev)
        topk = ffi.load().pa_topk_binarize_f32 if self.soft else ffi.load().pa_topk_binarize
        ffi.check(topk(ffi.ptr(self.act), ffi.ptr(self.count), self.T, self.K, int(cap), ffi.ptr(out),
                       ffi.ptr(tie), ffi.stream()), "pa_topk_binarize")
        idx = torch.nonzero(tie).view(-1)
        binary = out.cpu().numpy().astype(np.float32)
        if idx.numel():
            rows = idx.cpu().numpy()
            act = self.act[idx].cpu().numpy().astype(np.float32)
            n = np.minimum(np.minimum(self.count[idx].cpu().numpy().astype(np.int64), cap), self.K)
            order = np.argsort(-act, axis=-1)
            keep = np.arange(self.K)[None, :] < n[:, None]
            fixed = np.zeros_like(act)
            fixed[np.nonzero(keep)[0], order[keep]] = 1.0
            binary[rows] = fixed
        self.num_tie_frames = int(idx.numel())
        return SlidingWindowFeature(binary, self.frames)
