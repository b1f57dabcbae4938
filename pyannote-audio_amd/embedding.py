"""Device-side WeSpeaker ResNet34 embedding extractor over `pa_emb_forward`
(mirrors models/embedding/wespeaker/__init__.py:324-343 and the b3 interface of SURVEY.md 8b)."""
from __future__ import annotations

import os
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from . import ffi
from .weights import EmbeddingPack, XVectorMFCCPack, XVectorPack


class EmbeddingEngine:
    """fbank -> ResNet34 -> weighted statistics pooling -> Linear over strided chunks of a
    device-resident waveform.  The backbone runs once per chunk; all S masks are pooled from it."""

    def __init__(self, pack: EmbeddingPack, max_chunks: Optional[int] = None):
        self.pack = pack
        # chunks per launch group: ~31 MB of activations per 10 s chunk -> 62 GB at 2 048 of the 288 GB.  Measured
        # per audio-hour (profiles/r3_emb_batch_sweep.txt): 64 -> 1 131 ms, 128 -> 1 068, 256 -> 1 039,
        # 512 -> 1 023 / 1 013 (split evenly), 1 024 -> 1 007, 2 048 -> 1 001, the whole file in one group (111 GB)
        # -> 1 000: every launch pays a pipeline fill and a tail, so fewer and longer launches win (Winograd
        # kernel 0.55 -> 0.62 of peak); groups sized to the 256-MiB Infinity Cache (8 chunks, so that a convolution
        # would read its predecessor's output on-die) are far on the wrong side of that trade.  The chunks of a
        # file are split EVENLY over the groups (3 591 = 2 x 1 796).
        # Round 6: the limit is a WORKSPACE SIZE, not a chunk count -- all 10 000 segments of 3 s in one group:
        # BASELINE.json configs[2] 16 001 -> 16 529 segments/s (2 048 per group: 115 launches of the F(4x4) kernel; 3 334:
        # 69, 16 195; 5 000: 46, 16 419; 10 000: 23 launches).  First 96 GB (a one-hour file = 2 x 1 796 chunks), then 128 GB:
        # the 3 591 chunks of a one-hour file in ONE group (111 GB) measured 757.1 / 757.6 ms per file against 760.6 / 765.6
        # as two groups and 766.6 / 769.9 as three (A/B pairs in one call, profiles/r6_emb_group_ab.txt).
        # `max_chunks` / PA_EMB_BATCH (a chunk count) overrides it.
        env = os.environ.get("PA_EMB_BATCH")
        self.max_chunks = max_chunks or (int(env) if env else None)
        self._ws = None
        self._idx_cache: dict = {}

    # share of the device's FREE memory one launch group's workspace may take (several pipelines / processes on one
    # GPU, or a smaller device, must not run out where the 2 048-chunk default asks for ~62 GB)
    MAX_FREE_FRACTION = 0.5
    #: workspace of one launch group when no chunk count is given (bytes)
    GROUP_WORKSPACE_BYTES = 128 << 30

    def _group_size(self, num_chunks: int, num_samples: int, S: int) -> int:
        """chunks per launch group: `max_chunks` (or as many as GROUP_WORKSPACE_BYTES hold), the file split EVENLY over
        the groups, and halved until the workspace fits MAX_FREE_FRACTION of what is free right now (a cached workspace
        counts as free)."""
        lib = ffi.load()
        limit = self.max_chunks
        if limit is None:
            # (the workspace is linear in the chunk count up to alignment: measured on 64 chunks)
            per_chunk = lib.pa_emb_workspace_bytes(self.pack.struct, 64, num_samples, S) / 64.0
            limit = max(8, int(self.GROUP_WORKSPACE_BYTES / max(per_chunk, 1.0)))
        groups = -(-num_chunks // limit)
        per_group = -(-num_chunks // groups)
        free, _ = torch.cuda.mem_get_info(self.pack.device)
        # + what torch's caching allocator holds without using it, + this engine's own cached workspace
        free += torch.cuda.memory_reserved(self.pack.device) - torch.cuda.memory_allocated(self.pack.device)
        free += self._ws.numel() if self._ws is not None else 0
        while per_group > 8 and lib.pa_emb_workspace_bytes(self.pack.struct, per_group, num_samples, S) > \
                self.MAX_FREE_FRACTION * free:
            groups *= 2
            per_group = -(-num_chunks // groups)
        return per_group

    def _workspace(self, nbytes: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.pack.device)
        return self._ws

    def release_workspace(self):
        self._ws = None

    def num_pool_frames(self, num_samples: int) -> int:
        return ffi.load().pa_emb_num_pool_frames(self.pack.struct, num_samples)

    def nearest_index(self, mask_frames: int, pool_frames: int) -> torch.Tensor:
        """source index of F.interpolate(mode="nearest") (blocks/pooling.py:113-117): obtained by
        running torch's own op on an index ramp, so it is exactly what the reference does."""
        key = (mask_frames, pool_frames)
        if key not in self._idx_cache:
            ramp = torch.arange(mask_frames, dtype=torch.float32).view(1, 1, -1)
            idx = F.interpolate(ramp, size=pool_frames, mode="nearest").view(-1).to(torch.int32)
            self._idx_cache[key] = idx.to(self.pack.device)
        return self._idx_cache[key]

    @ffi.on_device(lambda self, *a, **k: self.pack.device)
    def forward_strided(self, wav: torch.Tensor, chunk_stride: int, num_chunks: int, num_samples: int,
                        masks: torch.Tensor | None = None) -> torch.Tensor:
        """wav: 1-D fp32 device tensor; masks: (C, S, Fm) fp32 device or None -> (C, S, D) fp32."""
        lib = ffi.load()
        w = self.pack.struct
        dev = self.pack.device
        if num_samples < 400:
            raise ValueError("chunk shorter than one fbank frame (400 samples)")
        S = 1 if masks is None else masks.shape[1]
        Fm = 0 if masks is None else masks.shape[2]
        Tp = self.num_pool_frames(num_samples)
        idx = self.nearest_index(Fm, Tp) if masks is not None else None
        if masks is not None:
            masks = masks.to(dev, torch.float32).contiguous()
        emb = torch.empty((num_chunks, S, w.embed_dim), dtype=torch.float32, device=dev)
        c0 = 0
        per_group = self._group_size(num_chunks, num_samples, S)
        while c0 < num_chunks:
            nb = min(per_group, num_chunks - c0)
            ws = self._workspace(lib.pa_emb_workspace_bytes(w, nb, num_samples, S))
            off = c0 * chunk_stride
            sub = wav[off:]
            rc = lib.pa_emb_forward(
                w, ffi.c_fp(sub.data_ptr()), sub.numel(), chunk_stride, nb, num_samples,
                ffi.ptr(masks[c0:c0 + nb]) if masks is not None else None, S, Fm,
                ffi.ptr(idx) if idx is not None else None, ffi.ptr(emb[c0:c0 + nb]),
                ffi.ptr(ws), ws.numel(), ffi.stream())
            ffi.check(rc, "pa_emb_forward")
            c0 += nb
        return emb

    #: most pool frames `pa_stats_pool` (and so `forward_strided`) takes; longer single-weight inputs go through the
    #: ragged pooling, which has no such limit
    POOL_MAX_FRAMES = 512
    #: longest / shortest utterance of one ragged bucket (the padding stays below 1 - 1 / RAGGED_RATIO of the samples)
    RAGGED_RATIO = 1.10
    #: utterances per ragged launch group at most (the grids carry the batch in their y / z dimension)
    RAGGED_MAX_GROUP = 16384
    #: whether the front end reads samples past the end of the waveform as zeros (k_fbank does): the orphan chunk
    #: of a sliding window is then the reference's zero-padded chunk without a copy
    READS_PAST_END_AS_ZERO = True

    def forward(self, waveforms: torch.Tensor, weights: torch.Tensor | None = None) -> torch.Tensor:
        """(B,1,N) [, (B,Fm) or (B,S,Fm)] -> (B,D) or (B,S,D): the reference forward contract."""
        B, ch, N = waveforms.shape
        assert ch == 1
        x = waveforms.to(self.pack.device, torch.float32).contiguous().view(-1)
        if self._ragged_supported() and N >= 400 and self.num_pool_frames(N) > self.POOL_MAX_FRAMES and \
                (weights is None or weights.dim() == 2):
            # long inputs (whole files): the ragged path with equal lengths, whose pooling takes any length
            masks = None if weights is None else [m for m in weights.to(self.pack.device, torch.float32)]
            return self.forward_ragged(x, [i * N for i in range(B)], [N] * B, masks)
        squeeze = weights is None or weights.dim() == 2
        m = None
        if weights is not None:
            m = weights.unsqueeze(1) if weights.dim() == 2 else weights
        emb = self.forward_strided(x, N, B, N, m)
        return emb[:, 0] if squeeze else emb


    # ------------------------------------------------------------------------------ ragged batches
    def _ragged_supported(self) -> bool:
        """`pa_emb_forward_ragged` covers global fbank centring; fbank_centering_span checkpoints fall back"""
        return self.pack.struct.fb_center_kernel == 0

    def pool_weights(self, mask: torch.Tensor, num_samples: int) -> torch.Tensor:
        """weights of any frame rate -> the pool frames of `num_samples`, by torch's own nearest mapping"""
        mask = mask.to(self.pack.device, torch.float32).reshape(-1)
        return mask[self.nearest_index(mask.numel(), self.num_pool_frames(num_samples)).long()]

    @ffi.on_device(lambda self, *a, **k: self.pack.device)
    def forward_ragged(self, wav: torch.Tensor, offsets: Sequence[int], lengths: Sequence[int],
                       masks: Optional[Sequence[Optional[torch.Tensor]]] = None) -> torch.Tensor:
        """Utterances of different lengths in one pass: utterance b = wav[offsets[b] : offsets[b] + lengths[b]] of a
        1-D fp32 device waveform; masks: None, or one 1-D weight tensor (any frame rate, mapped to the pool frames
        like F.interpolate(mode="nearest")) or None per utterance.  -> (B, D), in input order; row b equals the
        embedding of utterance b on its own.

        The utterances are sorted by length and bucketed so that within a bucket the longest is at most RAGGED_RATIO
        times the shortest; each bucket runs as launch groups of `_group_size` at its longest length."""
        offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
        lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        B = lengths.size
        if offsets.size != B or (masks is not None and len(masks) != B):
            raise ValueError("offsets, lengths (and masks) must have one entry per utterance")
        self._check_lengths(lengths)
        if B and (offsets.min() < 0 or (offsets + lengths).max() > wav.numel()):
            raise ValueError("an utterance reaches outside the waveform")
        pooled = None
        if masks is not None:
            pooled = [None if m is None else self.pool_weights(m, int(n)) for m, n in zip(masks, lengths)]
        if not self._ragged_supported():
            return self._forward_by_length(wav, offsets, lengths, pooled)
        lib = ffi.load()
        w = self.pack.struct
        dev = self.pack.device
        order = np.argsort(lengths, kind="stable")
        out_sorted = torch.empty((B, self.embed_dim), dtype=torch.float32, device=dev)
        for b0, b1 in length_buckets(lengths[order], self.RAGGED_RATIO):
            n_max = int(lengths[order[b1 - 1]])
            per_group = min(self._group_size(b1 - b0, n_max, 1), self.RAGGED_MAX_GROUP)
            groups = -(-(b1 - b0) // per_group)
            per_group = -(-(b1 - b0) // groups)          # split evenly
            for g0 in range(b0, b1, per_group):
                g1 = min(g0 + per_group, b1)
                sel = order[g0:g1]
                n_max = int(lengths[sel].max())
                off_d = torch.from_numpy(offsets[sel].copy()).to(dev)
                len_d = torch.from_numpy(lengths[sel].astype(np.int32)).to(dev)
                m = None
                if pooled is not None:
                    m = torch.ones((g1 - g0, self.num_pool_frames(n_max)), dtype=torch.float32, device=dev)
                    for j, i in enumerate(sel):
                        if pooled[i] is not None:
                            m[j, :pooled[i].numel()] = pooled[i]
                ws = self._workspace(lib.pa_emb_ragged_workspace_bytes(w, g1 - g0, n_max))
                rc = lib.pa_emb_forward_ragged(
                    w, ffi.c_fp(wav.data_ptr()), wav.numel(), ffi.ptr(off_d), ffi.ptr(len_d), g1 - g0, n_max,
                    ffi.ptr(m) if m is not None else None, ffi.ptr(out_sorted[g0:g1]), ffi.ptr(ws), ws.numel(),
                    ffi.stream())
                ffi.check(rc, "pa_emb_forward_ragged")
        out = torch.empty_like(out_sorted)
        out[torch.from_numpy(order).to(dev)] = out_sorted
        return out

    @property
    def embed_dim(self) -> int:
        return self.pack.struct.embed_dim

    @staticmethod
    def _check_lengths(lengths: np.ndarray, minimum: int = 400):
        short = np.flatnonzero(lengths < minimum)
        if short.size:
            i = int(short[0])
            raise ValueError(f"utterance {i} has {int(lengths[i])} samples: shorter than one fbank frame "
                             f"({minimum} samples)")

    def _forward_by_length(self, wav: torch.Tensor, offsets: np.ndarray, lengths: np.ndarray,
                           pooled: Optional[list]) -> torch.Tensor:
        """fallback of `forward_ragged`: one `forward_strided` launch sequence per distinct length, the utterances
        of that length gathered contiguously, their weights already at pool resolution (identity index)"""
        dev = self.pack.device
        out = torch.empty((lengths.size, self.embed_dim), dtype=torch.float32, device=dev)
        for n in np.unique(lengths):
            n = int(n)
            sel = np.flatnonzero(lengths == n)
            buf = torch.cat([wav[int(offsets[i]):int(offsets[i]) + n] for i in sel])
            m = None
            if pooled is not None:
                tp = self.num_pool_frames(n)
                m = torch.stack([torch.ones(tp, device=dev) if pooled[i] is None else pooled[i] for i in sel])[:, None]
            emb = self.forward_strided(buf, n, sel.size, n, m)
            out[torch.from_numpy(sel).to(dev)] = emb[:, 0]
        return out


def length_buckets(sorted_lengths: Sequence[int], ratio: float = EmbeddingEngine.RAGGED_RATIO) -> list:
    """[(begin, end)) ranges of ascending lengths in which the longest is at most `ratio` x the shortest"""
    L = np.asarray(sorted_lengths)
    buckets, b0 = [], 0
    while b0 < L.size:
        b1 = int(np.searchsorted(L, ratio * L[b0], side="right"))
        b1 = max(b1, b0 + 1)
        buckets.append((b0, b1))
        b0 = b1
    return buckets


class XVectorEngine(EmbeddingEngine):
    """XVectorSincNet (models/embedding/xvector.py:205-349) over `pa_xvec_forward`: SincNet -> 5 TDNN layers
    -> weighted statistics pooling -> Linear; same strided-chunk / all-masks-at-once interface."""

    def __init__(self, pack: XVectorPack, max_chunks: Optional[int] = None):
        self.pack = pack
        self.max_chunks = max_chunks or 512      # ~5.3 MB of activations per 10 s chunk
        self._ws = None
        self._idx_cache = {}

    READS_PAST_END_AS_ZERO = False    # pa_row_stats normalises over the samples present only
    #: prefix of the C entry points (_num_frames, _workspace_bytes, _forward) and the front end's name in messages
    _ABI, _FRONT = "pa_xvec", "SincNet"

    def num_pool_frames(self, num_samples: int) -> int:
        return getattr(ffi.load(), self._ABI + "_num_frames")(self.pack.struct, num_samples)

    def _ragged_supported(self) -> bool:
        return False        # InstanceNorm layers are per utterance: one launch sequence per length

    @property
    def embed_dim(self) -> int:
        return self.pack.struct.dimension

    def _check_lengths(self, lengths: np.ndarray, minimum: int = 400):
        short = [i for i, n in enumerate(lengths) if self.num_pool_frames(int(n)) < 1]
        if short:
            raise ValueError(f"utterance {short[0]} has {int(lengths[short[0]])} samples: too short for {self._FRONT} + "
                             "the TDNN stack")

    @ffi.on_device(lambda self, *a, **k: self.pack.device)
    def forward_strided(self, wav: torch.Tensor, chunk_stride: int, num_chunks: int, num_samples: int,
                        masks: torch.Tensor | None = None) -> torch.Tensor:
        lib = ffi.load()
        w = self.pack.struct
        dev = self.pack.device
        Tp = self.num_pool_frames(num_samples)
        if Tp < 1:
            raise ValueError(f"chunks of {num_samples} samples are too short for {self._FRONT} + the TDNN stack")
        S = 1 if masks is None else masks.shape[1]
        Fm = 0 if masks is None else masks.shape[2]
        idx = self.nearest_index(Fm, Tp) if masks is not None else None
        if masks is not None:
            masks = masks.to(dev, torch.float32).contiguous()
        emb = torch.empty((num_chunks, S, w.dimension), dtype=torch.float32, device=dev)
        c0 = 0
        while c0 < num_chunks:
            nb = min(self.max_chunks, num_chunks - c0)
            ws = self._workspace(getattr(lib, self._ABI + "_workspace_bytes")(w, nb, num_samples, S))
            sub = wav[c0 * chunk_stride:]
            rc = getattr(lib, self._ABI + "_forward")(
                w, ffi.c_fp(sub.data_ptr()), sub.numel(), chunk_stride, nb, num_samples,
                ffi.ptr(masks[c0:c0 + nb]) if masks is not None else None, S, Fm,
                ffi.ptr(idx) if idx is not None else None, ffi.ptr(emb[c0:c0 + nb]),
                ffi.ptr(ws), ws.numel(), ffi.stream())
            ffi.check(rc, self._ABI + "_forward")
            c0 += nb
        return emb


class XVectorMFCCEngine(XVectorEngine):
    """XVectorMFCC (models/embedding/xvector.py:42-202) over `pa_xvec_mfcc_forward`: torchaudio MFCC (csrc/mfcc.hip)
    -> the TDNN stack, pooling and Linear of XVectorEngine.  The MFCC of a chunk depends on that chunk alone (its own
    reflect padding, its own top_db maximum), so ragged batches fall back to one launch sequence per length."""

    _ABI, _FRONT = "pa_xvec_mfcc", "the MFCC front end"
    READS_PAST_END_AS_ZERO = True     # k_mfcc_mel reads samples past the waveform as zeros before reflecting

    def __init__(self, pack: XVectorMFCCPack, max_chunks: Optional[int] = None):
        super().__init__(pack, max_chunks)

    def _ragged_supported(self) -> bool:
        return False

    @ffi.on_device(lambda self, *a, **k: self.pack.device)
    def features(self, wav: torch.Tensor, chunk_stride: int, num_chunks: int, num_samples: int) -> torch.Tensor:
        """the MFCC front end alone: (num_chunks, frames, n_mfcc), torchaudio's MFCC of each chunk transposed"""
        lib = ffi.load()
        w = self.pack.struct
        if num_chunks <= 0:
            return torch.empty((0, 0, w.n_mfcc), dtype=torch.float32, device=self.pack.device)
        if (w.center and num_samples <= w.n_fft // 2) or (not w.center and num_samples < w.n_fft):
            raise ValueError(f"chunks of {num_samples} samples leave no MFCC frame")
        T = 1 + num_samples // w.hop_length if w.center else 1 + (num_samples - w.n_fft) // w.hop_length
        out = torch.empty((num_chunks, T, w.n_mfcc), dtype=torch.float32, device=self.pack.device)
        nbytes = 4 * (num_chunks * T * w.n_mels + num_chunks + 128)     # the mel energies + the chunk maxima, aligned
        ws = self._workspace(nbytes)
        rc = lib.pa_mfcc_features(w, ffi.c_fp(wav.data_ptr()), wav.numel(), chunk_stride, num_chunks, num_samples,
                                  ffi.ptr(out), ffi.ptr(ws), ws.numel(), ffi.stream())
        ffi.check(rc, "pa_mfcc_features")
        return out
