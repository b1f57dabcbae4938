"""Open-set speaker identification: who `SPEAKER_00` is, against a gallery of enrolled voiceprints, scored on the device.

The reference stops at `DiarizeOutput.speaker_embeddings`; this is the step after it (no reference counterpart; the
metric it is scored with, `annotation_metrics.IdentificationErrorRate`, restates pyannote.metrics).

* A `Gallery` is a table of named voiceprints, one float64 row per enrolled speaker; a voiceprint is the mean of the
  speaker's file embeddings, taken by `distance.centroid_means` (the arithmetic of a clustering centroid).
* The score of a (speaker, gallery entry) pair is their cosine distance, with the bits of
  `scipy.spatial.distance.cdist(., ., "cosine")`; with a cohort it is normalised by adaptive S-norm: with (mean, std) the
  statistics of each side's `top` smallest distances to the cohort, `0.5 * ((d - q_mean) / q_std + (d - g_mean) / g_std)`.
  The statistics are `np.cumsum(.)[-1] / K` over the ascending distances (`pa_cohort_stats_f64`): every addition in
  ascending order, every operation rounded on its own, so a numpy model (tests/identify_model.py) gives the same bits.
* `identify` names the speakers of a list of files in ONE set of launches: one statistics call for all their rows, one
  top-k call (`pa_gallery_topk_f64`), one call for the candidate cost matrices (`pa_gallery_pairs_f64`) and one batched
  assignment per distinct number of speakers (`distance.linear_sum_assignment_batch`); a speaker takes at most one name per file and a name at most one
  speaker.  Candidates per file are the union of its rows' k best columns with k = the file's speakers: that restriction
  keeps the optimum over the whole gallery.
* `SpeakerIdentification` wraps a diarization pipeline and renames the accepted speakers in its output.

There is no host implementation of the device parts: without a GPU they raise (ffi.require_gpu)."""
from __future__ import annotations

import json
import warnings
from dataclasses import dataclass, field
from typing import Iterable, Iterator, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ffi
from .pipeline import Parameter, Pipeline, Uniform
from .speaker_diarization import DiarizeOutput

GALLERY_FORMAT = "pyannote_audio_amd.gallery/1"


def identify_geometry() -> Tuple[int, int, int]:
    """(rows per tile, largest `top`, largest k) of the selection kernels, asked of the library (csrc/identify.hip)"""
    lib = ffi.load()
    return int(lib.pa_identify_tile()), int(lib.pa_identify_max_top()), int(lib.pa_identify_max_k())


#: a row's largest |entry| must lie in this range: below it the squares underflow and the float64 norm can be 0, above it
#: they overflow and the norm is inf -- either way the kernels' cosine distance of the row is NaN
NORM_SAFE_RANGE = (1e-150, 1e150)


def valid_rows(table: np.ndarray) -> np.ndarray:
    """(S,) bool: rows with a direction the kernels can use -- every entry finite and the largest magnitude within
    NORM_SAFE_RANGE, so that the float64 norm is neither 0 nor inf.  The padded centroids of `speaker_diarization.py`
    (all zero) and rows with a NaN have none and stay anonymous."""
    table = np.asarray(table)
    if table.shape[0] == 0:
        return np.zeros(0, dtype=bool)
    with np.errstate(invalid="ignore"):
        largest = np.abs(table).max(axis=1)
    return np.isfinite(table).all(axis=1) & (largest >= NORM_SAFE_RANGE[0]) & (largest <= NORM_SAFE_RANGE[1])


def _float64_table(x, what: str) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    table = np.asarray(x, dtype=np.float64)
    if table.ndim != 2 or table.shape[1] < 1:
        raise ValueError(f"{what} must be a (rows, dimension) array, got shape {tuple(table.shape)}")
    return np.ascontiguousarray(table)


def _checked_table(x, what: str) -> np.ndarray:
    table = _float64_table(x, what)
    if table.shape[0] < 1:
        raise ValueError(f"{what} is empty")
    bad = np.flatnonzero(~valid_rows(table))
    if bad.size:
        raise ValueError(f"{what}: row {int(bad[0])} is zero or not finite ({bad.size} such row(s); magnitudes outside "
                         f"{NORM_SAFE_RANGE} count as such)")
    return table


def _clipped_top(top: int, cohort_rows: int, warn: bool = True) -> int:
    """K of the statistics: `top`, clipped to the cohort and refused beyond the kernel's limit.  `warn`: say so when it
    clips (`Gallery.normalise`, where the choice is made; `identify` repeats the gallery's K without a word)"""
    top = int(top)
    if top < 1:
        raise ValueError(f"`top` must be positive, got {top}")
    if top > cohort_rows:
        if warn:
            warnings.warn(f"top={top} exceeds the {cohort_rows} cohort rows: every cohort row is used")
        top = cohort_rows
    limit = identify_geometry()[1]
    if top > limit:
        raise ValueError(f"top={top}: at most {limit} cohort distances per row are supported")
    return top


def _device() -> torch.device:
    ffi.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


# ------------------------------------------------------------------------------------------------ the three kernels
def cohort_stats(rows: torch.Tensor, cohort: torch.Tensor, top: int):
    """`pa_cohort_stats_f64` on device tensors: rows (M, D) and cohort (N, D) float64, 1 <= top <= N.
    -> (mean (M,), std (M,), status (M,) int32) on the device; status 1 = a row without a direction (its statistics NaN)"""
    ffi.require_gpu()
    lib = ffi.load()
    M, D = rows.shape
    N = cohort.shape[0]
    if cohort.shape[1] != D:
        raise ValueError(f"rows of dimension {D} against a cohort of dimension {cohort.shape[1]}")
    dev = rows.device
    mean = torch.empty(M, dtype=torch.float64, device=dev)
    std = torch.empty(M, dtype=torch.float64, device=dev)
    status = torch.empty(M, dtype=torch.int32, device=dev)
    nbytes = int(lib.pa_cohort_stats_workspace_bytes(M, N, D))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        ffi.check(lib.pa_cohort_stats_f64(ffi.ptr(rows), M, ffi.ptr(cohort), N, D, int(top), ffi.ptr(mean),
                                          ffi.ptr(std), ffi.ptr(status), ffi.ptr(work), nbytes, ffi.stream()),
                  "pa_cohort_stats_f64")
    return mean, std, status


def _stat_pointers(stats):
    if stats is None:
        return (None,) * 4
    if len(stats) != 4 or any(s is None for s in stats):
        raise ValueError("the statistics are (q_mean, q_std, g_mean, g_std), all four or None")
    return tuple(ffi.ptr(s) for s in stats)


def gallery_topk(queries: torch.Tensor, gallery: torch.Tensor, k: int, stats=None):
    """`pa_gallery_topk_f64`: -> (values (M, k) float64, indices (M, k) int32) on the device, per query the k smallest
    values over the gallery, ascending, ties to the lower index.  `stats`: None for distances, or the device tensors
    (q_mean, q_std, g_mean, g_std) for normalised scores."""
    ffi.require_gpu()
    lib = ffi.load()
    M, D = queries.shape
    Ng = gallery.shape[0]
    dev = queries.device
    values = torch.empty((M, k), dtype=torch.float64, device=dev)
    indices = torch.empty((M, k), dtype=torch.int32, device=dev)
    nbytes = int(lib.pa_gallery_workspace_bytes(M, Ng, D))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        ffi.check(lib.pa_gallery_topk_f64(ffi.ptr(queries), M, ffi.ptr(gallery), Ng, D, *_stat_pointers(stats), int(k),
                                          ffi.ptr(values), ffi.ptr(indices), ffi.ptr(work), nbytes, ffi.stream()),
                  "pa_gallery_topk_f64")
    return values, indices


def gallery_pairs(queries: torch.Tensor, gallery: torch.Tensor, iq: torch.Tensor, ig: torch.Tensor, stats=None):
    """`pa_gallery_pairs_f64`: the value of every pair (iq[p], ig[p]) (int32 device tensors) -> (P,) float64 on the device"""
    ffi.require_gpu()
    lib = ffi.load()
    M, D = queries.shape
    Ng = gallery.shape[0]
    dev = queries.device
    P = int(iq.shape[0])
    out = torch.empty(P, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ffi.check(lib.pa_gallery_pairs_f64(ffi.ptr(queries), M, ffi.ptr(gallery), Ng, D, *_stat_pointers(stats),
                                           ffi.ptr(iq), ffi.ptr(ig), P, ffi.ptr(out), ffi.stream()),
                  "pa_gallery_pairs_f64")
    return out


def _host_statistics(mean: torch.Tensor, std: torch.Tensor, status: torch.Tensor, what: str):
    """one download of the three (M,) outputs; refuses what cannot normalise a score"""
    packed = torch.stack([mean, std, status.to(torch.float64)]).cpu().numpy()
    mean_h, std_h, status_h = packed[0], packed[1], packed[2]
    if status_h.any():
        raise ValueError(f"{what}: row {int(np.flatnonzero(status_h)[0])} has no direction (zero or not finite)")
    if not np.isfinite(mean_h).all() or not np.isfinite(std_h).all():
        raise ValueError(f"{what}: a cohort statistic is not finite")
    if (std_h == 0).any():
        raise ValueError(f"{what}: row {int(np.flatnonzero(std_h == 0)[0])} has std == 0 over its cohort distances "
                         "(a constant cohort cannot normalise a score)")
    return mean_h, std_h


# ---------------------------------------------------------------------------------------------------------- gallery
class Gallery:
    """Named voiceprints: `names` (G unique non-empty strings) and `voiceprints` (G, D), kept as float64 (a float32
    embedding converts exactly).  The table goes to the device when a call first needs it.  After
    `normalise(cohort, top)` the gallery also holds `g_mean`, `g_std` (G,), its side of the score normalisation."""

    def __init__(self, names: Sequence[str], voiceprints):
        names = list(names)
        for name in names:
            if not isinstance(name, str) or not name:
                raise ValueError(f"gallery names must be non-empty strings, got {name!r}")
        if len(set(names)) != len(names):
            seen: set = set()
            duplicates = sorted({n for n in names if n in seen or seen.add(n)})
            raise ValueError(f"gallery names must be unique, got {duplicates} more than once")
        table = _checked_table(voiceprints, "the gallery")
        if table.shape[0] != len(names):
            raise ValueError(f"{len(names)} names for {table.shape[0]} voiceprints")
        self.names: List[str] = names
        self.voiceprints: np.ndarray = table
        self.g_mean: Optional[np.ndarray] = None
        self.g_std: Optional[np.ndarray] = None
        self.cohort_rows: Optional[int] = None       # the cohort the statistics were taken over, and its K
        self.top: Optional[int] = None
        self._on_device: dict = {}

    def __len__(self) -> int:
        return len(self.names)

    @property
    def dimension(self) -> int:
        return self.voiceprints.shape[1]

    @property
    def normalised(self) -> bool:
        return self.g_mean is not None

    def table(self, device: torch.device) -> torch.Tensor:
        """the (G, D) float64 table on `device`"""
        return self._cached("voiceprints", self.voiceprints, device)

    def statistics(self, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
        if not self.normalised:
            raise ValueError("the gallery has no cohort statistics: call gallery.normalise(cohort, top) first")
        return self._cached("g_mean", self.g_mean, device), self._cached("g_std", self.g_std, device)

    def _cached(self, key: str, array: np.ndarray, device: torch.device) -> torch.Tensor:
        slot = (key, str(device))
        if slot not in self._on_device:
            self._on_device[slot] = torch.from_numpy(array).to(device)
        return self._on_device[slot]

    def normalise(self, cohort, top: int = 300) -> "Gallery":
        """the gallery's side of adaptive S-norm: per voiceprint the mean and std of its `top` smallest distances to
        the `cohort` rows (N, D), in one `pa_cohort_stats_f64` call.  A cohort row that is zero or not finite, or a
        voiceprint whose distances have std == 0, raises ValueError."""
        cohort = _checked_table(cohort, "the cohort")
        if cohort.shape[1] != self.dimension:
            raise ValueError(f"a cohort of dimension {cohort.shape[1]} for a gallery of dimension {self.dimension}")
        K = _clipped_top(top, cohort.shape[0])
        dev = _device()
        mean, std, status = cohort_stats(self.table(dev), torch.from_numpy(cohort).to(dev), K)
        self.g_mean, self.g_std = _host_statistics(mean, std, status, "the gallery")
        self.cohort_rows, self.top = cohort.shape[0], K
        self._on_device = {k: v for k, v in self._on_device.items() if k[0] == "voiceprints"}
        return self

    # -- persistence: safetensors, the names as JSON in the metadata
    def save(self, path) -> None:
        from safetensors.numpy import save_file
        tensors = {"voiceprints": self.voiceprints}
        metadata = {"format": GALLERY_FORMAT, "names": json.dumps(self.names)}
        if self.normalised:
            tensors["g_mean"], tensors["g_std"] = self.g_mean, self.g_std
            metadata["cohort"] = json.dumps({"rows": self.cohort_rows, "top": self.top})
        save_file(tensors, str(path), metadata=metadata)

    @classmethod
    def load(cls, path) -> "Gallery":
        from safetensors import safe_open
        with safe_open(str(path), framework="np") as fp:
            metadata = fp.metadata() or {}
            if metadata.get("format") != GALLERY_FORMAT or "names" not in metadata:
                raise ValueError(f"{path} is not a gallery file ({GALLERY_FORMAT})")
            tensors = {key: fp.get_tensor(key) for key in fp.keys()}
        gallery = cls(json.loads(metadata["names"]), tensors["voiceprints"])
        if "g_mean" in tensors:
            cohort = json.loads(metadata["cohort"])
            gallery.g_mean = np.ascontiguousarray(tensors["g_mean"], dtype=np.float64)
            gallery.g_std = np.ascontiguousarray(tensors["g_std"], dtype=np.float64)
            gallery.cohort_rows, gallery.top = int(cohort["rows"]), int(cohort["top"])
        return gallery

    @classmethod
    def enroll(cls, pipeline, speakers: Mapping[str, Iterable], batch_size: int = 32) -> "Gallery":
        """`speakers`: {name: [AudioFile, ...]}.  Every file is embedded once through `pipeline.apply_batch` (a
        `SpeakerEmbedding`), `batch_size` files at a time; a voiceprint is the mean of its speaker's embeddings by
        `distance.centroid_means`: the rows added in the order given, in float32, one float32 division."""
        from .distance import centroid_means
        if batch_size < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        names, files, owner = [], [], []
        for name, speaker_files in speakers.items():
            speaker_files = list(speaker_files)
            if not speaker_files:
                raise ValueError(f"speaker {name!r} has no enrolment file")
            owner += [len(names)] * len(speaker_files)
            files += speaker_files
            names.append(name)
        if not names:
            raise ValueError("no speaker to enrol")
        ffi.require_gpu()
        embeddings = []
        for first in range(0, len(files), batch_size):
            embeddings.extend(pipeline.apply_batch(files[first:first + batch_size]))
        table = np.concatenate([np.asarray(e, dtype=np.float32).reshape(1, -1) for e in embeddings], axis=0)
        dev = _device()
        model = getattr(pipeline, "embedding_model_", None)
        if model is not None and getattr(model.device, "type", None) == "cuda":
            dev = model.device
        means = centroid_means(torch.from_numpy(table).to(dev).contiguous(), np.arange(len(files)),
                               np.asarray(owner, dtype=np.int64), len(names), dev)
        return cls(names, means)


# --------------------------------------------------------------------------------------------------------- identify
def candidate_columns(indices: np.ndarray, k: int) -> np.ndarray:
    """the gallery columns a file's assignment is solved over: the union of its rows' k best, ascending"""
    return np.unique(indices[:, :k])


def identify(embeddings_per_file: Sequence, gallery: Gallery, threshold: Optional[float] = None, cohort=None,
             top: int = 300) -> List[Tuple[np.ndarray, np.ndarray]]:
    """Name the speakers of a list of files against `gallery`.

    `embeddings_per_file`: per file an (S_f, D) array, one row per speaker (`DiarizeOutput.speaker_embeddings`).  Rows
    that are all zero or not finite are left out and stay anonymous.  `cohort` (N, D): scores are normalised by adaptive
    S-norm over it; the gallery must have been normalised with the same cohort size and `top`.  Within a file the
    pairing is the one-to-one assignment of the smallest total score; a pair is accepted iff its score <= `threshold`
    (None accepts every pair).
    -> per file `(index, value)`: (S_f,) int64 gallery index of every speaker row, -1 for an anonymous one, and (S_f,)
    float64 score of the row's assigned pair, accepted or not (NaN for a row that was left out or got no partner)."""
    from scipy.optimize import linear_sum_assignment
    from .distance import linear_sum_assignment_batch
    tables = [e.detach().cpu().numpy() if isinstance(e, torch.Tensor) else np.asarray(e) for e in embeddings_per_file]
    for f, table in enumerate(tables):
        if table.ndim != 2:
            raise ValueError(f"file {f} must be a (speakers, dimension) array, got shape {tuple(table.shape)}")
        if table.shape[1] != gallery.dimension:
            raise ValueError(f"file {f}: embeddings of dimension {table.shape[1]} against a gallery of dimension "
                             f"{gallery.dimension}")
    if threshold is not None and np.isnan(threshold):
        raise ValueError("`threshold` is NaN")
    if cohort is not None:
        cohort = _checked_table(cohort, "the cohort")
        if cohort.shape[1] != gallery.dimension:
            raise ValueError(f"a cohort of dimension {cohort.shape[1]} for a gallery of dimension {gallery.dimension}")
    # every file's rows in one float64 table: one conversion and one validity pass for the whole list
    row0 = np.concatenate([[0], np.cumsum([t.shape[0] for t in tables])]).astype(np.int64)
    stacked = np.concatenate(tables + [np.zeros((0, gallery.dimension))], axis=0).astype(np.float64, copy=False)
    valid = valid_rows(stacked)
    kept = [np.flatnonzero(valid[row0[f]:row0[f + 1]]) for f in range(len(tables))]
    results = [(np.full(t.shape[0], -1, dtype=np.int64), np.full(t.shape[0], np.nan)) for t in tables]
    first = np.concatenate([[0], np.cumsum([len(rows) for rows in kept])]).astype(np.int64)
    M, G = int(first[-1]), len(gallery)
    lib = ffi.load()
    _, _, max_k = identify_geometry()
    per_file_k = [min(len(rows), G) for rows in kept]
    if max(per_file_k, default=0) > max_k:
        raise ValueError(f"a file with {max(per_file_k)} speakers: at most {max_k} per file are supported")
    stats = None
    if cohort is not None:
        K = _clipped_top(top, cohort.shape[0], warn=False)
        if not gallery.normalised or (gallery.cohort_rows, gallery.top) != (cohort.shape[0], K):
            raise ValueError(f"the gallery is not normalised over this cohort ({cohort.shape[0]} rows, top {K}): call "
                             "gallery.normalise(cohort, top) first")
    if M == 0:
        return results
    dev = _device()
    queries = torch.from_numpy(np.ascontiguousarray(stacked[valid])).to(dev)
    table = gallery.table(dev)
    if cohort is not None:
        q_mean, q_std, status = cohort_stats(queries, torch.from_numpy(cohort).to(dev), K)
        _host_statistics(q_mean, q_std, status, "the speakers")
        stats = (q_mean, q_std) + gallery.statistics(dev)
    _, indices = gallery_topk(queries, table, max(per_file_k), stats)
    indices = indices.cpu().numpy()

    # the candidate cost matrix of every file, all from one pairs call.  Files the device solver takes are grouped by
    # their number of speakers S: a group is one (B, S, C) block, C its widest candidate list (at most S * S), whose
    # padding columns point at gallery row 0 and are masked out -- a file with many speakers does not widen the blocks
    # of the others.  The files SciPy solves follow as flat matrices.
    limit = int(lib.pa_lsap_max_size())
    columns = [candidate_columns(indices[first[f]:first[f + 1]], per_file_k[f]) if per_file_k[f] else
               np.zeros(0, dtype=np.int64) for f in range(len(tables))]
    scored = [f for f in range(len(tables)) if per_file_k[f]]
    solved_host = [f for f in scored if len(kept[f]) > limit or len(columns[f]) > limit]
    groups: dict = {}
    for f in scored:
        if len(kept[f]) <= limit and len(columns[f]) <= limit:
            groups.setdefault(len(kept[f]), []).append(f)
    flat_q, flat_g, blocks = [], [], []
    for S, members in sorted(groups.items()):
        Cn = max(len(columns[f]) for f in members)
        iq = np.zeros((len(members), S, Cn), dtype=np.int32)
        ig = np.zeros((len(members), S, Cn), dtype=np.int32)
        col_mask = np.zeros((len(members), Cn), dtype=bool)
        for b, f in enumerate(members):
            iq[b] = (first[f] + np.arange(S))[:, None]
            ig[b, :, :len(columns[f])] = columns[f][None, :]
            col_mask[b, :len(columns[f])] = True
        flat_q.append(iq.reshape(-1))
        flat_g.append(ig.reshape(-1))
        blocks.append((members, S, Cn, col_mask))
    for f in solved_host:
        flat_q.append(np.repeat(first[f] + np.arange(len(kept[f])), len(columns[f])).astype(np.int32))
        flat_g.append(np.tile(columns[f], len(kept[f])).astype(np.int32))
    iq_d = torch.from_numpy(np.concatenate(flat_q)).to(dev)
    ig_d = torch.from_numpy(np.concatenate(flat_g)).to(dev)
    values = gallery_pairs(queries, table, iq_d, ig_d, stats)
    host_values = values.cpu().numpy()

    def settle(f: int, cost: np.ndarray, col4row: np.ndarray):
        index, value = results[f]
        for r, c in enumerate(col4row):
            if c < 0:
                continue
            value[kept[f][r]] = cost[r, c]
            if threshold is None or cost[r, c] <= threshold:
                index[kept[f][r]] = columns[f][c]

    at = 0
    for members, S, Cn, col_mask in blocks:      # one launch per distinct number of speakers
        size = len(members) * S * Cn
        cost = values[at:at + size].view(len(members), S, Cn)
        col4row = linear_sum_assignment_batch(cost, col_mask=col_mask).cpu().numpy()
        host_cost = host_values[at:at + size].reshape(len(members), S, Cn)
        at += size
        for b, f in enumerate(members):
            settle(f, host_cost[b], col4row[b])
    for f in solved_host:
        S, U = len(kept[f]), len(columns[f])
        cost = host_values[at:at + S * U].reshape(S, U)
        at += S * U
        col4row = np.full(S, -1, dtype=np.int64)
        rows, cols = linear_sum_assignment(cost)
        col4row[rows] = cols
        settle(f, cost, col4row)
    return results


# --------------------------------------------------------------------------------------------------------- pipeline
@dataclass
class IdentifiedOutput(DiarizeOutput):
    """a `DiarizeOutput` whose accepted speakers carry their gallery names; `matches`: {anonymous label: (name, value)}
    for every speaker that got a partner, the name None where the pair was rejected by the threshold"""
    matches: dict = field(default_factory=dict)


def rename_speakers(output: DiarizeOutput, names: Sequence[str], index: np.ndarray, value: np.ndarray) -> IdentifiedOutput:
    """`output` with the speakers that `identify` accepted renamed in both annotations.  Row r of `index` / `value`
    belongs to `output.speaker_diarization.labels()[r]`, the row order of `speaker_embeddings`; rejected speakers keep
    their label.  A gallery name equal to a label that stays in the file raises ValueError."""
    labels = output.speaker_diarization.labels()
    if len(index) != len(labels) or len(value) != len(labels):
        raise ValueError(f"{len(index)} identification rows for {len(labels)} speakers")
    mapping, matches = {}, {}
    for label, i, v in zip(labels, index, value):
        if i >= 0:
            mapping[label] = names[int(i)]
            matches[label] = (names[int(i)], float(v))
        elif not np.isnan(v):
            matches[label] = (None, float(v))
    kept = {label for label in labels if label not in mapping}
    clash = sorted(kept & set(mapping.values()), key=str)
    if clash:
        raise ValueError(f"gallery name(s) {clash} equal anonymous speaker label(s) of {output.speaker_diarization.uri!r}")
    return IdentifiedOutput(
        speaker_diarization=output.speaker_diarization.rename_labels(mapping=mapping),
        exclusive_speaker_diarization=output.exclusive_speaker_diarization.rename_labels(mapping=mapping),
        speaker_embeddings=output.speaker_embeddings, matches=matches)


class SpeakerIdentification(Pipeline):
    """`SpeakerIdentification(diarization_pipeline, gallery, cohort=None, top=300)`: diarize, then name every speaker
    whose best one-to-one partner in `gallery` scores at most `threshold` (the pipeline's one hyper-parameter of its
    own; cosine distance without a cohort, S-normalised with one).  `apply(file, **kw)` and `apply_batch(files, **kw)`
    pass their keyword arguments (`num_speakers=`, `pack=`, ...) to the diarization pipeline; `apply_batch` identifies
    the speakers of all files in one set of launches.

    Limits, each a `ValueError`: with a `cohort` the gallery must already be normalised over it
    (`gallery.normalise(cohort, top)`: the pipeline does not change the caller's gallery); a file with more than
    `pa_identify_max_k()` = 64 speakers; `joint_clustering=True`, whose outputs share one centroid table that is not
    a file's list of speakers (row r of `speaker_embeddings` must be `labels()[r]`, which the per-file back end
    guarantees); a gallery name equal to an anonymous label that stays in the file."""

    def __init__(self, diarization_pipeline: Pipeline, gallery: Gallery, cohort=None, top: int = 300):
        super().__init__()
        if not isinstance(gallery, Gallery):
            raise TypeError(f"`gallery` must be a Gallery, got {type(gallery).__name__}")
        if getattr(diarization_pipeline, "legacy", False):
            raise ValueError("the diarization pipeline must return DiarizeOutput (legacy=False): the speaker "
                             "embeddings are what gets identified")
        self.diarization = diarization_pipeline
        self.gallery = gallery
        self.cohort = None if cohort is None else _checked_table(cohort, "the cohort")
        self.top = top
        self.threshold = Uniform(0., 2.)

    def default_parameters(self):
        return {"threshold": 2.0}

    def get_metric(self):
        from . import annotation_metrics
        device = getattr(self, "device", None)
        on_gpu = device is not None and getattr(device, "type", None) == "cuda"
        return annotation_metrics.IdentificationErrorRate(device=device if on_gpu else None)

    def get_direction(self) -> str:
        return "minimize"

    def _identify(self, outputs: List[DiarizeOutput]) -> List[IdentifiedOutput]:
        for output in outputs:
            if not isinstance(output, DiarizeOutput) or output.speaker_embeddings is None:
                raise ValueError("the diarization pipeline returned no speaker embeddings to identify")
        if isinstance(self.threshold, Parameter):
            raise RuntimeError("A pipeline must be instantiated with `pipeline.instantiate(parameters)` before it can "
                               "be applied.")
        found = identify([o.speaker_embeddings for o in outputs], self.gallery, threshold=self.threshold,
                         cohort=self.cohort, top=self.top)
        return [rename_speakers(o, self.gallery.names, index, value) for o, (index, value) in zip(outputs, found)]

    def apply(self, file, **kwargs) -> IdentifiedOutput:
        ffi.require_gpu()
        return self._identify([self.diarization.apply(file, **kwargs)])[0]

    def apply_batch(self, files: Iterable, **kwargs) -> Iterator[tuple]:
        if kwargs.get("joint_clustering"):
            raise ValueError("joint_clustering=True returns one centroid table for all files, whose rows are not a "
                             "file's speakers: identify per-file outputs")
        ffi.require_gpu()
        done = list(self.diarization.apply_batch(files, **kwargs))
        named = self._identify([output for _, output in done])
        for (file, _), output in zip(done, named):
            yield file, output
