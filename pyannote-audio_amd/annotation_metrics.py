"""Time-based diarization and detection error rates on `Annotation`s in seconds: what the reference's pipelines
return from `get_metric()` (pipelines/speaker_diarization.py:786, pipelines/voice_activity_detection.py:207) and
what `pipelines/utils/diarization.py:104-148` maps speakers with.

pyannote.metrics is not a dependency of this package and its source was not at hand where this was written: the
classes below are a restatement of its published behaviour (as `core.py` is for pyannote.core), unpinned.  The
contract is the one written down in include/pyannote_amd.h (`pa_annot_counts`) and DESIGN.md section 21, and the
tests hold it to an independent exact-arithmetic computation (tests/annotation_metrics_truth.py).  Two deliberate
differences from pyannote.metrics: overlapping tracks of ONE label count once (pyannote.metrics counts them twice;
the pipelines never produce such tracks), and intervals are taken exactly (no 1e-6 "segment precision" rule: pieces
of zero length contribute 0, shorter-than-a-microsecond pieces their length).  `MacroAverageFMeasure` follows the
reference's own class (utils/metric.py:289-377).  `JaccardErrorRate` (the other metric the reference's command line
offers, __main__.py:46) is restated and unpinned like the rest.

Every class splits into "the counts of a file" and `components_from_counts(counts)`: `evaluation.Corpus` takes the
counts of all files of a corpus in one device call and hands them to `add_counts`.

`annotation_counts` is the one place the integrals are taken: on a `cuda` device by the kernels of
csrc/annot_metrics.hip, otherwise (or with more than 64 labels on a side) by a numpy sweep over the same elementary
intervals.  `window_counts` takes them for many windows of one file from ONE sweep (`pa_annot_window_counts`, DESIGN.md
section 29); `SlidingDiarizationErrorRate`, the reference's own class (utils/metric.py:245-286), is built on it.
The names here are this module's own: `metrics.DiarizationErrorRate` is the torchmetrics class."""
from __future__ import annotations

import warnings
from typing import Mapping, Optional

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from . import ffi
from .core import Annotation, SlidingWindow
from .metrics import BaseMetric, _as_timeline

MAX_LABELS = 64          # a side's labels travel as one 64-bit mask on the device

_SCALARS = ("total", "false_alarm", "missed", "both", "ref_speech", "hyp_speech", "both_speech")


# -------------------------------------------------------------------------------------------------- inputs
def _rows(annotation) -> tuple:
    """(labels in `labels()` order, (N, 2) float64 start / end, (N,) int32 label index)"""
    labels = annotation.labels()
    index = {label: i for i, label in enumerate(labels)}
    if hasattr(annotation, "flat_rows"):
        rows = [(a, b, l) for a, b, _, l in annotation.flat_rows()]
    else:  # pragma: no cover - pyannote.core's own Annotation
        rows = [(s.start, s.end, l) for s, _, l in annotation.itertracks(yield_label=True)]
    seg = np.array([(a, b) for a, b, _ in rows], dtype=np.float64).reshape(-1, 2)
    lab = np.array([index[l] for _, _, l in rows], dtype=np.int32)
    return labels, seg, lab


def _uem_rows(uem) -> np.ndarray:
    return np.array([(s.start, s.end) for s in uem], dtype=np.float64).reshape(-1, 2)


def _check(name: str, seg: np.ndarray):
    if np.isnan(seg).any():
        raise ValueError(f"{name}: a segment boundary is NaN")
    if (seg[:, 1] < seg[:, 0]).any():
        raise ValueError(f"{name}: a segment ends before it starts")


def _split(reference, uem):
    """a file mapping as `reference` ("annotation", optional "annotated") -> (annotation, uem)"""
    if isinstance(reference, Mapping):
        if uem is None and "annotated" in reference:
            uem = reference["annotated"]
        reference = reference["annotation"]
    return reference, uem


def _device(device) -> Optional[torch.device]:
    if device is None:
        return None
    device = torch.device(device)
    if device.type != "cuda":
        return None
    if device.index is None:
        ffi.require_gpu()
        device = torch.device("cuda", torch.cuda.current_device())
    return device


# -------------------------------------------------------------------------------------------------- counts
def _host_sweep(ref_seg, ref_lab, Kr, hyp_seg, hyp_lab, Kh, uem_seg, collar, skip_overlap, extra=None):
    """The kernel's sweep in numpy: cut the axis at every boundary (and at the `extra` values, which are cuts
    only), mark per elementary interval which labels are on and whether it is evaluated.  -> the sorted distinct
    cuts (n + 1), bool R (n, Kr) and H (n, Kh), the label counts nr, nh (n) and the evaluated lengths d (n); None
    without an interval."""
    half = 0.5 * collar
    bounds = np.concatenate([ref_seg.ravel(), ref_seg.ravel() - half, ref_seg.ravel() + half])
    cuts = np.unique(np.concatenate([bounds if collar > 0 else ref_seg.ravel(), hyp_seg.ravel(), uem_seg.ravel()] +
                                    ([] if extra is None else [extra])))
    n = max(len(cuts) - 1, 0)
    if n == 0:
        return None

    def coverage(seg, columns, width):
        """(n, width) number of segments of every column that cover every interval"""
        delta = np.zeros((n + 1, width), dtype=np.int64)
        np.add.at(delta, (np.searchsorted(cuts, seg[:, 0]), columns), 1)
        np.add.at(delta, (np.searchsorted(cuts, seg[:, 1]), columns), -1)
        return np.cumsum(delta, axis=0)[:n]

    R = coverage(ref_seg, ref_lab, Kr) > 0
    H = coverage(hyp_seg, hyp_lab, Kh) > 0
    nr, nh = R.sum(axis=1), H.sum(axis=1)
    evaluated = coverage(uem_seg, np.zeros(len(uem_seg), dtype=np.int64), 1)[:, 0] > 0
    if collar > 0:
        b = ref_seg.ravel()
        around = np.stack([b - half, b + half], axis=1)
        evaluated &= coverage(around, np.zeros(len(b), dtype=np.int64), 1)[:, 0] == 0
    if skip_overlap:
        evaluated &= nr < 2
    return cuts, R, H, nr, nh, np.where(evaluated, np.diff(cuts), 0.0)


def _scalar_weights(nr, nh) -> tuple:
    """per interval, what multiplies its length in each of the seven scalars, in `_SCALARS` order"""
    return (nr, np.maximum(0, nh - nr), np.maximum(0, nr - nh), np.minimum(nr, nh), nr > 0, nh > 0,
            (nr > 0) & (nh > 0))


def _host_counts(ref_seg, ref_lab, Kr, hyp_seg, hyp_lab, Kh, uem_seg, collar, skip_overlap) -> np.ndarray:
    """The kernel's sums by the numpy sweep: sum the lengths of the evaluated elementary intervals."""
    out = np.zeros(Kr * Kh + Kr + Kh + len(_SCALARS))
    sweep = _host_sweep(ref_seg, ref_lab, Kr, hyp_seg, hyp_lab, Kh, uem_seg, collar, skip_overlap)
    if sweep is None:
        return out
    _, R, H, nr, nh, d = sweep
    Rd = R * d[:, None]
    n0 = Kr * Kh
    out[:n0] = (Rd.T @ H.astype(np.float64)).ravel()
    out[n0:n0 + Kr] = Rd.sum(axis=0)
    out[n0 + Kr:n0 + Kr + Kh] = (H * d[:, None]).sum(axis=0)
    out[n0 + Kr + Kh:] = [np.sum(w * d) for w in _scalar_weights(nr, nh)]
    return out


def _host_window_counts(ref_seg, ref_lab, Kr, hyp_seg, hyp_lab, Kh, uem_seg, win_seg, collar,
                        skip_overlap) -> np.ndarray:
    """`pa_annot_window_counts` in numpy, (W, Kr*Kh + Kr + Kh + 7): the sweep of `_host_counts` with the window
    boundaries among the cuts, then per window the sum over its range of intervals (`searchsorted` of its
    boundaries; `np.add.reduceat` sums every range by itself, in order -- differences of running sums would carry
    the rounding of everything in front of the window)."""
    W, n0 = len(win_seg), Kr * Kh
    out = np.zeros((W, n0 + Kr + Kh + len(_SCALARS)))
    sweep = _host_sweep(ref_seg, ref_lab, Kr, hyp_seg, hyp_lab, Kh, uem_seg, collar, skip_overlap,
                        extra=win_seg.ravel()) if W else None
    if sweep is None:
        return out
    cuts, R, H, nr, nh, d = sweep
    first, last = np.searchsorted(cuts, win_seg[:, 0]), np.searchsorted(cuts, win_seg[:, 1])
    empty = last <= first
    pairs = np.stack([first, last], axis=1).ravel()       # reduceat sums [pairs[i], pairs[i + 1]): the even ones

    def ranges(terms):
        """(n, C) terms -> (W, C) sums over every window's intervals (a row of zeros behind: index n is valid)"""
        sums = np.add.reduceat(np.concatenate([terms, np.zeros((1, terms.shape[1]))]), pairs, axis=0)[0::2]
        sums[empty] = 0.0                                 # (reduceat gives one row, not none, for an empty range)
        return sums

    Rd, Hf = R * d[:, None], H.astype(np.float64)
    for i in range(Kr):                                   # (labels, not windows: (n, Kr * Kh) at once is too much)
        out[:, i * Kh:(i + 1) * Kh] = ranges(Rd[:, i:i + 1] * Hf)
    out[:, n0:] = ranges(np.concatenate([Rd, Hf * d[:, None], np.stack(_scalar_weights(nr, nh), axis=1) * d[:, None]],
                                        axis=1))
    return out


def device_counts(ref_seg, ref_lab, Kr, hyp_seg, hyp_lab, Kh, uem_seg, collar, skip_overlap,
                  device: torch.device) -> torch.Tensor:
    """`pa_annot_counts` on host arrays: one upload, four launches; -> the (Kr*Kh + Kr + Kh + 7,) float64 device
    tensor (nothing is copied back here)."""
    Nr, Nh, Nu = len(ref_seg), len(hyp_seg), len(uem_seg)
    # one upload: [ref_seg][hyp_seg][uem_seg] float64, then the labels as int32 in the same buffer
    f64 = np.concatenate([ref_seg.ravel(), hyp_seg.ravel(), uem_seg.ravel()]).astype(np.float64)
    i32 = np.concatenate([ref_lab, hyp_lab]).astype(np.int32)
    if len(i32) % 2:
        i32 = np.concatenate([i32, np.zeros(1, dtype=np.int32)])
    packed = torch.from_numpy(np.concatenate([f64, i32.view(np.float64)])).to(device)
    segs, labs = packed[:len(f64)], packed[len(f64):].view(torch.int32)
    lib = ffi.load()
    ws_bytes = int(lib.pa_annot_counts_workspace_bytes(Nr, Nh, Nu))
    if ws_bytes == 0:
        raise ValueError(f"{Nr} + {Nh} + {Nu} segments are more than the device sort accepts")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    out = torch.empty(Kr * Kh + Kr + Kh + len(_SCALARS), dtype=torch.float64, device=device)

    def at(t, offset, n):
        return ffi.ptr(t[offset:offset + n]) if n else None

    with torch.cuda.device(device):
        ffi.check(lib.pa_annot_counts(at(segs, 0, 2 * Nr), at(labs, 0, Nr), Nr, Kr,
                                      at(segs, 2 * Nr, 2 * Nh), at(labs, Nr, Nh), Nh, Kh,
                                      at(segs, 2 * (Nr + Nh), 2 * Nu), Nu, float(collar), int(bool(skip_overlap)),
                                      ffi.ptr(out), ffi.ptr(ws), ws_bytes, ffi.stream()), "pa_annot_counts")
    return out


def _inputs(reference, hypothesis, uem, collar, warn: bool) -> tuple:
    """what `annotation_counts` and `window_counts` check and flatten, called from them directly (the warning
    names their caller): -> ref_labels, ref_seg, ref_lab, hyp_labels, hyp_seg, hyp_lab, uem_seg"""
    reference, uem = _split(reference, uem)
    ref_labels, ref_seg, ref_lab = _rows(reference)
    hyp_labels, hyp_seg, hyp_lab = _rows(hypothesis)
    _check("reference", ref_seg)
    _check("hypothesis", hyp_seg)
    if not collar >= 0.0:
        raise ValueError(f"collar must be >= 0, got {collar}")
    if uem is None:
        if warn:       # (`diarization.cooccurrence` means the whole extent)
            warnings.warn("'uem' was approximated by the union of 'reference' and 'hypothesis' extents.",
                          UserWarning, stacklevel=3)
        both = np.concatenate([ref_seg, hyp_seg])
        uem_seg = np.array([[both[:, 0].min(), both[:, 1].max()]]) if len(both) else np.zeros((0, 2))
    else:
        uem_seg = _uem_rows(uem)
        _check("uem", uem_seg)
    return ref_labels, ref_seg, ref_lab, hyp_labels, hyp_seg, hyp_lab, uem_seg


def annotation_counts(reference: Annotation, hypothesis: Annotation, uem=None, collar: float = 0.0,
                      skip_overlap: bool = False, device=None, _warn: bool = True) -> dict:
    """The integrals every class below is made of (include/pyannote_amd.h, `pa_annot_counts`).  Labels are indexed
    in `labels()` order on each side.  `uem`: a `Timeline`, a list of `Segment`s, or None -- then the evaluated
    region is the one segment from the earliest start to the latest end over both annotations, with a warning, as
    pyannote.metrics does.  A `cuda` device runs the kernels; None, `cpu`, or more than 64 labels on a side the
    numpy sweep.  -> `ref_labels`, `hyp_labels`, float64 numpy `cooc` (Kr, Kh), `ref_dur`, `hyp_dur`, and floats
    `total`, `false_alarm`, `missed`, `both`, `ref_speech`, `hyp_speech`, `both_speech`."""
    ref_labels, ref_seg, ref_lab, hyp_labels, hyp_seg, hyp_lab, uem_seg = _inputs(reference, hypothesis, uem, collar,
                                                                                  _warn)
    Kr, Kh = len(ref_labels), len(hyp_labels)
    dev = _device(device) if Kr <= MAX_LABELS and Kh <= MAX_LABELS else None
    if dev is not None:
        flat = device_counts(ref_seg, ref_lab, Kr, hyp_seg, hyp_lab, Kh, uem_seg, collar, skip_overlap,
                             dev).cpu().numpy()
    else:
        flat = _host_counts(ref_seg, ref_lab, Kr, hyp_seg, hyp_lab, Kh, uem_seg, float(collar), bool(skip_overlap))
    return counts_dict(ref_labels, hyp_labels, flat)


def counts_dict(ref_labels: list, hyp_labels: list, flat: np.ndarray) -> dict:
    """the Kr*Kh + Kr + Kh + 7 values of `pa_annot_counts` as the dict `annotation_counts` returns"""
    Kr, Kh = len(ref_labels), len(hyp_labels)
    n0 = Kr * Kh
    counts = {"ref_labels": ref_labels, "hyp_labels": hyp_labels, "cooc": flat[:n0].reshape(Kr, Kh),
              "ref_dur": flat[n0:n0 + Kr], "hyp_dur": flat[n0 + Kr:n0 + Kr + Kh]}
    counts.update({name: float(v) for name, v in zip(_SCALARS, flat[n0 + Kr + Kh:])})
    return counts


# -------------------------------------------------------------------------------------------------- windows
def device_window_counts(ref_seg, ref_lab, Kr, hyp_seg, hyp_lab, Kh, uem_seg, win_seg, collar, skip_overlap,
                         device: torch.device) -> torch.Tensor:
    """`pa_annot_window_counts` on host arrays: one upload, four launches; -> the (W, Kr*Kh + Kr + Kh + 7) float64
    device tensor (nothing is copied back here)."""
    Nr, Nh, Nu, W = len(ref_seg), len(hyp_seg), len(uem_seg), len(win_seg)
    out = torch.empty((W, Kr * Kh + Kr + Kh + len(_SCALARS)), dtype=torch.float64, device=device)
    if W == 0:
        return out
    f64 = np.concatenate([ref_seg.ravel(), hyp_seg.ravel(), uem_seg.ravel(), win_seg.ravel()]).astype(np.float64)
    i32 = np.concatenate([ref_lab, hyp_lab]).astype(np.int32)
    if len(i32) % 2:
        i32 = np.concatenate([i32, np.zeros(1, dtype=np.int32)])
    packed = torch.from_numpy(np.concatenate([f64, i32.view(np.float64)])).to(device)
    segs, labs = packed[:len(f64)], packed[len(f64):].view(torch.int32)
    lib = ffi.load()
    ws_bytes = int(lib.pa_annot_window_counts_workspace_bytes(Nr, Nh, Nu, W))
    if ws_bytes == 0:
        raise ValueError(f"{Nr} + {Nh} + {Nu} segments and {W} windows are more than the device sort accepts")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)

    def at(t, offset, n):
        return ffi.ptr(t[offset:offset + n]) if n else None

    with torch.cuda.device(device):
        ffi.check(lib.pa_annot_window_counts(at(segs, 0, 2 * Nr), at(labs, 0, Nr), Nr, Kr,
                                             at(segs, 2 * Nr, 2 * Nh), at(labs, Nr, Nh), Nh, Kh,
                                             at(segs, 2 * (Nr + Nh), 2 * Nu), Nu,
                                             at(segs, 2 * (Nr + Nh + Nu), 2 * W), W, float(collar),
                                             int(bool(skip_overlap)), ffi.ptr(out), ffi.ptr(ws), ws_bytes,
                                             ffi.stream()), "pa_annot_window_counts")
    return out


def _window_rows(windows) -> np.ndarray:
    """a list of `Segment`s (or pairs) or a (W, 2) array -> (W, 2) float64 start / end"""
    if isinstance(windows, np.ndarray):
        rows = np.asarray(windows, dtype=np.float64)
    else:
        rows = np.array([tuple(w) for w in windows], dtype=np.float64)
    if rows.size and (rows.ndim != 2 or rows.shape[1] != 2):
        raise ValueError(f"windows: expected (W, 2) start / end, got shape {rows.shape}")
    return np.ascontiguousarray(rows.reshape(-1, 2))


def window_counts(reference: Annotation, hypothesis: Annotation, windows, uem=None, collar: float = 0.0,
                  skip_overlap: bool = False, device=None) -> dict:
    """`annotation_counts` for every window of one file at once (include/pyannote_amd.h, `pa_annot_window_counts`):
    the counts of window w are those of (reference, hypothesis, uem intersected with the window), labels indexed
    file-wide, collars around the reference boundaries of the FILE (a crop would put new ones at the window's
    edges).  `windows`: a list of `Segment`s or a (W, 2) array, in any order, overlapping or not.  A `cuda` device
    does one upload, one call and one download; None, `cpu`, or more than 64 labels on a side the numpy form of the
    same sweep.  -> `ref_labels`, `hyp_labels`, float64 numpy `cooc` (W, Kr, Kh), `ref_dur` (W, Kr), `hyp_dur`
    (W, Kh) and (W,) arrays `total`, `false_alarm`, `missed`, `both`, `ref_speech`, `hyp_speech`, `both_speech`."""
    ref_labels, ref_seg, ref_lab, hyp_labels, hyp_seg, hyp_lab, uem_seg = _inputs(reference, hypothesis, uem, collar,
                                                                                  True)
    win_seg = _window_rows(windows)
    _check("windows", win_seg)
    Kr, Kh = len(ref_labels), len(hyp_labels)
    dev = _device(device) if Kr <= MAX_LABELS and Kh <= MAX_LABELS else None
    if dev is not None:
        flat = device_window_counts(ref_seg, ref_lab, Kr, hyp_seg, hyp_lab, Kh, uem_seg, win_seg, collar,
                                    skip_overlap, dev).cpu().numpy()
    else:
        flat = _host_window_counts(ref_seg, ref_lab, Kr, hyp_seg, hyp_lab, Kh, uem_seg, win_seg, float(collar),
                                   bool(skip_overlap))
    W, n0 = len(win_seg), Kr * Kh
    counts = {"ref_labels": ref_labels, "hyp_labels": hyp_labels, "cooc": flat[:, :n0].reshape(W, Kr, Kh),
              "ref_dur": flat[:, n0:n0 + Kr], "hyp_dur": flat[:, n0 + Kr:n0 + Kr + Kh]}
    counts.update({name: flat[:, n0 + Kr + Kh + s] for s, name in enumerate(_SCALARS)})
    return counts


# ------------------------------------------------------------------------------------------------- mappings
def optimal_mapping(cooc) -> dict:
    """{hypothesis index: reference index} of the one-to-one mapping with the largest matched duration, from the
    (Kr, Kh) `cooc` of `annotation_counts`: `linear_sum_assignment` on the negated (hypothesis, reference) matrix;
    pairs that never overlap stay unmapped."""
    together = np.asarray(cooc, dtype=np.float64).T
    if not together.size:
        return {}
    return {int(j): int(i) for j, i in zip(*linear_sum_assignment(-together)) if together[j, i] > 0}


def greedy_mapping(cooc) -> dict:
    """{hypothesis index: reference index}: repeatedly the first maximum, in row-major order of the (hypothesis,
    reference) matrix, then its row and column are out, while the maximum is > 0."""
    together = np.array(cooc, dtype=np.float64).T
    mapping = {}
    while together.size:
        j, i = np.unravel_index(np.argmax(together), together.shape)   # (argmax: the first of equal maxima)
        if not together[j, i] > 0:
            break
        mapping[int(j)] = int(i)
        together[j, :] = -np.inf
        together[:, i] = -np.inf
    return mapping


# -------------------------------------------------------------------------------------------------- classes
class _AnnotationMetric(BaseMetric):
    """what the classes share: the variant (`collar`, `skip_overlap`), where the counting runs (`device`), and the
    `uem=` keyword of a call"""

    def __init__(self, collar: float = 0.0, skip_overlap: bool = False, device=None, **kwargs):
        super().__init__(**kwargs)
        self.collar = collar
        self.skip_overlap = skip_overlap
        self.device = device

    def counts(self, reference, hypothesis, uem=None) -> dict:
        return annotation_counts(reference, hypothesis, uem=uem, collar=self.collar,
                                 skip_overlap=self.skip_overlap, device=self.device)

    def components_from_counts(self, counts: dict) -> dict:
        """the components of one file from its `annotation_counts`"""
        raise NotImplementedError

    def compute_components(self, reference, hypothesis, uem=None, **kwargs) -> dict:
        return self.components_from_counts(self.counts(reference, hypothesis, uem=uem))

    def add_counts(self, counts: dict, uri: Optional[str] = None, detailed: bool = False):
        """what `metric(reference, hypothesis, uri=uri)` does after the counting, for counts taken elsewhere
        (`evaluation.Corpus.counts` takes those of all files in one device call)"""
        components = self.components_from_counts(counts)
        components[self.metric_name_] = self.compute_metric(components)
        self.add_components(components, uri or "NA")
        return components if detailed else components[self.metric_name_]

    def report(self) -> dict:
        """{uri: {component: value, ..., metric name: the file's value}, ..., "TOTAL": the same over everything
        accumulated} (the reference's data frame, as a dict; `MacroAverageFMeasure.report` has the same shape)"""
        table = {uri: dict(components) for uri, components in self.results_}
        table["TOTAL"] = dict(self.accumulated_)
        table["TOTAL"][self.metric_name_] = abs(self)
        return table


def _error_rate(components: dict) -> float:
    """(false alarm + missed detection + confusion) / total; an empty reference gives 0 without errors, else 1"""
    errors = components["false alarm"] + components["missed detection"] + components["confusion"]
    total = components["total"]
    if total == 0:
        return 0.0 if errors == 0 else 1.0
    return float(errors / total)


class DiarizationErrorRate(_AnnotationMetric):
    """pyannote.metrics.diarization.DiarizationErrorRate: hypothesis labels are mapped one-to-one onto reference
    labels so that the matched duration is largest (Hungarian), then
    (false alarm + missed detection + confusion) / total.  `metric(reference, hypothesis, uem=None)`."""

    _mapper = staticmethod(optimal_mapping)

    @classmethod
    def metric_name(cls):
        return "diarization error rate"

    @classmethod
    def metric_components(cls):
        return ["total", "correct", "false alarm", "missed detection", "confusion"]

    def _mapping(self, reference, hypothesis, uem=None, mapper=None) -> dict:
        counts = self.counts(reference, hypothesis, uem=uem)
        pairs = (mapper or self._mapper)(counts["cooc"])
        return {counts["hyp_labels"][j]: counts["ref_labels"][i] for j, i in pairs.items()}

    def optimal_mapping(self, reference, hypothesis, uem=None) -> dict:
        """{hypothesis label: reference label}"""
        return self._mapping(reference, hypothesis, uem=uem, mapper=optimal_mapping)

    def components_from_counts(self, counts: dict) -> dict:
        cooc = counts["cooc"]
        # the mapping works on indices: a hypothesis label that is left unmapped is nobody, even when a reference
        # label carries the same name
        correct = float(sum(cooc[i, j] for j, i in sorted(self._mapper(cooc).items())))
        return {"total": counts["total"], "correct": correct, "false alarm": counts["false_alarm"],
                "missed detection": counts["missed"], "confusion": counts["both"] - correct}

    def compute_metric(self, components):
        return _error_rate(components)


class GreedyDiarizationErrorRate(DiarizationErrorRate):
    """pyannote.metrics.diarization.GreedyDiarizationErrorRate: the mapping is found greedily (`greedy_mapping`)"""

    _mapper = staticmethod(greedy_mapping)

    def greedy_mapping(self, reference, hypothesis, uem=None) -> dict:
        """{hypothesis label: reference label}"""
        return self._mapping(reference, hypothesis, uem=uem, mapper=greedy_mapping)


_WINDOW_COMPONENTS = ("total", "correct", "false alarm", "missed detection", "confusion")


def window_rates_from_counts(counts: dict) -> dict:
    """`window_counts` -> per window what `DiarizationErrorRate` makes of a file: (W,) float64 arrays `total`,
    `correct`, `false alarm`, `missed detection`, `confusion` and `diarization error rate`.  Every window has its
    own optimal mapping, found on the window's own matrix: the labels are compacted to those with a positive
    duration in the window (the labels a crop to the window would keep), and `optimal_mapping` -- SciPy on the
    host, W small matrices -- sees exactly the matrix it would see for the cropped file."""
    der = DiarizationErrorRate()
    W = len(counts["total"])
    table = {name: np.zeros(W) for name in _WINDOW_COMPONENTS + (der.metric_name(),)}
    for w in range(W):
        rows, columns = counts["ref_dur"][w] > 0, counts["hyp_dur"][w] > 0
        one = der.components_from_counts({"cooc": counts["cooc"][w][rows][:, columns],
                                          **{name: float(counts[name][w])
                                             for name in ("total", "false_alarm", "missed", "both")}})
        one[der.metric_name()] = der.compute_metric(one)
        for name, value in one.items():
            table[name][w] = value
    return table


def window_error_rates(reference: Annotation, hypothesis: Annotation, windows, uem=None, collar: float = 0.0,
                       skip_overlap: bool = False, device=None) -> dict:
    """The diarization error rate of every window of one file (`window_rates_from_counts` of `window_counts`).  On a
    `cuda` device the W mappings are found there as well (`device_window_rates`): the table is the same, value for
    value, and W x 5 numbers come back instead of the counts."""
    ref_labels, hyp_labels = _split(reference, uem)[0].labels(), hypothesis.labels()
    dev = _device(device) if len(ref_labels) <= MAX_LABELS and len(hyp_labels) <= MAX_LABELS else None
    if dev is None:
        return window_rates_from_counts(window_counts(reference, hypothesis, windows, uem=uem, collar=collar,
                                                      skip_overlap=skip_overlap, device=device))
    ref_labels, ref_seg, ref_lab, hyp_labels, hyp_seg, hyp_lab, uem_seg = _inputs(reference, hypothesis, uem, collar,
                                                                                  True)
    win_seg = _window_rows(windows)
    _check("windows", win_seg)
    Kr, Kh = len(ref_labels), len(hyp_labels)
    flat = device_window_counts(ref_seg, ref_lab, Kr, hyp_seg, hyp_lab, Kh, uem_seg, win_seg, collar, skip_overlap, dev)
    return device_window_rates(flat, Kr, Kh)


def device_window_rates(flat: torch.Tensor, Kr: int, Kh: int) -> dict:
    """`window_rates_from_counts` for the (W, Kr*Kh + Kr + Kh + 7) device tensor of `device_window_counts`, the W
    optimal mappings in ONE launch (`pa_lsap_batch`, csrc/lsap.hip): problem w is the (hypothesis, reference) view of
    its co-occurrence matrix, read through the strides, restricted to the labels with a positive duration in the
    window, maximised; its `total` -- the matched durations added in ascending hypothesis order, as the host adds
    them -- is `correct`.  One download of W x 5 numbers: total, false alarm, missed, both, correct."""
    from .distance import linear_sum_assignment_batch
    W, n0 = flat.shape[0], Kr * Kh
    scalars = flat[:, n0 + Kr + Kh:n0 + Kr + Kh + 4]
    if W and Kr and Kh:
        together = flat.as_strided((W, Kh, Kr), (flat.stride(0), 1, Kh))
        _, correct, status = linear_sum_assignment_batch(
            together, maximize=True, row_mask=flat[:, n0 + Kr:n0 + Kr + Kh] > 0, col_mask=flat[:, n0:n0 + Kr] > 0,
            return_total=True, check=False)
        correct = torch.where(status != 0, torch.full_like(correct, float("nan")), correct)
    else:
        correct = torch.zeros(W, dtype=torch.float64, device=flat.device)
    host = torch.cat([scalars, correct[:, None]], dim=1).cpu().numpy()
    total, false_alarm, missed, both, correct = (np.ascontiguousarray(host[:, k]) for k in range(5))
    if np.isnan(correct).any():      # (durations are finite: a refused matrix means the counts are not counts)
        raise ValueError(f"window {int(np.flatnonzero(np.isnan(correct))[0])}: the co-occurrence matrix is not finite")
    confusion = both - correct
    errors = false_alarm + missed + confusion
    with np.errstate(divide="ignore", invalid="ignore"):
        rate = np.where(total == 0, np.where(errors == 0, 0.0, 1.0), errors / total)
    return dict(zip(_WINDOW_COMPONENTS + (DiarizationErrorRate.metric_name(),),
                    (total, correct, false_alarm, missed, confusion, rate)))


class SlidingDiarizationErrorRate(BaseMetric):
    """The reference's `SlidingDiarizationErrorRate` (utils/metric.py:245-286): a window of `window` seconds slides
    over the `uem` with a step of half a window; every window is scored by a complete `DiarizationErrorRate` with
    its own optimal mapping, and the components are summed.  `metric(reference, hypothesis, uem=uem)`; `uem` is
    required.  All windows are counted in one call (`window_counts`; on `device` when it is a `cuda` device).
    Intervals are taken exactly (no 1e-6 rule), as everywhere in this module.  `windows(...)` returns the per-window
    table, which says WHERE in a file the errors are."""

    @classmethod
    def metric_name(cls):
        return "window diarization error rate"

    @classmethod
    def metric_components(cls):
        return ["total", "false alarm", "missed detection", "confusion"]

    def __init__(self, window: float = 10.0, device=None):
        super().__init__()
        self.window = window
        self.device = device

    def windows(self, reference, hypothesis, uem=None) -> dict:
        """-> `windows`, the list of `Segment`s, and per window the (W,) arrays of `window_error_rates`"""
        reference, uem = _split(reference, uem)
        if uem is None:
            raise ValueError("SlidingDiarizationErrorRate expects `uem` to be provided.")
        uem = _as_timeline(uem)
        chunks = list(SlidingWindow(duration=self.window, step=0.5 * self.window)(uem))
        table = window_error_rates(reference, hypothesis, chunks, uem=uem, device=self.device)
        return {"windows": chunks, **table}

    def compute_components(self, reference, hypothesis, uem=None, **kwargs) -> dict:
        table = self.windows(reference, hypothesis, uem=uem)
        # (added window after window from 0, as an accumulating `DiarizationErrorRate` adds them)
        return {name: sum(table[name].tolist()) for name in _WINDOW_COMPONENTS}

    def compute_metric(self, components):
        return (components["false alarm"] + components["missed detection"] + components["confusion"]) / \
            components["total"]


class JaccardErrorRate(_AnnotationMetric):
    """pyannote.metrics.diarization.JaccardErrorRate, restated from its published behaviour like its siblings
    (unpinned: pyannote.metrics was not at hand).  Speakers are mapped as for `DiarizationErrorRate`
    (`optimal_mapping`); every reference speaker with speech inside the evaluated region counts once, and its error
    is 1 when no hypothesis speaker is mapped to it, else (false alarm + missed) / (union) of the pair:
    fa = hyp_dur[j] - cooc[i, j], miss = ref_dur[i] - cooc[i, j], union = ref_dur[i] + hyp_dur[j] - cooc[i, j].
    The value is "speaker error" / "speaker count" (0 without a counted speaker).  `collar`, `skip_overlap`, `uem` and
    `device` as for `DiarizationErrorRate`."""

    @classmethod
    def metric_name(cls):
        return "jaccard error rate"

    @classmethod
    def metric_components(cls):
        return ["speaker count", "speaker error"]

    def components_from_counts(self, counts: dict) -> dict:
        cooc, ref_dur, hyp_dur = counts["cooc"], counts["ref_dur"], counts["hyp_dur"]
        mapped = {i: j for j, i in optimal_mapping(cooc).items()}
        count, error = 0, 0.0
        for i in range(len(ref_dur)):
            if not ref_dur[i] > 0:
                continue
            count += 1
            if i not in mapped:
                error += 1.0
                continue
            j = mapped[i]
            fa, miss = hyp_dur[j] - cooc[i, j], ref_dur[i] - cooc[i, j]
            total = ref_dur[i] + hyp_dur[j] - cooc[i, j]
            error += float((fa + miss) / total)
        return {"speaker count": count, "speaker error": error}

    def compute_metric(self, components):
        if components["speaker count"] == 0:
            return 0.0
        return float(components["speaker error"] / components["speaker count"])


class IdentificationErrorRate(_AnnotationMetric):
    """pyannote.metrics.identification.IdentificationErrorRate: labels are matched by name, no mapping"""

    @classmethod
    def metric_name(cls):
        return "identification error rate"

    @classmethod
    def metric_components(cls):
        return ["total", "correct", "false alarm", "missed detection", "confusion"]

    def components_from_counts(self, counts: dict) -> dict:
        column = {label: j for j, label in enumerate(counts["hyp_labels"])}
        correct = float(sum(counts["cooc"][i, column[label]] for i, label in enumerate(counts["ref_labels"])
                            if label in column))
        return {"total": counts["total"], "correct": correct, "false alarm": counts["false_alarm"],
                "missed detection": counts["missed"], "confusion": counts["both"] - correct}

    def compute_metric(self, components):
        return _error_rate(components)


class DetectionErrorRate(_AnnotationMetric):
    """pyannote.metrics.detection.DetectionErrorRate: (false alarm + miss) / total on speech / non-speech"""

    @classmethod
    def metric_name(cls):
        return "detection error rate"

    @classmethod
    def metric_components(cls):
        return ["total", "false alarm", "miss"]

    def components_from_counts(self, counts: dict) -> dict:
        return {"total": counts["ref_speech"], "false alarm": counts["hyp_speech"] - counts["both_speech"],
                "miss": counts["ref_speech"] - counts["both_speech"]}

    def compute_metric(self, components):
        errors = components["false alarm"] + components["miss"]
        if components["total"] == 0:
            return 0.0 if errors == 0 else 1.0
        return float(errors / components["total"])


class DetectionPrecisionRecallFMeasure(_AnnotationMetric):
    """pyannote.metrics.detection.DetectionPrecisionRecallFMeasure: the value is the F-measure of detected speech;
    `compute_metrics()` returns (precision, recall, f)"""

    @classmethod
    def metric_name(cls):
        return "F[precision|recall]"

    @classmethod
    def metric_components(cls):
        return ["retrieved", "relevant", "relevant retrieved"]

    def __init__(self, collar: float = 0.0, skip_overlap: bool = False, beta: float = 1.0, device=None, **kwargs):
        super().__init__(collar=collar, skip_overlap=skip_overlap, device=device, **kwargs)
        self.beta = beta

    def components_from_counts(self, counts: dict) -> dict:
        return {"retrieved": counts["hyp_speech"], "relevant": counts["ref_speech"],
                "relevant retrieved": counts["both_speech"]}

    def compute_metrics(self, components: Optional[dict] = None) -> tuple:
        """-> (precision, recall, f) of `components` (default: everything accumulated); a side without speech
        has precision / recall 1"""
        if components is None:
            components = self.accumulated_
        both = components["relevant retrieved"]
        precision = 1.0 if components["retrieved"] == 0 else float(both / components["retrieved"])
        recall = 1.0 if components["relevant"] == 0 else float(both / components["relevant"])
        if precision + recall == 0.0:
            return precision, recall, 0.0
        b2 = self.beta * self.beta
        return precision, recall, (1.0 + b2) * precision * recall / (b2 * precision + recall)

    def compute_metric(self, components):
        return self.compute_metrics(components)[2]


class MacroAverageFMeasure(BaseMetric):
    """Mean over `classes` of the detection F-measure of each class by itself (utils/metric.py:289-377): one
    `DetectionPrecisionRecallFMeasure` per class on the tracks of that class, a component per class."""

    @classmethod
    def metric_name(cls):
        return "Macro F-measure"

    def metric_components(self):
        return self.classes

    def __init__(self, classes: list, collar: float = 0.0, beta: float = 1.0, **kwargs):
        self.metric_name_ = self.metric_name()
        self.classes = classes
        self.components_ = set(self.metric_components())
        self.collar = collar
        self.beta = beta
        self._sub_metrics = {label: DetectionPrecisionRecallFMeasure(collar=collar, beta=beta, **kwargs)
                             for label in self.classes}
        self.reset()

    def reset(self):
        super().reset()
        for sub_metric in self._sub_metrics.values():
            sub_metric.reset()

    @staticmethod
    def _subset(annotation, label) -> Annotation:
        out = Annotation(uri=getattr(annotation, "uri", None))
        for segment, track, l in annotation.itertracks(yield_label=True):
            if l == label:
                out[segment, track] = l
        return out

    def compute_components(self, reference, hypothesis, uem=None, **kwargs) -> dict:
        reference, uem = _split(reference, uem)
        details = self.init_components()
        for label, sub_metric in self._sub_metrics.items():
            details[label] = sub_metric(self._subset(reference, label), self._subset(hypothesis, label), uem=uem,
                                        **kwargs)
        return details

    def compute_metric(self, detail: dict):
        return float(np.mean([detail[label] for label in self.classes]))

    def report(self) -> dict:
        """{uri: {class: F-measure of that file, ..., "Macro F-measure": ...}, ..., "TOTAL": {class: F-measure
        over everything accumulated, ...}} (the reference's data frame, as a dict)"""
        table = {uri: dict(components) for uri, components in self.results_}
        table["TOTAL"] = {label: abs(sub_metric) for label, sub_metric in self._sub_metrics.items()}
        table["TOTAL"][self.metric_name_] = abs(self)
        return table

    def __abs__(self):
        return float(np.mean([abs(sub_metric) for sub_metric in self._sub_metrics.values()]))
