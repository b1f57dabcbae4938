"""Frame-level diarization error rates, counted on the device.

Two families, both pinned to the reference's own code (tests/golden/make_metrics_golden.py):

* FILE MODE (utils/metric.py:41-242): `discrete_diarization_error_rate` and `DiscreteDiarizationErrorRate` on
  (frames, speakers) 0/1 arrays.  `pa_der_counts` takes the co-occurrence matrix and the mapping-independent sums
  in one pass over the frames; the optimal speaker mapping is a Hungarian assignment on the (at most 32 x 32)
  co-occurrence matrix on the host, and confusion = both - correct (identity: csrc/metrics.hip).
* CHUNK MODE (torchmetrics/functional/audio/diarization_error_rate.py, torchmetrics/audio/diarization_error_rate.py):
  `diarization_error_rate`, `optimal_diarization_error_rate` and the stateful classes, on (batch, speakers, frames)
  scores against 0/1 targets over up to 64 thresholds per launch (`pa_der_chunks`).

Counts are integers everywhere (int64 tensors / Python ints) and rates are float64 quotients of them.  The
reference sums in half precision (file mode: not every integer above 2048 is representable, and the total of a
one-hour file is `inf`) and in float32 through (batch, speakers, frames, thresholds) temporaries (chunk mode): it
is a valid yardstick only below those sizes, which is where the goldens are.

There is no host implementation of the counting: without a GPU every entry point raises (ffi.require_gpu)."""
from __future__ import annotations

from numbers import Number
from typing import Optional

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from . import ffi
from .core import HAVE_PYANNOTE_CORE, SEGMENT_PRECISION, Annotation, Segment, SlidingWindowFeature
from .permutation import permutate, permutate_batch  # noqa: F401  (`permutate` stays importable from here)
from .verification import EqualErrorRate  # noqa: F401  (the classification half of the reference's torchmetrics)

MAX_SPEAKERS = 32        # a frame's speakers travel as one 32-bit mask
MAX_THRESHOLDS = 64      # per launch; longer sweeps are split
AUTO_PERMUTATION = 4     # the chunk kernel enumerates the S! permutations itself up to here


if HAVE_PYANNOTE_CORE:  # pragma: no cover - exercised only where pyannote.core exists
    from pyannote.core import Timeline  # type: ignore
else:

    class Timeline:
        """Ordered set of segments: the subset of pyannote.core.Timeline that `uem` handling needs (iteration,
        `support`, `covers`), restated from its published behaviour."""

        def __init__(self, segments=None, uri=None):
            self.segments_ = sorted(s for s in (segments or []) if s)
            self.uri = uri

        def __iter__(self):
            return iter(self.segments_)

        def __len__(self):
            return len(self.segments_)

        def support(self) -> "Timeline":
            merged: list = []
            for s in self.segments_:
                if merged and s.start <= merged[-1].end:
                    merged[-1] = Segment(merged[-1].start, max(merged[-1].end, s.end))
                else:
                    merged.append(s)
            return Timeline(merged, uri=self.uri)

        def covers(self, other) -> bool:
            """every segment of `other` lies inside the support of this timeline"""
            mine = list(self.support())
            return all(any(m.start - SEGMENT_PRECISION <= s.start and s.end <= m.end + SEGMENT_PRECISION
                           for m in mine) for s in other)


def _as_timeline(uem) -> "Timeline":
    return uem if isinstance(uem, Timeline) else Timeline(list(uem))


# ----------------------------------------------------------------------------------------------- file mode
def _device_of(*arrays) -> torch.device:
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    ffi.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def _as_device_u8(x, device: torch.device) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    t = t.to(device)                               # (a tensor that already lies there is not copied)
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    elif t.dtype != torch.uint8:
        t = (t != 0).to(torch.uint8)
    return t.contiguous()


def der_counts(reference, hypothesis, keep=None) -> dict:
    """`pa_der_counts` on (frames, Sr) and (frames, Sh) 0/1 arrays (numpy, or torch tensors used where they lie);
    `keep` (frames,) marks the frames that count.  -> int64 numpy `cooc` (Sr, Sh), `ref_frames`, `hyp_frames` and
    Python ints `total`, `false_alarm`, `missed`, `both`."""
    dev = _device_of(hypothesis, reference, keep)
    ref, hyp = _as_device_u8(reference, dev), _as_device_u8(hypothesis, dev)
    if ref.ndim != 2 or hyp.ndim != 2 or ref.shape[0] != hyp.shape[0]:
        raise ValueError(f"expected (frames, speakers) arrays over the same frames, got {tuple(ref.shape)} and "
                         f"{tuple(hyp.shape)}")
    T = ref.shape[0]
    if ref.shape[1] == 0:                          # nobody ever speaks: one silent speaker
        ref = torch.zeros((T, 1), dtype=torch.uint8, device=dev)
    if hyp.shape[1] == 0:
        hyp = torch.zeros((T, 1), dtype=torch.uint8, device=dev)
    Sr, Sh = ref.shape[1], hyp.shape[1]
    if Sr > MAX_SPEAKERS or Sh > MAX_SPEAKERS:
        raise ValueError(f"at most {MAX_SPEAKERS} speakers per side are supported, got {Sr} and {Sh}")
    mask = None
    if keep is not None:
        mask = _as_device_u8(keep, dev).view(-1)
        if mask.shape[0] != T:
            raise ValueError(f"`keep` has {mask.shape[0]} frames, the arrays have {T}")
    out = torch.empty(Sr * Sh + Sr + Sh + 4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        ffi.check(ffi.load().pa_der_counts(ffi.ptr(ref), ffi.ptr(hyp), ffi.ptr(mask), T, Sr, Sh, ffi.ptr(out),
                                           ffi.stream()), "pa_der_counts")
    host = out.cpu().numpy()
    n = Sr * Sh
    total, false_alarm, missed, both = (int(v) for v in host[n + Sr + Sh:])
    return {"cooc": host[:n].reshape(Sr, Sh), "ref_frames": host[n:n + Sr], "hyp_frames": host[n + Sr:n + Sr + Sh],
            "total": total, "false_alarm": false_alarm, "missed": missed, "both": both}


def components_from_counts(counts: dict) -> dict:
    """Optimal one-to-one mapping on the host (the reference's `permutate` minimises the summed mean squared
    difference, which for 0/1 arrays is maximising the matched co-occurrence; every optimum has the same sum) and
    the reference's four components as Python ints."""
    cooc = np.asarray(counts["cooc"], dtype=np.int64)
    rows, cols = linear_sum_assignment(-cooc)
    correct = int(cooc[rows, cols].sum())
    return {"false alarm": int(counts["false_alarm"]), "missed detection": int(counts["missed"]),
            "confusion": int(counts["both"]) - correct, "total": int(counts["total"])}


def _rate(components: dict) -> float:
    """float64 quotient; an empty reference gives nan (no errors) or inf, as the reference's numpy division does"""
    errors = components["false alarm"] + components["missed detection"] + components["confusion"]
    total = components["total"]
    if total == 0:
        return float("nan") if errors == 0 else float("inf")
    return float(np.float64(errors) / np.float64(total))


def discrete_diarization_error_rate(reference, hypothesis):
    """utils/metric.py:41-93 on (num_frames, num_speakers) 0/1 arrays: numpy arrays or torch tensors (device
    tensors are used where they lie).  -> (der, components): components are Python ints under the reference's keys
    "false alarm", "missed detection", "confusion", "total"; der is their float64 quotient.  The side with fewer
    speakers counts as padded with silent ones (what `DiscreteDiarizationErrorRate` does before it calls the
    reference's function)."""
    components = components_from_counts(der_counts(reference, hypothesis))
    return _rate(components), components


class BaseMetric:
    """The accumulation protocol the reference's metric classes inherit from `pyannote.metrics.base.BaseMetric`.
    pyannote.metrics is not a dependency of this package: this is a restatement of its published behaviour (as
    the other `pyannote.*` stand-ins of this package are), not a copy pinned to its code.
    `metric(reference, hypothesis, detailed=False, uri=None, **kwargs)` computes the components of one file,
    accumulates them and returns the file's value (or all components); `abs(metric)` is the value over everything
    accumulated, `metric[:]` / `metric[name]` the accumulated components, `reset()` forgets them."""

    @classmethod
    def metric_name(cls) -> str:
        raise NotImplementedError(cls.__name__ + " is missing a 'metric_name' class method.")

    @classmethod
    def metric_components(cls) -> list:
        raise NotImplementedError(cls.__name__ + " is missing a 'metric_components' class method.")

    def __init__(self, **kwargs):
        self.metric_name_ = self.__class__.metric_name()
        self.components_ = set(self.__class__.metric_components())
        self.reset()

    def init_components(self) -> dict:
        return {name: 0 for name in self.components_}

    def reset(self):
        self.accumulated_ = self.init_components()
        self.results_: list = []

    @property
    def name(self) -> str:
        return self.metric_name()

    def __call__(self, reference, hypothesis, detailed: bool = False, uri: Optional[str] = None, **kwargs):
        components = self.compute_components(reference, hypothesis, **kwargs)
        components[self.metric_name_] = self.compute_metric(components)
        if uri is None:
            uri = getattr(reference, "uri", None) or "NA"
        self.add_components(components, uri)
        return components if detailed else components[self.metric_name_]

    def add_components(self, components: dict, uri: str):
        """accumulates one file's components (with the file's value under the metric's name), computed anywhere"""
        self.results_.append((uri, components))
        for name in self.components_:
            self.accumulated_[name] += components[name]

    def __abs__(self):
        return self.compute_metric(self.accumulated_)

    def __getitem__(self, component):
        if component == slice(None, None, None):
            return dict(self.accumulated_)
        return self.accumulated_[component]

    def __iter__(self):
        return iter(self.results_)

    def compute_components(self, reference, hypothesis, **kwargs) -> dict:
        raise NotImplementedError

    def compute_metric(self, components: dict):
        raise NotImplementedError


class DiscreteDiarizationErrorRate(BaseMetric):
    """Diarization error rate on discretized annotations (utils/metric.py:96-242), counted on the device.

    `metric(reference, hypothesis, uem=None)` dispatches on the hypothesis as the reference does:
      * a (frames, speakers) array pair (numpy or torch; `uem` refused); the side with fewer speakers is padded;
      * a `SlidingWindowFeature` with 2-D data against an `Annotation`: the annotation is discretized on the
        hypothesis' extent and frames; `uem` (a `Timeline` or an iterable of `Segment`) must be covered by the extent;
      * a `SlidingWindowFeature` with 3-D per-chunk data: one error count per chunk with its own mapping, chunks that
        `uem` does not fully cover are skipped.
    `hypothesis.data` may be a device tensor (the pipeline's `discrete_diarization` moved or left on the GPU): it is
    not copied down.

    Two deliberate differences in the 2-D path.  The reference scores every `uem` segment by itself, each with its own
    speaker mapping, on loosely cropped frames (a frame on the border of two segments counts twice); here the `uem`
    becomes the kernel's frame mask and ONE mapping serves the file, which is what a file-level error rate means.
    And where `Annotation.discretize` yields a frame or two more than the hypothesis has (it does whenever the frame
    duration differs from the frame step) the reference raises; here the common frames are scored, as the reference's
    own 3-D path does.  The base-class protocol is a restatement of pyannote.metrics' published behaviour (see
    `BaseMetric`); only the component arithmetic is pinned to the reference's code."""

    @classmethod
    def metric_name(cls):
        return "discrete diarization error rate"

    @classmethod
    def metric_components(cls):
        return ["total", "false alarm", "missed detection", "confusion"]

    def compute_components(self, reference, hypothesis, uem=None):
        return self.compute_components_helper(hypothesis, reference, uem=uem)

    def compute_components_helper(self, hypothesis, reference, uem=None):
        if isinstance(hypothesis, SlidingWindowFeature):
            return self.der_from_swf(hypothesis, reference, uem=uem)
        if isinstance(hypothesis, (np.ndarray, torch.Tensor)):
            return self.der_from_ndarray(hypothesis, reference, uem=uem)
        klass = hypothesis.__class__.__name__
        raise NotImplementedError(f"Providing hypothesis as {klass} instances is not supported.")

    def der_from_ndarray(self, hypothesis, reference, uem=None, keep=None):
        if reference.ndim != 2:
            raise NotImplementedError("Only (num_frames, num_speakers)-shaped reference is supported.")
        if uem is not None:
            raise ValueError("`uem` is not supported with numpy arrays.")
        if hypothesis.ndim != 2:
            raise NotImplementedError("Only (num_frames, num_speakers)-shaped hypothesis is supported.")
        if reference.shape[0] != hypothesis.shape[0]:
            raise ValueError("reference and hypothesis must have the same number of frames.")
        # the reference pads the narrower side with silent speakers (:154-161); silent speakers add nothing to any
        # count, so the kernel takes the two widths as they are
        return components_from_counts(der_counts(reference, hypothesis, keep=keep))

    def der_from_swf(self, hypothesis: SlidingWindowFeature, reference: Annotation, uem=None):
        data = hypothesis.data
        ndim = data.ndim
        if ndim < 2 or ndim > 3:
            raise NotImplementedError(
                "Only (num_frames, num_speakers) or (num_chunks, num_frames, num_speakers)-shaped "
                "hypothesis is supported.")
        if uem is not None:
            uem = _as_timeline(uem)

        if ndim == 2:
            support = hypothesis.extent
            resolution = hypothesis.sliding_window
        else:
            chunks = hypothesis.sliding_window
            num_chunks, num_frames, _ = data.shape
            support = Segment(chunks[0].start, chunks[num_chunks - 1].end)
            resolution = chunks.duration / num_frames

        reference = reference.discretize(support, resolution=resolution)

        if ndim == 2:
            common = min(data.shape[0], reference.data.shape[0])
            keep = None
            if uem is not None:
                if not Timeline([support]).covers(uem):
                    raise ValueError("`uem` must fully cover hypothesis extent.")
                keep = np.zeros(common, dtype=np.uint8)
                for segment in uem:
                    for first, stop in hypothesis.sliding_window.crop(segment, mode="loose", return_ranges=True):
                        keep[max(first, 0):max(min(stop, common), 0)] = 1
            return self.der_from_ndarray(data[:common], reference.data[:common], keep=keep)

        components = self.init_components()
        for i in range(num_chunks):
            window = chunks[i]
            # skip any window not fully covered by a segment of the uem
            if uem is not None and not uem.covers(Timeline([window])):
                continue
            reference_window = reference.crop(window, mode="center")
            common = min(num_frames, reference_window.shape[0])
            window_components = self.der_from_ndarray(data[i][:common], reference_window[:common])
            for name in self.components_:
                components[name] += window_components[name]
        return components

    def compute_metric(self, components):
        return _rate(components)


# ---------------------------------------------------------------------------------------------- chunk mode
def chunk_workspace_bytes(batch_size: int, num_thresholds: int) -> int:
    """scratch of a batch-reduced `diarization_error_rate` call per launch of at most 64 thresholds: the per-chunk
    int32 tables, 4 B (3 Q + 1) bytes whatever the number of frames (pa_der_chunks_workspace_bytes)"""
    return int(ffi.load().pa_der_chunks_workspace_bytes(int(batch_size), int(num_thresholds)))


def _der_update(preds: torch.Tensor, target: torch.Tensor, threshold=0.5, reduce: str = "batch"):
    """Components of the diarization error rate (functional/audio/diarization_error_rate.py:33-162): int64 tensors
    on `preds.device`.  `reduce="batch"`: (num_thresholds,) false alarm, missed detection, confusion and a scalar
    speech total; `reduce="chunk"`: (batch_size, num_thresholds) and (batch_size,).  A scalar threshold drops the
    last axis."""
    prd_batch_size, prd_num_speakers, prd_num_frames = preds.shape
    tgt_batch_size, tgt_num_speakers, tgt_num_frames = target.shape
    if prd_batch_size != tgt_batch_size:
        raise ValueError(f"Batch size mismatch: {prd_batch_size} != {tgt_batch_size}.")
    if prd_num_frames != tgt_num_frames:
        raise ValueError(f"Number of frames mismatch: {prd_num_frames} != {tgt_num_frames}.")
    if reduce == "frame":
        raise NotImplementedError('reduce="frame" is not implemented: the kernel never holds per-frame counts '
                                  '(use reduce="chunk" or "batch")')
    if reduce not in ("batch", "chunk"):
        raise ValueError(f"reduce must be 'batch' or 'chunk', got {reduce!r}")

    home = preds.device
    dev = _device_of(preds, target)
    preds = preds.detach().to(dev, torch.float32)
    target = target.detach().to(dev)
    if target.dtype == torch.bool:
        target = target.to(torch.uint8)
    elif target.dtype not in (torch.uint8, torch.float32):
        target = (target != 0).to(torch.uint8)
    # pad number of speakers if necessary (:78-82)
    if prd_num_speakers > tgt_num_speakers:
        target = torch.nn.functional.pad(target, (0, 0, 0, prd_num_speakers - tgt_num_speakers))
    elif prd_num_speakers < tgt_num_speakers:
        preds = torch.nn.functional.pad(preds, (0, 0, 0, tgt_num_speakers - prd_num_speakers))
    preds, target = preds.contiguous(), target.contiguous()
    B, S, F = preds.shape
    if S > MAX_SPEAKERS:
        raise ValueError(f"at most {MAX_SPEAKERS} speakers are supported, got {S}")
    if S < 1 or F < 1:
        raise ValueError(f"expected at least one speaker and one frame, got {S} and {F}")

    scalar_threshold = isinstance(threshold, Number)
    if scalar_threshold:
        thresholds = torch.tensor([threshold], dtype=torch.float32)
    else:
        thresholds = torch.as_tensor(threshold).detach().to(torch.float32).reshape(-1)
    thresholds = thresholds.to(dev).contiguous()
    Q = thresholds.shape[0]

    perm = None
    if S > AUTO_PERMUTATION and B > 0:
        # larger speaker sets: the Hungarian `permutate` (:90-92), on the tensors as they lie (`permutate_batch`:
        # the costs, SciPy's assignment and nothing downloaded)
        _, perm = permutate_batch(target.to(torch.float32).transpose(1, 2), preds.transpose(1, 2))

    lib = ffi.load()
    is_f32 = int(target.dtype == torch.float32)
    pieces = []
    with torch.cuda.device(dev):
        for q0 in range(0, Q, MAX_THRESHOLDS):
            thr = thresholds[q0:q0 + MAX_THRESHOLDS]
            q = thr.shape[0]
            if reduce == "batch":
                work = torch.empty(int(lib.pa_der_chunks_workspace_bytes(B, q)) // 4, dtype=torch.int32, device=dev)
                counts, total = work[:B * 3 * q], work[B * 3 * q:]
            else:
                counts = torch.empty((B, q, 3), dtype=torch.int32, device=dev)
                total = torch.empty(B, dtype=torch.int32, device=dev)
            ffi.check(lib.pa_der_chunks(ffi.ptr(preds), ffi.ptr(target), is_f32, B, S, F, ffi.ptr(thr), q,
                                        ffi.ptr(perm), ffi.ptr(counts), ffi.ptr(total), ffi.stream()),
                      "pa_der_chunks")
            if reduce == "batch":
                sums = torch.empty(3 * q + 1, dtype=torch.int64, device=dev)
                ffi.check(lib.pa_der_chunks_sum(ffi.ptr(counts), ffi.ptr(total), B, q, ffi.ptr(sums), ffi.stream()),
                          "pa_der_chunks_sum")
                pieces.append((sums[:3 * q].view(q, 3), sums[3 * q]))
            else:
                pieces.append((counts.to(torch.int64), total.to(torch.int64)))
    if len(pieces) == 1:
        table, speech_total = pieces[0]
    else:
        table, speech_total = torch.cat([p[0] for p in pieces], dim=-2), pieces[0][1]
    false_alarm, missed_detection, speaker_confusion = table[..., 0], table[..., 1], table[..., 2]
    if scalar_threshold:
        false_alarm, missed_detection, speaker_confusion = (x[..., 0] for x in
                                                            (false_alarm, missed_detection, speaker_confusion))
    return tuple(x.to(home) for x in (false_alarm, missed_detection, speaker_confusion, speech_total))


def _der_compute(false_alarm, missed_detection, speaker_confusion, speech_total) -> torch.Tensor:
    """(false alarm + missed detection + confusion) / (total + 1e-8) (:165-187) as a float64 quotient of the integer
    counts; a per-chunk total divides every threshold of its chunk"""
    errors = (false_alarm + missed_detection + speaker_confusion).to(torch.float64)
    total = torch.as_tensor(speech_total).to(torch.float64)
    if total.ndim and total.ndim < errors.ndim:
        total = total.unsqueeze(-1)
    return errors / (total + 1e-8)


def diarization_error_rate(preds: torch.Tensor, target: torch.Tensor, threshold=0.5, reduce: str = "batch",
                           return_components: bool = False):
    """Diarization error rate of (batch_size, num_speakers, num_frames) scores against 0/1 targets
    (functional/audio/diarization_error_rate.py:190-232).  `threshold`: a number or a tensor of thresholds;
    `reduce`: "batch" -> (num_thresholds,), "chunk" -> (batch_size, num_thresholds); a scalar threshold drops the
    last axis.  `reduce="frame"` is refused.  With `return_components` also the int64 (false_alarm,
    missed_detection, speaker_confusion, speech_total)."""
    components = _der_update(preds, target, threshold=threshold, reduce=reduce)
    der = _der_compute(*components)
    if return_components:
        return der, components
    return der


def _default_thresholds() -> torch.Tensor:
    return torch.linspace(0.0, 1.0, 51)            # (on the host: the values the reference's default has there)


def optimal_diarization_error_rate(preds: torch.Tensor, target: torch.Tensor,
                                   threshold: Optional[torch.Tensor] = None):
    """-> (optimal error rate, the threshold that reaches it) over `threshold` (default torch.linspace(0, 1, 51));
    functional/audio/diarization_error_rate.py:235-262.  A tensor `threshold` is accepted (the reference's
    `threshold or ...` raises for one)."""
    threshold = _default_thresholds() if threshold is None else torch.as_tensor(threshold)
    threshold = threshold.to(preds.device)
    der = diarization_error_rate(preds, target, threshold=threshold)
    opt_der, opt_threshold_idx = torch.min(der, dim=0)
    return opt_der, threshold[opt_threshold_idx]


class DiarizationErrorRate:
    """Stateful diarization error rate at one threshold (torchmetrics/audio/diarization_error_rate.py:35-100):
    `update(preds, target)` accumulates int64 counts on the device of the first batch, `compute()` returns the rate
    over everything seen, `reset()` forgets it.  Not a `torchmetrics.Metric` (torchmetrics is not a dependency):
    the three methods are the protocol."""

    higher_is_better = False
    is_differentiable = False
    _states = ("false_alarm", "missed_detection", "speaker_confusion", "speech_total")

    def __init__(self, threshold: float = 0.5):
        self.threshold = threshold
        self.reset()

    def reset(self):
        for name in self._states:
            setattr(self, name, torch.zeros((), dtype=torch.int64))

    def _accumulate(self, values):
        for name, value in zip(self._states, values):
            setattr(self, name, getattr(self, name).to(value.device) + value)

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        self._accumulate(_der_update(preds, target, threshold=self.threshold))

    def __call__(self, preds, target):
        self.update(preds, target)
        return self.compute()

    def compute(self):
        return _der_compute(self.false_alarm, self.missed_detection, self.speaker_confusion, self.speech_total)

    def _total(self):
        return self.speech_total.to(torch.float64) + 1e-8


class SegmentationErrorRate(DiarizationErrorRate):
    """Local diarization error rate on sliding windows of `window_size` frames (:103-163)"""

    def __init__(self, window_size: int, step_size: Optional[int] = None, threshold: float = 0.5):
        super().__init__(threshold=threshold)
        self.window_size = window_size
        self.step_size = step_size or window_size // 2

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        _, _, num_frames = preds.shape
        if num_frames > self.window_size:
            # "b s c f -> (b c) s f"
            preds, target = (x.unfold(2, self.window_size, self.step_size).permute(0, 2, 1, 3)
                             .reshape(-1, x.shape[1], self.window_size) for x in (preds, target))
        super().update(preds, target)


class SpeakerConfusionRate(DiarizationErrorRate):
    def compute(self):
        return self.speaker_confusion.to(torch.float64) / self._total()


class DiarizationPrecision(DiarizationErrorRate):
    """correctly identified speech over correctly detected speech"""
    higher_is_better = True

    def compute(self):
        detected = (self.speech_total - self.missed_detection).to(torch.float64)
        return (detected - self.speaker_confusion.to(torch.float64)) / (detected + 1e-8)


class DiarizationRecall(DiarizationErrorRate):
    """correctly identified speech over total speech"""
    higher_is_better = True

    def compute(self):
        detected = (self.speech_total - self.missed_detection).to(torch.float64)
        return (detected - self.speaker_confusion.to(torch.float64)) / self._total()


class FalseAlarmRate(DiarizationErrorRate):
    def compute(self):
        return self.false_alarm.to(torch.float64) / self._total()


class MissedDetectionRate(DiarizationErrorRate):
    def compute(self):
        return self.missed_detection.to(torch.float64) / self._total()


class DetectionErrorRate(DiarizationErrorRate):
    def compute(self):
        return (self.false_alarm + self.missed_detection).to(torch.float64) / self._total()


class OptimalDiarizationErrorRate:
    """Stateful error rate swept over thresholds (default torch.linspace(0, 1, 51)); `compute()` is the smallest
    (:274-361).  States carry the reference's names (CamelCase for per-threshold ones)."""

    higher_is_better = False
    is_differentiable = False

    def __init__(self, threshold: Optional[torch.Tensor] = None):
        self.threshold = _default_thresholds() if threshold is None else torch.as_tensor(threshold).reshape(-1)
        self.reset()

    def reset(self):
        (num_thresholds,) = self.threshold.shape
        self.FalseAlarm = torch.zeros(num_thresholds, dtype=torch.int64)
        self.MissedDetection = torch.zeros(num_thresholds, dtype=torch.int64)
        self.SpeakerConfusion = torch.zeros(num_thresholds, dtype=torch.int64)
        self.speech_total = torch.zeros((), dtype=torch.int64)

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        values = _der_update(preds, target, threshold=self.threshold)
        for name, value in zip(("FalseAlarm", "MissedDetection", "SpeakerConfusion", "speech_total"), values):
            setattr(self, name, getattr(self, name).to(value.device) + value)

    def __call__(self, preds, target):
        self.update(preds, target)
        return self.compute()

    def _der(self):
        return _der_compute(self.FalseAlarm, self.MissedDetection, self.SpeakerConfusion, self.speech_total)

    def _at_optimum(self, per_threshold: torch.Tensor):
        _, opt_threshold_idx = torch.min(self._der(), dim=0)
        return per_threshold[opt_threshold_idx].to(torch.float64) / (self.speech_total.to(torch.float64) + 1e-8)

    def compute(self):
        opt_der, _ = torch.min(self._der(), dim=0)
        return opt_der


class OptimalDiarizationErrorRateThreshold(OptimalDiarizationErrorRate):
    def compute(self):
        der = self._der()
        _, opt_threshold_idx = torch.min(der, dim=0)
        return self.threshold.to(der.device)[opt_threshold_idx]


class OptimalSpeakerConfusionRate(OptimalDiarizationErrorRate):
    def compute(self):
        return self._at_optimum(self.SpeakerConfusion)


class OptimalFalseAlarmRate(OptimalDiarizationErrorRate):
    def compute(self):
        return self._at_optimum(self.FalseAlarm)


class OptimalMissedDetectionRate(OptimalDiarizationErrorRate):
    def compute(self):
        return self._at_optimum(self.MissedDetection)
