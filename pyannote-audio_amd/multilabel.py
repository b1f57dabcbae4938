"""Multi-label segmentation pipeline (mirrors pipelines/multilabel.py:44-229): one hysteresis detector per class of
a multi-label model (speech / music / noise, child / adult / ...).

The reference binarizes the aggregated scores class by class in Python (`Binarize`, utils/signal.py:254-318, then
`Annotation.support` and the min_duration_on deletion).  Here everything after the model stays on the device: the
chunk scores are aggregated by `pa_aggregate` without leaving HBM (`Inference.slide_device`), and one call of
`pa_binarize_regions` (csrc/regions.hip) turns the (frames, classes) aggregate into the region lists of all classes
-- the reference's state-dependent rule, including `offset > onset`, which `diarization.Binarize` does not follow.
Only the region lists are copied to the host; the aggregated scores are copied down when a hook asks for them (or in
training mode, where they are cached)."""
from __future__ import annotations

from itertools import islice
from typing import Callable, Optional

import numpy as np
import torch

from .audio import Audio, AudioFile
from .core import Annotation, SlidingWindowFeature, string_generator
from .detection_batch import PackedDetection
from .inference import Inference
from .model import Problem, Resolution
from .pipeline import ParamDict, Pipeline, Uniform
from .speaker_verification import PipelineModel, get_model


def regions_to_annotation(regions, positions, classes, uri) -> Annotation:
    """per-class region lists (n_k, 2) and track positions -> the Annotation `Binarize` gives class by class"""
    # track names as Binarize / support leave them: each class is binarized on its own, so its tracks restart
    # from the first generated name; `support` (min_duration_off > 0) names the merged regions in time order
    # before the short ones are deleted, otherwise every region keeps the class's single track name
    num_names = 1 + max((int(p.max()) for p in positions if len(p)), default=0)
    names = np.array(list(islice(string_generator(), num_names)), dtype=object)
    tracks = np.concatenate([names[p] for p in positions]).tolist()
    labels = np.repeat(np.array(classes, dtype=object), [len(r) for r in regions]).tolist()
    times = np.concatenate(regions)
    if hasattr(Annotation, "from_columns"):
        return Annotation.from_columns(times[:, 0], times[:, 1], tracks, labels, uri=uri)
    # the real pyannote.core.Annotation (re-exported by core.py when it is importable) has no columnar constructor
    from .core import Segment
    detection = Annotation(uri=uri)
    for (start, end), track, label in zip(times.tolist(), tracks, labels):
        detection[Segment(start, end), track] = label
    return detection


class MultiLabelSegmentation(PackedDetection, Pipeline):
    """Hyper-parameters: `thresholds[label]` = onset, offset [, min_duration_on, min_duration_off]; the two
    durations are top-level and shared between labels when `share_min_duration`.

    A list of files goes through `apply_batch` (detection_batch.py): `pipeline(files, pack=True)` runs short files in
    shared launches, with the Annotations of `apply`."""

    CACHED_SEGMENTATION = "cache/segmentation"

    def __init__(self, segmentation: PipelineModel = None, fscore: bool = False, share_min_duration: bool = False,
                 token=None, cache_dir=None, **inference_kwargs):
        super().__init__()
        if segmentation is None:
            raise ValueError("MultiLabelSegmentation pipeline must be provided with a `segmentation` model.")
        self.segmentation = segmentation
        self.fscore = fscore
        self.share_min_duration = share_min_duration
        model = get_model(segmentation, token=token, cache_dir=cache_dir)
        specifications = model.specifications
        if specifications.powerset:
            raise ValueError("MultiLabelSegmentation is the pipeline of multi-label models (one sigmoid score per "
                             "class); this checkpoint is a powerset (multi-class) model: use SpeakerDiarization or "
                             "VoiceActivityDetection.")
        if specifications.problem not in (Problem.MULTI_LABEL_CLASSIFICATION, Problem.BINARY_CLASSIFICATION) \
                or specifications.resolution != Resolution.FRAME:
            raise ValueError("MultiLabelSegmentation needs a frame-level multi-label model, got "
                             f"{specifications.problem} at {specifications.resolution} resolution.")
        if specifications.permutation_invariant:
            raise ValueError("the classes of a permutation-invariant model have no identity across chunks: its "
                             "scores cannot be aggregated class by class.")
        self._classes = list(specifications.classes)
        self._segmentation = Inference(model, **inference_kwargs)
        if share_min_duration:
            self.min_duration_on = Uniform(0.0, 2.0)
            self.min_duration_off = Uniform(0.0, 2.0)
            self.thresholds = ParamDict(**{
                label: ParamDict(onset=Uniform(0.0, 1.0), offset=Uniform(0.0, 1.0)) for label in self._classes})
        else:
            self.thresholds = ParamDict(**{
                label: ParamDict(onset=Uniform(0.0, 1.0), offset=Uniform(0.0, 1.0),
                                 min_duration_on=Uniform(0.0, 2.0), min_duration_off=Uniform(0.0, 2.0))
                for label in self._classes})

    def classes(self):
        return self._classes

    def initialize(self):
        """per-class arrays handed to the kernel; `Binarize.__init__` semantics (`offset or onset`)"""
        per_label = [self.thresholds[label] for label in self._classes]
        self._onset = np.array([t["onset"] for t in per_label], dtype=np.float64)
        self._offset = np.array([t["offset"] or t["onset"] for t in per_label], dtype=np.float64)
        if self.share_min_duration:
            self._min_duration_on = np.full(len(per_label), self.min_duration_on, dtype=np.float64)
            self._min_duration_off = np.full(len(per_label), self.min_duration_off, dtype=np.float64)
        else:
            self._min_duration_on = np.array([t["min_duration_on"] for t in per_label], dtype=np.float64)
            self._min_duration_off = np.array([t["min_duration_off"] for t in per_label], dtype=np.float64)

    def _packed_detector(self) -> Optional[dict]:
        """what `apply_batch(pack=...)` runs for a group of files, None: the per-file loop (a pre-aggregation hook is
        host code between the network and the aggregation)"""
        if self._segmentation.pre_aggregation_hook is not None:
            return None
        if not hasattr(self, "_onset"):
            self.initialize()
        return {"any": False, "hard": False, "onset": self._onset, "offset": self._offset,
                "min_duration_on": self._min_duration_on, "min_duration_off": self._min_duration_off,
                "classes": self._classes}

    def _aggregate(self, file: AudioFile, hook: Callable):
        """-> (frames, classes) float32 device tensor, frame grid"""
        inference = self._segmentation
        progress = (lambda **kw: hook("segmentation", None, **kw))
        if inference.window == "sliding" and inference.pre_aggregation_hook is None and not inference.skip_aggregation:
            waveform, sample_rate = Audio(inference.model.audio.sample_rate, mono="downmix",
                                          device=inference.device)(file)
            return inference.slide_device(waveform, sample_rate, hook=progress)
        # a pre-aggregation hook is host code: its result is aggregated as `Inference` does it, then sent back
        scores = inference(file, hook=progress)
        return self._upload(scores)

    def _upload(self, scores: SlidingWindowFeature):
        data = torch.from_numpy(np.ascontiguousarray(scores.data, dtype=np.float32))
        return data.to(self._segmentation.model.device), scores.sliding_window

    def apply(self, file: AudioFile, hook: Optional[Callable] = None) -> Annotation:
        """-> detected regions, labelled with the class names (pipelines/multilabel.py:156-216)"""
        wants_scores = hook is not None or self.training
        hook = self.setup_hook(file, hook=hook)
        if not hasattr(self, "_onset"):
            self.initialize()
        host_scores = None
        if self.training and self.CACHED_SEGMENTATION in file:
            host_scores = file[self.CACHED_SEGMENTATION]
            scores, frames = self._upload(host_scores)
        else:
            scores, frames = self._aggregate(file, hook)
            if wants_scores:
                host_scores = SlidingWindowFeature(scores.cpu().numpy(), frames)
            if self.training:
                file[self.CACHED_SEGMENTATION] = host_scores
        hook("segmentation", host_scores)

        return self._detect(scores, frames, file["uri"])

    def _detect(self, scores: torch.Tensor, frames, uri) -> Annotation:
        """aggregated (frames, classes) device scores -> Annotation: one kernel call, one copy of the region lists"""
        from . import frames as frame_ops
        regions, positions = frame_ops.binarize_regions(
            scores, frames, self._onset, self._offset, self._min_duration_on, self._min_duration_off,
            return_tracks=True)
        return regions_to_annotation(regions, positions, self._classes, uri)

    def get_metric(self):
        raise NotImplementedError(
            "MultiLabelSegmentation.get_metric returns pyannote.metrics' IdentificationErrorRate (or "
            "MacroAverageFMeasure with fscore=True): pyannote.metrics is not installed; its restatements "
            "`annotation_metrics.IdentificationErrorRate` and `annotation_metrics.MacroAverageFMeasure` are "
            "available stand-alone.")

    def get_direction(self):
        return "maximize" if self.fscore else "minimize"
