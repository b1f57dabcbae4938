"""`apply_batch` of the detection pipelines (VoiceActivityDetection, MultiLabelSegmentation): a list of files in packed
launches.

`pack=False` (the default) is the per-file loop `Pipeline._apply_batch` runs for a pipeline without `apply_batch`.
With `pack`, consecutive files form groups by a chunk budget (`pipelining.PackGrouper`), and a group is

    SegmentationEngine.forward_files      the chunks of all files in shared launch groups
    frames.aggregate_files                one launch: overlap-add of every file (VAD: max over speakers first)
    frames.binarize_regions_files         one pass: the region lists of every (file, class)
    one copy of the packed rows, one of the offset table, then the Annotations (`regions_to_annotation`)

Every file's Annotation is the one `apply(file)` returns.  What the packed route cannot reproduce takes the per-file
loop instead (`_pack_budget`); a pipeline says what it needs through `_packed_detector`."""
from __future__ import annotations

from typing import Callable, Iterable, Iterator, List, Optional, Tuple

import torch

from .audio import Audio, AudioFile
from .core import Annotation, SlidingWindow
from .pipelining import PackGrouper


class PackedDetection:
    """Mixin of a detection `Pipeline` with a sliding `self._segmentation` Inference.  The pipeline provides
    `_packed_detector()` -> None (this pipeline, as configured, takes the per-file loop) or a dict:
        any             collapse the chunk scores to one class, the maximum over the columns, before aggregation
        hard            aggregate the uint8 hard multilabel output of a powerset model (else the float32 scores)
        onset, offset, min_duration_on, min_duration_off    per class, or scalars
        classes         the label of every class"""

    #: apply_batch(pack=...): the URIs of every group of the last call; empty where it took the per-file loop
    last_pack_groups: list = []

    def _packed_detector(self) -> Optional[dict]:
        raise NotImplementedError()

    def _pack_budget(self, pack, hook, files: List[dict]) -> Optional[int]:
        """chunks per group of `apply_batch(pack=...)`, or None where the call takes the per-file loop"""
        if pack is False or pack is None:
            return None
        inference = self._segmentation
        engine = getattr(inference.model, "engine", None)
        budget = getattr(engine, "max_chunks", 0) if pack is True else int(pack)
        if budget < 1:
            raise ValueError(f"pack must be True, False or a positive number of chunks (got {pack!r})")
        if hook is not None or self.training or any(f.get("pipeline_kwargs") for f in files):
            return None
        if not getattr(engine, "PACKS_FILES", False):
            return None
        if inference.window != "sliding" or inference.skip_aggregation:
            return None
        return budget

    def _detect_group(self, files: List[dict], waveforms: List[torch.Tensor], detector: dict) -> List[Annotation]:
        """one group: the Annotations of `files`, whose (1, samples) waveforms are loaded"""
        from . import frames as frame_ops
        from .multilabel import regions_to_annotation
        inference = self._segmentation
        model = inference.model
        sample_rate = model.audio.sample_rate
        window = model.audio.get_num_samples(inference.duration)
        step = round(inference.step * sample_rate)
        counts, chunk0, row0, T = frame_ops.files_layout([w.shape[1] for w in waveforms], inference)
        wavs = [w.to(model.device, torch.float32).contiguous().view(-1) for w in waveforms]
        hard = detector["hard"]
        logp, multilabel = model.engine.forward_files(wavs, step, counts.tolist(), window, want_logp=not hard,
                                                      want_multilabel=hard)
        scores, frames = frame_ops.aggregate_files(
            multilabel if hard else logp, chunk0, row0, T,
            SlidingWindow(start=0.0, duration=inference.duration, step=inference.step), model.receptive_field,
            any=detector["any"], warm_up=inference.warm_up, hamming=True, missing=0.0, packed=True)
        regions, positions = frame_ops.binarize_regions_files(
            scores, row0, T, frames, detector["onset"], detector["offset"], detector["min_duration_on"],
            detector["min_duration_off"], return_tracks=True)
        return [regions_to_annotation(r, p, detector["classes"], file["uri"])
                for file, r, p in zip(files, regions, positions)]

    def apply_batch(self, files: Iterable[AudioFile], hook: Optional[Callable] = None, pack=False,
                    **kwargs) -> Iterator[Tuple[AudioFile, Annotation]]:
        """Several files (`Pipeline.__call__` routes lists here) -> (file, Annotation) pairs in input order.

        `pack=False`: `apply` file by file, each with its own `pipeline_kwargs`.  `pack=True` (the segmentation
        engine's `max_chunks`) or a number of chunks: consecutive files share launches while their chunks together
        stay within that budget, a larger file is a group of its own; `last_pack_groups` lists the URIs of every
        group.  Every file's Annotation equals `apply(file)`.  The call takes the per-file loop after all -- and
        `last_pack_groups` stays empty -- with a hook, in training mode, when a file carries `pipeline_kwargs`, with
        an engine that does not pack files, with `window="whole"` or `skip_aggregation`, and where the pipeline's
        own configuration asks for it (`_packed_detector`)."""
        files = [Audio.validate_file(f) for f in files]
        self.last_pack_groups = []
        budget = self._pack_budget(pack, hook, files)
        detector = self._packed_detector() if budget is not None else None
        if detector is None:
            if hook is not None:
                kwargs = {"hook": hook, **kwargs}
            for file in files:
                yield file, self.apply(file, **file.get("pipeline_kwargs", {}), **kwargs)
            return
        if kwargs:
            raise TypeError(f"apply() got an unexpected keyword argument {sorted(kwargs)[0]!r}")
        inference = self._segmentation
        audio = Audio(inference.model.audio.sample_rate, mono="downmix", device=inference.device)
        window = inference.model.audio.get_num_samples(inference.duration)
        step = round(inference.step * inference.model.audio.sample_rate)

        def finish(group):
            self.last_pack_groups.append([file["uri"] for file, _ in group])
            outs = self._detect_group([file for file, _ in group], [w for _, w in group], detector)
            return [(file, out) for (file, _), out in zip(group, outs)]

        # a file's chunk count is known once it is loaded, so the groups form while the files arrive
        grouper, loaded = PackGrouper(budget), []
        for file in files:
            waveform, _ = audio(file)
            n_full, has_last = inference.num_chunks(waveform.shape[1], window, step)
            if grouper.add(n_full + has_last) is not None:
                yield from finish(loaded)
                loaded = []
            loaded.append((file, waveform))
        if grouper.flush():
            yield from finish(loaded)
