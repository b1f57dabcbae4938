"""Speaker-embedding extractor as the diarization pipeline sees it: the b3 interface of SURVEY.md
section 8b (pipelines/speaker_verification.py:622-778; model resolution pipelines/utils/getter.py:74-136).

Contract kept: `extractor(waveforms (B,1,N), masks (B,F) | None) -> (B, D) float32 ndarray`, `.to(device)`
(TypeError for anything but a torch.device), read-only `sample_rate`, `dimension`, `metric`,
`min_num_samples`.  The diarization pipeline itself does not go through `__call__`: it hands the
device-resident waveform and all masks of a chunk to the engine at once (`model_.engine`, one backbone
pass per chunk instead of one per (chunk, speaker))."""
from __future__ import annotations

from pathlib import Path
from typing import Callable, Iterable, Iterator, List, Mapping, Optional, Tuple, Union

import numpy as np
import torch

from . import ffi
from .audio import Audio, AudioFile
from .model import Model
from .pipeline import BaseInference, Pipeline

PipelineModel = Union[Model, str, Mapping]


def get_model(model: PipelineModel, token=None, cache_dir=None) -> Model:
    """anything the config may hold for a model -> a `Model` in eval mode: an instance, a checkpoint
    path / directory, or the keyword arguments of `Model.from_pretrained` (what `$model/<subfolder>`
    expands to)."""
    if isinstance(model, Mapping):
        options = {"token": token, "cache_dir": cache_dir, **model}
        model = Model.from_pretrained(**options)
    elif isinstance(model, (str, Path)):
        model = Model.from_pretrained(model, token=token, cache_dir=cache_dir, strict=False)
    elif not isinstance(model, Model):
        raise TypeError(f"Unsupported type ({type(model)}) for loading model: expected `str` or `dict`.")
    model.eval()
    return model


def first_true(predicate: Callable[[int], bool], lo: int, hi: int) -> int:
    """smallest n in (lo, hi] with predicate(n), for a monotone predicate with predicate(lo) false and
    predicate(hi) true"""
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if predicate(mid):
            hi = mid
        else:
            lo = mid
    return hi


class PyannoteAudioPretrainedSpeakerEmbedding(BaseInference):
    """wrapper around a pyannote-format embedding checkpoint (WeSpeaker ResNet here)"""

    metric = "cosine"

    def __init__(self, embedding: PipelineModel, device: Optional[torch.device] = None, token=None,
                 cache_dir=None):
        super().__init__()
        self.embedding = embedding
        self.model_: Model = get_model(embedding, token=token, cache_dir=cache_dir)
        self.device = device or torch.device("cpu")
        self.model_.to(self.device)
        self._min_num_samples: Optional[int] = None

    def to(self, device: torch.device):
        if not isinstance(device, torch.device):
            raise TypeError(
                f"`device` must be an instance of `torch.device`, got `{type(device).__name__}`")
        self.model_.to(device)
        self.device = device
        return self

    @property
    def sample_rate(self) -> int:
        return self.model_.audio.sample_rate

    @property
    def dimension(self) -> int:
        return self.model_.dimension

    @property
    def min_num_samples(self) -> int:
        """shortest waveform the model can embed.  The reference finds it by running the model on
        shorter and shorter random inputs until it raises (:688-702); here the only failure mode is
        "shorter than one fbank frame", which the C ABI answers directly (`pa_emb_num_fbank_frames`)."""
        if self._min_num_samples is None:
            if hasattr(self.model_, "_TDNN"):     # x-vector: SincNet + TDNN must leave at least one frame
                enough = lambda n: self.model_.num_frames(n) > 0   # noqa: E731
            else:
                frames = ffi.load().pa_emb_num_fbank_frames
                enough = lambda n: frames(n) > 0                   # noqa: E731
            self._min_num_samples = first_true(enough, 2, round(0.5 * self.sample_rate))
        return self._min_num_samples

    def __call__(self, waveforms: torch.Tensor, masks: Optional[torch.Tensor] = None) -> np.ndarray:
        return self.model_(waveforms, weights=masks).cpu().numpy()


def PretrainedSpeakerEmbedding(embedding: PipelineModel, device: Optional[torch.device] = None,
                               token=None, cache_dir=None):
    """factory of :719-778: SpeechBrain / NeMo / ONNX names select third-party runtimes that are not part
    of this build; everything else is a pyannote-format checkpoint."""
    third_party = isinstance(embedding, str) and not Path(embedding).exists() and \
        any(vendor in embedding for vendor in ("speechbrain", "nvidia"))
    if third_party:
        raise NotImplementedError(f"{embedding}: SpeechBrain/NeMo embedding back-ends are out of scope")
    return PyannoteAudioPretrainedSpeakerEmbedding(embedding, device=device, token=token,
                                                   cache_dir=cache_dir)


def vad_weights(scores: np.ndarray) -> np.ndarray:
    """aggregated voice-activity scores (frames, 1) -> pooling weights (frames,): NaN -> 0, cubed (:848-852)"""
    weights = np.array(scores, dtype=np.float32, copy=True)
    weights[np.isnan(weights)] = 0.0
    return (weights ** 3)[:, 0]


class SpeakerEmbedding(Pipeline):
    """One embedding per file, which is assumed to hold one speaker (pipelines/speaker_verification.py:781-856).

    `SpeakerEmbedding(embedding, segmentation=None)`: with a segmentation model the statistics pooling is weighted by
    the cubed voice-activity scores of the file (max over speakers of the aggregated scores).  `apply(file)` -> (1, D);
    `apply_batch(files)` -> one (1, D) per file, in order, with all files of different lengths batched together
    (`EmbeddingEngine.forward_ragged`)."""

    def __init__(self, embedding: PipelineModel = None, segmentation: Optional[PipelineModel] = None, token=None,
                 cache_dir=None):
        super().__init__()
        if embedding is None:
            raise ValueError("`embedding` must be a local checkpoint (or a Model instance): Hugging Face "
                             "defaults cannot be downloaded in this build.")
        from .inference import Inference
        from .voice_activity_detection import any_speaker
        self.embedding = embedding
        self.segmentation = segmentation
        self.embedding_model_: Model = get_model(embedding, token=token, cache_dir=cache_dir)
        if segmentation is not None:
            segmentation_model = get_model(segmentation, token=token, cache_dir=cache_dir)
            self._segmentation = Inference(segmentation_model, pre_aggregation_hook=any_speaker)

    def _audio(self) -> Audio:
        return Audio(self.embedding_model_.audio.sample_rate, mono="downmix")

    def _weights(self, file: AudioFile) -> Optional[torch.Tensor]:
        if self.segmentation is None:
            return None
        return torch.from_numpy(vad_weights(self._segmentation(file).data))

    def apply(self, file: AudioFile) -> np.ndarray:
        device = self.embedding_model_.device
        waveform = self._audio()(file)[0][None].to(device)
        weights = self._weights(file)
        if weights is not None:
            weights = weights[None].to(device)
        return self.embedding_model_(waveform, weights=weights).cpu().numpy()

    def apply_batch(self, files: Iterable[AudioFile]) -> List[np.ndarray]:
        files = [Audio.validate_file(f) for f in files]
        if not files:
            return []
        device = self.embedding_model_.device
        audio = self._audio()
        waves = [audio(f)[0].reshape(-1) for f in files]
        lengths = [w.numel() for w in waves]
        offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        wav = torch.cat(waves).to(device, torch.float32)
        masks = None
        if self.segmentation is not None:
            masks = [self._weights(f) for f in files]
        emb = self.embedding_model_.engine.forward_ragged(wav, offsets, lengths, masks).cpu().numpy()
        return [emb[i:i + 1] for i in range(len(files))]

    def _apply_batch(self, files: list, **kwargs) -> Iterator[Tuple[AudioFile, np.ndarray]]:
        for f, embedding in zip(files, self.apply_batch(files, **kwargs)):
            yield f, embedding

