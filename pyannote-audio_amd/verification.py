"""Speaker-verification trials, scored and evaluated on the device.

The step the reference takes once it can embed a file (pipelines/speaker_verification.py:858-895 `main`, and
torchmetrics/classification/equal_error_rate.py `EqualErrorRate`): every trial of a list gets the cosine distance of
its two files' embeddings, and the list gets the equal error rate of its detection-error-tradeoff curve.

* `trial_distances` is `scipy.spatial.distance.cdist(E[i:i+1], E[j:j+1], "cosine")[0, 0]` per trial, bit for bit
  (`pa_trial_cosine_f64`, the arithmetic of the clustering stage's `pa_cdist_cosine_f64`).
* `det_curve` / `equal_error_rate` are `pyannote.metrics.binary_classification.det_curve`: sklearn's `roc_curve`
  (drop_intermediate=True), `fnr = 1 - tpr`, the first point with `fpr > fnr` and the mean of the four rates around
  it.  pyannote.metrics is not a dependency of this package and is not installed where this was written: this is a
  restatement of its published behaviour (as `metrics.BaseMetric` is), pinned to `sklearn.metrics.roc_curve` 1.7.2
  by tests/golden/make_verification_golden.py.  Counts are integers and every rate is one float64 division, so the
  results equal sklearn's with `==`.  The sort is `torch.sort(stable=True)`; everything after it is
  `pa_det_curve_f64` (csrc/verification.hip).

Two deliberate differences, both a `ValueError` before any curve is returned: a non-finite score is refused (sklearn
refuses it too), and so is a trial list without both a target and a non-target trial (the reference warns, then dies
on an IndexError).

There is no host implementation of the device parts: without a GPU they raise (ffi.require_gpu)."""
from __future__ import annotations

from typing import Iterable, Mapping, Tuple

import numpy as np
import torch

from . import ffi


def det_geometry() -> Tuple[int, int]:
    """(scores one workgroup of the curve kernels takes, workgroup sums per chunk of their two-level scan), asked of
    the library (csrc/verification.hip DET_BLOCK, DET_CHUNK): the sizes at which the kernels change path"""
    lib = ffi.load()
    return int(lib.pa_det_block_elements()), int(lib.pa_det_scan_chunk())


MAX_TRIALS = 2 ** 31 - 1


def _device_of(*arrays) -> torch.device:
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    ffi.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def _as_tensor(x) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.detach()
    return torch.from_numpy(np.ascontiguousarray(x))


def _trial_index(index, name: str, num_embeddings: int) -> torch.Tensor:
    """(T,) integer tensor where it lies, every entry checked against the table"""
    idx = _as_tensor(index)
    if idx.ndim != 1:
        raise ValueError(f"`{name}` must be one-dimensional, got shape {tuple(idx.shape)}")
    if idx.dtype == torch.bool or idx.is_floating_point() or idx.is_complex():
        raise ValueError(f"`{name}` must hold integers, got {idx.dtype}")
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= num_embeddings):
        raise ValueError(f"`{name}` must lie in 0..{num_embeddings - 1}, got {int(idx.min())}..{int(idx.max())}")
    return idx


def trial_distances(embeddings, index1, index2, metric: str = "cosine") -> torch.Tensor:
    """Distance of embeddings[index1[t]] and embeddings[index2[t]] for every trial t.

    `embeddings`: (N, D) numpy array or torch tensor, used where it lies; `index1`, `index2`: (T,) integers in
    0..N-1.  -> (T,) float64 tensor on the device, each entry the bits of
    `scipy.spatial.distance.cdist(E[i:i+1], E[j:j+1], "cosine")[0, 0]` on the float64 table (a zero row gives NaN).
    Only the cosine metric exists."""
    if metric != "cosine":
        raise ValueError(f"only the 'cosine' metric is supported, got {metric!r}")
    table = _as_tensor(embeddings)
    if table.ndim != 2 or table.shape[0] < 1 or table.shape[1] < 1:
        raise ValueError(f"`embeddings` must be a non-empty (num_embeddings, dimension) array, got "
                         f"{tuple(table.shape)}")
    N, D = table.shape
    idx1, idx2 = _trial_index(index1, "index1", N), _trial_index(index2, "index2", N)
    if idx1.shape[0] != idx2.shape[0]:
        raise ValueError(f"`index1` and `index2` must have one entry per trial, got {idx1.shape[0]} and "
                         f"{idx2.shape[0]}")
    T = idx1.shape[0]
    if T > MAX_TRIALS or N > MAX_TRIALS:
        raise ValueError(f"at most {MAX_TRIALS} trials and embeddings are supported")
    dev = _device_of(table, idx1, idx2)
    table = table.to(dev, torch.float64).contiguous()
    idx1, idx2 = (i.to(dev, torch.int32).contiguous() for i in (idx1, idx2))
    out = torch.empty(T, dtype=torch.float64, device=dev)
    norms = torch.empty(N, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ffi.check(ffi.load().pa_trial_cosine_f64(ffi.ptr(table), N, D, ffi.ptr(idx1), ffi.ptr(idx2), T, ffi.ptr(out),
                                                 ffi.ptr(norms), ffi.stream()), "pa_trial_cosine_f64")
    return out


def _curve_on_device(y_true, scores, distances: bool, rates: bool):
    """sort, `pa_det_curve_f64`, refusals.  -> (status, fps, tps, thresholds, fpr, fnr) with the status block on
    the host and the (T + 1) arrays on the device (the float64 ones None without `rates`)."""
    y, s = _as_tensor(y_true), _as_tensor(scores)
    if y.ndim != 1 or s.ndim != 1 or y.shape[0] != s.shape[0]:
        raise ValueError(f"`y_true` and `scores` must be one-dimensional and of one length, got "
                         f"{tuple(y.shape)} and {tuple(s.shape)}")
    T = s.shape[0]
    if T < 2:
        raise ValueError(f"a curve needs a target and a non-target trial, got {T} trial(s)")
    if T > MAX_TRIALS:
        raise ValueError(f"at most {MAX_TRIALS} trials are supported, got {T}")
    dev = _device_of(s, y)
    keys = s.to(dev, torch.float64)
    if distances:
        keys = -keys
    labels = y.to(dev)
    labels = labels.to(torch.uint8) if labels.dtype == torch.bool else (labels != 0).to(torch.uint8)
    # ascending and stable, read from the far end by the kernels: sklearn's mergesort followed by [::-1]
    keys, order = torch.sort(keys, stable=True)
    labels = labels[order].contiguous()
    del order
    lib = ffi.load()
    fps = torch.empty(T + 1, dtype=torch.int32, device=dev)
    tps = torch.empty(T + 1, dtype=torch.int32, device=dev)
    thresholds = fpr = fnr = None
    if rates:
        thresholds, fpr, fnr = (torch.empty(T + 1, dtype=torch.float64, device=dev) for _ in range(3))
    status = torch.empty(8, dtype=torch.int64, device=dev)
    nbytes = int(lib.pa_det_workspace_bytes(T))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        ffi.check(lib.pa_det_curve_f64(ffi.ptr(keys), ffi.ptr(labels), T, int(bool(distances)), ffi.ptr(fps),
                                       ffi.ptr(tps), ffi.ptr(thresholds), ffi.ptr(fpr), ffi.ptr(fnr),
                                       ffi.ptr(status), ffi.ptr(work), nbytes, ffi.stream()), "pa_det_curve_f64")
    status = status.cpu().numpy()
    nonfinite, positives, negatives, _, k = (int(v) for v in status[:5])
    if nonfinite:
        raise ValueError(f"{nonfinite} of the {T} scores are NaN or infinite")
    if positives == 0 or negatives == 0:
        raise ValueError(f"a curve needs a target and a non-target trial, got {positives} target and {negatives} "
                         "non-target trials")
    if k < 1:                                        # (cannot happen with both classes: the last point is (1, 0))
        raise RuntimeError("pa_det_curve_f64 found no point with fpr > fnr")
    return status, fps, tps, thresholds, fpr, fnr


def _eer_of(status: np.ndarray) -> float:
    return float(status[5:6].view(np.float64)[0])


def det_curve(y_true, scores, distances: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray, float]:
    """Detection-error-tradeoff curve of `scores` (higher = more likely a target trial; `distances=True`: lower)
    against the 0/1 or boolean `y_true`, numpy arrays or torch tensors used where they lie.
    -> (fpr, fnr, thresholds, eer): float64 numpy arrays over the curve's points and a Python float."""
    status, _, _, thresholds, fpr, fnr = _curve_on_device(y_true, scores, distances, rates=True)
    points = int(status[3])
    return (fpr[:points].cpu().numpy(), fnr[:points].cpu().numpy(), thresholds[:points].cpu().numpy(),
            _eer_of(status))


def equal_error_rate(y_true, scores, distances: bool = False) -> float:
    """`det_curve(...)[3]` without the curve: only the status block of `pa_det_curve_f64` comes back"""
    return _eer_of(_curve_on_device(y_true, scores, distances, rates=False)[0])


class EqualErrorRate:
    """Stateful equal error rate (torchmetrics/classification/equal_error_rate.py): `update(scores, y_true)` keeps
    the batch on the device, `compute()` evaluates everything seen at once and returns a 0-d float64 tensor,
    `reset()` forgets it.  Not a `torchmetrics.Metric` (torchmetrics is not a dependency): the three methods are the
    protocol."""

    is_differentiable = False
    higher_is_better = False
    full_state_update = True

    def __init__(self, distances: bool = True):
        self.distances = distances
        self.reset()

    def reset(self) -> None:
        self.scores: list = []
        self.y_true: list = []

    def update(self, scores, y_true) -> None:
        s, y = _as_tensor(scores).reshape(-1), _as_tensor(y_true).reshape(-1)
        if s.shape[0] != y.shape[0]:
            raise ValueError(f"`scores` and `y_true` must be of one length, got {s.shape[0]} and {y.shape[0]}")
        dev = _device_of(s, y)
        self.scores.append(s.to(dev, torch.float64))
        self.y_true.append(y.to(dev) != 0)

    def __call__(self, scores, y_true) -> torch.Tensor:
        self.update(scores, y_true)
        return self.compute()

    def compute(self) -> torch.Tensor:
        if not self.scores:
            raise ValueError("EqualErrorRate.compute() before any update()")
        eer = equal_error_rate(torch.cat(self.y_true), torch.cat(self.scores), distances=self.distances)
        return torch.tensor(eer, dtype=torch.float64)


def evaluate_trials(pipeline, trials: Iterable[Mapping], batch_size: int = 32) -> dict:
    """The reference's verification experiment (pipelines/speaker_verification.py:858-895) without the protocol
    lookup and the command line.

    `trials`: an iterable of {"file1": AudioFile, "file2": AudioFile, "reference": bool} (pyannote.database's trial
    shape); a file is identified by its "audio" entry.  Every distinct file is embedded once through
    `pipeline.apply_batch` (a `SpeakerEmbedding`), `batch_size` files at a time in order of first appearance; every
    trial is scored with the cosine distance on the device.
    -> {"eer": float, "distances": (T,) float64 device tensor, "y_true": (T,) bool device tensor, "num_files": int}"""
    if batch_size < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    rows: dict = {}
    files: list = []
    index1, index2, y_true = [], [], []
    for trial in trials:
        pair = []
        for side in ("file1", "file2"):
            file = trial[side]
            if not isinstance(file, Mapping) or "audio" not in file:
                raise ValueError(f"trial {len(y_true)}: `{side}` must be a mapping with an 'audio' entry")
            key = file["audio"]
            if key not in rows:
                rows[key] = len(files)
                files.append(file)
            pair.append(rows[key])
        index1.append(pair[0])
        index2.append(pair[1])
        y_true.append(bool(trial["reference"]))
    if not y_true:
        raise ValueError("no trials")
    ffi.require_gpu()
    embeddings = []
    for first in range(0, len(files), batch_size):
        embeddings.extend(pipeline.apply_batch(files[first:first + batch_size]))
    table = np.concatenate([np.asarray(e).reshape(1, -1) for e in embeddings], axis=0)
    dev = _device_of()
    model = getattr(pipeline, "embedding_model_", None)
    if model is not None and getattr(model.device, "type", None) == "cuda":
        dev = model.device
    table = torch.from_numpy(table).to(dev)
    labels = torch.tensor(y_true, dtype=torch.bool, device=dev)
    dist = trial_distances(table, np.asarray(index1, dtype=np.int64), np.asarray(index2, dtype=np.int64))
    return {"eer": equal_error_rate(labels, dist, distances=True), "distances": dist, "y_true": labels,
            "num_files": len(files)}
