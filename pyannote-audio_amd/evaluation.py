"""Evaluating a corpus: the accuracy half of the reference's `pyannote-audio benchmark` command
(src/pyannote/audio/__main__.py:430-510 `MinDurationOffOptimizer`, :656-849 the report), for a list of file dicts
(there is no pyannote.database here).

`Corpus` lists the turns of all files once and, on a `cuda` device, uploads them once; `Corpus.counts(fill)` then
gives every file's `annotation_counts(reference, hypothesis.support(fill), uem)` from one device call
(`pa_annot_corpus_counts`, include/pyannote_amd.h) and one download.  That is the call the gap
search repeats for every candidate: the corpus does not change between candidates, only `fill` does.  `CorpusCall`
is the one place that knows the table format of that call; `tuning.candidate_counts` fills it too, with rows that are
already on the device.

Reports are dicts (`_AnnotationMetric.report`); pandas is not required."""
from __future__ import annotations

import ctypes
import json
import time
import warnings
from functools import partial
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import annotation_metrics as am
from . import ffi
from .core import Annotation


# ------------------------------------------------------------------------------- one `pa_annot_corpus` call
def cut_slots(Nr: int, Nh: int, Nu: int) -> int:
    """cut slots of a file with that many reference, hypothesis and uem rows (sized with a collar)"""
    return 2 * (Nr + Nh + Nu) + 4 * Nr


def output_values(Kr: int, Kh: int) -> int:
    """values in the output block of a file with that many labels a side (`pa_annot_counts`)"""
    return Kr * Kh + Kr + Kh + len(am._SCALARS)


def corpus_workspace_bytes(hyp_rows: int, slots: int) -> int:
    """`annot_corpus_workspace` (csrc/annot_metrics.hip) from the totals of a call, for sizing a call before it has
    tables (tests/test_evaluation_cpu.py holds it to `pa_annot_corpus_workspace_bytes`)"""
    return 256 + 36 * hyp_rows + 44 * slots


def _int32(values) -> np.ndarray:
    values = np.asarray(values)
    if values.size and int(values.max()) > 0x7fffffff:
        raise ValueError("more rows in one counts call than 32-bit tables index (a tuner: lower workspace_bytes)")
    return np.ascontiguousarray(values, dtype=np.int32)


def _offsets(sizes) -> np.ndarray:
    return _int32(np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]))


class CorpusCall:
    """One `pa_annot_corpus` (include/pyannote_amd.h), its workspace and its result buffer, and
    every tensor the struct points into: they live as long as this object.

    Per file: `Nr`, `Nh`, `Nu` rows and `Kr`, `Kh` labels; per run (a hypothesis label of a file, files in order)
    `run_sizes` rows, listed in `run_rows` as indices into the hypothesis rows.  `arrays`: "ref_seg", "hyp_seg",
    "uem_seg" (float64 rows), "ref_label", "hyp_label" (None: the kernels label a row by its run), each a numpy array
    -- uploaded here, with the tables, in ONE copy -- or a tensor on `device`, used where it lies."""

    def __init__(self, device, Nr, Nh, Nu, Kr, Kh, run_sizes, run_rows, arrays: dict):
        host = {"ref_off": _offsets(Nr), "hyp_off": _offsets(Nh), "uem_off": _offsets(Nu),
                "cut_off": _offsets([cut_slots(a, b, c) for a, b, c in zip(Nr, Nh, Nu)]),
                "out_off": _offsets([output_values(a, b) for a, b in zip(Kr, Kh)]),
                "Kr": _int32(Kr), "Kh": _int32(Kh), "run_first": _offsets(Kh),
                "run_off": _offsets(run_sizes), "run_rows": _int32(run_rows)}
        F = len(host["Kr"])
        upload = {name: np.ascontiguousarray(a, dtype=np.float64).ravel() if name.endswith("_seg") else _int32(a)
                  for name, a in arrays.items() if isinstance(a, np.ndarray)}
        upload.update(host)
        starts = np.cumsum([0] + [(a.nbytes + 7) // 8 for a in upload.values()])      # every array starts on 8 bytes
        packed = np.zeros(int(starts[-1]), dtype=np.float64)
        for a, s, e in zip(upload.values(), starts, starts[1:]):
            packed[s:e].view(a.dtype)[:len(a)] = a
        packed = torch.from_numpy(packed).to(device)
        struct = ffi.AnnotCorpus()
        struct.F, struct.R = F, int(host["run_first"][-1])
        for (name, a), s in zip(upload.items(), starts):
            setattr(struct, name, packed.data_ptr() + 8 * int(s) if len(a) else None)
        for name, a in arrays.items():
            if isinstance(a, torch.Tensor):
                setattr(struct, name, a.data_ptr() if a.numel() else None)
        for name in ("ref_off", "hyp_off", "uem_off", "Kr", "Kh"):
            setattr(struct, "h_" + name, host[name].ctypes.data)
        self.device, self.struct, self._alive = device, struct, (host, packed, arrays)
        ws_bytes = int(ffi.load().pa_annot_corpus_workspace_bytes(ctypes.byref(struct)))
        if ws_bytes == 0:
            raise ValueError("the tables are more than pa_annot_corpus_counts accepts (65535 files, "
                             f"{am.MAX_LABELS} labels a side and 2^22 cuts a file)")
        self._ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        # [the files' output blocks][merged rows, int32, two to a float64]: one download
        self.out_off = host["out_off"]
        self.out = torch.empty(int(self.out_off[-1]) + (F + 1) // 2, dtype=torch.float64, device=device)

    def run(self, fill: float, collar: float, skip_overlap: bool) -> torch.Tensor:
        """`pa_annot_corpus_counts` -> the result buffer on the device; nothing is copied back here"""
        merged = self.out[int(self.out_off[-1]):].view(torch.int32)
        with torch.cuda.device(self.device):
            ffi.check(ffi.load().pa_annot_corpus_counts(ctypes.byref(self.struct), float(fill), float(collar),
                                                        int(bool(skip_overlap)), ffi.ptr(self.out), ffi.ptr(merged),
                                                        ffi.ptr(self._ws), self._ws.numel(), ffi.stream()),
                      "pa_annot_corpus_counts")
        return self.out

    def split(self, values: np.ndarray) -> tuple:
        """the downloaded result buffer -> (per file its output values, per file its merged row count)"""
        off = self.out_off
        return [values[a:b] for a, b in zip(off[:-1], off[1:])], values[int(off[-1]):].view(np.int32)[:len(off) - 1]


class Corpus:
    """The turns of `files` (dicts with "annotation", `hypothesis_key` and optionally "annotated"), listed once.
    A file without "annotated" is evaluated on the extent of its two annotations, as `annotation_counts` does, with
    its warning once per corpus.  `device`: a `cuda` device runs `counts` on the GPU; None or `cpu` (or, for that
    file alone, more than 64 labels on a side) goes through `hypothesis.support(fill)` and the host sweep."""

    def __init__(self, files, hypothesis_key: str = "speaker_diarization", device=None):
        self.files = list(files)
        self.hypothesis_key = hypothesis_key
        self.device = am._device(device)
        self.merged_rows_: Optional[list] = None      # rows of every supported hypothesis after the last `counts`
        self._rows = []
        approximated = False
        for file in self.files:
            ref_labels, ref_seg, ref_lab = am._rows(file["annotation"])
            hyp_labels, hyp_seg, hyp_lab = am._rows(file[hypothesis_key])
            am._check("reference", ref_seg)
            am._check("hypothesis", hyp_seg)
            uem = file.get("annotated")
            if uem is None:
                approximated = True
                both = np.concatenate([ref_seg, hyp_seg])      # (`support` keeps the extent of the hypothesis)
                uem_seg = np.array([[both[:, 0].min(), both[:, 1].max()]]) if len(both) else np.zeros((0, 2))
            else:
                uem_seg = am._uem_rows(uem)
                am._check("uem", uem_seg)
            self._rows.append((ref_labels, ref_seg, ref_lab, hyp_labels, hyp_seg, hyp_lab, uem_seg))
        if approximated:
            warnings.warn("'uem' was approximated by the union of 'reference' and 'hypothesis' extents.",
                          UserWarning, stacklevel=2)
        self._on_device = [self.device is not None and len(r[0]) <= am.MAX_LABELS and len(r[3]) <= am.MAX_LABELS
                           for r in self._rows]
        self._device_files = [f for f, on in enumerate(self._on_device) if on]
        if self._device_files:
            self._upload()

    # ------------------------------------------------------------------------------------------- device side
    def _upload(self):
        """the rows and labels of the files evaluated on the device, and their runs in the order `support` walks"""
        rows = [self._rows[f] for f in self._device_files]
        first, run_sizes, run_rows = 0, [], []
        for _, _, _, hyp_labels, seg, lab, _ in rows:
            run_rows.append(first + np.lexsort((seg[:, 1], seg[:, 0], lab)))     # by label, then (start, end)
            run_sizes.append(np.bincount(lab, minlength=len(hyp_labels)))
            first += len(seg)
        names = ("ref_seg", "ref_label", "hyp_seg", "hyp_label", "uem_seg")
        self._call = CorpusCall(self.device, *([len(r[i]) for r in rows] for i in (1, 4, 6, 0, 3)),
                                np.concatenate(run_sizes), np.concatenate(run_rows),
                                {name: np.concatenate([r[i] for r in rows]) for name, i in zip(names, (1, 2, 4, 5, 6))})

    def device_counts(self, fill: float, collar: float = 0.0, skip_overlap: bool = False) -> torch.Tensor:
        """`pa_annot_corpus_counts` on the uploaded corpus -> the device buffer (the output blocks of the files that
        are evaluated on the device, then their merged row counts as int32); nothing is copied back here"""
        if not self._device_files:
            raise RuntimeError("no file of this corpus is evaluated on a device")
        return self._call.run(fill, collar, skip_overlap)

    # ------------------------------------------------------------------------------------------------ counts
    def counts(self, fill: float, collar: float = 0.0, skip_overlap: bool = False) -> list:
        """per file, the dict `annotation_counts(reference, hypothesis.support(fill), uem, collar, skip_overlap)`
        returns (bit for bit on the device; the same code on the host)"""
        if not fill >= 0.0:
            raise ValueError(f"fill must be >= 0, got {fill}")
        if not collar >= 0.0:
            raise ValueError(f"collar must be >= 0, got {collar}")
        flat: dict = {}
        rows_after: dict = {}
        if self._device_files:
            values, merged = self._call.split(self.device_counts(fill, collar, skip_overlap).cpu().numpy())
            for k, f in enumerate(self._device_files):
                flat[f], rows_after[f] = values[k], int(merged[k])
        results = []
        for f, (file, r) in enumerate(zip(self.files, self._rows)):
            ref_labels, ref_seg, ref_lab, hyp_labels, _, _, uem_seg = r
            if f not in flat:
                supported = file[self.hypothesis_key].support(fill)
                labels, hyp_seg, hyp_lab = am._rows(supported)
                assert labels == hyp_labels
                flat[f] = am._host_counts(ref_seg, ref_lab, len(ref_labels), hyp_seg, hyp_lab, len(hyp_labels),
                                          uem_seg, float(collar), bool(skip_overlap))
                rows_after[f] = len(hyp_seg)
            results.append(am.counts_dict(ref_labels, hyp_labels, flat[f]))
        self.merged_rows_ = [rows_after[f] for f in range(len(self.files))]
        return results


# ---------------------------------------------------------------------------------------------- gap filling
class MinDurationOffOptimizer:
    """Find the `min_duration_off` (how short a within-speaker gap must be to be filled) that minimises `metric`
    over `files`: the reference's utility of the same name (__main__.py:430-510), with its call signature and
    control flow.  `optimizer(files, metric, bounds=(0.0, 1.0))` -> (best_min_duration_off, best_report); every file
    gets "best_speaker_diarization".  Files carry "annotation", "speaker_diarization" and optionally "annotated".

    For the count-based metrics of `annotation_metrics` the objective is `Corpus.counts` (one device call per
    candidate when `metric.device` is a GPU); any other metric object is called file by file on
    `file["speaker_diarization"].support(candidate)`, as the reference does."""

    hypothesis_key = "speaker_diarization"

    def _compute_metric(self, files, metric, corpus, collar: float) -> float:
        collar = float(collar)
        metric.reset()
        if corpus is not None:
            per_file = corpus.counts(collar, collar=metric.collar, skip_overlap=metric.skip_overlap)
            for file, counts in zip(files, per_file):
                metric.add_counts(counts, uri=getattr(file["annotation"], "uri", None))
        else:
            for file in files:
                metric(file["annotation"], file[self.hypothesis_key].support(collar), uem=file.get("annotated"))
        self._reports[collar] = metric.report()
        value = abs(metric)
        self._best_metric = min(self._best_metric, value)
        return value

    def __call__(self, files, metric, bounds: tuple = (0.0, 1.0)) -> tuple:
        from scipy.optimize import minimize_scalar
        files = list(files)
        self._best_metric = float("inf")          # (the metric is taken as one to minimise, as in the reference)
        self._reports: dict = {}
        corpus = None
        if isinstance(metric, am._AnnotationMetric):
            corpus = Corpus(files, hypothesis_key=self.hypothesis_key, device=metric.device)
        objective = partial(self._compute_metric, files, metric, corpus)
        without = objective(0.0)                  # filling nothing is always tried
        found = minimize_scalar(objective, bounds=bounds, method="Bounded")
        best = 0.0 if without == self._best_metric else float(found.x)
        for file in files:
            file["best_speaker_diarization"] = file[self.hypothesis_key].support(best)
        return best, self._reports[best]


# ------------------------------------------------------------------------------------------------- reports
def _columns(metric) -> list:
    return [metric.metric_name_] + list(metric.metric_components())


def report_to_csv(report: dict, columns: list) -> str:
    """one line per file and a TOTAL line; values in full precision (`repr`)"""
    lines = ["item," + ",".join(columns)]
    for item, row in report.items():
        lines.append(",".join([str(item)] + [repr(row[c]) for c in columns]))
    return "\n".join(lines) + "\n"


def report_to_text(report: dict, columns: list) -> str:
    """the same table for reading: the metric itself in percent, everything with two decimals"""
    head = ["item", columns[0] + " %"] + columns[1:]
    table = [head] + [[str(item), f"{100.0 * row[columns[0]]:.2f}"] + [f"{row[c]:.2f}" for c in columns[1:]]
                      for item, row in report.items()]
    widths = [max(len(line[i]) for line in table) for i in range(len(head))]
    return "\n".join("  ".join(cell.ljust(w) if i == 0 else cell.rjust(w)
                               for i, (cell, w) in enumerate(zip(line, widths))) for line in table) + "\n"


def get_diarization(prediction) -> Annotation:
    """the speaker diarization of what a pipeline returns: the annotation itself or its `speaker_diarization`"""
    if hasattr(prediction, "speaker_diarization"):
        return prediction.speaker_diarization
    if hasattr(prediction, "itertracks"):
        return prediction
    raise ValueError("Could not find speaker diarization in prediction.")


def _playing_time(file) -> float:
    if "audio" in file or "waveform" in file:
        from .audio import Audio
        return float(Audio().get_duration(file))
    if "duration" in file:
        return float(file["duration"])
    raise ValueError(f"file {file.get('uri')!r} has neither audio nor a 'duration'")


def benchmark(pipeline, files, into, metric=None, optimize: bool = False, per_file: bool = False,
              num_speakers: str = "auto", name: str = "benchmark") -> dict:
    """The body of the reference's `benchmark` command (__main__.py:656-849) for a list of file dicts ("uri",
    "audio" or "waveform" -- or a "duration" in seconds --, and for the accuracy half "annotation" and optionally
    "annotated").  `pipeline(files)` must yield (file, prediction) pairs; a prediction is an `Annotation` or carries
    `speaker_diarization` (and, optionally, `serialize()`).  `metric` defaults to `DiarizationErrorRate()`.

    Written under `into`, every name starting with `name` (plus ".OracleNumSpeakers" with num_speakers="oracle",
    which passes every file's number of reference speakers to the pipeline through file["pipeline_kwargs"]):
    `.rttm` (or, with `per_file`, a directory with rttm/<uri>.rttm and json/<uri>.json), `.json` of the serialised
    predictions, the speed `.yml` (`.<device name>.yml` and a "device" entry when the pipeline sits on a GPU), and,
    unless a file lacks "annotation", the metric's `.csv` / `.txt`, `.SpeakerCount.csv` and with `optimize` the four
    `.OptimizedMinDurationOff.{csv,txt,yml,rttm}`.  Existing output is not overwritten (FileExistsError).
    -> {"files": [paths written], "speed": {...}, and when evaluated "report", "value", "speaker_count",
    "speaker_count_accuracy", "speaker_count_error", with `optimize` "min_duration_off", "optimized_report"}."""
    import yaml
    if num_speakers not in ("auto", "oracle"):
        raise ValueError(f"num_speakers must be 'auto' or 'oracle', got {num_speakers!r}")
    into = Path(into)
    files = list(files)
    skip_metric = any(file.get("annotation") is None for file in files)
    if num_speakers == "oracle":
        name += ".OracleNumSpeakers"
        for file in files:
            file["pipeline_kwargs"] = {"num_speakers": len(file["annotation"].labels())}
    if not skip_metric and metric is None:
        metric = am.DiarizationErrorRate()
    written: list = []

    if per_file:
        directory = into / name
        if directory.exists():
            raise FileExistsError(f"{directory} already exists.")
        rttm_dir = directory / "rttm"
        rttm_dir.mkdir(parents=True)
    else:
        rttm_file = into / f"{name}.rttm"
        if rttm_file.exists():
            raise FileExistsError(f"{rttm_file} already exists.")
        into.mkdir(parents=True, exist_ok=True)
        written.append(rttm_file)

    serialized: dict = {}
    speaker_count: dict = {}
    started = time.time()
    processed = []                 # the files as the pipeline hands them back (it may work on copies)
    for file, prediction in pipeline(files):
        uri = file["uri"]
        processed.append(file)
        if hasattr(prediction, "serialize"):
            if per_file:
                (directory / "json").mkdir(exist_ok=True)
                with open(directory / "json" / f"{uri}.json", "w") as fp:
                    json.dump(prediction.serialize(), fp, indent=2)
                written.append(directory / "json" / f"{uri}.json")
            else:
                serialized[uri] = prediction.serialize()
        diarization = get_diarization(prediction)
        if per_file:
            rttm_file = rttm_dir / f"{uri}.rttm"
            written.append(rttm_file)
        with open(rttm_file, "w" if per_file else "a") as fp:
            diarization.write_rttm(fp)
        if not skip_metric:
            metric(file["annotation"], diarization, uem=file.get("annotated"))
            true_speakers, predicted = len(file["annotation"].labels()), len(diarization.labels())
            row = speaker_count.setdefault(true_speakers, {})
            row[predicted] = row.get(predicted, 0) + 1
        if optimize:
            file["speaker_diarization"] = diarization
    elapsed = time.time() - started

    if serialized and not per_file:
        with open(into / f"{name}.json", "w") as fp:
            json.dump(serialized, fp, indent=2)
        written.append(into / f"{name}.json")

    playing = sum(_playing_time(file) for file in files)
    speed = {"seconds_per_hour": elapsed / (playing / 3600.0), "times_faster_than_realtime": playing / elapsed,
             "total_processing_time": elapsed}
    device = getattr(pipeline, "device", None)
    speed_yml = into / f"{name}.yml"
    if isinstance(device, torch.device) and device.type == "cuda":
        props = torch.cuda.get_device_properties(device)
        speed["device"] = {}
        for attribute in dir(props):
            value = None if attribute.startswith("_") else getattr(props, attribute)
            if isinstance(value, (bool, int, float, str)):
                speed["device"][attribute] = value
            elif isinstance(value, (tuple, list)):
                speed["device"][attribute] = [v for v in value if isinstance(v, (bool, int, float, str))]
        speed_yml = into / f"{name}.{speed['device']['name'].replace(' ', '-')}.yml"
    with open(speed_yml, "w") as fp:
        yaml.safe_dump(speed, fp)
    written.append(speed_yml)
    result = {"files": written, "speed": speed}
    if skip_metric:
        print("Manual annotation is not available for every file: skipping metric evaluation.")
        return result

    columns = _columns(metric)
    report = metric.report()
    for suffix, text in ((".csv", report_to_csv(report, columns)), (".txt", report_to_text(report, columns))):
        with open(into / f"{name}{suffix}", "w") as fp:
            fp.write(text)
        written.append(into / f"{name}{suffix}")

    # matrix[i, j] = files with i reference speakers and j predicted ones
    matrix = np.zeros((max(speaker_count) + 1, max(max(row) for row in speaker_count.values()) + 1), dtype=int)
    for true_speakers, row in speaker_count.items():
        for predicted, count in row.items():
            matrix[true_speakers, predicted] = count
    off = sum(abs(i - j) * count for i, row in speaker_count.items() for j, count in row.items()) / matrix.sum()
    accuracy = np.trace(matrix) / matrix.sum()
    np.savetxt(into / f"{name}.SpeakerCount.csv", matrix, delimiter=",", fmt="%3d",
               footer=f"Accuracy = {accuracy:.1%} / Average error = {off:.2f} speakers off")
    written.append(into / f"{name}.SpeakerCount.csv")
    result.update({"report": report, "value": abs(metric), "speaker_count": matrix,
                   "speaker_count_accuracy": float(accuracy), "speaker_count_error": float(off)})

    if optimize:
        best, best_report = MinDurationOffOptimizer()(processed, metric)
        given = {file.get("uri"): file for file in files}
        for file in processed:     # (the caller's dicts get the two annotations too)
            for key in ("speaker_diarization", "best_speaker_diarization"):
                given.get(file["uri"], file)[key] = file[key]
        stem = f"{name}.OptimizedMinDurationOff"
        for suffix, text in ((".csv", report_to_csv(best_report, columns)),
                             (".txt", report_to_text(best_report, columns)),
                             (".yml", yaml.safe_dump({"min_duration_off": best}))):
            with open(into / f"{stem}{suffix}", "w") as fp:
                fp.write(text)
            written.append(into / f"{stem}{suffix}")
        if not per_file:
            optimized_rttm = into / f"{stem}.rttm"
            if optimized_rttm.exists():
                raise FileExistsError(f"{optimized_rttm} already exists.")
            written.append(optimized_rttm)
        for file in processed:
            if per_file:
                optimized_rttm = rttm_dir / f"{file['uri']}.OptimizedMinDurationOff.rttm"
                written.append(optimized_rttm)
            with open(optimized_rttm, "w" if per_file else "a") as fp:
                file["best_speaker_diarization"].write_rttm(fp)
        result.update({"min_duration_off": best, "optimized_report": best_report})
    return result
