"""Tuning on a corpus.  `DetectionTuner` (below `ClusteringTuner`, after `candidate_counts`, the counts of all its
candidates on a file) tunes the thresholds of the detection pipelines; `OnlineTuner` (last) the three thresholds of
the online rule, every (file, candidate) a job of one `pao_replay` launch; `ClusteringTuner` the clustering of a
`SpeakerDiarization` pipeline: the search the reference's `optimize` command runs
(src/pyannote/audio/__main__.py:116-283 -- the pipeline applied to every development file again for every candidate
`clustering.threshold` / `min_cluster_size`), organised so that a candidate only pays for what depends on it.

  once per file      the front end (both networks; kept in the file dict by the pipeline's training cache),
                     `filter_embeddings` and the dendrogram (it depends on `method`, not on the threshold)
  once per file      ALL candidate cuts of that dendrogram: `Dendrogram.cuts` (`pa_dendrogram_cuts`, one launch)
  per candidate      the rest of `AgglomerativeClustering.cluster` on the cut labels, `assign_embeddings`, the back end
                     and the metric -- and not even those when an earlier candidate gave this file the same
                     `hard_clusters` (two thresholds between the same pair of merge heights do): its results are copies

With `VBxClustering` (threshold, Fa, Fb; `sweep_vbx`) the dendrogram of the unit vectors and the PLDA projection are
the per-file part, and what the candidates of a file share further is worked out by `plan_vbx_jobs`: equal cuts are one
initialisation, distinct (initialisation, Fa, Fb) triples one VB inference, all of them jobs of `pa_vbx_run_batch`
(DESIGN.md section 26).

There is no sampler, no journal and no `pyannote.database` here: the candidates are a grid in the order given, files
are dicts as `evaluation.benchmark` takes them ("annotation", optionally "annotated" and "pipeline_kwargs")."""
from __future__ import annotations

import copy
import time
import warnings
from dataclasses import dataclass, field, replace
from datetime import datetime
from pathlib import Path
from typing import Callable, Iterable, Optional

import numpy as np
import torch

from . import annotation_metrics as am
from .clustering import AgglomerativeClustering, Dendrogram, VBxClustering
from .evaluation import CorpusCall, corpus_workspace_bytes, cut_slots, get_diarization


@dataclass
class _Tree:
    """what `BaseClustering.__call__` does before the cut, for one file and linkage method"""
    tree: Dendrogram
    train: np.ndarray          # the filtered embeddings the tree was built from
    chunk_idx: np.ndarray
    speaker_idx: np.ndarray
    bounds: tuple              # (num, min, max) clusters of `set_num_clusters`


@dataclass
class _VBxFront:
    """`VBxClustering.before_cut` of one file"""
    train: np.ndarray
    unit: np.ndarray
    tree: Dendrogram
    fea: object                # PLDA features on the device


@dataclass
class _Outcome:
    """one (candidate, file): what its route found (`hard` None: still to be assigned from `train_labels`) and, once
    its back end and metric have run, what later candidates with an equal clustering share"""
    hard: Optional[np.ndarray] = None
    centroids: Optional[np.ndarray] = None
    train_labels: Optional[np.ndarray] = None
    train_clusters: Optional[int] = None
    vbx_iterations: Optional[int] = None
    hypothesis: object = None
    components: Optional[dict] = None
    other: str = ""            # the candidate's parameters beyond the clustering


@dataclass
class _Prepared:
    """one file of the corpus: its validated dict, its (cached) front end, the speaker bounds of its
    `pipeline_kwargs`, what the clustering needs before the cut, and what the candidates of one `evaluate` share
    (`cuts`, `evaluated` and the "jobs" of `vbx` start empty with every `evaluate`)"""
    file: dict
    front: object
    bounds: tuple
    trees: dict = field(default_factory=dict)      # linkage method -> None or _Tree
    vbx: dict = field(default_factory=dict)        # once asked: "front" -> None or _VBxFront, "jobs" -> `_vbx_file`
    cuts: dict = field(default_factory=dict)       # linkage method -> the tree's `cuts` at the candidates' thresholds
    evaluated: list = field(default_factory=list)  # [_Outcome] whose back end and metric were run


def best_entry(entries: list, direction: str = "minimize") -> dict:
    """the first entry, in candidate order, whose loss no other entry beats"""
    if not entries:
        raise ValueError("no candidate was evaluated")
    sign = 1.0 if direction == "minimize" else -1.0
    best = entries[0]
    for entry in entries[1:]:
        if sign * (entry["loss"] - best["loss"]) < 0:
            best = entry
    return best


def plan_vbx_jobs(cut_rows: np.ndarray, picks: list) -> tuple:
    """What one file's VBx candidates share.  `cut_rows` (T, n): the AHC labels at the T distinct thresholds;
    `picks`: per candidate (row of `cut_rows`, Fa, Fb), in candidate order.  Returns
      inits    the rows that get an initialisation: the first of every run of equal rows, in row order
      jobs     the distinct (index into `inits`, Fa, Fb) triples, in order of first use: one VB inference each
      job_of   per candidate, its index into `jobs`"""
    seen, inits, init_of_row = {}, [], []
    for t, row in enumerate(cut_rows):
        key = np.ascontiguousarray(row).tobytes()
        if key not in seen:
            seen[key] = len(inits)
            inits.append(t)
        init_of_row.append(seen[key])
    jobs, job_of = {}, []
    for row, Fa, Fb in picks:
        job_of.append(jobs.setdefault((init_of_row[row], float(Fa), float(Fb)), len(jobs)))
    return inits, list(jobs), job_of


class ClusteringTuner:
    """`ClusteringTuner(pipeline).prepare(files).sweep(thresholds, min_cluster_sizes)` -> {"entries": [{"params",
    "loss"} per candidate, thresholds outermost], "best": the first minimum, "shared_evaluations": how many (candidate,
    file) pairs reused an earlier candidate's back end and metric components, "evaluations": all such pairs}.

    `metric`: a factory of fresh metrics (default `pipeline.get_metric`); the loss of a candidate is `abs(metric)`
    after every file, i.e. what `pipeline.instantiate(params)`, `pipeline(file)` per file and
    `metric(file["annotation"], output, uem=file.get("annotated"))` give.  Every parameter but the two swept ones
    stays as the pipeline is instantiated; the pipeline is left instantiated with the last candidate.

    With `VBxClustering` (`sweep_vbx(thresholds, Fas, Fbs)`), per file: the linkage and the PLDA projection once, every
    candidate threshold from one `Dendrogram.cuts` call, and the VB inferences of all candidates -- one per distinct
    (cut, Fa, Fb) -- from `pa_vbx_run_batch` calls that no iteration reads back from (`VBxClustering.vbx_batch`);
    per candidate the centroids (host), the assignment (`pa_constrained_assign`), the back end and the metric."""

    #: bound on what one `pa_vbx_run_batch` call allocates (kernel workspace + result buffer); a file's jobs beyond it
    #: take several calls
    workspace_bytes: int = 1 << 30
    #: False: a VBxClustering candidate goes through the pipeline's own call on the cached front end, like any other
    #: clustering without a dendrogram to share (what tools/time_vbx_tuning.py measures the batched route against)
    batch_vbx: bool = True
    #: "device" cuts every dendrogram with `pa_dendrogram_cuts` on the pipeline's GPU, "host" runs the same plan
    #: through numpy (profiles/clustering_tuning_timing.txt has both at one audio-hour)
    cut_on: str = "device"

    def __init__(self, pipeline, metric: Optional[Callable] = None):
        self.pipeline = pipeline
        self.metric = metric if metric is not None else pipeline.get_metric
        self.prepared: list = []
        self.shared_evaluations = 0
        self.evaluations = 0
        #: per candidate, per file: clusters of the training embeddings (None where no dendrogram was cut)
        self.train_clusters: list = []
        #: per candidate, per file: the speaker diarization that was scored
        self.hypotheses: list = []
        #: per candidate, per file: VB iterations of the candidate's inference (None where none was run)
        self.vbx_iterations: list = []
        #: of the last `evaluate` with VBxClustering: candidates x files with an inference, VB inferences run,
        #: initialisations built, `pa_vbx_run_batch` calls
        self.vbx_shared: dict = {}

    # ------------------------------------------------------------------------------------------ preparation
    def prepare(self, files: Iterable) -> "ClusteringTuner":
        """runs every file's front end once (or takes it from the file's training cache) with `pipeline.training`
        set, and restores `training` whatever happens"""
        pipeline = self.pipeline
        if not pipeline.instantiated:
            pipeline.instantiate(pipeline.default_parameters())
        previous = pipeline.training
        pipeline.training = True
        try:
            self.prepared = [self._prepare_one(file) for file in files]
        finally:
            pipeline.training = previous
        return self

    def _prepare_one(self, file) -> _Prepared:
        pipeline = self.pipeline
        file = pipeline.prepare_one(file)
        if not hasattr(pipeline, "_cached_front_end"):     # not a SpeakerDiarization: nothing to keep between candidates
            return _Prepared(file=file, front=None, bounds=())
        own = dict(file.get("pipeline_kwargs", {}))
        bounds = pipeline._speaker_bounds(own.pop("num_speakers", None), own.pop("min_speakers", None),
                                          own.pop("max_speakers", None), own, file=file)
        pipeline._require_device()
        front = pipeline._cached_front_end(file, pipeline.setup_hook(file, None))
        return _Prepared(file=file, front=front, bounds=bounds)

    def _tree(self, item: _Prepared) -> Optional[_Tree]:
        """what `BaseClustering.__call__` does before the cut, once per file and linkage method.  The tree is kept
        with the training copy it was built from: `dendrogram` normalises that copy in place for the geometric
        methods and `cluster_from_cut` takes the small-cluster centroids from it, so every method gets a fresh copy
        of the filtered embeddings and no copy is normalised twice."""
        clustering = self.pipeline.clustering
        method = clustering.method
        if method not in item.trees:
            front = item.front
            num_speakers, min_speakers, max_speakers = item.bounds
            train, chunk_idx, speaker_idx = clustering.filter_embeddings(
                front.embeddings, segmentations=front.segmentations, num_clean_frames=front.clean)
            bounds = clustering.set_num_clusters(train.shape[0], num_clusters=num_speakers,
                                                 min_clusters=min_speakers, max_clusters=max_speakers)
            if bounds[2] < 2 or train.shape[0] < 2:
                item.trees[method] = None       # one cluster whatever the candidate says: the pipeline's own path
            else:
                tree = Dendrogram(clustering.dendrogram(train))
                item.trees[method] = _Tree(tree, train, chunk_idx, speaker_idx, bounds)
        return item.trees[method]

    def _vbx_front(self, item: _Prepared) -> Optional[_VBxFront]:
        """`VBxClustering.before_cut`, once per file: None where the pipeline's own call decides (a silent file,
        fewer than two training embeddings)"""
        if "front" not in item.vbx:
            front, clustering = item.front, self.pipeline.clustering
            item.vbx["front"] = None
            if clustering.plda is not None and clustering.plda.lda_dimension != 128:
                # `pa_vbx_run_batch` is built for the 128 PLDA dimensions of the published models
                warnings.warn(f"ClusteringTuner: a PLDA of {clustering.plda.lda_dimension} dimensions is not batched; every "
                              "VBx candidate goes through the pipeline's own call")
            elif front is not None and not front.silent and clustering.plda is not None:
                before = clustering.before_cut(front.embeddings, front.segmentations, num_clean_frames=front.clean)
                if before is not None:
                    train, unit, Z, fea = before
                    item.vbx["front"] = _VBxFront(train, unit, Dendrogram(Z), fea)
        return item.vbx["front"]

    def _vbx_file(self, item: _Prepared, thresholds: list, picks: list) -> Optional[dict]:
        """every candidate's VB inference on one file: {"job_of": per candidate, "q": per job (responsibilities,
        ELBO history), "finished": per job, filled by `_vbx_route`}"""
        plan = self._vbx_front(item)
        if plan is None:
            return None
        clustering = self.pipeline.clustering
        rows = plan.tree.cuts(thresholds, device=self.cut_device())
        rows = np.stack([np.unique(row, return_inverse=True)[1] for row in rows])
        inits, jobs, job_of = plan_vbx_jobs(rows, picks)
        starts = [clustering.initial_responsibilities(rows[t]) for t in inits]
        results = clustering.vbx_batch(plan.fea, starts, jobs, workspace_bytes=self.workspace_bytes)
        for name, more in (("candidates", len(picks)), ("jobs", len(jobs)), ("initialisations", len(inits)),
                           ("calls", clustering.last_vbx_calls)):
            self.vbx_shared[name] = self.vbx_shared.get(name, 0) + more
        return {"job_of": job_of, "q": results, "finished": {}}

    def cut_device(self):
        return self.pipeline.clustering.device if self.cut_on == "device" else None

    # ------------------------------------------------------------------------------------------------ sweep
    def candidates(self, thresholds, min_cluster_sizes=None) -> list:
        """the parameter dicts (as `pipeline.instantiate` takes them) of the grid, thresholds outermost"""
        base = self.pipeline.parameters(instantiated=True)
        if min_cluster_sizes is None:
            min_cluster_sizes = [None]
        out = []
        for threshold in thresholds:
            for size in min_cluster_sizes:
                params = copy.deepcopy(base)
                params["clustering"]["threshold"] = float(threshold)
                if size is not None:
                    params["clustering"]["min_cluster_size"] = int(size)
                out.append(params)
        return out

    def sweep(self, thresholds, min_cluster_sizes=None) -> dict:
        """the grid `thresholds` x `min_cluster_sizes` (None: the instantiated size), in the given order"""
        thresholds = [float(t) for t in thresholds]
        if any(np.isnan(thresholds)):
            raise ValueError("ClusteringTuner.sweep: a threshold is NaN")
        return self.evaluate(self.candidates(thresholds, min_cluster_sizes))

    def sweep_vbx(self, thresholds, Fas, Fbs) -> dict:
        """the grid `thresholds` x `Fas` x `Fbs` of a `VBxClustering` pipeline: thresholds outermost, then Fa, then Fb"""
        if not isinstance(getattr(self.pipeline, "clustering", None), VBxClustering):
            raise TypeError("ClusteringTuner.sweep_vbx: the pipeline's clustering is not VBxClustering")
        grid = [(float(t), float(a), float(b)) for t in thresholds for a in Fas for b in Fbs]
        if any(np.isnan(point).any() for point in grid):
            raise ValueError("ClusteringTuner.sweep_vbx: a threshold, Fa or Fb is NaN")
        base = self.pipeline.parameters(instantiated=True)
        candidates = []
        for threshold, Fa, Fb in grid:
            params = copy.deepcopy(base)
            params["clustering"].update(threshold=threshold, Fa=Fa, Fb=Fb)
            candidates.append(params)
        return self.evaluate(candidates)

    def evaluate(self, candidates: list) -> dict:
        """any list of parameter dicts, in order.  With `AgglomerativeClustering` every file's dendrogram (one per
        linkage method among the candidates) is cut ONCE, at the thresholds of all candidates; with `VBxClustering`
        the VB inferences of all candidates on a file are the jobs of batched launches (`_vbx_file`)."""
        if not self.prepared:
            raise RuntimeError("ClusteringTuner: call prepare(files) first")
        pipeline = self.pipeline
        clustering = getattr(pipeline, "clustering", None)
        # the route of every (candidate, file): None is the candidate through the pipeline's own `__call__`
        route = self._cut_route if isinstance(clustering, AgglomerativeClustering) else \
            self._vbx_route if self.batch_vbx and isinstance(clustering, VBxClustering) else None
        self.shared_evaluations = self.evaluations = 0
        self.train_clusters, self.hypotheses, self.vbx_iterations = [], [], []
        self.vbx_shared = {}
        for item in self.prepared:
            item.cuts, item.evaluated = {}, []
            item.vbx.pop("jobs", None)
        row_of, picks = {}, []       # threshold -> row of a file's cuts; VBx: per candidate (row, Fa, Fb)
        if route is not None:
            row_of = {t: k for k, t in enumerate(dict.fromkeys(float(p["clustering"]["threshold"]) for p in candidates))}
        if route == self._vbx_route:
            if any(np.isnan(list(row_of))):
                raise ValueError("ClusteringTuner.evaluate: a threshold is NaN")
            picks = [(row_of[float(p["clustering"]["threshold"])], float(p["clustering"]["Fa"]),
                      float(p["clustering"]["Fb"])) for p in candidates]
        previous = pipeline.training
        pipeline.training = True      # (the generic path goes through the pipeline's call: cached front ends there too)
        entries = []
        try:
            for c, params in enumerate(candidates):
                pipeline.instantiate(params)
                # results are shared only between candidates that differ in nothing but the clustering
                other = repr({name: value for name, value in params.items() if name != "clustering"})
                metric = self.metric()
                done = []
                for item in self.prepared:
                    found = None if route is None or item.front is None else route(item, c, row_of, picks)
                    done.append(self._evaluate(item, found, other, metric))
                self.train_clusters.append([outcome.train_clusters for outcome in done])
                self.vbx_iterations.append([outcome.vbx_iterations for outcome in done])
                self.hypotheses.append([outcome.hypothesis for outcome in done])
                entries.append({"params": params, "loss": abs(metric)})
        finally:
            pipeline.training = previous
        direction = pipeline.get_direction() if hasattr(pipeline, "get_direction") else "minimize"
        return {"entries": entries, "best": best_entry(entries, direction),
                "shared_evaluations": self.shared_evaluations, "evaluations": self.evaluations}

    def _cut_route(self, item: _Prepared, c: int, row_of: dict, picks: list) -> _Outcome:
        """the candidate's row of the file's cuts -> training labels.  Nothing found: a silent file, or one cluster
        whatever the candidate says (`_tree`)"""
        clustering = self.pipeline.clustering
        method = clustering.method
        if item.front.silent:
            return _Outcome()
        if method not in item.cuts:
            plan = self._tree(item)
            item.cuts[method] = None if plan is None else plan.tree.cuts(list(row_of), device=self.cut_device())
        if item.cuts[method] is None:
            return _Outcome()
        plan = item.trees[method]
        num, lo, hi = plan.bounds
        train_labels = clustering.cluster_from_cut(plan.train, plan.tree,
                                                   item.cuts[method][row_of[float(clustering.threshold)]],
                                                   min_clusters=lo, max_clusters=hi, num_clusters=num)
        return _Outcome(train_labels=train_labels, train_clusters=int(np.max(train_labels)) + 1)

    def _vbx_route(self, item: _Prepared, c: int, row_of: dict, picks: list) -> _Outcome:
        """the candidate's job among the file's inferences (`_vbx_file`, once per file) -> hard clusters.  Nothing
        found where `_vbx_front` leaves the file to the pipeline"""
        if "jobs" not in item.vbx:
            item.vbx["jobs"] = self._vbx_file(item, list(row_of), picks)
        inference = item.vbx["jobs"]
        if inference is None:
            return _Outcome()
        front, clustering = item.front, self.pipeline.clustering
        num_speakers, min_speakers, max_speakers = item.bounds
        job = inference["job_of"][c]
        q, history = inference["q"][job]
        if job not in inference["finished"]:      # (candidates that differ beyond the clustering share a job)
            plan = item.vbx["front"]
            hard, _, centroids = clustering.after_vbx(
                front.embeddings, front.segmentations, plan.train, plan.unit, q, num_clusters=num_speakers,
                min_clusters=1 if min_speakers is None else min_speakers,
                max_clusters=np.inf if max_speakers is None else max_speakers, assign_on_device=True)
            inference["finished"][job] = (hard, centroids, clustering.timings["vbx_speakers"])
        hard, centroids, kept = inference["finished"][job]
        return _Outcome(hard=hard, centroids=centroids, train_clusters=kept, vbx_iterations=len(history))

    def _evaluate(self, item: _Prepared, found: Optional[_Outcome], other: str, metric) -> _Outcome:
        """one file under the currently instantiated candidate, accumulated into `metric`: the tail all routes share.
        `found`: what the route gave, None for the candidate through the pipeline's own `__call__`.  -> the outcome
        with its hypothesis: that of an earlier candidate with the same `other` parameters and an equal clustering
        of this file, whose back end and metric components are shared, or its own"""
        pipeline, front, file = self.pipeline, item.front, item.file
        self.evaluations += 1
        if found is None or front.silent:
            # no route: another clustering (or pipeline) through its own `__call__`; with `training` set a
            # SpeakerDiarization takes the front end from the cache that `prepare` filled
            output = pipeline(file) if found is None else pipeline._empty_output(file)
            found = _Outcome(hypothesis=get_diarization(output))
            self._score(metric, file, found.hypothesis)
            return found
        num_speakers, min_speakers, max_speakers = item.bounds
        same = [known for known in item.evaluated if known.other == other]
        known = None
        if found.train_labels is not None:       # the same training labels: the same assignment, not computed again
            known = next((k for k in same if k.train_labels is not None
                          and np.array_equal(k.train_labels, found.train_labels)), None)
            if known is None:
                plan, clustering = item.trees[pipeline.clustering.method], pipeline.clustering
                found.hard, _, found.centroids = clustering.assign_embeddings(
                    front.embeddings, plan.chunk_idx, plan.speaker_idx, found.train_labels,
                    constrained=clustering.constrained_assignment, device_embeddings=front.dev_emb)
        elif found.hard is None:                 # no route found anything: the pipeline's own clustering
            found.hard, found.centroids = pipeline._cluster_one(front, num_speakers, min_speakers, max_speakers)
        if known is None:
            known = next((k for k in same if np.array_equal(k.hard, found.hard)), None)
        if known is not None:
            self.shared_evaluations += 1
            found.hypothesis = known.hypothesis
            self._score(metric, file, known.hypothesis, known.components)
            return found
        fresh = replace(front, marks=[("start", time.perf_counter())], enqueued={})
        output = pipeline._back_end(fresh, found.hard, found.centroids, min_speakers, max_speakers,
                                    pipeline.setup_hook(file, None))
        found.hypothesis, found.other = get_diarization(output), other
        found.components = self._score(metric, file, found.hypothesis)
        item.evaluated.append(found)
        return found

    @staticmethod
    def _score(metric, file, hypothesis, components=None):
        """accumulates one file into `metric` and returns its components: computed by the metric, or -- for the
        package's metrics, whose accumulation is a sum of component dicts -- copied from an equal evaluation"""
        if components is not None and hasattr(metric, "accumulated_") and hasattr(metric, "results_"):
            metric.add_components(dict(components), getattr(file["annotation"], "uri", None) or "NA")
            return components
        computed = metric(file["annotation"], hypothesis, uem=file.get("annotated"), detailed=True)
        return computed if isinstance(computed, dict) else None


# ------------------------------------------------------------------------------------ detection thresholds
@dataclass
class _Detection:
    """one file of a detection corpus: its aggregated scores (uploaded once when the pipeline sits on a GPU) and the
    rows the metric's integrals are taken from"""
    file: dict
    scores: object            # (T, K) float32: device tensor, or numpy on the host
    frames: object
    ref_labels: list
    ref_seg: np.ndarray
    ref_lab: np.ndarray
    uem_seg: np.ndarray
    device_rows: dict = field(default_factory=dict)     # the reference and uem rows on the counting device


def _ranges(starts: np.ndarray, lengths: np.ndarray) -> np.ndarray:
    """concatenated arange(starts[i], starts[i] + lengths[i])"""
    total = int(lengths.sum())
    if total == 0:
        return np.zeros(0, dtype=np.int64)
    first = np.cumsum(lengths) - lengths
    return np.repeat(starts - first, lengths) + np.arange(total, dtype=np.int64)


def candidate_counts(item: _Detection, rows, offsets, counts, entry_jobs, todo, names, collar: float,
                     skip_overlap: bool, device, workspace_bytes: int) -> dict:
    """The metric's integrals of one file for the entries `todo` of `entry_jobs` (an entry: one job of the sweep per
    class of `names`; `rows`, `offsets`, `counts`: the sweep's rows, where job j's begin, and how many it has).
    -> entry -> (hypothesis labels in `labels()` order, the Kr Kh + Kr + Kh + 7 values of `pa_annot_counts`).
    On `device`: `pa_annot_corpus_counts` with one corpus entry per (file, candidate) -- the reference and uem rows
    repeated on the device, the hypothesis rows where the sweep left them (a job's rows are sorted: runs are plain
    ranges), only the tables uploaded; one download per call, calls chunked at the entry point's limits and at
    `workspace_bytes`.  Without a device, or for an entry beyond those limits: the host sweep."""
    order = sorted(range(len(names)), key=lambda k: str(names[k]))         # `Annotation.labels()`
    Nr, Nu, Kr = len(item.ref_seg), len(item.uem_seg), len(item.ref_labels)
    labels, runs, Nh, slots = {}, {}, {}, {}
    for e in todo:       # classes without rows are not labels of the hypothesis
        picked = [k for k in order if counts[entry_jobs[e, k]] > 0]
        labels[e] = [names[k] for k in picked]
        runs[e] = np.array([int(entry_jobs[e, k]) for k in picked], dtype=np.int64)
        Nh[e] = int(counts[runs[e]].sum())
        slots[e] = cut_slots(Nr, Nh[e], Nu)
    out = {}
    entries = [e for e in todo if device is not None and Kr <= am.MAX_LABELS and slots[e] <= (1 << 22)]
    if entries:
        if device not in item.device_rows:
            item.device_rows[device] = (torch.from_numpy(np.ascontiguousarray(item.ref_seg)).to(device),
                                        torch.from_numpy(item.ref_lab.astype(np.int32)).to(device),
                                        torch.from_numpy(np.ascontiguousarray(item.uem_seg)).to(device))
        ref_seg, ref_lab, uem_seg = item.device_rows[device]
        hyp = rows.to(device).contiguous()
    at = 0
    while at < len(entries):
        chunk, hyp_rows, used = [], 0, 0
        while at < len(entries) and len(chunk) < 65535 and (not chunk or corpus_workspace_bytes(
                hyp_rows + Nh[entries[at]], used + slots[entries[at]]) <= workspace_bytes):
            chunk.append(entries[at])
            hyp_rows += Nh[entries[at]]
            used += slots[entries[at]]
            at += 1
        F = len(chunk)
        jobs = np.concatenate([runs[e] for e in chunk])
        # (every entry reads the same reference and uem rows: repeated, so that the offset tables stay offsets)
        call = CorpusCall(device, [Nr] * F, [Nh[e] for e in chunk], [Nu] * F, [Kr] * F, [len(runs[e]) for e in chunk],
                          counts[jobs], _ranges(offsets[jobs], counts[jobs]),
                          {"ref_seg": ref_seg.repeat(F, 1), "ref_label": ref_lab.repeat(F),
                           "uem_seg": uem_seg.repeat(F, 1), "hyp_seg": hyp})
        values, _ = call.split(call.run(0.0, collar, skip_overlap).cpu().numpy())
        out.update({e: (labels[e], v) for e, v in zip(chunk, values)})
    rest = [e for e in todo if e not in out]
    if rest:
        host_rows = rows.cpu().numpy()
        for e in rest:
            seg = np.concatenate([host_rows[offsets[j]:offsets[j + 1]] for j in runs[e]] or [np.zeros((0, 2))])
            lab = np.repeat(np.arange(len(runs[e]), dtype=np.int32), counts[runs[e]])
            out[e] = (labels[e], am._host_counts(item.ref_seg, item.ref_lab, Kr, seg, lab, len(labels[e]),
                                                 item.uem_seg, collar, skip_overlap))
    return out


class DetectionTuner:
    """`DetectionTuner(pipeline).prepare(files).sweep(onsets, offsets, min_duration_ons, min_duration_offs)` for a
    `VoiceActivityDetection` or `MultiLabelSegmentation` pipeline -> {"entries": [{"params", "loss"} per candidate],
    "best": the first optimum in the pipeline's direction, "shared": how many detectors the candidates name and how
    many hysteresis lanes and duration jobs they were computed from, ...} (`write_config` takes it).

    The whole hyper-parameter set of these pipelines is what the reference's `optimize` searches, so a candidate
    costs no network and no Annotation: per file, ONE region sweep gives the region lists of all candidates
    (`frames.binarize_regions_sweep`: distinct (class, onset, offset) triples are lanes, distinct (lane, durations)
    pairs are jobs, a candidate is one job per class) and ONE counts call gives the metric's integrals of every
    (file, candidate) (`pa_annot_corpus_counts` with the hypothesis rows where the sweep left them; the host sweep
    without a device or beyond its limits).  The loss of a candidate is `abs(metric)` after `metric.add_counts` of
    every file, equal (`==`) to `pipeline.instantiate(params)`, `pipeline(file)` and
    `metric(file["annotation"], hypothesis, uem=file["annotated"])` per file with the same metric.

    `metric`: a factory of fresh metrics.  Default: `pipeline.get_metric` for VoiceActivityDetection;
    `annotation_metrics.IdentificationErrorRate` (`MacroAverageFMeasure` with `fscore`) on the pipeline's device for
    MultiLabelSegmentation, whose `get_metric` needs pyannote.metrics.  A metric without `add_counts` gets
    Annotations built from the region lists.  `keep_hypotheses`: also keep every candidate's Annotations in
    `self.hypotheses[candidate][file]`.  The pipeline is left instantiated with the last candidate."""

    #: bound on the workspace of one counts call (`evaluation.corpus_workspace_bytes`) and on the sweep's
    workspace_bytes: int = 1 << 30

    def __init__(self, pipeline, metric: Optional[Callable] = None, keep_hypotheses: bool = False):
        from .multilabel import MultiLabelSegmentation
        from .voice_activity_detection import VoiceActivityDetection
        self.pipeline = pipeline
        self.multilabel = isinstance(pipeline, MultiLabelSegmentation)
        if not self.multilabel and not isinstance(pipeline, VoiceActivityDetection):
            raise TypeError("DetectionTuner tunes VoiceActivityDetection and MultiLabelSegmentation pipelines, got "
                            f"{type(pipeline).__name__}")
        self.classes = list(pipeline.classes())
        self.powerset = bool(pipeline._segmentation.model.specifications.powerset)
        if metric is not None:
            self.metric = metric
        elif not self.multilabel:
            self.metric = pipeline.get_metric
        elif pipeline.fscore:
            self.metric = lambda: am.MacroAverageFMeasure(classes=self.classes, device=self._device())
        else:
            self.metric = lambda: am.IdentificationErrorRate(device=self._device())
        self.keep_hypotheses = keep_hypotheses
        self.prepared: list = []
        self.hypotheses: list = []

    def _device(self):
        device = getattr(self.pipeline._segmentation, "device", None)
        return device if device is not None and device.type == "cuda" else None

    # ------------------------------------------------------------------------------------------ preparation
    def prepare(self, files: Iterable) -> "DetectionTuner":
        """every file's aggregated scores, from its training cache or computed (and cached) once, uploaded once when
        the pipeline sits on a GPU; `pipeline.training` is restored whatever happens"""
        pipeline = self.pipeline
        previous = pipeline.training
        pipeline.training = True
        try:
            self.prepared = [self._prepare_one(file) for file in files]
        finally:
            pipeline.training = previous
        return self

    def _prepare_one(self, file) -> _Detection:
        from collections.abc import MutableMapping
        pipeline = self.pipeline
        origin, file = file, pipeline.prepare_one(file)
        if file.get("annotated") is None:
            raise ValueError(f"file {file.get('uri')!r} has no 'annotated': the evaluated region would be approximated "
                             "by the extent of a hypothesis that changes with the candidate")
        key = pipeline.CACHED_SEGMENTATION
        if key not in file:
            if self.multilabel:
                scores, frames = pipeline._aggregate(file, pipeline.setup_hook(file, None))
                from .core import SlidingWindowFeature
                file[key] = SlidingWindowFeature(scores.cpu().numpy(), frames)
            else:
                file[key] = pipeline._segmentation(file)
        cached = file[key]
        if isinstance(origin, MutableMapping) and key not in origin:     # (`prepare_one` works on a copy)
            origin[key] = cached
        data = np.ascontiguousarray(cached.data, dtype=np.float32)
        if data.ndim != 2 or data.shape[1] != len(self.classes):
            raise ValueError(f"cached scores of shape {data.shape}, (frames, {len(self.classes)}) expected")
        device = self._device()
        scores = torch.from_numpy(data).to(device) if device is not None else data
        ref_labels, ref_seg, ref_lab = am._rows(file["annotation"])
        uem_seg = am._uem_rows(file["annotated"])
        am._check("reference", ref_seg)
        am._check("uem", uem_seg)
        return _Detection(file=file, scores=scores, frames=cached.sliding_window, ref_labels=ref_labels,
                          ref_seg=ref_seg, ref_lab=ref_lab, uem_seg=uem_seg)

    # ------------------------------------------------------------------------------------------- candidates
    def candidates(self, onsets=None, offsets=None, min_duration_ons=(0.0,), min_duration_offs=(0.0,)) -> tuple:
        """(parameter dicts of the grid, onsets outermost, then offsets, min_duration_on, min_duration_off; how many
        grid points were left out because `offset > onset`, which VoiceActivityDetection does not reproduce)"""
        if self.powerset and not self.multilabel:
            if onsets is not None or offsets is not None:
                raise ValueError("the onset and offset of a powerset model are fixed: only the durations are tuned")
            pairs = [(None, None)]
        else:
            if onsets is None:
                raise ValueError("DetectionTuner.sweep: no onsets")
            pairs = [(float(a), float(a) if offsets is None else float(b))
                     for a in onsets for b in ([None] if offsets is None else offsets)]
        out, skipped = [], 0
        for onset, offset in pairs:
            if not self.multilabel and onset is not None and np.float32(offset or onset) > np.float32(onset):
                skipped += len(min_duration_ons) * len(min_duration_offs)
                continue
            for d_on in min_duration_ons:
                for d_off in min_duration_offs:
                    d_on, d_off = float(d_on), float(d_off)
                    if not self.multilabel:
                        params = {"min_duration_on": d_on, "min_duration_off": d_off}
                        if onset is not None:
                            params.update(onset=onset, offset=offset)
                    elif self.pipeline.share_min_duration:
                        params = {"thresholds": {c: {"onset": onset, "offset": offset} for c in self.classes},
                                  "min_duration_on": d_on, "min_duration_off": d_off}
                    else:
                        params = {"thresholds": {c: {"onset": onset, "offset": offset, "min_duration_on": d_on,
                                                     "min_duration_off": d_off} for c in self.classes}}
                    out.append(params)
        return out, skipped

    def sweep(self, onsets=None, offsets=None, min_duration_ons=(0.0,), min_duration_offs=(0.0,)) -> dict:
        """the grid in that nesting order; `offsets=None`: offset = onset; the same values for every class"""
        candidates, skipped = self.candidates(onsets, offsets, min_duration_ons, min_duration_offs)
        result = self.evaluate(candidates)
        result["skipped_offset_above_onset"] = skipped
        return result

    def _detectors(self, params) -> list:
        """instantiates the candidate and reads back what the pipeline will binarize with: per class
        (onset, offset, min_duration_on, min_duration_off), thresholds rounded to float32 (the comparison's type)"""
        pipeline = self.pipeline
        if self.multilabel:
            pipeline.instantiate(params)
            rows = zip(pipeline._onset, pipeline._offset, pipeline._min_duration_on, pipeline._min_duration_off)
        else:
            if self.powerset and ("onset" in params or "offset" in params):
                raise ValueError("the onset and offset of a powerset model are fixed")
            pipeline.instantiate(params)
            binarize = pipeline._binarize
            rows = [(binarize.onset, binarize.offset, binarize.min_duration_on, binarize.min_duration_off)]
        out = []
        for onset, offset, d_on, d_off in rows:
            values = (float(np.float32(onset)), float(np.float32(offset)), float(d_on), float(d_off))
            if any(np.isnan(values)):
                raise ValueError(f"a candidate has a NaN parameter: {params}")
            if not self.multilabel and values[1] > values[0]:
                raise ValueError(
                    f"offset {offset} > onset {onset}: VoiceActivityDetection's Binarize takes a frame between the two "
                    "as active, where the reference swaps the state; a value tuned there would not reproduce")
            out.append(values)
        return out

    # ------------------------------------------------------------------------------------------- evaluation
    def evaluate(self, candidates: list) -> dict:
        """any list of parameter dicts (as `pipeline.instantiate` takes them), in order"""
        if not self.prepared:
            raise RuntimeError("DetectionTuner: call prepare(files) first")
        candidates = list(candidates)
        K = len(self.classes)
        lanes, jobs, picks = {}, {}, []
        for params in candidates:
            pick = []
            for k, (onset, offset, d_on, d_off) in enumerate(self._detectors(params)):
                lane = lanes.setdefault((k, onset, offset), len(lanes))
                pick.append(jobs.setdefault((lane, d_on, d_off), len(jobs)))
            picks.append(tuple(pick))
        picks_array = np.array(picks, dtype=np.int64).reshape(len(candidates), K)
        lane_class = np.array([key[0] for key in lanes], dtype=np.int32)
        onset = np.array([key[1] for key in lanes], dtype=np.float32)
        offset = np.array([key[2] for key in lanes], dtype=np.float32)
        job_lane = np.array([key[0] for key in jobs], dtype=np.int32)
        d_on = np.array([key[1] for key in jobs], dtype=np.float64)
        d_off = np.array([key[2] for key in jobs], dtype=np.float64)
        job_class = lane_class[job_lane] if len(jobs) else np.zeros(0, dtype=np.int32)

        probe = self.metric()
        by_counts = hasattr(probe, "add_counts") and hasattr(probe, "collar") and hasattr(probe, "skip_overlap")
        variant = (float(probe.collar), bool(probe.skip_overlap)) if by_counts else None
        device = am._device(getattr(probe, "device", None)) if by_counts else None
        # distinct job tuples: two candidates with the same detectors share their counts
        distinct = {}
        entry_of = [distinct.setdefault(pick, len(distinct)) for pick in picks]
        entry_jobs = np.array(list(distinct), dtype=np.int64).reshape(len(distinct), K)

        metrics = [probe] + [self.metric() for _ in candidates[1:]]
        self.hypotheses = [[] for _ in candidates] if self.keep_hypotheses else []
        self.collisions = 0
        for item in self.prepared:
            self._evaluate_file(item, (lane_class, onset, offset, job_lane, d_on, d_off), job_class, entry_jobs,
                                entry_of, metrics, variant, device)
        entries = [{"params": params, "loss": abs(metric)} for params, metric in zip(candidates, metrics)]
        direction = self.pipeline.get_direction()
        return {"entries": entries, "best": best_entry(entries, direction),
                "shared": {"candidates": len(candidates), "detectors": len(candidates) * K, "lanes": len(lanes),
                           "jobs": len(jobs), "counted": len(distinct), "collisions": self.collisions}}

    def _evaluate_file(self, item: _Detection, tables, job_class, entry_jobs, entry_of, metrics, variant, device):
        """one sweep and one counts call for all candidates, then every candidate's metric takes the file.
        `variant`: the (collar, skip_overlap) of metrics that take counts (on `device`), None for any other metric"""
        from . import frames as frame_ops
        K = len(self.classes)
        by_counts = variant is not None
        want_tracks = K > 1 or self.keep_hypotheses or not by_counts
        rows, tracks, offsets = frame_ops.binarize_regions_sweep(
            item.scores, item.frames, *tables, return_tracks=want_tracks, to_host=False,
            workspace_bytes=self.workspace_bytes)
        counts = np.diff(offsets)
        flagged = self._collisions(rows, tracks, counts, job_class, entry_jobs) if K > 1 else set()
        self.collisions += sum(1 for e in entry_of if e in flagged)
        flat = {}
        host = None
        if by_counts:
            todo = [e for e in range(len(entry_jobs)) if e not in flagged]
            flat = candidate_counts(item, rows, offsets, counts, entry_jobs, todo,
                                    [self._labels(k) for k in range(K)], *variant, device, self.workspace_bytes)
        need_annotations = self.keep_hypotheses or not by_counts or flagged
        if need_annotations:
            host = (rows.cpu().numpy(), tracks.cpu().numpy())
        uri = getattr(item.file["annotation"], "uri", None)
        built = {}
        for c, (e, metric) in enumerate(zip(entry_of, metrics)):
            hypothesis = None
            if self.keep_hypotheses or e not in flat:
                if e not in built:
                    built[e] = self._annotation(item, host, offsets, entry_jobs[e])
                hypothesis = built[e]
            if e in flat:
                hyp_labels, values = flat[e]
                metric.add_counts(am.counts_dict(item.ref_labels, hyp_labels, values), uri=uri)
            else:
                metric(item.file["annotation"], hypothesis, uem=item.file["annotated"])
            if self.keep_hypotheses:
                self.hypotheses[c].append(hypothesis)

    def _labels(self, k: int):
        return self.classes[k] if self.multilabel else "SPEECH"

    def _annotation(self, item, host, offsets, picked):
        """the Annotation the pipeline returns for one candidate, from the sweep's rows"""
        from .core import Annotation
        from .multilabel import regions_to_annotation
        rows, tracks = host
        regions = [rows[offsets[j]:offsets[j + 1]] for j in picked]
        positions = [tracks[offsets[j]:offsets[j + 1]] for j in picked]
        if not sum(len(r) for r in regions):
            return Annotation(uri=item.file["uri"])
        return regions_to_annotation(regions, positions, [self._labels(k) for k in range(len(picked))],
                                     item.file["uri"])

    def _collisions(self, rows, tracks, counts, job_class, entry_jobs) -> set:
        """entries in which two classes hold a row with equal start, end and track position: the pipeline's
        Annotation is keyed by (segment, track name), so the later class overwrites the earlier one's row there.
        Those candidates are scored on the Annotation itself."""
        if rows.shape[0] == 0:
            return set()
        dev = rows.device
        job_of_row = torch.repeat_interleave(torch.arange(len(counts), device=dev),
                                             torch.from_numpy(counts).to(dev))
        cls = torch.from_numpy(job_class.astype(np.int64)).to(dev)[job_of_row]
        keys = torch.cat([rows.contiguous().view(torch.int64), tracks.to(torch.int64)[:, None]], dim=1)
        # a key held by two classes: distinct (key, class) pairs first, then keys that are left more than once
        pairs = torch.unique(torch.cat([keys, cls[:, None]], dim=1), dim=0)
        shared, held = torch.unique(pairs[:, :3], dim=0, return_counts=True)
        shared = shared[held > 1]
        if shared.shape[0] == 0:
            return set()
        both, inverse = torch.unique(torch.cat([shared, keys]), dim=0, return_inverse=True)
        is_shared = torch.zeros(both.shape[0], dtype=torch.bool, device=dev)
        is_shared[inverse[:shared.shape[0]]] = True
        hit = is_shared[inverse[shared.shape[0]:]]
        suspects = {}
        for job, key in zip(job_of_row[hit].cpu().tolist(), inverse[shared.shape[0]:][hit].cpu().tolist()):
            suspects.setdefault(job, set()).add(key)
        flagged = set()
        for e, picked in enumerate(entry_jobs.tolist()):
            seen = [suspects[j] for j in picked if j in suspects]
            if len(seen) > 1 and any(a & b for i, a in enumerate(seen) for b in seen[i + 1:]):
                flagged.add(e)
        return flagged


# ----------------------------------------------------------------------------------- online thresholds
class OnlineTuner:
    """`OnlineTuner(pipeline).prepare(files).sweep(delta_news, min_actives, min_updates)` for an
    `online.OnlineSpeakerDiarization`: the three thresholds of the online rule act only inside the clustering step, so
    a file's front end (`StreamBank.front_end`: segmentation, statistics, masks, embeddings of every chunk) is computed
    ONCE by `prepare`, and a candidate is a replay of the same (chunks x speakers) embeddings through the rule with
    other numbers.  `evaluate(candidates)` -- dicts with "delta_new", "min_active", "min_update" -- makes every
    (file, distinct triple) a job of `StreamBank.replay_pairs` (`pao_replay`: one workgroup per job, launches split
    by `StreamBank.replay_bytes`).  Distinct means distinct (min_active_frames, min_update_frames, delta_new): two
    candidates whose seconds round to the same frame counts share a job.  Equal decision arrays of a file share the
    Annotation and its metric components.

    -> {"entries": [{"params", "loss"}], "best": the first minimum, "evaluations": candidates x files,
    "shared_evaluations": the (candidate, file) pairs that reused another candidate's job or hypothesis}.  The loss of
    a candidate is what a fresh pipeline with its three values, streaming `apply` per file and
    `metric(file["annotation"], hypothesis, uem=file.get("annotated"))` give.  `apply_best(result)` writes the three
    values into `pipeline.bank_options`; they are constructor arguments, not `Parameter`s, so there is no
    `write_config` leg."""

    NAMES = ("delta_new", "min_active", "min_update")

    def __init__(self, pipeline, metric: Optional[Callable] = None):
        self.pipeline = pipeline
        self.metric = metric if metric is not None else pipeline.get_metric
        self.bank = None
        self.files: list = []
        self.front_ends: list = []
        self.shared_evaluations = 0
        self.evaluations = 0
        #: per candidate, per file: the speaker diarization that was scored
        self.hypotheses: list = []
        #: of the last `evaluate`: jobs replayed (distinct triples x files)
        self.jobs = 0

    def prepare(self, files: Iterable) -> "OnlineTuner":
        """runs every file's front end once, consecutive files sharing launch groups"""
        from .audio import Audio
        self.files = [Audio.validate_file(f) for f in files]
        self.bank = self.pipeline.bank(1)
        audio = Audio(sample_rate=self.bank.sample_rate, mono="downmix")
        self.front_ends = self.bank.front_ends([audio(f)[0].reshape(-1) for f in self.files])
        return self

    def candidates(self, delta_news, min_actives, min_updates) -> list:
        return [{"delta_new": float(d), "min_active": float(a), "min_update": float(u)}
                for d in delta_news for a in min_actives for u in min_updates]

    def sweep(self, delta_news, min_actives, min_updates) -> dict:
        """the grid, `delta_news` outermost"""
        return self.evaluate(self.candidates(delta_news, min_actives, min_updates))

    def evaluate(self, candidates: list) -> dict:
        if self.bank is None:
            raise RuntimeError("OnlineTuner: call prepare(files) first")
        bank = self.bank
        triples, job_of = {}, []
        for params in candidates:
            active, update = bank.threshold_frames(params["min_active"], params["min_update"])
            job_of.append(triples.setdefault((float(params["delta_new"]), active, update), len(triples)))
        triples = list(triples)
        pairs = [(f, t) for f in range(len(self.files)) for t in range(len(triples))]
        replayed = bank.replay_pairs(self.front_ends, triples, pairs)
        self.jobs = len(pairs)
        self.shared_evaluations = self.evaluations = 0
        self.hypotheses = []
        # per file: hypothesis and metric components of every distinct decision array, and which a job gave
        known = [dict() for _ in self.files]
        of_job = [dict() for _ in self.files]
        entries = []
        for c, params in enumerate(candidates):
            metric = self.metric()
            row = []
            for f, file in enumerate(self.files):
                self.evaluations += 1
                t = job_of[c]
                key = of_job[f].get(t)
                if key is None:
                    rows = replayed[f * len(triples) + t].decisions
                    key = of_job[f][t] = rows.tobytes()
                    fresh = key not in known[f]
                    if fresh:
                        known[f][key] = [bank.annotation_of(rows, uri=file.get("uri")), None]
                else:
                    fresh = False
                hypothesis, components = known[f][key]
                if fresh or components is None:
                    known[f][key][1] = ClusteringTuner._score(metric, file, hypothesis)
                else:
                    self.shared_evaluations += 1
                    ClusteringTuner._score(metric, file, hypothesis, components)
                row.append(hypothesis)
            self.hypotheses.append(row)
            entries.append({"params": params, "loss": abs(metric)})
        direction = self.pipeline.get_direction() if hasattr(self.pipeline, "get_direction") else "minimize"
        return {"entries": entries, "best": best_entry(entries, direction),
                "shared_evaluations": self.shared_evaluations, "evaluations": self.evaluations}

    def apply_best(self, result: dict) -> dict:
        """writes the best candidate's three values into `pipeline.bank_options` -> those values"""
        best = {name: float(result["best"]["params"][name]) for name in self.NAMES}
        self.pipeline.bank_options.update(best)
        return best


def write_config(config_yml, result: dict, name: str) -> Path:
    """`<stem>.<name>.yaml` next to `config_yml`: the loaded config with `params` replaced by the best candidate's and
    the reference's `optimization` block (__main__.py:267-277); `name` stands in for its protocol and subset"""
    import yaml
    config_yml = Path(config_yml)
    with open(config_yml, "r") as fp:
        config = yaml.load(fp, Loader=yaml.SafeLoader)
    best = result["best"]
    config["params"] = copy.deepcopy(best["params"])
    config["optimization"] = {"protocol": name, "subset": name,
                              "status": {"best_loss": float(best["loss"]),
                                         "last_updated": datetime.now().isoformat()}}
    out = config_yml.with_suffix(f".{name}.yaml")
    with open(out, "w") as fp:
        yaml.dump(config, fp)
    return out
