"""Tuning the clustering of a `SpeakerDiarization` pipeline on a corpus: the search the reference's `optimize` command
runs (src/pyannote/audio/__main__.py:116-283 -- the pipeline applied to every development file again for every
candidate `clustering.threshold` / `min_cluster_size`), organised so that a candidate only pays for what depends on it.

  once per file      the front end (both networks; kept in the file dict by the pipeline's training cache),
                     `filter_embeddings` and the dendrogram (it depends on `method`, not on the threshold)
  once per file      ALL candidate cuts of that dendrogram: `Dendrogram.cuts` (`pa_dendrogram_cuts`, one launch)
  per candidate      the rest of `AgglomerativeClustering.cluster` on the cut labels, `assign_embeddings`, the back end
                     and the metric -- and not even those when an earlier candidate gave this file the same
                     `hard_clusters` (two thresholds between the same pair of merge heights do): its results are copies

There is no sampler, no journal and no `pyannote.database` here: the candidates are a grid in the order given, files
are dicts as `evaluation.benchmark` takes them ("annotation", optionally "annotated" and "pipeline_kwargs")."""
from __future__ import annotations

import copy
import time
from dataclasses import dataclass, field, replace
from datetime import datetime
from pathlib import Path
from typing import Callable, Iterable, Optional

import numpy as np

from . import distance
from .clustering import AgglomerativeClustering, Dendrogram
from .evaluation import get_diarization


@dataclass
class _Prepared:
    """one file of the corpus: its validated dict, its (cached) front end, the speaker bounds of its
    `pipeline_kwargs`, and per linkage method what the clustering needs before the cut"""
    file: dict
    front: object
    bounds: tuple
    trees: dict = field(default_factory=dict)     # method -> None or (tree, train, chunk_idx, speaker_idx, bounds)
    evaluated: list = field(default_factory=list)  # [(train labels, hard_clusters, hypothesis, components, other params)]


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


class ClusteringTuner:
    """`ClusteringTuner(pipeline).prepare(files).sweep(thresholds, min_cluster_sizes)` -> {"entries": [{"params",
    "loss"} per candidate, thresholds outermost], "best": the first minimum, "shared_evaluations": how many (candidate,
    file) pairs reused an earlier candidate's back end and metric components, "evaluations": all such pairs}.

    `metric`: a factory of fresh metrics (default `pipeline.get_metric`); the loss of a candidate is `abs(metric)`
    after every file, i.e. what `pipeline.instantiate(params)`, `pipeline(file)` per file and
    `metric(file["annotation"], output, uem=file.get("annotated"))` give.  Every parameter but the two swept ones
    stays as the pipeline is instantiated; the pipeline is left instantiated with the last candidate."""

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

    def _tree(self, item: _Prepared):
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
                with distance.device_to_ourselves():
                    tree = Dendrogram(clustering.dendrogram(train))
                item.trees[method] = (tree, train, chunk_idx, speaker_idx, bounds)
        return item.trees[method]

    #: "device" cuts every dendrogram with `pa_dendrogram_cuts` on the pipeline's GPU, "host" runs the same plan
    #: through numpy (profiles/clustering_tuning_timing.txt has both at one audio-hour)
    cut_on: str = "device"

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

    def evaluate(self, candidates: list) -> dict:
        """any list of parameter dicts, in order.  With `AgglomerativeClustering` every file's dendrogram (one per
        linkage method among the candidates) is cut ONCE, at the thresholds of all candidates."""
        if not self.prepared:
            raise RuntimeError("ClusteringTuner: call prepare(files) first")
        pipeline = self.pipeline
        agglomerative = isinstance(getattr(pipeline, "clustering", None), AgglomerativeClustering)
        self.shared_evaluations = self.evaluations = 0
        self.train_clusters, self.hypotheses = [], []
        for item in self.prepared:
            item.evaluated = []
        thresholds, cuts = [], {}
        if agglomerative:
            thresholds = list(dict.fromkeys(float(params["clustering"]["threshold"]) for params in candidates))
        row_of = {t: k for k, t in enumerate(thresholds)}
        previous = pipeline.training
        pipeline.training = True      # (the generic path goes through the pipeline's call: cached front ends there too)
        entries = []
        try:
            for params in candidates:
                pipeline.instantiate(params)
                # results are shared only between candidates that differ in nothing but the clustering
                self._beyond_clustering = repr({name: value for name, value in params.items() if name != "clustering"})
                metric = self.metric()
                self.train_clusters.append([])
                self.hypotheses.append([])
                for i, item in enumerate(self.prepared):
                    labels = None
                    if agglomerative and item.front is not None and not item.front.silent:
                        key = (i, pipeline.clustering.method)
                        if key not in cuts:
                            plan = self._tree(item)
                            cuts[key] = None if plan is None else plan[0].cuts(thresholds, device=self.cut_device())
                        if cuts[key] is not None:
                            labels = cuts[key][row_of[float(pipeline.clustering.threshold)]]
                    self._evaluate(item, labels, metric)
                    self.train_clusters[-1].append(self._train_clusters)
                entries.append({"params": params, "loss": abs(metric)})
        finally:
            pipeline.training = previous
        direction = pipeline.get_direction() if hasattr(pipeline, "get_direction") else "minimize"
        return {"entries": entries, "best": best_entry(entries, direction),
                "shared_evaluations": self.shared_evaluations, "evaluations": self.evaluations}

    def _evaluate(self, item: _Prepared, cut_labels, metric):
        """one file under the currently instantiated candidate, accumulated into `metric`"""
        pipeline, front, file = self.pipeline, item.front, item.file
        self.evaluations += 1
        self._train_clusters = None
        if front is None or not isinstance(getattr(pipeline, "clustering", None), AgglomerativeClustering):
            # another clustering (or pipeline): the candidate through its own `__call__`; with `training` set a
            # SpeakerDiarization takes the front end from the cache that `prepare` filled
            return self._score(metric, file, get_diarization(pipeline(file)), None)
        if front.silent:
            return self._score(metric, file, get_diarization(pipeline._empty_output(file)), None)
        num_speakers, min_speakers, max_speakers = item.bounds
        clustering = pipeline.clustering
        train_labels = None
        if cut_labels is None:       # one cluster whatever the candidate says (`_tree`)
            hard, centroids = pipeline._cluster_one(front, num_speakers, min_speakers, max_speakers)
        else:
            tree, train, chunk_idx, speaker_idx, (num, lo, hi) = item.trees[clustering.method]
            train_labels = clustering.cluster_from_cut(train, tree, cut_labels, min_clusters=lo, max_clusters=hi,
                                                       num_clusters=num)
            self._train_clusters = int(np.max(train_labels)) + 1
            for known in item.evaluated:       # the same training labels: the same assignment, not computed again
                if known[0] is not None and known[4] == self._beyond_clustering \
                        and np.array_equal(known[0], train_labels):
                    return self._share(metric, file, known)
            hard, _, centroids = clustering.assign_embeddings(
                front.embeddings, chunk_idx, speaker_idx, train_labels,
                constrained=clustering.constrained_assignment, device_embeddings=front.dev_emb)
        for known in item.evaluated:
            if known[4] == self._beyond_clustering and np.array_equal(known[1], hard):
                return self._share(metric, file, known)
        fresh = replace(front, marks=[("start", time.perf_counter())], enqueued={})
        output = pipeline._back_end(fresh, hard, centroids, min_speakers, max_speakers, pipeline.setup_hook(file, None))
        hypothesis = get_diarization(output)
        components = self._score(metric, file, hypothesis, None)
        item.evaluated.append((train_labels, hard, hypothesis, components, self._beyond_clustering))

    def _share(self, metric, file, known):
        self.shared_evaluations += 1
        self._score(metric, file, known[2], known[3])

    def _score(self, metric, file, hypothesis, components):
        """accumulates one file into `metric` and returns its components: computed by the metric, or -- for the
        package's metrics, whose accumulation is a sum of component dicts -- copied from an equal evaluation"""
        self.hypotheses[-1].append(hypothesis)
        if components is not None and hasattr(metric, "accumulated_") and hasattr(metric, "results_"):
            metric.results_.append((getattr(file["annotation"], "uri", None) or "NA", dict(components)))
            for name in metric.accumulated_:
                metric.accumulated_[name] += components[name]
            return components
        computed = metric(file["annotation"], hypothesis, uem=file.get("annotated"), detailed=True)
        return computed if isinstance(computed, dict) else None


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
