"""Pipelines, corpora and the literal tuning loop for the `tuning.DetectionTuner` tests (TEST INFRASTRUCTURE ONLY).
Checkpoints are seeded as tests/test_multilabel_cpu.py seeds them; the aggregated scores are synthetic and sit in the
file dicts' cache keys, so no network runs."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import multilabel_oracle as mo  # noqa: E402

CLASSES = ["speech", "music", "noise"]
FRAMES = (0.0, 0.0619375, 0.016875)             # start, duration, step


def checkpoint(path, classes, powerset=False):
    from conftest import PYANNET_HPARAMS
    from oracle import seeded_pyannet
    from pyannote_audio_amd.model import (Problem, PyanNet, Resolution, Specifications, save_checkpoint,
                                          segmentation_specifications)
    state = seeded_pyannet(seed=5, num_layers=4).state_dict()
    if powerset:
        spec = segmentation_specifications(10.0, powerset=True)
    else:
        g = torch.Generator().manual_seed(1)
        state["classifier.weight"] = 0.1 * torch.randn(len(classes), 128, generator=g)
        state["classifier.bias"] = torch.zeros(len(classes))
        spec = Specifications(problem=Problem.MULTI_LABEL_CLASSIFICATION, resolution=Resolution.FRAME, duration=10.0,
                              min_duration=None, warm_up=(0.0, 0.0), classes=list(classes),
                              permutation_invariant=False)
    save_checkpoint(str(path), state, PYANNET_HPARAMS, PyanNet.ARCHITECTURE, spec)
    return str(path)


def corpus(cache_key, K, labels, seed=0, durations=(20.0, 31.0, 40.0), always_on=()):
    """seeded files: synthetic scores under `cache_key`, a random reference over `labels`, a uem with a hole"""
    from pyannote_audio_amd.core import Annotation, Segment, SlidingWindow, SlidingWindowFeature
    rng = np.random.default_rng(seed)
    files = []
    for n, seconds in enumerate(durations):
        T = int(seconds / FRAMES[2])
        data = mo.smooth_scores(rng, T, K, width=int(rng.integers(8, 40)), nan_fraction=0.01 if n == 1 else 0.0)
        for k in always_on:
            data[:, k] = 0.99
        scores = SlidingWindowFeature(data, SlidingWindow(start=FRAMES[0], duration=FRAMES[1], step=FRAMES[2]))
        reference = Annotation(uri=f"file{n}")
        for label in labels:
            t = float(rng.uniform(0.0, 2.0))
            while t < seconds - 1.0:
                length = float(rng.uniform(0.3, 4.0))
                reference[Segment(t, min(t + length, seconds)), label] = label
                t += length + float(rng.uniform(0.2, 3.0))
        hole = seconds * 0.4
        files.append({"waveform": torch.zeros(1, 1600), "sample_rate": 16000, "uri": f"file{n}",
                      "annotation": reference, cache_key: scores,
                      "annotated": [Segment(0.25, hole), Segment(hole + 1.5, seconds - 0.5)]})
    return files


def reference_and_uem(rng, uri, seconds, labels):
    from pyannote_audio_amd.core import Annotation, Segment
    reference = Annotation(uri=uri)
    for label in labels:
        t = float(rng.uniform(0.0, 2.0))
        while t < seconds - 1.0:
            length = float(rng.uniform(0.3, 4.0))
            reference[Segment(t, min(t + length, seconds)), label] = label
            t += length + float(rng.uniform(0.2, 3.0))
    hole = seconds * 0.4
    return reference, [Segment(0.25, hole), Segment(hole + 1.5, seconds - 0.5)]


@functools.lru_cache(maxsize=None)
def _conversation(seconds, seed):
    from oracle.synthetic import synth_conversation
    return synth_conversation(seconds, seed=seed)[0]


def audio_corpus(labels, seed=0, durations=(20.0, 31.0, 40.0)):
    """seeded synthetic conversations with a random reference and a uem with a hole; no cached scores"""
    rng = np.random.default_rng(seed)
    files = []
    for n, seconds in enumerate(durations):
        wav = _conversation(seconds, seed + n)
        reference, uem = reference_and_uem(rng, f"audio{n}", seconds, labels)
        files.append({"waveform": wav, "sample_rate": 16000, "uri": f"audio{n}", "annotation": reference,
                      "annotated": uem})
    return files


def rows(annotation):
    return [(s.start, s.end, t, l) for s, t, l in annotation.itertracks(yield_label=True)]


def literal_loop(pipeline, files, candidates, metric_factory):
    """`instantiate`, `pipeline(file)`, `metric(reference, hypothesis, uem=annotated)`; the pipeline in training mode,
    so that it takes the cached scores"""
    previous, pipeline.training = pipeline.training, True
    losses, hypotheses = [], []
    try:
        for params in candidates:
            pipeline.instantiate(params)
            metric = metric_factory()
            hypotheses.append([])
            for file in files:
                hypothesis = pipeline(file)
                metric(file["annotation"], hypothesis, uem=file["annotated"])
                hypotheses[-1].append(hypothesis)
            losses.append(abs(metric))
    finally:
        pipeline.training = previous
    return losses, hypotheses


def oracle_loop(pipeline, files, candidates, metric_factory):
    """the same loop for a MultiLabelSegmentation pipeline without a GPU: the hypothesis is built row by row from the
    frame-by-frame oracle, as the pipeline's Annotation is keyed ((segment, track) -> label, later classes overwrite)"""
    from pyannote_audio_amd.core import Annotation, Segment
    losses, hypotheses = [], []
    for params in candidates:
        pipeline.instantiate(params)
        metric = metric_factory()
        hypotheses.append([])
        for file in files:
            scores = file[pipeline.CACHED_SEGMENTATION]
            per_class = mo.all_regions(scores.data, *FRAMES, pipeline._onset, pipeline._offset,
                                       pipeline._min_duration_on, pipeline._min_duration_off)
            hypothesis = Annotation(uri=file["uri"])
            for (regions, positions), label in zip(per_class, pipeline.classes()):
                for (a, b), position in zip(regions, positions):
                    hypothesis[Segment(a, b), mo.track_name(position)] = label
            metric(file["annotation"], hypothesis, uem=file["annotated"])
            hypotheses[-1].append(hypothesis)
        losses.append(abs(metric))
    return losses, hypotheses


def multilabel_candidates(shared: bool, always_on_at=None):
    """per-class candidates, `offset > onset` among them, and one built to collide: two classes on throughout (their
    scores are 0.99 in `corpus(always_on=(0, 1))`) with min_duration_off = 0"""
    out = []
    grid = [((0.5, 0.4), (0.6, 0.6), (0.45, 0.55)), ((0.4, 0.6), (0.55, 0.0), (0.5, 0.3)),
            ((0.9, 0.9), (0.95, 0.5), (0.5, 0.5)), ((0.5, 0.4), (0.6, 0.6), (0.5, 0.3))]
    if always_on_at is not None:      # (scores are above this everywhere: both classes are one region, track "A")
        grid.append(((always_on_at, always_on_at), (always_on_at, always_on_at), (0.5, 0.5)))
    durations = [(0.0, 0.0), (0.1, 0.2), (0.3, 0.05)]
    for n, thresholds in enumerate(grid):
        for d_on, d_off in (durations if n < 2 else durations[:1]):
            per_label = {c: {"onset": a, "offset": b} for c, (a, b) in zip(CLASSES, thresholds)}
            if shared:
                out.append({"thresholds": per_label, "min_duration_on": d_on, "min_duration_off": d_off})
            else:
                for k, c in enumerate(CLASSES):
                    per_label[c].update(min_duration_on=d_on * (k + 1) / 2.0, min_duration_off=d_off if k else 0.0)
                out.append({"thresholds": per_label})
    return out
