"""Regenerates tests/golden/multilabel_v1.npz: what the REFERENCE'S OWN `Binarize` (utils/signal.py) and
`MultiLabelSegmentation.initialize` / `.apply` (pipelines/multilabel.py) make of fixed, seeded score arrays.

The reference is loaded where it lies by tests/refharness.py.  The pipeline object is created without its constructor
(which needs a model and `pyannote.audio`'s loader): `_classes`, `share_min_duration`, the instantiated `thresholds`
and a `_segmentation` that hands out the stored scores are set by hand; `initialize` and `apply` then run unchanged.
`pyannote.core` (Annotation, Segment, SlidingWindow, SlidingWindowFeature, string_generator) is the product's core.py
on both sides of every comparison made with this file, as everywhere in this repository: what is pinned here is the
reference's hysteresis rule, its region bookkeeping, its use of `support` and its track / label handling -- not
pyannote.core itself.  Arrays only; the cases are described where they are built.

Run from the repository root:  python tests/golden/make_multilabel_golden.py"""
import os
import sys

os.environ.setdefault("PYANNOTE_SKIP_DEPENDENCY_CHECK", "1")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refharness  # noqa: E402
from multilabel_oracle import smooth_scores  # noqa: E402  (score generator only)

CLASSES = ["speech", "music", "noise"]
FRAMES = (0.0, 0.0619375, 0.016875)          # start, duration, step of PyanNet's receptive field
T = 2000


def cases():
    """name -> scores (T, 3) float32, frames, onset, offset, min_duration_on, min_duration_off (3 each), shared"""
    rng = np.random.default_rng(20240607)
    zero = [0.0, 0.0, 0.0]
    out = {}
    out["offset_below_onset"] = (smooth_scores(rng, T, 3), FRAMES, [0.6, 0.55, 0.7], [0.4, 0.45, 0.2], zero, zero, False)
    out["offset_equals_onset"] = (smooth_scores(rng, T, 3), FRAMES, [0.5, 0.3, 0.62], [0.5, 0.3, 0.62], zero, zero, False)
    out["offset_above_onset"] = (smooth_scores(rng, T, 3), FRAMES, [0.4, 0.45, 0.2], [0.6, 0.55, 0.7], zero, zero, False)
    nan = smooth_scores(rng, T, 3, nan_fraction=0.02)
    nan[0, 0] = np.nan
    nan[0, 2] = np.nan
    nan[-1, 1] = np.nan
    out["nan"] = (nan, FRAMES, [0.6, 0.4, 0.5], [0.4, 0.6, 0.5], zero, [0.0, 0.05, 0.0], False)
    out["all_nan"] = (np.full((50, 3), np.nan, dtype=np.float32), FRAMES, [0.5] * 3, [0.5] * 3, zero, zero, False)
    out["all_on"] = (np.full((T, 3), 0.9, dtype=np.float32), FRAMES, [0.6, 0.4, 0.5], [0.4, 0.6, 0.5], zero, zero, False)
    out["all_off"] = (np.full((T, 3), 0.1, dtype=np.float32), FRAMES, [0.6, 0.4, 0.5], [0.4, 0.6, 0.5], zero, zero, False)
    # alternating scores: a region every two frames, the most a class can have (T / 2); column 1 starts low, column 2
    # sits between offset and onset with offset > onset: the state swaps on every frame
    alt = np.empty((T + 1, 3), dtype=np.float32)
    alt[0::2, 0], alt[1::2, 0] = 0.9, 0.1
    alt[0::2, 1], alt[1::2, 1] = 0.1, 0.9
    alt[:, 2] = 0.5
    out["alternating"] = (alt, FRAMES, [0.6, 0.6, 0.4], [0.4, 0.4, 0.6], zero, zero, False)
    out["alternating_collar"] = (alt[:401], FRAMES, [0.6, 0.6, 0.4], [0.4, 0.4, 0.6], [0.0, 0.02, 0.05],
                                 [0.02, 0.0, 0.0], False)
    last = np.full((300, 3), 0.1, dtype=np.float32)
    last[-1, 0] = 0.9                # opens on the last frame: an empty region, which does not exist
    last[-2:, 1] = 0.9               # opens one frame earlier: one step long
    last[100:120, 2] = 0.9
    last[-1, 2] = 0.9
    out["opens_on_last_frame"] = (last, (1.5, 0.0619375, 0.016875), [0.5] * 3, [0.5] * 3, zero, [0.0, 0.0, 0.1], False)
    out["two_frames"] = (np.array([[0.9, 0.1, 0.9], [0.9, 0.9, 0.1]], dtype=np.float32), FRAMES, [0.5] * 3, [0.5] * 3,
                         zero, zero, False)
    out["shared_min_duration"] = (smooth_scores(rng, T, 3, width=9), FRAMES, [0.6, 0.45, 0.5], [0.4, 0.55, 0.5],
                                  [0.1] * 3, [0.1] * 3, True)
    out["per_class_min_duration"] = (smooth_scores(rng, T, 3, width=9), FRAMES, [0.6, 0.45, 0.5], [0.4, 0.55, 0.5],
                                     [0.0, 0.3, 0.15], [0.2, 0.0, 0.15], False)
    # scores equal to the float32-rounded threshold and its two float32 neighbours.  0.4 rounds UP in float32 and 0.6
    # rounds DOWN (so does 0.7): in float64 `np.float32(0.4) > 0.4` would be true, in float32 it is not.
    edge = np.full((40, 3), 0.0, dtype=np.float32)
    for k, (on, off) in enumerate([(0.4, 0.6), (0.6, 0.4), (0.7, 0.7)]):
        on32, off32 = np.float32(on), np.float32(off)
        lo, hi = np.float32(min(on, off) - 0.2), np.float32(max(on, off) + 0.2)
        seq = [lo, on32, lo, np.nextafter(on32, np.float32(1)), off32, np.nextafter(off32, np.float32(1)),
               np.nextafter(off32, np.float32(0)), lo, np.nextafter(on32, np.float32(0)), hi, off32, hi,
               np.nextafter(off32, np.float32(0)), on32, np.nextafter(on32, np.float32(1)), lo]
        edge[:, k] = lo
        edge[2:2 + len(seq), k] = seq
        edge[22:22 + len(seq), k] = seq[::-1]
    out["threshold_neighbours"] = (edge, FRAMES, [0.4, 0.6, 0.7], [0.6, 0.4, 0.7], zero, zero, False)
    return out


def main():
    out = {"classes": np.array(CLASSES)}
    with refharness.reference_modules(third_party=True) as ref:
        ref.load_pipelines()                 # `from pyannote.audio import Inference, Pipeline` must resolve
        signal = ref.load("pyannote.audio.utils.signal")
        multilabel = ref.load("pyannote.audio.pipelines.multilabel")
        core = sys.modules["pyannote.core"]
        pipeline_base = sys.modules["pyannote.pipeline"].Pipeline
        names = []
        for name, (scores, frames, onset, offset, d_on, d_off, shared) in cases().items():
            names.append(name)
            window = core.SlidingWindow(start=frames[0], duration=frames[1], step=frames[2])
            out[f"{name}/scores"] = scores
            out[f"{name}/frames"] = np.array(frames, dtype=np.float64)
            for key, value in (("onset", onset), ("offset", offset), ("min_duration_on", d_on),
                               ("min_duration_off", d_off)):
                out[f"{name}/{key}"] = np.array(value, dtype=np.float64)
            out[f"{name}/shared"] = np.array(shared)

            # the reference's Binarize, class by class
            for k in range(len(CLASSES)):
                binarize = signal.Binarize(onset=onset[k], offset=offset[k], min_duration_on=d_on[k],
                                           min_duration_off=d_off[k])
                active = binarize(core.SlidingWindowFeature(scores[:, k:k + 1], window))
                rows = [(s.start, s.end, t) for s, t in active.itertracks()]
                out[f"{name}/binarize{k}_times"] = np.array([r[:2] for r in rows], dtype=np.float64).reshape(-1, 2)
                out[f"{name}/binarize{k}_tracks"] = np.array([r[2] for r in rows], dtype=str)

            # the reference's pipeline: initialize + apply
            pipeline = multilabel.MultiLabelSegmentation.__new__(multilabel.MultiLabelSegmentation)
            pipeline_base.__init__(pipeline)
            pipeline._classes = CLASSES
            pipeline.share_min_duration = shared
            pipeline.fscore = False
            feature = core.SlidingWindowFeature(scores, window)
            pipeline._segmentation = lambda file, hook=None, feature=feature: feature
            ParamDict = sys.modules["pyannote.pipeline.parameter"].ParamDict
            if shared:
                pipeline.thresholds = ParamDict(**{c: ParamDict(onset=None, offset=None) for c in CLASSES})
                Uniform = sys.modules["pyannote.pipeline.parameter"].Uniform
                pipeline.min_duration_on = Uniform(0.0, 2.0)
                pipeline.min_duration_off = Uniform(0.0, 2.0)
                params = {"min_duration_on": d_on[0], "min_duration_off": d_off[0],
                          "thresholds": {c: {"onset": onset[k], "offset": offset[k]} for k, c in enumerate(CLASSES)}}
            else:
                pipeline.thresholds = ParamDict(**{c: ParamDict(onset=None, offset=None, min_duration_on=None,
                                                                min_duration_off=None) for c in CLASSES})
                params = {"thresholds": {c: {"onset": onset[k], "offset": offset[k], "min_duration_on": d_on[k],
                                             "min_duration_off": d_off[k]} for k, c in enumerate(CLASSES)}}
            pipeline.instantiate(params)            # calls the reference's initialize()
            detection = pipeline.apply({"uri": name})
            assert detection.uri == name
            rows = [(s.start, s.end, t, l) for s, t, l in detection.itertracks(yield_label=True)]
            out[f"{name}/apply_times"] = np.array([r[:2] for r in rows], dtype=np.float64).reshape(-1, 2)
            out[f"{name}/apply_tracks"] = np.array([r[2] for r in rows], dtype=str)
            out[f"{name}/apply_labels"] = np.array([r[3] for r in rows], dtype=str)
            print(f"{name}: T = {len(scores)}, binarize regions = "
                  f"{[len(out[f'{name}/binarize{k}_times']) for k in range(3)]}, apply rows = {len(rows)}")
        out["cases"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "multilabel_v1.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
