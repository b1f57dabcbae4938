"""Times the tail of MultiLabelSegmentation on one synthetic audio-hour: from "chunk scores on the device" to
"Annotation returned",

  (a) through the device path: pa_aggregate (result stays on the device) -> pa_binarize_regions -> Annotation;
  (b) through the composition available before that path existed: chunk scores copied to the host, frames.aggregate
      (upload, pa_aggregate, copy back), crop, diarization.Binarize per class, labels renamed, annotations merged.

Thresholds (0.6, 0.4) -- offset <= onset, where both give the same regions (checked) -- with minimum durations 0 and
0.1 s.  Warm-up, then the median of repeated runs; host clock around a synchronised region.

    python tools/multilabel_tail.py [--out FILE] [--repeats N]
    python tools/multilabel_tail.py --device-path-only      (a few runs of (a): for a kernel trace)"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLASSES = ["speech", "music", "noise"]


def build_pipeline(device):
    import pyannote_audio_amd as pa
    from conftest import PYANNET_HPARAMS
    from oracle.synthetic import calibrated_multilabel_pyannet
    from pyannote_audio_amd.model import Problem, PyanNet, Resolution, Specifications, save_checkpoint
    seg_o = calibrated_multilabel_pyannet(calib_seconds=40.0)
    path = os.path.join(tempfile.mkdtemp(), "pytorch_model.bin")
    spec = Specifications(problem=Problem.MULTI_LABEL_CLASSIFICATION, resolution=Resolution.FRAME, duration=10.0,
                          min_duration=None, warm_up=(0.0, 0.0), classes=list(CLASSES), permutation_invariant=False)
    save_checkpoint(path, seg_o.state_dict(), PYANNET_HPARAMS, PyanNet.ARCHITECTURE, spec)
    return pa.MultiLabelSegmentation(segmentation=path).to(device)


def rows(annotation):
    return [(s.start, s.end, t, l) for s, t, l in annotation.itertracks(yield_label=True)]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=None)
    parser.add_argument("--repeats", type=int, default=15)
    parser.add_argument("--device-path-only", action="store_true")
    args = parser.parse_args()

    from oracle.synthetic import synth_conversation
    from pyannote_audio_amd import frames as frame_ops
    from pyannote_audio_amd.core import Annotation, Segment, SlidingWindow, SlidingWindowFeature
    from pyannote_audio_amd.diarization import Binarize
    device = torch.device("cuda:0")
    pipeline = build_pipeline(device)
    inference = pipeline._segmentation
    minute, _ = synth_conversation(120.0, seed=11)
    wav = minute.repeat(1, 30)                                  # one hour
    seconds = wav.shape[1] / 16000
    inference.slide_device(wav.to(device), 16000)
    chunk_scores = inference.last_device_output                 # (chunks, 589, 3) float32 on the device
    C, F, K = chunk_scores.shape
    chunks = SlidingWindow(start=0.0, duration=inference.duration, step=inference.step)
    receptive_field = inference.model.receptive_field
    lines = [f"MultiLabelSegmentation tail, {seconds:.0f} s of audio: {C} chunks x {F} frames x {K} classes on the device"]

    def device_path():
        scores, frames = frame_ops.aggregate_device(chunk_scores, chunks, receptive_field, device, hamming=True,
                                                    missing=0.0)
        return pipeline._detect(scores, frames, "hour")

    def host_path(onset, offset, d_on, d_off):
        outputs = chunk_scores.cpu().numpy()
        aggregated = frame_ops.aggregate(outputs, chunks, receptive_field, device, hamming=True, missing=0.0)
        aggregated.data = aggregated.crop(Segment(0.0, seconds), mode="loose")
        detection = Annotation(uri="hour")
        binarize = Binarize(onset=onset, offset=offset, min_duration_on=d_on, min_duration_off=d_off)
        for k, label in enumerate(CLASSES):
            active = binarize(SlidingWindowFeature(aggregated.data[:, k:k + 1], aggregated.sliding_window))
            detection.update(active.rename_labels({l: label for l in active.labels()}, copy=False))
        return detection

    def timed(fn, repeats, warmup=3):
        for _ in range(warmup):
            fn()
        samples = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            samples.append(time.perf_counter() - t0)
        return statistics.median(samples), min(samples), max(samples)

    for d in (0.0, 0.1):
        pipeline.instantiate({"thresholds": {c: {"onset": 0.6, "offset": 0.4, "min_duration_on": d,
                                                 "min_duration_off": d} for c in CLASSES}})
        if args.device_path_only:
            for _ in range(5):
                device_path()
            torch.cuda.synchronize()
            continue
        new, old = device_path(), host_path(0.6, 0.4, d, d)
        same = rows(new) == rows(old)
        a = timed(device_path, args.repeats)
        b = timed(lambda: host_path(0.6, 0.4, d, d), max(args.repeats // 3, 5))
        lines.append(f"min_duration_on = min_duration_off = {d:g} s: {len(rows(new))} regions, "
                     f"same regions on both paths: {same}")
        lines.append(f"  (a) device path   median {1e3 * a[0]:9.3f} ms   (min {1e3 * a[1]:.3f}, max {1e3 * a[2]:.3f}, "
                     f"{args.repeats} runs)")
        lines.append(f"  (b) host path     median {1e3 * b[0]:9.3f} ms   (min {1e3 * b[1]:.3f}, max {1e3 * b[2]:.3f}, "
                     f"{max(args.repeats // 3, 5)} runs)")
        lines.append(f"  (b) / (a) = {b[0] / a[0]:.1f}")
    if not args.device_path_only:
        T = 1 + int(np.rint((chunks.duration + (C - 1) * chunks.step) / receptive_field.step))
        lines.append(f"bytes, T ~ {T} frames: pa_aggregate reads {4 * C * F * K} and writes {4 * T * K}; "
                     f"pa_binarize_regions reads the scores twice ({2 * 4 * T * K}), writes and reads one event word "
                     f"per frame ({2 * 4 * T}) and two count words per class and 64 frames ({2 * 4 * K * (T // 64)}); "
                     f"host copies on the device path: {K} counts, then 16 bytes + 4 bytes per region")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(text + "\n")


if __name__ == "__main__":
    main()
