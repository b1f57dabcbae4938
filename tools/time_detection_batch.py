"""Wall time of `list(pipeline(files))` for the two detection pipelines on one audio-hour cut into files, with and
without `pack=True` (apply_batch of detection_batch.py: the files of a group share one segmentation forward, one
`pa_aggregate_files` and one pass of `pa_binarize_regions_files`), synthetic conversations.

Workloads (one audio-hour each): 120 x 30 s, 12 x 5 min and 1 x 1 h (nothing to pack) for VoiceActivityDetection, the
first of them for MultiLabelSegmentation.  Per workload: two warm-ups of each form, then the two forms ALTERNATING,
`--runs` (5) timed runs each; the clock is a host clock around the whole call followed by a device synchronise.
Reports the median and [min, max] per form, the groups `pack=True` formed, whether the two forms gave the same
Annotations, and -- from one more packed run with a device synchronise after every stage -- the time of the three group
calls apart from the host time spent building Annotations.

usage (GPU box):  python tools/time_detection_batch.py [--runs 5] [--out FILE] [--no-pack]
`--no-pack`: time the plain list call only, without passing `pack` at all (a checkout from before the option existed:
the reference for what `pack=False` must still cost)."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import yaml

import bench
import pyannote_audio_amd as pa

SR = 16000
CLASSES = ["speech", "music", "noise"]


def cut(hour: torch.Tensor, durations: list, tag: str) -> list:
    files, a = [], 0
    for i, d in enumerate(durations):
        b = a + int(round(d * SR))
        files.append({"waveform": hour[:, a:b].clone(), "sample_rate": SR, "uri": f"{tag}_{i:03d}"})
        a = b
    return files


def signature(outputs) -> list:
    return [(f["uri"], o.uri, [(s.start, s.end, t, l) for s, t, l in o.itertracks(yield_label=True)])
            for f, o in outputs]


def multilabel_pipeline(workdir: str):
    """a multi-label checkpoint (three named classes) in the reference's format, and its pipeline"""
    from oracle.synthetic import calibrated_multilabel_pyannet
    from pyannote_audio_amd.model import Problem, PyanNet, Resolution, Specifications, save_checkpoint
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import PYANNET_HPARAMS
    root = os.path.join(workdir, "multilabel")
    os.makedirs(os.path.join(root, "segmentation"))
    spec = Specifications(problem=Problem.MULTI_LABEL_CLASSIFICATION, resolution=Resolution.FRAME, duration=10.0,
                          min_duration=None, warm_up=(0.0, 0.0), classes=list(CLASSES), permutation_invariant=False)
    save_checkpoint(os.path.join(root, "segmentation", "pytorch_model.bin"),
                    calibrated_multilabel_pyannet(calib_seconds=40.0).state_dict(), PYANNET_HPARAMS,
                    PyanNet.ARCHITECTURE, spec)
    thresholds = {c: {"onset": 0.6, "offset": 0.4, "min_duration_on": 0.05, "min_duration_off": 0.1} for c in CLASSES}
    with open(os.path.join(root, "config.yaml"), "w") as fp:
        yaml.safe_dump({"version": "3.1.0",
                        "pipeline": {"name": "pyannote.audio.pipelines.MultiLabelSegmentation",
                                     "params": {"segmentation": "$model/segmentation"}},
                        "params": {"thresholds": thresholds}}, fp)
    return pa.Pipeline.from_pretrained(root)


def stage_times(pipeline, files) -> dict:
    """one packed run with a device synchronise after every stage: ms per stage, summed over the groups"""
    import pyannote_audio_amd.frames as frame_ops
    import pyannote_audio_amd.multilabel as multilabel
    engine = pipeline._segmentation.model.engine
    spent = {}

    def timed(name, fn):
        def wrapper(*args, **kwargs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*args, **kwargs)
            torch.cuda.synchronize()
            spent[name] = spent.get(name, 0.0) + 1e3 * (time.perf_counter() - t0)
            return out
        return wrapper

    saved = (engine.forward_files, frame_ops.aggregate_files, frame_ops.binarize_regions_files,
             multilabel.regions_to_annotation)
    engine.forward_files = timed("forward_files", saved[0])
    frame_ops.aggregate_files = timed("aggregate_files", saved[1])
    frame_ops.binarize_regions_files = timed("binarize_regions_files (with its two copies)", saved[2])
    multilabel.regions_to_annotation = timed("Annotations (host)", saved[3])
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        list(pipeline([dict(f) for f in files], pack=True))
        torch.cuda.synchronize()
        spent["whole call"] = 1e3 * (time.perf_counter() - t0)
    finally:
        del engine.forward_files
        frame_ops.aggregate_files, frame_ops.binarize_regions_files, multilabel.regions_to_annotation = saved[1:]
    return spent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-pack", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    workdir = tempfile.mkdtemp(prefix="pa_detect_")
    bench.build_checkpoints(workdir)
    vad = pa.VoiceActivityDetection(segmentation=os.path.join(workdir, "segmentation"))
    vad.instantiate({"min_duration_on": 0.05, "min_duration_off": 0.1}).to(device)
    multilabel = multilabel_pipeline(workdir).to(device)
    hour = bench.synth_hour(1.0, seed=0, device=device)
    workloads = [("VoiceActivityDetection", vad, "120 x 30 s", [30.0] * 120),
                 ("VoiceActivityDetection", vad, "12 x 5 min", [300.0] * 12),
                 ("VoiceActivityDetection", vad, "1 x 1 h", [3600.0]),
                 ("MultiLabelSegmentation", multilabel, "120 x 30 s", [30.0] * 120)]
    forms = [("plain", {})] if args.no_pack else [("pack=False", {"pack": False}), ("pack=True", {"pack": True})]
    say(f"# time_detection_batch: {torch.cuda.get_device_name(0)}, {args.runs} alternating runs per form after 2 "
        f"warm-ups each; ms per call of list(pipeline(files)) over one audio-hour, host clock + device synchronise")

    def run(pipeline, files, kwargs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outputs = list(pipeline([dict(f) for f in files], **kwargs))
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), outputs

    for who, pipeline, name, durations in workloads:
        files = cut(hour, durations, name.split()[0])
        results, times = {}, {form: [] for form, _ in forms}
        for _ in range(2):
            for form, kwargs in forms:
                _, results[form] = run(pipeline, files, kwargs)
        groups = [len(g) for g in getattr(pipeline, "last_pack_groups", [])]
        for _ in range(args.runs):
            for form, kwargs in forms:
                times[form].append(run(pipeline, files, kwargs)[0])
        regions = sum(len(rows) for _, _, rows in signature(results[forms[-1][0]]))
        say(f"\n## {who}, {name}: {len(files)} files, {sum(durations):.0f} s of audio, {regions} regions")
        for form, _ in forms:
            t = times[form]
            say(f"{form:>11}: median {statistics.median(t):8.1f} ms   [{min(t):8.1f}, {max(t):8.1f}]   "
                f"runs {' '.join(f'{x:.1f}' for x in t)}")
        if not args.no_pack:
            a, b = statistics.median(times["pack=False"]), statistics.median(times["pack=True"])
            same = signature(results["pack=False"]) == signature(results["pack=True"])
            say(f"  pack=True / pack=False = {b / a:.3f}   groups of pack=True (files per group): {groups}   "
                f"same Annotations: {same}")
            spent = stage_times(pipeline, files)
            whole = spent.pop("whole call")
            rest = whole - sum(spent.values())
            say("  one packed run, synchronised after every stage: " +
                ", ".join(f"{k} {v:.1f} ms" for k, v in spent.items()) +
                f", loading the files and the rest {rest:.1f} ms (whole call {whole:.1f} ms)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
