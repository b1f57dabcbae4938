"""Time a search over the detection thresholds on a synthetic corpus (GPU), three ways with the same candidates.

Input: bench.py's `synth_hour` for seeds 0.. as audio (one file per entry of --minutes), the turns it draws as the
reference (`bench_turns` of tools/time_annotation_metrics.py), a seeded NON-powerset segmentation model with the
calibrated read-out of oracle.synthetic (three scores per frame).  The network runs once per file (`prepare`).

VoiceActivityDetection: the grid --onsets x --offsets x --durations x --durations over the quantiles of the files' own
scores; grid points with offset > onset are left out (tuning.DetectionTuner says why) and counted.
MultiLabelSegmentation (3 classes, the speakers as classes): a smaller grid, all threshold orders.

  (a) the literal loop on cached scores: `pipeline.instantiate(params)`, `pipeline(file)` for every file (training
      mode: no network), a fresh metric on the device.  It builds and lists an Annotation per candidate and file, so
      it is timed per candidate on --literal candidates spread evenly over the grid and scaled to the grid;
  (b) `DetectionTuner.evaluate` with the numpy forms of the sweep and of the counts (scores and metric on the host);
  (c) `DetectionTuner.evaluate` on the device: one region sweep and one counts call per file.

The legs alternate, --repeats times, after a warm-up of each, with a device synchronise inside every timed window.
(a) and (c) count on the device and must give the same losses (`==`) on (a)'s candidates; (b) counts with the numpy
sweep, whose additions run in another order: its losses must agree with (c)'s within 1e-12 over the whole grid, and
all three must choose the same best parameters.

Apart from that, from device events (the library's profiler): the sweep and the counts call for one hour-sized file
(T = 213 334 frames) at 256 lanes x 16 jobs each.

Writes profiles/detection_tuning_timing.txt (or --out)."""
import argparse
import os
import statistics
import sys
import tempfile
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLASSES = ["spk0", "spk1", "spk2"]


def checkpoint(path: str) -> str:
    from conftest import PYANNET_HPARAMS
    from oracle.synthetic import calibrated_multilabel_pyannet
    from pyannote_audio_amd.model import Problem, PyanNet, Resolution, Specifications, save_checkpoint
    spec = Specifications(problem=Problem.MULTI_LABEL_CLASSIFICATION, resolution=Resolution.FRAME, duration=10.0,
                          min_duration=None, warm_up=(0.0, 0.0), classes=list(CLASSES), permutation_invariant=False)
    save_checkpoint(path, calibrated_multilabel_pyannet(calib_seconds=60.0).state_dict(), PYANNET_HPARAMS,
                    PyanNet.ARCHITECTURE, spec)
    return path


def corpus(minutes: list, device) -> list:
    import pyannote_audio_amd as pa
    from bench import synth_hour
    from pyannote_audio_amd.core import Segment
    from time_annotation_metrics import bench_turns
    files = []
    for seed, length in enumerate(minutes):
        hours = length / 60.0
        turns = bench_turns(hours, seed=seed)
        uri = f"synth{seed:02d}"
        reference = pa.Annotation.from_columns([t[0] for t in turns], [t[1] for t in turns], list(range(len(turns))),
                                               [f"spk{t[2]}" for t in turns], uri=uri)
        files.append({"waveform": synth_hour(hours, seed=seed, device=device), "sample_rate": 16000, "uri": uri,
                      "annotation": reference, "annotated": [Segment(0.0, hours * 3600.0)]})
    return files


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def ms(values) -> str:
    return f"median {statistics.median(values) * 1e3:10.3f} ms   [{min(values) * 1e3:.3f}, {max(values) * 1e3:.3f}]"


def literal(pipeline, files, candidates, metric_factory):
    """-> (losses, seconds per candidate); the pipeline in training mode takes the cached scores"""
    losses, seconds = [], []
    pipeline.training = True
    try:
        for params in candidates:
            def one():
                pipeline.instantiate(params)
                metric = metric_factory()
                for file in files:
                    metric(file["annotation"], pipeline(file), uem=file["annotated"])
                return abs(metric)
            dt, loss = clock(one)
            losses.append(loss)
            seconds.append(dt)
    finally:
        pipeline.training = False
    return losses, seconds


def host_tuner(tuner_class, pipeline, files, metric_factory):
    """a tuner whose scores stay on the host and whose metric counts there: the numpy forms"""
    tuner = tuner_class(pipeline, metric=metric_factory)
    tuner._device = lambda: None
    return tuner.prepare(files)


def run(name, pipeline, files, candidates, picked, device_metric, host_metric, repeats, note):
    from pyannote_audio_amd.tuning import DetectionTuner, best_entry
    on_device = DetectionTuner(pipeline, metric=device_metric).prepare(files)
    on_host = host_tuner(DetectionTuner, pipeline, files, host_metric)
    subset = [candidates[i] for i in picked]
    literal(pipeline, files, subset[:1], device_metric)           # warm-ups
    on_host.evaluate(candidates[:2])
    on_device.evaluate(candidates[:2])
    times = {"a": [], "b": [], "c": []}
    for _ in range(repeats):
        losses_a, seconds = literal(pipeline, files, subset, device_metric)
        times["a"].append(sum(seconds))
        dt, result_b = clock(lambda: on_host.evaluate(candidates))
        times["b"].append(dt)
        dt, result_c = clock(lambda: on_device.evaluate(candidates))
        times["c"].append(dt)
    losses_b = [e["loss"] for e in result_b["entries"]]
    losses_c = [e["loss"] for e in result_c["entries"]]
    # (a) and (c) count with the same kernels and must agree to the bit; (b) counts with the numpy sweep, whose
    # additions run in another order: its losses may differ from (c)'s in the last bits, and how much is reported
    same_ac = [losses_c[i] for i in picked] == losses_a
    differ_bc = sum(1 for x, y in zip(losses_b, losses_c) if x != y)
    worst_bc = max(abs(x - y) for x, y in zip(losses_b, losses_c))
    same = same_ac and worst_bc <= 1e-12
    same_best = result_b["best"]["params"] == result_c["best"]["params"]
    direction = pipeline.get_direction()
    best_a = best_entry([{"params": p, "loss": l} for p, l in zip(subset, losses_a)], direction)
    best_c_on_subset = best_entry([result_c["entries"][i] for i in picked], direction)
    same_best = same_best and best_a["params"] == best_c_on_subset["params"]
    scale = len(candidates) / len(subset)
    med = {k: statistics.median(v) for k, v in times.items()}
    shared = result_c["shared"]
    lines = [
        f"{name}: {len(candidates)} candidates{note}; {shared['lanes']} lanes, {shared['jobs']} jobs for "
        f"{shared['detectors']} detectors; {shared['collisions']} (file, candidate) pairs scored on the Annotation",
        f"  (a) literal loop on cached scores, {len(subset)} candidates spread over the grid: {ms(times['a'])}"
        f"  = {med['a'] / len(subset) * 1e3:.3f} ms per candidate; scaled to the grid: {med['a'] * scale:.3f} s",
        f"  (b) DetectionTuner, numpy forms, whole grid : {ms(times['b'])}",
        f"  (c) DetectionTuner, device, whole grid      : {ms(times['c'])}",
        f"  (a, scaled) / (c) = {med['a'] * scale / med['c']:.1f};  (b) / (c) = {med['b'] / med['c']:.1f};  "
        f"(c) is faster than (a): {med['c'] < med['a'] * scale}" +
        (f";  (c) on the whole grid is faster than (a) on its {len(subset)} candidates alone: {med['c'] < med['a']}"),
        f"  losses of (a) == losses of (c) on (a)'s candidates: {same_ac};  (b) against (c) on the grid: {differ_bc} of "
        f"{len(candidates)} losses differ, by at most {worst_bc:.3g} (numpy sweep against device kernels: another "
        f"order of additions);  same best parameters in (a), (b), (c): {same_best};  best loss {result_c['best']['loss']:.6f} at {result_c['best']['params']}",
    ]
    return lines, same and same_best


def hour_sized(device, repeats: int) -> list:
    """device events of one sweep and one counts call: T = 213 334, 256 lanes x 16 jobs, one candidate per job"""
    import pyannote_audio_amd.ffi as ffi
    from multilabel_oracle import smooth_scores
    from pyannote_audio_amd import frames as frame_ops
    from pyannote_audio_amd.core import Annotation, Segment, SlidingWindow, SlidingWindowFeature
    from pyannote_audio_amd.tuning import DetectionTuner, _Detection, candidate_counts
    from pyannote_audio_amd import annotation_metrics as am
    from time_annotation_metrics import bench_turns
    T, L, J = 213334, 256, 16
    window = SlidingWindow(start=0.0, duration=0.0619375, step=0.016875)
    scores = torch.from_numpy(smooth_scores(np.random.default_rng(3), T, 1, width=25)).to(device)
    onset = np.linspace(0.35, 0.65, L).astype(np.float32)
    offset = (onset - np.float32(0.05)).astype(np.float32)
    job_lane = np.repeat(np.arange(L, dtype=np.int32), J)
    d_on = np.tile(np.repeat([0.0, 0.1, 0.2, 0.4], 4), L)
    d_off = np.tile(np.tile([0.0, 0.1, 0.2, 0.4], 4), L)
    tables = (np.zeros(L, dtype=np.int32), onset, offset, job_lane, d_on, d_off)
    turns = bench_turns(1.0, seed=0)
    reference = Annotation.from_columns([t[0] for t in turns], [t[1] for t in turns], list(range(len(turns))),
                                        [f"spk{t[2]}" for t in turns], uri="hour")
    ref_labels, ref_seg, ref_lab = am._rows(reference)
    item = _Detection(file={"uri": "hour"}, scores=scores, frames=window, ref_labels=ref_labels, ref_seg=ref_seg,
                      ref_lab=ref_lab, uem_seg=am._uem_rows([Segment(0.0, 3600.0)]))
    entry_jobs = np.arange(L * J, dtype=np.int64)[:, None]

    def once():
        rows, _, offsets = frame_ops.binarize_regions_sweep(scores, window, *tables, to_host=False)
        return rows, offsets, candidate_counts(item, rows, offsets, np.diff(offsets), entry_jobs,
                                               list(range(len(entry_jobs))), ["SPEECH"], 0.0, False, device,
                                               DetectionTuner.workspace_bytes)

    rows, offsets, _ = once()                                     # warm-up
    sweep_ms, counts_ms, calls = [], [], 0
    for _ in range(repeats):
        ffi.prof_enable(True)
        ffi.prof_report()
        once()
        torch.cuda.synchronize()
        report = ffi.prof_report()
        ffi.prof_enable(False)
        sweep_ms.append((report["k_regions_sweep_count"]["ms"] + report["k_regions_sweep_emit"]["ms"]) * 1e-3)
        counts_ms.append(report["k_annot_corpus_counts"]["ms"] * 1e-3)
        calls = report["k_annot_corpus_counts"]["launches"]
    per_job = np.diff(offsets)
    return [
        f"one hour-sized file (T = {T} frames, one class), {L} lanes x {J} jobs = {L * J} candidates, {len(ref_seg)} "
        f"reference turns; rows per job {int(per_job.min())}..{int(per_job.max())}, {int(offsets[-1])} rows in all; "
        "device events:",
        f"  region sweep (counting phase + emitting phase)         {ms(sweep_ms)}",
        f"  counts of all candidates ({calls} pa_annot_corpus_counts calls)   {ms(counts_ms)}",
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, nargs="+", default=[10.0, 20.0, 30.0])
    ap.add_argument("--onsets", type=int, default=16)
    ap.add_argument("--offsets", type=int, default=16)
    ap.add_argument("--durations", type=int, default=4)
    ap.add_argument("--literal", type=int, default=16, help="candidates of the literal loop, spread over the grid")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detection_tuning_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import pyannote_audio_amd as pa
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd import annotation_metrics as am
    from pyannote_audio_amd.tuning import DetectionTuner
    ffi.require_gpu()
    device = torch.device("cuda:0")
    ckpt = checkpoint(os.path.join(tempfile.mkdtemp(prefix="detection_timing_"), "seg.bin"))
    files = corpus(args.minutes, device)

    vad = pa.VoiceActivityDetection(segmentation=ckpt).to(device)
    t_prepare, tuner = clock(lambda: DetectionTuner(vad).prepare(files))
    scores = np.concatenate([f[vad.CACHED_SEGMENTATION].data.ravel() for f in files])
    scores = scores[~np.isnan(scores)]
    onsets = [float(q) for q in np.quantile(scores, np.linspace(0.2, 0.8, args.onsets))]
    offsets = [float(q) for q in np.quantile(scores, np.linspace(0.15, 0.75, args.offsets))]
    durations = [float(d) for d in np.linspace(0.0, 0.6, args.durations)]
    candidates, skipped = tuner.candidates(onsets, offsets, durations, durations)
    picked = [int(i) for i in np.linspace(0, len(candidates) - 1, args.literal)]
    grid = args.onsets * args.offsets * args.durations ** 2
    note = f" ({len(candidates)} of the {grid} grid points have offset <= onset, {skipped} are left out)"
    vad_lines, vad_ok = run("VoiceActivityDetection", vad, files, candidates, picked, vad.get_metric,
                            lambda: am.DetectionErrorRate(), args.repeats, note)

    multilabel = pa.MultiLabelSegmentation(segmentation=ckpt).to(device)
    for f in files:
        f.pop(vad.CACHED_SEGMENTATION, None)
    ml_tuner = DetectionTuner(multilabel).prepare(files)
    ml_scores = np.concatenate([f[multilabel.CACHED_SEGMENTATION].data.ravel() for f in files])
    ml_scores = ml_scores[~np.isnan(ml_scores)]
    ml_onsets = [float(q) for q in np.quantile(ml_scores, np.linspace(0.3, 0.8, 6))]
    ml_candidates, _ = ml_tuner.candidates(ml_onsets, ml_onsets, durations[:2], durations[:2])
    ml_picked = [int(i) for i in np.linspace(0, len(ml_candidates) - 1, min(args.literal, 8))]
    ml_lines, ml_ok = run("MultiLabelSegmentation, 3 classes", multilabel, files, ml_candidates, ml_picked,
                          lambda: am.IdentificationErrorRate(device=device), lambda: am.IdentificationErrorRate(),
                          args.repeats, " (6 onsets x 6 offsets x 2 x 2 durations, the same for every class)")

    lines = [
        f"tools/time_detection_tuning.py --minutes {' '.join(f'{m:g}' for m in args.minutes)} --onsets {args.onsets} "
        f"--offsets {args.offsets} --durations {args.durations} --literal {args.literal} --repeats {args.repeats}",
        f"device: {torch.cuda.get_device_name(0)}",
        f"input: {len(files)} synthetic files of {', '.join(f'{m:g}' for m in args.minutes)} min (bench.py synth_hour "
        f"seeds 0..{len(files) - 1}, their drawn turns as the reference), a seeded non-powerset segmentation model; "
        f"thresholds over the quantiles of the files' scores, durations {durations}",
        f"prepare (the network, once per file; in no leg's time): {t_prepare:.3f} s",
        "host-clock times of whole legs, a device synchronise inside every timed window; the legs alternate",
        "",
    ] + vad_lines + [""] + ml_lines + [""] + hour_sized(device, args.repeats)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(text)
    assert vad_ok and ml_ok, "the legs disagree"


if __name__ == "__main__":
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        main()
