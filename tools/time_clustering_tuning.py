"""Time a search over `clustering.threshold` on a synthetic corpus (GPU), three ways with the same candidates.

Input: bench.py's `synth_hour` for seeds 0.. as audio (one file per entry of --minutes), the turns it draws as the
reference (`bench_turns` of tools/time_annotation_metrics.py), bench.py's synthetic speaker-diarization-3.1 directory as
the pipeline.  Candidates: --thresholds values spread over the quantiles of the files' own merge heights.

  (a) the literal loop with `training` off: `pipeline.instantiate(params)`, `pipeline(file)` for every file, a fresh
      metric -- both networks run again for every candidate;
  (b) the same loop with `training` on: cached front ends, but a new dendrogram and a SciPy `fcluster` per candidate
      and file;
  (c) `tuning.ClusteringTuner.sweep`: one dendrogram per file, one `Dendrogram.cuts` call per file, the back end only
      for assignments not seen before.  Timed with the cuts on the device and with the host plan path.

Every candidate of (a) and (b) is timed by the host clock (it ends with its results on the host); (c) is timed as a
whole, --repeats times, alternating the two cut paths, `prepare` (the front ends, once) apart.  All legs must give the
same losses and the same best parameters.

Apart from that: `Dendrogram.cuts` for 32 thresholds of one centroid dendrogram over 7 176 unit-norm 256-d points on the
device (plan build and upload in the first call, then further calls), the host plan path, and 32
`scipy.cluster.hierarchy.fcluster` calls on this machine's CPU, --repeats times each, alternating.

Writes profiles/clustering_tuning_timing.txt (or --out)."""
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


def loop(pipeline, files, candidates):
    """-> (losses, seconds per candidate)"""
    losses, seconds = [], []
    for params in candidates:
        def one():
            pipeline.instantiate(params)
            metric = pipeline.get_metric()
            for file in files:
                metric(file["annotation"], pipeline(file).speaker_diarization, uem=file["annotated"])
            return abs(metric)
        dt, loss = clock(one)
        losses.append(loss)
        seconds.append(dt)
    return losses, seconds


def cut_timings(device, repeats: int, count: int) -> list:
    from scipy.cluster.hierarchy import fcluster
    from pyannote_audio_amd import distance
    from pyannote_audio_amd.clustering import Dendrogram
    rng = np.random.default_rng(11)
    centres = rng.normal(size=(12, 256))
    X = centres[rng.integers(0, 12, size=7176)] + 0.6 * rng.normal(size=(7176, 256))
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    Z = distance.linkage_centroid(X, device)
    heights = np.sort(Z[:, 2])
    thresholds = np.quantile(heights, np.linspace(0.02, 0.999, count))
    Dendrogram(Z).cuts(thresholds[:1], device=device)             # warm-up: code object, allocator
    t_plan, _ = clock(lambda: Dendrogram(Z).plan())
    tree = Dendrogram(Z)
    t_first, got = clock(lambda: tree.cuts(thresholds, device=device))
    dev, host, scipy_ = [], [], []
    want = None
    for _ in range(repeats):
        dev.append(clock(lambda: tree.cuts(thresholds, device=device))[0])
        host.append(clock(lambda: tree.cuts(thresholds))[0])
        dt, want = clock(lambda: np.stack([fcluster(Z, t, criterion="distance") - 1 for t in thresholds]))
        scipy_.append(dt)
    same = bool((got == want).all() and (tree.cuts(thresholds) == want).all())
    ffi_report = device_share(lambda: tree.cuts(thresholds, device=device), "k_dendrogram_cuts")
    beats = statistics.median(dev) < min(scipy_)
    return [
        f"`Dendrogram.cuts`, {count} thresholds over the quantiles of the heights, one centroid dendrogram of 7 176 "
        "unit-norm 256-d points (host clock, labels back on the host):",
        f"  plan (host C++, once per dendrogram)        {t_plan * 1e3:10.3f} ms",
        f"  device, first call (plan + upload + cuts)   {t_first * 1e3:10.3f} ms",
        f"  device, further calls                       {ms(dev)}   kernel (events) {ffi_report:.3f} ms",
        f"  host plan path (numpy), further calls       {ms(host)}",
        f"  {count} x scipy fcluster on this machine's CPU   {ms(scipy_)}",
        f"  rows equal to fcluster - 1: {same};  the device cut beats SciPy at this size: {beats}"
        + ("" if beats else "   <-- it does NOT"),
    ], same


def device_share(fn, kernel: str) -> float:
    import pyannote_audio_amd.ffi as ffi
    ffi.prof_enable(True)
    ffi.prof_report()
    fn()
    torch.cuda.synchronize()
    report = ffi.prof_report()
    ffi.prof_enable(False)
    return report[kernel]["ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, nargs="+", default=[10.0, 20.0, 30.0])
    ap.add_argument("--thresholds", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clustering_tuning_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import pyannote_audio_amd as pa
    import pyannote_audio_amd.ffi as ffi
    from bench import build_checkpoints
    from pyannote_audio_amd.tuning import ClusteringTuner
    ffi.require_gpu()
    device = torch.device("cuda:0")
    workdir = tempfile.mkdtemp(prefix="tuning_timing_")
    build_checkpoints(workdir)
    pipeline = pa.Pipeline.from_pretrained(workdir).to(device)
    files = corpus(args.minutes, device)

    # (c) first: its dendrograms give the thresholds
    t_prepare, tuner = clock(lambda: ClusteringTuner(pipeline).prepare(files))
    trees = [tuner._tree(item) for item in tuner.prepared]
    heights = np.concatenate([plan.tree.Z[:, 2] for plan in trees])
    thresholds = [float(t) for t in np.quantile(heights, np.linspace(0.5, 0.9995, args.thresholds))]
    tuner.sweep(thresholds[:2])                                   # warm-up
    sweeps = {"device": [], "host": []}
    results = {}
    for _ in range(args.repeats):
        for where in ("device", "host"):
            tuner.cut_on = where
            dt, results[where] = clock(lambda: tuner.sweep(thresholds))
            sweeps[where].append(dt)
    result = results["device"]
    candidates = [e["params"] for e in result["entries"]]
    losses_c = [e["loss"] for e in result["entries"]]
    clusters = sorted({row[-1] for row in tuner.train_clusters})

    bare = [{k: v for k, v in f.items() if not k.startswith("training_cache/")} for f in files]
    loop(pipeline, bare, candidates[:1])                          # warm-up
    losses_a, seconds_a = loop(pipeline, bare, candidates)
    pipeline.training = True
    try:
        loop(pipeline, files, candidates[:1])
        losses_b, seconds_b = loop(pipeline, files, candidates)
    finally:
        pipeline.training = False
    same_losses = losses_a == losses_b == losses_c == [e["loss"] for e in results["host"]["entries"]]
    best = result["best"]["params"]["clustering"]
    best_a = candidates[int(np.argmin(losses_a))]["clustering"]
    best_b = candidates[int(np.argmin(losses_b))]["clustering"]

    cut_lines, same_cuts = cut_timings(device, args.repeats, 32)
    total_a, total_b = sum(seconds_a), sum(seconds_b)
    med_c = statistics.median(sweeps["device"])
    spread_b = (max(seconds_b) - min(seconds_b)) * len(candidates)
    spread_a = (max(seconds_a) - min(seconds_a)) * len(candidates)
    train = [plan.train.shape[0] for plan in trees]
    lines = [
        f"tools/time_clustering_tuning.py --minutes {' '.join(f'{m:g}' for m in args.minutes)} --thresholds "
        f"{args.thresholds} --repeats {args.repeats}",
        f"device: {torch.cuda.get_device_name(0)}",
        f"input: {len(files)} synthetic files of {', '.join(f'{m:g}' for m in args.minutes)} min (bench.py synth_hour "
        f"seeds 0..{len(files) - 1}, their drawn turns as the reference), {sum(train)} training embeddings "
        f"({', '.join(map(str, train))}); {len(candidates)} candidate thresholds over the quantiles 0.5..0.9995 of the "
        f"files' merge heights ({thresholds[0]:.4f}..{thresholds[-1]:.4f}), every other parameter as in "
        "speaker-diarization-3.1; metric: the pipeline's own (GreedyDiarizationErrorRate on the device)",
        f"training clusters of the last file over the candidates: {clusters[0]}..{clusters[-1]} "
        f"({len(clusters)} different counts)",
        "",
        f"(a) literal loop, training off   : {total_a:8.3f} s for {len(candidates)} candidates; per candidate {ms(seconds_a)}",
        f"(b) literal loop, cached front end: {total_b:8.3f} s for {len(candidates)} candidates; per candidate {ms(seconds_b)}",
        f"(c) ClusteringTuner.sweep, device cuts: whole sweep {ms(sweeps['device'])}  ({args.repeats} sweeps)",
        f"    ClusteringTuner.sweep, host plan cuts: whole sweep {ms(sweeps['host'])}",
        f"    prepare (front ends of all files, once; not in the sweep times, as the first candidate of (b) pays it): "
        f"{t_prepare:.3f} s;  evaluations shared with an earlier candidate: {result['shared_evaluations']} of "
        f"{result['evaluations']}",
        f"same losses in (a), (b), (c device) and (c host): {same_losses};  best parameters: (a) {best_a}  (b) {best_b}  "
        f"(c) {best};  best loss {result['best']['loss']:.6f}",
        "",
        f"(a) / (b) = {total_a / total_b:.1f};  (b) / (c) = {total_b / med_c:.1f};  (a) / (c) = {total_a / med_c:.1f}",
        f"(b) is not slower than (a) beyond the spread of (a): {total_b <= total_a + spread_a};  (c) is not slower than "
        f"(b) beyond the spread of (b): {med_c <= total_b + spread_b}",
        "",
    ] + cut_lines
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(text)
    assert same_losses and best == best_a == best_b and same_cuts, "the legs disagree"


if __name__ == "__main__":
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        main()
