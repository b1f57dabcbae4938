"""Time a search over `clustering.threshold` x `Fa` x `Fb` of a VBxClustering pipeline on a synthetic corpus (GPU), three
ways with the same candidates, and say where the time of one candidate goes.

Input: bench.py's `synth_hour` for seeds 0.. as audio (one file per entry of --minutes), the turns it draws as the
reference (`bench_turns` of tools/time_annotation_metrics.py), bench.py's synthetic checkpoints in the community-1 layout
(`clustering: VBxClustering`, `plda: $model/plda`) with oracle.vbx.synth_plda as the PLDA.  Candidates: --grid thresholds
over the upper quantiles of the files' own merge heights x --grid values of Fa x --grid values of Fb.

  (a) the literal loop with `training` off: `pipeline.instantiate(params)`, `pipeline(file)` for every file, a fresh
      metric -- both networks run again for every candidate; the first --literal candidates, scaled to the grid;
  (b) `ClusteringTuner.evaluate` with `batch_vbx` off: every candidate through the pipeline's own call on cached front
      ends, which is what the tuner did with a VBxClustering pipeline before it had a VBx route;
  (c) `ClusteringTuner.sweep_vbx`: per file one linkage, one PLDA projection, one cut call, the VB inferences of all
      candidates in batched launches, the assignment on the device.
(b) and (c) are timed as wholes by the host clock, --repeats times, alternating; `prepare` (the front ends, once) apart.
All legs must give the same losses.

Then, on one file of --hour minutes and one candidate: the phases of (b) -- filter, linkage, cut, PLDA projection, VB
loop, centroids and similarities, host assignment, back end, metric -- each by the host clock around a synchronised
call, --repeats times; `pa_vbx_run_batch` with 64 jobs (4 cuts x 16 (Fa, Fb)) against 64 sequential `_vbx` calls, and
`pa_constrained_assign` on that file's chunks against the host `constrained_argmax`, by the host clock and, for the two
entry points, by device events (the library's profiler).

Writes profiles/vbx_tuning_timing.txt (or --out)."""
import argparse
import os
import shutil
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
sys.path.insert(0, os.path.join(ROOT, "tests"))        # conftest.write_pipeline_dir, as bench.py takes it

FAS = (0.03, 0.07, 0.2, 0.4)
FBS = (0.2, 0.8, 3.0, 12.0)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def ms(values) -> str:
    return f"median {statistics.median(values) * 1e3:10.3f} ms   [{min(values) * 1e3:.3f}, {max(values) * 1e3:.3f}]"


def seconds(values) -> str:
    return f"median {statistics.median(values):8.3f} s   [{min(values):.3f}, {max(values):.3f}]"


def vbx_pipeline(device):
    import pyannote_audio_amd as pa
    from bench import build_checkpoints
    from conftest import write_pipeline_dir
    from oracle.vbx import synth_plda
    workdir = tempfile.mkdtemp(prefix="vbx_tuning_timing_")
    seg_o, emb_o = build_checkpoints(workdir)
    write_pipeline_dir(workdir, seg_o, emb_o, config_extra={
        "pipeline": {"name": "pyannote.audio.pipelines.SpeakerDiarization",
                     "params": {"clustering": "VBxClustering", "embedding": "$model/embedding",
                                "embedding_batch_size": 32, "embedding_exclude_overlap": True,
                                "plda": "$model/plda", "segmentation": "$model/segmentation",
                                "segmentation_batch_size": 32}},
        "params": {"clustering": {"threshold": 0.6, "Fa": 0.07, "Fb": 0.8},
                   "segmentation": {"min_duration_off": 0.0}}})
    shutil.copytree(synth_plda(tempfile.mkdtemp(prefix="plda_")), os.path.join(workdir, "plda"))
    pipeline = pa.Pipeline.from_pretrained(workdir).to(device)
    assert isinstance(pipeline.clustering, pa.VBxClustering)
    return pipeline


def literal(pipeline, files, candidates):
    losses, taken = [], []
    for params in candidates:
        def one():
            pipeline.instantiate(params)
            metric = pipeline.get_metric()
            for file in files:
                metric(file["annotation"], pipeline(file).speaker_diarization, uem=file["annotated"])
            return abs(metric)
        dt, loss = clock(one)
        losses.append(loss)
        taken.append(dt)
    return losses, taken


def events(fn, kernel: str) -> float:
    import pyannote_audio_amd.ffi as ffi
    ffi.prof_enable(True)
    ffi.prof_report()
    fn()
    torch.cuda.synchronize()
    report = ffi.prof_report()
    ffi.prof_enable(False)
    return report[kernel]["ms"]


def phases(pipeline, file, params, levels, repeats: int) -> list:
    """one file, one candidate through the pieces of `pipeline(file)` with `training` on, each piece timed on its own"""
    from scipy.cluster.hierarchy import fcluster
    from pyannote_audio_amd.clustering import Dendrogram
    from pyannote_audio_amd.evaluation import get_diarization
    from pyannote_audio_amd.tuning import ClusteringTuner
    from dataclasses import replace
    tuner = ClusteringTuner(pipeline).prepare([file])
    item = tuner.prepared[0]
    front, clustering = item.front, pipeline.clustering
    num, lo, hi = item.bounds
    train, unit, Z, fea = clustering.before_cut(front.embeddings, front.segmentations, num_clean_frames=front.clean)
    thresholds = [float(t) for t in np.quantile(Z[:, 2], levels)]
    params = {**params, "clustering": {**params["clustering"], "threshold": thresholds[len(thresholds) // 2]}}
    pipeline.instantiate(params)
    names = ("filter_embeddings", "linkage (unit vectors, pa_linkage_centroid)", "cut (SciPy fcluster)",
             "PLDA projection", "VB loop (_vbx)", "centroids + similarities", "host assignment (constrained_argmax)",
             "back end", "metric")
    taken = {name: [] for name in names}
    whole = []
    hook = pipeline.setup_hook(item.file, None)
    for _ in range(repeats + 1):
        marks = []

        def step(fn):
            dt, out = clock(fn)
            marks.append(dt)
            return out
        kept, _, _ = step(lambda: clustering.filter_embeddings(front.embeddings, segmentations=front.segmentations,
                                                               num_clean_frames=front.clean))
        tree, vectors = step(lambda: clustering._unit_linkage(kept))
        labels = step(lambda: np.unique(fcluster(tree, clustering.threshold, criterion="distance") - 1,
                                        return_inverse=True)[1])
        features = step(lambda: clustering.plda.transform_device(kept, clustering.device))
        q, priors = step(lambda: clustering._vbx(features, labels))

        def soft_scores():
            W = q[:, priors > clustering.prune_below]
            centroids = W.T @ kept / W.sum(axis=0, keepdims=True).T
            soft = clustering._similarities(front.embeddings, centroids)
            silent = front.segmentations.data.sum(axis=1) == 0
            soft[silent] = soft.min() - 1.0
            return soft, silent, centroids
        soft, silent, centroids = step(soft_scores)
        hard = step(lambda: clustering.constrained_argmax(soft))
        fresh = replace(front, marks=[("start", time.perf_counter())], enqueued={})
        output = step(lambda: pipeline._back_end(fresh, hard, centroids, lo, hi, hook))
        metric = pipeline.get_metric()
        step(lambda: metric(item.file["annotation"], get_diarization(output), uem=item.file["annotated"]))
        for name, dt in zip(names, marks):
            taken[name].append(dt)
        pipeline.training = True
        try:
            whole.append(clock(lambda: pipeline(item.file))[0])
        finally:
            pipeline.training = False
    C, S, K = soft.shape
    lines = [f"phases of one candidate of (b) on one file of {len(kept)} training embeddings, {C} chunks x {S} local "
             f"speakers, {labels.max() + 1} initial clusters -> {K} speakers kept, "
             f"{clustering.timings.get('vbx_iterations')} VB iterations (host clock, each phase synchronised; "
             f"{repeats} runs after one warm-up):"]
    total = sum(statistics.median(v[1:]) for v in taken.values())
    for name in names:
        v = taken[name][1:]
        lines.append(f"  {name:<45} {ms(v)}   {100 * statistics.median(v) / total:5.1f} %")
    lines.append(f"  {'sum of the medians':<45} {total * 1e3:17.3f} ms;  `pipeline(file)` on the cached front end as a whole: "
                 f"{ms(whole[1:])}")

    # ---- the two entry points on this file
    jobs_levels = np.linspace(levels[0], levels[-1], 4)
    rows = Dendrogram(Z).cuts([float(t) for t in np.quantile(Z[:, 2], jobs_levels)])
    rows = [np.unique(row, return_inverse=True)[1] for row in rows]
    inits = [clustering.initial_responsibilities(row) for row in rows]
    jobs = [(i, Fa, Fb) for i in range(4) for Fa in FAS for Fb in FBS]
    clustering.vbx_batch(fea, inits, jobs[:2])                                      # warm-up
    batch, sequential = [], []
    for _ in range(repeats):
        dt, results = clock(lambda: clustering.vbx_batch(fea, inits, jobs))
        batch.append(dt)

        def one_by_one():
            out = []
            for i, Fa, Fb in jobs:
                clustering.instantiate({"threshold": 0.6, "Fa": Fa, "Fb": Fb})
                out.append((clustering._vbx(fea, rows[i])[0], clustering.timings["vbx_iterations"]))
            return out
        dt, loop = clock(one_by_one)
        sequential.append(dt)
    same_vb = all(np.array_equal(a[0], b[0]) and len(a[1]) == b[1] for a, b in zip(results, loop))
    kernel_batch = events(lambda: clustering.vbx_batch(fea, inits, jobs), "k_vbx_run_batch")
    iterations = [b[1] for b in loop]
    pipeline.instantiate(params)
    device_assign, host_assign = [], []
    clustering.constrained_argmax_device(soft, silent)
    for _ in range(repeats):
        dt, got = clock(lambda: clustering.constrained_argmax_device(soft, silent))
        device_assign.append(dt)
        dt, want = clock(lambda: clustering.constrained_argmax(soft))
        host_assign.append(dt)
    same_assign = bool(np.array_equal(got, np.where(silent, -2, want)))
    kernel_assign = events(lambda: clustering.constrained_argmax_device(soft, silent), "k_constrained_assign")
    lines += [
        "",
        f"64 VB inferences on that file (4 cuts with {', '.join(str(q0.shape[1]) for q0 in inits)} clusters x 16 (Fa, Fb); "
        f"{min(iterations)}..{max(iterations)} iterations, {sum(iterations)} in all), responsibilities back on the host:",
        f"  pa_vbx_run_batch, one call            {ms(batch)}   launches (device events) {kernel_batch:.3f} ms",
        f"  64 sequential _vbx calls              {ms(sequential)}",
        f"  same responsibilities and iteration counts: {same_vb};  ratio of the medians "
        f"{statistics.median(sequential) / statistics.median(batch):.1f}",
        f"constrained assignment of {C} chunks x {S} local speakers to {K} clusters, host array in, host array out:",
        f"  constrained_argmax_device             {ms(device_assign)}   kernel (device events) {kernel_assign:.3f} ms; "
        f"{clustering.last_flagged_chunks} chunks solved on the host",
        f"  constrained_argmax (SciPy per chunk)  {ms(host_assign)}",
        f"  same assignment: {same_assign};  ratio of the medians "
        f"{statistics.median(host_assign) / statistics.median(device_assign):.1f}",
    ]
    return lines, same_vb and same_assign


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, nargs="+", default=[10.0, 20.0, 30.0])
    ap.add_argument("--hour", type=float, default=60.0)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--literal", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vbx_tuning_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd.tuning import ClusteringTuner
    from time_clustering_tuning import corpus
    ffi.require_gpu()
    device = torch.device("cuda:0")
    pipeline = vbx_pipeline(device)
    files = corpus(args.minutes, device)
    levels = np.linspace(0.97, 0.999, args.grid)

    t_prepare, tuner = clock(lambda: ClusteringTuner(pipeline).prepare(files))
    plans = [tuner._vbx_front(item) for item in tuner.prepared]
    heights = np.concatenate([plan.tree.Z[:, 2] for plan in plans])
    thresholds = [float(t) for t in np.quantile(heights, levels)]
    Fas, Fbs = FAS[:args.grid], FBS[:args.grid]
    tuner.sweep_vbx(thresholds[:1], Fas[:1], Fbs[:2])                         # warm-up of both routes
    tuner.batch_vbx = False
    tuner.sweep_vbx(thresholds[:1], Fas[:1], Fbs[:2])
    generic, batched, results = [], [], {}
    for _ in range(args.repeats):
        for route, into in ((False, generic), (True, batched)):
            tuner.batch_vbx = route
            dt, results[route] = clock(lambda: tuner.sweep_vbx(thresholds, Fas, Fbs))
            into.append(dt)
            print(f"sweep, batched {route}: {dt:.3f} s", flush=True)
    shared = dict(tuner.vbx_shared)
    result = results[True]
    candidates = [e["params"] for e in result["entries"]]
    losses_c = [e["loss"] for e in result["entries"]]
    losses_b = [e["loss"] for e in results[False]["entries"]]
    kept = sorted({k for row in tuner.train_clusters for k in row if k is not None})

    bare = [{k: v for k, v in f.items() if not k.startswith("training_cache/")} for f in files]
    literal(pipeline, bare, candidates[:1])                                   # warm-up
    losses_a, seconds_a = literal(pipeline, bare, candidates[:args.literal])
    scale = len(candidates) / len(seconds_a)
    same_losses = losses_b == losses_c and losses_a == losses_c[:len(losses_a)]
    apart = min(generic) > max(batched)

    print(f"literal loop: {seconds_a}", flush=True)
    hour_file = corpus([args.hour], device)[0]
    phase_lines, same_parts = phases(pipeline, hour_file, candidates[0], levels, args.repeats)

    train = [plan.train.shape[0] for plan in plans]
    lines = [
        f"tools/time_vbx_tuning.py --minutes {' '.join(f'{m:g}' for m in args.minutes)} --hour {args.hour:g} --grid "
        f"{args.grid} --literal {args.literal} --repeats {args.repeats}",
        f"device: {torch.cuda.get_device_name(0)}",
        f"input: {len(files)} synthetic files of {', '.join(f'{m:g}' for m in args.minutes)} min (bench.py synth_hour "
        f"seeds 0..{len(files) - 1}, their drawn turns as the reference), {sum(train)} training embeddings "
        f"({', '.join(map(str, train))}); synthetic PLDA (oracle.vbx.synth_plda); {len(candidates)} candidates = "
        f"{len(thresholds)} thresholds over the quantiles {levels[0]:g}..{levels[-1]:g} of the files' merge heights "
        f"({thresholds[0]:.4f}..{thresholds[-1]:.4f}) x Fa {list(Fas)} x Fb {list(Fbs)}; metric: the pipeline's own "
        "(GreedyDiarizationErrorRate on the device)",
        f"speakers VBx kept over files and candidates: {kept[0]}..{kept[-1]} ({len(kept)} different counts)",
        "",
        f"(a) literal loop, training off: {sum(seconds_a):8.3f} s for {len(seconds_a)} candidates, per candidate "
        f"{seconds(seconds_a)}; scaled to {len(candidates)} candidates: {sum(seconds_a) * scale:.3f} s",
        f"(b) ClusteringTuner, every candidate through the pipeline's call on cached front ends: whole sweep "
        f"{seconds(generic)}  ({args.repeats} sweeps, alternating with (c))",
        f"(c) ClusteringTuner.sweep_vbx, batched: whole sweep {seconds(batched)}",
        f"    prepare (front ends of all files, once; in neither sweep time): {t_prepare:.3f} s;  of {shared['candidates']} "
        f"(candidate, file) pairs: {shared['initialisations']} initialisations, {shared['jobs']} VB inferences in "
        f"{shared['calls']} pa_vbx_run_batch calls; evaluations that shared an earlier back end and metric: "
        f"{result['shared_evaluations']} of {result['evaluations']} in (c), {results[False]['shared_evaluations']} in (b)",
        f"same losses in (a), (b) and (c): {same_losses};  best: {result['best']['params']['clustering']}, loss "
        f"{result['best']['loss']:.6f}",
        "",
        f"(b) / (c) = {statistics.median(generic) / statistics.median(batched):.2f} (medians);  (a) / (c) = "
        f"{sum(seconds_a) * scale / statistics.median(batched):.1f};  the ranges of (b) and (c) do not overlap and (c) is "
        f"the faster: {apart}" + ("" if apart else "   <-- they DO overlap, or (c) is not faster"),
        "",
    ] + phase_lines
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(text)
    assert same_losses and same_parts, "the legs disagree"


if __name__ == "__main__":
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        main()
