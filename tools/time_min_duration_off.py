"""Time the search for `min_duration_off` on 16 synthetic hours (GPU), two ways.

Input: `bench_turns` of tools/time_annotation_metrics.py (bench.py's `synth_hour` draws) for seeds 0..15 as the
references; every hypothesis is its reference with starts and ends jittered by up to 0.2 s, as there, and then every
turn split in two by a gap of 0.05 to 0.3 s, so that filling gaps changes the error rate.

  (a) the literal loop of the reference's MinDurationOffOptimizer: `hypothesis.support(candidate)` on the host and
      the per-file `DiarizationErrorRate(device=cuda)` call, file by file, for every candidate;
  (b) `evaluation.MinDurationOffOptimizer` with the same metric: `evaluation.Corpus` lists and uploads the turns
      once, then one `pa_annot_corpus_counts` call and one download per candidate.

Both searches run once in full (the same scipy bounded minimisation, so the same candidates as long as the values
agree) and must return the same best value and the same reports.  Every objective evaluation is timed by the host
clock (each ends with its results on the host, which synchronises).  The spread is taken from `--repeats` further
evaluations of each way at the best value found, alternating (a) and (b).  The device share is taken in one more
evaluation of each way with the library's event profiler on (HIP events around the launches of `pa_annot_counts` /
`pa_annot_corpus_counts`): device call = that sum, host = the evaluation's host-clock time minus it.

Writes profiles/min_duration_off_timing.txt (or --out)."""
import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def corpus(files: int, hours: float) -> list:
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.core import Segment
    from pyannote_audio_amd.metrics import Timeline
    from time_annotation_metrics import bench_turns
    out = []
    for seed in range(files):
        turns = bench_turns(hours, seed=seed)
        rng = np.random.default_rng(1000 + seed)
        starts, ends = np.array([t[0] for t in turns]), np.array([t[1] for t in turns])
        speakers = [t[2] for t in turns]
        uri = f"hour{seed:02d}"
        reference = pa.Annotation.from_columns(starts, ends, list(range(len(turns))), [f"spk{s}" for s in speakers],
                                               uri=uri)
        jitter = rng.uniform(-0.2, 0.2, (2, len(turns)))
        a = np.maximum(starts + jitter[0], 0.0)
        b = np.maximum(ends + jitter[1], a + 0.5)
        gap = rng.uniform(0.05, 0.3, len(turns))
        middle = 0.5 * (a + b)
        labels = [(s + 1) % 3 for s in speakers]
        hypothesis = pa.Annotation.from_columns(np.concatenate([a, middle + 0.5 * gap]),
                                                np.concatenate([middle - 0.5 * gap, b]),
                                                list(range(2 * len(turns))), labels + labels, uri=uri)
        out.append({"uri": uri, "annotation": reference, "speaker_diarization": hypothesis,
                    "annotated": Timeline([Segment(0.0, hours * 3600.0)])})
    return out


class Timed:
    """an objective with the host-clock time of every evaluation"""

    def __init__(self, objective):
        self.objective, self.seconds, self.candidates = objective, [], []

    def __call__(self, candidate):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        value = self.objective(candidate)
        torch.cuda.synchronize()
        self.seconds.append(time.perf_counter() - t0)
        self.candidates.append(float(candidate))
        return value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "min_duration_off_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from scipy.optimize import minimize_scalar

    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd import annotation_metrics as am
    from pyannote_audio_amd import evaluation
    ffi.require_gpu()
    device = torch.device("cuda:0")
    files = corpus(args.files, args.hours)
    rows = sum(len(f["speaker_diarization"].flat_rows()) for f in files)

    # (a) the literal loop
    metric_a = am.DiarizationErrorRate(device=device)
    reports_a, values_a = {}, {}

    def literal(candidate):
        candidate = float(candidate)
        metric_a.reset()
        for file in files:
            metric_a(file["annotation"], file["speaker_diarization"].support(candidate), uem=file["annotated"])
        reports_a[candidate] = metric_a.report()
        values_a[candidate] = abs(metric_a)
        return values_a[candidate]

    def search(objective):
        without = objective(0.0)
        found = minimize_scalar(objective, bounds=(0.0, 1.0), method="Bounded")
        return 0.0 if without == min(values_a.values()) else float(found.x)

    # (b) the corpus path: the optimizer itself, its objective wrapped for timing
    metric_b = am.DiarizationErrorRate(device=device)
    optimizer = evaluation.MinDurationOffOptimizer()
    timed_b = Timed(None)
    inner = optimizer._compute_metric

    def wrapped(files_, metric_, corpus_, candidate):
        timed_b.objective = lambda c: inner(files_, metric_, corpus_, c)
        return timed_b(candidate)

    optimizer._compute_metric = wrapped
    literal(0.0)                                     # warm-up: code objects, allocator
    evaluation.Corpus(files, device=device).counts(0.0)

    t0 = time.perf_counter()
    best_b, report_b = optimizer(files, metric_b)
    total_b = time.perf_counter() - t0
    timed_a = Timed(literal)
    t0 = time.perf_counter()
    best_a = search(timed_a)
    total_a = time.perf_counter() - t0
    same_candidates = timed_a.candidates == timed_b.candidates
    same_best = best_a == best_b
    same_reports = same_candidates and all(reports_a[c] == optimizer._reports[c] for c in timed_a.candidates)

    # spread: further evaluations at the best value, alternating
    t0 = time.perf_counter()
    shared = evaluation.Corpus(files, device=device)
    build_b = time.perf_counter() - t0

    def corpus_evaluation(candidate):
        return inner(files, metric_b, shared, candidate)

    again_a, again_b = Timed(literal), Timed(corpus_evaluation)
    for _ in range(args.repeats):
        again_a(best_a)
        again_b(best_a)

    # device share: one evaluation each with the event profiler on
    def device_ms(objective, kernel):
        ffi.prof_enable(True)
        ffi.prof_report()
        timed = Timed(objective)
        timed(best_a)
        report = ffi.prof_report()
        ffi.prof_enable(False)
        return report[kernel]["ms"], report[kernel]["launches"], timed.seconds[0] * 1e3

    dev_a, calls_a, wall_a = device_ms(literal, "k_annot_counts")
    dev_b, calls_b, wall_b = device_ms(corpus_evaluation, "k_annot_corpus_counts")

    def ms(values):
        return f"median {statistics.median(values) * 1e3:10.3f} ms   [{min(values) * 1e3:.3f}, {max(values) * 1e3:.3f}]"

    med_a, med_b = statistics.median(again_a.seconds), statistics.median(again_b.seconds)
    spread_a = max(again_a.seconds) - min(again_a.seconds)
    faster = med_a - med_b > spread_a
    lines = [
        f"tools/time_min_duration_off.py --files {args.files} --hours {args.hours:g} --repeats {args.repeats}",
        f"device: {torch.cuda.get_device_name(0)}",
        f"input: {args.files} files of {args.hours:g} h (bench.py synth_hour seeds 0..{args.files - 1}), {rows} hypothesis "
        f"turns in all (every jittered turn split by a gap of 0.05..0.3 s), 3 speakers, 1 uem region per file",
        "metric: annotation_metrics.DiarizationErrorRate(device=cuda); scipy minimize_scalar(method='Bounded'), "
        "bounds (0, 1), after an evaluation at 0",
        "",
        f"(a) literal loop : {len(timed_a.seconds)} objective evaluations, {total_a:.3f} s in all; per evaluation "
        f"{ms(timed_a.seconds)}",
        f"(b) corpus path  : {len(timed_b.seconds)} objective evaluations, {total_b:.3f} s in all (listing and "
        "uploading the corpus once and support(best) of every file at the end included; building the corpus alone: "
        f"{build_b:.3f} s); per evaluation {ms(timed_b.seconds)}",
        f"same candidates: {same_candidates}; same best value: {same_best} ({best_a!r} / {best_b!r}); same reports at "
        f"every candidate: {same_reports}",
        f"error rate at 0: {optimizer._reports[0.0]['TOTAL']['diarization error rate']:.6f}; at the best value: "
        f"{report_b['TOTAL']['diarization error rate']:.6f}",
        "",
        f"{args.repeats} further evaluations each at the best value, alternating (host clock, results on the host):",
        f"(a) {ms(again_a.seconds)}   spread (max - min) {spread_a * 1e3:.3f} ms",
        f"(b) {ms(again_b.seconds)}",
        f"one evaluation with the event profiler on: (a) {calls_a} pa_annot_counts calls, device {dev_a:.3f} ms, host "
        f"{wall_a - dev_a:.3f} ms; (b) {calls_b} pa_annot_corpus_counts call, device {dev_b:.3f} ms, host "
        f"{wall_b - dev_b:.3f} ms",
        "",
        f"(a) / (b) per evaluation = {med_a / med_b:.1f}; whole search (a) / (b) = {total_a / total_b:.1f}",
        f"(b) is faster than (a) by more than the spread of (a): {faster}"
        + ("" if faster else "   <-- the corpus path is NOT faster here"),
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(text)
    assert same_best and same_reports, "the two ways disagree"


if __name__ == "__main__":
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        main()
