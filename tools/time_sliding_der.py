"""Time the sliding-window diarization error rate on one synthetic hour (GPU).

Input: the file of tools/time_annotation_metrics.py (the turns of the benchmark's conversation as the reference, a
jittered copy with other speaker ids as the hypothesis), one uem region, windows of `--window` seconds with a step of
half a window.  Timed, after warm-up, as the median of `--runs` runs, the legs alternating round by round, host clock
around calls that end with their result on the host:

  * the literal loop of the reference's class (crop, `DiarizationErrorRate`, accumulate), counts on the device: what a
    user can run without `window_counts`,
  * the same loop with the counts in numpy,
  * `SlidingDiarizationErrorRate()`: all windows from one numpy sweep,
  * `SlidingDiarizationErrorRate(device=cuda)`: all windows from one device call; split into the call (upload, four
    launches, download: device events) and the per-window assignment on the host (host clock).

The four totals are compared before anything is timed.  Writes profiles/sliding_der_timing.txt (or --out)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--window", type=float, default=10.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sliding_der_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import pyannote_audio_amd as pa
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd import annotation_metrics as am
    from pyannote_audio_amd.core import Segment, SlidingWindow
    from pyannote_audio_amd.metrics import Timeline
    from time_annotation_metrics import bench_turns
    ffi.require_gpu()
    device = torch.device("cuda:0")

    turns = bench_turns(args.hours, seed=0)
    rng = np.random.default_rng(1)
    starts = np.array([t[0] for t in turns])
    ends = np.array([t[1] for t in turns])
    speakers = [t[2] for t in turns]
    reference = pa.Annotation.from_columns(starts, ends, list(range(len(turns))), [f"spk{s}" for s in speakers],
                                           uri="hour")
    jitter = rng.uniform(-0.2, 0.2, (2, len(turns)))
    hyp_starts = np.maximum(starts + jitter[0], 0.0)
    hypothesis = pa.Annotation.from_columns(hyp_starts, np.maximum(ends + jitter[1], hyp_starts + 0.05),
                                            list(range(len(turns))), [(s + 1) % 3 for s in speakers], uri="hour")
    uem = Timeline([Segment(0.0, args.hours * 3600.0)])
    chunks = list(SlidingWindow(duration=args.window, step=0.5 * args.window)(uem))

    def loop(dev):
        der = am.DiarizationErrorRate(device=dev)
        for chunk in chunks:
            der(reference.crop(chunk), hypothesis.crop(chunk), uem=Timeline([chunk]))
        return der[:]

    def sliding(dev):
        return am.SlidingDiarizationErrorRate(window=args.window, device=dev).compute_components(
            reference, hypothesis, uem=uem)

    candidates = {"literal loop, counts on the device": lambda: loop(device),
                  "literal loop, counts in numpy": lambda: loop(None),
                  "SlidingDiarizationErrorRate(), numpy": lambda: sliding(None),
                  "SlidingDiarizationErrorRate(device=cuda)": lambda: sliding(device)}
    results = {name: fn() for name, fn in candidates.items()}           # (also the first warm-up)
    first = next(iter(results.values()))
    for name, components in results.items():
        for key, value in first.items():
            # (a crop rounds nothing, but the loop's cuts are not the sweep's: sums of other pieces)
            assert abs(components[key] - value) <= 1e-9 * max(1.0, abs(value)), (name, key, components[key], value)

    times = {name: [] for name in candidates}
    for _ in range(max(args.warmup - 1, 0)):
        for fn in candidates.values():
            fn()
    for _ in range(args.runs):
        for name, fn in candidates.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)

    # the device route in its two parts
    call_ms, assign_ms = [], []
    for _ in range(args.warmup + args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        counts = am.window_counts(reference, hypothesis, chunks, uem=uem, device=device)
        e1.record()
        e1.synchronize()
        call_ms.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        am.window_rates_from_counts(counts)
        assign_ms.append((time.perf_counter() - t0) * 1e3)
    call_ms, assign_ms = call_ms[args.warmup:], assign_ms[args.warmup:]

    def line(name, values, scale=1e3):
        return f"{name:52s} {statistics.median(values) * scale:10.3f} ms   [{min(values) * scale:.3f}, " \
               f"{max(values) * scale:.3f}]"

    cuts = 2 * (2 * len(turns) + 1 + len(chunks))
    total = statistics.median(times["SlidingDiarizationErrorRate(device=cuda)"]) * 1e3
    lines = [f"tools/time_sliding_der.py --hours {args.hours:g} --window {args.window:g} --runs {args.runs} "
             f"--warmup {args.warmup}",
             f"device: {torch.cuda.get_device_name(0)}",
             f"input: {len(turns)} reference turns (3 speakers, bench.py synth_hour seed 0), {len(turns)} hypothesis "
             f"turns (starts and ends jittered by up to 0.2 s), 1 uem region, {len(chunks)} windows of "
             f"{args.window:g} s; {cuts} cuts",
             f"host clock, median [min, max] of {args.runs} runs, alternating; results on the host at the end", ""]
    lines += [line(name, values) for name, values in times.items()]
    lines += ["", "the device route in parts:",
              line("  window_counts (flatten, upload, 4 launches, download; device events)", call_ms, 1.0),
              line("  window_rates_from_counts (SciPy assignment per window, host clock)", assign_ms, 1.0),
              f"  the assignment is {100.0 * statistics.median(assign_ms) / total:.0f} % of the device route's "
              f"{total:.3f} ms",
              "", "components: " + ", ".join(f"{k} = {v:.6f}" for k, v in results[
                  "SlidingDiarizationErrorRate(device=cuda)"].items())]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(text)


if __name__ == "__main__":
    main()
