"""Time the batched assignment solver (`pa_lsap_batch`, csrc/lsap.hip) and the three routes it takes off the host (GPU).

  * Sliding DER: the synthetic hour of tools/time_sliding_der.py (719 windows of 10 s).  `window_error_rates` on the
    device at this commit (counts, the W mappings and W x 5 numbers back) against the route of the commit before it
    (counts on the device, all counts back, SciPy per window: `window_rates_from_counts(window_counts(device=cuda))`,
    unchanged in the code) and against the numpy form.
  * Frame-level DER: `diarization_error_rate` at B = 32, S = 8, F = 589 with `permutate_batch` against the route of the
    commit before it (both arrays to the host, `permutate` in a loop, the permutation uploaded).
  * The kernel alone, by device events: 719 problems of 4 x 4, 3 000 of 8 x 8 and 256 of 64 x 64 (continuous costs, and
    integer costs 0..2 full of ties), each against the SciPy loop on the same host (host clock).

Median of `--runs` runs [min, max], the legs alternating round by round, after `--warmup` rounds; the results of the
legs are compared with `==` before anything is timed.  Writes profiles/lsap_timing.txt (or --out)."""
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


def alternate(candidates: dict, runs: int, warmup: int) -> dict:
    """host clock around calls that end with their result on the host -> {name: [seconds]}"""
    times = {name: [] for name in candidates}
    for n in range(warmup + runs):
        for name, fn in candidates.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if n >= warmup:
                times[name].append(time.perf_counter() - t0)
    return times


def line(name, values, scale=1e3):
    return f"{name:64s} {statistics.median(values) * scale:10.3f} ms   [{min(values) * scale:.3f}, " \
           f"{max(values) * scale:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsap_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import pyannote_audio_amd as pa
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd import annotation_metrics as am
    from pyannote_audio_amd import metrics, permutation
    from pyannote_audio_amd.core import Segment, SlidingWindow
    from pyannote_audio_amd.distance import linear_sum_assignment_batch
    from pyannote_audio_amd.metrics import Timeline
    from scipy.optimize import linear_sum_assignment
    from time_annotation_metrics import bench_turns
    ffi.require_gpu()
    device = torch.device("cuda:0")
    lines = [f"tools/time_lsap.py --runs {args.runs} --warmup {args.warmup}",
             f"device: {torch.cuda.get_device_name(0)}; {os.cpu_count()} host CPUs, torch threads "
             f"{torch.get_num_threads()}",
             f"median [min, max] of {args.runs} runs, the legs alternating round by round", ""]

    # ---------------------------------------------------------------------------------------------- sliding DER
    turns = bench_turns(1.0, seed=0)
    rng = np.random.default_rng(1)
    starts, ends = np.array([t[0] for t in turns]), np.array([t[1] for t in turns])
    speakers = [t[2] for t in turns]
    reference = pa.Annotation.from_columns(starts, ends, list(range(len(turns))), [f"spk{s}" for s in speakers],
                                           uri="hour")
    jitter = rng.uniform(-0.2, 0.2, (2, len(turns)))
    hyp_starts = np.maximum(starts + jitter[0], 0.0)
    hypothesis = pa.Annotation.from_columns(hyp_starts, np.maximum(ends + jitter[1], hyp_starts + 0.05),
                                            list(range(len(turns))), [(s + 1) % 3 for s in speakers], uri="hour")
    uem = Timeline([Segment(0.0, 3600.0)])
    chunks = list(SlidingWindow(duration=10.0, step=5.0)(uem))
    sliding = {
        "window_error_rates(device=cuda): mappings on the device":
            lambda: am.window_error_rates(reference, hypothesis, chunks, uem=uem, device=device),
        "the commit before: counts on the device, SciPy per window":
            lambda: am.window_rates_from_counts(am.window_counts(reference, hypothesis, chunks, uem=uem, device=device)),
        "numpy counts, SciPy per window":
            lambda: am.window_rates_from_counts(am.window_counts(reference, hypothesis, chunks, uem=uem, device=None)),
    }
    tables = [fn() for fn in sliding.values()]
    for key in tables[0]:       # the two device routes share their counts: `==`; the numpy sweep adds other pieces
        assert tables[0][key].tolist() == tables[1][key].tolist(), key
        assert np.allclose(tables[0][key], tables[2][key], rtol=1e-9, atol=1e-9), key
    lines += [f"sliding DER: one synthetic hour, {len(turns)} turns a side, {len(chunks)} windows of 10 s; host clock, "
              f"the table on the host at the end"]
    lines += [line("  " + name, values) for name, values in alternate(sliding, args.runs, args.warmup).items()]

    # ------------------------------------------------------------------------------------------ frame-level DER
    B, S, F = 32, 8, 589
    rng = np.random.default_rng(2)
    change = rng.random((B, S, F)) < 0.01
    target = ((np.cumsum(change, axis=2) + rng.integers(0, 2, (B, S, 1))) % 2).astype(np.uint8)
    target[:, 5:] = 0                                                   # silent speakers: the usual case
    on = np.where(rng.random(target.shape) < 0.15, 1 - target, target)
    preds = np.where(on == 1, rng.uniform(0.4, 1.0, target.shape), rng.uniform(0.0, 0.6, target.shape))
    preds = np.take_along_axis(preds, np.argsort(rng.random((B, S)), axis=1)[:, :, None], axis=1).astype(np.float32)
    d_preds, d_target = torch.from_numpy(preds).to(device), torch.from_numpy(target).to(device)
    thresholds = torch.linspace(0.0, 1.0, 51)

    def before(y1, y2):
        _, found = permutation.permutate(y1, y2)
        return None, torch.tensor([[-1 if j is None else j for j in row] for row in found],
                                  dtype=torch.int32).to(y1.device)

    def der(route):
        saved, metrics.permutate_batch = metrics.permutate_batch, route
        try:
            value, parts = metrics.diarization_error_rate(d_preds, d_target, threshold=thresholds,
                                                          return_components=True)
            return [value.cpu()] + [p.cpu() for p in parts]
        finally:
            metrics.permutate_batch = saved

    frame = {"diarization_error_rate: permutate_batch on the device": lambda: der(permutation.permutate_batch),
             "the commit before: download, permutate on the host, upload": lambda: der(before)}
    first, second = [fn() for fn in frame.values()]
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    lines += ["", f"frame-level DER: B = {B}, S = {S}, F = {F}, 51 thresholds; host clock, the rates on the host at "
                  f"the end"]
    lines += [line("  " + name, values) for name, values in alternate(frame, args.runs, args.warmup).items()]

    # ------------------------------------------------------------------------------------------ the kernel alone
    lines += ["", "pa_lsap_batch alone (device events around linear_sum_assignment_batch(check=False), costs on the "
                  "device) against the SciPy loop (host clock, costs on the host)"]
    for count, size in ((719, 4), (3000, 8), (256, 64)):
        for kind in ("continuous", "integers 0..2"):
            rng = np.random.default_rng(size)
            cost = rng.standard_normal((count, size, size)) if kind == "continuous" else \
                rng.integers(0, 3, (count, size, size)).astype(np.float64)
            d_cost = torch.from_numpy(cost).to(device)
            want = np.stack([linear_sum_assignment(m)[1] for m in cost])
            got, status = linear_sum_assignment_batch(d_cost, check=False)
            assert np.array_equal(got.cpu().numpy(), want) and not status.any()
            kernel, host = [], []
            for n in range(args.warmup + args.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                linear_sum_assignment_batch(d_cost, check=False)
                e1.record()
                e1.synchronize()
                t0 = time.perf_counter()
                for m in cost:
                    linear_sum_assignment(m)
                t1 = time.perf_counter()
                if n >= args.warmup:
                    kernel.append(e0.elapsed_time(e1) * 1e-3)
                    host.append(t1 - t0)
            lines += [line(f"  {count} x ({size} x {size}), {kind}: device", kernel),
                      line(f"  {count} x ({size} x {size}), {kind}: SciPy loop", host)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(text)


if __name__ == "__main__":
    main()
