"""Time the speaker mapping and a full time-based error rate on one synthetic hour (GPU).

Input: the turns of the benchmark's conversation (bench.py `synth_hour`: the same seeded draws, without
synthesising the waveform) as the reference, a jittered copy with anonymous speaker ids as the hypothesis.  Timed,
after warm-up, as the median of `--calls` calls, the three alternating round by round, host clock around calls that
end with their result on the host (so every device call ends in a copy back, which synchronises):

  * `diarization.optimal_mapping` as it was before `annotation_metrics` (the pair loop, kept here as the baseline),
  * `diarization.optimal_mapping` now, counting on the device,
  * one `GreedyDiarizationErrorRate(collar=0.25)` call on the device.

The two mappings are compared before anything is timed.  Writes profiles/annotation_metrics_timing.txt (or --out)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_turns(hours: float, seed: int) -> list:
    """(start, end, speaker) of bench.py's `synth_hour`: the same draws in the same order"""
    sr, S = 16000, 3
    n = int(hours * 3600 * sr)
    rng = np.random.default_rng(seed)
    turns = []

    def add(s, a, b):
        a, b = max(0, a), min(n, b)
        if b - a >= 200:
            turns.append((a / sr, b / sr, s))

    pos, dur = 0.0, n / sr
    while pos < dur:
        pos += rng.uniform(0.1, 1.2)
        s = int(rng.integers(S))
        d = rng.uniform(0.8, 4.0)
        a, b = int(pos * sr), int((pos + d) * sr)
        if a >= n:
            break
        add(s, a, b)
        if rng.uniform() < 0.25:
            s2 = (s + 1 + int(rng.integers(S - 1))) % S
            a2 = a + (b - a) // 2
            b2 = b + int(rng.uniform(0.3, 1.5) * sr)
            add(s2, a2, b2)
            pos = min(b2, n) / sr
        else:
            pos = min(b, n) / sr
    return turns


def pair_loop_mapping(reference, hypothesis):
    """`diarization.cooccurrence` + `optimal_mapping` as they were before this module existed"""
    from scipy.optimize import linear_sum_assignment
    a, b = hypothesis, reference
    la, lb = a.labels(), b.labels()
    ia, ib = {l: i for i, l in enumerate(la)}, {l: j for j, l in enumerate(lb)}
    tb = [(s.start, s.end, ib[l]) for s, _, l in b.itertracks(yield_label=True)]
    together = np.zeros((len(la), len(lb)))
    for s, _, l in a.itertracks(yield_label=True):
        for start, end, j in tb:
            lo, hi = max(s.start, start), min(s.end, end)
            if hi > lo:
                together[ia[l], j] += hi - lo
    mapping = {}
    for i, j in zip(*linear_sum_assignment(-together)):
        if together[i, j] > 0:
            mapping[la[i]] = lb[j]
    return mapping


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "annotation_metrics_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import pyannote_audio_amd as pa
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd import annotation_metrics as am
    from pyannote_audio_amd import diarization
    from pyannote_audio_amd.core import Segment
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
    uem = [Segment(0.0, args.hours * 3600.0)]
    metric = am.GreedyDiarizationErrorRate(collar=0.25, device=device)

    def before():
        return pair_loop_mapping(reference, hypothesis)

    def after():
        return diarization.optimal_mapping(reference, hypothesis, return_mapping=True, device=device)[1]

    def after_host():
        return diarization.optimal_mapping(reference, hypothesis, return_mapping=True)[1]

    def error_rate():
        return metric(reference, hypothesis, uem=uem, detailed=True)

    assert before() == after() == after_host() == {1: "spk0", 2: "spk1", 0: "spk2"}
    on_device, on_host = error_rate(), am.GreedyDiarizationErrorRate(collar=0.25)(reference, hypothesis, uem=uem,
                                                                                    detailed=True)
    for name, value in on_host.items():
        assert abs(on_device[name] - value) <= 1e-9 * max(1.0, abs(value)), (name, on_device[name], value)

    candidates = {"optimal_mapping, pair loop (before)": before, "optimal_mapping, device (now)": after,
                  "optimal_mapping, host sweep (now, no GPU)": after_host,
                  "GreedyDiarizationErrorRate(collar=0.25), device": error_rate}
    times = {name: [] for name in candidates}
    for name, fn in candidates.items():
        for _ in range(1 if fn is before else args.warmup):
            fn()
    for _ in range(args.calls):
        for name, fn in candidates.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)

    # the four launches alone, by device events
    _, ref_seg, ref_lab = am._rows(reference)
    _, hyp_seg, hyp_lab = am._rows(hypothesis)
    uem_seg = np.array([[0.0, args.hours * 3600.0]])
    kernel_ms = []
    for _ in range(args.warmup + args.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        # (the upload and the allocations of `device_counts` are inside the events: that is the call a user makes)
        e0.record()
        am.device_counts(ref_seg, ref_lab, 3, hyp_seg, hyp_lab, 3, uem_seg, 0.25, False, device)
        e1.record()
        e1.synchronize()
        kernel_ms.append(e0.elapsed_time(e1))
    kernel_ms = kernel_ms[args.warmup:]

    cuts = 2 * (2 * len(turns) + 1) + 4 * len(turns)
    lines = [f"tools/time_annotation_metrics.py --hours {args.hours:g} --calls {args.calls} --warmup {args.warmup}",
             f"device: {torch.cuda.get_device_name(0)}",
             f"input: {len(turns)} reference turns (3 speakers, bench.py synth_hour seed 0), {len(turns)} hypothesis "
             f"turns (starts and ends jittered by up to 0.2 s), 1 uem region; {cuts} cuts with a collar",
             f"host clock, median [min, max] of {args.calls} calls, alternating; results on the host at the end",
             ""]
    for name, values in times.items():
        lines.append(f"{name:52s} {statistics.median(values) * 1e3:10.3f} ms   [{min(values) * 1e3:.3f}, "
                     f"{max(values) * 1e3:.3f}]")
    base = statistics.median(times["optimal_mapping, pair loop (before)"])
    now = statistics.median(times["optimal_mapping, device (now)"])
    lines += ["", f"optimal_mapping: before / now = {base / now:.1f}",
              f"device_counts alone (upload + 4 launches, device events, collar 0.25): median "
              f"{statistics.median(kernel_ms):.3f} ms [{min(kernel_ms):.3f}, {max(kernel_ms):.3f}]",
              f"DER on the device: " + ", ".join(f"{k} = {v:.6f}" for k, v in on_device.items())]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(text)
    assert now <= base, "the new optimal_mapping is slower than the pair loop"


if __name__ == "__main__":
    main()
