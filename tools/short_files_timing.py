"""Wall time of `list(pipeline(files))` on one audio-hour cut into SHORT files, with and without `pack=True`
(apply_batch: the front ends of several files in shared launch groups), full 3.1 pipeline, synthetic conversations.

Workloads (one audio-hour each): 120 x 30 s, 12 x 5 min, a mix of 30 s ... 10 min, 1 x 1 h (sanity: nothing to pack).
Per workload: two warm-ups of each form, then the two forms ALTERNATING, `--runs` (5) timed runs each; the clock is a
host clock around the whole call followed by a device synchronise.  Reports the median and the range per form, the
sizes of the groups `pack=True` formed, and whether the two forms gave the same turns and centroids.

usage (GPU box):  python tools/short_files_timing.py [--runs 5] [--out FILE] [--no-pack]
`--no-pack`: time the plain call only, without passing `pack` at all (a checkout from before the option existed: the
baseline that `pack=False` must agree with)."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
import pyannote_audio_amd as pa

SR = 16000


def mixed_durations(seed: int = 0, total: float = 3600.0) -> list:
    """30 s ... 10 min, drawn until they fill the hour (the last one is what is left, joined to its predecessor when
    it is shorter than 30 s)"""
    rng = np.random.default_rng(seed)
    out, left = [], total
    while left > 0:
        d = float(rng.choice([30.0, 45.0, 60.0, 90.0, 120.0, 180.0, 300.0, 600.0]))
        d = min(d, left)
        if d < 30.0 and out:
            out[-1] += d
        else:
            out.append(d)
        left -= d
    return out


def cut(hour: torch.Tensor, durations: list, tag: str) -> list:
    files, a = [], 0
    for i, d in enumerate(durations):
        b = a + int(round(d * SR))
        files.append({"waveform": hour[:, a:b].clone(), "sample_rate": SR, "uri": f"{tag}_{i:03d}"})
        a = b
    return files


def signature(outputs) -> list:
    return [(f["uri"], [(s.start, s.end, l) for s, _, l in o.speaker_diarization.itertracks(yield_label=True)],
             o.speaker_embeddings.tobytes()) for f, o in outputs]


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
    workdir = tempfile.mkdtemp(prefix="pa_short_")
    bench.build_checkpoints(workdir)
    pipeline = pa.Pipeline.from_pretrained(workdir)
    pipeline.to(device)
    hour = bench.synth_hour(1.0, seed=0, device=device)
    workloads = [("120 x 30 s", [30.0] * 120), ("12 x 5 min", [300.0] * 12),
                 ("mix 30 s .. 10 min", mixed_durations()), ("1 x 1 h", [3600.0])]
    forms = [("plain", {})] if args.no_pack else [("pack=False", {"pack": False}), ("pack=True", {"pack": True})]
    say(f"# short_files_timing: {torch.cuda.get_device_name(0)}, {args.runs} alternating runs per form after 2 warm-ups "
        f"each; ms per call of list(pipeline(files)) over one audio-hour, host clock + device synchronise")

    def run(files, kwargs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outputs = list(pipeline([dict(f) for f in files], **kwargs))
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), outputs

    for name, durations in workloads:
        files = cut(hour, durations, name.split()[0])
        results, times = {}, {form: [] for form, _ in forms}
        for _ in range(2):
            for form, kwargs in forms:
                _, results[form] = run(files, kwargs)
        groups = [len(g) for g in getattr(pipeline, "last_pack_groups", [])]
        for _ in range(args.runs):
            for form, kwargs in forms:
                times[form].append(run(files, kwargs)[0])
        say(f"\n## {name}: {len(files)} files, {sum(durations):.0f} s of audio")
        for form, _ in forms:
            t = times[form]
            say(f"{form:>11}: median {statistics.median(t):8.1f} ms   range {min(t):8.1f} .. {max(t):8.1f}   "
                f"runs {' '.join(f'{x:.1f}' for x in t)}")
        if not args.no_pack:
            a, b = statistics.median(times["pack=False"]), statistics.median(times["pack=True"])
            same = signature(results["pack=False"]) == signature(results["pack=True"])
            say(f"  pack=True / pack=False = {b / a:.3f}   groups of pack=True (files per group): {groups}   "
                f"same turns and centroids: {same}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
