"""Times the fused diarization-error kernels (csrc/metrics.hip) at the sizes the pipeline produces, beside the same
definitions written as plain torch ops on the same GPU (tests/metrics_truth.py `torch_file_counts` /
`torch_chunk_counts`):

  file mode    one audio-hour: T = 213 334 frames, 3 reference and 3 hypothesis speakers (pa_der_counts)
  chunk mode   one audio-hour of chunks: 7 176 x 3 x 589 scores at 51 thresholds (pa_der_chunks + pa_der_chunks_sum)

Device events around `reps` back-to-back calls after a warm-up of the same shapes, alternating the two formulations
round by round; the median round is reported with the fastest and the slowest.  Outputs are compared before timing.
Peak device memory of one call comes from torch's allocator statistics.

    python tools/bench_metrics.py [--out profiles/metrics_eval.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def time_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def compare(name, fused, plain, rounds, reps_fused, reps_plain, lines):
    for _ in range(3):
        fused()
        plain()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(rounds):                      # alternate: both see the same clocks and the same neighbours
        a.append(time_ms(fused, reps_fused))
        b.append(time_ms(plain, reps_plain))
    peak = []
    for fn in (fused, plain):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak.append(torch.cuda.max_memory_allocated() - before)
    for label, t, p in (("fused kernels", a, peak[0]), ("plain torch ops", b, peak[1])):
        lines.append(f"{name:<11} {label:<16} median {statistics.median(t) * 1e3:10.1f} us   min {min(t) * 1e3:10.1f}"
                     f"   max {max(t) * 1e3:10.1f}   peak memory of a call {p / 2 ** 20:10.2f} MiB")
    lines.append(f"{name:<11} plain / fused = {statistics.median(b) / statistics.median(a):.1f} x")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args(argv)
    import metrics_truth
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd import metrics
    ffi.require_gpu()
    dev = torch.device("cuda:0")
    lib = ffi.load()
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; device events, "
             f"{args.rounds} alternating rounds"]
    rng = np.random.default_rng(0)

    # ---- file mode, one audio-hour
    T, S = 213334, 3
    ref = torch.from_numpy((rng.random((T, S)) < 0.3).astype(np.uint8)).to(dev)
    hyp = torch.from_numpy((rng.random((T, S)) < 0.3).astype(np.uint8)).to(dev)
    out = torch.empty(S * S + 2 * S + 4, dtype=torch.int64, device=dev)

    def file_fused():
        ffi.check(lib.pa_der_counts(ffi.ptr(ref), ffi.ptr(hyp), None, T, S, S, ffi.ptr(out), ffi.stream()))

    def file_plain():
        return metrics_truth.torch_file_counts(ref, hyp)

    file_fused()
    cooc, total, fa, miss, both = file_plain()
    want = torch.cat([cooc.reshape(-1), ref.sum(0), hyp.sum(0), torch.stack([total, fa, miss, both])])
    assert torch.equal(out, want), "file mode: fused and plain counts differ"
    lines.append(f"file mode: T = {T}, {S} + {S} speakers; bytes moved by the fused kernel: {T * 2 * S} in, "
                 f"{out.numel() * 8} out")
    compare("file mode", file_fused, file_plain, args.rounds, 200, 20, lines)

    # ---- chunk mode, one audio-hour of chunks
    B, S, F, Q = 7176, 3, 589, 51
    target = (rng.random((B, S, F)) < 0.3)
    preds = np.where(target, rng.uniform(0.3, 1.0, target.shape), rng.uniform(0.0, 0.7, target.shape)).astype(np.float32)
    preds, target = torch.from_numpy(preds).to(dev), torch.from_numpy(target.astype(np.uint8)).to(dev)
    thresholds = torch.linspace(0.0, 1.0, Q).to(dev)
    state = {}

    def chunk_fused():
        state["fused"] = metrics._der_update(preds, target, threshold=thresholds)

    # the permutation the kernel finds by itself is host work in the torch formulation: computed once, outside the timing
    perm = torch.from_numpy(metrics_truth.chunk_permutations(preds.cpu().numpy(), target.cpu().numpy())[0]).to(dev)
    perm = perm.to(torch.int64)

    def chunk_plain():
        counts, total = metrics_truth.torch_chunk_counts(preds, target, thresholds, perm)
        state["plain"] = (counts.sum(dim=0), total.sum())

    chunk_fused()
    chunk_plain()
    fa, md, conf, total = state["fused"]
    assert torch.equal(torch.stack([fa, md, conf], dim=-1), state["plain"][0]) and total == state["plain"][1], \
        "chunk mode: fused and plain counts differ"
    lines.append(f"chunk mode: {B} x {S} x {F} scores, {Q} thresholds; bytes moved by the fused kernels: "
                 f"{B * S * F * 5} in, {2 * 4 * B * (3 * Q + 1)} per-chunk tables written and read, {8 * (3 * Q + 1)} out; "
                 f"workspace {metrics.chunk_workspace_bytes(B, Q)} bytes; a (B, S, F, Q) float32 array is "
                 f"{B * S * F * Q * 4 / 2 ** 30:.2f} GiB")
    compare("chunk mode", chunk_fused, chunk_plain, args.rounds, 20, 2, lines)

    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
