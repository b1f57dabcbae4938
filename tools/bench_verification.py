"""Times a speaker-verification evaluation on the device (pyannote_audio_amd.verification: `trial_distances` then
`equal_error_rate`, csrc/verification.hip) beside the reference's host recipe on the same machine
(pipelines/speaker_verification.py:880-892: `scipy.spatial.distance.cdist` on two (1, D) arrays per trial, then
`det_curve`, which is `sklearn.metrics.roc_curve` and a few numpy lines), on seeded 256-d float32 embeddings of
4 874 files from 40 speakers:

  37 720 trials            the size of VoxCeleb1-O
  580 000 trials           about VoxCeleb1-E / -H
  all pairs of 4 874       11 875 501 trials

Device: the embedding table and the trial indices already lie in device memory (where `forward_ragged` leaves the
embeddings); a call ends when the equal error rate is a Python float, so the host clock around it includes the
launches, torch's sort and the copy of the status block.  Warm-up calls of the same size first; the median of
`--rounds` calls is reported with the fastest and the slowest.  The three stages (trial kernels; negation, sort and
label gather; `pa_det_curve_f64` on the sorted keys) are then run one after the other, each between device events of
its own.  Host: one run (it is long); the per-trial loop of the all-pairs size is
timed over its first `--host-trials` trials unless `--full-host` is given, and the line says so.  The two sides'
results are compared with `==` wherever the host computed them.

    python tools/bench_verification.py [--out profiles/verification_eval.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NUM_FILES, NUM_SPEAKERS, DIM = 4874, 40, 256


def embeddings(rng):
    speaker = rng.integers(0, NUM_SPEAKERS, size=NUM_FILES)
    centres = rng.normal(size=(NUM_SPEAKERS, DIM))
    return (centres[speaker] + 2.5 * rng.normal(size=(NUM_FILES, DIM))).astype(np.float32), speaker


def host_distances(table, index1, index2):
    from scipy.spatial.distance import cdist
    rows = [table[i:i + 1] for i in range(len(table))]
    return [cdist(rows[i], rows[j], metric="cosine")[0][0] for i, j in zip(index1.tolist(), index2.tolist())]


def host_eer(y_true, distances):
    from sklearn.metrics import roc_curve
    fpr, tpr, _ = roc_curve(y_true, -np.asarray(distances), pos_label=True)
    fnr = 1 - tpr
    k = np.where(fpr > fnr)[0][0]
    return float(0.25 * (fpr[k - 1] + fpr[k] + fnr[k - 1] + fnr[k]))


def event_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--host-trials", type=int, default=1000000)
    ap.add_argument("--full-host", action="store_true")
    ap.add_argument("--sizes", default="37720,580000,all")
    args = ap.parse_args(argv)
    import scipy
    import sklearn
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd import verification as v
    ffi.require_gpu()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    table, speaker = embeddings(rng)
    table_dev = torch.from_numpy(table).to(dev)
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; scipy {scipy.__version__}; "
             f"scikit-learn {sklearn.__version__}; {NUM_FILES} x {DIM} float32 embeddings, {NUM_SPEAKERS} speakers; "
             f"host clock around whole evaluations, device: median of {args.rounds} calls after 2 warm-up calls, "
             f"host: one run"]
    for size in args.sizes.split(","):
        if size == "all":
            index1, index2 = (a.astype(np.int32) for a in np.triu_indices(NUM_FILES, k=1))
            name = f"all pairs of {NUM_FILES}"
        else:
            index1, index2 = (rng.integers(0, NUM_FILES, size=int(size)).astype(np.int32) for _ in range(2))
            name = f"{int(size)} trials"
        T = len(index1)
        y_true = speaker[index1] == speaker[index2]
        i1, i2, y = (torch.from_numpy(a).to(dev) for a in (index1, index2, y_true))

        def evaluate():
            dist = v.trial_distances(table_dev, i1, i2)
            return dist, v.equal_error_rate(y, dist, distances=True)

        for _ in range(2):
            dist, eer = evaluate()
        torch.cuda.synchronize()
        whole = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            dist, eer = evaluate()
            whole.append(time.perf_counter() - t0)
        # the three stages of one evaluation, each between device events of its own, in one run per round
        lib = ffi.load()
        fps, tps = (torch.empty(T + 1, dtype=torch.int32, device=dev) for _ in range(2))
        status = torch.empty(8, dtype=torch.int64, device=dev)
        nbytes = int(lib.pa_det_workspace_bytes(T))
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        parts = {"trial kernels": [], "negate, sort, gather": [], "curve kernels": []}

        def sort_stage():
            keys, order = torch.sort(-dist, stable=True)
            return keys, y[order].to(torch.uint8).contiguous()

        def curve_stage():
            ffi.check(lib.pa_det_curve_f64(ffi.ptr(keys), ffi.ptr(labels), T, 1, ffi.ptr(fps), ffi.ptr(tps), None, None,
                                           None, ffi.ptr(status), ffi.ptr(work), nbytes, ffi.stream()))

        for _ in range(args.rounds):
            ms, dist = event_ms(lambda: v.trial_distances(table_dev, i1, i2))
            parts["trial kernels"].append(ms)
            ms, (keys, labels) = event_ms(sort_stage)
            parts["negate, sort, gather"].append(ms)
            parts["curve kernels"].append(event_ms(curve_stage)[0])
        staged = float(status.cpu().numpy()[5:6].view(np.float64)[0])
        assert staged == eer, f"staged eer {staged!r} != eer of the whole evaluation {eer!r}"
        del keys, labels, fps, tps, work
        lines.append(f"{name}: T = {T}, {int(y_true.sum())} target trials, eer = {eer!r}; device reads "
                     f"{table.nbytes} B of embeddings and {8 * T} B of indices, writes {8 * T} B of distances; curve "
                     f"workspace {ffi.load().pa_det_workspace_bytes(T)} B")
        lines.append(f"  device  whole evaluation   median {statistics.median(whole) * 1e3:10.3f} ms   min "
                     f"{min(whole) * 1e3:10.3f}   max {max(whole) * 1e3:10.3f}")
        for label, t in parts.items():
            lines.append(f"  device  {label:<22} median {statistics.median(t):10.3f} ms   min {min(t):10.3f}   max "
                         f"{max(t):10.3f}   (device events around that stage alone)")
        limit = T if args.full_host else min(T, args.host_trials)
        t0 = time.perf_counter()
        host = host_distances(table, index1[:limit], index2[:limit])
        loop = time.perf_counter() - t0
        assert np.array_equal(np.asarray(host), dist[:limit].cpu().numpy()), "host and device distances differ"
        scores = host if limit == T else dist.cpu().numpy()
        t0 = time.perf_counter()
        want = host_eer(y_true, scores)
        curve = time.perf_counter() - t0
        assert want == eer, f"host eer {want!r} != device eer {eer!r}"
        lines.append(f"  host    per-trial cdist    {loop * 1e3:10.1f} ms over "
                     + (f"all {T} trials" if limit == T else f"the first {limit} of {T} trials (not the whole list)")
                     + f" = {loop / limit * 1e6:.2f} us per trial; distances equal the device's bit for bit")
        lines.append(f"  host    sklearn roc_curve  {curve * 1e3:10.1f} ms over all {T} trials"
                     + ("" if limit == T else " (on the device's distances)") + "; eer equal with ==")
        if limit == T:
            lines.append(f"  host / device = {(loop + curve) / statistics.median(whole):.1f} x")
        else:
            lines.append(f"  host / device: not measured for the whole list (the host loop was cut short); per trial, "
                         f"the host loop alone takes {loop / limit * 1e6:.2f} us against "
                         f"{statistics.median(whole) / T * 1e6:.4f} us for the whole device evaluation")
        del i1, i2, y, dist
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
