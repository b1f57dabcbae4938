"""KMeans on the device against the scikit-learn call it replaces, on the same machine in the same run.

1. `distance.kmeans` (csrc/kmeans.hip; upload, all launches, one download, the choice among the initialisations) against
   `KMeans(n_clusters=k, n_init=3, random_state=42, copy_x=False).fit_predict` on float32 unit vectors
   (tests/kmeans_model.py `data`): an hour-sized training set with k = 4 and 9, a short file, the joint-clustering size.
   Median of --repeats alternating runs with ranges; both sides once beforehand, untimed.
2. How the Lloyd iterations are enqueued (`distance.KMEANS_ROUND_ITERATIONS`): in rounds of 4, 8, 16 with the done flags
   read back in between, or all 300 at once without a read-back.
3. One synthetic file through a VBxClustering pipeline with a `num_speakers` that VBx does not find, with
   `kmeans_on_device` off and on: the KMeans step, the clustering tail and the whole call.

    python tools/time_kmeans.py [--repeats 5] [--hours 1.0] [--out profiles/kmeans_timing.txt]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(7176, 256, 6, 4), (7176, 256, 6, 9), (1200, 256, 3, 3), (57387, 256, 12, 16)]     # n, d, groups, k


def ms(values) -> str:
    return f"median {statistics.median(values) * 1e3:9.2f} ms  [{min(values) * 1e3:.2f}, {max(values) * 1e3:.2f}]"


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def sklearn_call(X, k):
    from sklearn.cluster import KMeans
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return KMeans(n_clusters=k, n_init=3, random_state=42, copy_x=False).fit_predict(X.copy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--num-speakers", type=int, default=5)
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_timing.txt"))
    args = ap.parse_args()
    import pyannote_audio_amd.distance as distance
    from kmeans_model import data
    device = torch.device("cuda:0")
    lines = [f"KMeans on the device (distance.kmeans -> pa_kmeans_f64) against sklearn.cluster.KMeans(n_init=3, "
             f"random_state=42) on the host; {torch.cuda.get_device_name(0)}, {torch.get_num_threads()} host threads, "
             f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS')}; median of {args.repeats} alternating runs [min, max]",
             ""]

    def emit(line=""):
        lines.append(line)
        print(line, flush=True)

    emit("1. the call: float32 unit vectors in, labels out")
    for n, d, g, k in SHAPES:
        X = data(n, d, g, 0.8, 100, np.float32)
        want = sklearn_call(X, k)
        want64 = sklearn_call(X.astype(np.float64), k)
        got, out = distance.kmeans(X, k, device, details=True)
        dev_t, host_t = [], []
        for _ in range(args.repeats):
            dev_t.append(clock(lambda: distance.kmeans(X, k, device))[0])
            host_t.append(clock(lambda: sklearn_call(X, k))[0])
        emit(f"  ({n}, {d}) k={k:2d}  device {ms(dev_t)}   sklearn {ms(host_t)}   "
             f"x{statistics.median(host_t) / statistics.median(dev_t):.1f}; Lloyd iterations "
             f"{out['status'][:, 0].tolist()}, {int((got != want64).sum())} labels differ from sklearn on the float64 values, "
             f"{int((got != want).sum())} from its float32 run")
    emit()
    emit(f"2. rounds of Lloyd iterations between two reads of the done flags (0: all 300 enqueued, no read-back); "
         f"the library's setting is {distance.KMEANS_ROUND_ITERATIONS}")
    setting = distance.KMEANS_ROUND_ITERATIONS
    for n, d, g, k in SHAPES[:3]:
        X = data(n, d, g, 0.8, 100, np.float32)
        taken = {r: [] for r in (0, 4, 8, 16)}
        for _ in range(args.repeats):
            for r in taken:
                distance.KMEANS_ROUND_ITERATIONS = r
                taken[r].append(clock(lambda: distance.kmeans(X, k, device))[0])
        distance.KMEANS_ROUND_ITERATIONS = setting
        for r, values in taken.items():
            emit(f"  ({n}, {d}) k={k:2d}  rounds of {r:2d}: {ms(values)}")
    if not args.skip_pipeline:
        emit()
        emit(f"3. one synthetic {args.hours:g} h file (bench.synth_hour, 3 speakers) through the VBxClustering pipeline "
             f"with num_speakers={args.num_speakers}")
        from bench import synth_hour
        from time_vbx_tuning import vbx_pipeline
        pipeline = vbx_pipeline(device)
        wav = synth_hour(args.hours, seed=0, device=device).cpu()
        file = {"waveform": wav, "sample_rate": 16000, "uri": "hour"}
        clu = pipeline.clustering
        taken = {False: {"kmeans": [], "cluster": [], "call": []}, True: {"kmeans": [], "cluster": [], "call": []}}
        pipeline(file, num_speakers=args.num_speakers)        # untimed
        for _ in range(args.repeats):
            for on in (False, True):
                clu.kmeans_on_device = on
                dt, out = clock(lambda: pipeline(file, num_speakers=args.num_speakers))
                assert clu.timings["kmeans_route"] == ("device" if on else "host")
                taken[on]["kmeans"].append(clu.timings["kmeans"])
                taken[on]["cluster"].append(pipeline.timings["clustering"])
                taken[on]["call"].append(dt)
        emit(f"  {clu.timings['num_embeddings']} training embeddings, VBx keeps {clu.timings['vbx_speakers']} speakers")
        for on in (False, True):
            emit(f"  kmeans_on_device={on!s:5}  KMeans {ms(taken[on]['kmeans'])}   clustering {ms(taken[on]['cluster'])}"
                 f"   whole call {ms(taken[on]['call'])}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
