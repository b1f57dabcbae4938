"""Time open-set speaker identification (`pyannote_audio_amd.identification`, csrc/identify.hip) against two other routes
(GPU).

Sizes: M = 4 096 speaker rows (1 024 files of 4 speakers), a gallery of G = 10 000 voiceprints, a cohort of N = 20 000
rows, D = 256, top = 300; half of the speakers are gallery entries plus noise, the rest strangers.  Three routes from the
per-file embeddings on the host to the per-file (index, value) arrays on the host, the gallery's own statistics taken
beforehand (enrolment-time work, timed on its own line):

  * device        `identify`: pa_cohort_stats_f64, pa_gallery_topk_f64, pa_gallery_pairs_f64 and pa_lsap_batch; no
                  (M, N) or (M, G) matrix exists anywhere;
  * host          SciPy `cdist` for both matrices, `np.sort` and `np.cumsum` for the statistics, SciPy's
                  `linear_sum_assignment` per file on its rows of the full matrix;
  * torch float64 the matrices materialised on the device by a float64 matmul of normalised rows, `torch.topk` for the
                  300 smallest and for the candidates, the same batched assignment as the device route.  Its distances
                  are not SciPy's bits, so it is compared by names, not by values.

Then the selection alone by device events: the fused kernels against matmul + `torch.topk` on the same tensors.
Median of `--runs` runs [min, max], the legs alternating round by round, after `--warmup` rounds; the names the routes
find are compared before anything is timed.  Writes profiles/identification_timing.txt (or --out)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
        print(f"round {n + 1} of {warmup + runs} done", flush=True)
    return times


def by_events(fn, runs: int, warmup: int) -> list:
    out = []
    for n in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if n >= warmup:
            out.append(e0.elapsed_time(e1) * 1e-3)
    return out


def line(name, values, scale=1e3):
    return f"{name:72s} {statistics.median(values) * scale:10.3f} ms   [{min(values) * scale:.3f}, " \
           f"{max(values) * scale:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--speakers", type=int, default=4)
    ap.add_argument("--gallery", type=int, default=10000)
    ap.add_argument("--cohort", type=int, default=20000)
    ap.add_argument("--dimension", type=int, default=256)
    ap.add_argument("--top", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "identification_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd.distance import linear_sum_assignment_batch
    from pyannote_audio_amd.identification import Gallery, cohort_stats, gallery_topk, identify
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial.distance import cdist
    ffi.require_gpu()
    device = torch.device("cuda:0")
    F, S, G, N, D, top = args.files, args.speakers, args.gallery, args.cohort, args.dimension, args.top
    M = F * S
    lines = [f"tools/time_identification.py --runs {args.runs} --warmup {args.warmup}",
             f"device: {torch.cuda.get_device_name(0)}; {os.cpu_count()} host CPUs, torch threads "
             f"{torch.get_num_threads()}",
             f"M = {M} speaker rows ({F} files of {S}), G = {G} voiceprints, N = {N} cohort rows, D = {D}, top = {top}",
             f"median [min, max] of {args.runs} runs, the legs alternating round by round", ""]

    rng = np.random.default_rng(0)
    table = rng.standard_normal((G, D)).astype(np.float32)
    cohort = rng.standard_normal((N, D)).astype(np.float32)
    rows = rng.standard_normal((M, D)).astype(np.float32)
    enrolled = rng.permutation(G)[:M // 2]
    rows[:M // 2] = table[enrolled] + 0.3 * rng.standard_normal((M // 2, D)).astype(np.float32)
    rows = rows[rng.permutation(M)]
    files = [rows[f * S:(f + 1) * S] for f in range(F)]
    gallery = Gallery([f"speaker {g}" for g in range(G)], table)
    gallery.normalise(cohort, top=top)
    threshold = -20.0     # between the enrolled speakers' normalised scores (about -50 at these sizes) and the strangers'

    # ---------------------------------------------------------------------------------------------------- routes
    def device_route():
        return identify(files, gallery, threshold=threshold, cohort=cohort, top=top)

    table64, cohort64, rows64 = (x.astype(np.float64) for x in (table, cohort, rows))

    def settle(cost_rows, columns):
        index, value = np.full(S, -1, dtype=np.int64), np.full(S, np.nan)
        r, c = linear_sum_assignment(cost_rows)
        value[r] = cost_rows[r, c]
        keep = value[r] <= threshold
        index[r[keep]] = columns[c[keep]] if columns is not None else c[keep]
        return index, value

    def host_route():
        s = np.sort(cdist(rows64, cohort64, "cosine"), axis=1)[:, :top]
        q_mean = np.cumsum(s, axis=1)[:, -1] / top
        e = (s - q_mean[:, None]) * (s - q_mean[:, None])
        q_std = np.sqrt(np.cumsum(e, axis=1)[:, -1] / top)
        d = cdist(rows64, table64, "cosine")
        score = 0.5 * ((d - q_mean[:, None]) / q_std[:, None] + (d - gallery.g_mean[None, :]) / gallery.g_std[None, :])
        return [settle(score[f * S:(f + 1) * S], None) for f in range(F)]

    g_mean_d, g_std_d = gallery.statistics(device)

    def torch_scores():
        q = torch.from_numpy(rows64).to(device)
        c, g = torch.from_numpy(cohort64).to(device), gallery.table(device)
        unit = lambda x: x / x.norm(dim=1, keepdim=True)   # noqa: E731
        qn = unit(q)
        s = torch.topk(1.0 - qn @ unit(c).T, top, dim=1, largest=False, sorted=True).values
        q_mean = s.cumsum(dim=1)[:, -1] / top
        q_std = (((s - q_mean[:, None]) ** 2).cumsum(dim=1)[:, -1] / top).sqrt()
        d = 1.0 - qn @ unit(g).T
        return 0.5 * ((d - q_mean[:, None]) / q_std[:, None] + (d - g_mean_d[None, :]) / g_std_d[None, :])

    def torch_route():
        score = torch_scores()
        best = torch.topk(score, S, dim=1, largest=False, sorted=True).indices.view(F, S * S)
        columns = torch.sort(best, dim=1).values                         # (duplicates stay: equal columns tie)
        cost = torch.gather(score.view(F, S, G), 2, columns[:, None, :].expand(F, S, S * S)).contiguous()
        col4row = linear_sum_assignment_batch(cost).cpu().numpy()
        cost, columns = cost.cpu().numpy(), columns.cpu().numpy()
        out = []
        for f in range(F):
            value = cost[f][np.arange(S), col4row[f]]
            out.append((np.where(value <= threshold, columns[f][col4row[f]], -1), value))
        return out

    routes = {"device: identify (cohort statistics, top-k, pairs, batched assignment)": device_route,
              "host: SciPy cdist, np.sort, SciPy assignment per file": host_route,
              "torch float64: matmul, torch.topk, batched assignment": torch_route}
    found = {name: fn() for name, fn in routes.items()}
    print("routes ran once", flush=True)
    names = list(routes)
    for f in range(F):
        assert np.array_equal(found[names[0]][f][0], found[names[1]][f][0]), f
        assert np.array_equal(found[names[0]][f][1], found[names[1]][f][1]), f    # SciPy's bits on both sides
        assert np.array_equal(found[names[0]][f][0], found[names[2]][f][0]), f
    accepted = int(sum((index >= 0).sum() for index, _ in found[names[0]]))
    lines += [f"whole routes, host clock, per-file results on the host at the end; {accepted} of {M} speakers named "
              f"(threshold {threshold}), the same by all three routes, values equal with == between device and host"]
    lines += [line("  " + name, values) for name, values in alternate(routes, args.runs, args.warmup).items()]

    # ------------------------------------------------------------------------------------------- selection alone
    q_d, c_d, g_d = (torch.from_numpy(x).to(device) for x in (rows64, cohort64, table64))
    mean_d, std_d, _ = cohort_stats(q_d, c_d, top)
    stats = (mean_d, std_d, g_mean_d, g_std_d)
    unit = lambda x: x / x.norm(dim=1, keepdim=True)   # noqa: E731
    qn, cn, gn = unit(q_d), unit(c_d), unit(g_d)
    def torch_statistics():
        s = torch.topk(1.0 - qn @ cn.T, top, dim=1, largest=False, sorted=True).values
        mean = s.cumsum(dim=1)[:, -1] / top
        return mean, (((s - mean[:, None]) ** 2).cumsum(dim=1)[:, -1] / top).sqrt()

    def torch_topk():
        d = 1.0 - qn @ gn.T
        return torch.topk(0.5 * ((d - mean_d[:, None]) / std_d[:, None] + (d - g_mean_d[None, :]) / g_std_d[None, :]),
                          S, dim=1, largest=False, sorted=True)

    lines += ["", "the selection alone, device events, inputs on the device, each side from the two tables to the same "
                  "outputs (mean and std; k sorted values and indices)"]
    lines += [line(f"  pa_cohort_stats_f64: {M} x {N}, K = {top}",
                   by_events(lambda: cohort_stats(q_d, c_d, top), args.runs, args.warmup)),
              line(f"  torch: 1 - Q @ C.T, topk({top}), cumsum mean and std",
                   by_events(torch_statistics, args.runs, args.warmup)),
              line(f"  pa_gallery_topk_f64: {M} x {G}, k = {S}, normalised",
                   by_events(lambda: gallery_topk(q_d, g_d, S, stats), args.runs, args.warmup)),
              line(f"  torch: 1 - Q @ G.T, normalise, topk({S})",
                   by_events(torch_topk, args.runs, args.warmup)),
              line(f"  gallery.normalise (enrolment time): {G} x {N}, K = {top}, upload and download included",
                   [_timed(lambda: gallery.normalise(cohort, top=top)) for _ in range(args.runs)])]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(text)


def _timed(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


if __name__ == "__main__":
    main()
