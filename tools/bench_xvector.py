"""Throughput of the two x-vector embedding models on 10 s chunks: XVectorSincNet (`pa_xvec_forward`) and XVectorMFCC
(`pa_xvec_mfcc_forward`, torchaudio MFCC front end of csrc/mfcc.hip), seeded weights, B = 512 chunks per call, in one
process.  Every figure is the median of 3 timed calls after one warm-up call, with device synchronisation.  Then a
separate `rocprofv3 --kernel-trace --stats` run of XVectorMFCC alone (a fresh child process) gives the MFCC front-end
kernels' share of the kernel time of `pa_xvec_mfcc_forward`.  Prints one JSON line.

    python tools/bench_xvector.py [--chunks 512] [--out profiles/xvector_mfcc.json]
                                  [--stats-csv profiles/xvector_mfcc_kernels.csv]
    python tools/bench_xvector.py --only mfcc --calls 3     # what the traced child runs
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))     # the seeded XVectorMFCC oracle (tests/xvector_mfcc_oracle.py)

SR = 16000
FRONT_END_KERNELS = ("k_mfcc_mel", "k_mfcc_dct")


def engines(device):
    from oracle import seeded_xvector
    from xvector_mfcc_oracle import seeded_xvector_mfcc, xvector_mfcc_hparams
    from pyannote_audio_amd.embedding import XVectorEngine, XVectorMFCCEngine
    from pyannote_audio_amd.weights import XVectorMFCCPack, XVectorPack
    sinc = XVectorEngine(XVectorPack(seeded_xvector().state_dict(), {"sincnet": {"stride": 10}}, device))
    m = seeded_xvector_mfcc()
    mfcc = XVectorMFCCEngine(XVectorMFCCPack(m.state_dict(), xvector_mfcc_hparams(m), device))
    return {"sincnet": sinc, "mfcc": mfcc}


def timed(fn, repeats: int = 3) -> float:
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def front_end_share(stats_csv: str) -> dict:
    """the MFCC front-end kernels' share of all kernel time in a rocprofv3 --stats kernel table"""
    total = front = 0.0
    with open(stats_csv) as fp:
        for row in csv.DictReader(fp):
            ns = float(row["TotalDurationNs"])
            total += ns
            if any(k in row["Name"] for k in FRONT_END_KERNELS):
                front += ns
    return {"front_end_share": front / total if total else None, "front_end_ms": front * 1e-6,
            "kernel_ms": total * 1e-6}


def traced_share(args) -> dict:
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return {"front_end_share": None, "trace_error": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as d:
        cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "xvector_mfcc", "--",
               sys.executable, os.path.abspath(__file__), "--only", "mfcc", "--calls", "3", "--chunks", str(args.chunks)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not found:
            return {"front_end_share": None, "trace_error": f"rocprofv3 exit {r.returncode}: {r.stdout[-400:]}"}
        if args.stats_csv:
            os.makedirs(os.path.dirname(os.path.abspath(args.stats_csv)), exist_ok=True)
            shutil.copyfile(found[0], args.stats_csv)
        return front_end_share(found[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=512)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--only", choices=["mfcc"], default=None)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats-csv", default=None)
    args = ap.parse_args()
    import pyannote_audio_amd.ffi as ffi
    ffi.require_gpu()
    dev = torch.device("cuda:0")
    N, B = int(args.seconds * SR), args.chunks
    g = torch.Generator().manual_seed(0)
    wav = (0.1 * torch.randn(B * N, generator=g)).clamp(-1, 1).to(dev)   # made on the host: no setup kernels
    eng = engines(dev)
    if args.only == "mfcc":
        for _ in range(args.calls):
            eng["mfcc"].forward_strided(wav, N, B, N)
        torch.cuda.synchronize()
        return
    rate = {}
    for name, e in eng.items():
        rate[name] = B / timed(lambda: e.forward_strided(wav, N, B, N))
        e.release_workspace()
    out = {"workload": f"{B} chunks of {args.seconds:g} s per call, seeded weights, median of 3 after a warm-up",
           "xvector_sincnet_chunks_per_s": round(rate["sincnet"], 1),
           "xvector_mfcc_chunks_per_s": round(rate["mfcc"], 1),
           "mfcc_over_sincnet": round(rate["mfcc"] / rate["sincnet"], 4),
           "mfcc_frames": eng["mfcc"].num_pool_frames(N) + 14, "sincnet_frames": eng["sincnet"].num_pool_frames(N) + 14,
           "device": torch.cuda.get_device_name(dev)}
    del eng
    torch.cuda.empty_cache()
    if not args.no_trace:
        out.update({k: (round(v, 4) if isinstance(v, float) else v) for k, v in traced_share(args).items()})
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
