"""Times single / complete / average / weighted / Ward linkage on the device (csrc/linkage_chain.hip, through
`distance.linkage_chain`: X on the host -> Z on the host) against the path these methods took before: pdist on the
device + download + scipy.cluster.hierarchy.linkage for the Euclidean and "geometric" cases, SciPy alone (pdist
included) for cosine with a non-geometric method.  n = 7 176 (one audio-hour), d = 256, clustered unit vectors; median
of 5 after one warm-up; every device result is compared with the host's.
usage (GPU box): python tools/time_linkage_methods.py [n]      -> profiles/linkage_methods_timing.txt
LM_DEVICE_ONLY=1 times the device path alone and writes no file (comparing two builds of the library: PA_LIB)."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from scipy.cluster.hierarchy import linkage
from pyannote_audio_amd import distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dev = torch.device("cuda:0")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 7176
repeats = int(os.environ.get("LM_REPEATS", "5"))
device_only = os.environ.get("LM_DEVICE_ONLY") == "1"
rng = np.random.default_rng(0)
c = rng.standard_normal((4, 256))
X = (c[rng.integers(0, 4, n)] + 0.6 * rng.standard_normal((n, 256))).astype(np.float32)
X /= np.linalg.norm(X, axis=1, keepdims=True)


def device_path(method, metric):
    return distance.linkage_chain(X, method, metric, dev)


def parent_path(method, metric):
    """what AgglomerativeClustering.dendrogram did for these methods before the chain kernels"""
    if metric == "euclidean":
        return linkage(distance.pdist_euclidean(X, device=dev), method=method)
    return linkage(X, method=method, metric=metric)


def median_seconds(fn, *args):
    Z = fn(*args)                      # warm-up
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        Z = fn(*args)
        times.append(time.perf_counter() - t)
    return statistics.median(times), Z


lines = [f"linkage methods, n = {n}, d = 256, clustered unit vectors; wall time X on the host -> Z on the host, "
         f"median of {repeats} after one warm-up ({torch.cuda.get_device_name(0)})",
         f"{'method':10s} {'pdist':10s} {'device ms':>10s} {'parent path ms':>15s} {'speed-up':>9s}  identical"]
# (method, pdist) as AgglomerativeClustering.dendrogram pairs them for metric="cosine" (ward is geometric: Euclidean
# pdist of the normalised rows), then the metric="euclidean" pairing of one chain method and of single
for method, metric in [("single", "cosine"), ("complete", "cosine"), ("average", "cosine"), ("weighted", "cosine"),
                       ("ward", "euclidean"), ("single", "euclidean"), ("average", "euclidean")]:
    t_dev, Z = median_seconds(device_path, method, metric)
    if device_only:
        print(f"{method:10s} {metric:10s} {1e3 * t_dev:10.1f}", flush=True)
        continue
    t_par, Z_ref = median_seconds(parent_path, method, metric)
    lines.append(f"{method:10s} {metric:10s} {1e3 * t_dev:10.1f} {1e3 * t_par:15.1f} {t_par / t_dev:8.1f}x  "
                 f"{np.array_equal(Z, Z_ref)}")
    print(lines[-1], flush=True)
if device_only:
    sys.exit(0)
out = os.path.join(ROOT, "profiles", "linkage_methods_timing.txt")
with open(out, "w") as fp:
    fp.write("\n".join(lines) + "\n")
print("\n".join(lines[:2]))
print("written to", out)
