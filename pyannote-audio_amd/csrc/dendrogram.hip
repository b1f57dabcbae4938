// Every flat cut of one dendrogram in one launch on gfx950
// (reference: the `optimize` command, __main__.py:116-283, re-runs pipelines/clustering.py:384-392 --
//  scipy.cluster.hierarchy.fcluster(Z, threshold, "distance") -- for every candidate threshold of every file).
//
// The plan (csrc/dendrogram_plan.h, host, once per dendrogram) lists the 2n - 1 nodes in the order in which SciPy's
// cluster_monocrit hands out cluster numbers.  For a threshold t a node starts a flat cluster iff
// own_md <= t < parent_md (float64 comparisons, as SciPy makes them), so:
//   1. inclusive prefix SUM of those flags along the timeline = the cluster's number, written at the first leaf
//      position `lo` of the node (left-first leaf order: the leaves of a subtree are contiguous, the starting nodes
//      of a cut partition the positions into spans and each span's first position receives its number);
//   2. inclusive prefix scan over the positions with the associative operator "last non-zero wins" carries every
//      number across its span;
//   3. leaf l reads position leaf_lo[l].
// One workgroup per threshold walks the timeline, then the positions, in tiles of 1024 and carries the running value
// from tile to tile: O(n) work per threshold, no atomics, no workgroup waits for another.  The row of positions is
// a scratch row in global memory that only its own workgroup touches (__syncthreads orders it at workgroup scope).
#include "common.h"
#include "dendrogram_plan.h"

namespace pa {

constexpr int DC_THREADS = 256;                     // 4 waves
constexpr int DC_ITEMS = 4;                         // consecutive elements per thread
constexpr int DC_TILE = DC_THREADS * DC_ITEMS;
constexpr int DC_MAX_CHUNK = 256;                   // thresholds per launch (bounds the scratch rows)

struct ScanSum {
  __device__ static __forceinline__ int apply(int a, int b) { return a + b; }
};
struct ScanLastNonZero {   // identity 0 on both sides, associative: the right-most non-zero operand
  __device__ static __forceinline__ int apply(int a, int b) { return b != 0 ? b : a; }
};

// exclusive scan of one value per thread over the block (0 = identity of both operators); `total` = all of them.
// `wave_tot`: DC_THREADS / 64 ints of LDS, free again when the call returns.
template <class Op>
__device__ __forceinline__ int block_scan_exclusive(int v, int* wave_tot, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x = Op::apply(y, x);
  }
  if (lane == 63) wave_tot[w] = x;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < DC_THREADS / 64; ++i) {
    if (i < w) before = Op::apply(before, wave_tot[i]);
    all = Op::apply(all, wave_tot[i]);
  }
  int left = __shfl_up(x, 1, 64);
  if (lane == 0) left = 0;
  __syncthreads();
  total = all;
  return Op::apply(before, left);
}

// grid = thresholds of this launch, block = DC_THREADS.  M = 2n - 1 timeline slots.
__global__ __launch_bounds__(DC_THREADS) void k_dendrogram_cuts(
    const double* __restrict__ tl_own, const double* __restrict__ tl_parent, const int* __restrict__ tl_lo,
    const int* __restrict__ leaf_lo, int n, const double* __restrict__ thresholds, int* __restrict__ labels,
    int* __restrict__ num_clusters, int* scratch) {
  __shared__ int wave_tot[DC_THREADS / 64];
  const int tid = threadIdx.x;
  const int M = 2 * n - 1;
  // (+inf must still lie under the root's parent_md = +inf: it counts as the largest finite double)
  const double t = fmin(thresholds[blockIdx.x], 1.7976931348623157e308);
  int* pos = scratch + (size_t)blockIdx.x * n;
  int* out = labels + (size_t)blockIdx.x * n;

  for (int p = tid; p < n; p += DC_THREADS) pos[p] = 0;
  __syncthreads();

  // 1. cluster numbers along the timeline
  int carry = 0;
  for (int base = 0; base < M; base += DC_TILE) {
    const int s0 = base + tid * DC_ITEMS;
    bool f[DC_ITEMS];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < DC_ITEMS; ++j) {
      const int s = s0 + j;
      f[j] = s < M && tl_own[s] <= t && t < tl_parent[s];
      mine += f[j] ? 1 : 0;
    }
    int total;
    int number = carry + block_scan_exclusive<ScanSum>(mine, wave_tot, total);
#pragma unroll
    for (int j = 0; j < DC_ITEMS; ++j) {
      if (f[j]) {
        ++number;
        const int p = tl_lo[s0 + j];
        if ((unsigned)p < (unsigned)n) pos[p] = number;   // (always true for a plan of dendrogram_plan)
      }
    }
    carry += total;
  }
  if (tid == 0) num_clusters[blockIdx.x] = carry;
  __syncthreads();

  // 2. every number across its span of positions
  carry = 0;
  for (int base = 0; base < n; base += DC_TILE) {
    const int p0 = base + tid * DC_ITEMS;
    int v[DC_ITEMS];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < DC_ITEMS; ++j) {
      v[j] = p0 + j < n ? pos[p0 + j] : 0;
      mine = ScanLastNonZero::apply(mine, v[j]);
    }
    int total;
    int running = ScanLastNonZero::apply(carry, block_scan_exclusive<ScanLastNonZero>(mine, wave_tot, total));
#pragma unroll
    for (int j = 0; j < DC_ITEMS; ++j) {
      running = ScanLastNonZero::apply(running, v[j]);
      if (p0 + j < n) pos[p0 + j] = running;
    }
    carry = ScanLastNonZero::apply(carry, total);
  }
  __syncthreads();

  // 3. leaves read their position
  for (int l = tid; l < n; l += DC_THREADS) {
    const int p = leaf_lo[l];
    out[l] = ((unsigned)p < (unsigned)n ? pos[p] : 0) - 1;
  }
}

}  // namespace pa

extern "C" {

int pa_dendrogram_plan(const double* Z, int n, double* tl_own, double* tl_parent, int32_t* tl_lo, int32_t* leaf_lo) {
  PA_REQUIRE(Z && tl_own && tl_parent && tl_lo && leaf_lo, "pa_dendrogram_plan: null argument");
  PA_REQUIRE(n >= 2 && n <= (1 << 30), "pa_dendrogram_plan: n = %d outside 2..2^30", n);
  const int rc = pa::dendrogram_plan(Z, n, tl_own, tl_parent, tl_lo, leaf_lo);
  if (rc == 2) pa::set_error("pa_dendrogram_plan: out of host memory for n = %d", n);
  if (rc == 3) pa::set_error("pa_dendrogram_plan: Z is not a valid linkage matrix of %d leaves", n);
  return rc;
}

int pa_dendrogram_cuts_chunk(void) { return pa::DC_MAX_CHUNK; }

size_t pa_dendrogram_cuts_workspace_bytes(int n, long T) {
  if (n < 2 || n > (1 << 30) || T < 1) return 0;
  return (size_t)(T < pa::DC_MAX_CHUNK ? T : pa::DC_MAX_CHUNK) * (size_t)n * sizeof(int32_t);
}

int pa_dendrogram_cuts(const double* tl_own, const double* tl_parent, const int32_t* tl_lo, const int32_t* leaf_lo,
                       int n, const double* thresholds, long T, int32_t* labels, int32_t* num_clusters, void* ws,
                       size_t ws_bytes, void* stream) {
  if (T == 0) return 0;
  PA_REQUIRE(n >= 2 && n <= (1 << 30), "pa_dendrogram_cuts: n = %d outside 2..2^30", n);
  PA_REQUIRE(T > 0, "pa_dendrogram_cuts: T = %ld", T);
  PA_REQUIRE(tl_own && tl_parent && tl_lo && leaf_lo && thresholds && labels && num_clusters && ws,
             "pa_dendrogram_cuts: null argument");
  const size_t row = (size_t)n * sizeof(int32_t);
  long chunk = (long)(ws_bytes / row);
  if (chunk > pa::DC_MAX_CHUNK) chunk = pa::DC_MAX_CHUNK;
  PA_REQUIRE(chunk >= 1, "pa_dendrogram_cuts: workspace of %zu bytes holds no row of %d positions", ws_bytes, n);
  pa::ProfScope prof("k_dendrogram_cuts", stream, 0.0, (double)T * (20.0 * (2.0 * n - 1) + 20.0 * n));
  for (long t0 = 0; t0 < T; t0 += chunk) {
    const int count = (int)(T - t0 < chunk ? T - t0 : chunk);
    hipLaunchKernelGGL(pa::k_dendrogram_cuts, dim3(count), dim3(pa::DC_THREADS), 0, (hipStream_t)stream, tl_own,
                       tl_parent, tl_lo, leaf_lo, n, thresholds + t0, labels + (size_t)t0 * n, num_clusters + t0,
                       (int*)ws);
    PA_CHECK_LAUNCH("pa_dendrogram_cuts");
  }
  return 0;
}

}  // extern "C"
