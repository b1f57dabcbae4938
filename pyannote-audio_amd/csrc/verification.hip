// Speaker-verification trials on the device: the cosine distance of every trial (i, j) over one embedding table,
// and the detection-error-tradeoff curve with its equal error rate over the sorted scores
// (reference: pipelines/speaker_verification.py:858-895 `main`, torchmetrics/classification/equal_error_rate.py).
//
// TRIAL DISTANCES.  scipy.spatial.distance.cdist(E[i:i+1], E[j:j+1], "cosine")[0, 0] in float64, bit for bit, by
// the device functions that pa_cdist_cosine_f64 uses (cosine_f64.h): every row norm once, then one thread per trial,
// which keeps dot2way's sequential order.
//
// DET CURVE.  sklearn.metrics.roc_curve (drop_intermediate=True) followed by det_curve's fnr = 1 - tpr and its
// crossing rule, restated in integers.  The caller sorts the keys ASCENDING with a stable sort and gathers the
// labels alongside; position p of the DESCENDING order is element T - 1 - p, which is what sklearn's mergesort
// followed by [::-1] visits, so the element that ends a tie group is the same one, sign of zero included.
// A tie group is a run of numerically equal keys (-0.0 == 0.0: the comparison is on values).
//
// Launch sequence (DET_BLOCK = 1024 positions per workgroup, DET_CHUNK = 1024 workgroup sums per scan chunk):
//   1  k_det_block_counts   per workgroup: positives and group ends, packed in one 64-bit word; non-finite keys
//   2  k_det_chunk_sums, k_det_scan_top, k_det_scan_chunks   exclusive scan of the workgroup sums, two levels
//   3  k_det_groups         per position: inclusive positives and group ordinal; a group's end writes the group's
//                           (elements so far, positives so far)
//   4  k_det_corner_counts  per group: kept or not; kept per workgroup -> the scan of 2 again -> k_det_compact
//                           writes the kept points in order and takes the first crossing fpr > fnr by a minimum
//   5  k_det_finish         k, eer and the status block
// No workgroup waits for another one: every dependency is a kernel boundary.  All counts are integers, the minimum
// is an integer atomic, and every float64 value is one correctly rounded division (or 1 - x) of integers, so a
// second call returns the same bits.
// hipcc-flags: -ffp-contract=off
#include <cstddef>

#include "common.h"
#include "cosine_f64.h"
#include "pyannote_amd.h"

namespace pa {

constexpr int DET_THREADS = 256;
constexpr int DET_ITEMS = 4;                          // consecutive positions per thread
constexpr int DET_BLOCK = DET_THREADS * DET_ITEMS;    // positions per workgroup
constexpr int DET_CHUNK = 1024;                       // workgroup sums per chunk of the scan's lower level
constexpr int DET_TOP_ITEMS = 8;                      // chunk sums per thread of the single top-level workgroup
constexpr long DET_MAX_T = 0x7fffffffL;
static_assert(DET_CHUNK == DET_THREADS * DET_ITEMS, "a chunk is scanned by one workgroup, DET_ITEMS per thread");
static_assert((DET_MAX_T + DET_BLOCK - 1) / DET_BLOCK <= (long)DET_CHUNK * DET_THREADS * DET_TOP_ITEMS,
              "the top level holds every chunk of the largest input");

// a pair of counts that travels, and is summed, as one word: positives (or kept points) low, group ends high.
// Both stay below 2^31, so the low half never carries.
typedef unsigned long long pair64;
__device__ __forceinline__ pair64 make_pair64(uint32_t lo, uint32_t hi) { return (pair64)lo | ((pair64)hi << 32); }
__device__ __forceinline__ uint32_t pair_lo(pair64 v) { return (uint32_t)v; }
__device__ __forceinline__ uint32_t pair_hi(pair64 v) { return (uint32_t)(v >> 32); }

// workspace header
struct DetHeader {
  pair64 totals;        // (positives, groups)
  pair64 kept;          // (kept groups, 0)
  uint32_t first_cross; // smallest kept index with fpr > fnr
  uint32_t pad;
};

// exclusive prefix of v over the DET_THREADS threads of the workgroup (red: 4 words of LDS); *total = the sum
__device__ __forceinline__ pair64 block_exclusive_scan(pair64 v, pair64* red, pair64* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  pair64 inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const pair64 up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  __syncthreads();                     // (red may still be read from a previous call)
  if (lane == 63) red[w] = inc;
  __syncthreads();
  pair64 before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < DET_THREADS / 64; ++i) {
    if (i < w) before += red[i];
    all += red[i];
  }
  *total = all;
  return before + inc - v;
}

// key and label of position p of the descending order; p in [0, T)
__device__ __forceinline__ double det_key(const double* __restrict__ keys, long T, long p) { return keys[T - 1 - p]; }

// flags of the DET_ITEMS positions from p0 on: bit i = positive, bit 8 + i = ends a tie group; positions >= T: none
__device__ __forceinline__ uint32_t det_flags(const double* __restrict__ keys, const uint8_t* __restrict__ labels,
                                              long T, long p0, int* nonfinite) {
  uint32_t f = 0;
  if (p0 >= T) return 0;
  double cur = det_key(keys, T, p0);
#pragma unroll
  for (int i = 0; i < DET_ITEMS; ++i) {
    const long p = p0 + i;
    if (p >= T) break;
    if (nonfinite && !(fabs(cur) <= 1.7976931348623157e308)) ++*nonfinite;
    if (labels[T - 1 - p]) f |= 1u << i;
    if (p + 1 == T) {
      f |= 0x100u << i;
    } else {
      const double next = det_key(keys, T, p + 1);
      if (cur != next) f |= 0x100u << i;   // a comparison of values: -0.0 == 0.0; NaN ends a group
      cur = next;
    }
  }
  return f;
}

__global__ __launch_bounds__(DET_THREADS) void k_det_block_counts(const double* __restrict__ keys,
                                                                  const uint8_t* __restrict__ labels, long T,
                                                                  pair64* __restrict__ block_sums,
                                                                  unsigned long long* __restrict__ nonfinite_out) {
  __shared__ pair64 red[DET_THREADS / 64];
  __shared__ int s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  int bad = 0;
  const uint32_t f = det_flags(keys, labels, T, (long)blockIdx.x * DET_BLOCK + threadIdx.x * DET_ITEMS, &bad);
  pair64 total;
  block_exclusive_scan(make_pair64(__popc(f & 0xffu), __popc(f >> 8)), red, &total);
  if (bad) atomicAdd(&s_bad, bad);
  __syncthreads();
  if (threadIdx.x == 0) {
    block_sums[blockIdx.x] = total;
    if (s_bad) atomicAdd(nonfinite_out, (unsigned long long)s_bad);
  }
}

// chunk_sums[c] = sum of block_sums[c * DET_CHUNK ...), n entries in all
__global__ __launch_bounds__(DET_THREADS) void k_det_chunk_sums(const pair64* __restrict__ block_sums, int n,
                                                                pair64* __restrict__ chunk_sums) {
  __shared__ pair64 red[DET_THREADS / 64];
  pair64 v = 0;
  const long base = (long)blockIdx.x * DET_CHUNK + threadIdx.x * DET_ITEMS;
#pragma unroll
  for (int i = 0; i < DET_ITEMS; ++i)
    if (base + i < n) v += block_sums[base + i];
  pair64 total;
  block_exclusive_scan(v, red, &total);
  if (threadIdx.x == 0) chunk_sums[blockIdx.x] = total;
}

// one workgroup: chunk_sums (nc <= DET_THREADS * DET_TOP_ITEMS) -> exclusive prefixes in place; *total = the sum
__global__ __launch_bounds__(DET_THREADS) void k_det_scan_top(pair64* __restrict__ chunk_sums, int nc,
                                                              pair64* __restrict__ total_out) {
  __shared__ pair64 red[DET_THREADS / 64];
  pair64 v[DET_TOP_ITEMS], sum = 0;
  const int base = threadIdx.x * DET_TOP_ITEMS;
#pragma unroll
  for (int i = 0; i < DET_TOP_ITEMS; ++i) {
    v[i] = base + i < nc ? chunk_sums[base + i] : 0;
    sum += v[i];
  }
  pair64 total;
  pair64 run = block_exclusive_scan(sum, red, &total);
#pragma unroll
  for (int i = 0; i < DET_TOP_ITEMS; ++i) {
    if (base + i < nc) chunk_sums[base + i] = run;
    run += v[i];
  }
  if (threadIdx.x == 0) *total_out = total;
}

// block_sums -> exclusive prefixes in place, chunk by chunk, each chunk starting from its scanned chunk sum
__global__ __launch_bounds__(DET_THREADS) void k_det_scan_chunks(pair64* __restrict__ block_sums, int n,
                                                                 const pair64* __restrict__ chunk_offsets) {
  __shared__ pair64 red[DET_THREADS / 64];
  pair64 v[DET_ITEMS], sum = 0;
  const long base = (long)blockIdx.x * DET_CHUNK + threadIdx.x * DET_ITEMS;
#pragma unroll
  for (int i = 0; i < DET_ITEMS; ++i) {
    v[i] = base + i < n ? block_sums[base + i] : 0;
    sum += v[i];
  }
  pair64 total;
  pair64 run = chunk_offsets[blockIdx.x] + block_exclusive_scan(sum, red, &total);
#pragma unroll
  for (int i = 0; i < DET_ITEMS; ++i) {
    if (base + i < n) block_sums[base + i] = run;
    run += v[i];
  }
}

// group g ends at position p: group_end[g] = p + 1 (elements so far), group_tps[g] = positives so far
__global__ __launch_bounds__(DET_THREADS) void k_det_groups(const double* __restrict__ keys,
                                                            const uint8_t* __restrict__ labels, long T,
                                                            const pair64* __restrict__ block_offsets,
                                                            uint32_t* __restrict__ group_end,
                                                            uint32_t* __restrict__ group_tps) {
  __shared__ pair64 red[DET_THREADS / 64];
  const long p0 = (long)blockIdx.x * DET_BLOCK + threadIdx.x * DET_ITEMS;
  const uint32_t f = det_flags(keys, labels, T, p0, nullptr);
  pair64 total;
  const pair64 run = block_offsets[blockIdx.x] +
                     block_exclusive_scan(make_pair64(__popc(f & 0xffu), __popc(f >> 8)), red, &total);
  uint32_t tps = pair_lo(run), g = pair_hi(run);
#pragma unroll
  for (int i = 0; i < DET_ITEMS; ++i) {
    tps += (f >> i) & 1u;
    if (((f >> (8 + i)) & 1u) && g < (uint32_t)T) {   // (only positions < T carry the flag, so g < groups <= T)
      group_end[g] = (uint32_t)(p0 + i + 1);
      group_tps[g] = tps;
      ++g;
    }
  }
}

// roc_curve's drop_intermediate: with more than two groups, an inner group stays when its step towards the next
// group differs from the step that led to it (np.diff(fps, 2) | np.diff(tps, 2)); fps = elements - tps
__device__ __forceinline__ bool det_keep(const uint32_t* __restrict__ group_end,
                                         const uint32_t* __restrict__ group_tps, uint32_t g, uint32_t G) {
  if (G <= 2 || g == 0 || g + 1 == G) return true;
  const long t0 = group_tps[g - 1], t1 = group_tps[g], t2 = group_tps[g + 1];
  const long f0 = (long)group_end[g - 1] - t0, f1 = (long)group_end[g] - t1, f2 = (long)group_end[g + 1] - t2;
  return (t2 - t1 != t1 - t0) || (f2 - f1 != f1 - f0);
}

__device__ __forceinline__ uint32_t det_keep_flags(const DetHeader* __restrict__ head,
                                                   const uint32_t* __restrict__ group_end,
                                                   const uint32_t* __restrict__ group_tps, long T, long g0) {
  const uint32_t G = min(pair_hi(head->totals), (uint32_t)T);   // (there are at most T groups)
  uint32_t f = 0;
#pragma unroll
  for (int i = 0; i < DET_ITEMS; ++i)
    if (g0 + i < (long)G && det_keep(group_end, group_tps, (uint32_t)(g0 + i), G)) f |= 1u << i;
  return f;
}

// (the grid covers T groups, the most there can be; workgroups past the last group write a zero)
__global__ __launch_bounds__(DET_THREADS) void k_det_corner_counts(const DetHeader* __restrict__ head,
                                                                   const uint32_t* __restrict__ group_end,
                                                                   const uint32_t* __restrict__ group_tps, long T,
                                                                   pair64* __restrict__ block_sums) {
  __shared__ pair64 red[DET_THREADS / 64];
  const uint32_t f =
      det_keep_flags(head, group_end, group_tps, T, (long)blockIdx.x * DET_BLOCK + threadIdx.x * DET_ITEMS);
  pair64 total;
  block_exclusive_scan(make_pair64(__popc(f), 0), red, &total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// fpr = fps / fps[-1], fnr = 1 - tps / tps[-1], as numpy divides int64 arrays: both sides converted to float64
__device__ __forceinline__ void det_rates(uint32_t fps, uint32_t tps, uint32_t P, uint32_t N, double* fpr,
                                          double* fnr) {
  *fpr = (double)fps / (double)N;
  *fnr = 1.0 - (double)tps / (double)P;
}

// kept group number r (in order) becomes point 1 + r; point 0 is roc_curve's extra (0, 0) at threshold +inf.
// thr / fpr / fnr may be NULL together (a caller who wants the equal error rate alone).
__global__ __launch_bounds__(DET_THREADS) void k_det_compact(const double* __restrict__ keys, long T, int negate,
                                                             DetHeader* __restrict__ head,
                                                             const uint32_t* __restrict__ group_end,
                                                             const uint32_t* __restrict__ group_tps,
                                                             const pair64* __restrict__ block_offsets,
                                                             int32_t* __restrict__ out_fps,
                                                             int32_t* __restrict__ out_tps,
                                                             double* __restrict__ out_thr,
                                                             double* __restrict__ out_fpr,
                                                             double* __restrict__ out_fnr) {
  __shared__ pair64 red[DET_THREADS / 64];
  __shared__ uint32_t s_cross;
  if (threadIdx.x == 0) s_cross = 0xffffffffu;
  const uint32_t P = pair_lo(head->totals), N = (uint32_t)T - P;
  const long g0 = (long)blockIdx.x * DET_BLOCK + threadIdx.x * DET_ITEMS;
  const uint32_t f = det_keep_flags(head, group_end, group_tps, T, g0);
  pair64 total;
  uint32_t r = pair_lo(block_offsets[blockIdx.x] + block_exclusive_scan(make_pair64(__popc(f), 0), red, &total));
  uint32_t cross = 0xffffffffu;
  if (g0 == 0) {
    out_fps[0] = 0;
    out_tps[0] = 0;
    if (out_thr) {
      const double inf = __builtin_huge_val();
      out_thr[0] = negate ? -inf : inf;
      det_rates(0, 0, P, N, &out_fpr[0], &out_fnr[0]);
    }
  }
#pragma unroll
  for (int i = 0; i < DET_ITEMS; ++i) {
    if (!((f >> i) & 1u)) continue;
    const uint32_t end = group_end[g0 + i], tps = group_tps[g0 + i], fps = end - tps, at = 1 + r;
    if (at > (uint32_t)T || end < 1 || end > (uint32_t)T) continue;   // (cannot happen: the outputs hold T + 1 points)
    double fpr, fnr;
    det_rates(fps, tps, P, N, &fpr, &fnr);
    out_fps[at] = (int32_t)fps;
    out_tps[at] = (int32_t)tps;
    if (out_thr) {
      const double key = keys[T - end];        // the group's last element in descending order
      out_thr[at] = negate ? -key : key;
      out_fpr[at] = fpr;
      out_fnr[at] = fnr;
    }
    if (fpr > fnr) cross = min(cross, at);
    ++r;
  }
  __syncthreads();
  if (cross != 0xffffffffu) atomicMin(&s_cross, cross);
  __syncthreads();
  if (threadIdx.x == 0 && s_cross != 0xffffffffu) atomicMin(&head->first_cross, s_cross);
}

// status: [0] non-finite keys (already there), [1] P, [2] N, [3] points, [4] k (-1: no crossing), [5] the bits of
// eer (NaN without a crossing), [6] tie groups
__global__ void k_det_finish(const DetHeader* __restrict__ head, long T, const int32_t* __restrict__ out_fps,
                             const int32_t* __restrict__ out_tps, int64_t* __restrict__ status) {
  if (threadIdx.x || blockIdx.x) return;
  const uint32_t P = pair_lo(head->totals), N = (uint32_t)T - P, k = head->first_cross;
  const uint32_t points = 1 + pair_lo(head->kept);
  double eer = __builtin_nan("");
  const bool found = k >= 1 && k < points && k <= (uint32_t)T;
  if (found) {
    double fpr0, fnr0, fpr1, fnr1;
    det_rates((uint32_t)out_fps[k - 1], (uint32_t)out_tps[k - 1], P, N, &fpr0, &fnr0);
    det_rates((uint32_t)out_fps[k], (uint32_t)out_tps[k], P, N, &fpr1, &fnr1);
    eer = 0.25 * (((fpr0 + fpr1) + fnr0) + fnr1);
  }
  status[1] = P;
  status[2] = N;
  status[3] = points;
  status[4] = found ? (int64_t)k : -1;
  status[5] = __double_as_longlong(eer);
  status[6] = pair_hi(head->totals);
}

// one thread per trial: the whole dot product in dot2way's order
__global__ __launch_bounds__(128) void k_trial_cosine_f64(const double* __restrict__ E, int D,
                                                          const double* __restrict__ nrm,
                                                          const int32_t* __restrict__ idx1,
                                                          const int32_t* __restrict__ idx2, long T,
                                                          double* __restrict__ out) {
  const long t = (long)blockIdx.x * 128 + threadIdx.x;
  if (t >= T) return;
  const int i = idx1[t], j = idx2[t];
  out[t] = cosine_distance_f64(dot2way(E + (long)i * D, E + (long)j * D, D), nrm[i], nrm[j]);
}

// The workspace of pa_det_curve_f64 in 256-byte-aligned blocks
struct DetLayout {
  int nb, nc;
  DetHeader* head;
  pair64 *block_sums, *chunk_sums;   // (nb), (nc)
  uint32_t *group_end, *group_tps;   // (T) each
};
static DetLayout det_layout(Carver& c, long T) {
  DetLayout l;
  l.nb = cdiv(T, DET_BLOCK);
  l.nc = cdiv(l.nb, DET_CHUNK);
  l.head = c.take<DetHeader>(1);
  l.block_sums = c.take<pair64>(l.nb);
  l.chunk_sums = c.take<pair64>(l.nc);
  l.group_end = c.take<uint32_t>(T);
  l.group_tps = c.take<uint32_t>(T);
  return l;
}

// exclusive scan of ws.block_sums in place (launch 2 of the header comment); the grand total goes to *total_out
static void det_scan(const DetLayout& l, pair64* total_out, hipStream_t s) {
  hipLaunchKernelGGL(k_det_chunk_sums, dim3(l.nc), dim3(DET_THREADS), 0, s, l.block_sums, l.nb, l.chunk_sums);
  hipLaunchKernelGGL(k_det_scan_top, dim3(1), dim3(DET_THREADS), 0, s, l.chunk_sums, l.nc, total_out);
  hipLaunchKernelGGL(k_det_scan_chunks, dim3(l.nc), dim3(DET_THREADS), 0, s, l.block_sums, l.nb, l.chunk_sums);
}

}  // namespace pa

extern "C" {

int pa_trial_cosine_f64(const double* E, int N, int D, const int32_t* idx1, const int32_t* idx2, long T,
                        double* out, double* norms_scratch, void* stream) {
  PA_REQUIRE(N >= 1 && D >= 1, "pa_trial_cosine_f64: %d embeddings of dimension %d", N, D);
  PA_REQUIRE(T >= 0 && T <= pa::DET_MAX_T, "pa_trial_cosine_f64: %ld trials, 0..2^31-1 supported", T);
  PA_REQUIRE(E && norms_scratch && (T == 0 || (idx1 && idx2 && out)), "pa_trial_cosine_f64: null array");
  if (T == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  pa::ProfScope prof("k_trial_cosine_f64", stream, 2.0 * D * ((double)T + N),
                     8.0 * (double)N * D + 8.0 * N + 16.0 * (double)T);
  pa_row_norms_f64(E, N, D, norms_scratch, stream);
  hipLaunchKernelGGL(pa::k_trial_cosine_f64, dim3(pa::cdiv(T, 128)), dim3(128), 0, s, E, D, norms_scratch, idx1,
                     idx2, T, out);
  PA_CHECK_LAUNCH("pa_trial_cosine_f64");
  return 0;
}

int pa_det_block_elements(void) { return pa::DET_BLOCK; }
int pa_det_scan_chunk(void) { return pa::DET_CHUNK; }

size_t pa_det_workspace_bytes(long T) {
  if (T < 1 || T > pa::DET_MAX_T) return 0;
  return pa::carved_bytes([&](pa::Carver& c) { pa::det_layout(c, T); });
}

int pa_det_curve_f64(const double* sorted_keys, const uint8_t* labels, long T, int negate, int32_t* fps,
                     int32_t* tps, double* thresholds, double* fpr, double* fnr, int64_t* status, void* workspace,
                     size_t workspace_bytes, void* stream) {
  PA_REQUIRE(T >= 1 && T <= pa::DET_MAX_T, "pa_det_curve_f64: %ld scores, 1..2^31-1 supported", T);
  PA_REQUIRE(sorted_keys && labels && fps && tps && status && workspace, "pa_det_curve_f64: null array");
  PA_REQUIRE((thresholds != nullptr) == (fpr != nullptr) && (fpr != nullptr) == (fnr != nullptr),
             "pa_det_curve_f64: thresholds, fpr and fnr are given together or not at all");
  pa::Carver carver(workspace);
  const pa::DetLayout l = pa::det_layout(carver, T);
  PA_REQUIRE(workspace_bytes >= carver.bytes(), "pa_det_curve_f64: workspace of %zu bytes, %zu needed",
             workspace_bytes, carver.bytes());
  hipStream_t s = (hipStream_t)stream;
  pa::DetHeader* head = l.head;
  // header: counts 0, first_cross (and its padding) all ones; status: all 0
  if (pa::fill_async(head, 0, offsetof(pa::DetHeader, first_cross), s) != hipSuccess ||
      pa::fill_async(&head->first_cross, 0xff, 8, s) != hipSuccess ||
      pa::fill_async(status, 0, sizeof(int64_t) * 8, s) != hipSuccess) {
    pa::set_error("pa_det_curve_f64: the fill launch failed");
    return 1;
  }
  pa::ProfScope prof("k_det_curve_f64", stream, 0.0, 2.0 * 9.0 * (double)T + 16.0 * (double)T);
  const dim3 grid(l.nb), block(pa::DET_THREADS);
  hipLaunchKernelGGL(pa::k_det_block_counts, grid, block, 0, s, sorted_keys, labels, T, l.block_sums,
                     (unsigned long long*)status);
  pa::det_scan(l, &head->totals, s);
  hipLaunchKernelGGL(pa::k_det_groups, grid, block, 0, s, sorted_keys, labels, T, l.block_sums, l.group_end,
                     l.group_tps);
  hipLaunchKernelGGL(pa::k_det_corner_counts, grid, block, 0, s, head, l.group_end, l.group_tps, T, l.block_sums);
  pa::det_scan(l, &head->kept, s);
  hipLaunchKernelGGL(pa::k_det_compact, grid, block, 0, s, sorted_keys, T, negate, head, l.group_end, l.group_tps,
                     l.block_sums, fps, tps, thresholds, fpr, fnr);
  hipLaunchKernelGGL(pa::k_det_finish, dim3(1), dim3(64), 0, s, head, T, fps, tps, status);
  PA_CHECK_LAUNCH("pa_det_curve_f64");
  return 0;
}

}  // extern "C"
