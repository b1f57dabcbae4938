// Open-set speaker identification against an enrolled gallery (identification.py): cosine
// distances of query rows to cohort / gallery rows in float64 with the bits of scipy.spatial.distance.cdist(.,
// "cosine") (cosine_f64.h), and on top of them
//   pa_cohort_stats_f64    mean and standard deviation of the K smallest distances of every row to a cohort (the two
//                          statistics of adaptive S-norm), added in ascending order, every operation rounded on its own;
//   pa_gallery_topk_f64    the k smallest (optionally normalised) values of every query over the gallery, with their
//                          indices, ascending, ties to the lower index (np.argsort(kind="stable")[:k]);
//   pa_gallery_pairs_f64   the same value for a list of (query, gallery) pairs.
//
// SELECTION (the first two).  The (M, N) matrix is never written: a workgroup owns ID_ROWS query rows (one wave each in
// the merge) and walks the other table in tiles of ID_TILE rows.  The table is first copied TRANSPOSED into the workspace
// (k_transpose_f64: Ct[k][j] = C[j][k]), so that the lanes of a wave, which own consecutive rows j, read consecutive
// doubles at every k; read row-major, every lane would pull a line of its own.  Per tile, thread t computes the values of
// row tile * ID_TILE + t against the ID_ROWS queries -- the whole dot product in dot2way's order -- and keeps a value only if
// it beats the query's current K-th best; the survivors (few, once the list has settled) are merged into the sorted
// list of the K best by RANK: an element's place is the number of elements before it in the total order below, found
// by a binary search in the list plus a scan of the survivors.  Ranks do not depend on the order in which the
// survivors were appended, so the LDS atomic that appends them does not reach the result.
// ORDER.  (value, index) pairs, compared as np.sort / np.argsort(kind="stable") compare: by value, -0.0 equal to 0.0,
// NaN after everything else; equal values (and NaNs among themselves) by index.  The list starts as K sentinels
// (NaN, INT_MAX), which every real pair beats.
// Every loop has a bound known on entry: tiles = ceil(N / ID_TILE), at most ID_TILE survivors, a binary search of
// ID_SEARCH_STEPS steps, K additions.  No allocation, no synchronisation, no floating-point atomics.
// hipcc-flags: -ffp-contract=off
#include <cstddef>

#include "common.h"
#include "cosine_f64.h"
#include "pyannote_amd.h"

namespace pa {

constexpr int ID_THREADS = 256;
constexpr int ID_TILE = ID_THREADS;          // table rows per tile: one per thread
constexpr int ID_ROWS = ID_THREADS / 64;     // query rows per workgroup: one per wave in the merge
constexpr int ID_MAX_TOP = 512;              // largest K of pa_cohort_stats_f64
constexpr int ID_MAX_K = 64;                 // largest k of pa_gallery_topk_f64
constexpr int ID_SEARCH_STEPS = 10;          // lower bound in a list of up to 512: the interval is empty after 10 halvings
constexpr int ID_MAX_ROWS = 1 << 30;         // rows of either table (indices stay below the sentinel's INT_MAX)
static_assert((1 << (ID_SEARCH_STEPS - 1)) >= ID_MAX_TOP, "the binary search ends within its steps");
static_assert(ID_MAX_K <= ID_MAX_TOP, "one search depth for both lists");

// leading dimension of the transposed table: N rounded up to whole 256-byte lines
static inline long transposed_ld(int N) { return ((long)N + 31) & ~31L; }

// Ct[k * ldt + j] = C[j * D + k] through a 32 x 32 LDS tile (one padding column): both sides in whole lines.
// grid = (ceil(N / 32), ceil(D / 32)), block = 256 (32 x 8).  Columns j >= N of Ct are not written and never read.
__global__ __launch_bounds__(ID_THREADS) void k_transpose_f64(const double* __restrict__ C, int N, int D, long ldt,
                                                              double* __restrict__ Ct) {
  __shared__ double tile[32][33];
  const int j0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const long j = j0 + r;
    const int k = k0 + tx;
    if (j < N && k < D) tile[r][tx] = C[j * D + k];
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int k = k0 + r;
    const long j = j0 + tx;
    if (j < N && k < D) Ct[(long)k * ldt + j] = tile[tx][r];
  }
}

// np.sort's order of float64 as an unsigned key: -0.0 and 0.0 share a key, every NaN takes the largest one
__device__ __forceinline__ unsigned long long order_key(double v) {
  if (v != v) return ~0ull;
  if (v == 0.0) v = 0.0;
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ bool pair_less(unsigned long long ka, int ia, unsigned long long kb, int ib) {
  return ka < kb || (ka == kb && ia < ib);
}

// the value of pair (query, j): the distance, or its symmetric normalisation by the two sides' cohort statistics
__device__ __forceinline__ double pair_value(double d, bool normalise, double qm, double qs, double gm, double gs) {
  if (!normalise) return d;
  const double a = (d - qm) / qs;
  const double b = (d - gm) / gs;
  return 0.5 * (a + b);
}

// TOPK false: pa_cohort_stats_f64 (out_a = mean, out_b = std, out_i = status); true: pa_gallery_topk_f64 (out_a =
// values (M, K), out_i = indices (M, K), out_b unused).  Ct: the second table transposed, (D, ldt).
// 1 <= K <= min(N, MAXTOP).  grid = ceil(M / ID_ROWS).
template <int MAXTOP, bool TOPK>
__global__ __launch_bounds__(ID_THREADS) void k_select(const double* __restrict__ X, int M,
                                                       const double* __restrict__ Ct, long ldt, int N, int D,
                                                       const double* __restrict__ nx, const double* __restrict__ nc,
                                                       int K, const double* __restrict__ q_mean,
                                                       const double* __restrict__ q_std,
                                                       const double* __restrict__ g_mean,
                                                       const double* __restrict__ g_std, double* __restrict__ out_a,
                                                       double* __restrict__ out_b, int32_t* __restrict__ out_i) {
  constexpr int ELEMS = (MAXTOP + ID_TILE) / 64;   // list and survivors of one query, per lane of its wave
  __shared__ double l_v[ID_ROWS][MAXTOP];
  __shared__ int l_i[ID_ROWS][MAXTOP];
  __shared__ double s_v[ID_ROWS][ID_TILE];
  __shared__ int s_i[ID_ROWS][ID_TILE];
  __shared__ int s_n[ID_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long row0 = (long)blockIdx.x * ID_ROWS;

  for (int e = tid; e < ID_ROWS * MAXTOP; e += ID_THREADS) {
    (&l_v[0][0])[e] = __builtin_nan("");
    (&l_i[0][0])[e] = 0x7fffffff;
  }
  // rows past the last one repeat it and write nothing
  const double* xq[ID_ROWS];
  double nq[ID_ROWS], qm[ID_ROWS], qs[ID_ROWS];
  const bool normalise = TOPK && q_mean != nullptr;
#pragma unroll
  for (int q = 0; q < ID_ROWS; ++q) {
    const long r = row0 + q < M ? row0 + q : (long)M - 1;
    xq[q] = X + r * D;
    nq[q] = nx[r];
    qm[q] = normalise ? q_mean[r] : 0.0;
    qs[q] = normalise ? q_std[r] : 1.0;
  }

  const int tiles = (N + ID_TILE - 1) / ID_TILE;
  for (int t = 0; t < tiles; ++t) {
    if (tid < ID_ROWS) s_n[tid] = 0;
    __syncthreads();   // (the list of the tile before is complete as well)
    const long j = (long)t * ID_TILE + tid;
    if (j < N) {
      const double* __restrict__ c = Ct + j;   // element k of row j at c[k * ldt]
      double s0[ID_ROWS], s1[ID_ROWS];
#pragma unroll
      for (int q = 0; q < ID_ROWS; ++q) s0[q] = s1[q] = 0.0;
      const int m = D & ~1;
#pragma unroll 4
      for (int k = 0; k < m; k += 2) {   // dot2way (cosine_f64.h) for ID_ROWS rows at once
        const double c0 = c[(long)k * ldt], c1 = c[(long)(k + 1) * ldt];
#pragma unroll
        for (int q = 0; q < ID_ROWS; ++q) {
          s0[q] = s0[q] + xq[q][k] * c0;
          s1[q] = s1[q] + xq[q][k + 1] * c1;
        }
      }
      const double ncj = nc[j];
      const double gm = normalise ? g_mean[j] : 0.0, gs = normalise ? g_std[j] : 1.0;
#pragma unroll
      for (int q = 0; q < ID_ROWS; ++q) {
        double dot = s0[q] + s1[q];
        if (D & 1) dot = dot + xq[q][D - 1] * c[(long)(D - 1) * ldt];
        const double v = pair_value(cosine_distance_f64(dot, nq[q], ncj), normalise, qm[q], qs[q], gm, gs);
        if (pair_less(order_key(v), (int)j, order_key(l_v[q][K - 1]), l_i[q][K - 1])) {
          const int p = atomicAdd(&s_n[q], 1);   // (p < ID_TILE: one append per thread and query)
          s_v[q][p] = v;
          s_i[q][p] = (int)j;
        }
      }
    }
    __syncthreads();
    // wave w merges the survivors of query w into its list: ranks first, from the old list, then the writes
    const int s = s_n[w];
    double ev[ELEMS];
    int ei[ELEMS], er[ELEMS];
#pragma unroll
    for (int u = 0; u < ELEMS; ++u) {
      const int e = lane + 64 * u;
      er[u] = 0x7fffffff;
      if (s > 0 && e < K + s) {
        int rank;
        if (e < K) {
          ev[u] = l_v[w][e];
          ei[u] = l_i[w][e];
          rank = e;
        } else {
          ev[u] = s_v[w][e - K];
          ei[u] = s_i[w][e - K];
          const unsigned long long key = order_key(ev[u]);
          int lo = 0, hi = K;
          for (int it = 0; it < ID_SEARCH_STEPS; ++it) {
            if (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (pair_less(order_key(l_v[w][mid]), l_i[w][mid], key, ei[u])) lo = mid + 1;
              else hi = mid;
            }
          }
          rank = lo;
        }
        const unsigned long long key = order_key(ev[u]);
        for (int p = 0; p < s; ++p) rank += pair_less(order_key(s_v[w][p]), s_i[w][p], key, ei[u]) ? 1 : 0;
        er[u] = rank;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < ELEMS; ++u) {
      if (er[u] < K) {
        l_v[w][er[u]] = ev[u];
        l_i[w][er[u]] = ei[u];
      }
    }
  }
  __syncthreads();

  const long row = row0 + w;
  if (row >= M) return;
  if (TOPK) {
    for (int e = lane; e < K; e += 64) {
      out_a[row * K + e] = l_v[w][e];
      out_i[row * K + e] = l_i[w][e];
    }
  } else if (lane == 0) {
    // np.cumsum(s)[-1] / K and sqrt(np.cumsum((s - mean) * (s - mean))[-1] / K): left to right from the first element
    const double na = nq[w];
    const bool bad = !(na > 0.0 && na <= 1.7976931348623157e308);
    double mean = __builtin_nan(""), sd = __builtin_nan("");
    if (!bad) {
      double acc = l_v[w][0];
      for (int e = 1; e < K; ++e) acc = acc + l_v[w][e];
      mean = acc / (double)K;
      const double d0 = l_v[w][0] - mean;
      double acc2 = d0 * d0;
      for (int e = 1; e < K; ++e) {
        const double de = l_v[w][e] - mean;
        acc2 = acc2 + de * de;
      }
      sd = __dsqrt_rn(acc2 / (double)K);
    }
    out_a[row] = mean;
    out_b[row] = sd;
    out_i[row] = bad ? 1 : 0;
  }
}

// one thread per pair: the two norms and the whole dot product in dot2way's order, so a handful of pairs costs a
// handful of rows and no workspace; an index outside its table gives NaN
__global__ __launch_bounds__(128) void k_gallery_pairs_f64(const double* __restrict__ Q, int M,
                                                           const double* __restrict__ G, int Ng, int D,
                                                           const double* __restrict__ q_mean,
                                                           const double* __restrict__ q_std,
                                                           const double* __restrict__ g_mean,
                                                           const double* __restrict__ g_std,
                                                           const int32_t* __restrict__ iq,
                                                           const int32_t* __restrict__ ig, long P,
                                                           double* __restrict__ out) {
  const long t = (long)blockIdx.x * 128 + threadIdx.x;
  if (t >= P) return;
  const int i = iq[t], j = ig[t];
  if (i < 0 || i >= M || j < 0 || j >= Ng) {
    out[t] = __builtin_nan("");
    return;
  }
  const double *q = Q + (long)i * D, *g = G + (long)j * D;
  const double d = cosine_distance_f64(dot2way(q, g, D), row_norm_f64(q, D), row_norm_f64(g, D));
  const bool normalise = q_mean != nullptr;
  out[t] = pair_value(d, normalise, normalise ? q_mean[i] : 0.0, normalise ? q_std[i] : 1.0,
                      normalise ? g_mean[j] : 0.0, normalise ? g_std[j] : 1.0);
}

// The workspace of the two selecting entry points: the row norms of both tables and the transposed copy of the second
struct IdentifyLayout {
  double *na, *nb;   // (M), (N)
  long ldt;
  double* Ct;        // (D, ldt)
};
static IdentifyLayout identify_layout(Carver& c, int M, int N, int D) {
  IdentifyLayout l;
  l.na = c.take<double>(M);
  l.nb = c.take<double>(N);
  l.ldt = transposed_ld(N);
  l.Ct = c.take<double>((size_t)D * l.ldt);
  return l;
}
static void transpose_table(const double* C, int N, int D, const IdentifyLayout& l, hipStream_t s) {
  hipLaunchKernelGGL(k_transpose_f64, dim3(cdiv(N, 32), cdiv(D, 32)), dim3(ID_THREADS), 0, s, C, N, D, l.ldt, l.Ct);
}
static bool identify_sizes_ok(int M, int N, int D) {
  return M >= 1 && N >= 1 && M <= ID_MAX_ROWS && N <= ID_MAX_ROWS && D >= 1 && D <= (1 << 20);
}

}  // namespace pa

extern "C" {

int pa_identify_tile(void) { return pa::ID_TILE; }
int pa_identify_max_top(void) { return pa::ID_MAX_TOP; }
int pa_identify_max_k(void) { return pa::ID_MAX_K; }

size_t pa_cohort_stats_workspace_bytes(int M, int N, int D) {
  if (!pa::identify_sizes_ok(M, N, D)) return 0;
  return pa::carved_bytes([&](pa::Carver& c) { pa::identify_layout(c, M, N, D); });
}

int pa_cohort_stats_f64(const double* X, int M, const double* C, int N, int D, int K, double* mean, double* stdev,
                        int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  PA_REQUIRE(pa::identify_sizes_ok(M, N, D), "pa_cohort_stats_f64: %d rows against %d cohort rows of dimension %d", M,
             N, D);
  PA_REQUIRE(K >= 1 && K <= N && K <= pa::ID_MAX_TOP,
             "pa_cohort_stats_f64: K = %d, 1..min(%d cohort rows, %d) supported", K, N, pa::ID_MAX_TOP);
  PA_REQUIRE(X && C && mean && stdev && status && workspace, "pa_cohort_stats_f64: null array");
  pa::Carver carver(workspace);
  const pa::IdentifyLayout l = pa::identify_layout(carver, M, N, D);
  PA_REQUIRE(workspace_bytes >= carver.bytes(), "pa_cohort_stats_f64: workspace of %zu bytes, %zu needed",
             workspace_bytes, carver.bytes());
  pa::ProfScope prof("k_cohort_stats_f64", stream, 2.0 * D * (double)M * N, 8.0 * ((double)M + N) * D + 20.0 * M);
  pa_row_norms_f64(X, M, D, l.na, stream);
  pa_row_norms_f64(C, N, D, l.nb, stream);
  pa::transpose_table(C, N, D, l, (hipStream_t)stream);
  hipLaunchKernelGGL((pa::k_select<pa::ID_MAX_TOP, false>), dim3(pa::cdiv(M, pa::ID_ROWS)), dim3(pa::ID_THREADS), 0,
                     (hipStream_t)stream, X, M, l.Ct, l.ldt, N, D, l.na, l.nb, K, nullptr, nullptr, nullptr, nullptr, mean,
                     stdev, status);
  PA_CHECK_LAUNCH("pa_cohort_stats_f64");
  return 0;
}

size_t pa_gallery_workspace_bytes(int M, int Ng, int D) {
  if (!pa::identify_sizes_ok(M, Ng, D)) return 0;
  return pa::carved_bytes([&](pa::Carver& c) { pa::identify_layout(c, M, Ng, D); });
}

int pa_gallery_topk_f64(const double* Q, int M, const double* G, int Ng, int D, const double* q_mean,
                        const double* q_std, const double* g_mean, const double* g_std, int k, double* values,
                        int32_t* indices, void* workspace, size_t workspace_bytes, void* stream) {
  PA_REQUIRE(pa::identify_sizes_ok(M, Ng, D), "pa_gallery_topk_f64: %d queries against %d gallery rows of dimension %d",
             M, Ng, D);
  PA_REQUIRE(k >= 1 && k <= Ng && k <= pa::ID_MAX_K, "pa_gallery_topk_f64: k = %d, 1..min(%d gallery rows, %d) supported",
             k, Ng, pa::ID_MAX_K);
  PA_REQUIRE(Q && G && values && indices && workspace, "pa_gallery_topk_f64: null array");
  const int given = (q_mean != nullptr) + (q_std != nullptr) + (g_mean != nullptr) + (g_std != nullptr);
  PA_REQUIRE(given == 0 || given == 4, "pa_gallery_topk_f64: the four statistics are given together or not at all");
  pa::Carver carver(workspace);
  const pa::IdentifyLayout l = pa::identify_layout(carver, M, Ng, D);
  PA_REQUIRE(workspace_bytes >= carver.bytes(), "pa_gallery_topk_f64: workspace of %zu bytes, %zu needed",
             workspace_bytes, carver.bytes());
  pa::ProfScope prof("k_gallery_topk_f64", stream, 2.0 * D * (double)M * Ng, 8.0 * ((double)M + Ng) * D + 12.0 * M * k);
  pa_row_norms_f64(Q, M, D, l.na, stream);
  pa_row_norms_f64(G, Ng, D, l.nb, stream);
  pa::transpose_table(G, Ng, D, l, (hipStream_t)stream);
  hipLaunchKernelGGL((pa::k_select<pa::ID_MAX_K, true>), dim3(pa::cdiv(M, pa::ID_ROWS)), dim3(pa::ID_THREADS), 0,
                     (hipStream_t)stream, Q, M, l.Ct, l.ldt, Ng, D, l.na, l.nb, k, q_mean, q_std, g_mean, g_std, values,
                     nullptr, indices);
  PA_CHECK_LAUNCH("pa_gallery_topk_f64");
  return 0;
}

int pa_gallery_pairs_f64(const double* Q, int M, const double* G, int Ng, int D, const double* q_mean,
                         const double* q_std, const double* g_mean, const double* g_std, const int32_t* iq,
                         const int32_t* ig, long P, double* out, void* stream) {
  PA_REQUIRE(pa::identify_sizes_ok(M, Ng, D), "pa_gallery_pairs_f64: %d queries against %d gallery rows of dimension %d",
             M, Ng, D);
  PA_REQUIRE(P >= 0 && P <= 0x7fffffffL, "pa_gallery_pairs_f64: %ld pairs, 0..2^31-1 supported", P);
  PA_REQUIRE(Q && G && (P == 0 || (iq && ig && out)), "pa_gallery_pairs_f64: null array");
  const int given = (q_mean != nullptr) + (q_std != nullptr) + (g_mean != nullptr) + (g_std != nullptr);
  PA_REQUIRE(given == 0 || given == 4, "pa_gallery_pairs_f64: the four statistics are given together or not at all");
  if (P == 0) return 0;
  pa::ProfScope prof("k_gallery_pairs_f64", stream, 6.0 * D * (double)P, 16.0 * D * (double)P + 16.0 * (double)P);
  hipLaunchKernelGGL(pa::k_gallery_pairs_f64, dim3(pa::cdiv(P, 128)), dim3(128), 0, (hipStream_t)stream, Q, M, G, Ng, D,
                     q_mean, q_std, g_mean, g_std, iq, ig, P, out);
  PA_CHECK_LAUNCH("pa_gallery_pairs_f64");
  return 0;
}

}  // extern "C"
