// Single, complete, average, weighted and Ward linkage on gfx950, bit-identical to
// scipy.cluster.hierarchy.linkage(y, method) (SciPy 1.15.3 `_hierarchy.nn_chain` and `_hierarchy.mst_single_linkage`),
// which AgglomerativeClustering.cluster calls for these values of its `method` hyper-parameter (reference:
// pipelines/clustering.py:292-480) -- plus the cosine pdist that feeds them (pa_pdist_cosine_f64) and the finite check
// SciPy's linkage makes on its input (pa_nonfinite_flag_f64).
//
// Why a kernel: both algorithms are N-1 dependent merges with O(N) independent work per step -- a row scan for the
// nearest neighbour, a Lance-Williams update of one row and column -- that SciPy walks on one host core after the
// whole condensed matrix crossed PCIe.  Here the matrix stays in HBM: a SQUARE SYMMETRIC copy (8 n ld bytes in the
// workspace, built by pa_square_from_condensed of cluster.hip) makes the scan of row x and the update of row y
// contiguous; in condensed layout the i < x half of a row is a stride-n gather.
//
// ONE persistent 1024-thread workgroup (a multi-workgroup form is out of scope), __syncthreads between phases, no
// grid barrier and no spinning on memory.  Two kernels:
//   * k_lc_nn_chain<METHOD, LDS_STATE>: the nearest-neighbour chain.  Every chain step is one arg-min over row x
//     (wave shuffles, then 16 LDS slots, double-buffered: ONE barrier per step); a merge is two barriers more.
//   * k_lc_mst_single<LDS_STATE>: Prim's order; the Dmin update is fused with the arg-min; one barrier per merge.
// LDS_STATE: size[] and the chain live in LDS (8 n bytes: up to 20 352 points; single linkage keeps size[] alone
// there, 4 n bytes: up to 40 704), else in the workspace.
//
// Exactness contract (tests/test_linkage_methods_gpu.py): the kernels emit SciPy's UNSORTED merge list (x, y,
// height, size); the stable sort by height and the union-find relabelling are distance.linkage_finish on the host.
//   * the update is SciPy's expression, evaluated left to right in double, every operation rounded on its own
//     (lc_update; this file is compiled with -ffp-contract=off);
//   * a row scan returns the SMALLEST index attaining the minimum (SciPy scans ascending with a strict `<`) and
//     replaces the seeded previous chain element only on a strictly smaller value;
//   * NaN never wins a comparison, as in SciPy (the Python side refuses non-finite matrices before the launch).
// Every loop is bounded by the algorithm: a chain never holds more than n entries and all merges together push at
// most 3 n; beyond either bound -- or when a scan finds no neighbour -- the kernel stores an error word (first int
// of the workspace) and ends.
// hipcc-flags: -ffp-contract=off
#include <stdlib.h>

#include "common.h"
#include "cosine_f64.h"
#include "pyannote_amd.h"

namespace pa {

constexpr int LC_T = 1024;  // threads (16 waves)
constexpr int LC_W = LC_T / 64;
constexpr int LC_U = 8;  // row elements per thread in flight (one audio-hour = 7 176 points = ONE trip)

enum { LC_OK = 0, LC_ERR_CHAIN = 1, LC_ERR_NO_NEIGHBOUR = 2 };

// first minimum over the workgroup, valid in every thread.  `red`: LC_W slots nobody else touches until the next
// barrier but one (the callers alternate between two sets).  ONE barrier.
__device__ __forceinline__ MinPair lc_block_min(MinPair best, MinPair* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    MinPair other;
    other.d = __shfl_xor(best.d, o, 64);
    other.i = __shfl_xor(best.i, o, 64);
    best = min_pair(best, other);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
  __syncthreads();
  MinPair r = red[0];
#pragma unroll
  for (int q = 1; q < LC_W; ++q) r = min_pair(r, red[q]);
  return r;
}

// SciPy's Lance-Williams updates (_hierarchy_distance_update.pxi): a = d(i, x), b = d(i, y), c = d(x, y).
// THE OPERATION ORDER IS THE CONTRACT: left to right in double, every operation rounded on its own.
template <int METHOD>
__device__ __forceinline__ double lc_update(double a, double b, double c, int nx, int ny, int ni) {
  if (METHOD == PA_LINKAGE_COMPLETE) return a > b ? a : b;
  if (METHOD == PA_LINKAGE_AVERAGE) return (nx * a + ny * b) / (nx + ny);
  if (METHOD == PA_LINKAGE_WEIGHTED) return 0.5 * (a + b);
  const double t = 1.0 / (nx + ny + ni);  // PA_LINKAGE_WARD
  return sqrt((ni + nx) * t * a * a + (ni + ny) * t * b * b - ni * t * c * c);
}

// nn_chain(D, n, method): raw[k] = (x, y, height, size) for k = 0 .. n-2, x < y cluster SLOTS (not ids).
template <int METHOD, bool LDS_STATE>
__global__ __launch_bounds__(LC_T) void k_lc_nn_chain(double* __restrict__ S, int n, long ld, double* __restrict__ raw,
                                                       int* __restrict__ g_size, int* __restrict__ g_chain,
                                                       int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lc_smem[];
  __shared__ MinPair red[2][LC_W];
  int* const size = LDS_STATE ? reinterpret_cast<int*>(lc_smem) : g_size;
  int* const chain = LDS_STATE ? size + n : g_chain;
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += LC_T) size[i] = 1;
  __syncthreads();

  // uniform in every thread: the chain length, its two top entries, the first slot that may still be active
  int len = 0, x = -1, prev = -1, first = 0, step = 0;
  long pushes = 0;
  for (int k = 0; k < n - 1; ++k) {
    if (len == 0) {
      while (first < n && size[first] == 0) ++first;  // (amortised: `first` only grows, n steps in total)
      if (first >= n) {
        if (tid == 0) *status = LC_ERR_NO_NEIGHBOUR;
        return;
      }
      if (tid == 0) chain[0] = first;
      len = 1;
      x = first;
      prev = -1;
    }
    double cur;
    int y;
    for (;;) {
      // ---- nearest active neighbour of x; the previous chain element is preferred on equal distance
      const double* row = S + (long)x * ld;
      MinPair best{__builtin_inf(), -1};
      for (int i0 = tid; i0 < n; i0 += LC_U * LC_T) {
        double d[LC_U];
        bool act[LC_U];
#pragma unroll
        for (int u = 0; u < LC_U; ++u) {
          const int i = i0 + u * LC_T;
          act[u] = i < n && i != x && size[i] != 0;
          d[u] = i < n ? row[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < LC_U; ++u)  // ascending i per thread, strict `<`: the first minimum
          if (act[u] && d[u] < best.d) {
            best.d = d[u];
            best.i = i0 + u * LC_T;
          }
      }
      const double seed = len > 1 ? row[prev] : __builtin_inf();
      best = lc_block_min(best, red[step & 1]);
      ++step;
      cur = seed;
      y = len > 1 ? prev : -1;
      if (best.i >= 0 && best.d < cur) {
        cur = best.d;
        y = best.i;
      }
      if (len > 1 && y == prev) break;
      // ---- push y; the bounds below follow from the algorithm, a violation is a logic error
      ++pushes;
      if (y < 0 || len >= n || pushes > 3L * n + 8) {
        if (tid == 0) *status = y < 0 ? LC_ERR_NO_NEIGHBOUR : LC_ERR_CHAIN;
        return;
      }
      if (tid == 0) chain[len] = y;
      ++len;
      prev = x;
      x = y;
    }
    // ---- merge the mutual nearest neighbours x and y (= prev) at height cur
    len -= 2;
    if (x > y) {
      const int t = x;
      x = y;
      y = t;
    }
    const int nx = size[x], ny = size[y];
    __syncthreads();  // every thread holds nx, ny (and is done with the scan's size[]) before lane 0 changes them
    if (tid == 0) {
      raw[4 * (long)k + 0] = (double)x;
      raw[4 * (long)k + 1] = (double)y;
      raw[4 * (long)k + 2] = cur;
      raw[4 * (long)k + 3] = (double)(nx + ny);
      size[x] = 0;
      size[y] = nx + ny;
    }
    // ---- D[i, y] = f(D[i, x], D[i, y], ...) for every active i: rows x and y are contiguous, the mirror D[y, i] ->
    // D[i, y] is one store per i.  (i == x and i == y are skipped by index: size[x], size[y] are in flight.)
    const double* rx = S + (long)x * ld;
    double* ry = S + (long)y * ld;
    for (int i0 = tid; i0 < n; i0 += LC_U * LC_T) {
      double a[LC_U], b[LC_U];
      int ni[LC_U];
#pragma unroll
      for (int u = 0; u < LC_U; ++u) {
        const int i = i0 + u * LC_T;
        ni[u] = (i < n && i != x && i != y) ? size[i] : 0;
        a[u] = i < n ? rx[i] : 0.0;
        b[u] = i < n ? ry[i] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < LC_U; ++u) {
        if (ni[u] == 0) continue;
        const int i = i0 + u * LC_T;
        const double v = lc_update<METHOD>(a[u], b[u], cur, nx, ny, ni[u]);
        ry[i] = v;
        S[(long)i * ld + y] = v;
      }
    }
    __syncthreads();  // the new row / column y and the sizes are visible to the next scan
    if (len > 0) {
      x = chain[len - 1];
      prev = len > 1 ? chain[len - 2] : -1;
    }
  }
  if (tid == 0) *status = LC_OK;
}

// mst_single_linkage(dists, n): raw[k] = (x, y, height, 0).  Thread t owns the slots t, t + 1024, ...: their
// `merged` flags (size[] == 0) and Dmin entries are read and written by their owner only.
template <bool LDS_STATE>
__global__ __launch_bounds__(LC_T) void k_lc_mst_single(const double* __restrict__ S, int n, long ld,
                                                         double* __restrict__ raw, int* __restrict__ g_size,
                                                         double* __restrict__ dmin, int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lc_smem[];
  __shared__ MinPair red[2][LC_W];
  int* const size = LDS_STATE ? reinterpret_cast<int*>(lc_smem) : g_size;
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += LC_T) {
    size[i] = 1;
    dmin[i] = __builtin_inf();
  }
  int x = 0;
  for (int k = 0; k < n - 1; ++k) {
    if ((x & (LC_T - 1)) == tid) size[x] = 0;  // merged[x] = 1, by its owner
    const double* row = S + (long)x * ld;
    MinPair best{__builtin_inf(), -1};
    for (int i0 = tid; i0 < n; i0 += LC_U * LC_T) {
      double d[LC_U], m[LC_U];
      bool act[LC_U];
#pragma unroll
      for (int u = 0; u < LC_U; ++u) {
        const int i = i0 + u * LC_T;
        act[u] = i < n && size[i] != 0;
        d[u] = i < n ? row[i] : 0.0;
        m[u] = i < n ? dmin[i] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < LC_U; ++u) {
        if (!act[u]) continue;
        const int i = i0 + u * LC_T;
        if (m[u] > d[u]) {
          m[u] = d[u];
          dmin[i] = d[u];
        }
        if (m[u] < best.d) {
          best.d = m[u];
          best.i = i;
        }
      }
    }
    best = lc_block_min(best, red[k & 1]);
    if (best.i < 0) {
      if (tid == 0) *status = LC_ERR_NO_NEIGHBOUR;
      return;
    }
    if (tid == 0) {
      raw[4 * (long)k + 0] = (double)x;
      raw[4 * (long)k + 1] = (double)best.i;
      raw[4 * (long)k + 2] = best.d;
      raw[4 * (long)k + 3] = 0.0;
    }
    x = best.i;
  }
  if (tid == 0) *status = LC_OK;
}

// *flag = 1 when any of the `count` doubles is NaN or infinite (the caller zeroes it); grid-stride
__global__ __launch_bounds__(256) void k_lc_nonfinite(const double* __restrict__ v, long count, int* __restrict__ flag) {
  bool bad = false;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256)
    bad |= !(fabs(v[i]) < __builtin_inf());
  if (__any(bad) && (threadIdx.x & 63) == 0) *flag = 1;  // (racing writers all store 1)
}

constexpr int LC_PT = 64;  // pairs tile edge
constexpr int LC_PK = 32;  // k chunk (even: the parity of k survives the chunking)
constexpr int LC_PLD = LC_PK + 1;

// pdist(X, "cosine"): the tiling of k_pdist_f64 (cluster.hip) with dot2way's summation order per pair -- even and odd
// k in two accumulators, ascending, their sum, then the odd tail element -- and cosine_distance_f64 on top.
// grid = (ceil(N/64), ceil(N/64)), upper tiles only; block = 256, 4 x 4 pairs per thread.
__global__ __launch_bounds__(256) void k_lc_pdist_cosine(const double* __restrict__ X, int N, int D,
                                                          const double* __restrict__ nrm, double* __restrict__ out) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  __shared__ double As[LC_PT * LC_PLD];
  __shared__ double Bs[LC_PT * LC_PLD];
  const int tid = threadIdx.x;
  const int ti = tid >> 4, tj = tid & 15;
  double s0[4][4], s1[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) s0[a][b] = s1[a][b] = 0.0;
  const int m = D & ~1;
  int k0 = 0;
  for (; k0 < D; k0 += LC_PK) {
    __syncthreads();
    for (int i = tid; i < LC_PT * LC_PK; i += 256) {
      const int r = i / LC_PK, c = i % LC_PK;
      const int gi = bi * LC_PT + r, gj = bj * LC_PT + r, k = k0 + c;
      As[r * LC_PLD + c] = (gi < N && k < D) ? X[(long)gi * D + k] : 0.0;
      Bs[r * LC_PLD + c] = (gj < N && k < D) ? X[(long)gj * D + k] : 0.0;
    }
    __syncthreads();
    const int kmax = min(LC_PK, m - k0);  // (even; <= 0 in a chunk that only holds the odd tail)
    for (int k = 0; k < kmax; k += 2) {
      double av[4], bv[4], aw[4], bw[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        av[a] = As[(ti + 16 * a) * LC_PLD + k];
        aw[a] = As[(ti + 16 * a) * LC_PLD + k + 1];
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        bv[b] = Bs[(tj + 16 * b) * LC_PLD + k];
        bw[b] = Bs[(tj + 16 * b) * LC_PLD + k + 1];
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          s0[a][b] = s0[a][b] + av[a] * bv[b];
          s1[a][b] = s1[a][b] + aw[a] * bw[b];
        }
    }
  }
  // (the chunk that holds element D - 1 is the last one loaded and still in LDS)
  const int ktail = (D - 1) - (k0 - LC_PK);
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const long i = bi * LC_PT + ti + 16 * a, j = bj * LC_PT + tj + 16 * b;
      if (i < j && j < N) {
        double t = s0[a][b] + s1[a][b];
        if (D & 1) t = t + As[(ti + 16 * a) * LC_PLD + ktail] * Bs[(tj + 16 * b) * LC_PLD + ktail];
        out[(long)N * i - i * (i + 1) / 2 + (j - i - 1)] = cosine_distance_f64(t, nrm[i], nrm[j]);
      }
    }
}

constexpr size_t LC_LDS_MAX = 160 * 1024 - 1024;  // dynamic LDS budget (static part: 512 B)

// The workspace of pa_linkage_chain_f64 in 256-byte-aligned blocks: the status word with its padding, size[] and the
// chain (used when they do not live in LDS), Dmin of single linkage, the square matrix
struct LcState {
  int *status, *size, *chain;
  double *dmin, *S;
};
static LcState lc_layout(Carver& c, int n) {
  LcState s;
  s.status = c.take<int>(64);
  s.size = c.take<int>(n);
  s.chain = c.take<int>(n);
  s.dmin = c.take<double>(n);
  s.S = c.take<double>((size_t)n * (size_t)square_ld(n));
  return s;
}

// dynamic LDS of the merge kernels: size[] and the chain for nn_chain (8 n B: up to n = 20 352), size[] alone for
// single linkage (4 n B: up to n = 40 704); 0 = the state lives in the workspace.  PA_LINKAGE_CHAIN_LDS=0 asks for
// that form at every n (the form large n takes; tests).
static size_t lc_smem_bytes(int n, int method) {
  const char* e = getenv("PA_LINKAGE_CHAIN_LDS");
  if (e != nullptr && atoi(e) == 0) return 0;
  const size_t bytes = (method == PA_LINKAGE_SINGLE ? 4 : 8) * (size_t)n;
  return bytes <= LC_LDS_MAX ? bytes : 0;
}

}  // namespace pa

extern "C" {

// scipy.spatial.distance.pdist(X, "cosine"): condensed upper triangle in pa_pdist_f64's order; `norms`: N doubles
int pa_pdist_cosine_f64(const double* X, int N, int D, double* out, double* norms, void* stream) {
  if (N < 2) return 0;
  PA_REQUIRE(D >= 1, "pa_pdist_cosine_f64: dimension %d", D);
  PA_REQUIRE(X && out && norms, "pa_pdist_cosine_f64: null array");
  hipStream_t st = (hipStream_t)stream;
  const int nt = pa::cdiv(N, pa::LC_PT);
  pa::ProfScope prof("k_pdist_cosine_f64", stream, 2.0 * D * ((double)N * (N - 1) / 2),
                     8.0 * ((double)N * D + (double)N * (N - 1) / 2));
  pa_row_norms_f64(X, N, D, norms, stream);
  hipLaunchKernelGGL(pa::k_lc_pdist_cosine, dim3(nt, nt), dim3(256), 0, st, X, N, D, norms, out);
  PA_CHECK_LAUNCH("pa_pdist_cosine_f64");
  return 0;
}

// *flag (device int) = 1 when v holds a NaN or an infinity, else 0
int pa_nonfinite_flag_f64(const double* v, long count, int* flag, void* stream) {
  PA_REQUIRE(count >= 0 && flag && (count == 0 || v), "pa_nonfinite_flag_f64: null array");
  hipStream_t st = (hipStream_t)stream;
  if (pa::fill_async(flag, 0, sizeof(int), st) != hipSuccess) return 1;
  if (count == 0) return 0;
  const long blocks = (count + 256L * 8 - 1) / (256L * 8);
  hipLaunchKernelGGL(pa::k_lc_nonfinite, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, v, count,
                     flag);
  PA_CHECK_LAUNCH("pa_nonfinite_flag_f64");
  return 0;
}

// 0: n < 2, or the square copy exceeds the cap (the caller keeps the host path)
size_t pa_linkage_chain_workspace_bytes(int n) {
  if (n < 2 || !pa::square_fits(n)) return 0;
  return pa::carved_bytes([&](pa::Carver& c) { pa::lc_layout(c, n); });
}

int pa_linkage_chain_f64(const double* D, int n, int method, double* raw, void* workspace, size_t workspace_bytes,
                         void* stream) {
  PA_REQUIRE(n >= 2, "pa_linkage_chain_f64: n = %d, at least 2 points needed", n);
  PA_REQUIRE(method == PA_LINKAGE_SINGLE || method == PA_LINKAGE_COMPLETE || method == PA_LINKAGE_AVERAGE ||
                 method == PA_LINKAGE_WEIGHTED || method == PA_LINKAGE_WARD,
             "pa_linkage_chain_f64: unknown method %d", method);
  PA_REQUIRE(D && raw && workspace, "pa_linkage_chain_f64: null array");
  PA_REQUIRE(pa::square_fits(n),
             "pa_linkage_chain_f64: the square matrix of %d points exceeds PA_LINKAGE_FAST_MAX_GB", n);
  pa::Carver carver(workspace);
  const pa::LcState s = pa::lc_layout(carver, n);
  PA_REQUIRE(workspace_bytes >= carver.bytes(), "pa_linkage_chain_f64: workspace too small");
  const long ld = pa::square_ld(n);
  hipStream_t st = (hipStream_t)stream;
  // ~3 row scans + 1 update (2 rows in, row + column out) per merge
  pa::ProfScope prof("k_linkage_chain", stream, 4.0 * n * (double)n, 8.0 * 7.0 * n * (double)n);
  // the status word stays non-zero unless the merge kernel runs to its end
  if (pa::fill_async(s.status, 0xFF, 256, st) != hipSuccess) return 1;
  pa_square_from_condensed(D, n, ld, s.S, stream);
  PA_CHECK_LAUNCH("pa_linkage_chain_f64 (square copy)");
  const size_t lds_bytes = pa::lc_smem_bytes(n, method);
  const bool lds = lds_bytes != 0;
  // one workgroup; `state`: the chain (nn_chain) or Dmin (single linkage).  The LDS grant is per KERNEL (launch_state.h):
  // the nn-chain kernels share one signature, so a generic lambda would give them one static between them.
#define PA_LC_LAUNCH(LDS, kernel, state)                                                                              \
  do {                                                                                                                \
    if (LDS) PA_ALLOW_LDS("pa_linkage_chain_f64", kernel, pa::LC_LDS_MAX);                                            \
    hipLaunchKernelGGL(kernel, dim3(1), dim3(pa::LC_T), lds_bytes, st, s.S, n, ld, raw, s.size, state, s.status);     \
  } while (0)
#define PA_LC_CHAIN(M)                                                  \
  case M:                                                               \
    if (lds) PA_LC_LAUNCH(true, (pa::k_lc_nn_chain<M, true>), s.chain); \
    else PA_LC_LAUNCH(false, (pa::k_lc_nn_chain<M, false>), s.chain);   \
    break;
  switch (method) {
    PA_LC_CHAIN(PA_LINKAGE_COMPLETE)
    PA_LC_CHAIN(PA_LINKAGE_AVERAGE)
    PA_LC_CHAIN(PA_LINKAGE_WEIGHTED)
    PA_LC_CHAIN(PA_LINKAGE_WARD)
    default:
      if (lds) PA_LC_LAUNCH(true, (pa::k_lc_mst_single<true>), s.dmin);
      else PA_LC_LAUNCH(false, (pa::k_lc_mst_single<false>), s.dmin);
  }
#undef PA_LC_CHAIN
#undef PA_LC_LAUNCH
  PA_CHECK_LAUNCH("pa_linkage_chain_f64");
  return 0;
}

}  // extern "C"
