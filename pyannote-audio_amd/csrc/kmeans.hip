// KMeans on gfx950, fp64: scikit-learn 1.7.2's dense `KMeans(init="k-means++", algorithm="lloyd")` with unit sample
// weights (sklearn/cluster/_kmeans.py: _kmeans_plusplus, _kmeans_single_lloyd), the call behind
// KMeansClustering.cluster and the forced speaker counts of VBxClustering (pipelines/clustering.py:545-547, 635-637).
//
// Sizes: N = training embeddings of a file (<= ~10^4; 6 x 10^4 for a joint clustering), D = 256 (512 for XVector),
// K = speakers (units to tens), n_init = 3 initialisations.  One Lloyd iteration is 2 N K D flops -- tens of MFLOP:
// the cost is launches, not arithmetic.  So the initialisations are JOBS (blockIdx.y) served by one set of launches,
// the stop tests run on the device, and a job that has stopped makes its workgroups return at entry.
//
// Determinism: every sum has a fixed order that depends on the problem's shape alone.  A workgroup owns KM_ROWS
// consecutive rows whatever N is and writes per-block partial results; the kernel after it adds the partials in block
// order.  A row's dot products are 64 lane sums (columns lane, lane + 64, ...) joined by a butterfly, which gives every
// lane the same bits.  No floating-point atomics, and no workgroup reads what another wrote in the same launch.
// What scikit-learn computes with BLAS in another order differs in the last bits of the VALUES; labels, picks and
// iteration counts are integers that only a knife edge could move (tests/kmeans_model.py measures the distance).
#include "common.h"

#include <algorithm>
#include <vector>

namespace pa {

constexpr int KM_T = 256;           // threads of the row-block kernels: 4 waves
constexpr int KM_WAVES = KM_T / 64;
constexpr int KM_ROWS = 64;         // rows a workgroup owns
constexpr int KM_WROWS = KM_ROWS / KM_WAVES;
constexpr int KM_MAX_K = 64;
constexpr int KM_MAX_D = 512;
constexpr int KM_CHUNKS = KM_MAX_D / 64;   // columns of a row a lane holds
constexpr int KM_MAX_T = 6;         // 2 + int(log(64)) candidates per k-means++ centre
constexpr int KM_SCAN_T = 1024;     // threads of the scan workgroup
constexpr int KM_ACC = 6144;        // doubles of LDS for a block's partial sums (K x DC)
enum { KM_STRICT = 0, KM_TOL = 1, KM_MAXITER = 2 };

struct KmState {
  const double* X;        // (N, D) the caller's rows
  const int32_t* first;   // (J)
  const double* uniforms; // (J, K - 1, T)
  double* Xc;             // (N, D) rows minus the column means
  double* mean;           // (D)
  double* tolv;           // (1) tol * mean of the column variances
  double* closest;        // (J, N) squared distance to the nearest centre picked so far
  double* nd;             // (J, T, N) the same with each candidate added
  double* potpart;        // (J, T, NB) per-block sums of nd
  double* pot;            // (J)
  double* C;              // (J, 2, K, D) centres: the current ones and the ones being computed
  double* csq;            // (J, 2, K) their squared norms
  double* part;           // (J, NB, K, D) per-block sums of the members' rows
  double* shiftpart;      // (J, K)
  double* inpart;         // (J, NB) per-block inertia
  int* cnt;               // (J, NB, K) per-block member counts
  int* changed;           // (J, NB) labels that changed, per block
  int* cand;              // (J, T) candidate rows
  int* counts;            // (J, K) members
  int* done;              // (J)
  int* cur;               // (J) which half of C is current
  int32_t* labels;        // (J, N)  outputs from here on
  double* centers;        // (J, K, D)
  double* inertia;        // (J)
  int32_t* picks;         // (J, K)
  int32_t* status;        // (J, 4): iterations, stop kind, empty-cluster flag, non-finite flag
  int N, D, K, J, T, NB, DC, max_iter;
  double tol;
};

// the columns lane, lane + 64, ... of a row; columns past D read as zero
__device__ __forceinline__ void km_load_row(const double* __restrict__ row, int D, int lane, double (&x)[KM_CHUNKS]) {
#pragma unroll
  for (int m = 0; m < KM_CHUNKS; ++m) {
    const int d = lane + 64 * m;
    x[m] = d < D ? row[d] : 0.0;
  }
}

// |x - c|^2, the same bits in every lane
__device__ __forceinline__ double km_sqdist(const double (&x)[KM_CHUNKS], const double* __restrict__ c, int D,
                                            int lane) {
  double s = 0.0;
#pragma unroll
  for (int m = 0; m < KM_CHUNKS; ++m) {
    const int d = lane + 64 * m;
    if (d < D) {
      const double t = x[m] - c[d];
      s += t * t;
    }
  }
  return wave_sum_d(s);
}

// first argmin over the centres of |c|^2 - 2 x.c (what sklearn's lloyd_iter minimises), the same in every lane
__device__ __forceinline__ int km_nearest(const double (&x)[KM_CHUNKS], const double* __restrict__ C,
                                          const double* __restrict__ csq, int K, int D, int lane) {
  int best = 0;
  double best_v = 0.0;
  for (int k = 0; k < K; ++k) {
    const double* c = C + (size_t)k * D;
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < KM_CHUNKS; ++m) {
      const int d = lane + 64 * m;
      if (d < D) s += x[m] * c[d];
    }
    const double v = csq[k] - 2.0 * wave_sum_d(s);
    if (k == 0 || v < best_v) best = k, best_v = v;
  }
  return best;
}

// sum of p[0..n) by one wave: lane l adds p[l], p[l + 64], ... in that order, then the butterfly
__device__ __forceinline__ double km_wave_ordered_sum(const double* __restrict__ p, long n, int lane) {
  double s = 0.0;
  for (long i = lane; i < n; i += 64) s += p[i];
  return wave_sum_d(s);
}

// ---- preparation: column means, centred rows, tolerance ------------------------------------------------------------
// per-block column sums of X (centred == 0) or of the squares of Xc = X - mean, which it also writes (centred == 1)
__global__ __launch_bounds__(KM_T) void k_km_colpart(KmState s, int centred) {
  const int b = blockIdx.x;
  const long row0 = (long)b * KM_ROWS;
  const int rows = (int)min((long)KM_ROWS, s.N - row0);
  for (int d = threadIdx.x; d < s.D; d += KM_T) {
    const double mu = centred ? s.mean[d] : 0.0;
    double acc = 0.0;
    for (int r = 0; r < rows; ++r) {
      const size_t at = (size_t)(row0 + r) * s.D + d;
      if (centred) {
        const double v = s.X[at] - mu;
        s.Xc[at] = v;
        acc += v * v;
      } else {
        acc += s.X[at];
      }
    }
    s.part[(size_t)b * s.D + d] = acc;
  }
}

// the block partials added in block order: the column means (centred == 0), or the variances and from them tolv, the
// non-finite flag and the initial state of every job (centred == 1)
__global__ __launch_bounds__(KM_MAX_D) void k_km_colfinish(KmState s, int centred) {
  __shared__ double var[KM_MAX_D];
  const int d = threadIdx.x;
  if (d < s.D) {
    double acc = 0.0;
    for (int b = 0; b < s.NB; ++b) acc += s.part[(size_t)b * s.D + d];
    if (centred) var[d] = acc / s.N;
    else s.mean[d] = acc / s.N;
  }
  if (!centred) return;
  __syncthreads();
  if (d == 0) {
    double total = 0.0;
    for (int i = 0; i < s.D; ++i) total += var[i];
    s.tolv[0] = s.tol * (total / s.D);
    const int bad = !isfinite(total);
    for (int j = 0; j < s.J; ++j) {
      s.done[j] = bad;
      s.cur[j] = 0;
      s.status[4 * j + 0] = 0;
      s.status[4 * j + 1] = KM_MAXITER;
      s.status[4 * j + 2] = 0;
      s.status[4 * j + 3] = bad;
    }
  }
}

// ---- k-means++ -------------------------------------------------------------------------------------------------------
// the candidates' distance vectors nd[t] = min(closest, |x - X[cand_t]|^2) and their per-block sums; `begin`: the
// first centre, one "candidate" (the drawn row) and no closest yet; it also resets the labels
__global__ __launch_bounds__(KM_T) void k_km_pp_dist(KmState s, int begin) {
  __shared__ double red[KM_WAVES][KM_MAX_T];
  const int j = blockIdx.y, b = blockIdx.x;
  if (s.done[j]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ntr = begin ? 1 : s.T;
  int cand[KM_MAX_T];
#pragma unroll
  for (int t = 0; t < KM_MAX_T; ++t) {
    int c = 0;
    if (t < ntr) c = begin ? s.first[j] : s.cand[j * s.T + t];
    cand[t] = min(max(c, 0), s.N - 1);
  }
  if (begin && b == 0 && threadIdx.x == 0) s.cand[j * s.T] = cand[0];
  double sum[KM_MAX_T];
#pragma unroll
  for (int t = 0; t < KM_MAX_T; ++t) sum[t] = 0.0;
  for (int r = 0; r < KM_WROWS; ++r) {
    const long i = (long)b * KM_ROWS + w * KM_WROWS + r;
    if (i >= s.N) break;
    double x[KM_CHUNKS];
    km_load_row(s.Xc + (size_t)i * s.D, s.D, lane, x);
    const double cl = begin ? 0.0 : s.closest[(size_t)j * s.N + i];
#pragma unroll
    for (int t = 0; t < KM_MAX_T; ++t) {
      if (t < ntr) {
        const double dist = km_sqdist(x, s.Xc + (size_t)cand[t] * s.D, s.D, lane);
        const double v = begin ? dist : fmin(cl, dist);
        sum[t] += v;
        if (lane == 0) s.nd[((size_t)j * s.T + t) * s.N + i] = v;
      }
    }
    if (begin && lane == 0) s.labels[(size_t)j * s.N + i] = -1;
  }
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < KM_MAX_T; ++t) red[w][t] = sum[t];
  }
  __syncthreads();
  if ((int)threadIdx.x < ntr) {
    double total = red[0][threadIdx.x];
    for (int v = 1; v < KM_WAVES; ++v) total += red[v][threadIdx.x];
    s.potpart[((size_t)j * s.T + threadIdx.x) * s.NB + b] = total;
  }
}

// the candidate with the smallest potential (the first of equals) becomes centre `c`: its row goes into the centres,
// its distance vector becomes `closest`, its sum the potential.  One workgroup per job.
__global__ __launch_bounds__(KM_T) void k_km_pp_adopt(KmState s, int c) {
  __shared__ double pots[KM_MAX_T];
  __shared__ int best_s;
  const int j = blockIdx.x;
  if (s.done[j]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ntr = c == 0 ? 1 : s.T;
  for (int t = w; t < ntr; t += KM_WAVES) {
    const double v = km_wave_ordered_sum(s.potpart + ((size_t)j * s.T + t) * s.NB, s.NB, lane);
    if (lane == 0) pots[t] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int best = 0;
    for (int t = 1; t < ntr; ++t)
      if (pots[t] < pots[best]) best = t;
    best_s = best;
    s.pot[j] = pots[best];
    s.picks[j * s.K + c] = s.cand[j * s.T + best];
  }
  __syncthreads();
  const int best = best_s;
  const int row = s.cand[j * s.T + best];
  const double* src = s.nd + ((size_t)j * s.T + best) * s.N;
  double* dst = s.closest + (size_t)j * s.N;
  for (long i = threadIdx.x; i < s.N; i += KM_T) dst[i] = src[i];
  double* centre = s.C + ((size_t)(j * 2) * s.K + c) * s.D;
  const double* x = s.Xc + (size_t)row * s.D;
  for (int d = threadIdx.x; d < s.D; d += KM_T) centre[d] = x[d];
  if (w == 0) {
    double sq = 0.0;
    for (int d = lane; d < s.D; d += 64) sq += x[d] * x[d];
    sq = wave_sum_d(sq);
    if (lane == 0) s.csq[(size_t)(j * 2) * s.K + c] = sq;
  }
}

// cand[t] = min(searchsorted(cumsum(closest), u[t] * pot, side="left"), N - 1) for the T draws of centre c.  One
// workgroup per job; thread i owns the rows [i seg, (i + 1) seg), seg = ceil(N / KM_SCAN_T): the running sum of a row
// is (the sum of the segments before, added in order) + (the rows of its segment so far, added in order).
__global__ __launch_bounds__(KM_SCAN_T) void k_km_pp_scan(KmState s, int c) {
  __shared__ double seg_sum[KM_SCAN_T];
  __shared__ int found[KM_MAX_T];
  const int j = blockIdx.x;
  if (s.done[j]) return;
  const int tid = threadIdx.x;
  const double* closest = s.closest + (size_t)j * s.N;
  const long seg = ((long)s.N + KM_SCAN_T - 1) / KM_SCAN_T;
  const long lo = min((long)s.N, tid * seg), hi = min((long)s.N, lo + seg);
  double local = 0.0;
  for (long i = lo; i < hi; ++i) local += closest[i];
  seg_sum[tid] = local;
  if (tid < KM_MAX_T) found[tid] = 0x7fffffff;
  __syncthreads();
  if (tid == 0) {
    double run = 0.0;
    for (int i = 0; i < KM_SCAN_T; ++i) {
      const double v = seg_sum[i];
      seg_sum[i] = run;
      run += v;
    }
  }
  __syncthreads();
  const double before = seg_sum[tid], pot = s.pot[j];
  double target[KM_MAX_T];
  bool open[KM_MAX_T];
#pragma unroll
  for (int t = 0; t < KM_MAX_T; ++t) {
    open[t] = t < s.T;
    target[t] = open[t] ? s.uniforms[((size_t)j * (s.K - 1) + (c - 1)) * s.T + t] * pot : 0.0;
  }
  double run = 0.0;
  for (long i = lo; i < hi; ++i) {
    run += closest[i];
    const double cum = before + run;
#pragma unroll
    for (int t = 0; t < KM_MAX_T; ++t) {
      if (open[t] && cum >= target[t]) {
        open[t] = false;
        atomicMin(&found[t], (int)i);
      }
    }
  }
  __syncthreads();
  if (tid < s.T) s.cand[j * s.T + tid] = min(found[tid], s.N - 1);
}

// ---- Lloyd -----------------------------------------------------------------------------------------------------------
// labels of the block's rows, how many changed, and the block's member counts and member sums per centre
__global__ __launch_bounds__(KM_T) void k_km_assign(KmState s) {
  __shared__ int lab[KM_ROWS];
  __shared__ int chg[KM_WAVES];
  extern __shared__ __attribute__((aligned(16))) double acc[];   // (K, DC); a thread only touches its own columns
  const int j = blockIdx.y, b = blockIdx.x;
  if (s.done[j]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int cur = s.cur[j];
  const double* C = s.C + (size_t)(j * 2 + cur) * s.K * s.D;
  const double* csq = s.csq + (size_t)(j * 2 + cur) * s.K;
  const long row0 = (long)b * KM_ROWS;
  const int rows = (int)min((long)KM_ROWS, s.N - row0);
  int changed = 0;
  for (int r = 0; r < KM_WROWS; ++r) {
    const int local = w * KM_WROWS + r;
    int label = -1;
    if (local < rows) {
      double x[KM_CHUNKS];
      km_load_row(s.Xc + (size_t)(row0 + local) * s.D, s.D, lane, x);
      label = km_nearest(x, C, csq, s.K, s.D, lane);
      int32_t* out = s.labels + (size_t)j * s.N + row0 + local;
      changed += label != *out;
      if (lane == 0) *out = label;
    }
    if (lane == 0) lab[local] = label;
  }
  if (lane == 0) chg[w] = changed;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int v = 0; v < KM_WAVES; ++v) total += chg[v];
    s.changed[(size_t)j * s.NB + b] = total;
  }
  if ((int)threadIdx.x < s.K) {
    int members = 0;
    for (int r = 0; r < rows; ++r) members += lab[r] == (int)threadIdx.x;
    s.cnt[((size_t)j * s.NB + b) * s.K + threadIdx.x] = members;
  }
  double* part = s.part + ((size_t)j * s.NB + b) * s.K * s.D;
  for (int d0 = 0; d0 < s.D; d0 += s.DC) {
    for (int dd = threadIdx.x; dd < s.DC && d0 + dd < s.D; dd += KM_T) {
      for (int k = 0; k < s.K; ++k) acc[k * s.DC + dd] = 0.0;
      for (int r = 0; r < rows; ++r) acc[lab[r] * s.DC + dd] += s.Xc[(size_t)(row0 + r) * s.D + d0 + dd];
      for (int k = 0; k < s.K; ++k) part[(size_t)k * s.D + d0 + dd] = acc[k * s.DC + dd];
    }
  }
}

// centre k of job j: the block partials added in block order, divided by the members; its squared norm and its
// share of the shift.  grid (K, J)
__global__ __launch_bounds__(KM_T) void k_km_update(KmState s) {
  __shared__ int cnt_red[KM_T];
  __shared__ double red[2][KM_WAVES];
  const int j = blockIdx.y, k = blockIdx.x;
  if (s.done[j]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int members = 0;
  for (int b = threadIdx.x; b < s.NB; b += KM_T) members += s.cnt[((size_t)j * s.NB + b) * s.K + k];
  cnt_red[threadIdx.x] = members;
  __syncthreads();
  for (int o = KM_T / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) cnt_red[threadIdx.x] += cnt_red[threadIdx.x + o];
    __syncthreads();
  }
  members = cnt_red[0];
  const int cur = s.cur[j];
  const double* old_c = s.C + ((size_t)(j * 2 + cur) * s.K + k) * s.D;
  double* new_c = s.C + ((size_t)(j * 2 + (cur ^ 1)) * s.K + k) * s.D;
  double shift = 0.0, sq = 0.0;
  for (int d = threadIdx.x; d < s.D; d += KM_T) {
    double total = 0.0;
    for (int b = 0; b < s.NB; ++b) total += s.part[(((size_t)j * s.NB + b) * s.K + k) * s.D + d];
    // an empty cluster keeps its centre: the job is given up by k_km_decide
    const double v = members > 0 ? total / members : old_c[d];
    const double t = v - old_c[d];
    new_c[d] = v;
    shift += t * t;
    sq += v * v;
  }
  shift = wave_sum_d(shift);
  sq = wave_sum_d(sq);
  if (lane == 0) red[0][w] = shift, red[1][w] = sq;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = red[0][0], q = red[1][0];
    for (int v = 1; v < KM_WAVES; ++v) a += red[0][v], q += red[1][v];
    s.shiftpart[j * s.K + k] = a;
    s.csq[(size_t)(j * 2 + (cur ^ 1)) * s.K + k] = q;
    s.counts[j * s.K + k] = members;
  }
}

// sklearn's tests after iteration `it` (the centres are swapped BEFORE them): the same labels as before -> strict
// stop; else shift <= tolv -> tol stop; an empty cluster gives the job up.  One wave per job.
__global__ __launch_bounds__(64) void k_km_decide(KmState s, int it) {
  const int j = blockIdx.x;
  if (s.done[j]) return;
  const int lane = threadIdx.x;
  int changed = 0;
  for (int b = lane; b < s.NB; b += 64) changed += s.changed[(size_t)j * s.NB + b] != 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) changed += __shfl_xor(changed, o, 64);
  if (lane != 0) return;
  double shift = 0.0;
  bool empty = false;
  for (int k = 0; k < s.K; ++k) {
    shift += s.shiftpart[j * s.K + k];
    empty |= s.counts[j * s.K + k] == 0;
  }
  s.cur[j] ^= 1;
  s.status[4 * j + 0] = it + 1;
  if (empty) {
    s.status[4 * j + 2] = 1;
    s.done[j] = 1;
  } else if (changed == 0) {
    s.status[4 * j + 1] = KM_STRICT;
    s.done[j] = 1;
  } else if (shift <= s.tolv[0]) {
    s.status[4 * j + 1] = KM_TOL;
    s.done[j] = 1;
  } else if (it + 1 >= s.max_iter) {
    s.done[j] = 1;   // status[1] is KM_MAXITER from the start
  }
}

// after the last iteration: one more assignment with the final centres unless the stop was strict, and the block's
// share of the inertia (sum of |x - C_label|^2)
__global__ __launch_bounds__(KM_T) void k_km_last_assign(KmState s) {
  __shared__ double red[KM_WAVES];
  const int j = blockIdx.y, b = blockIdx.x;
  if (s.status[4 * j + 2] || s.status[4 * j + 3]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int cur = s.cur[j];
  const double* C = s.C + (size_t)(j * 2 + cur) * s.K * s.D;
  const double* csq = s.csq + (size_t)(j * 2 + cur) * s.K;
  const bool again = s.status[4 * j + 1] != KM_STRICT;
  double sum = 0.0;
  for (int r = 0; r < KM_WROWS; ++r) {
    const long i = (long)b * KM_ROWS + w * KM_WROWS + r;
    if (i >= s.N) break;
    double x[KM_CHUNKS];
    km_load_row(s.Xc + (size_t)i * s.D, s.D, lane, x);
    int32_t* out = s.labels + (size_t)j * s.N + i;
    int label;
    if (again) {
      label = km_nearest(x, C, csq, s.K, s.D, lane);
      if (lane == 0) *out = label;
    } else {
      label = min(max(*out, 0), s.K - 1);
    }
    sum += km_sqdist(x, C + (size_t)label * s.D, s.D, lane);
  }
  if (lane == 0) red[w] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = red[0];
    for (int v = 1; v < KM_WAVES; ++v) total += red[v];
    s.inpart[(size_t)j * s.NB + b] = total;
  }
}

// inertia = the block shares added in order; the centres go out in the caller's coordinates.  One workgroup per job.
__global__ __launch_bounds__(KM_T) void k_km_finish(KmState s) {
  const int j = blockIdx.x;
  if (s.status[4 * j + 2] || s.status[4 * j + 3]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (w == 0) {
    const double v = km_wave_ordered_sum(s.inpart + (size_t)j * s.NB, s.NB, lane);
    if (lane == 0) s.inertia[j] = v;
  }
  const double* C = s.C + (size_t)(j * 2 + s.cur[j]) * s.K * s.D;
  double* out = s.centers + (size_t)j * s.K * s.D;
  for (int i = threadIdx.x; i < s.K * s.D; i += KM_T) out[i] = C[i] + s.mean[i % s.D];
}

static int km_trials(int K) { return 2 + (K >= 3) + (K >= 8) + (K >= 21) + (K >= 55); }   // 2 + int(log(K)), K <= 64

static bool km_supported(int N, int D, int K, int n_init) {
  return K >= 2 && K <= KM_MAX_K && D >= 1 && D <= KM_MAX_D && N >= K && N < (1 << 24) && n_init >= 1 &&
         n_init <= 65535;
}

// The workspace of pa_kmeans_f64, one 256-byte-aligned block per array: the KmState fields the caller does not give
static KmState km_layout(Carver& c, int N, int D, int K, int n_init) {
  KmState s;
  const size_t n = N, d = D, k = K, J = n_init, T = km_trials(K), NB = (n + KM_ROWS - 1) / KM_ROWS;
  s.Xc = c.take<double>(n * d);
  s.mean = c.take<double>(d + 1);
  s.tolv = s.mean + d;
  s.closest = c.take<double>(J * n);
  s.nd = c.take<double>(J * T * n);
  s.potpart = c.take<double>(J * T * NB);
  s.pot = c.take<double>(J);
  s.C = c.take<double>(J * 2 * k * d);
  s.csq = c.take<double>(J * 2 * k);
  s.part = c.take<double>(J * NB * k * d);
  s.shiftpart = c.take<double>(J * k);
  s.inpart = c.take<double>(J * NB);
  s.cnt = c.take<int>(J * NB * k);
  s.changed = c.take<int>(J * NB);
  s.cand = c.take<int>(J * T);
  s.counts = c.take<int>(J * k);
  s.done = c.take<int>(J);
  s.cur = c.take<int>(J);
  s.N = N, s.D = D, s.K = K, s.J = n_init, s.T = (int)T, s.NB = (int)NB;
  s.DC = std::min(D, KM_ACC / K);
  return s;
}

}  // namespace pa

extern "C" {

int pa_kmeans_max_clusters(void) { return pa::KM_MAX_K; }
int pa_kmeans_max_dim(void) { return pa::KM_MAX_D; }

size_t pa_kmeans_workspace_bytes(int N, int D, int K, int n_init) {
  if (!pa::km_supported(N, D, K, n_init)) return 0;
  return pa::carved_bytes([&](pa::Carver& c) { pa::km_layout(c, N, D, K, n_init); });
}

int pa_kmeans_f64(const double* X, int N, int D, int K, int n_init, const int32_t* first, const double* uniforms,
                  int max_iter, double tol, int round_iterations, int32_t* labels, double* centers, double* inertia,
                  int32_t* picks, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  PA_REQUIRE(K >= 2, "pa_kmeans_f64: fewer than 2 clusters");
  PA_REQUIRE(K <= pa::KM_MAX_K, "pa_kmeans_f64: more clusters than pa_kmeans_max_clusters()");
  PA_REQUIRE(D >= 1 && D <= pa::KM_MAX_D, "pa_kmeans_f64: dimension outside 1..pa_kmeans_max_dim()");
  PA_REQUIRE(N >= K, "pa_kmeans_f64: fewer rows than clusters");
  PA_REQUIRE(N < (1 << 24), "pa_kmeans_f64: 2^24 rows or more");
  PA_REQUIRE(n_init >= 1 && n_init <= 65535, "pa_kmeans_f64: n_init outside 1..65535");
  PA_REQUIRE(max_iter >= 1, "pa_kmeans_f64: max_iter below 1");
  pa::Carver carver(workspace);
  pa::KmState s = pa::km_layout(carver, N, D, K, n_init);
  PA_REQUIRE(workspace_bytes >= carver.bytes(), "pa_kmeans_f64: workspace too small");
  s.X = X, s.first = first, s.uniforms = uniforms;
  s.labels = labels, s.centers = centers, s.inertia = inertia, s.picks = picks, s.status = status;
  s.max_iter = max_iter, s.tol = tol;
  const size_t n = N, d = D, k = K, J = n_init, NB = s.NB;
  hipStream_t st = (hipStream_t)stream;
  const dim3 row_grid((unsigned)NB, (unsigned)J), job_grid((unsigned)J);
  const size_t acc_bytes = (size_t)K * s.DC * 8;
  pa::ProfScope prof("k_kmeans", stream, 2.0 * n * k * d * J, 8.0 * n * d * J);
  hipLaunchKernelGGL(pa::k_km_colpart, dim3((unsigned)NB), dim3(pa::KM_T), 0, st, s, 0);
  hipLaunchKernelGGL(pa::k_km_colfinish, dim3(1), dim3(pa::KM_MAX_D), 0, st, s, 0);
  hipLaunchKernelGGL(pa::k_km_colpart, dim3((unsigned)NB), dim3(pa::KM_T), 0, st, s, 1);
  hipLaunchKernelGGL(pa::k_km_colfinish, dim3(1), dim3(pa::KM_MAX_D), 0, st, s, 1);
  hipLaunchKernelGGL(pa::k_km_pp_dist, row_grid, dim3(pa::KM_T), 0, st, s, 1);
  hipLaunchKernelGGL(pa::k_km_pp_adopt, job_grid, dim3(pa::KM_T), 0, st, s, 0);
  for (int c = 1; c < K; ++c) {
    hipLaunchKernelGGL(pa::k_km_pp_scan, job_grid, dim3(pa::KM_SCAN_T), 0, st, s, c);
    hipLaunchKernelGGL(pa::k_km_pp_dist, row_grid, dim3(pa::KM_T), 0, st, s, 0);
    hipLaunchKernelGGL(pa::k_km_pp_adopt, job_grid, dim3(pa::KM_T), 0, st, s, c);
  }
  PA_CHECK_LAUNCH("pa_kmeans_f64");
  // the Lloyd iterations in rounds; between two rounds the done flags come back and the loop ends once every job
  // has stopped (round_iterations <= 0: all max_iter iterations are enqueued and nothing is read back)
  std::vector<int> done(J);
  for (int it = 0; it < max_iter;) {
    const int upto = round_iterations > 0 ? std::min(max_iter, it + round_iterations) : max_iter;
    for (; it < upto; ++it) {
      hipLaunchKernelGGL(pa::k_km_assign, row_grid, dim3(pa::KM_T), acc_bytes, st, s);
      hipLaunchKernelGGL(pa::k_km_update, dim3((unsigned)K, (unsigned)J), dim3(pa::KM_T), 0, st, s);
      hipLaunchKernelGGL(pa::k_km_decide, job_grid, dim3(64), 0, st, s, it);
    }
    PA_CHECK_LAUNCH("pa_kmeans_f64");
    if (round_iterations > 0 && it < max_iter) {
      hipError_t e = hipMemcpyAsync(done.data(), s.done, 4 * J, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) {
        pa::set_error("pa_kmeans_f64: reading the done flags failed: %s", hipGetErrorString(e));
        return 1;
      }
      if (std::all_of(done.begin(), done.end(), [](int v) { return v != 0; })) break;
    }
  }
  hipLaunchKernelGGL(pa::k_km_last_assign, row_grid, dim3(pa::KM_T), 0, st, s);
  hipLaunchKernelGGL(pa::k_km_finish, job_grid, dim3(pa::KM_T), 0, st, s);
  PA_CHECK_LAUNCH("pa_kmeans_f64");
  return 0;
}

}  // extern "C"
