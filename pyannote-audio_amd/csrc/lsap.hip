// Batched linear sum assignment, `scipy.optimize.linear_sum_assignment` bit for bit and tie for tie, and the cost
// matrices of `permutation.permutate` (utils/permutation.py:99-196 of the reference): DESIGN.md section 30.
//
// k_lsap: one 64-lane workgroup (one wave) per problem of at most 64 x 64.  SciPy's solver is the shortest augmenting
// path algorithm of Crouse (2016); tests/lsap_model.py restates it.  Only additions, subtractions and comparisons of
// doubles occur, in SciPy's order, so the duals, and with them every tie, are SciPy's.  What is parallel is the scan of
// one row over the remaining columns: lane j owns column j (v, the shortest path cost, the path's row, the column's row,
// its SC bit and its POSITION in SciPy's `remaining` array), lane i owns row i (u, the row's column).  SciPy scans
// `remaining` in order and keeps, among the columns at the minimum, the last unassigned one, or else the first one;
// `remaining` is permuted by its swap-removal, so the position is carried: the lane at position num - 1 takes the
// position of the removed column.
// Every loop is a `for` with a bound known on entry (an augmentation scans at most nc times, a path has at most nr
// rows); the `break`s only leave earlier.  No input bit pattern makes the kernel run longer than nr * nc scan steps.
//
// k_pair_costs: one thread per (batch, i, j) adds the frames one after the other in the input dtype, product and sum
// rounded separately (this file is compiled with -ffp-contract=off), and divides once: numpy's `np.mean(.., axis=0)`
// of a (frames, C1, C2) array.
// hipcc-flags: -ffp-contract=off
#include "common.h"

namespace pa {

constexpr int LS_MAX = 64;

__device__ __forceinline__ double ls_shfl(double x, int lane) { return __shfl(x, lane, 64); }

// the smallest value over the wave, by `<` alone (no NaN reaches this: the entries were checked, and sums of finite
// values and +inf never give one unless the duals overflow, where SciPy's comparisons are as false as these)
__device__ __forceinline__ double ls_wave_min(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double y = __shfl_xor(x, o, 64);
    x = y < x ? y : x;
  }
  return x;
}
__device__ __forceinline__ int ls_wave_max(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int y = __shfl_xor(x, o, 64);
    x = y > x ? y : x;
  }
  return x;
}

// LDS: the compacted problem, rows <= columns, negated for `maximize`: c[i * nc + j]; then three int tables of 64
__global__ __launch_bounds__(LS_MAX) void k_lsap(const double* __restrict__ cost, long batch_stride, long row_stride,
                                                 long col_stride, int rows, int cols,
                                                 const unsigned long long* __restrict__ row_mask,
                                                 const unsigned long long* __restrict__ col_mask, int maximize,
                                                 int* __restrict__ col4row_out, double* __restrict__ total_out,
                                                 unsigned char* __restrict__ status_out) {
  extern __shared__ __attribute__((aligned(16))) char ls_smem[];
  double* c = (double*)ls_smem;
  int* row_of = (int*)(c + (size_t)rows * cols);   // compacted row -> row of the caller
  int* col_of = row_of + LS_MAX;                   // compacted column -> column of the caller
  int* answer = col_of + LS_MAX;                   // row of the caller -> column of the caller, -1: none
  const int lane = threadIdx.x;
  const long b = blockIdx.x;
  const double* mine = cost + b * batch_stride;
  const double INF = __builtin_inf();

  const unsigned long long all_rows = rows >= 64 ? ~0ull : (1ull << rows) - 1;
  const unsigned long long all_cols = cols >= 64 ? ~0ull : (1ull << cols) - 1;
  const unsigned long long rm = (row_mask ? row_mask[b] : ~0ull) & all_rows;
  const unsigned long long cm = (col_mask ? col_mask[b] : ~0ull) & all_cols;
  const int nR = __popcll(rm), nC = __popcll(cm);
  const unsigned long long below = (1ull << lane) - 1;
  if ((rm >> lane) & 1) row_of[__popcll(rm & below)] = lane;
  if ((cm >> lane) & 1) col_of[__popcll(cm & below)] = lane;
  answer[lane] = -1;
  __syncthreads();

  const bool transposed = nC < nR;               // SciPy solves the transpose of a tall matrix
  const int nr = transposed ? nC : nR, nc = transposed ? nR : nC;
  bool bad = false;
  for (int e = lane; e < nr * nc; e += LS_MAX) {
    const int i = e / nc, j = e - i * nc;
    const int r = transposed ? row_of[j] : row_of[i], k = transposed ? col_of[i] : col_of[j];
    double x = mine[r * row_stride + k * col_stride];
    if (maximize) x = -x;
    bad |= x != x || x == -INF;
    c[e] = x;
  }
  __syncthreads();
  int status = __ballot(bad) != 0 ? 1 : 0;

  // lane j: column j; lane i: row i
  double v = 0.0, u = 0.0, spc = INF;
  int path = -1, row4col = -1, col4row = -1;
  if (status == 0) {
    for (int cur = 0; cur < nr; ++cur) {
      double min_val = 0.0;
      int i = cur, num = nc, sink = -1;
      int pos = lane < nc ? nc - 1 - lane : -1;   // remaining[it] = nc - 1 - it
      unsigned long long SR = 0, SC = 0;
      spc = INF;
      for (int step = 0; step < nc; ++step) {
        SR |= 1ull << i;
        const double ui = ls_shfl(u, i);
        if (pos >= 0) {
          const double r = ((min_val + c[i * nc + lane]) - ui) - v;
          if (r < spc) {
            path = i;
            spc = r;
          }
        }
        const double lowest = ls_wave_min(pos >= 0 ? spc : INF);
        if (lowest == INF) {
          status = 2;
          break;
        }
        min_val = lowest;
        const bool at_min = pos >= 0 && spc == lowest;
        const bool any_free = __ballot(at_min && row4col == -1) != 0;
        // the last unassigned column at the minimum in scan order, or else the first column at the minimum
        const int key = !at_min ? -1 : any_free ? (row4col == -1 ? pos : -1) : LS_MAX - 1 - pos;
        const int best = ls_wave_max(key);
        const unsigned long long chosen = __ballot(key == best && key >= 0);
        if (chosen == 0) {   // (cannot happen: some lane is at the minimum)
          status = 2;
          break;
        }
        const int j = __ffsll((long long)chosen) - 1;
        const int index = any_free ? best : LS_MAX - 1 - best;
        const int owner = __shfl(row4col, j, 64);
        if (owner == -1) sink = j; else i = owner;
        SC |= 1ull << j;
        --num;
        if (pos == num) pos = index;    // remaining[index] = remaining[num]
        if (lane == j) pos = -1;
        if (sink != -1) break;
      }
      if (status != 0) break;
      if (sink == -1) {      // (cannot happen: nc columns were removed and none was free, with nr <= nc)
        status = 2;
        break;
      }
      // the duals
      const int mate = col4row >= 0 ? col4row : 0;
      const double spc_mate = ls_shfl(spc, mate);
      if (lane == cur) u += min_val;
      else if ((SR >> lane) & 1) u += min_val - spc_mate;
      if ((SC >> lane) & 1) v -= min_val - spc;
      // augment along the path
      int j = sink;
      for (int hop = 0; hop < nr; ++hop) {
        const int i2 = __shfl(path, j, 64);
        if (lane == j) row4col = i2;
        const int old = __shfl(col4row, i2, 64);
        if (lane == i2) col4row = j;
        j = old;
        if (i2 == cur) break;
        if (j < 0) {         // (cannot happen: every row of the path but `cur` has a column)
          status = 2;
          break;
        }
      }
      if (status != 0) break;
    }
  }

  if (status == 0 && lane < nr && col4row >= 0) {
    if (transposed) answer[row_of[col4row]] = col_of[lane];
    else answer[row_of[lane]] = col_of[col4row];
  }
  __syncthreads();
  const int mine_col = lane < rows ? answer[lane] : -1;
  if (lane < rows) col4row_out[b * rows + lane] = mine_col;
  if (total_out) {
    const double x = mine_col >= 0 ? mine[lane * row_stride + mine_col * col_stride] : 0.0;
    double total = 0.0;
    for (int r = 0; r < rows; ++r) {
      const double xr = ls_shfl(x, r);
      if (__shfl(mine_col, r, 64) >= 0) total += xr;
    }
    if (lane == 0) total_out[b] = total;
  }
  if (lane == 0) status_out[b] = (unsigned char)status;
}

// ------------------------------------------------------------------------------------------ permutate's costs
template <typename T>
__global__ __launch_bounds__(256) void k_pair_costs(const T* __restrict__ y1, long s1b, long s1f, long s1c,
                                                    const T* __restrict__ y2, long s2b, long s2f, long s2c, long batch,
                                                    int frames, int C1, int C2, int R, int mae,
                                                    double* __restrict__ cost) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= batch * C1 * C2) return;
  const int j = (int)(t % C2), i = (int)(t / C2 % C1);
  const long b = t / ((long)C1 * C2);
  const T* a = y1 + b * s1b + i * s1c;
  const T* p = y2 + b * s2b + j * s2c;
  T acc = 0;
  for (int f = 0; f < frames; ++f) {
    const T d = a[f * s1f] - p[f * s2f];
    const T term = mae ? (d < 0 ? -d : d) : d * d;
    acc = acc + term;
  }
  cost[(b * R + i) * C2 + j] = (double)(acc / (T)frames);
}

// rows C1..R-1 of every matrix: max(cost) + 1, both in T (np.max hands a NaN on)
template <typename T>
__global__ __launch_bounds__(64) void k_pair_cost_padding(long batch, int C1, int C2, int R, double* __restrict__ cost) {
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
  double* m = cost + b * R * C2;
  T top = (T)m[0];
  for (int e = 1; e < C1 * C2; ++e) {
    const T x = (T)m[e];
    if (x > top || x != x) top = x;
    if (top != top) break;
  }
  const double fill = (double)(T)(top + (T)1);
  for (int e = C1 * C2; e < R * C2; ++e) m[e] = fill;
}

// out (batch, frames, C1) contiguous: column i is class perm[b][i] of y2, zeros where perm is -1
template <typename T>
__global__ __launch_bounds__(256) void k_permute_classes(const T* __restrict__ y2, long s2b, long s2f, long s2c,
                                                         const int* __restrict__ perm, long perm_stride, long batch,
                                                         int frames, int C1, int C2, T* __restrict__ out) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= batch * frames * C1) return;
  const int i = (int)(t % C1);
  const long f = t / C1 % frames, b = t / ((long)C1 * frames);
  const int j = perm[b * perm_stride + i];
  out[t] = j >= 0 && j < C2 ? y2[b * s2b + f * s2f + j * s2c] : (T)0;
}

}  // namespace pa

extern "C" {

int pa_lsap_max_size(void) { return pa::LS_MAX; }

int pa_lsap_batch(const double* cost, long batch_stride, long row_stride, long col_stride, int batch, int rows,
                  int cols, const uint64_t* row_mask, const uint64_t* col_mask, int maximize, int32_t* col4row,
                  double* total, uint8_t* status, void* stream) {
  PA_REQUIRE(batch >= 0 && rows >= 0 && cols >= 0 && rows <= pa::LS_MAX && cols <= pa::LS_MAX,
             "pa_lsap_batch: at most 64 rows and 64 columns");
  if (batch == 0) return 0;
  PA_REQUIRE(status != nullptr && (col4row != nullptr || rows == 0) && (cost != nullptr || rows * cols == 0),
             "pa_lsap_batch: cost, col4row and status are required");
  const size_t lds = (size_t)rows * cols * sizeof(double) + 3 * pa::LS_MAX * sizeof(int);
  pa::ProfScope prof("k_lsap", stream, 0.0, (8.0 * rows * cols + 4.0 * rows + 9.0) * batch);
  hipLaunchKernelGGL(pa::k_lsap, dim3(batch), dim3(pa::LS_MAX), lds, (hipStream_t)stream, cost, batch_stride,
                     row_stride, col_stride, rows, cols, (const unsigned long long*)row_mask,
                     (const unsigned long long*)col_mask, maximize, col4row, total, status);
  PA_CHECK_LAUNCH("pa_lsap_batch");
  return 0;
}

int pa_pair_costs(const void* y1, long y1_batch_stride, long y1_frame_stride, long y1_class_stride, const void* y2,
                  long y2_batch_stride, long y2_frame_stride, long y2_class_stride, int is_f64, int batch, int frames,
                  int C1, int C2, int mae, double* cost, void* stream) {
  PA_REQUIRE(batch >= 0 && frames >= 1 && C1 >= 1 && C2 >= 1 && C1 <= pa::LS_MAX && C2 <= pa::LS_MAX,
             "pa_pair_costs: at least one frame and 1..64 classes a side");
  if (batch == 0) return 0;
  const int R = C1 > C2 ? C1 : C2;
  const long threads = (long)batch * C1 * C2;
  pa::ProfScope prof("k_pair_costs", stream, 3.0 * threads * frames,
                     (is_f64 ? 8.0 : 4.0) * batch * frames * (C1 + C2) + 8.0 * batch * R * C2);
  const dim3 grid(pa::cdiv(threads, 256)), pad_grid(pa::cdiv(batch, 64));
  hipStream_t st = (hipStream_t)stream;
  if (is_f64) {
    hipLaunchKernelGGL(pa::k_pair_costs<double>, grid, dim3(256), 0, st, (const double*)y1, y1_batch_stride,
                       y1_frame_stride, y1_class_stride, (const double*)y2, y2_batch_stride, y2_frame_stride,
                       y2_class_stride, (long)batch, frames, C1, C2, R, mae, cost);
    if (R > C1) hipLaunchKernelGGL(pa::k_pair_cost_padding<double>, pad_grid, dim3(64), 0, st, (long)batch, C1, C2, R, cost);
  } else {
    hipLaunchKernelGGL(pa::k_pair_costs<float>, grid, dim3(256), 0, st, (const float*)y1, y1_batch_stride,
                       y1_frame_stride, y1_class_stride, (const float*)y2, y2_batch_stride, y2_frame_stride,
                       y2_class_stride, (long)batch, frames, C1, C2, R, mae, cost);
    if (R > C1) hipLaunchKernelGGL(pa::k_pair_cost_padding<float>, pad_grid, dim3(64), 0, st, (long)batch, C1, C2, R, cost);
  }
  PA_CHECK_LAUNCH("pa_pair_costs");
  return 0;
}

int pa_permute_classes(const void* y2, long y2_batch_stride, long y2_frame_stride, long y2_class_stride, int is_f64,
                       const int32_t* perm, long perm_stride, int batch, int frames, int C1, int C2, void* out,
                       void* stream) {
  PA_REQUIRE(batch >= 0 && frames >= 0 && C1 >= 1 && C2 >= 1, "pa_permute_classes: at least one class a side");
  const long threads = (long)batch * frames * C1;
  if (threads == 0) return 0;
  pa::ProfScope prof("k_permute_classes", stream, 0.0, (is_f64 ? 16.0 : 8.0) * threads);
  const dim3 grid(pa::cdiv(threads, 256));
  if (is_f64)
    hipLaunchKernelGGL(pa::k_permute_classes<double>, grid, dim3(256), 0, (hipStream_t)stream, (const double*)y2,
                       y2_batch_stride, y2_frame_stride, y2_class_stride, perm, perm_stride, (long)batch, frames, C1, C2,
                       (double*)out);
  else
    hipLaunchKernelGGL(pa::k_permute_classes<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)y2,
                       y2_batch_stride, y2_frame_stride, y2_class_stride, perm, perm_stride, (long)batch, frames, C1, C2,
                       (float*)out);
  PA_CHECK_LAUNCH("pa_permute_classes");
  return 0;
}

}  // extern "C"
