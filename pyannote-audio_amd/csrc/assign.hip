// Constrained assignment of local speakers to clusters, every chunk of a file in one launch: what
// `BaseClustering.constrained_argmax` (clustering.py; pipelines/clustering.py:127-140 of the reference) gets from one
// scipy.optimize.linear_sum_assignment call per chunk.
//
// Sizes: C chunks (3 600 per audio-hour), S <= 4 local speakers, K <= 64 clusters.  One thread per chunk searches
// EXHAUSTIVELY over the injective maps of the chunk's non-silent rows into the clusters (partial maps of K rows when
// there are fewer clusters than rows).  With A active rows and K >= A a row only ever needs one of its A best
// columns (at most A - 1 of them are taken by the other rows), so the search visits at most (A + 1)^A = 625 nodes.
//
// SciPy does not say which optimum it returns when there are several, so the kernel does not guess: a chunk is
// FLAGGED, and solved by the caller with SciPy itself, when
//   * an active row holds a non-finite value, or
//   * another map comes within AS_MARGIN of the best total.  The search sees every map over the kept columns;
//     a map that uses a dropped column of row r loses at least v_A(r) - v_{A+1}(r) (the gap between the last kept and
//     the first dropped value of that row) against one over kept columns, so that gap is tested too.
// The totals are sums of <= 4 doubles of magnitude <= 3: rounding is ~1e-15, the margin 1e-9.
#include "common.h"

namespace pa {

constexpr int AS_MAXS = 4, AS_MAXK = 64, AS_T = 256;
constexpr double AS_MARGIN = 1e-9;

// soft (C, S, K) fp64; silent (C, S) uint8, non-zero = the local speaker never speaks; hard (C, S) int8: the
// cluster of every row, -2 for a silent or unassigned row; flagged (C) uint8
__global__ __launch_bounds__(AS_T) void k_constrained_assign(const double* __restrict__ soft,
                                                            const unsigned char* __restrict__ silent, int C,
                                                            int S, int K, signed char* __restrict__ hard,
                                                            unsigned char* __restrict__ flagged) {
  const long c = (long)blockIdx.x * AS_T + threadIdx.x;
  if (c >= C) return;
  const double* chunk = soft + c * S * K;
  int rows[AS_MAXS];
  int A = 0;
  for (int s = 0; s < S; ++s) {
    hard[c * S + s] = -2;
    if (!silent[c * S + s]) rows[A++] = s;
  }
  bool flag = false;
  for (int a = 0; a < A; ++a)
    for (int k = 0; k < K; ++k) flag |= !isfinite(chunk[rows[a] * K + k]);
  if (A == 0 || flag) {
    flagged[c] = flag;
    return;
  }
  // the L best columns of every active row, by selection (first index wins among equal values)
  const int L = A < K ? A : K, want = L;   // `want` rows are assigned: min(A, K)
  int col[AS_MAXS][AS_MAXS];
  double val[AS_MAXS][AS_MAXS];
  for (int a = 0; a < A; ++a) {
    const double* row = chunk + rows[a] * K;
    unsigned long long taken = 0;
    for (int l = 0; l < L; ++l) {
      int best = -1;
      for (int k = 0; k < K; ++k)
        if (!((taken >> k) & 1) && (best < 0 || row[k] > row[best])) best = k;
      taken |= 1ull << best;
      col[a][l] = best;
      val[a][l] = row[best];
    }
    if (K > L) {   // the first dropped value
      double next = -__builtin_inf();
      for (int k = 0; k < K; ++k)
        if (!((taken >> k) & 1)) next = fmax(next, row[k]);
      flag |= val[a][L - 1] - next < AS_MARGIN;
    }
  }
  // every row takes one of its kept columns or none (choice L); exactly `want` rows take one, no column twice
  double best_total = -__builtin_inf(), second_total = -__builtin_inf();
  int best_choice[AS_MAXS] = {0, 0, 0, 0};
  int choice[AS_MAXS] = {0, 0, 0, 0};
  int total_nodes = 1;
  for (int a = 0; a < A; ++a) total_nodes *= L + 1;
  for (int node = 0; node < total_nodes; ++node) {
    int rest = node, assigned = 0;
    unsigned long long used = 0;
    bool ok = true;
    double total = 0.0;
    for (int a = 0; a < A; ++a) {
      const int l = rest % (L + 1);
      rest /= L + 1;
      choice[a] = l;
      if (l == L) continue;
      const unsigned long long bit = 1ull << col[a][l];
      ok &= !(used & bit);
      used |= bit;
      total += val[a][l];
      ++assigned;
    }
    if (!ok || assigned != want) continue;
    if (total > best_total) {
      second_total = best_total;
      best_total = total;
      for (int a = 0; a < A; ++a) best_choice[a] = choice[a];
    } else if (total > second_total) {
      second_total = total;
    }
  }
  flag |= best_total - second_total < AS_MARGIN;
  flagged[c] = flag;
  if (flag) return;
  for (int a = 0; a < A; ++a)
    if (best_choice[a] < L) hard[c * S + rows[a]] = (signed char)col[a][best_choice[a]];
}

}  // namespace pa

extern "C" {

int pa_constrained_assign_max_speakers(void) { return pa::AS_MAXS; }
int pa_constrained_assign_max_clusters(void) { return pa::AS_MAXK; }

int pa_constrained_assign(const double* soft, const unsigned char* silent, int chunks, int speakers, int clusters,
                          signed char* hard, unsigned char* flagged, void* stream) {
  if (chunks <= 0) return 0;
  PA_REQUIRE(speakers >= 1 && speakers <= pa::AS_MAXS && clusters >= 1 && clusters <= pa::AS_MAXK,
             "pa_constrained_assign: at most 4 local speakers and 64 clusters");
  pa::ProfScope prof("k_constrained_assign", stream, 625.0 * 4 * chunks,
                     8.0 * chunks * speakers * clusters + 3.0 * chunks * speakers);
  hipLaunchKernelGGL(pa::k_constrained_assign, dim3((chunks + pa::AS_T - 1) / pa::AS_T), dim3(pa::AS_T), 0,
                     (hipStream_t)stream, soft, silent, chunks, speakers, clusters, hard, flagged);
  PA_CHECK_LAUNCH("pa_constrained_assign");
  return 0;
}

}  // extern "C"
