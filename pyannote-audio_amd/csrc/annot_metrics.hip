// Error counts of the time-based diarization and detection metrics (pyannote.metrics' DiarizationErrorRate,
// IdentificationErrorRate, DetectionErrorRate, DetectionPrecisionRecallFMeasure; restated from their published
// behaviour), on segments in seconds, in fp64.
//
// A label is on or off at a time t.  The time axis is cut at every boundary that can change what is on or what
// counts: the starts and ends of the reference, hypothesis and uem segments and, with a collar, the ends
// t -/+ collar/2 of the removed interval around every reference boundary.  Between two neighbouring cuts nothing
// changes, so every integral is a sum over these elementary intervals of (a small integer) * (the interval's
// length).  Four launches, each one thread per element with the other side staged through LDS:
//
//   k_annot_cuts       the M = 2 (Nr + Nh + Nu) [+ 4 Nr] cut values, in a fixed layout (cut_index below)
//   k_annot_rank       rank sort: rank[i] = #{j : c[j] < c[i], or c[j] == c[i] and j < i}; sorted[rank[i]] = c[i]
//   k_annot_intervals  interval k = [sorted[k], sorted[k+1]]: an item (segment, uem region, collar) that starts at
//                      rank lo and ends at rank hi covers it iff lo <= k < hi -- integer compares only.  (With tied
//                      cuts the test can differ from the comparison of the values only on intervals of length 0,
//                      which contribute 0.)  -> two 64-bit label masks and the evaluated length d per interval
//   k_annot_reduce     one workgroup per output value, a fixed order of additions: lane-strided partial sums, the
//                      xor butterfly, four wave partials added as (p0 + p1) + (p2 + p3).  No floating-point atomics:
//                      the same input gives the same bits, and inputs whose boundaries are dyadic give exact sums.
//
// pa_annot_corpus_counts (second half of this file) runs the same four steps for all files of a corpus in one call,
// after filling the within-label gaps of every hypothesis on the device (k_annot_support).
// pa_annot_window_counts takes the sums of many windows of one file from one sweep: the window boundaries are cuts
// too, a window is a contiguous range of the sorted intervals, and only the reduction runs per window.
//
// Every rank lies in 0..M-1 whatever the values are (NaN included: its rank is then meaningless, not out of
// range), a label outside 0..K-1 is ignored, a segment with end < start covers nothing: bad VALUES cannot make a
// kernel address out of bounds; the Python wrapper refuses them before the launch.
#include "common.h"
#include "pyannote_amd.h"

namespace pa {

constexpr int ANN_THREADS = 256;         // workgroup size = LDS tile of the rank sort and of the item sweep
constexpr int ANN_MAXK = 64;             // a side's labels travel as one 64-bit mask
constexpr long ANN_MAX_CUTS = 1L << 22;  // the rank sort is quadratic
constexpr int ANN_SCALARS = 7;

struct AnnotShape {
  int Nr, Nh, Nu, collar;  // collar: 0 / 1
  int W = 0;               // windows (pa_annot_window_counts): their boundaries are cuts, not items of the sweep
  __host__ __device__ int cuts() const { return 2 * (Nr + Nh + Nu) + (collar ? 4 * Nr : 0) + 2 * W; }
  __host__ __device__ int items() const { return Nr + Nh + Nu + (collar ? 2 * Nr : 0); }
};

// cut layout: [ref start Nr][ref end Nr][hyp start Nh][hyp end Nh][uem start Nu][uem end Nu]
//             [collar lo 2 Nr][collar hi 2 Nr]   (collar u < Nr: around ref start u; u >= Nr: around ref end u - Nr)
//             [window start W][window end W]     (pa_annot_window_counts only, written by k_annot_window_cuts)
// (the four steps are device functions of the workgroup index `blk`: the one-file kernels below and the corpus
// kernels further down run the same instructions on a file's arrays, which is what makes their bits equal)
__device__ __forceinline__ void annot_cuts(int blk, const double* __restrict__ ref_seg,
                                           const double* __restrict__ hyp_seg, const double* __restrict__ uem_seg,
                                           const AnnotShape& sh, double half_collar, double* __restrict__ cuts) {
  const int i = blk * ANN_THREADS + threadIdx.x;
  if (i >= sh.cuts()) return;
  const int Nr = sh.Nr, Nh = sh.Nh, Nu = sh.Nu;
  double v;
  int u = i;
  if (u < 2 * Nr) {
    v = u < Nr ? ref_seg[2 * u] : ref_seg[2 * (u - Nr) + 1];
  } else if ((u -= 2 * Nr) < 2 * Nh) {
    v = u < Nh ? hyp_seg[2 * u] : hyp_seg[2 * (u - Nh) + 1];
  } else if ((u -= 2 * Nh) < 2 * Nu) {
    v = u < Nu ? uem_seg[2 * u] : uem_seg[2 * (u - Nu) + 1];
  } else {
    u -= 2 * Nu;                                    // 0 .. 4 Nr - 1
    const int b = u < 2 * Nr ? u : u - 2 * Nr;      // which reference boundary
    const double t = b < Nr ? ref_seg[2 * b] : ref_seg[2 * (b - Nr) + 1];
    v = u < 2 * Nr ? t - half_collar : t + half_collar;
  }
  cuts[i] = v;
}

__global__ __launch_bounds__(ANN_THREADS) void k_annot_cuts(const double* __restrict__ ref_seg,
                                                            const double* __restrict__ hyp_seg,
                                                            const double* __restrict__ uem_seg, AnnotShape sh,
                                                            double half_collar, double* __restrict__ cuts) {
  annot_cuts(blockIdx.x, ref_seg, hyp_seg, uem_seg, sh, half_collar, cuts);
}

__device__ __forceinline__ void annot_rank(int blk, const double* __restrict__ cuts, int M,
                                           double* __restrict__ sorted, int* __restrict__ rank) {
  __shared__ double s_c[ANN_THREADS];
  const int tid = threadIdx.x, i = blk * ANN_THREADS + tid;
  const double ci = i < M ? cuts[i] : 0.0;
  int r = 0;
  for (int base = 0; base < M; base += ANN_THREADS) {
    __syncthreads();
    if (base + tid < M) s_c[tid] = cuts[base + tid];
    __syncthreads();
    const int n = min(ANN_THREADS, M - base);
    for (int t = 0; t < n; ++t) {
      const double v = s_c[t];
      r += (v < ci) | ((v == ci) & (base + t < i));
    }
  }
  if (i < M) {
    rank[i] = r;
    sorted[r] = ci;
  }
}

__global__ __launch_bounds__(ANN_THREADS) void k_annot_rank(const double* __restrict__ cuts, int M,
                                                            double* __restrict__ sorted, int* __restrict__ rank) {
  annot_rank(blockIdx.x, cuts, M, sorted, rank);
}

// item t of the sweep -> the cut indices of its start and end, the bit it sets and its kind
__device__ __forceinline__ void annot_item(int t, const AnnotShape& sh, const int32_t* __restrict__ ref_label,
                                           const int32_t* __restrict__ hyp_label, int Kr, int Kh, int& lo, int& hi,
                                           unsigned long long& rbit, unsigned long long& hbit, int& flag) {
  const int Nr = sh.Nr, Nh = sh.Nh, Nu = sh.Nu;
  rbit = hbit = 0;
  flag = 0;
  if (t < Nr) {
    lo = t, hi = Nr + t;
    const int l = ref_label[t];
    if (l >= 0 && l < Kr) rbit = 1ull << l;
  } else if ((t -= Nr) < Nh) {
    lo = 2 * Nr + t, hi = 2 * Nr + Nh + t;
    const int l = hyp_label[t];
    if (l >= 0 && l < Kh) hbit = 1ull << l;
  } else if ((t -= Nh) < Nu) {
    lo = 2 * (Nr + Nh) + t, hi = 2 * (Nr + Nh) + Nu + t;
    flag = 1;                                       // inside the uem
  } else {
    t -= Nu;
    lo = 2 * (Nr + Nh + Nu) + t, hi = 2 * (Nr + Nh + Nu) + 2 * Nr + t;
    flag = 2;                                       // inside a collar
  }
}

__device__ __forceinline__ void annot_intervals(
    int blk, const double* __restrict__ sorted, const int* __restrict__ rank, const int32_t* __restrict__ ref_label,
    const int32_t* __restrict__ hyp_label, const AnnotShape& sh, int Kr, int Kh, int skip_overlap,
    unsigned long long* __restrict__ rec_r, unsigned long long* __restrict__ rec_h, double* __restrict__ rec_d) {
  __shared__ unsigned long long s_rbit[ANN_THREADS], s_hbit[ANN_THREADS];
  __shared__ int s_lo[ANN_THREADS], s_hi[ANN_THREADS], s_flag[ANN_THREADS];
  const int tid = threadIdx.x, k = blk * ANN_THREADS + tid;
  const int nint = sh.cuts() - 1, nitems = sh.items();
  unsigned long long r = 0, h = 0;
  int flags = 0;
  for (int base = 0; base < nitems; base += ANN_THREADS) {
    __syncthreads();
    if (base + tid < nitems) {
      int lo, hi, flag;
      unsigned long long rb, hb;
      annot_item(base + tid, sh, ref_label, hyp_label, Kr, Kh, lo, hi, rb, hb, flag);
      s_lo[tid] = rank[lo];
      s_hi[tid] = rank[hi];
      s_rbit[tid] = rb;
      s_hbit[tid] = hb;
      s_flag[tid] = flag;
    }
    __syncthreads();
    const int n = min(ANN_THREADS, nitems - base);
    for (int t = 0; t < n; ++t) {
      const bool on = s_lo[t] <= k && k < s_hi[t];
      r |= on ? s_rbit[t] : 0ull;
      h |= on ? s_hbit[t] : 0ull;
      flags |= on ? s_flag[t] : 0;
    }
  }
  if (k >= nint) return;
  const bool evaluated = (flags & 1) && !(flags & 2) && !(skip_overlap && __popcll(r) >= 2);
  rec_r[k] = r;
  rec_h[k] = h;
  rec_d[k] = evaluated ? sorted[k + 1] - sorted[k] : 0.0;
}

__global__ __launch_bounds__(ANN_THREADS) void k_annot_intervals(
    const double* __restrict__ sorted, const int* __restrict__ rank, const int32_t* __restrict__ ref_label,
    const int32_t* __restrict__ hyp_label, AnnotShape sh, int Kr, int Kh, int skip_overlap,
    unsigned long long* __restrict__ rec_r, unsigned long long* __restrict__ rec_h, double* __restrict__ rec_d) {
  annot_intervals(blockIdx.x, sorted, rank, ref_label, hyp_label, sh, Kr, Kh, skip_overlap, rec_r, rec_h, rec_d);
}

// out: [cooc Kr*Kh][ref_dur Kr][hyp_dur Kh][total, false_alarm, missed, both, ref_speech, hyp_speech, both_speech]
__device__ __forceinline__ void annot_reduce(int o, const unsigned long long* __restrict__ rec_r,
                                             const unsigned long long* __restrict__ rec_h,
                                             const double* __restrict__ rec_d, int nint, int Kr, int Kh,
                                             double* __restrict__ out) {
  __shared__ double s_part[ANN_THREADS / 64];
  const int tid = threadIdx.x;
  const int ncooc = Kr * Kh;
  // what this workgroup sums: kind 0 cooc (i, j), 1 reference label i, 2 hypothesis label j, 3 + s scalar s
  int kind, i = 0, j = 0;
  if (o < ncooc) kind = 0, i = o / Kh, j = o % Kh;
  else if (o < ncooc + Kr) kind = 1, i = o - ncooc;
  else if (o < ncooc + Kr + Kh) kind = 2, j = o - ncooc - Kr;
  else kind = 3 + (o - ncooc - Kr - Kh);
  double acc = 0.0;
  for (int k = tid; k < nint; k += ANN_THREADS) {
    const unsigned long long r = rec_r[k], h = rec_h[k];
    const int nr = __popcll(r), nh = __popcll(h);
    int w;
    switch (kind) {
      case 0: w = (int)((r >> i) & 1ull) & (int)((h >> j) & 1ull); break;
      case 1: w = (int)((r >> i) & 1ull); break;
      case 2: w = (int)((h >> j) & 1ull); break;
      case 3: w = nr; break;
      case 4: w = max(0, nh - nr); break;
      case 5: w = max(0, nr - nh); break;
      case 6: w = min(nr, nh); break;
      case 7: w = nr > 0; break;
      case 8: w = nh > 0; break;
      default: w = nr > 0 && nh > 0; break;
    }
    acc += (double)w * rec_d[k];
  }
  acc = wave_sum_d(acc);
  if ((tid & 63) == 0) s_part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) out[o] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}

__global__ __launch_bounds__(ANN_THREADS) void k_annot_reduce(const unsigned long long* __restrict__ rec_r,
                                                              const unsigned long long* __restrict__ rec_h,
                                                              const double* __restrict__ rec_d, int nint, int Kr,
                                                              int Kh, double* __restrict__ out) {
  annot_reduce(blockIdx.x, rec_r, rec_h, rec_d, nint, Kr, Kh, out);
}

// ------------------------------------------------------------------------------------------------ windows
// pa_annot_window_counts: the sums of W windows of one file from ONE sweep.  The 2 W window boundaries join the cut
// list behind the file's own cuts; they are cuts only (no item of the sweep starts or ends there), so the label masks
// and the evaluated flag of every elementary interval are the file's.  Rank sort and sweep are the device functions
// above, run once; what is left per window is the reduction over its intervals.
__global__ __launch_bounds__(ANN_THREADS) void k_annot_window_cuts(const double* __restrict__ ref_seg,
                                                                   const double* __restrict__ hyp_seg,
                                                                   const double* __restrict__ uem_seg,
                                                                   const double* __restrict__ win_seg, AnnotShape sh,
                                                                   double half_collar, double* __restrict__ cuts) {
  AnnotShape file = sh;
  file.W = 0;
  annot_cuts(blockIdx.x, ref_seg, hyp_seg, uem_seg, file, half_collar, cuts);
  const int u = blockIdx.x * ANN_THREADS + threadIdx.x - file.cuts();
  if (u >= 0 && u < 2 * sh.W) cuts[file.cuts() + u] = u < sh.W ? win_seg[2 * u] : win_seg[2 * (u - sh.W) + 1];
}

// Window w is the rank range [a, b) of the interval list, a = rank of its start cut, b = rank of its end cut:
// sorted[a] is the window's start and sorted[b] its end, and `sorted` ascends, so an interval k < a ends at
// sorted[k + 1] <= start, an interval k >= b starts at sorted[k] >= end, and an interval a <= k < b lies inside
// [start, end].  An interval of non-zero length inside the window therefore has a <= k < b, and one of non-zero
// length outside it does not.  With tied cuts (a window edge on a segment boundary, the end of window w on the start
// of window w + 2) which of the equal cuts gets the lower rank is decided by the cut index, but the intervals that
// this moves across a or b lie between two equal cuts: length 0, contribution 0.  A window with end < start or a
// NaN boundary has an empty or meaningless range that still lies inside 0 .. cuts - 1.
// One workgroup per (window, output value): annot_reduce on the range, so the order of additions is fixed by the
// range alone -- no floating-point atomics, no workgroup waits for another.
__global__ __launch_bounds__(ANN_THREADS) void k_annot_window_reduce(const unsigned long long* __restrict__ rec_r,
                                                                     const unsigned long long* __restrict__ rec_h,
                                                                     const double* __restrict__ rec_d,
                                                                     const int* __restrict__ rank, AnnotShape sh,
                                                                     int Kr, int Kh, double* __restrict__ out) {
  const int w = blockIdx.x, first = sh.cuts() - 2 * sh.W;
  const int a = rank[first + w], b = rank[first + sh.W + w];
  const long nout = Kr * Kh + Kr + Kh + ANN_SCALARS;
  annot_reduce(blockIdx.y, rec_r + a, rec_h + a, rec_d + a, b > a ? b - a : 0, Kr, Kh, out + w * nout);
}

// the cuts of a file and of W windows over it (W = 0: pa_annot_counts' own count)
static bool annot_cut_count(int Nr, int Nh, int Nu, bool collar, long* M, int W = 0) {
  if (Nr < 0 || Nh < 0 || Nu < 0 || W < 0) return false;
  *M = 2 * ((long)Nr + Nh + Nu + W) + (collar ? 4 * (long)Nr : 0);
  return *M <= ANN_MAX_CUTS;
}

// The workspace of both entry points: 256 bytes of slack (the caller's pointer need not be aligned), then the arrays
// back to back.  NhT hypothesis rows of all files of a corpus (0 for pa_annot_counts), M cut slots.
constexpr size_t ANN_SLACK = 256;
struct AnnotBufs {
  double *tmp_seg, *m_seg;             // (NhT, 2) each: the merged hypothesis rows of stage A
  double *cuts, *sorted, *rec_d;       // (M) each, like the next three
  unsigned long long *rec_r, *rec_h;
  int* rank;
  int32_t* m_lab;                      // (NhT)
};
static AnnotBufs annot_layout(Carver& c, long NhT, long M) {
  AnnotBufs b;
  b.tmp_seg = c.take<double>(2 * NhT, 8);
  b.m_seg = c.take<double>(2 * NhT, 8);
  b.cuts = c.take<double>(M, 8);
  b.sorted = c.take<double>(M, 8);
  b.rec_r = c.take<unsigned long long>(M, 8);
  b.rec_h = c.take<unsigned long long>(M, 8);
  b.rec_d = c.take<double>(M, 8);
  b.rank = c.take<int>(M, 4);
  b.m_lab = c.take<int32_t>(NhT, 4);
  return b;
}

// ------------------------------------------------------------------------------------------------ a corpus
// F files in one call (pa_annot_corpus_counts).  Stage A fills the within-label gaps of every file's hypothesis
// (core.Annotation.support) and compacts the merged rows per file; stage B is the four steps above with the file
// as blockIdx.y.  A file's arrays start at its offsets; its cuts, ranks and interval records at cut_off[f], sized
// for the UNMERGED rows with a collar, so launches can be sized on the host; the merged row count is read on the
// device and workgroups beyond it leave at once.

// Timeline.support's rule for the current merged turn (.., E) and the next row (c, d) of the label, rows sorted by
// (start, end): merge when they intersect by more than the segment precision or the gap between them, taken as 0
// up to that precision, is < fill.  The float64 operations of core.Annotation.support, in its order.
__device__ __forceinline__ bool annot_merges(double E, double c, double d, double fill) {
  const double lo = d < E ? d : E;
  const double inter = lo - c, g = c - lo;
  return inter > 1e-6 || (g > 1e-6 ? g : 0.0) < fill;
}

// One workgroup per file, one wave per run (the rows of one label, listed in sorted order by run_rows).  The wave
// loads 64 rows at a time, one per lane, and walks them in order with every lane holding the same (a, E): the
// walk is the definition, the loads are what it would otherwise wait for.  Lane 0 writes the merged rows of the run
// to tmp_seg at the run's own positions; after the barrier the runs' counts are scanned and the rows copied to the
// file's first merged[f] hypothesis slots (run after run: any order serves stage B).
__global__ __launch_bounds__(ANN_THREADS) void k_annot_support(pa_annot_corpus c, double fill,
                                                               double* __restrict__ tmp_seg,
                                                               double* __restrict__ m_seg,
                                                               int32_t* __restrict__ m_lab,
                                                               int32_t* __restrict__ merged) {
  __shared__ int s_pre[ANN_MAXK + 1];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = c.run_first[f], nrun = min(c.run_first[f + 1] - r0, ANN_MAXK);
  for (int q = wave; q < nrun; q += ANN_THREADS / 64) {
    const int base = c.run_off[r0 + q], n = c.run_off[r0 + q + 1] - base;
    double a = 0.0, E = 0.0;
    int cnt = 0;
    // (a turn no longer than the segment precision is not a segment: `annotation[segment] = label` drops it)
    auto emit = [&]() {
      if (!(E - a > 1e-6)) return;
      if (lane == 0) tmp_seg[2 * (long)(base + cnt)] = a, tmp_seg[2 * (long)(base + cnt) + 1] = E;
      ++cnt;
    };
    for (int i0 = 0; i0 < n; i0 += 64) {
      double cl = 0.0, dl = 0.0;
      if (i0 + lane < n) {
        const int row = c.run_rows[base + i0 + lane];
        cl = c.hyp_seg[2 * (long)row];
        dl = c.hyp_seg[2 * (long)row + 1];
      }
      const int m = min(64, n - i0);
      for (int j = 0; j < m; ++j) {
        const double cj = __shfl(cl, j, 64), dj = __shfl(dl, j, 64);
        if (i0 + j == 0) {
          a = cj, E = dj;
        } else if (annot_merges(E, cj, dj, fill)) {
          E = dj > E ? dj : E;
        } else {
          emit();
          a = cj, E = dj;
        }
      }
    }
    if (n > 0) emit();
    if (lane == 0) s_pre[q + 1] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    s_pre[0] = 0;
    for (int q = 0; q < nrun; ++q) s_pre[q + 1] += s_pre[q];
    merged[f] = s_pre[nrun];
  }
  __syncthreads();
  const int h0 = c.hyp_off[f];
  for (int q = 0; q < nrun; ++q) {
    const int src = c.run_off[r0 + q], dst = h0 + s_pre[q], cnt = s_pre[q + 1] - s_pre[q];
    for (int k = tid; k < cnt; k += ANN_THREADS) {
      m_seg[2 * (long)(dst + k)] = tmp_seg[2 * (long)(src + k)];
      m_seg[2 * (long)(dst + k) + 1] = tmp_seg[2 * (long)(src + k) + 1];
      m_lab[dst + k] = q;
    }
  }
}

__device__ __forceinline__ AnnotShape corpus_shape(const pa_annot_corpus& c, const int32_t* __restrict__ merged,
                                                   int f, int collar) {
  return AnnotShape{c.ref_off[f + 1] - c.ref_off[f], merged[f], c.uem_off[f + 1] - c.uem_off[f], collar};
}

__global__ __launch_bounds__(ANN_THREADS) void k_annot_corpus_cuts(pa_annot_corpus c,
                                                                   const int32_t* __restrict__ merged,
                                                                   const double* __restrict__ m_seg, int collar,
                                                                   double half_collar, double* __restrict__ cuts) {
  const int f = blockIdx.y;
  const AnnotShape sh = corpus_shape(c, merged, f, collar);
  if ((int)blockIdx.x * ANN_THREADS >= sh.cuts()) return;
  annot_cuts(blockIdx.x, c.ref_seg + 2 * (long)c.ref_off[f], m_seg + 2 * (long)c.hyp_off[f],
             c.uem_seg + 2 * (long)c.uem_off[f], sh, half_collar, cuts + c.cut_off[f]);
}

__global__ __launch_bounds__(ANN_THREADS) void k_annot_corpus_rank(pa_annot_corpus c,
                                                                   const int32_t* __restrict__ merged, int collar,
                                                                   const double* __restrict__ cuts,
                                                                   double* __restrict__ sorted,
                                                                   int* __restrict__ rank) {
  const int f = blockIdx.y, M = corpus_shape(c, merged, f, collar).cuts();
  if ((int)blockIdx.x * ANN_THREADS >= M) return;          // (the whole workgroup: no barrier is left waiting)
  const int o = c.cut_off[f];
  annot_rank(blockIdx.x, cuts + o, M, sorted + o, rank + o);
}

__global__ __launch_bounds__(ANN_THREADS) void k_annot_corpus_intervals(
    pa_annot_corpus c, const int32_t* __restrict__ merged, const int32_t* __restrict__ m_lab, int collar,
    int skip_overlap, const double* __restrict__ sorted, const int* __restrict__ rank,
    unsigned long long* __restrict__ rec_r, unsigned long long* __restrict__ rec_h, double* __restrict__ rec_d) {
  const int f = blockIdx.y;
  const AnnotShape sh = corpus_shape(c, merged, f, collar);
  if ((int)blockIdx.x * ANN_THREADS >= sh.cuts() - 1) return;
  const int o = c.cut_off[f];
  annot_intervals(blockIdx.x, sorted + o, rank + o, c.ref_label + c.ref_off[f], m_lab + c.hyp_off[f], sh, c.Kr[f],
                  c.Kh[f], skip_overlap, rec_r + o, rec_h + o, rec_d + o);
}

__global__ __launch_bounds__(ANN_THREADS) void k_annot_corpus_reduce(
    pa_annot_corpus c, const int32_t* __restrict__ merged, int collar, const unsigned long long* __restrict__ rec_r,
    const unsigned long long* __restrict__ rec_h, const double* __restrict__ rec_d, double* __restrict__ out) {
  const int f = blockIdx.y, Kr = c.Kr[f], Kh = c.Kh[f];
  if ((int)blockIdx.x >= Kr * Kh + Kr + Kh + ANN_SCALARS) return;
  const int M = corpus_shape(c, merged, f, collar).cuts(), o = c.cut_off[f];
  annot_reduce(blockIdx.x, rec_r + o, rec_h + o, rec_d + o, M > 0 ? M - 1 : 0, Kr, Kh, out + c.out_off[f]);
}

// what the host tables allow: the totals, the largest file's cuts (with the collar asked for) and outputs
struct CorpusPlan {
  long NhT, Mt;         // hypothesis rows of all files; cut slots of all files (sized with a collar)
  int max_cuts, max_out;
};

static bool annot_corpus_plan(const pa_annot_corpus* c, bool collar, CorpusPlan* p) {
  if (!c || c->F < 0 || c->F > 65535 || c->R < 0) return false;
  if (c->F == 0) {
    *p = CorpusPlan{0, 0, 0, 0};
    return c->R == 0;
  }
  if (!c->h_ref_off || !c->h_hyp_off || !c->h_uem_off || !c->h_Kr || !c->h_Kh) return false;
  if (c->h_ref_off[0] != 0 || c->h_hyp_off[0] != 0 || c->h_uem_off[0] != 0) return false;
  long Mt = 0, runs = 0, nout = 0;
  int max_cuts = 0, max_out = 0;
  for (int f = 0; f < c->F; ++f) {
    const long Nr = (long)c->h_ref_off[f + 1] - c->h_ref_off[f], Nh = (long)c->h_hyp_off[f + 1] - c->h_hyp_off[f],
               Nu = (long)c->h_uem_off[f + 1] - c->h_uem_off[f];
    const int Kr = c->h_Kr[f], Kh = c->h_Kh[f];
    if (Nr < 0 || Nh < 0 || Nu < 0 || Kr < 0 || Kr > ANN_MAXK || Kh < 0 || Kh > ANN_MAXK) return false;
    const long cap = 2 * (Nr + Nh + Nu) + 4 * Nr, M = collar ? cap : cap - 4 * Nr;
    if (M > ANN_MAX_CUTS) return false;
    Mt += cap;
    runs += Kh;
    const int no = Kr * Kh + Kr + Kh + ANN_SCALARS;
    nout += no;
    max_cuts = max(max_cuts, (int)M);
    max_out = max(max_out, no);
  }
  if (Mt > 0x7fffffffL || nout > 0x7fffffffL || runs != c->R) return false;
  *p = CorpusPlan{(long)c->h_hyp_off[c->F], Mt, max_cuts, max_out};
  return true;
}

}  // namespace pa

extern "C" {

size_t pa_annot_counts_workspace_bytes(int Nr, int Nh, int Nu) {
  long M;
  if (!pa::annot_cut_count(Nr, Nh, Nu, true, &M)) return 0;
  return pa::carved_bytes([&](pa::Carver& c) { pa::annot_layout(c, 0, M); }, pa::ANN_SLACK);
}

int pa_annot_counts(const double* ref_seg, const int32_t* ref_label, int Nr, int Kr, const double* hyp_seg,
                    const int32_t* hyp_label, int Nh, int Kh, const double* uem_seg, int Nu, double collar,
                    int skip_overlap, double* out, void* ws, size_t ws_bytes, void* stream) {
  PA_REQUIRE(Kr >= 0 && Kr <= pa::ANN_MAXK && Kh >= 0 && Kh <= pa::ANN_MAXK,
             "pa_annot_counts: %d reference and %d hypothesis labels, 0..%d each supported", Kr, Kh, pa::ANN_MAXK);
  PA_REQUIRE(Nr >= 0 && Nh >= 0 && Nu >= 0, "pa_annot_counts: negative segment count (%d, %d, %d)", Nr, Nh, Nu);
  PA_REQUIRE(collar >= 0.0, "pa_annot_counts: collar %g is negative or NaN", collar);   // (NaN >= 0 is false)
  const bool with_collar = collar > 0.0;
  long M;
  PA_REQUIRE(pa::annot_cut_count(Nr, Nh, Nu, with_collar, &M), "pa_annot_counts: more than %ld cuts",
             pa::ANN_MAX_CUTS);
  PA_REQUIRE(out && (Nr == 0 || (ref_seg && ref_label)) && (Nh == 0 || (hyp_seg && hyp_label)) &&
                 (Nu == 0 || uem_seg),
             "pa_annot_counts: null array");
  pa::Carver carver(ws, pa::ANN_SLACK);
  const pa::AnnotBufs a = pa::annot_layout(carver, 0, M);
  PA_REQUIRE(ws && ws_bytes >= carver.bytes(), "pa_annot_counts: workspace of %zu bytes, %zu needed", ws_bytes,
             carver.bytes());
  hipStream_t s = (hipStream_t)stream;
  const pa::AnnotShape sh{Nr, Nh, Nu, with_collar ? 1 : 0};
  const int m = (int)M, nint = m > 0 ? m - 1 : 0;
  const int nout = Kr * Kh + Kr + Kh + pa::ANN_SCALARS;
  pa::ProfScope prof("k_annot_counts", stream, 0.0, 44.0 * m + 8.0 * nout);
  if (nint > 0) {
    const int grid = pa::cdiv(m, pa::ANN_THREADS);
    hipLaunchKernelGGL(pa::k_annot_cuts, dim3(grid), dim3(pa::ANN_THREADS), 0, s, ref_seg, hyp_seg, uem_seg, sh,
                       0.5 * collar, a.cuts);
    hipLaunchKernelGGL(pa::k_annot_rank, dim3(grid), dim3(pa::ANN_THREADS), 0, s, a.cuts, m, a.sorted, a.rank);
    hipLaunchKernelGGL(pa::k_annot_intervals, dim3(pa::cdiv(nint, pa::ANN_THREADS)), dim3(pa::ANN_THREADS), 0, s,
                       a.sorted, a.rank, ref_label, hyp_label, sh, Kr, Kh, skip_overlap ? 1 : 0, a.rec_r, a.rec_h,
                       a.rec_d);
  }
  // (without intervals the sums are empty: the kernel writes the zeros)
  hipLaunchKernelGGL(pa::k_annot_reduce, dim3(nout), dim3(pa::ANN_THREADS), 0, s, a.rec_r, a.rec_h, a.rec_d, nint, Kr,
                     Kh, out);
  PA_CHECK_LAUNCH("pa_annot_counts");
  return 0;
}

size_t pa_annot_window_counts_workspace_bytes(int Nr, int Nh, int Nu, int W) {
  long M;
  if (!pa::annot_cut_count(Nr, Nh, Nu, true, &M, W)) return 0;
  return pa::carved_bytes([&](pa::Carver& c) { pa::annot_layout(c, 0, M); }, pa::ANN_SLACK);
}

int pa_annot_window_counts(const double* ref_seg, const int32_t* ref_label, int Nr, int Kr, const double* hyp_seg,
                           const int32_t* hyp_label, int Nh, int Kh, const double* uem_seg, int Nu,
                           const double* win_seg, int W, double collar, int skip_overlap, double* out, void* ws,
                           size_t ws_bytes, void* stream) {
  PA_REQUIRE(Kr >= 0 && Kr <= pa::ANN_MAXK && Kh >= 0 && Kh <= pa::ANN_MAXK,
             "pa_annot_window_counts: %d reference and %d hypothesis labels, 0..%d each supported", Kr, Kh,
             pa::ANN_MAXK);
  PA_REQUIRE(Nr >= 0 && Nh >= 0 && Nu >= 0 && W >= 0,
             "pa_annot_window_counts: negative segment or window count (%d, %d, %d, %d)", Nr, Nh, Nu, W);
  PA_REQUIRE(collar >= 0.0, "pa_annot_window_counts: collar %g is negative or NaN", collar);
  const bool with_collar = collar > 0.0;
  long M;
  PA_REQUIRE(pa::annot_cut_count(Nr, Nh, Nu, with_collar, &M, W), "pa_annot_window_counts: more than %ld cuts",
             pa::ANN_MAX_CUTS);
  PA_REQUIRE((W == 0 || (out && win_seg)) && (Nr == 0 || (ref_seg && ref_label)) &&
                 (Nh == 0 || (hyp_seg && hyp_label)) && (Nu == 0 || uem_seg),
             "pa_annot_window_counts: null array");
  pa::Carver carver(ws, pa::ANN_SLACK);
  const pa::AnnotBufs a = pa::annot_layout(carver, 0, M);
  PA_REQUIRE(ws && ws_bytes >= carver.bytes(), "pa_annot_window_counts: workspace of %zu bytes, %zu needed", ws_bytes,
             carver.bytes());
  if (W == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const pa::AnnotShape sh{Nr, Nh, Nu, with_collar ? 1 : 0, W};
  const int m = (int)M;                                       // >= 2: the windows' own cuts
  const int nout = Kr * Kh + Kr + Kh + pa::ANN_SCALARS;
  pa::ProfScope prof("k_annot_window_counts", stream, 0.0, 44.0 * m + 8.0 * nout * W);
  const int grid = pa::cdiv(m, pa::ANN_THREADS);
  hipLaunchKernelGGL(pa::k_annot_window_cuts, dim3(grid), dim3(pa::ANN_THREADS), 0, s, ref_seg, hyp_seg, uem_seg,
                     win_seg, sh, 0.5 * collar, a.cuts);
  hipLaunchKernelGGL(pa::k_annot_rank, dim3(grid), dim3(pa::ANN_THREADS), 0, s, a.cuts, m, a.sorted, a.rank);
  hipLaunchKernelGGL(pa::k_annot_intervals, dim3(pa::cdiv(m - 1, pa::ANN_THREADS)), dim3(pa::ANN_THREADS), 0, s,
                     a.sorted, a.rank, ref_label, hyp_label, sh, Kr, Kh, skip_overlap ? 1 : 0, a.rec_r, a.rec_h,
                     a.rec_d);
  hipLaunchKernelGGL(pa::k_annot_window_reduce, dim3(W, nout), dim3(pa::ANN_THREADS), 0, s, a.rec_r, a.rec_h, a.rec_d,
                     a.rank, sh, Kr, Kh, out);
  PA_CHECK_LAUNCH("pa_annot_window_counts");
  return 0;
}

size_t pa_annot_corpus_workspace_bytes(const pa_annot_corpus* corpus) {
  pa::CorpusPlan p;
  if (!pa::annot_corpus_plan(corpus, true, &p)) return 0;
  return pa::carved_bytes([&](pa::Carver& c) { pa::annot_layout(c, p.NhT, p.Mt); }, pa::ANN_SLACK);
}

int pa_annot_corpus_counts(const pa_annot_corpus* corpus, double fill, double collar, int skip_overlap, double* out,
                           int32_t* merged_rows, void* ws, size_t ws_bytes, void* stream) {
  PA_REQUIRE(fill >= 0.0, "pa_annot_corpus_counts: fill %g is negative or NaN", fill);
  PA_REQUIRE(collar >= 0.0, "pa_annot_corpus_counts: collar %g is negative or NaN", collar);
  const bool with_collar = collar > 0.0;
  pa::CorpusPlan p;
  PA_REQUIRE(pa::annot_corpus_plan(corpus, with_collar, &p),
             "pa_annot_corpus_counts: the host tables are missing or not offsets, more than 65535 files, a file with "
             "more than %d labels on a side or more than %ld cuts, or R is not the sum of Kh",
             pa::ANN_MAXK, pa::ANN_MAX_CUTS);
  const pa_annot_corpus& c = *corpus;
  if (c.F == 0) return 0;
  PA_REQUIRE(out && merged_rows && c.ref_off && c.hyp_off && c.uem_off && c.cut_off && c.out_off && c.Kr && c.Kh &&
                 c.run_first && c.run_off &&
                 (c.h_ref_off[c.F] == 0 || (c.ref_seg && c.ref_label)) &&
                 (p.NhT == 0 || (c.hyp_seg && c.run_rows)) && (c.h_uem_off[c.F] == 0 || c.uem_seg),
             "pa_annot_corpus_counts: null array");
  pa::Carver carver(ws, pa::ANN_SLACK);
  const pa::AnnotBufs a = pa::annot_layout(carver, p.NhT, p.Mt);
  PA_REQUIRE(ws && ws_bytes >= carver.bytes(), "pa_annot_corpus_counts: workspace of %zu bytes, %zu needed", ws_bytes,
             carver.bytes());
  hipStream_t s = (hipStream_t)stream;
  const int col = with_collar ? 1 : 0;
  pa::ProfScope prof("k_annot_corpus_counts", stream, 0.0, 44.0 * p.Mt + 68.0 * p.NhT);
  const dim3 block(pa::ANN_THREADS);
  hipLaunchKernelGGL(pa::k_annot_support, dim3(c.F), block, 0, s, c, fill, a.tmp_seg, a.m_seg, a.m_lab,
                     merged_rows);
  if (p.max_cuts > 1) {
    const dim3 grid(pa::cdiv(p.max_cuts, pa::ANN_THREADS), c.F);
    hipLaunchKernelGGL(pa::k_annot_corpus_cuts, grid, block, 0, s, c, merged_rows, a.m_seg, col, 0.5 * collar,
                       a.cuts);
    hipLaunchKernelGGL(pa::k_annot_corpus_rank, grid, block, 0, s, c, merged_rows, col, a.cuts, a.sorted, a.rank);
    hipLaunchKernelGGL(pa::k_annot_corpus_intervals, dim3(pa::cdiv(p.max_cuts - 1, pa::ANN_THREADS), c.F), block, 0,
                       s, c, merged_rows, a.m_lab, col, skip_overlap ? 1 : 0, a.sorted, a.rank, a.rec_r, a.rec_h,
                       a.rec_d);
  }
  hipLaunchKernelGGL(pa::k_annot_corpus_reduce, dim3(p.max_out, c.F), block, 0, s, c, merged_rows, col, a.rec_r,
                     a.rec_h, a.rec_d, out);
  PA_CHECK_LAUNCH("pa_annot_corpus_counts");
  return 0;
}

}  // extern "C"
