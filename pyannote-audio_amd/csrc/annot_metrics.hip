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
  __host__ __device__ int cuts() const { return 2 * (Nr + Nh + Nu) + (collar ? 4 * Nr : 0); }
  __host__ __device__ int items() const { return Nr + Nh + Nu + (collar ? 2 * Nr : 0); }
};

// cut layout: [ref start Nr][ref end Nr][hyp start Nh][hyp end Nh][uem start Nu][uem end Nu]
//             [collar lo 2 Nr][collar hi 2 Nr]   (collar u < Nr: around ref start u; u >= Nr: around ref end u - Nr)
__global__ __launch_bounds__(ANN_THREADS) void k_annot_cuts(const double* __restrict__ ref_seg,
                                                            const double* __restrict__ hyp_seg,
                                                            const double* __restrict__ uem_seg, AnnotShape sh,
                                                            double half_collar, double* __restrict__ cuts) {
  const int i = blockIdx.x * ANN_THREADS + threadIdx.x;
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

__global__ __launch_bounds__(ANN_THREADS) void k_annot_rank(const double* __restrict__ cuts, int M,
                                                            double* __restrict__ sorted, int* __restrict__ rank) {
  __shared__ double s_c[ANN_THREADS];
  const int tid = threadIdx.x, i = blockIdx.x * ANN_THREADS + tid;
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

__global__ __launch_bounds__(ANN_THREADS) void k_annot_intervals(
    const double* __restrict__ sorted, const int* __restrict__ rank, const int32_t* __restrict__ ref_label,
    const int32_t* __restrict__ hyp_label, AnnotShape sh, int Kr, int Kh, int skip_overlap,
    unsigned long long* __restrict__ rec_r, unsigned long long* __restrict__ rec_h, double* __restrict__ rec_d) {
  __shared__ unsigned long long s_rbit[ANN_THREADS], s_hbit[ANN_THREADS];
  __shared__ int s_lo[ANN_THREADS], s_hi[ANN_THREADS], s_flag[ANN_THREADS];
  const int tid = threadIdx.x, k = blockIdx.x * ANN_THREADS + tid;
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

// out: [cooc Kr*Kh][ref_dur Kr][hyp_dur Kh][total, false_alarm, missed, both, ref_speech, hyp_speech, both_speech]
__global__ __launch_bounds__(ANN_THREADS) void k_annot_reduce(const unsigned long long* __restrict__ rec_r,
                                                              const unsigned long long* __restrict__ rec_h,
                                                              const double* __restrict__ rec_d, int nint, int Kr,
                                                              int Kh, double* __restrict__ out) {
  __shared__ double s_part[ANN_THREADS / 64];
  const int tid = threadIdx.x, o = blockIdx.x;
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

static bool annot_cut_count(int Nr, int Nh, int Nu, bool collar, long* M) {
  if (Nr < 0 || Nh < 0 || Nu < 0) return false;
  *M = 2 * ((long)Nr + Nh + Nu) + (collar ? 4 * (long)Nr : 0);
  return *M <= ANN_MAX_CUTS;
}

// workspace: [cuts M f64][sorted M f64][rec_r M u64][rec_h M u64][rec_d M f64][rank M i32]
static size_t annot_workspace(long M) { return 256 + (size_t)M * (5 * 8 + 4); }

}  // namespace pa

extern "C" {

size_t pa_annot_counts_workspace_bytes(int Nr, int Nh, int Nu) {
  long M;
  if (!pa::annot_cut_count(Nr, Nh, Nu, true, &M)) return 0;
  return pa::annot_workspace(M);
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
  PA_REQUIRE(ws && ws_bytes >= pa::annot_workspace(M), "pa_annot_counts: workspace of %zu bytes, %zu needed",
             ws_bytes, pa::annot_workspace(M));
  hipStream_t s = (hipStream_t)stream;
  const pa::AnnotShape sh{Nr, Nh, Nu, with_collar ? 1 : 0};
  const int m = (int)M, nint = m > 0 ? m - 1 : 0;
  const int nout = Kr * Kh + Kr + Kh + pa::ANN_SCALARS;
  char* base = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  double* cuts = (double*)base;
  double* sorted = cuts + m;
  unsigned long long* rec_r = (unsigned long long*)(sorted + m);
  unsigned long long* rec_h = rec_r + m;
  double* rec_d = (double*)(rec_h + m);
  int* rank = (int*)(rec_d + m);
  pa::ProfScope prof("k_annot_counts", stream, 0.0, 44.0 * m + 8.0 * nout);
  if (nint > 0) {
    const int grid = pa::cdiv(m, pa::ANN_THREADS);
    hipLaunchKernelGGL(pa::k_annot_cuts, dim3(grid), dim3(pa::ANN_THREADS), 0, s, ref_seg, hyp_seg, uem_seg, sh,
                       0.5 * collar, cuts);
    hipLaunchKernelGGL(pa::k_annot_rank, dim3(grid), dim3(pa::ANN_THREADS), 0, s, cuts, m, sorted, rank);
    hipLaunchKernelGGL(pa::k_annot_intervals, dim3(pa::cdiv(nint, pa::ANN_THREADS)), dim3(pa::ANN_THREADS), 0, s,
                       sorted, rank, ref_label, hyp_label, sh, Kr, Kh, skip_overlap ? 1 : 0, rec_r, rec_h, rec_d);
  }
  // (without intervals the sums are empty: the kernel writes the zeros)
  hipLaunchKernelGGL(pa::k_annot_reduce, dim3(nout), dim3(pa::ANN_THREADS), 0, s, rec_r, rec_h, rec_d, nint, Kr, Kh,
                     out);
  PA_CHECK_LAUNCH("pa_annot_counts");
  return 0;
}

}  // extern "C"
