// Error counts of the reference's two frame-level diarization metrics, taken where the pipeline leaves its
// outputs (in HBM), in one pass, in integers.
//
// FILE MODE (utils/metric.py:41-93 `discrete_diarization_error_rate`): reference (T, Sr) and hypothesis (T, Sh)
// 0/1 arrays -> co-occurrence matrix, per-speaker frame counts and four scalars.  With Nr / Nh the number of
// reference / hypothesis speakers on in a frame,
//     total = sum Nr     false_alarm = sum max(0, Nh - Nr)     missed = sum max(0, Nr - Nh)     both = sum min(Nr, Nh)
// do not depend on the speaker mapping.  Under a one-to-one mapping pi (hypothesis speaker pi(i) plays reference
// speaker i; the shorter side padded with silent speakers, as the reference pads) let c be the number of speakers
// on in BOTH the mapped hypothesis h' and the reference r of a frame.  The reference's confusion of that frame is
//     sum_s (h' != r) * h'  -  false_alarm  =  (Nh - c) - max(0, Nh - Nr)  =  min(Nr, Nh) - c,
// and sum over frames of c = sum_i cooc[i][pi(i)] = `correct`.  So confusion = both - correct, and the mapping that
// the reference's `permutate` finds (minimal sum of mean squared differences; for 0/1 arrays
// mse[i][j] = (ref_frames[i] + hyp_frames[j] - 2 cooc[i][j]) / T, so minimal cost = maximal correct) is
// linear_sum_assignment(-cooc) on the host, on a matrix of at most 32 x 32.  Every optimum has the same `correct`.
//
// CHUNK MODE (torchmetrics/functional/audio/diarization_error_rate.py:33-162 `_der_update`): soft scores
// (B, S, F) against 0/1 targets, one workgroup per chunk: the chunk's scores and the per-frame target masks are
// staged in LDS once, the speaker permutation is found (S <= 4: all S! of them on the fp64 squared-error cost)
// or taken from the caller, and every wave sweeps the frames once per threshold it owns.  No (B, S, F, Q) array
// exists; the outputs are (B, Q, 3) + (B) int32, summed over the batch by k_der_sum into int64.
//
// All sums are integer: wave and workgroup partials in int32 (bounded below), then ONE 64-bit atomic per
// counter per workgroup.  Integer addition is order independent, so every result is exact and bit-reproducible.
#include <algorithm>

#include "common.h"
#include "pyannote_amd.h"

namespace pa {

constexpr int DER_THREADS = 256;
constexpr int DER_MAXS = 32;
constexpr int DER_MAXQ = 64;
constexpr int DER_AUTO_MAXS = 4;          // the kernel enumerates permutations itself up to here
constexpr int DER_MAX_GROUPS = 1024;      // workgroups of the file-mode kernel
constexpr int DER_WAVE_GROUPS = 8;        // 64-frame groups a wave takes before another workgroup is added
constexpr int DER_STAGE = 12288;          // 32-bit words of LDS for one chunk: S * F scores + F target masks

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

__device__ __forceinline__ uint32_t der_row_mask(const uint8_t* __restrict__ row, int S) {
  uint32_t m = 0;
  for (int s = 0; s < S; ++s) m |= (uint32_t)(row[s] != 0) << s;
  return m;
}

// out: [cooc Sr*Sh][ref_frames Sr][hyp_frames Sh][total, false_alarm, missed, both], zeroed by the launcher.
// A wave walks groups of 64 consecutive frames with all lanes in the loop (the ballots need them).  int32 partials:
// a workgroup sees at most 4 * (ceil(ngroups / (4 * gridDim.x))) groups; with T < 2^31 and DER_MAX_GROUPS
// workgroups once T is large that is < 2^21 + 256 frames, times at most 32 speakers: < 2^27.
__global__ __launch_bounds__(DER_THREADS) void k_der_counts(const uint8_t* __restrict__ ref,
                                                            const uint8_t* __restrict__ hyp,
                                                            const uint8_t* __restrict__ keep, long T, int Sr, int Sh,
                                                            unsigned long long* __restrict__ out) {
  __shared__ int s_cooc[DER_MAXS * DER_MAXS];
  __shared__ int s_ref[DER_MAXS], s_hyp[DER_MAXS], s_scal[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int p = tid; p < Sr * Sh; p += DER_THREADS) s_cooc[p] = 0;
  if (tid < DER_MAXS) s_ref[tid] = s_hyp[tid] = 0;
  if (tid < 4) s_scal[tid] = 0;
  __syncthreads();

  int total = 0, fa = 0, miss = 0, both = 0;
  const long ngroups = (T + 63) / 64;
  for (long g = (long)blockIdx.x * 4 + w; g < ngroups; g += (long)gridDim.x * 4) {
    const long t = g * 64 + lane;
    uint32_t r = 0, h = 0;
    if (t < T && (!keep || keep[t])) {
      r = der_row_mask(ref + t * Sr, Sr);
      h = der_row_mask(hyp + t * Sh, Sh);
    }
    const int nr = __popc(r), nh = __popc(h);
    total += nr;
    fa += max(0, nh - nr);
    miss += max(0, nr - nh);
    both += min(nr, nh);
    // only speakers that are on somewhere in these 64 frames cost a ballot
    const uint32_t ra = wave_or(r), ha = wave_or(h);
    for (uint32_t rb = ra; rb; rb &= rb - 1) {
      const int i = __ffs(rb) - 1;
      const uint32_t ri = (r >> i) & 1u;
      const unsigned long long bi = __ballot(ri);
      if (lane == 0) atomicAdd(&s_ref[i], __popcll(bi));
      for (uint32_t hb = ha; hb; hb &= hb - 1) {
        const int j = __ffs(hb) - 1;
        const unsigned long long bij = __ballot(ri & (h >> j) & 1u);
        if (lane == 0 && bij) atomicAdd(&s_cooc[i * Sh + j], __popcll(bij));
      }
    }
    for (uint32_t hb = ha; hb; hb &= hb - 1) {
      const int j = __ffs(hb) - 1;
      const unsigned long long bj = __ballot((h >> j) & 1u);
      if (lane == 0) atomicAdd(&s_hyp[j], __popcll(bj));
    }
  }
  total = wave_sum_i(total);
  fa = wave_sum_i(fa);
  miss = wave_sum_i(miss);
  both = wave_sum_i(both);
  if (lane == 0) {
    atomicAdd(&s_scal[0], total);
    atomicAdd(&s_scal[1], fa);
    atomicAdd(&s_scal[2], miss);
    atomicAdd(&s_scal[3], both);
  }
  __syncthreads();
  // one 64-bit atomic per (non-zero) counter per workgroup
  const int ncooc = Sr * Sh;
  for (int p = tid; p < ncooc; p += DER_THREADS)
    if (s_cooc[p]) atomicAdd(out + p, (unsigned long long)s_cooc[p]);
  if (tid < Sr && s_ref[tid]) atomicAdd(out + ncooc + tid, (unsigned long long)s_ref[tid]);
  if (tid < Sh && s_hyp[tid]) atomicAdd(out + ncooc + Sr + tid, (unsigned long long)s_hyp[tid]);
  if (tid < 4 && s_scal[tid]) atomicAdd(out + ncooc + Sr + Sh + tid, (unsigned long long)s_scal[tid]);
}

template <bool TF32>
__device__ __forceinline__ bool der_target_on(const void* __restrict__ target, long idx) {
  if (TF32) return ((const float*)target)[idx] != 0.f;
  return ((const uint8_t*)target)[idx] != 0;
}

// One workgroup per chunk.  AUTO: no permutation was passed and S <= DER_AUTO_MAXS.
template <bool TF32, bool AUTO>
__global__ __launch_bounds__(DER_THREADS) void k_der_chunks(const float* __restrict__ preds,
                                                            const void* __restrict__ target, int S, int F,
                                                            const float* __restrict__ thresholds, int Q,
                                                            const int32_t* __restrict__ perm,
                                                            int32_t* __restrict__ counts,
                                                            int32_t* __restrict__ total) {
  __shared__ uint32_t s_words[DER_STAGE];
  __shared__ double s_cost[4][DER_AUTO_MAXS * DER_AUTO_MAXS];
  __shared__ int s_perm[DER_MAXS];
  __shared__ int s_total[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long b = blockIdx.x;
  const float* __restrict__ P = preds + b * S * F;
  const long tbase = b * S * F;
  // scores [S][F] then target masks [F]; larger chunks are read again through the L2 instead
  const bool staged = (long)(S + 1) * F <= DER_STAGE;
  float* s_p = (float*)s_words;
  uint32_t* s_t = s_words + (staged ? S * F : 0);

  auto target_mask = [&](int f) {
    uint32_t m = 0;
    for (int s = 0; s < S; ++s) m |= (uint32_t)der_target_on<TF32>(target, tbase + (long)s * F + f) << s;
    return m;
  };

  // pass A: the chunk comes in from HBM once; speech total; fp64 squared-error cost of every (target i, score j) pair
  double cost[DER_AUTO_MAXS][DER_AUTO_MAXS];
  if (AUTO) {
#pragma unroll
    for (int i = 0; i < DER_AUTO_MAXS; ++i)
#pragma unroll
      for (int j = 0; j < DER_AUTO_MAXS; ++j) cost[i][j] = 0.0;
  }
  int ntot = 0;
  for (int f = tid; f < F; f += DER_THREADS) {
    const uint32_t tm = target_mask(f);
    ntot += __popc(tm);
    if (staged) s_t[f] = tm;
    if (AUTO) {
      float p[DER_AUTO_MAXS];
#pragma unroll
      for (int j = 0; j < DER_AUTO_MAXS; ++j) {
        p[j] = j < S ? P[(long)j * F + f] : 0.f;
        if (staged && j < S) s_p[j * F + f] = p[j];
      }
#pragma unroll
      for (int i = 0; i < DER_AUTO_MAXS; ++i)
#pragma unroll
        for (int j = 0; j < DER_AUTO_MAXS; ++j)
          if (i < S && j < S) {
            const double d = (double)((tm >> i) & 1u) - (double)p[j];
            cost[i][j] += d * d;
          }
    } else if (staged) {
      for (int j = 0; j < S; ++j) s_p[j * F + f] = P[(long)j * F + f];
    }
  }
  ntot = wave_sum_i(ntot);
  if (lane == 0) s_total[w] = ntot;
  if (AUTO) {
#pragma unroll
    for (int i = 0; i < DER_AUTO_MAXS; ++i)
#pragma unroll
      for (int j = 0; j < DER_AUTO_MAXS; ++j) {
        const double c = wave_sum_d(cost[i][j]);
        if (lane == 0) s_cost[w][i * DER_AUTO_MAXS + j] = c;
      }
  } else if (tid < S) {
    const int j = perm[b * S + tid];
    s_perm[tid] = (j >= 0 && j < S) ? j : -1;       // out of range: nobody plays this speaker (a silent hypothesis)
  }
  __syncthreads();
  if (tid == 0) total[b] = s_total[0] + s_total[1] + s_total[2] + s_total[3];
  if (AUTO) {
    if (tid == 0) {
      double c[DER_AUTO_MAXS * DER_AUTO_MAXS];
      for (int k = 0; k < DER_AUTO_MAXS * DER_AUTO_MAXS; ++k)
        c[k] = (s_cost[0][k] + s_cost[1][k]) + (s_cost[2][k] + s_cost[3][k]);
      // the cheapest of the S! permutations, the first in lexicographic order among equals: what `permutate`'s
      // Hungarian assignment minimises (the mean is the sum / F)
      int codes = 1;
      for (int i = 0; i < S; ++i) codes *= S;
      double best = 0.0;
      int best_code = -1;
      for (int code = 0; code < codes; ++code) {
        int rest = code, used = 0;
        double sum = 0.0;
        bool ok = true;
        for (int i = 0; i < S; ++i) {
          const int j = rest % S;
          rest /= S;
          if (used & (1 << j)) { ok = false; break; }
          used |= 1 << j;
          sum += c[i * DER_AUTO_MAXS + j];
        }
        if (ok && (best_code < 0 || sum < best)) { best = sum; best_code = code; }
      }
      if (best_code < 0) best_code = 0;               // (all costs NaN: nothing compared smaller)
      for (int i = 0; i < S; ++i) {
        s_perm[i] = best_code % S;
        best_code /= S;
      }
    }
    __syncthreads();
  }

  // pass B: wave w owns thresholds w, w + 4, ...; hypothesis = score > threshold, a float32 comparison
  for (int q = w; q < Q; q += 4) {
    const float thr = thresholds[q];
    int fa = 0, miss = 0, conf = 0;
    for (int f = lane; f < F; f += 64) {
      const uint32_t tm = staged ? s_t[f] : target_mask(f);
      uint32_t hm = 0;
      for (int i = 0; i < S; ++i) {
        const int j = s_perm[i];
        const float p = j < 0 ? 0.f : (staged ? s_p[j * F + f] : P[(long)j * F + f]);
        hm |= (uint32_t)(p > thr) << i;
      }
      const int nr = __popc(tm), nh = __popc(hm);
      fa += max(0, nh - nr);
      miss += max(0, nr - nh);
      conf += min(nr, nh) - __popc(tm & hm);
    }
    fa = wave_sum_i(fa);
    miss = wave_sum_i(miss);
    conf = wave_sum_i(conf);
    if (lane == 0) {
      int32_t* o = counts + (b * Q + q) * 3;
      o[0] = fa;
      o[1] = miss;
      o[2] = conf;
    }
  }
}

// out (3 Q + 1) int64 += column sums of counts (B, 3 Q) and of total (B): 64 columns x 256 rows per workgroup
__global__ __launch_bounds__(DER_THREADS) void k_der_sum(const int32_t* __restrict__ counts,
                                                         const int32_t* __restrict__ total, int B, int ncols,
                                                         unsigned long long* __restrict__ out) {
  __shared__ long long s_part[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
  const int r1 = min(B, (int)(blockIdx.y + 1) * 256);
  long long acc = 0;
  if (c <= ncols)
    for (int r = blockIdx.y * 256 + g; r < r1; r += 4) acc += c < ncols ? counts[(long)r * ncols + c] : total[r];
  s_part[g][threadIdx.x & 63] = acc;
  __syncthreads();
  if (g == 0 && c <= ncols) {
    const int l = threadIdx.x;
    const long long sum = s_part[0][l] + s_part[1][l] + s_part[2][l] + s_part[3][l];
    if (sum) atomicAdd(out + c, (unsigned long long)sum);
  }
}

}  // namespace pa

extern "C" {

int pa_der_counts(const uint8_t* ref, const uint8_t* hyp, const uint8_t* keep, long T, int Sr, int Sh,
                  int64_t* out, void* stream) {
  PA_REQUIRE(Sr >= 1 && Sr <= pa::DER_MAXS && Sh >= 1 && Sh <= pa::DER_MAXS,
             "pa_der_counts: %d reference and %d hypothesis speakers, 1..%d each supported", Sr, Sh, pa::DER_MAXS);
  PA_REQUIRE(T >= 0 && T <= 0x7fffffffL, "pa_der_counts: %ld frames, 0..2^31-1 supported", T);
  PA_REQUIRE(out && (T == 0 || (ref && hyp)), "pa_der_counts: null array");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)Sr * Sh + Sr + Sh + 4;
  if (pa::fill_async(out, 0, sizeof(int64_t) * n, s) != hipSuccess) {
    pa::set_error("pa_der_counts: the fill launch failed");
    return 1;
  }
  if (T == 0) return 0;
  const long ngroups = (T + 63) / 64;
  const int grid = std::min(pa::DER_MAX_GROUPS, pa::cdiv(ngroups, 4 * pa::DER_WAVE_GROUPS));
  pa::ProfScope prof("k_der_counts", stream, 0.0, (double)T * (Sr + Sh + (keep ? 1 : 0)) + 8.0 * n);
  hipLaunchKernelGGL(pa::k_der_counts, dim3(grid), dim3(pa::DER_THREADS), 0, s, ref, hyp, keep, T, Sr, Sh,
                     (unsigned long long*)out);
  PA_CHECK_LAUNCH("pa_der_counts");
  return 0;
}

int pa_der_chunks(const float* preds, const void* target, int target_is_f32, int B, int S, int F,
                  const float* thresholds, int Q, const int32_t* perm, int32_t* counts, int32_t* total,
                  void* stream) {
  PA_REQUIRE(S >= 1 && S <= pa::DER_MAXS, "pa_der_chunks: %d speakers, 1..%d supported", S, pa::DER_MAXS);
  PA_REQUIRE(Q >= 1 && Q <= pa::DER_MAXQ, "pa_der_chunks: %d thresholds, 1..%d supported", Q, pa::DER_MAXQ);
  PA_REQUIRE(perm || S <= pa::DER_AUTO_MAXS,
             "pa_der_chunks: %d speakers need a permutation from the caller (the kernel finds its own up to %d)", S,
             pa::DER_AUTO_MAXS);
  PA_REQUIRE(B >= 0 && F >= 1 && (long)S * F <= 0x7fffffffL / 32, "pa_der_chunks: bad batch size or frame count");
  PA_REQUIRE(B == 0 || (preds && target && thresholds && counts && total), "pa_der_chunks: null array");
  if (B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  pa::ProfScope prof("k_der_chunks", stream, 0.0,
                     (double)B * S * F * (4.0 + (target_is_f32 ? 4.0 : 1.0)) + 4.0 * B * (3.0 * Q + 1.0));
#define PA_DER_LAUNCH(TF, AUTO)                                                                            \
  hipLaunchKernelGGL((pa::k_der_chunks<TF, AUTO>), dim3(B), dim3(pa::DER_THREADS), 0, s, preds, target, S, F, \
                     thresholds, Q, perm, counts, total)
  if (target_is_f32) {
    if (perm) PA_DER_LAUNCH(true, false); else PA_DER_LAUNCH(true, true);
  } else {
    if (perm) PA_DER_LAUNCH(false, false); else PA_DER_LAUNCH(false, true);
  }
#undef PA_DER_LAUNCH
  PA_CHECK_LAUNCH("pa_der_chunks");
  return 0;
}

size_t pa_der_chunks_workspace_bytes(int B, int Q) {
  if (B < 0 || Q < 1) return 0;
  return sizeof(int32_t) * (size_t)B * (3 * (size_t)Q + 1);
}

int pa_der_chunks_sum(const int32_t* counts, const int32_t* total, int B, int Q, int64_t* out, void* stream) {
  PA_REQUIRE(Q >= 1 && Q <= pa::DER_MAXQ && B >= 0, "pa_der_chunks_sum: bad B or Q");
  PA_REQUIRE(out && (B == 0 || (counts && total)), "pa_der_chunks_sum: null array");
  hipStream_t s = (hipStream_t)stream;
  const int ncols = 3 * Q;
  if (pa::fill_async(out, 0, sizeof(int64_t) * (ncols + 1), s) != hipSuccess) {
    pa::set_error("pa_der_chunks_sum: the fill launch failed");
    return 1;
  }
  if (B == 0) return 0;
  pa::ProfScope prof("k_der_sum", stream, 0.0, 4.0 * B * (ncols + 1.0));
  hipLaunchKernelGGL(pa::k_der_sum, dim3(pa::cdiv(ncols + 1, 64), pa::cdiv(B, 256)), dim3(pa::DER_THREADS), 0, s,
                     counts, total, B, ncols, (unsigned long long*)out);
  PA_CHECK_LAUNCH("pa_der_chunks_sum");
  return 0;
}

}  // extern "C"
