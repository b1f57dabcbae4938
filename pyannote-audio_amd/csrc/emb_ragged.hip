// Ragged batches of the WeSpeaker forward (pa_emb_forward_ragged, emb_forward.cpp): utterances of different lengths
// share one launch sequence over a map padded to the longest of them.
//
//   k_zero_tail          zero columns [Wv_b, W) of every row of utterance b of an NHWC map (H = mel rows, W = time
//                        columns): one contiguous run of (W - Wv_b) * C floats per row, written with 128-bit stores,
//                        so the traffic is that of the padding only.
//   k_stats_pool_ragged  the weighted statistics pooling of k_stats_pool (emb_pool.hip) over each utterance's own
//                        Wv_b valid columns, with optional weights given at pool resolution; no limit on the length.
//
// Wv_b follows make_plan (emb_forward.cpp): T_b = 1 + (N_b - 400) / 160 fbank frames, then (W - 1) / 2 + 1 per
// stride-2 layer (`halvings` of them).
#include "common.h"

namespace pa {

__device__ __forceinline__ int ragged_columns(int num_samples, int halvings) {
  int w = num_samples < 400 ? 0 : 1 + (num_samples - 400) / 160;
  for (int i = 0; i < halvings; ++i) w = (w - 1) / 2 + 1;
  return w;
}

// grid = (H, B), block = 256
__global__ __launch_bounds__(256) void k_zero_tail(float* __restrict__ x, int H, int W, int C,
                                                   const int* __restrict__ lens, int halvings) {
  const int b = blockIdx.y, h = blockIdx.x;
  const int wv = ragged_columns(lens[b], halvings);
  if (wv >= W) return;
  const long n4 = (long)(W - wv) * C / 4;
  float4* row = reinterpret_cast<float4*>(x + (((long)b * H + h) * W + wv) * C);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long i = threadIdx.x; i < n4; i += 256) row[i] = z;
}

constexpr int PR_TILE = 512;   // pool columns whose weights are staged in LDS at a time
constexpr int PR_LD = 16;      // time steps whose loads are in flight together

// feat[b][f][t][c] (t < W, valid t < Wv_b), weights masks[b][t] (ld_masks per row) or 1 -> stats[b][2 D] with
// D = C * Fh, d = c * Fh + f: mean | std, the formula of k_stats_pool (0/1 weights: the unbiased std up to rounding).
// grid = (ceil(C / 256), Fh, B), block = 256
__global__ __launch_bounds__(256) void k_stats_pool_ragged(const float* __restrict__ feat, int Fh, int W, int C,
                                                           const int* __restrict__ lens, int halvings,
                                                           const float* __restrict__ masks, int ld_masks,
                                                           float* __restrict__ stats) {
  __shared__ float ws[PR_TILE];
  __shared__ float v1s, dens;
  const int b = blockIdx.z, f = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  int Tv = ragged_columns(lens[b], halvings);
  if (Tv > W) Tv = W;
  const float* x = feat + (((long)b * Fh + f) * W) * C + (c < C ? c : 0);
  const float* mrow = masks != nullptr ? masks + (long)b * ld_masks : nullptr;
  double a = 0.0, q = 0.0;                    // the weight sums in double, as in k_stats_pool
  float m = 0.f, mc = 0.f, v = 0.f;           // mc: Kahan compensation of m, as in k_stats_pool
  // pass 0: weighted sum (+ the weight sums, in column order as k_stats_pool adds them); pass 1: weighted squares
  for (int pass = 0; pass < 2; ++pass) {
    for (int t0 = 0; t0 < Tv; t0 += PR_TILE) {
      const int n = Tv - t0 < PR_TILE ? Tv - t0 : PR_TILE;
      __syncthreads();
      for (int i = threadIdx.x; i < n; i += 256) ws[i] = mrow != nullptr ? mrow[t0 + i] : 1.f;
      __syncthreads();
      if (pass == 0 && threadIdx.x == 0)
        for (int t = 0; t < n; ++t) {
          const double w = (double)ws[t];
          a += w;
          q += w * w;
        }
      if (c < C) {
        for (int u0 = 0; u0 < n; u0 += PR_LD) {
          float xb[PR_LD];
#pragma unroll
          for (int u = 0; u < PR_LD; ++u) xb[u] = u0 + u < n ? x[(long)(t0 + u0 + u) * C] : 0.f;
#pragma unroll
          for (int u = 0; u < PR_LD; ++u)
            if (u0 + u < n) {
              if (pass == 0) {
                const float y = fmaf(xb[u], ws[u0 + u], -mc);
                const float t = m + y;
                mc = (t - m) - y;
                m = t;
              } else {
                const float d = xb[u] - m;
                v = fmaf(d * d, ws[u0 + u], v);
              }
            }
        }
      }
    }
    if (pass == 0) {
      if (threadIdx.x == 0) {
        const double v1 = a + 1e-8;
        v1s = (float)v1;
        dens = (float)(v1 - q / v1 + 1e-8);
      }
      __syncthreads();
      m /= v1s;
    }
  }
  if (c >= C) return;
  const int D = C * Fh;
  const int d = c * Fh + f;
  float* o = stats + (long)b * 2 * D;
  o[d] = m;
  o[D + d] = sqrtf(v / dens);
}

}  // namespace pa

extern "C" {

int pa_zero_tail_cols(float* x, int B, int H, int W, int C, const int32_t* lengths, int halvings, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  PA_REQUIRE(C > 0 && C % 4 == 0 && ((uintptr_t)x & 15) == 0 && halvings >= 0,
             "pa_zero_tail_cols: C must be a multiple of 4 and the map 16-byte aligned (C = %d)", C);
  pa::ProfScope prof("k_zero_tail", stream, 0.0, 0.0);
  hipLaunchKernelGGL(pa::k_zero_tail, dim3(H, B), dim3(256), 0, (hipStream_t)stream, x, H, W, C,
                     (const int*)lengths, halvings);
  PA_CHECK_LAUNCH("pa_zero_tail_cols");
  return 0;
}

int pa_stats_pool_ragged(const float* feat, int B, int Fh, int W, int C, const int32_t* lengths, int halvings,
                         const float* masks, int ld_masks, float* stats, void* stream) {
  if (B <= 0) return 0;
  PA_REQUIRE(Fh >= 1 && W >= 1 && C >= 1 && halvings >= 0 && (masks == nullptr || ld_masks >= W),
             "pa_stats_pool_ragged: bad geometry (Fh %d, W %d, C %d, ld_masks %d)", Fh, W, C, ld_masks);
  pa::ProfScope prof("k_stats_pool_ragged", stream, 6.0 * B * C * Fh * W, 8.0 * B * C * Fh * W + 8.0 * B * C * Fh);
  hipLaunchKernelGGL(pa::k_stats_pool_ragged, dim3(pa::cdiv(C, 256), Fh, B), dim3(256), 0, (hipStream_t)stream, feat,
                     Fh, W, C, (const int*)lengths, halvings, masks, ld_masks, stats);
  PA_CHECK_LAUNCH("pa_stats_pool_ragged");
  return 0;
}

}  // extern "C"
