// hipcc-flags of every file that includes this: -ffp-contract=off (the times below are bit-identical to the host)
// Device functions shared by the region kernels (regions.hip: one detector per class; regions_sweep.hip: many
// detectors per class): map composition, the wave scans, frame middles and Segment.duration.
#pragma once
#include "common.h"

namespace pa {

constexpr int RG_THREADS = 256;
constexpr int RG_PASSES = 4;
constexpr int RG_TILE = RG_THREADS * RG_PASSES;   // frames per workgroup
constexpr int RG_CHUNK = 64;                      // frames per wave and pass
constexpr int RG_MAXK = 16;
constexpr uint32_t RG_IDENTITY = 0xffff0000u;     // inactive -> inactive, active -> active
constexpr double RG_PRECISION = 1e-6;             // pyannote.core SEGMENT_PRECISION

struct RegionParams {
  float onset[RG_MAXK], offset[RG_MAXK];
  double min_on[RG_MAXK], min_off[RG_MAXK];
  double start, duration, step;
};

// map of "a, then b"
__device__ __forceinline__ uint32_t rg_compose(uint32_t a, uint32_t b) {
  const uint32_t a0 = a & 0xffffu, a1 = a >> 16, b0 = b & 0xffffu, b1 = b >> 16;
  const uint32_t c0 = (a0 & b1) | (~a0 & b0), c1 = (a1 & b1) | (~a1 & b0);
  return (c0 & 0xffffu) | (c1 << 16);
}

// the maps of frame i (identity past the end).  Frame 0 sets the state: `is_active = y > onset`, a constant map.
__device__ __forceinline__ uint32_t rg_frame_map(const float* __restrict__ scores, long i, int T, int K,
                                                 const RegionParams& p) {
  if (i >= T) return RG_IDENTITY;
  const float* row = scores + i * K;
  uint32_t f0 = 0, f1 = 0;
#pragma unroll
  for (int k = 0; k < RG_MAXK; ++k)
    if (k < K) {
      const float y = row[k];                       // NaN: both comparisons false -> identity
      f0 |= (uint32_t)(y > p.onset[k]) << k;
      f1 |= (uint32_t)(!(y < p.offset[k])) << k;
    }
  if (i == 0) f1 = f0;
  return f0 | (f1 << 16);
}

__device__ __forceinline__ uint32_t rg_wave_scan(uint32_t m, int lane) {   // inclusive
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t prev = __shfl_up(m, o, 64);
    if (lane >= o) m = rg_compose(prev, m);
  }
  return m;
}

__device__ __forceinline__ int rg_wave_scan_int(int v, int lane) {         // inclusive
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int prev = __shfl_up(v, o, 64);
    if (lane >= o) v += prev;
  }
  return v;
}

__device__ __forceinline__ double rg_time(long i, const RegionParams& p) {
  const double s = __dadd_rn(p.start, __dmul_rn((double)i, p.step));
  return __dmul_rn(0.5, __dadd_rn(s, __dadd_rn(s, p.duration)));
}

// inclusive block scan of 0/1 flags; `red` holds 4 ints; returns the block total in `total`
__device__ __forceinline__ int rg_block_scan_int(int v, int* red, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = rg_wave_scan_int(v, lane);
  __syncthreads();
  if (lane == 63) red[w] = inc;
  __syncthreads();
  int pre = 0, sum = 0;
  for (int j = 0; j < 4; ++j) {
    if (j == w) pre = sum;
    sum += red[j];
  }
  total = sum;
  return inc + pre;
}

// pyannote.core Segment.duration: 0 for segments not longer than the precision
__device__ __forceinline__ double rg_duration(double s, double e) {
  const double d = e - s;
  return d > RG_PRECISION ? d : 0.0;
}

}  // namespace pa
