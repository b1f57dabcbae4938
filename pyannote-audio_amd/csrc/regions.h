// hipcc-flags of every file that includes this: -ffp-contract=off (the times below are bit-identical to the host)
// The hysteresis region rule, every step written once.  regions.hip (one detector per class) and regions_sweep.hip
// (many detectors per class) wrap these bodies in their kernels, which is what makes their bits equal.
//
// The rule is state dependent: inactive -> active iff y > onset, active -> inactive iff y < offset.  Every frame is
// therefore one of four maps on {inactive, active} (identity, set, clear, swap; swap needs offset > onset), and the
// state sequence is a prefix scan under map composition, which is associative.  A map is two bits (image of
// "inactive", image of "active"); the maps of up to 16 detectors (SLOTS) of one frame travel in one 32-bit word (low
// half: images of "inactive", high half: images of "active") and compose bitwise, so one scan serves every slot.
//
// The steps, one launch each (NO workgroup ever waits for another one):
//   rg_reduce_tile     workgroup = tile of 1024 frames: composed map of the tile
//   rg_scan_tiles      one wave: exclusive scan of the tile maps -> state on entry of every tile
//   rg_apply_tile      workgroup = tile: states, on / off events per frame, number of on-events per 64-frame chunk
//   rg_scan_counts     one wave per slot: exclusive scan of the chunk counts
//   rg_emit_events     the n-th on-event and the n-th off-event of a slot are its region n
//   rg_drop_empty, rg_merge_gaps, rg_drop_short   one workgroup per region list: order-preserving compactions
// What a frame's map is made from, and where a frame lies in its file, are the things a step can be generic over: a
// MAP type provides `frame_map(scores, i, T, K)` and the three questions of RegionOneFile below (RegionParams here,
// SweepGroup in regions_sweep.hip: rows 0 .. T - 1 are one file; RegionFiles in regions_files.hip: the rows are the
// concatenation of many files, each with a first frame, a last frame and times of its own).  Everything else that
// differs between the callers is an argument.
// Times are float64 and bit-identical to the host's `0.5 * (s + (s + duration))`, `s = start + i * step`: the files are
// compiled without FMA contraction and the products / sums are the _rn intrinsics.
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

// where row i of the scores lies when rows 0 .. T - 1 are ONE file: the part of a MAP type that is the same for every
// caller whose rows are one file
struct RegionOneFile {
  __device__ __forceinline__ bool first_frame(long i, int) const { return i == 0; }      // no state comes before it
  __device__ __forceinline__ bool last_frame(long i, int T) const { return i == T - 1; } // closes what is open
  __device__ __forceinline__ bool no_frame(long i, int T) const { return i >= T; }       // past the end: no event
  __device__ __forceinline__ long time_frame(long i) const { return i; }                 // the index its time is of
};

// slot k = class k = column k of the scores
struct RegionParams : RegionOneFile {
  float onset[RG_MAXK], offset[RG_MAXK];
  double min_on[RG_MAXK], min_off[RG_MAXK];
  double start, duration, step;

  // the maps of one frame, `row` its K scores.  A first frame sets the state: `is_active = y > onset`, a constant map.
  __device__ __forceinline__ uint32_t row_map(const float* __restrict__ row, int K, bool first) const {
    uint32_t f0 = 0, f1 = 0;
#pragma unroll
    for (int k = 0; k < RG_MAXK; ++k)
      if (k < K) {
        const float y = row[k];                       // NaN: both comparisons false -> identity
        f0 |= (uint32_t)(y > onset[k]) << k;
        f1 |= (uint32_t)(!(y < offset[k])) << k;
      }
    if (first) f1 = f0;
    return f0 | (f1 << 16);
  }

  // the maps of frame i (identity past the end)
  __device__ __forceinline__ uint32_t frame_map(const float* __restrict__ scores, long i, int T, int K) const {
    if (i >= T) return RG_IDENTITY;
    return row_map(scores + i * K, K, i == 0);
  }
};

// map of "a, then b"
__device__ __forceinline__ uint32_t rg_compose(uint32_t a, uint32_t b) {
  const uint32_t a0 = a & 0xffffu, a1 = a >> 16, b0 = b & 0xffffu, b1 = b >> 16;
  const uint32_t c0 = (a0 & b1) | (~a0 & b0), c1 = (a1 & b1) | (~a1 & b0);
  return (c0 & 0xffffu) | (c1 << 16);
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

// the middle of frame i
__device__ __forceinline__ double rg_time(long i, double start, double duration, double step) {
  const double s = __dadd_rn(start, __dmul_rn((double)i, step));
  return __dmul_rn(0.5, __dadd_rn(s, __dadd_rn(s, duration)));
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

// ------------------------------------------------------------------------------------------ the steps, frame domain
// workgroup blockIdx.x: the composed map of its tile -> tile_map[blockIdx.x]
template <class Map>
__device__ __forceinline__ void rg_reduce_tile(const float* __restrict__ scores, int T, int K, const Map& f,
                                               uint32_t* __restrict__ tile_map) {
  __shared__ uint32_t part[RG_PASSES * 4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long t0 = (long)blockIdx.x * RG_TILE;
#pragma unroll
  for (int q = 0; q < RG_PASSES; ++q) {
    const uint32_t m = rg_wave_scan(f.frame_map(scores, t0 + q * RG_THREADS + threadIdx.x, T, K), lane);
    if (lane == 63) part[q * 4 + w] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t m = part[0];
    for (int j = 1; j < RG_PASSES * 4; ++j) m = rg_compose(m, part[j]);
    tile_map[blockIdx.x] = m;
  }
}

// one wave: state_in[t] = the states on entry of tile t
__device__ __forceinline__ void rg_scan_tiles(const uint32_t* __restrict__ tile_map, int ntiles,
                                              uint32_t* __restrict__ state_in) {
  const int lane = threadIdx.x;
  uint32_t carry = RG_IDENTITY;
  for (int base = 0; base < ntiles; base += 64) {
    const int t = base + lane;
    const uint32_t inc = rg_wave_scan(t < ntiles ? tile_map[t] : RG_IDENTITY, lane);
    uint32_t exc = __shfl_up(inc, 1, 64);
    if (lane == 0) exc = RG_IDENTITY;
    // frame 0 is a constant map, so the image of "inactive" is the state whatever came before
    if (t < ntiles) state_in[t] = rg_compose(carry, exc) & 0xffffu;
    carry = rg_compose(carry, __shfl(inc, 63, 64));
  }
}

// workgroup blockIdx.x, `state`: the states before its tile's first frame.  events[i] (unless `events` is NULL: only
// the counts are wanted) = on-events | off-events << 16 of frame i; chunk_cnt[k * nchunks + c] = on-events of slot
// k < slots in chunk c
template <class Map>
__device__ __forceinline__ void rg_apply_tile(const float* __restrict__ scores, int T, int K, const Map& f, int slots,
                                              uint32_t state, uint32_t* __restrict__ events,
                                              int* __restrict__ chunk_cnt, int nchunks) {
  __shared__ uint32_t part[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long t0 = (long)blockIdx.x * RG_TILE;
  for (int q = 0; q < RG_PASSES; ++q) {
    const long i = t0 + q * RG_THREADS + threadIdx.x;
    const uint32_t m = f.frame_map(scores, i, T, K);
    const uint32_t inc = rg_wave_scan(m, lane);
    __syncthreads();                                // `part` of the previous pass has been read
    if (lane == 63) part[w] = inc;
    __syncthreads();
    uint32_t exc = __shfl_up(inc, 1, 64);
    if (lane == 0) exc = RG_IDENTITY;
    uint32_t pre = RG_IDENTITY, total = part[0];
    for (int j = 1; j < 4; ++j) {
      if (j == w) pre = total;
      total = rg_compose(total, part[j]);
    }
    if (w == 0) pre = RG_IDENTITY;
    exc = rg_compose(pre, exc);
    uint32_t before = ((state & (exc >> 16)) | (~state & exc)) & 0xffffu;
    if (f.first_frame(i, T)) before = 0;   // (what frame 0 finds anyway; the state a previous file was left in)
    const uint32_t after = ((before & (m >> 16)) | (~before & m)) & 0xffffu;
    uint32_t on = ~before & after & 0xffffu, off = before & ~after;
    if (f.last_frame(i, T)) {   // a region still open closes on the last frame; one that would open there is empty
      off = before;
      on = 0;
    }
    if (f.no_frame(i, T)) on = off = 0;
    if (events && i < T) events[i] = on | (off << 16);
    const int chunk = blockIdx.x * (RG_TILE / RG_CHUNK) + q * 4 + w;
#pragma unroll
    for (int k = 0; k < RG_MAXK; ++k)
      if (k < slots) {
        const unsigned long long b = __ballot((on >> k) & 1u);
        if (lane == k && chunk < nchunks) chunk_cnt[(long)k * nchunks + chunk] = __popcll(b);
      }
    state = ((state & (total >> 16)) | (~state & total)) & 0xffffu;
  }
}

// one wave: off[c] = cnt[0] + ... + cnt[c - 1]; returns the sum of all n (in every lane)
__device__ __forceinline__ int rg_scan_counts(const int* __restrict__ cnt, int n, int* __restrict__ off) {
  const int lane = threadIdx.x & 63;
  int carry = 0;
  for (int base = 0; base < n; base += 64) {
    const int c = base + lane;
    const int v = c < n ? cnt[c] : 0;
    const int inc = rg_wave_scan_int(v, lane);
    if (c < n) off[c] = carry + inc - v;
    carry += __shfl(inc, 63, 64);
  }
  return carry;
}

// the region list of a slot: rows first .. first + room - 1 of `raw`
struct RegionRows {
  long first;
  int room;
};

// On- and off-events of a slot alternate, starting with an on-event: region n runs from the n-th on-event to the
// n-th off-event, and the off-event's n is (number of on-events up to and including its frame) - 1.
// `events`, `chunk_off`: as rg_apply_tile and rg_scan_counts left them (`nchunks`: the entries between two slots of
// `chunk_off`).  `f.time_frame(i)`: the frame index the time of row i is computed from.  `rows_of(k)`: the RegionRows
// of slot k, asked for by the lanes that hold one of its events only.
template <class Map, class RowsOf>
__device__ __forceinline__ void rg_emit_events(const uint32_t* __restrict__ events, int T, int slots, const Map& f,
                                               double start, double duration, double step,
                                               const int* __restrict__ chunk_off, int nchunks, RowsOf rows_of,
                                               double* __restrict__ raw) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * RG_THREADS + threadIdx.x;
  const int chunk = (int)(i >> 6);
  const uint32_t ev = i < T ? events[i] : 0u;
  if (__ballot(ev != 0u) == 0ull) return;
  const double t = rg_time(f.time_frame(i), start, duration, step);
  const unsigned long long upto = ~0ull >> (63 - lane);   // lanes 0..lane
#pragma unroll
  for (int k = 0; k < RG_MAXK; ++k)
    if (k < slots) {
      const unsigned long long b = __ballot((ev >> k) & 1u);
      if ((ev >> k) & 0x10001u) {
        const RegionRows rows = rows_of(k);
        const int n = chunk_off[(long)k * nchunks + chunk] + __popcll(b & upto) - 1;
        if (n >= 0 && n < rows.room) {
          double* r = raw + (rows.first + n) * 2;
          if ((ev >> k) & 1u) r[0] = t;
          if ((ev >> (16 + k)) & 1u) r[1] = t;
        }
      }
    }
}

// ----------------------------------------------------------------------------------------- the steps, region domain
// One workgroup over one sorted region list, `in` (n rows) -> `out`, order preserved; `red` holds 4 ints of LDS; each
// returns the number of rows it kept.  A caller that reads `out` next puts a __syncthreads() in between.

// drops the regions the reference's Annotation refuses on insertion (duration <= 1e-6)
__device__ __forceinline__ int rg_drop_empty(const double* __restrict__ in, int n, double* __restrict__ out,
                                             int* red) {
  int total, kept = 0;
  for (int base = 0; base < n; base += RG_THREADS) {
    const int i = base + threadIdx.x;
    double s = 0.0, e = 0.0;
    if (i < n) { s = in[2 * i]; e = in[2 * i + 1]; }
    const int keep = i < n && (e - s) > RG_PRECISION;
    const int pos = kept + rg_block_scan_int(keep, red, total) - 1;
    if (keep) { out[2 * pos] = s; out[2 * pos + 1] = e; }
    kept += total;
  }
  return kept;
}

// merges neighbours whose gap has Segment.duration < min_off (Annotation.support(collar))
__device__ __forceinline__ int rg_merge_gaps(const double* __restrict__ in, int n, double min_off,
                                             double* __restrict__ out, int* red) {
  int total, kept = 0;
  for (int base = 0; base < n; base += RG_THREADS) {
    const int i = base + threadIdx.x;
    int head = 0, tail = 0;
    double s = 0.0, e = 0.0;
    if (i < n) {
      s = in[2 * i]; e = in[2 * i + 1];
      head = i == 0 || !(min_off > 0.0 && rg_duration(in[2 * i - 1], s) < min_off);
      tail = i == n - 1 || !(min_off > 0.0 && rg_duration(e, in[2 * i + 2]) < min_off);
    }
    const int run = kept + rg_block_scan_int(head, red, total) - 1;
    if (head) out[2 * run] = s;
    if (tail) out[2 * run + 1] = e;
    kept += total;
  }
  return kept;
}

// drops regions with duration < min_on and records every survivor's index among the merged regions (its track name)
// in `tracks` (may be NULL).  `out` and `tracks` have room for `room` rows; nothing is written past them.
__device__ __forceinline__ int rg_drop_short(const double* __restrict__ in, int n, double min_on, double min_off,
                                             int room, double* __restrict__ out, int* __restrict__ tracks,
                                             int* red) {
  int total, kept = 0;
  for (int base = 0; base < n; base += RG_THREADS) {
    const int i = base + threadIdx.x;
    double s = 0.0, e = 0.0;
    if (i < n) { s = in[2 * i]; e = in[2 * i + 1]; }
    const int keep = i < n && !(min_on > 0.0 && rg_duration(s, e) < min_on);
    const int pos = kept + rg_block_scan_int(keep, red, total) - 1;
    if (keep && pos < room) {
      out[2 * pos] = s;
      out[2 * pos + 1] = e;
      if (tracks) tracks[pos] = min_off > 0.0 ? i : 0;   // support() renames tracks; without it all are the first name
    }
    kept += total;
  }
  return kept;
}

}  // namespace pa
