// hipcc-flags: -ffp-contract=off
// Hysteresis thresholding of an aggregated (T, K) score array into per-class region lists, on the device
// (what utils/signal.py:254-318 `Binarize.__call__` does to every class of a multi-label model, followed by
// `Annotation.support(collar)` and the min_duration_on deletion).
//
// The reference's rule is state dependent: inactive -> active iff y > onset, active -> inactive iff y < offset.
// Every frame is therefore one of four maps on {inactive, active} (identity, set, clear, swap; swap needs
// offset > onset), and the state sequence is a prefix scan under map composition, which is associative.  A map
// is two bits (image of "inactive", image of "active"); the maps of all K <= 16 classes of one frame travel in
// one 32-bit word (low half: images of "inactive", high half: images of "active") and compose bitwise, so one
// scan serves every class.
//
// Launch sequence (each kernel ends before the next starts; NO workgroup ever waits for another one):
//   k_regions_reduce   one workgroup per tile of 1024 frames: composed map of the tile
//   k_regions_scan     one wave: exclusive scan of the tile maps -> state on entry of every tile
//   k_regions_apply    per tile: states, on / off events per frame, number of on-events per 64-frame chunk
//   k_regions_offsets  one wave per class: exclusive scan of the chunk counts
//   k_regions_emit     per chunk: the n-th on-event and the n-th off-event of a class are region n
//   k_regions_finish   one workgroup per class: drop empty regions, merge across short gaps, drop short regions
// Times are float64 and bit-identical to the host's `0.5 * (s + (s + duration))`, `s = start + i * step`: this
// file is compiled without FMA contraction and the products / sums are the _rn intrinsics.
#include "common.h"
#include "pyannote_amd.h"
#include "regions.h"

namespace pa {

__global__ __launch_bounds__(RG_THREADS) void k_regions_reduce(const float* __restrict__ scores, int T, int K,
                                                               RegionParams p, uint32_t* __restrict__ tile_map) {
  __shared__ uint32_t part[RG_PASSES * 4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long t0 = (long)blockIdx.x * RG_TILE;
#pragma unroll
  for (int q = 0; q < RG_PASSES; ++q) {
    const uint32_t m = rg_wave_scan(rg_frame_map(scores, t0 + q * RG_THREADS + threadIdx.x, T, K, p), lane);
    if (lane == 63) part[q * 4 + w] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t m = part[0];
    for (int j = 1; j < RG_PASSES * 4; ++j) m = rg_compose(m, part[j]);
    tile_map[blockIdx.x] = m;
  }
}

__global__ __launch_bounds__(64) void k_regions_scan(const uint32_t* __restrict__ tile_map, int ntiles,
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

__global__ __launch_bounds__(RG_THREADS) void k_regions_apply(const float* __restrict__ scores, int T, int K,
                                                              RegionParams p,
                                                              const uint32_t* __restrict__ state_in,
                                                              uint32_t* __restrict__ events,
                                                              int* __restrict__ chunk_cnt, int nchunks) {
  __shared__ uint32_t part[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long t0 = (long)blockIdx.x * RG_TILE;
  uint32_t state = state_in[blockIdx.x];            // state of every class before the pass's first frame
  for (int q = 0; q < RG_PASSES; ++q) {
    const long i = t0 + q * RG_THREADS + threadIdx.x;
    const uint32_t m = rg_frame_map(scores, i, T, K, p);
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
    const uint32_t before = ((state & (exc >> 16)) | (~state & exc)) & 0xffffu;
    const uint32_t after = ((before & (m >> 16)) | (~before & m)) & 0xffffu;
    uint32_t on = ~before & after & 0xffffu, off = before & ~after;
    if (i == T - 1) {   // a region still open closes on the last frame; one that would open there is empty
      off = before;
      on = 0;
    }
    if (i >= T) on = off = 0;
    if (i < T) events[i] = on | (off << 16);
    const int chunk = blockIdx.x * (RG_TILE / RG_CHUNK) + q * 4 + w;
#pragma unroll
    for (int k = 0; k < RG_MAXK; ++k)
      if (k < K) {
        const unsigned long long b = __ballot((on >> k) & 1u);
        if (lane == k && chunk < nchunks) chunk_cnt[(long)k * nchunks + chunk] = __popcll(b);
      }
    state = ((state & (total >> 16)) | (~state & total)) & 0xffffu;
  }
}

// wave k: exclusive scan of class k's chunk counts; the total is the number of regions before any clean-up
__global__ __launch_bounds__(64 * RG_MAXK) void k_regions_offsets(const int* __restrict__ chunk_cnt, int nchunks, int* __restrict__ chunk_off,
                                  int* __restrict__ n_raw) {
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
  const int* cnt = chunk_cnt + (long)k * nchunks;
  int* out = chunk_off + (long)k * nchunks;
  int carry = 0;
  for (int base = 0; base < nchunks; base += 64) {
    const int c = base + lane;
    const int v = c < nchunks ? cnt[c] : 0;
    const int inc = rg_wave_scan_int(v, lane);
    if (c < nchunks) out[c] = carry + inc - v;
    carry += __shfl(inc, 63, 64);
  }
  if (lane == 0) n_raw[k] = carry;
}

// On- and off-events of a class alternate, starting with an on-event: region n runs from the n-th on-event to the
// n-th off-event, and the off-event's n is (number of on-events up to and including its frame) - 1.
__global__ __launch_bounds__(RG_THREADS) void k_regions_emit(const uint32_t* __restrict__ events, int T, int K,
                                                             RegionParams p, const int* __restrict__ chunk_off,
                                                             int nchunks, int capacity,
                                                             double* __restrict__ raw) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * RG_THREADS + threadIdx.x;
  const int chunk = (int)(i >> 6);
  const uint32_t ev = i < T ? events[i] : 0u;
  if (__ballot(ev != 0u) == 0ull) return;
  const double t = rg_time(i, p);
  const unsigned long long upto = ~0ull >> (63 - lane);   // lanes 0..lane
#pragma unroll
  for (int k = 0; k < RG_MAXK; ++k)
    if (k < K) {
      const unsigned long long b = __ballot((ev >> k) & 1u);
      if ((ev >> k) & 0x10001u) {
        const int n = chunk_off[(long)k * nchunks + chunk] + __popcll(b & upto) - 1;
        if (n >= 0 && n < capacity) {
          double* r = raw + ((long)k * capacity + n) * 2;
          if ((ev >> k) & 1u) r[0] = t;
          if ((ev >> (16 + k)) & 1u) r[1] = t;
        }
      }
    }
}

// One workgroup per class over its (few) regions, three order-preserving compactions: raw -> out drops regions the
// reference's Annotation refuses on insertion (duration <= 1e-6); out -> raw merges neighbours whose gap has
// Segment.duration < min_duration_off (Annotation.support(collar)); raw -> out drops regions with
// duration < min_duration_on and records every survivor's index among the merged regions (its track name).
__global__ __launch_bounds__(RG_THREADS) void k_regions_finish(int K, RegionParams p, const int* __restrict__ n_raw,
                                                               int capacity, double* raw_all, double* out_all,
                                                               int* __restrict__ tracks_all,
                                                               int* __restrict__ counts) {
  __shared__ int red[4];
  const int k = blockIdx.x, tid = threadIdx.x;
  double* raw = raw_all + (long)k * capacity * 2;
  double* out = out_all + (long)k * capacity * 2;
  int* tracks = tracks_all ? tracks_all + (long)k * capacity : nullptr;
  const double min_on = p.min_on[k], min_off = p.min_off[k];
  const int n0 = min(n_raw[k], capacity);
  int total;

  int n1 = 0;
  for (int base = 0; base < n0; base += RG_THREADS) {
    const int i = base + tid;
    double s = 0.0, e = 0.0;
    if (i < n0) { s = raw[2 * i]; e = raw[2 * i + 1]; }
    const int keep = i < n0 && (e - s) > RG_PRECISION;
    const int pos = n1 + rg_block_scan_int(keep, red, total) - 1;
    if (keep) { out[2 * pos] = s; out[2 * pos + 1] = e; }
    n1 += total;
  }
  __syncthreads();

  int n2 = 0;
  for (int base = 0; base < n1; base += RG_THREADS) {
    const int i = base + tid;
    int head = 0, tail = 0;
    double s = 0.0, e = 0.0;
    if (i < n1) {
      s = out[2 * i]; e = out[2 * i + 1];
      head = i == 0 || !(min_off > 0.0 && rg_duration(out[2 * i - 1], s) < min_off);
      tail = i == n1 - 1 || !(min_off > 0.0 && rg_duration(e, out[2 * i + 2]) < min_off);
    }
    const int run = n2 + rg_block_scan_int(head, red, total) - 1;
    if (head) raw[2 * run] = s;
    if (tail) raw[2 * run + 1] = e;
    n2 += total;
  }
  __syncthreads();

  int n3 = 0;
  for (int base = 0; base < n2; base += RG_THREADS) {
    const int i = base + tid;
    double s = 0.0, e = 0.0;
    if (i < n2) { s = raw[2 * i]; e = raw[2 * i + 1]; }
    const int keep = i < n2 && !(min_on > 0.0 && rg_duration(s, e) < min_on);
    const int pos = n3 + rg_block_scan_int(keep, red, total) - 1;
    if (keep) {
      out[2 * pos] = s;
      out[2 * pos + 1] = e;
      if (tracks) tracks[pos] = min_off > 0.0 ? i : 0;   // support() renames tracks; without it all are the first name
    }
    n3 += total;
  }
  if (tid == 0) counts[k] = n3;
}

// The workspace of pa_binarize_regions in 256-byte-aligned blocks
struct RegionWorkspace {
  double* raw;                              // (K, capacity, 2)
  uint32_t *tile_map, *state_in, *events;   // (ntiles), (ntiles), (T)
  int *chunk_cnt, *chunk_off, *n_raw;       // (K, nchunks) each, (RG_MAXK)
};

static RegionWorkspace region_workspace(Carver& c, int T, int K, int capacity) {
  const size_t ntiles = cdiv(T, RG_TILE), nchunks = cdiv(T, RG_CHUNK);
  RegionWorkspace w;
  w.raw = c.take<double>(2 * (size_t)K * capacity);
  w.tile_map = c.take<uint32_t>(ntiles);
  w.state_in = c.take<uint32_t>(ntiles);
  w.events = c.take<uint32_t>(T);
  w.chunk_cnt = c.take<int>((size_t)K * nchunks);
  w.chunk_off = c.take<int>((size_t)K * nchunks);
  w.n_raw = c.take<int>(RG_MAXK);
  return w;
}

}  // namespace pa

extern "C" {

size_t pa_binarize_regions_workspace_bytes(int T, int K, int capacity) {
  if (T < 2 || K <= 0 || K > pa::RG_MAXK || capacity < 0) return 0;
  return pa::carved_bytes([&](pa::Carver& c) { pa::region_workspace(c, T, K, capacity); });
}

int pa_binarize_regions(const float* scores, int T, int K, const float* onset, const float* offset,
                        const double* min_duration_on, const double* min_duration_off, double start,
                        double duration, double step, int capacity, int32_t* counts, double* regions,
                        int32_t* tracks, void* workspace, size_t workspace_bytes, void* stream) {
  PA_REQUIRE(K > 0 && K <= pa::RG_MAXK, "pa_binarize_regions: K = %d classes, 1..%d supported", K, pa::RG_MAXK);
  PA_REQUIRE(T >= 0 && capacity >= 0, "pa_binarize_regions: negative T or capacity");
  PA_REQUIRE(onset && offset && min_duration_on && min_duration_off && counts,
             "pa_binarize_regions: null parameter array");
  hipStream_t s = (hipStream_t)stream;
  if (T < 2) {   // the reference has no defined result for fewer than two frames
    if (hipMemsetAsync(counts, 0, sizeof(int32_t) * K, s) != hipSuccess) {
      pa::set_error("pa_binarize_regions: hipMemsetAsync failed");
      return 1;
    }
    return 0;
  }
  PA_REQUIRE(scores && (regions || capacity == 0), "pa_binarize_regions: null scores / regions");
  pa::Carver carver(workspace);
  const pa::RegionWorkspace w = pa::region_workspace(carver, T, K, capacity);
  PA_REQUIRE(workspace && workspace_bytes >= carver.bytes(), "pa_binarize_regions: workspace of %zu bytes, %zu needed",
             workspace_bytes, carver.bytes());
  pa::RegionParams p;
  for (int k = 0; k < pa::RG_MAXK; ++k) {
    p.onset[k] = k < K ? onset[k] : 0.f;
    p.offset[k] = k < K ? offset[k] : 0.f;
    p.min_on[k] = k < K ? min_duration_on[k] : 0.0;
    p.min_off[k] = k < K ? min_duration_off[k] : 0.0;
  }
  p.start = start; p.duration = duration; p.step = step;
  const int ntiles = pa::cdiv(T, pa::RG_TILE), nchunks = pa::cdiv(T, pa::RG_CHUNK);
  int32_t n_raw[pa::RG_MAXK];
  {
    pa::ProfScope prof("k_binarize_regions", stream, 4.0 * T * K, 8.0 * T * K + 8.0 * T + 16.0 * nchunks * K);
    hipLaunchKernelGGL(pa::k_regions_reduce, dim3(ntiles), dim3(pa::RG_THREADS), 0, s, scores, T, K, p, w.tile_map);
    hipLaunchKernelGGL(pa::k_regions_scan, dim3(1), dim3(64), 0, s, w.tile_map, ntiles, w.state_in);
    hipLaunchKernelGGL(pa::k_regions_apply, dim3(ntiles), dim3(pa::RG_THREADS), 0, s, scores, T, K, p, w.state_in,
                       w.events, w.chunk_cnt, nchunks);
    hipLaunchKernelGGL(pa::k_regions_offsets, dim3(1), dim3(64 * K), 0, s, w.chunk_cnt, nchunks, w.chunk_off,
                       w.n_raw);
    hipLaunchKernelGGL(pa::k_regions_emit, dim3(pa::cdiv(T, pa::RG_THREADS)), dim3(pa::RG_THREADS), 0, s, w.events,
                       T, K, p, w.chunk_off, nchunks, capacity, w.raw);
    hipLaunchKernelGGL(pa::k_regions_finish, dim3(K), dim3(pa::RG_THREADS), 0, s, K, p, w.n_raw, capacity, w.raw,
                       regions, tracks, counts);
    PA_CHECK_LAUNCH("pa_binarize_regions");
  }
  // the caller reads `counts` next anyway: wait here and report a capacity that was too small
  if (hipMemcpyAsync(n_raw, w.n_raw, sizeof(int32_t) * K, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    pa::set_error("pa_binarize_regions: reading the region counts back failed: %s",
                  hipGetErrorString(hipGetLastError()));
    return 1;
  }
  for (int k = 0; k < K; ++k)
    PA_REQUIRE(n_raw[k] <= capacity, "pa_binarize_regions: class %d has %d regions, capacity is %d", k, n_raw[k],
               capacity);
  return 0;
}

}  // extern "C"
