// hipcc-flags: -ffp-contract=off
// Hysteresis thresholding of an aggregated (T, K) score array into per-class region lists, on the device
// (what utils/signal.py:254-318 `Binarize.__call__` does to every class of a multi-label model, followed by
// `Annotation.support(collar)` and the min_duration_on deletion).  One detector per class: slot k of the map word is
// class k.  The rule and every step of it are in regions.h; the kernels here say where a step's data lies.
//
// Launch sequence (each kernel ends before the next starts):
//   k_regions_reduce, k_regions_scan, k_regions_apply, k_regions_offsets, k_regions_emit   the steps of regions.h
//   k_regions_finish   one workgroup per class: drop empty regions, merge across short gaps, drop short regions
#include "common.h"
#include "pyannote_amd.h"
#include "regions.h"

namespace pa {

__global__ __launch_bounds__(RG_THREADS) void k_regions_reduce(const float* __restrict__ scores, int T, int K,
                                                               RegionParams p, uint32_t* __restrict__ tile_map) {
  rg_reduce_tile(scores, T, K, p, tile_map);
}

__global__ __launch_bounds__(64) void k_regions_scan(const uint32_t* __restrict__ tile_map, int ntiles,
                                                     uint32_t* __restrict__ state_in) {
  rg_scan_tiles(tile_map, ntiles, state_in);
}

__global__ __launch_bounds__(RG_THREADS) void k_regions_apply(const float* __restrict__ scores, int T, int K,
                                                              RegionParams p,
                                                              const uint32_t* __restrict__ state_in,
                                                              uint32_t* __restrict__ events,
                                                              int* __restrict__ chunk_cnt, int nchunks) {
  rg_apply_tile(scores, T, K, p, K, state_in[blockIdx.x], events, chunk_cnt, nchunks);
}

// wave k: class k's chunk counts; the total is the number of regions before any clean-up
__global__ __launch_bounds__(64 * RG_MAXK) void k_regions_offsets(const int* __restrict__ chunk_cnt, int nchunks,
                                                                  int* __restrict__ chunk_off,
                                                                  int* __restrict__ n_raw) {
  const int k = threadIdx.x >> 6;
  const int total = rg_scan_counts(chunk_cnt + (long)k * nchunks, nchunks, chunk_off + (long)k * nchunks);
  if ((threadIdx.x & 63) == 0) n_raw[k] = total;
}

__global__ __launch_bounds__(RG_THREADS) void k_regions_emit(const uint32_t* __restrict__ events, int T, int K,
                                                             RegionParams p, const int* __restrict__ chunk_off,
                                                             int nchunks, int capacity,
                                                             double* __restrict__ raw) {
  rg_emit_events(events, T, K, p, p.start, p.duration, p.step, chunk_off, nchunks,
                 [=](int k) { return RegionRows{(long)k * capacity, capacity}; }, raw);
}

// One workgroup per class over its (few) regions: the three compactions of regions.h, raw -> out -> raw -> out
__global__ __launch_bounds__(RG_THREADS) void k_regions_finish(int K, RegionParams p, const int* __restrict__ n_raw,
                                                               int capacity, double* raw_all, double* out_all,
                                                               int* __restrict__ tracks_all,
                                                               int* __restrict__ counts) {
  __shared__ int red[4];
  const int k = blockIdx.x;
  double* raw = raw_all + (long)k * capacity * 2;
  double* out = out_all + (long)k * capacity * 2;
  int* tracks = tracks_all ? tracks_all + (long)k * capacity : nullptr;
  const int n1 = rg_drop_empty(raw, min(n_raw[k], capacity), out, red);
  __syncthreads();
  const int n2 = rg_merge_gaps(out, n1, p.min_off[k], raw, red);
  __syncthreads();
  const int n3 = rg_drop_short(raw, n2, p.min_on[k], p.min_off[k], capacity, out, tracks, red);
  if (threadIdx.x == 0) counts[k] = n3;
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
    if (pa::fill_async(counts, 0, sizeof(int32_t) * K, s) != hipSuccess) {
      pa::set_error("pa_binarize_regions: the fill launch failed");
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
