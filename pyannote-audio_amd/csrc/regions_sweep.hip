// hipcc-flags: -ffp-contract=off
// The regions of MANY hysteresis detectors from one pass over an aggregated (T, K) score array: what tuning the
// thresholds of VoiceActivityDetection / MultiLabelSegmentation on a corpus asks for (every candidate's region lists;
// DESIGN.md section 24).  The rule is pa_binarize_regions', bit for bit: both run the steps of regions.h.
//
// A LANE is (class, onset, offset); a JOB is (lane, min_duration_on, min_duration_off).  Lanes of one class travel
// sixteen to a map word -- the role the K classes play in regions.hip -- so a GROUP of up to 16 lanes reads its
// column of the scores once, and the hysteresis of a lane runs once however many jobs read it.
//
// Per launch batch of groups (blockIdx.y = group; as many groups at a time as the workspace holds, results do not
// depend on the split; NO workgroup ever waits for another one):
//   k_sweep_reduce / k_sweep_scan / k_sweep_apply / k_sweep_offsets   the steps of regions.h -> raw count per lane
//   (counting phase stops here: pa_regions_sweep_count reads the raw counts back, the caller sizes the row buffers)
//   k_sweep_emit       region n of a lane runs from its n-th on-event to its n-th off-event
//   k_sweep_clean      one workgroup per lane: drops the empty regions into a list that is only read from then on
// then, over all jobs:
//   k_sweep_merge      one workgroup per job: merges across short gaps into the job's own scratch, counts survivors
//   k_sweep_job_offsets  one wave: exclusive scan of the jobs' counts -> the (M + 1) offset table
//   k_sweep_remove     one workgroup per job: drops short regions, writes the job's slice of the packed output
#include <algorithm>
#include <vector>

#include "common.h"
#include "pyannote_amd.h"
#include "regions.h"

namespace pa {

struct SweepGroup : RegionOneFile {
  float onset[RG_MAXK], offset[RG_MAXK];   // unused slots: +inf / -inf, the identity map, never an event
  int32_t lane[RG_MAXK];                   // lane id of every slot, -1: unused
  int32_t cls;                             // the column every slot reads

  __device__ __forceinline__ uint32_t frame_map(const float* __restrict__ scores, long i, int T, int K) const {
    if (i >= T) return RG_IDENTITY;
    const float y = scores[i * K + cls];              // NaN: both comparisons false -> identity
    uint32_t f0 = 0, f1 = 0;
#pragma unroll
    for (int s = 0; s < RG_MAXK; ++s) {
      f0 |= (uint32_t)(y > onset[s]) << s;
      f1 |= (uint32_t)(!(y < offset[s])) << s;
    }
    if (i == 0) f1 = f0;
    return f0 | (f1 << 16);
  }
};

// grid (tile, group); a group's thresholds are read from LDS
__global__ __launch_bounds__(RG_THREADS) void k_sweep_reduce(const float* __restrict__ scores, int T, int K,
                                                             const SweepGroup* __restrict__ groups, int ntiles,
                                                             uint32_t* __restrict__ tile_map) {
  __shared__ SweepGroup g;
  if (threadIdx.x == 0) g = groups[blockIdx.y];
  __syncthreads();
  rg_reduce_tile(scores, T, K, g, tile_map + (long)blockIdx.y * ntiles);
}

__global__ __launch_bounds__(64) void k_sweep_scan(const uint32_t* __restrict__ tile_map, int ntiles,
                                                   uint32_t* __restrict__ state_in) {
  rg_scan_tiles(tile_map + (long)blockIdx.x * ntiles, ntiles, state_in + (long)blockIdx.x * ntiles);
}

// `events`: NULL in the counting phase (only the chunk counts are wanted)
__global__ __launch_bounds__(RG_THREADS) void k_sweep_apply(const float* __restrict__ scores, int T, int K,
                                                            const SweepGroup* __restrict__ groups, int ntiles,
                                                            const uint32_t* __restrict__ state_in,
                                                            uint32_t* __restrict__ events,
                                                            int* __restrict__ chunk_cnt, int nchunks) {
  __shared__ SweepGroup g;
  if (threadIdx.x == 0) g = groups[blockIdx.y];
  __syncthreads();
  rg_apply_tile(scores, T, K, g, RG_MAXK, state_in[(long)blockIdx.y * ntiles + blockIdx.x],
                events ? events + (long)blockIdx.y * T : nullptr, chunk_cnt + (long)blockIdx.y * RG_MAXK * nchunks,
                nchunks);
}

// workgroup = group, wave s = its slot s; the total of the slot's chunk counts is the lane's raw count
__global__ __launch_bounds__(64 * RG_MAXK) void k_sweep_offsets(const SweepGroup* __restrict__ groups,
                                                                const int* __restrict__ chunk_cnt, int nchunks,
                                                                int* __restrict__ chunk_off,
                                                                int* __restrict__ n_raw) {
  const int s = threadIdx.x >> 6;
  const long row = ((long)blockIdx.x * RG_MAXK + s) * nchunks;
  const int total = rg_scan_counts(chunk_cnt + row, nchunks, chunk_off + row);
  const int id = groups[blockIdx.x].lane[s];
  if ((threadIdx.x & 63) == 0 && id >= 0) n_raw[id] = total;
}

// raw rows of lane l: raw + 2 raw_off[l], raw_off[l + 1] - raw_off[l] of them (the counting phase's counts)
__global__ __launch_bounds__(RG_THREADS) void k_sweep_emit(const uint32_t* __restrict__ events, int T,
                                                           const SweepGroup* __restrict__ groups, double start,
                                                           double duration, double step,
                                                           const int* __restrict__ chunk_off, int nchunks,
                                                           const int* __restrict__ raw_off,
                                                           double* __restrict__ raw) {
  const int32_t* lane_of = groups[blockIdx.y].lane;
  rg_emit_events(events + (long)blockIdx.y * T, T, RG_MAXK, RegionOneFile{}, start, duration, step,
                 chunk_off + (long)blockIdx.y * RG_MAXK * nchunks, nchunks,
                 [=](int s) {
                   const int id = lane_of[s];
                   return id < 0 ? RegionRows{0, 0} : RegionRows{raw_off[id], raw_off[id + 1] - raw_off[id]};
                 },
                 raw);
}

// one workgroup per slot of the batch's groups: raw -> clean without the empty regions.  `clean` has the layout of
// `raw` and is only read afterwards.
__global__ __launch_bounds__(RG_THREADS) void k_sweep_clean(const SweepGroup* __restrict__ groups,
                                                            const int* __restrict__ n_raw,
                                                            const int* __restrict__ raw_off,
                                                            const double* __restrict__ raw_all,
                                                            double* __restrict__ clean_all,
                                                            int* __restrict__ n_clean) {
  __shared__ int red[4];
  const int id = groups[blockIdx.x / RG_MAXK].lane[blockIdx.x % RG_MAXK];
  if (id < 0) return;                                   // (the whole workgroup)
  const int n1 = rg_drop_empty(raw_all + (long)raw_off[id] * 2, min(n_raw[id], raw_off[id + 1] - raw_off[id]),
                               clean_all + (long)raw_off[id] * 2, red);
  if (threadIdx.x == 0) n_clean[id] = n1;
}

struct SweepJob {
  double min_on, min_off;
  int32_t lane, scratch_off;    // the job's merged rows: scratch + 2 scratch_off, room for the lane's raw count
};

// one workgroup per job: clean (read only) -> the job's scratch, merged across short gaps; then the survivors of the
// min_duration_on removal are counted
__global__ __launch_bounds__(RG_THREADS) void k_sweep_merge(const SweepJob* __restrict__ jobs,
                                                            const int* __restrict__ n_clean,
                                                            const int* __restrict__ raw_off,
                                                            const double* __restrict__ clean_all,
                                                            double* __restrict__ scratch_all,
                                                            int* __restrict__ n_merged, int* __restrict__ counts) {
  __shared__ int red[4];
  const SweepJob job = jobs[blockIdx.x];
  const int tid = threadIdx.x;
  double* out = scratch_all + (long)job.scratch_off * 2;
  const double min_on = job.min_on;
  const int n1 = min(n_clean[job.lane], raw_off[job.lane + 1] - raw_off[job.lane]);
  const int n2 = rg_merge_gaps(clean_all + (long)raw_off[job.lane] * 2, n1, job.min_off, out, red);
  __syncthreads();                                      // the merged rows are read by other threads below
  int total, n3 = 0;
  for (int base = 0; base < n2; base += RG_THREADS) {
    const int i = base + tid;
    const int keep = i < n2 && !(min_on > 0.0 && rg_duration(out[2 * i], out[2 * i + 1]) < min_on);
    rg_block_scan_int(keep, red, total);
    n3 += total;
  }
  if (tid == 0) { n_merged[blockIdx.x] = n2; counts[blockIdx.x] = n3; }
}

// one wave: the jobs' counts -> the (M + 1) offset table
__global__ __launch_bounds__(64) void k_sweep_job_offsets(const int* __restrict__ counts, int M,
                                                          int* __restrict__ job_off) {
  const int total = rg_scan_counts(counts, M, job_off);
  if (threadIdx.x == 0) job_off[M] = total;
}

// one workgroup per job: scratch -> the job's rows of the packed output (`rows` in all) without the short regions
__global__ __launch_bounds__(RG_THREADS) void k_sweep_remove(const SweepJob* __restrict__ jobs,
                                                             const double* __restrict__ scratch_all,
                                                             const int* __restrict__ n_merged,
                                                             const int* __restrict__ job_off, int rows,
                                                             double* __restrict__ regions,
                                                             int* __restrict__ tracks) {
  __shared__ int red[4];
  const SweepJob job = jobs[blockIdx.x];
  const int o = job_off[blockIdx.x];
  rg_drop_short(scratch_all + (long)job.scratch_off * 2, n_merged[blockIdx.x], job.min_on, job.min_off, rows - o,
                regions + (long)o * 2, tracks ? tracks + o : nullptr, red);
}

// ------------------------------------------------------------------------------------------------ host side
// The workspace of pa_regions_sweep_count / _emit in 256-byte-aligned blocks behind 256 bytes of slack (the caller's
// pointer need not be aligned).  First what does not depend on the launch batch (the counting phase passes M =
// raw_rows = job_rows = 0), then the arrays of a batch of `per` groups, a group's share of each rounded up to 256
// bytes: fixed + per * each bytes in all.
struct SweepWorkspace {
  SweepGroup* groups;
  int *n_raw, *raw_off, *n_clean;   // (L + 1) each
  double *raw, *clean;              // (raw_rows, 2) each
  SweepJob* jobs;
  int *n_merged, *counts;           // (M + 1) each
  double* scratch;                  // (job_rows, 2)
  uint32_t *tile_map, *state_in, *events;   // the batch
  int *chunk_cnt, *chunk_off;
};
static SweepWorkspace sweep_layout(Carver& c, int T, int groups, int per, int L, int M, long raw_rows, long job_rows) {
  const size_t ntiles = cdiv(T, RG_TILE), nchunks = cdiv(T, RG_CHUNK);
  SweepWorkspace w;
  w.groups = c.take<SweepGroup>(groups);
  w.n_raw = c.take<int>((size_t)L + 1);
  w.raw_off = c.take<int>((size_t)L + 1);
  w.n_clean = c.take<int>((size_t)L + 1);
  w.raw = c.take<double>(2 * (size_t)raw_rows);
  w.clean = c.take<double>(2 * (size_t)raw_rows);
  w.jobs = c.take<SweepJob>(M);
  w.n_merged = c.take<int>((size_t)M + 1);
  w.counts = c.take<int>((size_t)M + 1);
  w.scratch = c.take<double>(2 * (size_t)job_rows);
  w.tile_map = c.take<uint32_t>(per * align_up(4 * ntiles) / 4);
  w.state_in = c.take<uint32_t>(per * align_up(4 * ntiles) / 4);
  w.events = c.take<uint32_t>(per * align_up(4 * (size_t)T) / 4);
  w.chunk_cnt = c.take<int>(per * align_up(4 * RG_MAXK * nchunks) / 4);
  w.chunk_off = c.take<int>(per * align_up(4 * RG_MAXK * nchunks) / 4);
  return w;
}
static size_t sweep_bytes(int T, int groups, int per, int L, int M, long raw_rows, long job_rows) {
  return carved_bytes([&](Carver& c) { sweep_layout(c, T, groups, per, L, M, raw_rows, job_rows); }, 256);
}

// lanes of one class, in lane order, sixteen to a group; classes in ascending order.  false: a class out of range
static bool sweep_plan(int K, int L, const int32_t* lane_class, const float* onset, const float* offset,
                       std::vector<SweepGroup>* groups) {
  std::vector<std::vector<int>> by_class(K > 0 ? K : 0);
  for (int l = 0; l < L; ++l) {
    if (lane_class[l] < 0 || lane_class[l] >= K) return false;
    by_class[lane_class[l]].push_back(l);
  }
  for (int k = 0; k < K; ++k)
    for (size_t at = 0; at < by_class[k].size(); at += RG_MAXK) {
      SweepGroup g;
      g.cls = k;
      for (int s = 0; s < RG_MAXK; ++s) {
        const bool used = at + s < by_class[k].size();
        const int l = used ? by_class[k][at + s] : -1;
        g.lane[s] = l;
        g.onset[s] = used ? onset[l] : __builtin_inff();
        g.offset[s] = used ? offset[l] : -__builtin_inff();
      }
      groups->push_back(g);
    }
  return true;
}

static int sweep_check_lanes(const char* who, int T, int K, int L, const int32_t* lane_class, const float* onset,
                             const float* offset) {
  PA_REQUIRE(K > 0 && K <= RG_MAXK, "%s: K = %d classes, 1..%d supported", who, K, RG_MAXK);
  PA_REQUIRE(T >= 0 && L >= 0, "%s: negative T or lane count", who);
  PA_REQUIRE(L == 0 || (lane_class && onset && offset), "%s: null lane array", who);
  for (int l = 0; l < L; ++l) {
    PA_REQUIRE(lane_class[l] >= 0 && lane_class[l] < K, "%s: lane %d names class %d, 0..%d exist", who, l,
               lane_class[l], K - 1);
    PA_REQUIRE(onset[l] == onset[l] && offset[l] == offset[l], "%s: a threshold of lane %d is NaN", who, l);
  }
  return 0;
}

// What either phase does between its argument checks and its first launch: the plan of the lanes, how many groups a
// launch sequence takes (as many as the workspace holds), the carve and the upload of the plan.  Nothing is launched,
// and nothing written, before the last refusal here.
struct SweepSetup {
  std::vector<SweepGroup> groups;   // handed to an asynchronous copy: the phase waits for the stream before it returns
  int G, per;                       // groups in all and per launch sequence
  SweepWorkspace w;
};
static int sweep_setup(const char* who, int T, int K, int L, const int32_t* lane_class, const float* onset,
                       const float* offset, int M, long raw_rows, long job_rows, void* workspace,
                       size_t workspace_bytes, hipStream_t s, SweepSetup* u) {
  sweep_plan(K, L, lane_class, onset, offset, &u->groups);
  const int G = u->G = (int)u->groups.size();
  const size_t fixed = sweep_bytes(T, G, 0, L, M, raw_rows, job_rows),
               each = sweep_bytes(T, G, 1, L, M, raw_rows, job_rows) - fixed;
  PA_REQUIRE(workspace && workspace_bytes >= fixed + each, "%s: workspace of %zu bytes, at least %zu needed", who,
             workspace_bytes, fixed + each);
  u->per = (int)std::min<size_t>(std::min(G, 65535), (workspace_bytes - fixed) / each);   // (grid.y)
  Carver carver(workspace, 256);
  u->w = sweep_layout(carver, T, G, u->per, L, M, raw_rows, job_rows);
  PA_REQUIRE(workspace_bytes >= carver.bytes(), "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
             carver.bytes());
  if (hipMemcpyAsync(u->w.groups, u->groups.data(), sizeof(SweepGroup) * (size_t)G, hipMemcpyHostToDevice, s) !=
      hipSuccess) {
    set_error("%s: uploading the lane tables failed", who);
    return 1;
  }
  return 0;
}

// the launches of one batch of `n` groups starting at group `g0`; `emit` false: counting only
static void sweep_launch_batch(hipStream_t s, const float* scores, int T, int K, const SweepWorkspace& w, int g0,
                               int n, bool emit, double start, double duration, double step) {
  const int ntiles = cdiv(T, RG_TILE), nchunks = cdiv(T, RG_CHUNK);
  const SweepGroup* g = w.groups + g0;
  hipLaunchKernelGGL(k_sweep_reduce, dim3(ntiles, n), dim3(RG_THREADS), 0, s, scores, T, K, g, ntiles, w.tile_map);
  hipLaunchKernelGGL(k_sweep_scan, dim3(n), dim3(64), 0, s, w.tile_map, ntiles, w.state_in);
  hipLaunchKernelGGL(k_sweep_apply, dim3(ntiles, n), dim3(RG_THREADS), 0, s, scores, T, K, g, ntiles, w.state_in,
                     emit ? w.events : nullptr, w.chunk_cnt, nchunks);
  hipLaunchKernelGGL(k_sweep_offsets, dim3(n), dim3(64 * RG_MAXK), 0, s, g, w.chunk_cnt, nchunks, w.chunk_off,
                     w.n_raw);
  if (!emit) return;
  hipLaunchKernelGGL(k_sweep_emit, dim3(cdiv(T, RG_THREADS), n), dim3(RG_THREADS), 0, s, w.events, T, g, start,
                     duration, step, w.chunk_off, nchunks, w.raw_off, w.raw);
  hipLaunchKernelGGL(k_sweep_clean, dim3(n * RG_MAXK), dim3(RG_THREADS), 0, s, g, w.n_raw, w.raw_off, w.raw, w.clean,
                     w.n_clean);
}

}  // namespace pa

extern "C" {

int pa_regions_sweep_groups(int K, int L, const int32_t* lane_class) {
  if (K <= 0 || K > pa::RG_MAXK || L < 0 || (L > 0 && !lane_class)) return -1;
  int per_class[pa::RG_MAXK] = {0};
  for (int l = 0; l < L; ++l) {
    if (lane_class[l] < 0 || lane_class[l] >= K) return -1;
    ++per_class[lane_class[l]];
  }
  int groups = 0;
  for (int k = 0; k < K; ++k) groups += pa::cdiv(per_class[k], pa::RG_MAXK);
  return groups;
}

size_t pa_regions_sweep_workspace_bytes(int T, int groups, int groups_per_launch, int L, int M, long raw_rows,
                                        long job_rows) {
  if (T < 2 || groups < 0 || groups_per_launch < 0 || L < 0 || M < 0 || raw_rows < 0 || job_rows < 0) return 0;
  return pa::sweep_bytes(T, groups, groups_per_launch, L, M, raw_rows, job_rows);
}

int pa_regions_sweep_count(const float* scores, int T, int K, int L, const int32_t* lane_class, const float* onset,
                           const float* offset, int32_t* n_raw, int32_t* launches, void* workspace,
                           size_t workspace_bytes, void* stream) {
  const char* who = "pa_regions_sweep_count";
  if (launches) *launches = 0;
  if (int rc = pa::sweep_check_lanes(who, T, K, L, lane_class, onset, offset)) return rc;
  PA_REQUIRE(L == 0 || n_raw, "%s: null count array", who);
  for (int l = 0; l < L; ++l) n_raw[l] = 0;
  if (T < 2 || L == 0) return 0;      // the reference has no defined result for fewer than two frames
  PA_REQUIRE(scores, "%s: null scores", who);
  hipStream_t s = (hipStream_t)stream;
  pa::SweepSetup u;
  if (int rc = pa::sweep_setup(who, T, K, L, lane_class, onset, offset, 0, 0, 0, workspace, workspace_bytes, s, &u))
    return rc;
  const int G = u.G, per = u.per;
  const pa::SweepWorkspace& w = u.w;
  {
    pa::ProfScope prof("k_regions_sweep_count", stream, 4.0 * T * G * 16, 12.0 * T * G);
    for (int g0 = 0; g0 < G; g0 += per) {
      pa::sweep_launch_batch(s, scores, T, K, w, g0, std::min(per, G - g0), false, 0.0, 0.0, 0.0);
      PA_CHECK_LAUNCH(who);
      if (launches) ++*launches;
    }
  }
  // the one read-back the row buffers are sized from (it also keeps `groups` alive until the upload has happened)
  if (hipMemcpyAsync(n_raw, w.n_raw, sizeof(int32_t) * (size_t)L, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    pa::set_error("%s: reading the region counts back failed: %s", who, hipGetErrorString(hipGetLastError()));
    return 1;
  }
  return 0;
}

int pa_regions_sweep_emit(const float* scores, int T, int K, int L, const int32_t* lane_class, const float* onset,
                          const float* offset, const int32_t* n_raw, int M, const int32_t* job_lane,
                          const double* min_duration_on, const double* min_duration_off, double start, double duration,
                          double step, long rows, double* regions, int32_t* tracks, int32_t* job_off,
                          int32_t* launches, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "pa_regions_sweep_emit";
  if (launches) *launches = 0;
  if (int rc = pa::sweep_check_lanes(who, T, K, L, lane_class, onset, offset)) return rc;
  PA_REQUIRE(M >= 0 && rows >= 0, "%s: negative job or row count", who);
  PA_REQUIRE(M == 0 || (job_lane && min_duration_on && min_duration_off), "%s: null job array", who);
  PA_REQUIRE(job_off, "%s: null offset table", who);
  PA_REQUIRE(start == start && duration == duration && step == step, "%s: the frame grid has a NaN", who);
  for (int j = 0; j < M; ++j) {
    PA_REQUIRE(job_lane[j] >= 0 && job_lane[j] < L, "%s: job %d names lane %d, 0..%d exist", who, j, job_lane[j],
               L - 1);
    PA_REQUIRE(min_duration_on[j] == min_duration_on[j] && min_duration_off[j] == min_duration_off[j],
               "%s: a duration of job %d is NaN", who, j);
  }
  hipStream_t s = (hipStream_t)stream;
  if (T < 2 || L == 0 || M == 0) {
    if (pa::fill_async(job_off, 0, sizeof(int32_t) * ((size_t)M + 1), s) != hipSuccess) {
      pa::set_error("%s: the fill launch failed", who);
      return 1;
    }
    return 0;
  }
  PA_REQUIRE(scores && n_raw, "%s: null scores / raw counts", who);
  std::vector<int32_t> raw_off((size_t)L + 1, 0);
  long raw_rows = 0, job_rows = 0;
  for (int l = 0; l < L; ++l) {
    PA_REQUIRE(n_raw[l] >= 0 && n_raw[l] <= T / 2, "%s: lane %d is given %d raw regions, 0..%d possible", who, l,
               n_raw[l], T / 2);
    raw_rows += n_raw[l];
    PA_REQUIRE(raw_rows <= 0x7fffffffL, "%s: more than 2^31 - 1 raw regions: sweep fewer lanes per call", who);
    raw_off[l + 1] = (int32_t)raw_rows;
  }
  std::vector<pa::SweepJob> jobs((size_t)M);
  for (int j = 0; j < M; ++j) {
    jobs[j] = pa::SweepJob{min_duration_on[j], min_duration_off[j], job_lane[j], (int32_t)job_rows};
    job_rows += n_raw[job_lane[j]];
    PA_REQUIRE(job_rows <= 0x7fffffffL, "%s: more than 2^31 - 1 job rows: sweep fewer jobs per call", who);
  }
  PA_REQUIRE(rows >= job_rows && (regions || job_rows == 0), "%s: room for %ld rows, %ld needed", who, rows, job_rows);
  pa::SweepSetup u;
  if (int rc = pa::sweep_setup(who, T, K, L, lane_class, onset, offset, M, raw_rows, job_rows, workspace,
                               workspace_bytes, s, &u))
    return rc;
  const int G = u.G, per = u.per;
  const pa::SweepWorkspace& w = u.w;
  if (hipMemcpyAsync(w.raw_off, raw_off.data(), 4 * ((size_t)L + 1), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(w.jobs, jobs.data(), sizeof(pa::SweepJob) * (size_t)M, hipMemcpyHostToDevice, s) != hipSuccess) {
    pa::set_error("%s: uploading the lane and job tables failed", who);
    return 1;
  }
  {
    pa::ProfScope prof("k_regions_sweep_emit", stream, 4.0 * T * G * 16, 16.0 * T * G + 48.0 * job_rows);
    for (int g0 = 0; g0 < G; g0 += per) {
      pa::sweep_launch_batch(s, scores, T, K, w, g0, std::min(per, G - g0), true, start, duration, step);
      PA_CHECK_LAUNCH(who);
      if (launches) ++*launches;
    }
    hipLaunchKernelGGL(pa::k_sweep_merge, dim3(M), dim3(pa::RG_THREADS), 0, s, w.jobs, w.n_clean, w.raw_off, w.clean,
                       w.scratch, w.n_merged, w.counts);
    hipLaunchKernelGGL(pa::k_sweep_job_offsets, dim3(1), dim3(64), 0, s, w.counts, M, job_off);
    hipLaunchKernelGGL(pa::k_sweep_remove, dim3(M), dim3(pa::RG_THREADS), 0, s, w.jobs, w.scratch, w.n_merged, job_off,
                       (int)std::min<long>(rows, 0x7fffffffL), regions, tracks);
    PA_CHECK_LAUNCH(who);
  }
  // the host tables above were handed to asynchronous copies: they must outlive them
  if (hipStreamSynchronize(s) != hipSuccess) {
    pa::set_error("%s: the stream failed: %s", who, hipGetErrorString(hipGetLastError()));
    return 1;
  }
  return 0;
}

}  // extern "C"
