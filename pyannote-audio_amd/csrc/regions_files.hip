// hipcc-flags: -ffp-contract=off
// The region lists of every (file, class) of a RAGGED LIST OF FILES from one pass over the concatenation of their
// aggregated scores (pa_aggregate_files leaves them so): what VoiceActivityDetection / MultiLabelSegmentation ask for
// when a list of short files shares its launches.  The rule is pa_binarize_regions', bit for
// bit, file by file: both run the steps of regions.h.
//
// File f owns rows row0[f] .. row0[f + 1] - 1 of the (rows, K) scores, the first T[f] of them are its frames, the
// rest is padding; row0[f] is a multiple of RG_CHUNK.  Why one scan over everything is the per-file rule:
//   * frame 0 of a file is a constant map, so the scan forgets the file before it there without help, and
//     rg_apply_tile is told that nothing comes before a first frame;
//   * the last frame of a file closes what is open, padding rows are identity maps without events: every file closes
//     what it opens, so per slot the n-th on-event still pairs with the n-th off-event over the whole concatenation;
//   * a 64-frame count never straddles two files: the list of (file f, slot k) is events chunk_off[k][row0[f] / 64]
//     .. chunk_off[k][row0[f + 1] / 64] - 1 of slot k;
//   * times are counted from the file's own frame 0 (RegionFiles::time_frame).
//
// Launch sequence (each kernel ends before the next starts; NO workgroup ever waits for another one):
//   k_files_index      per 64-row chunk: where its first row lies in its file, and the file's frame count
//   k_files_reduce / k_files_scan / k_files_apply / k_files_offsets   the steps of regions.h -> raw count per slot
//   (counting phase stops here: pa_binarize_regions_files_count reads the K raw counts back)
//   k_files_emit       region n of a slot runs from its n-th on-event to its n-th off-event
//   k_files_merge      one workgroup per (file, class): drop empty regions, merge across short gaps, count survivors
//   k_files_list_off   one wave: exclusive scan of the lists' counts -> the (num_files K + 1) offset table
//   k_files_remove     one workgroup per (file, class): drop short regions into the list's slice of the packed output
#include <algorithm>

#include "common.h"
#include "pyannote_amd.h"
#include "regions.h"

namespace pa {

constexpr int RF_MAX_FILES = 65535;

// the MAP type of a concatenation of files: the thresholds of RegionParams, and per 64-row chunk `where` = (index in
// its file of the chunk's first row, frames of that file); a chunk that belongs to no file has (0, 0)
struct RegionFiles {
  RegionParams p;
  const int2* where;

  // (i < rows; the number of rows is a multiple of 64, so a wave that holds a row holds none past the end)
  __device__ __forceinline__ long time_frame(long i) const { return where[i >> 6].x + (i & 63); }
  __device__ __forceinline__ bool first_frame(long i, int rows) const {
    return i < rows && where[i >> 6].y > 0 && time_frame(i) == 0;
  }
  __device__ __forceinline__ bool last_frame(long i, int rows) const {
    return i < rows && time_frame(i) == where[i >> 6].y - 1;
  }
  __device__ __forceinline__ bool no_frame(long i, int rows) const {
    return i >= rows || time_frame(i) >= where[i >> 6].y;
  }
  // padding rows and rows past the end: identity
  __device__ __forceinline__ uint32_t frame_map(const float* __restrict__ scores, long i, int rows, int K) const {
    if (no_frame(i, rows)) return RG_IDENTITY;
    return p.row_map(scores + i * K, K, time_frame(i) == 0);
  }
};

// one thread per 64-row chunk: the file f with row0[f] <= 64 c < row0[f + 1] (row0 is non-decreasing, num_files + 1
// entries), none: (0, 0)
__global__ __launch_bounds__(256) void k_files_index(const int* __restrict__ row0, const int* __restrict__ T,
                                                     int num_files, int nchunks, int2* __restrict__ where) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nchunks) return;
  const int r = c * RG_CHUNK;
  int lo = 0, hi = num_files;   // first f with row0[f + 1] > r
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (row0[mid + 1] > r) hi = mid;
    else lo = mid + 1;
  }
  where[c] = (lo < num_files && row0[lo] <= r) ? make_int2(r - row0[lo], T[lo]) : make_int2(0, 0);
}

__global__ __launch_bounds__(RG_THREADS) void k_files_reduce(const float* __restrict__ scores, int rows, int K,
                                                             RegionFiles f, uint32_t* __restrict__ tile_map) {
  rg_reduce_tile(scores, rows, K, f, tile_map);
}

__global__ __launch_bounds__(64) void k_files_scan(const uint32_t* __restrict__ tile_map, int ntiles,
                                                   uint32_t* __restrict__ state_in) {
  rg_scan_tiles(tile_map, ntiles, state_in);
}

// `events`: NULL in the counting phase (only the chunk counts are wanted)
__global__ __launch_bounds__(RG_THREADS) void k_files_apply(const float* __restrict__ scores, int rows, int K,
                                                            RegionFiles f, const uint32_t* __restrict__ state_in,
                                                            uint32_t* __restrict__ events,
                                                            int* __restrict__ chunk_cnt, int nchunks) {
  rg_apply_tile(scores, rows, K, f, K, state_in[blockIdx.x], events, chunk_cnt, nchunks);
}

// wave k: class k's chunk counts -> chunk_off (K, nchunks + 1), the last entry of a class its raw count
__global__ __launch_bounds__(64 * RG_MAXK) void k_files_offsets(const int* __restrict__ chunk_cnt, int nchunks,
                                                                int* __restrict__ chunk_off,
                                                                int* __restrict__ n_raw) {
  const int k = threadIdx.x >> 6;
  int* off = chunk_off + (long)k * (nchunks + 1);
  const int total = rg_scan_counts(chunk_cnt + (long)k * nchunks, nchunks, off);
  if ((threadIdx.x & 63) == 0) off[nchunks] = n_raw[k] = total;
}

// the raw rows of class k: raw + 2 first[k], room[k] of them (the counting phase's counts)
struct FilesRows {
  int first[RG_MAXK], room[RG_MAXK];
};

__global__ __launch_bounds__(RG_THREADS) void k_files_emit(const uint32_t* __restrict__ events, int rows, int K,
                                                           RegionFiles f, const int* __restrict__ chunk_off,
                                                           int nchunks, FilesRows r, double* __restrict__ raw) {
  rg_emit_events(events, rows, K, f, f.p.start, f.p.duration, f.p.step, chunk_off, nchunks + 1,
                 [&](int k) { return RegionRows{r.first[k], r.room[k]}; }, raw);
}

// the raw rows of list (file, class k): (first row, number), never past the class's room
__device__ __forceinline__ RegionRows files_list(const int* __restrict__ row0, const int* __restrict__ chunk_off,
                                                 int nchunks, const FilesRows& r, int file, int k) {
  const int* off = chunk_off + (long)k * (nchunks + 1);
  const int a = min(off[row0[file] / RG_CHUNK], r.room[k]), b = min(off[row0[file + 1] / RG_CHUNK], r.room[k]);
  return RegionRows{(long)r.first[k] + a, max(b - a, 0)};
}

// one workgroup per list (blockIdx.x = file * K + class): raw -> tmp without the empty regions, tmp -> raw merged
// across short gaps (a list only shrinks: it stays inside its own rows); then the survivors of the min_duration_on
// removal are counted
__global__ __launch_bounds__(RG_THREADS) void k_files_merge(int K, RegionFiles f, const int* __restrict__ row0,
                                                            const int* __restrict__ chunk_off, int nchunks,
                                                            FilesRows r, double* raw_all, double* tmp_all,
                                                            int* __restrict__ n_merged, int* __restrict__ counts) {
  __shared__ int red[4];
  const int file = blockIdx.x / K, k = blockIdx.x % K;
  const RegionRows list = files_list(row0, chunk_off, nchunks, r, file, k);
  double* raw = raw_all + list.first * 2;
  double* tmp = tmp_all + list.first * 2;
  const double min_on = f.p.min_on[k];
  const int n1 = rg_drop_empty(raw, list.room, tmp, red);
  __syncthreads();
  const int n2 = rg_merge_gaps(tmp, n1, f.p.min_off[k], raw, red);
  __syncthreads();                                      // the merged rows are read by other threads below
  int total, n3 = 0;
  for (int base = 0; base < n2; base += RG_THREADS) {
    const int i = base + threadIdx.x;
    const int keep = i < n2 && !(min_on > 0.0 && rg_duration(raw[2 * i], raw[2 * i + 1]) < min_on);
    rg_block_scan_int(keep, red, total);
    n3 += total;
  }
  if (threadIdx.x == 0) { n_merged[blockIdx.x] = n2; counts[blockIdx.x] = n3; }
}

// one wave: the lists' counts -> the (lists + 1) offset table
__global__ __launch_bounds__(64) void k_files_list_off(const int* __restrict__ counts, int lists,
                                                       int* __restrict__ list_off) {
  const int total = rg_scan_counts(counts, lists, list_off);
  if (threadIdx.x == 0) list_off[lists] = total;
}

// one workgroup per list: its merged rows -> its rows of the packed output (`out_rows` in all) without the short ones
__global__ __launch_bounds__(RG_THREADS) void k_files_remove(int K, RegionFiles f, const int* __restrict__ row0,
                                                             const int* __restrict__ chunk_off, int nchunks,
                                                             FilesRows r, const double* __restrict__ raw_all,
                                                             const int* __restrict__ n_merged,
                                                             const int* __restrict__ list_off, int out_rows,
                                                             double* __restrict__ regions,
                                                             int* __restrict__ tracks) {
  __shared__ int red[4];
  const int file = blockIdx.x / K, k = blockIdx.x % K;
  const RegionRows list = files_list(row0, chunk_off, nchunks, r, file, k);
  const int o = list_off[blockIdx.x];
  rg_drop_short(raw_all + list.first * 2, min(n_merged[blockIdx.x], list.room), f.p.min_on[k], f.p.min_off[k],
                max(out_rows - o, 0), regions + (long)o * 2, tracks ? tracks + o : nullptr, red);
}

// ------------------------------------------------------------------------------------------------ host side
// The workspace of pa_binarize_regions_files_count / _emit in 256-byte-aligned blocks (the counting phase passes
// raw_rows = 0)
struct FilesWorkspace {
  int *row0, *T;                            // (num_files + 1), (num_files)
  int2* where;                              // (nchunks)
  uint32_t *tile_map, *state_in, *events;   // (ntiles), (ntiles), (rows)
  int *chunk_cnt, *chunk_off, *n_raw;       // (K, nchunks), (K, nchunks + 1), (RG_MAXK)
  double *raw, *tmp;                        // (raw_rows, 2) each
  int *n_merged, *counts;                   // (num_files K) each
};

static FilesWorkspace files_layout(Carver& c, long rows, int K, int num_files, long raw_rows) {
  const size_t ntiles = cdiv(rows, RG_TILE), nchunks = cdiv(rows, RG_CHUNK);
  FilesWorkspace w;
  w.row0 = c.take<int>((size_t)num_files + 1);
  w.T = c.take<int>(num_files);
  w.where = c.take<int2>(nchunks);
  w.tile_map = c.take<uint32_t>(ntiles);
  w.state_in = c.take<uint32_t>(ntiles);
  w.events = c.take<uint32_t>(rows);
  w.chunk_cnt = c.take<int>((size_t)K * nchunks);
  w.chunk_off = c.take<int>((size_t)K * (nchunks + 1));
  w.n_raw = c.take<int>(RG_MAXK);
  w.raw = c.take<double>(2 * (size_t)raw_rows);
  w.tmp = c.take<double>(2 * (size_t)raw_rows);
  w.n_merged = c.take<int>((size_t)num_files * K);
  w.counts = c.take<int>((size_t)num_files * K);
  return w;
}

// What either phase does between its argument checks and its first launch: nothing is launched, and nothing written,
// before the last refusal here.
struct FilesSetup {
  RegionFiles f;
  FilesWorkspace w;
  int rows, ntiles, nchunks;
};

static int files_setup(const char* who, const float* scores, int K, int num_files, const int32_t* row0,
                       const int32_t* T, const float* onset, const float* offset, const double* min_duration_on,
                       const double* min_duration_off, double start, double duration, double step, long raw_rows,
                       void* workspace, size_t workspace_bytes, FilesSetup* u) {
  PA_REQUIRE(K > 0 && K <= RG_MAXK, "%s: K = %d classes, 1..%d supported", who, K, RG_MAXK);
  PA_REQUIRE(num_files >= 0 && num_files <= RF_MAX_FILES, "%s: %d files, 0..%d supported", who, num_files,
             RF_MAX_FILES);
  PA_REQUIRE(row0 && (T || num_files == 0) && onset && offset && min_duration_on && min_duration_off,
             "%s: null parameter array", who);
  for (int k = 0; k < K; ++k)
    PA_REQUIRE(onset[k] == onset[k] && offset[k] == offset[k] && min_duration_on[k] == min_duration_on[k] &&
                   min_duration_off[k] == min_duration_off[k],
               "%s: a threshold or a duration of class %d is NaN", who, k);
  PA_REQUIRE(start == start && duration == duration && step == step, "%s: the frame grid has a NaN", who);
  PA_REQUIRE(row0[0] == 0, "%s: row0[0] = %d, the first file starts at row 0", who, row0[0]);
  for (int f = 0; f < num_files; ++f) {
    PA_REQUIRE(row0[f + 1] >= row0[f], "%s: row0 decreases at file %d", who, f);
    PA_REQUIRE(row0[f + 1] % RG_CHUNK == 0, "%s: row0[%d] = %d is not a multiple of %d", who, f + 1, row0[f + 1],
               RG_CHUNK);
    PA_REQUIRE(T[f] >= 0 && T[f] <= row0[f + 1] - row0[f], "%s: file %d keeps %d frames and owns %d rows", who, f,
               T[f], row0[f + 1] - row0[f]);
  }
  PA_REQUIRE(raw_rows >= 0, "%s: negative row count", who);
  u->rows = row0[num_files];
  u->ntiles = cdiv(u->rows, RG_TILE);
  u->nchunks = cdiv(u->rows, RG_CHUNK);
  PA_REQUIRE(scores || u->rows == 0, "%s: null scores", who);
  Carver carver(workspace);
  u->w = files_layout(carver, u->rows, K, num_files, raw_rows);
  PA_REQUIRE(workspace && workspace_bytes >= carver.bytes(), "%s: workspace of %zu bytes, %zu needed", who,
             workspace_bytes, carver.bytes());
  RegionParams& p = u->f.p;
  for (int k = 0; k < RG_MAXK; ++k) {
    p.onset[k] = k < K ? onset[k] : 0.f;
    p.offset[k] = k < K ? offset[k] : 0.f;
    p.min_on[k] = k < K ? min_duration_on[k] : 0.0;
    p.min_off[k] = k < K ? min_duration_off[k] : 0.0;
  }
  p.start = start; p.duration = duration; p.step = step;
  u->f.where = u->w.where;
  return 0;
}

// the tables and the frame-domain steps; `emit` false: counting only.  The host tables are handed to asynchronous
// copies: either phase waits for the stream before it returns.
static int files_launch(const char* who, hipStream_t s, const float* scores, int K, int num_files,
                        const int32_t* row0, const int32_t* T, const FilesSetup& u, bool emit) {
  const FilesWorkspace& w = u.w;
  if (hipMemcpyAsync(w.row0, row0, 4 * ((size_t)num_files + 1), hipMemcpyHostToDevice, s) != hipSuccess ||
      (num_files && hipMemcpyAsync(w.T, T, 4 * (size_t)num_files, hipMemcpyHostToDevice, s) != hipSuccess)) {
    set_error("%s: uploading the file tables failed", who);
    return 1;
  }
  hipLaunchKernelGGL(k_files_index, dim3(cdiv(u.nchunks, 256)), dim3(256), 0, s, w.row0, w.T, num_files, u.nchunks,
                     w.where);
  hipLaunchKernelGGL(k_files_reduce, dim3(u.ntiles), dim3(RG_THREADS), 0, s, scores, u.rows, K, u.f, w.tile_map);
  hipLaunchKernelGGL(k_files_scan, dim3(1), dim3(64), 0, s, w.tile_map, u.ntiles, w.state_in);
  hipLaunchKernelGGL(k_files_apply, dim3(u.ntiles), dim3(RG_THREADS), 0, s, scores, u.rows, K, u.f, w.state_in,
                     emit ? w.events : nullptr, w.chunk_cnt, u.nchunks);
  hipLaunchKernelGGL(k_files_offsets, dim3(1), dim3(64 * K), 0, s, w.chunk_cnt, u.nchunks, w.chunk_off, w.n_raw);
  return 0;
}

static int files_read_counts(const char* who, hipStream_t s, const int* dev, int K, int32_t* host) {
  if (hipMemcpyAsync(host, dev, sizeof(int32_t) * (size_t)K, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    set_error("%s: reading the region counts back failed: %s", who, hipGetErrorString(hipGetLastError()));
    return 1;
  }
  return 0;
}

}  // namespace pa

extern "C" {

size_t pa_binarize_regions_files_workspace_bytes(long rows, int K, int num_files, long raw_rows) {
  if (rows < 0 || rows > 0x7fffffffL || K <= 0 || K > pa::RG_MAXK || num_files < 0 || raw_rows < 0) return 0;
  return pa::carved_bytes([&](pa::Carver& c) { pa::files_layout(c, rows, K, num_files, raw_rows); });
}

int pa_binarize_regions_files_count(const float* scores, int K, int num_files, const int32_t* row0, const int32_t* T,
                                    const float* onset, const float* offset, int32_t* n_raw, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  const char* who = "pa_binarize_regions_files_count";
  const double zero[pa::RG_MAXK] = {0.0};
  pa::FilesSetup u;
  if (int rc = pa::files_setup(who, scores, K, num_files, row0, T, onset, offset, zero, zero, 0.0, 0.0, 0.0, 0,
                               workspace, workspace_bytes, &u))
    return rc;
  PA_REQUIRE(n_raw, "%s: null count array", who);
  for (int k = 0; k < K; ++k) n_raw[k] = 0;
  if (u.rows == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  {
    pa::ProfScope prof("k_regions_files_count", stream, 4.0 * u.rows * K, 8.0 * u.rows * K + 16.0 * u.nchunks * K);
    if (int rc = pa::files_launch(who, s, scores, K, num_files, row0, T, u, false)) return rc;
    PA_CHECK_LAUNCH(who);
  }
  // the one read-back the row buffers are sized from (it also keeps the host tables alive until they are uploaded)
  return pa::files_read_counts(who, s, u.w.n_raw, K, n_raw);
}

int pa_binarize_regions_files_emit(const float* scores, int K, int num_files, const int32_t* row0, const int32_t* T,
                                   const float* onset, const float* offset, const double* min_duration_on,
                                   const double* min_duration_off, double start, double duration, double step,
                                   const int32_t* n_raw, long rows_out, double* regions, int32_t* tracks,
                                   int32_t* list_off, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "pa_binarize_regions_files_emit";
  PA_REQUIRE(n_raw && list_off, "%s: null raw counts / offset table", who);
  long raw_rows = 0;
  pa::FilesRows r;
  for (int k = 0; k < pa::RG_MAXK; ++k) {
    r.first[k] = (int)raw_rows;
    r.room[k] = 0;
    if (k >= K || K > pa::RG_MAXK) continue;
    PA_REQUIRE(n_raw[k] >= 0, "%s: class %d is given %d raw regions", who, k, n_raw[k]);
    r.room[k] = n_raw[k];
    raw_rows += n_raw[k];
    PA_REQUIRE(raw_rows <= 0x7fffffffL, "%s: more than 2^31 - 1 raw regions", who);
  }
  pa::FilesSetup u;
  if (int rc = pa::files_setup(who, scores, K, num_files, row0, T, onset, offset, min_duration_on, min_duration_off,
                               start, duration, step, raw_rows, workspace, workspace_bytes, &u))
    return rc;
  PA_REQUIRE(rows_out >= raw_rows && (regions || raw_rows == 0), "%s: room for %ld rows, %ld needed", who, rows_out,
             raw_rows);
  hipStream_t s = (hipStream_t)stream;
  const int lists = num_files * K;
  if (u.rows == 0 || lists == 0) {
    if (pa::fill_async(list_off, 0, sizeof(int32_t) * ((size_t)lists + 1), s) != hipSuccess) {
      pa::set_error("%s: the fill launch failed", who);
      return 1;
    }
    return 0;
  }
  const pa::FilesWorkspace& w = u.w;
  {
    pa::ProfScope prof("k_regions_files_emit", stream, 4.0 * u.rows * K, 8.0 * u.rows * K + 8.0 * u.rows +
                       16.0 * u.nchunks * K + 64.0 * raw_rows);
    if (int rc = pa::files_launch(who, s, scores, K, num_files, row0, T, u, true)) return rc;
    hipLaunchKernelGGL(pa::k_files_emit, dim3(pa::cdiv(u.rows, pa::RG_THREADS)), dim3(pa::RG_THREADS), 0, s,
                       w.events, u.rows, K, u.f, w.chunk_off, u.nchunks, r, w.raw);
    hipLaunchKernelGGL(pa::k_files_merge, dim3(lists), dim3(pa::RG_THREADS), 0, s, K, u.f, w.row0, w.chunk_off,
                       u.nchunks, r, w.raw, w.tmp, w.n_merged, w.counts);
    hipLaunchKernelGGL(pa::k_files_list_off, dim3(1), dim3(64), 0, s, w.counts, lists, list_off);
    hipLaunchKernelGGL(pa::k_files_remove, dim3(lists), dim3(pa::RG_THREADS), 0, s, K, u.f, w.row0, w.chunk_off,
                       u.nchunks, r, w.raw, w.n_merged, list_off, (int)std::min<long>(rows_out, 0x7fffffffL), regions,
                       tracks);
    PA_CHECK_LAUNCH(who);
  }
  // the host tables were handed to asynchronous copies: they must outlive them.  The same wait tells whether the
  // counts the row buffers were sized from are the counts of these scores.
  int32_t seen[pa::RG_MAXK];
  if (int rc = pa::files_read_counts(who, s, w.n_raw, K, seen)) return rc;
  for (int k = 0; k < K; ++k)
    PA_REQUIRE(seen[k] == n_raw[k], "%s: class %d has %d raw regions, the call was given %d", who, k, seen[k],
               n_raw[k]);
  return 0;
}

}  // extern "C"
