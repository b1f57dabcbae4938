// Replay of recorded files through the online rule (include/pyannote_amd_online.h, pao_replay): one workgroup per job
// -- a file and a threshold triple -- walks every chunk of its file on the device: the clustering step, then the
// overlap-add and emission, then the flush, with no host in the loop.  The rule is that of online_rule.h, the very
// functions k_online_cluster_step and k_online_emit call, so a replay gives what the same chunks give streamed.
//
// A job works on its own rows of the state in global memory (they stay in L2: a few hundred KB per job), so any K, D
// and R the single-step kernels take work here too.  Steps of one job are ordered by workgroup barriers; jobs never
// communicate: no atomics, every element has one writer.
// hipcc-flags: -ffp-contract=off
#include <algorithm>
#include <vector>

#include "online_rule.h"
#include "pyannote_amd_online.h"

namespace pa {

// one file-table row is usable: it lies inside the concatenated inputs and its emission fits the int indices
__host__ __device__ __forceinline__ bool replay_file_valid(const long long* f, long long num_chunks,
                                                           long long num_sched, int K) {
  const long long off = f[0], C = f[1], so = f[2], total = f[3];
  return off >= 0 && C >= 0 && C <= num_chunks && off <= num_chunks - C && so >= 0 && C + 1 <= num_sched &&
         so <= num_sched - (C + 1) && total >= 0 && total <= INT_MAX / ON_K && K <= ON_K;
}

// row c of a file's schedule is consistent with the row before it (prev_to: that row's emit_to; the first row has
// none and starts the file at its own emit_from >= 0)
__host__ __device__ __forceinline__ bool replay_row_valid(const long long* row, bool first, long long prev_to,
                                                          bool last, int F, int R) {
  const long long g0 = row[0], ga = row[1], gb = row[2];
  return online_frames_valid(g0, ga, gb, F, R, gb - ga) && (first || ga == prev_to) && (!last || g0 < 0);
}

__global__ __launch_bounds__(ON_T) void k_online_replay(
    const float* __restrict__ emb, const int* __restrict__ active, const int* __restrict__ clean,
    const uint8_t* __restrict__ seg, long long num_chunks, int F, int S, int D, const long long* __restrict__ files,
    int num_files, const long long* __restrict__ sched, long long num_sched, const int* __restrict__ jobs,
    const double* __restrict__ delta_new, const long long* __restrict__ offsets, int J, long long map_rows,
    long long out_rows, int K, int R, double* centroid_sum, int* centroid_n, int* acc_sum, int* acc_cnt, int* map,
    uint8_t* out) {
  __shared__ OnlineStepShared sh;
  __shared__ int s_ok;
  const int j = blockIdx.x, tid = threadIdx.x;
  const int file = jobs[3 * j];
  // where the job's rows are: without that nothing can be written safely
  if (file < 0 || file >= num_files) return;
  const long long* ft = files + 4 * (long)file;
  if (!replay_file_valid(ft, num_chunks, num_sched, K)) return;
  const long long c0 = ft[0], C = ft[1], total = ft[3];
  const long long* sc = sched + 3 * ft[2];
  const long long mo = offsets[2 * j], oo = offsets[2 * j + 1];
  if (mo < 0 || mo > map_rows - C || oo < 0 || oo > out_rows - total || C > map_rows || total > out_rows) return;
  if (tid == 0) s_ok = 1;
  __syncthreads();
  // ... and no other job's rows under them (the host refuses this; a second line of defence)
  for (int o = tid; o < J; o += ON_T) {
    if (o == j) continue;
    const int f2 = jobs[3 * o];
    if (f2 < 0 || f2 >= num_files) continue;   // (writes nothing)
    const long long C2 = files[4 * (long)f2 + 1], t2 = files[4 * (long)f2 + 3];
    const long long mo2 = offsets[2 * o], oo2 = offsets[2 * o + 1];
    if (C > 0 && C2 > 0 && mo < mo2 + C2 && mo2 < mo + C) s_ok = 0;
    if (total > 0 && t2 > 0 && oo < oo2 + t2 && oo2 < oo + total) s_ok = 0;
  }
  __syncthreads();
  if (!s_ok) return;
  __syncthreads();
  // the schedule: the same conditions as on the host
  for (long long c = tid; c <= C; c += ON_T)
    if (!replay_row_valid(sc + 3 * c, c == 0, c == 0 ? 0 : sc[3 * (c - 1) + 2], c == C, F, R)) s_ok = 0;
  if (tid == 0 && sc[3 * C + 2] - sc[1] != total) s_ok = 0;
  __syncthreads();
  int* mp = map + mo * S;
  uint8_t* o = out + oo * K;
  if (!s_ok) {   // the state is left alone
    for (long long i = tid; i < C * S; i += ON_T) mp[i] = -1;
    for (long long i = tid; i < total * K; i += ON_T) o[i] = 0;
    return;
  }
  const int min_active = jobs[3 * j + 1], min_update = jobs[3 * j + 2];
  const double delta = delta_new[j];
  double* csum = centroid_sum + (long)j * K * D;
  int* cn = centroid_n + (long)j * K;
  int* sum = acc_sum + (long)j * R * K;
  int* cnt = acc_cnt + (long)j * R;
  const long long first = sc[1];
  for (long long c = 0; c <= C; ++c) {
    const long long g0 = sc[3 * c], ga = sc[3 * c + 1], gb = sc[3 * c + 2];
    const int* m = nullptr;
    if (c < C) {
      m = mp + c * S;
      online_cluster_step_one(sh, emb + (c0 + c) * S * D, active + (c0 + c) * S, clean + (c0 + c) * S, S, D, K,
                              min_active, min_update, delta, csum, cn, mp + c * S);
      __syncthreads();
    }
    online_emit_one(seg + (c0 + (c < C ? c : 0)) * F * S, F, S, m, g0, ga, gb, R, K, (int)(gb - ga), sum, cnt,
                    o + (ga - first) * K);
    __syncthreads();
  }
}

}  // namespace pa

extern "C" {

int pao_replay(const float* emb, const int32_t* active, const int32_t* clean, const uint8_t* seg, int64_t num_chunks,
               int F, int S, int D, const int64_t* files, const int64_t* files_host, int num_files,
               const int64_t* sched, const int64_t* sched_host, int64_t num_sched, const int32_t* jobs,
               const int32_t* jobs_host, const double* delta_new, const int64_t* offsets,
               const int64_t* offsets_host, int J, int64_t map_rows, int64_t out_rows, int K, int R,
               double* centroid_sum, int32_t* centroid_n, int32_t* acc_sum, int32_t* acc_cnt, int32_t* map,
               uint8_t* out, void* stream) {
  PA_REQUIRE(S >= 1 && S <= pa::ON_S, "pao_replay: %d local speakers per chunk, the kernel handles 1..%d", S, pa::ON_S);
  PA_REQUIRE(K >= 1 && K <= pa::ON_K, "pao_replay: %d global speakers per stream, the kernel handles 1..%d", K,
             pa::ON_K);
  PA_REQUIRE(D >= 1 && F >= 1 && R >= F && J >= 0 && num_files >= 0 && num_chunks >= 0 && num_sched >= 0 &&
                 map_rows >= 0 && out_rows >= 0,
             "pao_replay: needs D >= 1, F >= 1, R >= F and counts >= 0 (got D = %d, F = %d, R = %d)", D, F, R);
  PA_REQUIRE((long)R * (K + 1) <= INT_MAX, "pao_replay: ring too large");
  PA_REQUIRE(files_host != nullptr && sched_host != nullptr && jobs_host != nullptr && offsets_host != nullptr,
             "pao_replay: the host copies of the file table, the schedule, the job table and the offsets are required: "
             "the loop bounds come from them");
  for (int f = 0; f < num_files; ++f) {
    const int64_t* ft = files_host + 4 * (long)f;
    PA_REQUIRE(pa::replay_file_valid((const long long*)ft, num_chunks, num_sched, K),
               "pao_replay: file %d (chunks [%lld, +%lld), schedule rows from %lld, %lld frames) runs past the %lld "
               "chunks or the %lld schedule rows", f, (long long)ft[0], (long long)ft[1], (long long)ft[2],
               (long long)ft[3], (long long)num_chunks, (long long)num_sched);
    const long long* sc = (const long long*)sched_host + 3 * ft[2];
    const int64_t C = ft[1];
    for (int64_t c = 0; c <= C; ++c)
      PA_REQUIRE(pa::replay_row_valid(sc + 3 * c, c == 0, c == 0 ? 0 : sc[3 * (c - 1) + 2], c == C, F, R),
                 "pao_replay: inconsistent schedule of file %d, row %lld: chunk at %lld (F = %d), emission [%lld, %lld)"
                 ", R = %d%s", f, (long long)c, sc[3 * c], F, sc[3 * c + 1], sc[3 * c + 2], R,
                 c == C ? " (the last row is the flush: start_frame < 0)" : "");
    PA_REQUIRE(sc[3 * C + 2] - sc[1] == ft[3], "pao_replay: the schedule of file %d emits %lld frames, its frame "
               "total is %lld", f, sc[3 * C + 2] - sc[1], (long long)ft[3]);
  }
  std::vector<std::pair<int64_t, int64_t>> rows_map, rows_out;   // (offset, length) of the non-empty ranges
  for (int j = 0; j < J; ++j) {
    const int file = jobs_host[3 * (long)j];
    PA_REQUIRE(file >= 0 && file < num_files, "pao_replay: job %d names file %d of %d", j, file, num_files);
    const int64_t C = files_host[4 * (long)file + 1], total = files_host[4 * (long)file + 3];
    const int64_t mo = offsets_host[2 * (long)j], oo = offsets_host[2 * (long)j + 1];
    PA_REQUIRE(mo >= 0 && C <= map_rows && mo <= map_rows - C && oo >= 0 && total <= out_rows && oo <= out_rows - total,
               "pao_replay: job %d writes map rows [%lld, +%lld) of %lld and out rows [%lld, +%lld) of %lld", j,
               (long long)mo, (long long)C, (long long)map_rows, (long long)oo, (long long)total, (long long)out_rows);
    if (C > 0) rows_map.emplace_back(mo, C);
    if (total > 0) rows_out.emplace_back(oo, total);
  }
  for (auto* rows : {&rows_map, &rows_out}) {
    std::sort(rows->begin(), rows->end());
    for (size_t i = 1; i < rows->size(); ++i)
      PA_REQUIRE((*rows)[i - 1].first + (*rows)[i - 1].second <= (*rows)[i].first,
                 "pao_replay: two jobs share %s rows [%lld, %lld)", rows == &rows_map ? "map" : "out",
                 (long long)(*rows)[i].first, (long long)((*rows)[i - 1].first + (*rows)[i - 1].second));
  }
  if (J == 0) return 0;
  pa::ProfScope prof("k_online_replay", stream, 0.0, 0.0);
  hipLaunchKernelGGL(pa::k_online_replay, dim3(J), dim3(pa::ON_T), 0, (hipStream_t)stream, emb, active, clean, seg,
                     (long long)num_chunks, F, S, D, (const long long*)files, num_files, (const long long*)sched,
                     (long long)num_sched, jobs, delta_new, (const long long*)offsets, J, (long long)map_rows,
                     (long long)out_rows, K, R, centroid_sum, centroid_n, acc_sum, acc_cnt, map, out);
  PA_CHECK_LAUNCH("pao_replay");
  return 0;
}

}  // extern "C"
