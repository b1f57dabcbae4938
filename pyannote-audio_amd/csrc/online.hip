// Online (streaming) speaker diarization on gfx950: the incremental clustering step and the rolling overlap-add that
// advance every listed stream of a bank by one chunk, one launch each (include/pyannote_amd_online.h has the rule;
// Coria et al., "Overlap-aware low-latency online speaker diarization based on end-to-end local segmentation",
// ASRU 2021).  The state of a bank stays on the device between calls.
//
// One workgroup per stream, no communication between workgroups, no atomics: every state element has one writer.
// Distances are those of pa_cdist_cosine_f64 (cosine_f64.h): one thread per (local speaker, centroid) pair walks k in
// SciPy's order, so the file is compiled without contraction like cluster.hip.
// hipcc-flags: -ffp-contract=off
#include "online_rule.h"
#include "pyannote_amd_online.h"

namespace pa {

// the rule itself is in online_rule.h: these two kernels apply it to one chunk of every listed stream
__global__ __launch_bounds__(ON_T) void k_online_cluster_step(
    const int* __restrict__ slots, int N, const float* __restrict__ emb, const int* __restrict__ active,
    const int* __restrict__ clean, int S, int D, int K, int min_active, int min_update, double delta_new,
    double* centroid_sum, int* centroid_n, int* __restrict__ map) {
  __shared__ OnlineStepShared sh;
  const int m = blockIdx.x, tid = threadIdx.x;
  const int slot = slots[m];
  if (slot < 0 || slot >= N) {   // (refused on the host when the caller hands slots_host along)
    if (tid < S) map[m * S + tid] = -1;
    return;
  }
  online_cluster_step_one(sh, emb + (long)m * S * D, active + (long)m * S, clean + (long)m * S, S, D, K, min_active,
                          min_update, delta_new, centroid_sum + (long)slot * K * D, centroid_n + (long)slot * K,
                          map + (long)m * S);
}

__global__ __launch_bounds__(ON_T) void k_online_emit(
    const int* __restrict__ slots, int N, const uint8_t* __restrict__ seg, int F, int S, const int* __restrict__ map,
    const long long* __restrict__ start_frame, const long long* __restrict__ emit_from,
    const long long* __restrict__ emit_to, int R, int K, int E, int* acc_sum, int* acc_cnt,
    uint8_t* __restrict__ out) {
  const int m = blockIdx.x, tid = threadIdx.x;
  const int slot = slots[m];
  uint8_t* o = out + (long)m * E * K;
  const long long g0 = start_frame[m], ga = emit_from[m], gb = emit_to[m];
  // whatever the frames say, nothing below may leave the stream's own rows: the same conditions as on the host
  if (!(slot >= 0 && slot < N && online_frames_valid(g0, ga, gb, F, R, E))) {
    for (int i = tid; i < E * K; i += ON_T) o[i] = 0;
    return;
  }
  online_emit_one(seg + (long)m * F * S, F, S, map + (long)m * S, g0, ga, gb, R, K, E, acc_sum + (long)slot * R * K,
                  acc_cnt + (long)slot * R, o);
}

}  // namespace pa

extern "C" {

int pao_cluster_step_limits(int* max_local_host, int* max_speakers_host) {
  if (max_local_host != nullptr) *max_local_host = pa::ON_S;
  if (max_speakers_host != nullptr) *max_speakers_host = pa::ON_K;
  return 0;
}

int pao_cluster_step(const int32_t* slots, const int32_t* slots_host, int M, int N, const float* emb,
                     const int32_t* active, const int32_t* clean, int S, int D, int K, int min_active_frames,
                     int min_update_frames, double delta_new, double* centroid_sum, int32_t* centroid_n,
                     int32_t* map, void* stream) {
  PA_REQUIRE(S >= 1 && S <= pa::ON_S, "pao_cluster_step: %d local speakers per chunk, the kernel handles 1..%d", S,
             pa::ON_S);
  PA_REQUIRE(K >= 1 && K <= pa::ON_K, "pao_cluster_step: %d global speakers per stream, the kernel handles 1..%d", K,
             pa::ON_K);
  PA_REQUIRE(D >= 1 && N >= 1 && M >= 0, "pao_cluster_step: needs D >= 1, N >= 1, M >= 0 (got %d, %d, %d)", D, N, M);
  if (int rc = pa::check_slots("pao_cluster_step", slots_host, M, N)) return rc;
  if (M == 0) return 0;
  pa::ProfScope prof("k_online_cluster_step", stream, 2.0 * M * S * K * (double)D,
                     (double)M * (4.0 * S * D + 8.0 * K * D));
  hipLaunchKernelGGL(pa::k_online_cluster_step, dim3(M), dim3(pa::ON_T), 0, (hipStream_t)stream, slots, N, emb, active,
                     clean, S, D, K, min_active_frames, min_update_frames, delta_new, centroid_sum, centroid_n, map);
  PA_CHECK_LAUNCH("pao_cluster_step");
  return 0;
}

int pao_emit(const int32_t* slots, const int32_t* slots_host, int M, int N, const uint8_t* seg, int F, int S,
             const int32_t* map, const int64_t* start_frame, const int64_t* emit_from, const int64_t* emit_to,
             const int64_t* frames_host, int R, int K, int E, int32_t* acc_sum, int32_t* acc_cnt, uint8_t* out,
             void* stream) {
  PA_REQUIRE(S >= 1 && S <= pa::ON_S, "pao_emit: %d local speakers per chunk, the kernel handles 1..%d", S, pa::ON_S);
  PA_REQUIRE(K >= 1 && K <= pa::ON_K, "pao_emit: %d global speakers per stream, the kernel handles 1..%d", K,
             pa::ON_K);
  PA_REQUIRE(F >= 1 && E >= 0 && N >= 1 && M >= 0, "pao_emit: needs F >= 1, E >= 0, N >= 1, M >= 0");
  PA_REQUIRE((long)R >= (long)F + E, "pao_emit: a ring of %d frames is shorter than F + E = %d + %d", R, F, E);
  PA_REQUIRE((long)R * (K + 1) <= INT_MAX && (long)E * K <= INT_MAX, "pao_emit: ring or emission block too large");
  if (int rc = pa::check_slots("pao_emit", slots_host, M, N)) return rc;
  if (frames_host != nullptr)
    for (int i = 0; i < M; ++i) {
      const int64_t g0 = frames_host[i], ga = frames_host[M + i], gb = frames_host[2 * (long)M + i];
      PA_REQUIRE(pa::online_frames_valid(g0, ga, gb, F, R, E),
                 "pao_emit: inconsistent frames of entry %d: chunk at %lld (F = %d), emission [%lld, %lld), E = %d, "
                 "R = %d", i, (long long)g0, F, (long long)ga, (long long)gb, E, R);
    }
  if (M == 0) return 0;
  pa::ProfScope prof("k_online_emit", stream, 0.0, (double)M * ((double)F * S + (double)E * K + 8.0 * F * (K + 1)));
  hipLaunchKernelGGL(pa::k_online_emit, dim3(M), dim3(pa::ON_T), 0, (hipStream_t)stream, slots, N, seg, F, S, map,
                     (const long long*)start_frame, (const long long*)emit_from, (const long long*)emit_to, R, K, E,
                     acc_sum, acc_cnt, out);
  PA_CHECK_LAUNCH("pao_emit");
  return 0;
}

}  // extern "C"
