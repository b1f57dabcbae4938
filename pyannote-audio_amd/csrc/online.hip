// Online (streaming) speaker diarization on gfx950: the incremental clustering step and the rolling overlap-add that
// advance every listed stream of a bank by one chunk, one launch each (include/pyannote_amd_online.h has the rule;
// Coria et al., "Overlap-aware low-latency online speaker diarization based on end-to-end local segmentation",
// ASRU 2021).  The state of a bank stays on the device between calls.
//
// One workgroup per stream, no communication between workgroups, no atomics: every state element has one writer.
// Distances are those of pa_cdist_cosine_f64 (cosine_f64.h): one thread per (local speaker, centroid) pair walks k in
// SciPy's order, so the file is compiled without contraction like cluster.hip.
// hipcc-flags: -ffp-contract=off
#include <limits.h>

#include "common.h"
#include "cosine_f64.h"
#include "pyannote_amd_online.h"

namespace pa {

constexpr int ON_S = 4;      // local speakers per chunk
constexpr int ON_K = 32;     // global speakers per stream (one 32-bit mask of held / occupied centroids)
constexpr int ON_T = 256;    // threads per workgroup

// (total, code) candidates of the exhaustive search: the smaller total wins, equal totals -> the smaller code, which
// is the lexicographically smaller tuple (digit of speaker 0 first, "unmapped" the largest digit)
__device__ __forceinline__ bool on_better(double ta, int ca, double tb, int cb) {
  return ta < tb || (ta == tb && ca < cb);
}

__global__ __launch_bounds__(ON_T) void k_online_cluster_step(
    const int* __restrict__ slots, int N, const float* __restrict__ emb, const int* __restrict__ active,
    const int* __restrict__ clean, int S, int D, int K, int min_active, int min_update, double delta_new,
    double* centroid_sum, int* centroid_n, int* __restrict__ map) {
  __shared__ double s_dist[ON_S][ON_K];   // d[s][k] for present s and occupied k
  __shared__ double s_nk[ON_K];           // |centroid_sum[k]|
  __shared__ double s_ns[ON_S];           // |emb[s]|
  __shared__ int s_finite[ON_S];
  __shared__ int s_cn[ON_K];              // centroid_n before the step
  __shared__ double s_rt[ON_T];
  __shared__ int s_rc[ON_T];
  __shared__ int s_ps[ON_S], s_oc[ON_K];  // present speakers / occupied centroids, ascending
  __shared__ int s_P, s_Kocc;
  __shared__ int s_act[ON_S], s_tgt[ON_S];   // per speaker: 0 nothing, 1 found, 2 update; the centroid

  const int m = blockIdx.x, tid = threadIdx.x;
  const int slot = slots[m];
  if (slot < 0 || slot >= N) {   // (refused on the host when the caller hands slots_host along)
    if (tid < S) map[m * S + tid] = -1;
    return;
  }
  const float* e = emb + (long)m * S * D;
  double* csum = centroid_sum + (long)slot * K * D;
  int* cn = centroid_n + (long)slot * K;

  // norms and finiteness: S + K rows, one thread each
  if (tid < S) {
    const float* row = e + (long)tid * D;
    int fin = 1;
    for (int k = 0; k < D; ++k) fin &= (int)(fabsf(row[k]) <= 3.402823466e38f);   // false for NaN and Inf
    s_finite[tid] = fin;
    s_ns[tid] = __dsqrt_rn(dot2way_as_f64(row, row, D));
  } else if (tid >= 64 && tid < 64 + K) {
    const int k = tid - 64;
    const int n = cn[k];
    s_cn[k] = n;
    s_nk[k] = n > 0 ? row_norm_f64(csum + (long)k * D, D) : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    int P = 0, Kocc = 0;
    for (int s = 0; s < S; ++s)
      if (active[m * S + s] >= min_active && s_finite[s] && s_ns[s] > 0.0) s_ps[P++] = s;
    for (int k = 0; k < K; ++k)
      if (s_cn[k] > 0) s_oc[Kocc++] = k;
    s_P = P;
    s_Kocc = Kocc;
  }
  __syncthreads();
  const int P = s_P, Kocc = s_Kocc;
  // distances: one thread per (present speaker, occupied centroid)
  for (int p = tid; p < P * Kocc; p += ON_T) {
    const int s = s_ps[p / Kocc], k = s_oc[p % Kocc];
    s_dist[s][k] = cosine_distance_f64(dot2way_as_f64(e + (long)s * D, csum + (long)k * D, D), s_ns[s], s_nk[k]);
  }
  __syncthreads();

  // optimal map: every tuple of digits in [0, Kocc] (Kocc = unmapped), one digit per present speaker
  const int need = P < Kocc ? P : Kocc;
  double best = __builtin_inf();
  int best_code = INT_MAX;
  if (P > 0 && need > 0) {
    const int B = Kocc + 1;
    int total_codes = 1;
    for (int i = 0; i < P; ++i) total_codes *= B;   // <= 33^4
    for (int code = tid; code < total_codes; code += ON_T) {
      int dg[ON_S];
      int c = code;
      for (int i = P - 1; i >= 0; --i) {
        dg[i] = c % B;
        c /= B;
      }
      unsigned used = 0u;
      int cnt = 0;
      bool ok = true;
      double tot = 0.0;
      for (int i = 0; i < P; ++i) {
        if (dg[i] == Kocc) continue;
        const unsigned bit = 1u << dg[i];
        if (used & bit) {
          ok = false;
          break;
        }
        used |= bit;
        ++cnt;
        tot = tot + s_dist[s_ps[i]][s_oc[dg[i]]];
      }
      if (ok && cnt == need && on_better(tot, code, best, best_code)) {
        best = tot;
        best_code = code;
      }
    }
  }
  s_rt[tid] = best;
  s_rc[tid] = best_code;
  __syncthreads();
  for (int o = ON_T / 2; o > 0; o >>= 1) {
    if (tid < o && on_better(s_rt[tid + o], s_rc[tid + o], s_rt[tid], s_rc[tid])) {
      s_rt[tid] = s_rt[tid + o];
      s_rc[tid] = s_rc[tid + o];
    }
    __syncthreads();
  }

  // matching, founding, forcing: a handful of decisions, one thread
  if (tid == 0) {
    int mp[ON_S], matched[ON_S];
    for (int s = 0; s < ON_S; ++s) {
      mp[s] = -1;
      matched[s] = 0;
      s_act[s] = 0;
      s_tgt[s] = -1;
    }
    unsigned held = 0u, occupied = 0u;
    for (int j = 0; j < Kocc; ++j) occupied |= 1u << s_oc[j];
    int code = s_rc[0];
    if (code != INT_MAX) {
      const int B = Kocc + 1;
      for (int i = P - 1; i >= 0; --i) {
        const int d = code % B;
        code /= B;
        if (d == Kocc) continue;
        const int s = s_ps[i], k = s_oc[d];
        if (s_dist[s][k] > delta_new) continue;   // un-mapped
        mp[s] = k;
        matched[s] = 1;
        held |= 1u << k;
      }
    }
    unsigned taken = occupied;   // occupied before the step or founded in it
    for (int i = 0; i < P; ++i) {
      const int s = s_ps[i];
      const bool is_long = clean[m * S + s] >= min_update;
      if (matched[s]) {
        if (is_long) {
          s_act[s] = 2;
          s_tgt[s] = mp[s];
        }
        continue;
      }
      int free_k = -1;
      if (is_long)
        for (int k = 0; k < K; ++k)
          if (!(taken & (1u << k))) {
            free_k = k;
            break;
          }
      if (free_k >= 0) {
        mp[s] = free_k;
        taken |= 1u << free_k;
        held |= 1u << free_k;
        s_act[s] = 1;
        s_tgt[s] = free_k;
        continue;
      }
      int bk = -1;
      double bd = 0.0;
      for (int j = 0; j < Kocc; ++j) {   // ascending k: a strict < keeps the lower index on ties
        const int k = s_oc[j];
        if (held & (1u << k)) continue;
        const double d = s_dist[s][k];
        if (bk < 0 || d < bd) {
          bk = k;
          bd = d;
        }
      }
      if (bk >= 0) {
        mp[s] = bk;
        held |= 1u << bk;
      }
    }
    for (int s = 0; s < S; ++s) {
      map[m * S + s] = mp[s];
      if (s_act[s] == 1) cn[s_tgt[s]] = 1;
      if (s_act[s] == 2) cn[s_tgt[s]] = s_cn[s_tgt[s]] + 1;
    }
  }
  __syncthreads();
  // state: the map is injective, so every (k, column) has at most one writer
  for (int s = 0; s < S; ++s) {
    const int act = s_act[s];
    if (act == 0) continue;
    double* dst = csum + (long)s_tgt[s] * D;
    const float* row = e + (long)s * D;
    if (act == 1)
      for (int k = tid; k < D; k += ON_T) dst[k] = (double)row[k];
    else
      for (int k = tid; k < D; k += ON_T) dst[k] = dst[k] + (double)row[k];
  }
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
  const bool valid = slot >= 0 && slot < N && ga >= 0 && ga <= gb && gb - ga <= E && (g0 < 0 || g0 + F - ga <= R);
  if (!valid) {
    for (int i = tid; i < E * K; i += ON_T) o[i] = 0;
    return;
  }
  int* sum = acc_sum + (long)slot * R * K;
  int* cnt = acc_cnt + (long)slot * R;
  int mp[ON_S];
  for (int s = 0; s < ON_S; ++s) {
    const int k = s < S ? map[m * S + s] : -1;
    mp[s] = (k >= 0 && k < K) ? k : -1;
  }
  // overlap-add: a thread owns a frame, F <= R frames fall on distinct ring rows
  for (int f = tid; f < F && g0 >= 0; f += ON_T) {   // (g0 < 0: a flush, no chunk to add)
    const long long g = g0 + f;
    if (g < ga) continue;
    const int r = (int)(g % R);
    cnt[r] = cnt[r] + 1;
    const uint8_t* row = seg + ((long)m * F + f) * S;
    for (int s = 0; s < S; ++s)
      if (mp[s] >= 0 && row[s]) sum[(long)r * K + mp[s]] = sum[(long)r * K + mp[s]] + 1;
  }
  __syncthreads();
  for (int i = tid; i < E * K; i += ON_T) {
    const int k = i % K;
    const long long g = ga + i / K;
    uint8_t v = 0;
    if (g < gb) {
      const int r = (int)(g % R);
      v = (uint8_t)(2 * sum[(long)r * K + k] > cnt[r]);
    }
    o[i] = v;
  }
  __syncthreads();
  const int n = (int)(gb - ga);
  for (int i = tid; i < n * (K + 1); i += ON_T) {
    const int r = (int)((ga + i / (K + 1)) % R), k = i % (K + 1);
    if (k < K)
      sum[(long)r * K + k] = 0;
    else
      cnt[r] = 0;
  }
}

// slots_host: distinct and inside [0, N)
static int check_slots(const char* who, const int32_t* slots_host, int M, int N) {
  if (slots_host == nullptr) return 0;
  for (int i = 0; i < M; ++i) {
    PA_REQUIRE(slots_host[i] >= 0 && slots_host[i] < N, "%s: slot %d (entry %d) outside the bank of %d", who,
               (int)slots_host[i], i, N);
    for (int j = 0; j < i; ++j)   // (a step lists a few hundred slots at most)
      PA_REQUIRE(slots_host[i] != slots_host[j], "%s: duplicate slot %d (entries %d and %d): one workgroup owns one "
                 "stream", who, (int)slots_host[i], j, i);
  }
  return 0;
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
      PA_REQUIRE(ga >= 0 && ga <= gb && gb - ga <= E && (g0 < 0 || g0 + F - ga <= R),
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
