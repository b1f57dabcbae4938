// The online diarization rule for ONE stream, as device functions (include/pyannote_amd_online.h states it): one
// incremental clustering step and one rolling overlap-add with emission.  k_online_cluster_step and k_online_emit
// (online.hip) apply them to one chunk of every listed stream; k_online_replay (online_replay.hip) applies them to
// every chunk of a recorded file in turn.  The rule lives here and nowhere else.
//
// Both are called by a whole workgroup of ON_T threads with uniform arguments; the pointers are those of the stream
// (no slot or chunk index is applied here).  Files that include this are compiled with -ffp-contract=off: the distances
// are those of pa_cdist_cosine_f64 (cosine_f64.h).
#pragma once
#include <limits.h>

#include "common.h"
#include "cosine_f64.h"

namespace pa {

constexpr int ON_S = 4;      // local speakers per chunk
constexpr int ON_K = 32;     // global speakers per stream (one 32-bit mask of held / occupied centroids)
constexpr int ON_T = 256;    // threads per workgroup

// (total, code) candidates of the exhaustive search: the smaller total wins, equal totals -> the smaller code, which
// is the lexicographically smaller tuple (digit of speaker 0 first, "unmapped" the largest digit)
__device__ __forceinline__ bool on_better(double ta, int ca, double tb, int cb) {
  return ta < tb || (ta == tb && ca < cb);
}

// LDS of one clustering step (a kernel declares one, __shared__)
struct OnlineStepShared {
  double dist[ON_S][ON_K];   // d[s][k] for present s and occupied k
  double nk[ON_K];           // |centroid_sum[k]|
  double ns[ON_S];           // |emb[s]|
  int finite[ON_S];
  int cn[ON_K];              // centroid_n before the step
  double rt[ON_T];
  int rc[ON_T];
  int ps[ON_S], oc[ON_K];    // present speakers / occupied centroids, ascending
  int P, Kocc;
  int act[ON_S], tgt[ON_S];  // per speaker: 0 nothing, 1 found, 2 update; the centroid
};

// Rule items 1-8 for one stream: e (S, D), active / clean (S), csum (K, D) and cn (K) updated in place, map (S)
// written.  The caller puts a __syncthreads() behind it before anything reads the state or `sh` again; the map is
// visible to the workgroup on return.
__device__ __forceinline__ void online_cluster_step_one(OnlineStepShared& sh, const float* e, const int* active,
                                                        const int* clean, int S, int D, int K, int min_active,
                                                        int min_update, double delta_new, double* csum, int* cn,
                                                        int* map) {
  const int tid = threadIdx.x;
  // norms and finiteness: S + K rows, one thread each
  if (tid < S) {
    const float* row = e + (long)tid * D;
    int fin = 1;
    for (int k = 0; k < D; ++k) fin &= (int)(fabsf(row[k]) <= 3.402823466e38f);   // false for NaN and Inf
    sh.finite[tid] = fin;
    sh.ns[tid] = __dsqrt_rn(dot2way_as_f64(row, row, D));
  } else if (tid >= 64 && tid < 64 + K) {
    const int k = tid - 64;
    const int n = cn[k];
    sh.cn[k] = n;
    sh.nk[k] = n > 0 ? row_norm_f64(csum + (long)k * D, D) : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    int P = 0, Kocc = 0;
    for (int s = 0; s < S; ++s)
      if (active[s] >= min_active && sh.finite[s] && sh.ns[s] > 0.0) sh.ps[P++] = s;
    for (int k = 0; k < K; ++k)
      if (sh.cn[k] > 0) sh.oc[Kocc++] = k;
    sh.P = P;
    sh.Kocc = Kocc;
  }
  __syncthreads();
  const int P = sh.P, Kocc = sh.Kocc;
  // distances: one thread per (present speaker, occupied centroid)
  for (int p = tid; p < P * Kocc; p += ON_T) {
    const int s = sh.ps[p / Kocc], k = sh.oc[p % Kocc];
    sh.dist[s][k] = cosine_distance_f64(dot2way_as_f64(e + (long)s * D, csum + (long)k * D, D), sh.ns[s], sh.nk[k]);
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
        tot = tot + sh.dist[sh.ps[i]][sh.oc[dg[i]]];
      }
      if (ok && cnt == need && on_better(tot, code, best, best_code)) {
        best = tot;
        best_code = code;
      }
    }
  }
  sh.rt[tid] = best;
  sh.rc[tid] = best_code;
  __syncthreads();
  for (int o = ON_T / 2; o > 0; o >>= 1) {
    if (tid < o && on_better(sh.rt[tid + o], sh.rc[tid + o], sh.rt[tid], sh.rc[tid])) {
      sh.rt[tid] = sh.rt[tid + o];
      sh.rc[tid] = sh.rc[tid + o];
    }
    __syncthreads();
  }

  // matching, founding, forcing: a handful of decisions, one thread
  if (tid == 0) {
    int mp[ON_S], matched[ON_S];
    for (int s = 0; s < ON_S; ++s) {
      mp[s] = -1;
      matched[s] = 0;
      sh.act[s] = 0;
      sh.tgt[s] = -1;
    }
    unsigned held = 0u, occupied = 0u;
    for (int j = 0; j < Kocc; ++j) occupied |= 1u << sh.oc[j];
    int code = sh.rc[0];
    if (code != INT_MAX) {
      const int B = Kocc + 1;
      for (int i = P - 1; i >= 0; --i) {
        const int d = code % B;
        code /= B;
        if (d == Kocc) continue;
        const int s = sh.ps[i], k = sh.oc[d];
        if (sh.dist[s][k] > delta_new) continue;   // un-mapped
        mp[s] = k;
        matched[s] = 1;
        held |= 1u << k;
      }
    }
    unsigned taken = occupied;   // occupied before the step or founded in it
    for (int i = 0; i < P; ++i) {
      const int s = sh.ps[i];
      const bool is_long = clean[s] >= min_update;
      if (matched[s]) {
        if (is_long) {
          sh.act[s] = 2;
          sh.tgt[s] = mp[s];
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
        sh.act[s] = 1;
        sh.tgt[s] = free_k;
        continue;
      }
      int bk = -1;
      double bd = 0.0;
      for (int j = 0; j < Kocc; ++j) {   // ascending k: a strict < keeps the lower index on ties
        const int k = sh.oc[j];
        if (held & (1u << k)) continue;
        const double d = sh.dist[s][k];
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
      map[s] = mp[s];
      if (sh.act[s] == 1) cn[sh.tgt[s]] = 1;
      if (sh.act[s] == 2) cn[sh.tgt[s]] = sh.cn[sh.tgt[s]] + 1;
    }
  }
  __syncthreads();
  // state: the map is injective, so every (k, column) has at most one writer
  for (int s = 0; s < S; ++s) {
    const int act = sh.act[s];
    if (act == 0) continue;
    double* dst = csum + (long)sh.tgt[s] * D;
    const float* row = e + (long)s * D;
    if (act == 1)
      for (int k = tid; k < D; k += ON_T) dst[k] = (double)row[k];
    else
      for (int k = tid; k < D; k += ON_T) dst[k] = dst[k] + (double)row[k];
  }
}

// slots_host of an entry point that lists streams of a bank: distinct and inside [0, N) (NULL: the caller vouches)
inline int check_slots(const char* who, const int32_t* slots_host, int M, int N) {
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

// the frames of one emission are consistent: nothing the overlap-add or the emission touches leaves the ring of R
// frames or the E rows of the output (the same conditions on the host and on the device)
__host__ __device__ __forceinline__ bool online_frames_valid(long long g0, long long ga, long long gb, int F, int R,
                                                             long long E) {
  return ga >= 0 && ga <= gb && gb - ga <= E && (g0 < 0 || (g0 <= LLONG_MAX - F && g0 + F - ga <= R));
}

// Overlap-add, emission and ring clearing for one stream whose frames are valid: seg (F, S) of the chunk (not read
// when g0 < 0), map (S) or nullptr for "every entry -1", sum (R, K) and cnt (R) updated in place, o (E, K) written
// whole.  A frame R or more behind emit_from has no ring row of its own left: no chunk covered it, it gives 0.  The
// caller puts a __syncthreads() behind it before anything touches the ring again.
__device__ __forceinline__ void online_emit_one(const uint8_t* seg, int F, int S, const int* map, long long g0,
                                                long long ga, long long gb, int R, int K, int E, int* sum, int* cnt,
                                                uint8_t* o) {
  const int tid = threadIdx.x;
  int mp[ON_S];
  for (int s = 0; s < ON_S; ++s) {
    const int k = (s < S && map != nullptr) ? map[s] : -1;
    mp[s] = (k >= 0 && k < K) ? k : -1;
  }
  // overlap-add: a thread owns a frame, F <= R frames fall on distinct ring rows
  for (int f = tid; f < F && g0 >= 0; f += ON_T) {   // (g0 < 0: a flush, no chunk to add)
    const long long g = g0 + f;
    if (g < ga) continue;
    const int r = (int)(g % R);
    cnt[r] = cnt[r] + 1;
    const uint8_t* row = seg + (long)f * S;
    for (int s = 0; s < S; ++s)
      if (mp[s] >= 0 && row[s]) sum[(long)r * K + mp[s]] = sum[(long)r * K + mp[s]] + 1;
  }
  __syncthreads();
  for (int i = tid; i < E * K; i += ON_T) {
    const int k = i % K;
    const long long g = ga + i / K;
    uint8_t v = 0;
    if (g < gb && g - ga < R) {
      const int r = (int)(g % R);
      v = (uint8_t)(2 * sum[(long)r * K + k] > cnt[r]);
    }
    o[i] = v;
  }
  __syncthreads();
  const int n = gb - ga < R ? (int)(gb - ga) : R;
  for (int i = tid; i < n * (K + 1); i += ON_T) {
    const int r = (int)((ga + i / (K + 1)) % R), k = i % (K + 1);
    if (k < K)
      sum[(long)r * K + k] = 0;
    else
      cnt[r] = 0;
  }
}

}  // namespace pa
