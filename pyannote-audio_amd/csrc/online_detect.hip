// Online (streaming) detection on gfx950: voice activity / multi-label regions of many concurrent streams while their
// audio arrives.  One launch carries the arithmetic of the offline detection path -- the overlap-add of
// aggregate_gather (frames.hip) and the region rule of regions.h -- across pushes: a float ring per stream, a
// hysteresis state per class and the one region per class that is not final yet (include/pyannote_amd_online.h has
// the rule; it is the normative statement).
//
// One workgroup per stream, no communication between workgroups, no atomics: every ring element has one writer (a
// thread owns one (frame, class)), and the per-class state has one (lane k of wave 0 walks class k).  The emitted
// values go through LDS: the walk of a class reads E floats that K lanes would otherwise fetch with a stride of K.
// Times are those of rg_time, so the file is compiled without contraction like every file that includes regions.h.
// hipcc-flags: -ffp-contract=off
#include "online_rule.h"
#include "regions.h"
#include "pyannote_amd_online.h"

namespace pa {

constexpr int OD_T = 256;                 // threads per workgroup
constexpr int OD_MAX_VALUES = 12288;      // E * K: 4 + 1 bytes of LDS each (values, states), 60 KB

__device__ __forceinline__ float detect_score(float v) { return v; }
__device__ __forceinline__ float detect_score(uint8_t v) { return v ? 1.f : 0.f; }   // a hard decision (chunk_score)

// the value of class k at one frame of a chunk, `p` its S columns: column k, or with `any` np.max over the columns
template <typename VT>
__device__ __forceinline__ float detect_value(const VT* __restrict__ p, int S, int any, int k) {
  if (!any) return detect_score(p[k]);
  float best = detect_score(p[0]);
  for (int s = 1; s < S; ++s) {
    const float y = detect_score(p[s]);
    if (y != y || best != best) best = __builtin_nanf("");   // np.max propagates NaN
    else best = y > best ? y : best;
  }
  return best;
}

// the state of one class of one stream while lane k walks the emitted frames, and where its final regions go
struct DetectClass {
  double open_start, pend_s, pend_e, min_on, min_off;
  int has_pend, n_merged, count, cap;
  double* regions;
  int* tracks;

  // the pending region is final: out it goes unless it is too short; its track is its index among the merged regions
  __device__ __forceinline__ void finalise() {
    if (!(min_on > 0.0 && rg_duration(pend_s, pend_e) < min_on) && count < cap) {
      regions[2 * count] = pend_s;
      regions[2 * count + 1] = pend_e;
      tracks[count] = min_off > 0.0 ? n_merged - 1 : 0;
      ++count;
    }
    has_pend = 0;
  }

  // an on-event at time t: a pending region a later one can no longer merge with is final
  __device__ __forceinline__ void opens(double t) {
    open_start = t;
    if (has_pend && !(min_off > 0.0 && rg_duration(pend_e, t) < min_off)) finalise();
  }

  // the raw region (open_start, e) closes
  __device__ __forceinline__ void closes(double e) {
    const double s = open_start;
    if (!(e - s > RG_PRECISION)) return;                      // an empty region does not exist
    if (has_pend && min_off > 0.0 && rg_duration(pend_e, s) < min_off) {
      pend_e = e;                                             // merged into the pending region
    } else {
      if (has_pend) finalise();
      pend_s = s;
      pend_e = e;
      has_pend = 1;
      ++n_merged;
    }
    if (!(min_off > 0.0)) finalise();                         // nothing ever merges: final at once
  }
};

template <typename VT>
__global__ __launch_bounds__(OD_T) void k_online_detect(
    const int* __restrict__ slots, int N, const VT* __restrict__ scores, int F, int S, int any,
    const double* __restrict__ window, const double* __restrict__ warm, float epsilon, float missing,
    const long long* __restrict__ start_frame, const long long* __restrict__ emit_from,
    const long long* __restrict__ emit_to, const long long* __restrict__ closing, RegionParams prm, int R, int E,
    int cap, float* acc, float* cnt, uint8_t* msk, uint8_t* on, double* open_start, double* pend, uint8_t* has_pend,
    int* n_merged, float* __restrict__ values, uint8_t* __restrict__ active, int* __restrict__ counts,
    double* __restrict__ regions, int* __restrict__ tracks) {
  extern __shared__ __attribute__((aligned(16))) char od_smem[];
  const int K = any ? 1 : S;
  const int EK = E * K;
  float* sh_val = (float*)od_smem;                                        // (E, K) emitted values
  uint8_t* sh_act = (uint8_t*)(od_smem + (((size_t)EK * 4 + 15) & ~(size_t)15));   // (E, K) states after each frame
  __shared__ int sh_count[RG_MAXK];

  const int m = blockIdx.x, tid = threadIdx.x;
  const int slot = slots[m];
  const long long g0 = start_frame[m], ga = emit_from[m], gb = emit_to[m];
  float* o_val = values + (long)m * EK;
  uint8_t* o_act = active + (long)m * EK;
  int* o_cnt = counts + (long)m * K;
  double* o_reg = regions + (long)m * K * cap * 2;
  int* o_trk = tracks + (long)m * K * cap;

  // whatever the tables say, nothing below may leave the stream's own rows: the same conditions as on the host
  if (!(slot >= 0 && slot < N && online_frames_valid(g0, ga, gb, F, R, E))) {
    for (int i = tid; i < EK; i += OD_T) {
      o_val[i] = __builtin_nanf("");
      o_act[i] = 0;
    }
    for (int i = tid; i < K * cap; i += OD_T) {
      o_reg[2 * i] = o_reg[2 * i + 1] = __builtin_nan("");
      o_trk[i] = -1;
    }
    if (tid < K) o_cnt[tid] = 0;
    return;
  }
  float* r_acc = acc + (long)slot * R * K;
  float* r_cnt = cnt + (long)slot * R * K;
  uint8_t* r_msk = msk + (long)slot * R * K;
  const int n = (int)(gb - ga);                                           // frames this call emits, <= E

  // 1. overlap-add: a thread owns one (frame, class); the F frames of a chunk fall on distinct ring rows (F <= R)
  if (g0 >= 0) {                                                          // (g0 < 0: a flush, no chunk to add)
    const VT* mine = scores + (long)m * F * S;
    for (int i = tid; i < F * K; i += OD_T) {
      const int f = i / K, k = i - f * K;
      const long long g = g0 + f;
      if (g < ga) continue;                                               // emitted by an earlier call
      const long r = (long)(g % R) * K + k;
      const float x = detect_value(mine + (long)f * S, S, any, k);
      const bool nan = x != x;
      const double w = nan ? 0.0 : 1.0;
      // ((score * mask) * hamming) * warm_up and ((mask * hamming) * warm_up): aggregate_gather's expressions
      r_acc[r] = (float)((double)r_acc[r] + (((double)(nan ? 0.f : x) * w) * window[f]) * warm[f]);
      r_cnt[r] = (float)((double)r_cnt[r] + (w * window[f]) * warm[f]);
      if (!nan) r_msk[r] = 1;
    }
  }
  __syncthreads();

  // 2. emission: the value of every due frame, to the output and to LDS; its ring row is free again
  for (int i = tid; i < EK; i += OD_T) {
    const int e = i / K, k = i - e * K;
    float v = __builtin_nanf("");
    if (e < n) {
      const long r = (long)((ga + e) % R) * K + k;
      v = r_acc[r] / fmaxf(r_cnt[r], epsilon);
      if (r_msk[r] == 0) v = missing;
      r_acc[r] = 0.f;
      r_cnt[r] = 0.f;
      r_msk[r] = 0;
    }
    o_val[i] = v;
    sh_val[i] = v;
  }
  __syncthreads();

  // 3 - 5. one lane per class walks the emitted values: hysteresis, raw regions, the pending region, the close
  if (tid < K) {
    const int k = tid;
    const long sk = (long)slot * K + k;
    const float onset = prm.onset[k], offset = prm.offset[k];
    DetectClass c;
    c.open_start = open_start[sk];
    c.pend_s = pend[2 * sk];
    c.pend_e = pend[2 * sk + 1];
    c.min_on = prm.min_on[k];
    c.min_off = prm.min_off[k];
    c.has_pend = has_pend[sk] != 0;
    c.n_merged = n_merged[sk];
    c.count = 0;
    c.cap = cap;
    c.regions = o_reg + (long)k * cap * 2;
    c.tracks = o_trk + (long)k * cap;
    bool state = on[sk] != 0;
    for (int e = 0; e < n; ++e) {
      const long long g = ga + e;
      const float v = sh_val[e * K + k];                      // NaN: both comparisons false, nothing changes
      const bool before = g == 0 ? false : state;             // nothing comes before frame 0
      const bool after = before ? !(v < offset) : (v > onset);
      if (!before && after) c.opens(rg_time((long)g, prm.start, prm.duration, prm.step));
      if (before && !after) c.closes(rg_time((long)g, prm.start, prm.duration, prm.step));
      state = after;
      sh_act[e * K + k] = (uint8_t)after;
    }
    if (closing[m] != 0) {                                    // the stream ends behind frame emit_to - 1
      if (state) c.closes(rg_time((long)(gb - 1), prm.start, prm.duration, prm.step));
      state = false;
      if (c.has_pend) c.finalise();
    }
    on[sk] = (uint8_t)state;
    open_start[sk] = c.open_start;
    pend[2 * sk] = c.pend_s;
    pend[2 * sk + 1] = c.pend_e;
    has_pend[sk] = (uint8_t)c.has_pend;
    n_merged[sk] = c.n_merged;
    sh_count[k] = c.count;
    o_cnt[k] = c.count;
  }
  __syncthreads();

  // the rest of every output: states of the emitted frames, zero rows behind them, NaN / -1 behind the region counts
  for (int i = tid; i < EK; i += OD_T) o_act[i] = i < n * K ? sh_act[i] : (uint8_t)0;
  for (int i = tid; i < K * cap; i += OD_T) {
    const int k = i / cap, j = i - k * cap;
    if (j >= sh_count[k]) {
      o_reg[2 * i] = o_reg[2 * i + 1] = __builtin_nan("");
      o_trk[i] = -1;
    }
  }
}

}  // namespace pa

extern "C" {

int pao_detect_limits(int* max_classes_host, int* max_emit_values_host) {
  if (max_classes_host != nullptr) *max_classes_host = pa::RG_MAXK;
  if (max_emit_values_host != nullptr) *max_emit_values_host = pa::OD_MAX_VALUES;
  return 0;
}

int pao_detect_step(const int32_t* slots, const int32_t* slots_host, int M, int N, const void* scores,
                    int scores_uint8, int F, int S, int any, const double* window, const double* warm, float epsilon,
                    float missing, const int64_t* start_frame, const int64_t* emit_from, const int64_t* emit_to,
                    const int64_t* closing, const int64_t* frames_host, double start, double duration, double step,
                    const float* onset_host, const float* offset_host, const double* min_duration_on_host,
                    const double* min_duration_off_host, int R, int E, int cap, float* acc, float* cnt, uint8_t* msk,
                    uint8_t* on, double* open_start, double* pend, uint8_t* has_pend, int32_t* n_merged, float* values,
                    uint8_t* active, int32_t* counts, double* regions, int32_t* tracks, void* stream) {
  PA_REQUIRE(S >= 1 && S <= pa::RG_MAXK, "pao_detect_step: %d score columns per frame, the kernel handles 1..%d", S,
             pa::RG_MAXK);
  PA_REQUIRE(any || !scores_uint8, "pao_detect_step: uint8 scores are the hard multilabel output, any = 1 only");
  const int K = any ? 1 : S;
  PA_REQUIRE(F >= 1 && E >= 1 && N >= 1 && M >= 0, "pao_detect_step: needs F >= 1, E >= 1, N >= 1, M >= 0");
  PA_REQUIRE((long)R >= (long)F + E, "pao_detect_step: a ring of %d frames is shorter than F + E = %d + %d", R, F, E);
  PA_REQUIRE((long)E * K <= pa::OD_MAX_VALUES, "pao_detect_step: %d frames of %d classes per emission, at most %d "
             "values fit the workgroup's LDS", E, K, pa::OD_MAX_VALUES);
  PA_REQUIRE((long)R * K <= INT_MAX, "pao_detect_step: ring too large");
  PA_REQUIRE(cap >= E / 2 + 2 && (long)K * cap <= INT_MAX / 2, "pao_detect_step: room for %d regions per class, an "
             "emission of %d frames can finalise %d", cap, E, E / 2 + 2);
  PA_REQUIRE(onset_host && offset_host && min_duration_on_host && min_duration_off_host,
             "pao_detect_step: null parameter array");
  pa::RegionParams prm;
  for (int k = 0; k < pa::RG_MAXK; ++k) {
    const bool used = k < K;
    prm.onset[k] = used ? onset_host[k] : 0.f;
    prm.offset[k] = used ? offset_host[k] : 0.f;
    prm.min_on[k] = used ? min_duration_on_host[k] : 0.0;
    prm.min_off[k] = used ? min_duration_off_host[k] : 0.0;
    PA_REQUIRE(prm.onset[k] == prm.onset[k] && prm.offset[k] == prm.offset[k] && prm.min_on[k] == prm.min_on[k] &&
                   prm.min_off[k] == prm.min_off[k],
               "pao_detect_step: a threshold or a duration of class %d is NaN", k);
  }
  PA_REQUIRE(start == start && duration == duration && step == step, "pao_detect_step: the frame grid has a NaN");
  prm.start = start;
  prm.duration = duration;
  prm.step = step;
  if (int rc = pa::check_slots("pao_detect_step", slots_host, M, N)) return rc;
  if (frames_host != nullptr)
    for (int i = 0; i < M; ++i) {
      const int64_t g0 = frames_host[i], ga = frames_host[M + i], gb = frames_host[2 * (long)M + i];
      const int64_t last = frames_host[3 * (long)M + i];
      PA_REQUIRE(pa::online_frames_valid(g0, ga, gb, F, R, E) && (last == 0 || last == 1),
                 "pao_detect_step: inconsistent frames of entry %d: chunk at %lld (F = %d), emission [%lld, %lld), "
                 "closing %lld, E = %d, R = %d", i, (long long)g0, F, (long long)ga, (long long)gb, (long long)last,
                 E, R);
    }
  if (M == 0) return 0;
  const size_t lds = (((size_t)E * K * 4 + 15) & ~(size_t)15) + (size_t)E * K;
  pa::ProfScope prof("k_online_detect", stream, 6.0 * M * (double)F * K,
                     (double)M * ((scores_uint8 ? 1.0 : 4.0) * F * S + 18.0 * F * K + 14.0 * E * K + 20.0 * K * cap));
#define PA_DETECT_LAUNCH(VT)                                                                                        \
  hipLaunchKernelGGL(pa::k_online_detect<VT>, dim3(M), dim3(pa::OD_T), lds, (hipStream_t)stream, slots, N,          \
                     (const VT*)scores, F, S, any, window, warm, epsilon, missing, (const long long*)start_frame,   \
                     (const long long*)emit_from, (const long long*)emit_to, (const long long*)closing, prm, R, E,  \
                     cap, acc, cnt, msk, on, open_start, pend, has_pend, n_merged, values, active, counts, regions, \
                     tracks)
  if (scores_uint8) PA_DETECT_LAUNCH(uint8_t);
  else PA_DETECT_LAUNCH(float);
#undef PA_DETECT_LAUNCH
  PA_CHECK_LAUNCH("pao_detect_step");
  return 0;
}

}  // extern "C"
