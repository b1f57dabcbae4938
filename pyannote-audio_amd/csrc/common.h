// Common helpers for the gfx950 (MI355X / CDNA4) kernels of the speaker-diarization hot path.
// Everything here is written for wave64 + MFMA (f32-input forms) only; there is no other target.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// D(16x16) += A(16x4) * B(4x16);  lane l supplies A[l&15][l>>4], B[l>>4][l&15];
// D: lane l holds column l&15, rows 4*(l>>4)+r, r = 0..3.
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
// D(32x32) += A(32x2) * B(2x32);  lane l supplies A[l&31][l>>5], B[l>>5][l&31];
// D: lane l holds column l&31, rows (r&3) + 8*(r>>2) + 4*(l>>5), r = 0..15.
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// launchers shared between translation units of the library that are NOT part of the C ABI (include/pyannote_amd.h
// declares every exported symbol; tests/test_capi.py checks both directions)
#define PA_INTERNAL __attribute__((visibility("hidden")))
// csrc/mfcc.hip, csrc/emb_pool.hip -> csrc/xvec_forward.cpp
PA_INTERNAL int pa_mfcc_frontend(const float* wav, long wav_len, long chunk_stride, int B, int N, int T, int hop,
                                 int center, int log_mels, const float* window, const float* fft_tw,
                                 const float* mel_w, const int* mel_lo, const int* mel_hi, int nmel,
                                 const float* dct, int n_mfcc, float* mel_buf, unsigned int* chunk_max, float* out,
                                 int rows, void* stream);
PA_INTERNAL int pa_stats_pool_rows_any(const float* feat, int B, int T0, int Tp, int C, int ld, const float* masks,
                                       int S, int Fm, const int* nearest_idx, float* stats, int ld_stats,
                                       const float* aff_scale, const float* aff_shift, void* stream);
// csrc/emb_fbank.hip, csrc/emb_resnet.hip -> csrc/emb_forward.cpp: the fbank frames of a span of overlapping chunks,
// computed once, + the mean of every chunk; the stem that reads chunk b as frames[b * fps + t] - mean[b] (mean = NULL:
// nothing is subtracted; fps = T: pa_resnet_stem)
PA_INTERNAL int pa_fbank_shared(const float* wav, long wav_len, int fps, int B, int N, const float* window,
                                const float* tw256, const float* tw512, const float* mel_w, const int* mel_lo,
                                const int* mel_hi, int nmel, float* frames, float* mean, void* stream);
PA_INTERNAL int pa_resnet_stem_frames(const float* frames, int fps, const float* mean, int B, int T, int F,
                                      const float* w9, const float* shift, float* out, void* stream);
// csrc/cluster.hip -> csrc/linkage_fast.hip, csrc/linkage_chain.hip, csrc/verification.hip
// S (n x ld, symmetric, zero diagonal) from the condensed matrix `cond` in pa_pdist_f64's order
PA_INTERNAL void pa_square_from_condensed(const double* cond, int n, long ld, double* S, void* stream);
// nrm[i] = row_norm_f64 of row i of X (N, D) (cosine_f64.h)
PA_INTERNAL void pa_row_norms_f64(const double* X, int N, int D, double* nrm, void* stream);

#include "workspace.h"
#include "launch_state.h"
namespace pa {

// The square symmetric copy the linkage kernels merge on (csrc/cluster.hip): its leading dimension, a multiple of 8
// doubles, and whether n points may have one -- PA_LINKAGE_FAST_MAX_GB caps its bytes (default 96 GB: n = 110 k) and
// n <= 150 000 keeps an enormous cap from promising sizes nobody has run.  Both linkage paths ask here.
inline long square_ld(int n) { return ((long)n + 7) & ~7L; }
PA_INTERNAL bool square_fits(int n);

// csrc/linkage_fast.hip -> csrc/linkage.hip: the heap-free merge in front of the heap kernel, its part of the workspace
struct LfState {
  double *S, *mind0;          // (n, square_ld(n)) square symmetric matrix; (n) initial lower bounds
  int *nb0, *g_size, *g_cid;  // (n) each: initial neighbour candidates, sizes and ids of the multi-workgroup form
  unsigned long long* mail;   // tagged granules of the exchange
  int* status;                // the gate of the heap kernel: 0 = the dendrogram is complete
};
PA_INTERNAL bool lf_wanted(int n);
PA_INTERNAL void lf_layout(Carver& c, int n, LfState& s);
PA_INTERNAL int lf_launch(const double* cond, int n, double* Z, const LfState& s, long long* stats, hipStream_t st);

void set_error(const char* fmt, ...);

// every byte of [dst, dst + nbytes) <- value, by a kernel on `st` (csrc/fill.hip): the launchers' hipMemsetAsync.  A kernel
// node of a captured graph replays with the arguments it was captured with; a memset node did not.
hipError_t fill_async(void* dst, int value, size_t nbytes, hipStream_t st);

// tile queue of the persistent convolution kernels: protocol in tile_queue.h, counter pool in pa_core.cpp
int* tile_counters(const char* entry);   // a zeroed 16-int block of the current device; null: refused, message set
int xcd_ranges_wanted(bool by_default);   // tile order of those kernels (emb_winograd4.hip)
// Per-device launch state (launch_state.h) with this library's answers.  "Allow `kernel` (a constant: the grant is
// remembered per kernel and device, whichever sites ask) `bytes` of dynamic LDS on the current device"; refused: rc 3
int lds_refused(const char* entry, long answer, size_t bytes);   // the message names the entry, bytes and limit
#define PA_ALLOW_LDS(entry, kernel, bytes)                                                                        \
  do {                                                                                                            \
    const pa::LdsAnswer a__ = pa::allow_lds(pa::kernel_cell<(kernel)>(), (const void*)(kernel), (long)(bytes));   \
    if (a__ != pa::LDS_OK) return pa::lds_refused(entry, a__, bytes);                                             \
  } while (0)
// the one line of a persistent launcher (one function per kernel, so its static is per kernel): -> resident, counters
#define PA_PERSISTENT(entry, kernel, threads, lds, per_cu)                                                            \
  static pa::DeviceCell cell__;                                                                                       \
  const long resident = pa::resident_workgroups(cell__, (const void*)(kernel), threads, (long)(lds), per_cu);         \
  if (resident <= 0) return pa::lds_refused(entry, -resident, lds);                                                   \
  int* const counters = pa::tile_counters(entry);                                                                     \
  if (counters == nullptr) return 2
}  // namespace pa
#include "tile_queue.h"
namespace pa {

// HIP-event profiler scope (pa_core.cpp): brackets the launches issued while it is alive with two
// events on `stream`; `flops` / `bytes` are the ALGORITHMIC work of those launches.
struct ProfScope {
  ProfScope(const char* name, void* stream, double flops, double bytes);
  ~ProfScope();
  long idx_;
  void* stream_;
};

#define PA_CHECK_LAUNCH(name)                                              \
  do {                                                                     \
    hipError_t e__ = hipGetLastError();                                    \
    if (e__ != hipSuccess) {                                               \
      pa::set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
      return e__ == hipErrorOutOfMemory ? 2 : 1;                           \
    }                                                                      \
  } while (0)

#define PA_REQUIRE(cond, ...)        \
  do {                               \
    if (!(cond)) {                   \
      pa::set_error(__VA_ARGS__);    \
      return 3;                      \
    }                                \
  } while (0)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// a row scan's candidate (linkage.hip, linkage_chain.hip) and its lexicographic "first minimum": the smaller value wins,
// equal values -> the smaller index; i < 0 = empty; NaN never wins
struct MinPair {
  double d;
  int i;
};
__device__ __forceinline__ MinPair min_pair(MinPair a, MinPair b) {
  if (b.i >= 0 && (a.i < 0 || b.d < a.d || (b.d == a.d && b.i < a.i))) return b;
  return a;
}

// Block-wide sum for blocks of NW waves; `red` is an LDS array of >= NW floats.
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) s += red[i];
  return s;
}

__device__ __forceinline__ float leaky_relu(float x) { return x > 0.f ? x : 0.01f * x; }
// torch.nn.functional.gelu (approximate="none"): x * Phi(x) with the exact error function
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

}  // namespace pa
