// pa_xvec_forward: XVectorSincNet (models/embedding/xvector.py:205-349) sequenced on one stream:
//   SincNet front end (the segmentation model's kernels: row stats, sinc FIR + pool, conv5 + pool x2,
//   last InstanceNorm + leaky_relu written as rows [(tile, t, b16)][64])
//   -> 5 TDNN layers = Conv1d(k, dilation d) + LeakyReLU + BatchNorm1d (xvector.py:232-247).  In the
//      (tile, t, b16) row order one time step is 16 rows, so tap j of a dilated convolution is the SAME
//      activation matrix shifted by 16 j d rows: a layer is k chained GEMMs C += A(shift j) W_j^T on
//      pa_gemm_tn_ex (bias with the first, LeakyReLU with the last); rows whose taps run past the end of
//      their chunk hold garbage and are never read (valid frames shrink 589 -> 585 -> 581 -> 575).
//      Each BatchNorm (eval: an affine map) is folded on the host into the NEXT layer's weights / bias; the
//      last one is applied on load inside the pooling kernel (an all-zero mask must pool to 0, not to its shift).
//   -> weighted statistics pooling over the valid frames for all masks of a chunk (k_stats_pool_rows)
//   -> Linear(3000 -> dimension).
// pa_xvec_mfcc_forward: XVectorMFCC (xvector.py:42-202), the same layers after the torchaudio MFCC front end of
// csrc/mfcc.hip, which writes its coefficients straight into the rows [(tile, t, b16)][64] (xvec_tail below).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pyannote_amd.h"

#define PA_INTERNAL __attribute__((visibility("hidden")))
// csrc/mfcc.hip, csrc/emb_pool.hip
PA_INTERNAL int pa_mfcc_frontend(const float* wav, long wav_len, long chunk_stride, int B, int N, int T, int hop,
                                 int center, int log_mels, const float* window, const float* fft_tw,
                                 const float* mel_w, const int* mel_lo, const int* mel_hi, int nmel,
                                 const float* dct, int n_mfcc, float* mel_buf, unsigned int* chunk_max, float* out,
                                 int rows, void* stream);
PA_INTERNAL int pa_stats_pool_rows_any(const float* feat, int B, int T0, int Tp, int C, int ld, const float* masks,
                                       int S, int Fm, const int* nearest_idx, float* stats, int ld_stats,
                                       const float* aff_scale, const float* aff_shift, void* stream);

namespace pa {
void set_error(const char* fmt, ...);
}

namespace {

struct XvecPlan {
  int B, N, L1, P1, P2, T, ntiles, Tp, S, ldstats;
  long M;
  size_t wav_mean, wav_rstd, s1, st1m, st1r, s2, st2m, st2r, s3, st3m, st3r, x0, a0, a1, stats, total;
};
inline size_t align64(size_t n) { return (n + 63) & ~(size_t)63; }
constexpr int SLACK_ROWS = 128;   // >= 16 * (k - 1) * d of every layer (96)

bool make_plan(const pa_xvec_weights* w, int B, int N, int S, XvecPlan* p) {
  p->B = B;
  p->N = N;
  p->S = S < 1 ? 1 : S;
  p->L1 = (N - 251) / w->sinc_stride + 1;
  if (N < 251 || p->L1 < 3) return false;
  p->P1 = p->L1 / 3;
  if (p->P1 < 5) return false;
  p->P2 = (p->P1 - 4) / 3;
  if (p->P2 < 5) return false;
  p->T = (p->P2 - 4) / 3;
  p->Tp = p->T;
  for (int l = 0; l < PA_XVEC_TDNN; ++l) p->Tp -= (w->tdnn_kernel[l] - 1) * w->tdnn_dilation[l];
  if (p->Tp < 1) return false;
  p->ntiles = (B + 15) / 16;
  p->M = (long)p->ntiles * p->T * 16;
  int cmax = 64;
  for (int l = 0; l < PA_XVEC_TDNN; ++l) cmax = w->tdnn_channels[l] > cmax ? w->tdnn_channels[l] : cmax;
  p->ldstats = (2 * w->tdnn_channels[PA_XVEC_TDNN - 1] + 31) & ~31;
  size_t o = 0;
  auto take = [&](size_t n) {
    size_t r = o;
    o += align64(n);
    return r;
  };
  p->wav_mean = take(B);
  p->wav_rstd = take(B);
  p->s1 = take((size_t)B * 80 * p->P1);
  p->st1m = take((size_t)B * 80);
  p->st1r = take((size_t)B * 80);
  p->s2 = take((size_t)B * 60 * p->P2);
  p->st2m = take((size_t)B * 60);
  p->st2r = take((size_t)B * 60);
  p->s3 = take((size_t)B * 60 * p->T);
  p->st3m = take((size_t)B * 60);
  p->st3r = take((size_t)B * 60);
  p->x0 = take((size_t)(p->M + SLACK_ROWS) * 64);
  p->a0 = take((size_t)(p->M + SLACK_ROWS) * cmax);
  p->a1 = take((size_t)(p->M + SLACK_ROWS) * cmax);
  p->stats = take((size_t)B * p->S * p->ldstats);
  p->total = o;
  return true;
}


// the layers after the front end, shared by XVectorSincNet and XVectorMFCC (the fields of pa_xvec_weights and
// pa_xvec_mfcc_weights that carry the same names)
struct TdnnTail {
  int dimension;
  const int32_t* channels;
  const int32_t* kernel;
  const int32_t* dilation;
  const float* const* w;
  const float* const* b;
  const float *bn_scale, *bn_shift, *emb_w, *emb_b;
};
template <class W>
TdnnTail tail_of(const W* w) {
  return {w->dimension, w->tdnn_channels, w->tdnn_kernel, w->tdnn_dilation, w->tdnn_w, w->tdnn_b,
          w->bn_scale,  w->bn_shift,      w->emb_w,       w->emb_b};
}

// x0 [(tile, t, b16)][64] (+ SLACK_ROWS zero rows) -> TDNN stack (a0 / a1) -> pooling (stats) -> Linear -> emb
int xvec_tail(const TdnnTail& w, const float* x0, float* a0, float* a1, float* stats, int B, int T, int Tp, long M,
              int ldstats, const float* masks, int num_masks, int mask_frames, const int32_t* nearest_idx, float* emb,
              void* stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc;
#define RUN(call)           \
  do {                      \
    rc = (call);            \
    if (rc != 0) return rc; \
  } while (0)
  // TDNN stack
  const float* in = x0;
  int cin = 64;
  float* buf[2] = {a0, a1};
  for (int l = 0; l < PA_XVEC_TDNN; ++l) {
    const int cout = w.channels[l], k = w.kernel[l], d = w.dilation[l];
    float* out = buf[l & 1];
    if (hipMemsetAsync(out + (size_t)M * cout, 0, sizeof(float) * SLACK_ROWS * cout, st) != hipSuccess) return 1;
    for (int j = 0; j < k; ++j) {
      // tap j: rows shifted by j * d time steps = 16 j d rows; W_j = tdnn_w[l] + j * cout * cin
      RUN(pa_gemm_tn_ex(in + (size_t)16 * j * d * cin, cin, w.w[l] + (size_t)j * cout * cin, cin,
                        j == 0 ? w.b[l] : nullptr, j == 0 ? nullptr : out, out, cout, (int)M, cout, cin,
                        j == k - 1 ? 1 : 0, 0, stream));
    }
    in = out;
    cin = cout;
  }
  // statistics pooling over the Tp valid frames, for every mask of a chunk at once
  const int S = masks ? num_masks : 1;
  RUN(pa_stats_pool_rows_any(in, B, T, Tp, cin, cin, masks, S, mask_frames, nearest_idx, stats, ldstats, w.bn_scale,
                             w.bn_shift, stream));
  // embedding Linear(2 C -> dimension) (xvector.py:250, 348); K padded to a multiple of 32 with zeros
  RUN(pa_gemm_tn_ex(stats, ldstats, w.emb_w, ldstats, w.emb_b, nullptr, emb, w.dimension, B * S, w.dimension, ldstats,
                    0, 0, stream));
#undef RUN
  return 0;
}

// XVectorMFCC: MFCC frames (xvector.py:111-118), then the TDNN stack
struct MfccPlan {
  int B, N, T, Tp, ntiles, S, ldstats;
  long M;
  size_t mel, cmax, x0, a0, a1, stats, frontend, total;
};

int mfcc_frames(const pa_xvec_mfcc_weights* w, int N) {
  if (w->n_fft != 400 || w->hop_length < 1 || w->hop_length > w->n_fft) return 0;
  if (w->center) return N > w->n_fft / 2 ? 1 + N / w->hop_length : 0;   // torch's reflect pad needs pad < N
  return N >= w->n_fft ? 1 + (N - w->n_fft) / w->hop_length : 0;
}

bool make_mfcc_plan(const pa_xvec_mfcc_weights* w, int B, int N, int S, MfccPlan* p) {
  p->B = B;
  p->N = N;
  p->S = S < 1 ? 1 : S;
  p->T = mfcc_frames(w, N);
  if (p->T < 1) return false;
  p->Tp = p->T;
  for (int l = 0; l < PA_XVEC_TDNN; ++l) p->Tp -= (w->tdnn_kernel[l] - 1) * w->tdnn_dilation[l];
  p->ntiles = (B + 15) / 16;
  p->M = (long)p->ntiles * p->T * 16;
  int cmax = 64;
  for (int l = 0; l < PA_XVEC_TDNN; ++l) cmax = w->tdnn_channels[l] > cmax ? w->tdnn_channels[l] : cmax;
  p->ldstats = (2 * w->tdnn_channels[PA_XVEC_TDNN - 1] + 31) & ~31;
  size_t o = 0;
  auto take = [&](size_t n) {
    size_t r = o;
    o += align64(n);
    return r;
  };
  p->mel = take((size_t)B * p->T * w->n_mels);
  p->cmax = take((size_t)B);
  p->frontend = o;
  p->x0 = take((size_t)(p->M + SLACK_ROWS) * 64);
  p->a0 = take((size_t)(p->M + SLACK_ROWS) * cmax);
  p->a1 = take((size_t)(p->M + SLACK_ROWS) * cmax);
  p->stats = take((size_t)B * p->S * p->ldstats);
  p->total = o;
  return true;
}

}  // namespace

extern "C" {

int pa_xvec_num_frames(const pa_xvec_weights* w, int num_samples) {
  XvecPlan p;
  return make_plan(w, 1, num_samples, 1, &p) ? p.Tp : 0;
}

size_t pa_xvec_workspace_bytes(const pa_xvec_weights* w, int num_chunks, int num_samples, int num_masks) {
  XvecPlan p;
  if (!make_plan(w, num_chunks, num_samples, num_masks, &p)) return 0;
  return p.total * sizeof(float);
}

int pa_xvec_forward(const pa_xvec_weights* w, const float* wav, int64_t wav_len, int64_t chunk_stride,
                    int num_chunks, int num_samples, const float* masks, int num_masks, int mask_frames,
                    const int32_t* nearest_idx, float* emb, void* workspace, size_t workspace_bytes,
                    void* stream) {
  if (num_chunks <= 0) return 0;
  XvecPlan p;
  if (!make_plan(w, num_chunks, num_samples, masks ? num_masks : 1, &p)) {
    pa::set_error("pa_xvec_forward: %d samples leave no frame after SincNet + the TDNN stack", num_samples);
    return 3;
  }
  if (workspace_bytes < p.total * sizeof(float)) {
    pa::set_error("pa_xvec_forward: workspace too small (%zu < %zu bytes)", workspace_bytes,
                  p.total * sizeof(float));
    return 3;
  }
  float* ws = (float*)workspace;
  const int B = p.B;
  hipStream_t st = (hipStream_t)stream;
  int rc;
#define RUN(call)           \
  do {                      \
    rc = (call);            \
    if (rc != 0) return rc; \
  } while (0)

  // SincNet (models/blocks/sincnet.py:163-184), as in pa_seg_forward
  RUN(pa_row_stats(wav, chunk_stride, wav_len, B, p.N, 1e-5f, ws + p.wav_mean, ws + p.wav_rstd, stream));
  RUN(pa_sinc_fir_pool(wav, wav_len, chunk_stride, B, p.N, w->sinc_stride, ws + p.wav_mean, ws + p.wav_rstd,
                       w->wav_gamma, w->wav_beta, w->sinc_filt, ws + p.s1, stream));
  RUN(pa_row_stats(ws + p.s1, p.P1, (long)B * 80 * p.P1, B * 80, p.P1, 1e-5f, ws + p.st1m, ws + p.st1r, stream));
  RUN(pa_conv5_pool(ws + p.s1, B, 80, p.P1, ws + p.st1m, ws + p.st1r, w->norm0, w->norm0 + 80, w->conv1_w,
                    w->conv1_b, ws + p.s2, stream));
  RUN(pa_row_stats(ws + p.s2, p.P2, (long)B * 60 * p.P2, B * 60, p.P2, 1e-5f, ws + p.st2m, ws + p.st2r, stream));
  RUN(pa_conv5_pool(ws + p.s2, B, 60, p.P2, ws + p.st2m, ws + p.st2r, w->norm1, w->norm1 + 60, w->conv2_w,
                    w->conv2_b, ws + p.s3, stream));
  RUN(pa_row_stats(ws + p.s3, p.T, (long)B * 60 * p.T, B * 60, p.T, 1e-5f, ws + p.st3m, ws + p.st3r, stream));
  if (hipMemsetAsync(ws + p.x0 + (size_t)p.M * 64, 0, sizeof(float) * SLACK_ROWS * 64, st) != hipSuccess) return 1;
  RUN(pa_norm_transpose(ws + p.s3, B, p.T, ws + p.st3m, ws + p.st3r, w->norm2, w->norm2 + 60, ws + p.x0, stream));

  return xvec_tail(tail_of(w), ws + p.x0, ws + p.a0, ws + p.a1, ws + p.stats, B, p.T, p.Tp, p.M, p.ldstats,
                   masks, num_masks, mask_frames, nearest_idx, emb, stream);
#undef RUN
}

int pa_xvec_mfcc_num_frames(const pa_xvec_mfcc_weights* w, int num_samples) {
  MfccPlan p;
  return make_mfcc_plan(w, 1, num_samples, 1, &p) && p.Tp > 0 ? p.Tp : 0;
}

size_t pa_xvec_mfcc_workspace_bytes(const pa_xvec_mfcc_weights* w, int num_chunks, int num_samples, int num_masks) {
  MfccPlan p;
  if (!make_mfcc_plan(w, num_chunks, num_samples, num_masks, &p) || p.Tp < 1) return 0;
  return p.total * sizeof(float);
}

int pa_xvec_mfcc_forward(const pa_xvec_mfcc_weights* w, const float* wav, int64_t wav_len, int64_t chunk_stride,
                         int num_chunks, int num_samples, const float* masks, int num_masks, int mask_frames,
                         const int32_t* nearest_idx, float* emb, void* workspace, size_t workspace_bytes,
                         void* stream) {
  if (num_chunks <= 0) return 0;
  MfccPlan p;
  if (!make_mfcc_plan(w, num_chunks, num_samples, masks ? num_masks : 1, &p) || p.Tp < 1) {
    pa::set_error("pa_xvec_mfcc_forward: %d samples leave no frame after the MFCC front end + the TDNN stack",
                  num_samples);
    return 3;
  }
  if (workspace_bytes < p.total * sizeof(float)) {
    pa::set_error("pa_xvec_mfcc_forward: workspace too small (%zu < %zu bytes)", workspace_bytes,
                  p.total * sizeof(float));
    return 3;
  }
  float* ws = (float*)workspace;
  int rc = pa_mfcc_frontend(wav, wav_len, chunk_stride, p.B, p.N, p.T, w->hop_length, w->center, w->log_mels,
                            w->window, w->fft_tw, w->mel_w, w->mel_lo, w->mel_hi, w->n_mels, w->dct, w->n_mfcc,
                            ws + p.mel, (unsigned int*)(ws + p.cmax), ws + p.x0, 1, stream);
  if (rc != 0) return rc;
  if (hipMemsetAsync(ws + p.x0 + (size_t)p.M * 64, 0, sizeof(float) * SLACK_ROWS * 64, (hipStream_t)stream) !=
      hipSuccess)
    return 1;
  return xvec_tail(tail_of(w), ws + p.x0, ws + p.a0, ws + p.a1, ws + p.stats, p.B, p.T, p.Tp, p.M, p.ldstats, masks,
                   num_masks, mask_frames, nearest_idx, emb, stream);
}

int pa_mfcc_features(const pa_xvec_mfcc_weights* w, const float* wav, int64_t wav_len, int64_t chunk_stride,
                     int num_chunks, int num_samples, float* out, void* workspace, size_t workspace_bytes,
                     void* stream) {
  if (num_chunks <= 0) return 0;
  MfccPlan p;
  if (!make_mfcc_plan(w, num_chunks, num_samples, 1, &p)) {
    pa::set_error("pa_mfcc_features: %d samples leave no MFCC frame", num_samples);
    return 3;
  }
  if (workspace_bytes < p.frontend * sizeof(float)) {
    pa::set_error("pa_mfcc_features: workspace too small (%zu < %zu bytes)", workspace_bytes,
                  p.frontend * sizeof(float));
    return 3;
  }
  float* ws = (float*)workspace;
  return pa_mfcc_frontend(wav, wav_len, chunk_stride, p.B, p.N, p.T, w->hop_length, w->center, w->log_mels, w->window,
                          w->fft_tw, w->mel_w, w->mel_lo, w->mel_hi, w->n_mels, w->dct, w->n_mfcc, ws + p.mel,
                          (unsigned int*)(ws + p.cmax), out, 0, stream);
}

}  // extern "C"
