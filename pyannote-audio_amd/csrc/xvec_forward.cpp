// pa_xvec_forward: XVectorSincNet (models/embedding/xvector.py:205-349) sequenced on one stream:
//   SincNet front end (forward_common.h: row stats, sinc FIR + pool, conv5 + pool x2, last InstanceNorm +
//   leaky_relu written as rows [(tile, t, b16)][64])
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
#include "forward_common.h"

namespace {

constexpr int SLACK_ROWS = 128;   // >= 16 * (k - 1) * d of every layer (96)

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

// T input frames -> Tp valid frames after the stack; the input rows, the two ping-pong activations (each with
// SLACK_ROWS rows past the last tile) and the pooled statistics of S masks per chunk
struct TdnnPlan {
  int T, Tp, S, ldstats;
  long M;
  size_t x0, a0, a1, stats;
};
void tdnn_plan(const TdnnTail& w, int B, int T, int S, pa::Bump* ws, TdnnPlan* p) {
  p->T = p->Tp = T;
  p->S = S < 1 ? 1 : S;
  for (int l = 0; l < PA_XVEC_TDNN; ++l) p->Tp -= (w.kernel[l] - 1) * w.dilation[l];
  p->M = pa::tile_rows(B, T);
  int cmax = 64;
  for (int l = 0; l < PA_XVEC_TDNN; ++l) cmax = w.channels[l] > cmax ? w.channels[l] : cmax;
  p->ldstats = (2 * w.channels[PA_XVEC_TDNN - 1] + 31) & ~31;
  p->x0 = ws->take((size_t)(p->M + SLACK_ROWS) * 64);
  p->a0 = ws->take((size_t)(p->M + SLACK_ROWS) * cmax);
  p->a1 = ws->take((size_t)(p->M + SLACK_ROWS) * cmax);
  p->stats = ws->take((size_t)B * p->S * p->ldstats);
}

// x0 [(tile, t, b16)][64] (+ SLACK_ROWS zero rows) -> TDNN stack (a0 / a1) -> pooling (stats) -> Linear -> emb
int xvec_tail(const TdnnTail& w, const TdnnPlan& p, float* ws, int B, const float* masks, int num_masks,
              int mask_frames, const int32_t* nearest_idx, float* emb, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // TDNN stack
  const float* in = ws + p.x0;
  int cin = 64;
  float* buf[2] = {ws + p.a0, ws + p.a1};
  for (int l = 0; l < PA_XVEC_TDNN; ++l) {
    const int cout = w.channels[l], k = w.kernel[l], d = w.dilation[l];
    float* out = buf[l & 1];
    if (pa::fill_async(out + (size_t)p.M * cout, 0, sizeof(float) * SLACK_ROWS * cout, st) != hipSuccess) return 1;
    for (int j = 0; j < k; ++j) {
      // tap j: rows shifted by j * d time steps = 16 j d rows; W_j = tdnn_w[l] + j * cout * cin
      PA_RUN(pa_gemm_tn_ex(in + (size_t)16 * j * d * cin, cin, w.w[l] + (size_t)j * cout * cin, cin,
                           j == 0 ? w.b[l] : nullptr, j == 0 ? nullptr : out, out, cout, (int)p.M, cout, cin,
                           j == k - 1 ? 1 : 0, 0, stream));
    }
    in = out;
    cin = cout;
  }
  // statistics pooling over the Tp valid frames, for every mask of a chunk at once
  const int S = masks ? num_masks : 1;
  PA_RUN(pa_stats_pool_rows_any(in, B, p.T, p.Tp, cin, cin, masks, S, mask_frames, nearest_idx, ws + p.stats,
                                p.ldstats, w.bn_scale, w.bn_shift, stream));
  // embedding Linear(2 C -> dimension) (xvector.py:250, 348); K padded to a multiple of 32 with zeros
  return pa_gemm_tn_ex(ws + p.stats, p.ldstats, w.emb_w, p.ldstats, w.emb_b, nullptr, emb, w.dimension, B * S,
                       w.dimension, p.ldstats, 0, 0, stream);
}

// the zero rows past the last tile of x0 that the taps of the last frames read
int zero_x0_slack(const TdnnPlan& p, float* ws, void* stream) {
  return pa::fill_async(ws + p.x0 + (size_t)p.M * 64, 0, sizeof(float) * SLACK_ROWS * 64, (hipStream_t)stream) !=
                 hipSuccess ? 1 : 0;
}

struct XvecPlan {
  pa::SincNetPlan sinc;
  TdnnPlan tdnn;
  size_t total;
};

bool make_plan(const pa_xvec_weights* w, int B, int N, int S, XvecPlan* p) {
  pa::Bump ws;
  if (!pa::sincnet_plan(w->sinc_stride, B, N, &ws, &p->sinc)) return false;
  tdnn_plan(tail_of(w), B, p->sinc.T, S, &ws, &p->tdnn);
  p->total = ws.o;
  return p->tdnn.Tp >= 1;
}

// XVectorMFCC: MFCC frames (xvector.py:111-118), then the TDNN stack
struct MfccPlan {
  size_t mel, cmax, frontend, total;
  TdnnPlan tdnn;
};

int mfcc_frames(const pa_xvec_mfcc_weights* w, int N) {
  if (w->n_fft != 400 || w->hop_length < 1 || w->hop_length > w->n_fft) return 0;
  if (w->center) return N > w->n_fft / 2 ? 1 + N / w->hop_length : 0;   // torch's reflect pad needs pad < N
  return N >= w->n_fft ? 1 + (N - w->n_fft) / w->hop_length : 0;
}

// true with at least one MFCC frame (pa_mfcc_features); the embedding also needs tdnn.Tp >= 1
bool make_mfcc_plan(const pa_xvec_mfcc_weights* w, int B, int N, int S, MfccPlan* p) {
  const int T = mfcc_frames(w, N);
  if (T < 1) return false;
  pa::Bump ws;
  p->mel = ws.take((size_t)B * T * w->n_mels);
  p->cmax = ws.take((size_t)B);
  p->frontend = ws.o;
  tdnn_plan(tail_of(w), B, T, S, &ws, &p->tdnn);
  p->total = ws.o;
  return true;
}

int mfcc_frontend(const pa_xvec_mfcc_weights* w, const MfccPlan& p, const float* wav, int64_t wav_len,
                  int64_t chunk_stride, int B, int N, float* ws, float* out, int rows, void* stream) {
  return pa_mfcc_frontend(wav, wav_len, chunk_stride, B, N, p.tdnn.T, w->hop_length, w->center, w->log_mels, w->window,
                          w->fft_tw, w->mel_w, w->mel_lo, w->mel_hi, w->n_mels, w->dct, w->n_mfcc, ws + p.mel,
                          (unsigned int*)(ws + p.cmax), out, rows, stream);
}

}  // namespace

extern "C" {

int pa_xvec_num_frames(const pa_xvec_weights* w, int num_samples) {
  XvecPlan p;
  return make_plan(w, 1, num_samples, 1, &p) ? p.tdnn.Tp : 0;
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
  // the slack rows first: no launch of the front end writes them
  PA_RUN(zero_x0_slack(p.tdnn, ws, stream));
  PA_RUN(pa::sincnet_run(pa::sincnet_of(w), p.sinc, wav, wav_len, chunk_stride, num_chunks, num_samples, ws,
                         ws + p.tdnn.x0, stream));
  return xvec_tail(tail_of(w), p.tdnn, ws, num_chunks, masks, num_masks, mask_frames, nearest_idx, emb, stream);
}

int pa_xvec_mfcc_num_frames(const pa_xvec_mfcc_weights* w, int num_samples) {
  MfccPlan p;
  return make_mfcc_plan(w, 1, num_samples, 1, &p) && p.tdnn.Tp > 0 ? p.tdnn.Tp : 0;
}

size_t pa_xvec_mfcc_workspace_bytes(const pa_xvec_mfcc_weights* w, int num_chunks, int num_samples, int num_masks) {
  MfccPlan p;
  if (!make_mfcc_plan(w, num_chunks, num_samples, num_masks, &p) || p.tdnn.Tp < 1) return 0;
  return p.total * sizeof(float);
}

int pa_xvec_mfcc_forward(const pa_xvec_mfcc_weights* w, const float* wav, int64_t wav_len, int64_t chunk_stride,
                         int num_chunks, int num_samples, const float* masks, int num_masks, int mask_frames,
                         const int32_t* nearest_idx, float* emb, void* workspace, size_t workspace_bytes,
                         void* stream) {
  if (num_chunks <= 0) return 0;
  MfccPlan p;
  if (!make_mfcc_plan(w, num_chunks, num_samples, masks ? num_masks : 1, &p) || p.tdnn.Tp < 1) {
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
  PA_RUN(mfcc_frontend(w, p, wav, wav_len, chunk_stride, num_chunks, num_samples, ws, ws + p.tdnn.x0, 1, stream));
  PA_RUN(zero_x0_slack(p.tdnn, ws, stream));
  return xvec_tail(tail_of(w), p.tdnn, ws, num_chunks, masks, num_masks, mask_frames, nearest_idx, emb, stream);
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
  return mfcc_frontend(w, p, wav, wav_len, chunk_stride, num_chunks, num_samples, (float*)workspace, out, 0, stream);
}

}  // extern "C"
