// The launch sequences that more than one forward entry point contains (forward_common.h).
#include "forward_common.h"

#include <stdlib.h>

namespace pa {

bool sincnet_frames(int sinc_stride, int N, SincNetPlan* p) {
  p->L1 = (N - 251) / sinc_stride + 1;
  if (N < 251 || p->L1 < 3) return false;
  p->P1 = p->L1 / 3;
  if (p->P1 < 5) return false;
  p->P2 = (p->P1 - 4) / 3;
  if (p->P2 < 5) return false;
  p->T = (p->P2 - 4) / 3;
  return p->T >= 1;
}

bool sincnet_plan(int sinc_stride, int B, int N, Bump* ws, SincNetPlan* p) {
  if (!sincnet_frames(sinc_stride, N, p)) return false;
  p->wav_mean = ws->take(B);
  p->wav_rstd = ws->take(B);
  p->s1 = ws->take((size_t)B * 80 * p->P1);
  p->st1m = ws->take((size_t)B * 80);
  p->st1r = ws->take((size_t)B * 80);
  p->s2 = ws->take((size_t)B * 60 * p->P2);
  p->st2m = ws->take((size_t)B * 60);
  p->st2r = ws->take((size_t)B * 60);
  p->s3 = ws->take((size_t)B * 60 * p->T);
  p->st3m = ws->take((size_t)B * 60);
  p->st3r = ws->take((size_t)B * 60);
  p->span = p->span_pos = 0;
  p->span_s = p->tap_sums = 0;
  return true;
}

// see seg_frontend.hip (k_sinc_fix_pool).  Measured on MI355X (round 4, one audio-hour = 3 591 chunks): k_sinc_fir_pool
// 21.2 ms -> k_sinc_fir_span 2.6 ms + k_sinc_fix_pool 3.2 ms, pipeline step 914.9 -> 903.7 ms; parity tests
// tests/test_seg_frontend_gpu.py::test_shared_sinc_pair* (float64, DC offsets included) and
// tests/test_seg_gpu.py::test_shared_sinc_layer_matches_the_per_chunk_layer.
// Default; PA_SEG_SHARED_SINC=0 selects the per-chunk layer for an A/B.
void sincnet_plan_span(int sinc_stride, int B, int N, int64_t chunk_stride, Bump* ws, SincNetPlan* p) {
  const char* e = getenv("PA_SEG_SHARED_SINC");
  if ((e == nullptr || atoi(e) != 0) && sinc_stride == 10 && B >= 2 && chunk_stride > 0 && chunk_stride < N &&
      chunk_stride % 10 == 0 && (int64_t)(B - 1) * chunk_stride + N <= 0x7fffffffLL) {
    p->span = (long)(B - 1) * chunk_stride + N;
    p->span_pos = (p->span - 251) / 10 + 1;
    p->span_s = ws->take((size_t)80 * p->span_pos);
    p->tap_sums = ws->take(80);
  }
}

int sincnet_sinc_stage(const SincNetView& w, const SincNetPlan& p, const float* wav, int64_t wav_len,
                       int64_t chunk_stride, int B, int N, float* ws, void* stream) {
  PA_RUN(pa_row_stats(wav, chunk_stride, wav_len, B, N, 1e-5f, ws + p.wav_mean, ws + p.wav_rstd, stream));
  if (p.span_pos > 0) {
    // (chunk 0's statistics decide the constant the span is re-centred by: no further pass over the audio)
    PA_RUN(pa_sinc_fir_span_centred(wav, wav_len, p.span, ws + p.wav_mean, ws + p.wav_rstd, w.sinc_filt,
                                    ws + p.span_s, stream));
    PA_RUN(pa_sinc_fix_pool_centred(ws + p.span_s, p.span_pos, (int)(chunk_stride / 10), B, p.P1, wav, wav_len, N,
                                    ws + p.wav_mean, ws + p.wav_rstd, w.wav_gamma, w.wav_beta, w.sinc_filt,
                                    ws + p.tap_sums, ws + p.s1, stream));
  } else {
    PA_RUN(pa_sinc_fir_pool(wav, wav_len, chunk_stride, B, N, w.sinc_stride, ws + p.wav_mean, ws + p.wav_rstd,
                            w.wav_gamma, w.wav_beta, w.sinc_filt, ws + p.s1, stream));
  }
  return 0;
}

int sincnet_after_sinc(const SincNetView& w, const SincNetPlan& p, int B, float* ws, float* x0, void* stream) {
  PA_RUN(pa_row_stats(ws + p.s1, p.P1, (long)B * 80 * p.P1, B * 80, p.P1, 1e-5f, ws + p.st1m, ws + p.st1r, stream));
  PA_RUN(pa_conv5_pool(ws + p.s1, B, 80, p.P1, ws + p.st1m, ws + p.st1r, w.norm0, w.norm0 + 80, w.conv1_w, w.conv1_b,
                       ws + p.s2, stream));
  PA_RUN(pa_row_stats(ws + p.s2, p.P2, (long)B * 60 * p.P2, B * 60, p.P2, 1e-5f, ws + p.st2m, ws + p.st2r, stream));
  PA_RUN(pa_conv5_pool(ws + p.s2, B, 60, p.P2, ws + p.st2m, ws + p.st2r, w.norm1, w.norm1 + 60, w.conv2_w, w.conv2_b,
                       ws + p.s3, stream));
  PA_RUN(pa_row_stats(ws + p.s3, p.T, (long)B * 60 * p.T, B * 60, p.T, 1e-5f, ws + p.st3m, ws + p.st3r, stream));
  return pa_norm_transpose(ws + p.s3, B, p.T, ws + p.st3m, ws + p.st3r, w.norm2, w.norm2 + 60, x0, stream);
}

int sincnet_run(const SincNetView& w, const SincNetPlan& p, const float* wav, int64_t wav_len, int64_t chunk_stride,
                int B, int N, float* ws, float* x0, void* stream) {
  PA_RUN(sincnet_sinc_stage(w, p, wav, wav_len, chunk_stride, B, N, ws, stream));
  return sincnet_after_sinc(w, p, B, ws, x0, stream);
}

bool lstm_head_check(const LstmHeadView& w, const char* who) {
  if (w.lstm_hidden < 16 || w.lstm_hidden % 16 != 0 || w.lstm_hidden > 512 ||
      (!w.lstm_bidir && w.lstm_hidden % 32 != 0) || w.lstm_layers < 1 || w.lstm_layers > PA_MAX_LSTM_LAYERS ||
      w.num_linear > PA_MAX_LINEAR || (w.num_linear > 0 && (w.linear_hidden < 32 || w.linear_hidden % 32 != 0))) {
    set_error("%s: LSTM hidden size must be a multiple of 16 (32 when unidirectional) up to 512, "
              "Linear widths multiples of 32 (got %d, %d)", who, w.lstm_hidden, w.linear_hidden);
    return false;
  }
  return true;
}

void lstm_head_plan(const LstmHeadView& w, int B, int T, Bump* ws, LstmHeadPlan* p) {
  p->ntiles = num_tiles(B);
  p->M = tile_rows(B, T);
  const size_t nd = w.lstm_bidir ? 2 : 1, Hh = (size_t)w.lstm_hidden;
  const size_t lw = w.num_linear > 0 ? (size_t)w.linear_hidden : 0;
  p->xproj = ws->take((size_t)p->M * nd * 4 * Hh);
  p->h0 = ws->take((size_t)p->M * nd * Hh);
  p->h1 = ws->take((size_t)p->M * nd * Hh);
  p->l0 = ws->take((size_t)p->M * lw);
  p->l1 = ws->take((size_t)p->M * lw);
}

int lstm_head_run(const LstmHeadView& w, const LstmHeadPlan& p, const float* x0, int kin, int B, int T, float* ws,
                  float* logp, uint8_t* multilabel, void* stream) {
  const float* in = x0;
  float* hbuf[2] = {ws + p.h0, ws + p.h1};
  const int ndir = w.lstm_bidir ? 2 : 1, Hh = w.lstm_hidden;
  for (int l = 0; l < w.lstm_layers; ++l) {
    PA_RUN(pa_gemm_tn(in, kin, w.lstm_wih[l], kin, w.lstm_bias[l], ws + p.xproj, 0, (int)p.M, ndir * 4 * Hh, kin, 0, 1,
                      stream));
    PA_RUN(pa_lstm_rec_h(ws + p.xproj, w.lstm_whh[l], hbuf[l & 1], p.ntiles, ndir, T, Hh, stream));
    in = hbuf[l & 1];
    kin = ndir * Hh;
  }
  float* lbuf[2] = {ws + p.l0, ws + p.l1};
  for (int l = 0; l < w.num_linear; ++l) {
    PA_RUN(pa_gemm_tn(in, kin, w.lin_w[l], kin, w.lin_b[l], lbuf[l & 1], w.linear_hidden, (int)p.M, w.linear_hidden,
                      kin, 1, 0, stream));
    in = lbuf[l & 1];
    kin = w.linear_hidden;
  }
  return pa_classifier(in, kin, kin, p.ntiles, T, B, w.cls_w, w.cls_b, w.num_classes, w.powerset_map, w.num_speakers,
                       logp, multilabel, stream);
}

}  // namespace pa
