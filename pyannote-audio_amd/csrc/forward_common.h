// Host-side pieces that the forward entry points share (seg_forward.cpp, sser_forward.cpp, xvec_forward.cpp,
// emb_forward.cpp): the workspace allocator, the run-and-return macro and the two launch sequences that more than one
// model contains -- the SincNet front end and the LSTM stack + feed-forward head + classifier.  Nothing here is part
// of the C ABI; common.h brings PA_INTERNAL, pa::set_error and the prototypes of the hidden launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pyannote_amd.h"
#include "common.h"

// issue a launcher; leave the entry point with its code if it fails
#define PA_RUN(call)                \
  do {                              \
    const int rc__ = (call);        \
    if (rc__ != 0) return rc__;     \
  } while (0)

namespace pa {

// workspace offsets in floats: every block starts on a 64-float boundary
struct Bump {
  size_t o = 0;
  static size_t align(size_t n) { return (n + 63) & ~(size_t)63; }
  size_t take(size_t n) {
    const size_t r = o;
    o += align(n);
    return r;
  }
};

// rows of an activation matrix in the (tile, t, b16) order: 16 chunks per tile, T frames
inline int num_tiles(int B) { return (B + 15) / 16; }
inline long tile_rows(int B, int T) { return (long)num_tiles(B) * T * 16; }

// ---- SincNet front end (models/blocks/sincnet.py:163-184): pa_seg_forward, pa_xvec_forward
struct SincNetView {   // the fields of pa_seg_weights / pa_xvec_weights that carry the same names
  int sinc_stride;
  float wav_gamma, wav_beta;
  const float *sinc_filt, *norm0, *conv1_w, *conv1_b, *norm1, *conv2_w, *conv2_b, *norm2;
};
template <class W>
SincNetView sincnet_of(const W* w) {
  return {w->sinc_stride, w->wav_gamma, w->wav_beta, w->sinc_filt, w->norm0, w->conv1_w,
          w->conv1_b,     w->norm1,     w->conv2_w,  w->conv2_b,   w->norm2};
}

struct SincNetPlan {
  int L1, P1, P2, T;   // frames after the sinc layer, after each of the three pools
  size_t wav_mean, wav_rstd, s1, st1m, st1r, s2, st2m, st2r, s3, st3m, st3r;
  // optional: the sinc layer once per span of overlapping chunks (sincnet_plan_span); span_pos = 0 without it
  long span, span_pos;
  size_t span_s, tap_sums;
};
// frame counts only; false when `N` samples leave no frame
PA_INTERNAL bool sincnet_frames(int sinc_stride, int N, SincNetPlan* p);
// frame counts + the eleven buffers of the per-chunk sequence
PA_INTERNAL bool sincnet_plan(int sinc_stride, int B, int N, Bump* ws, SincNetPlan* p);
// the shared sinc layer, where the chunks overlap by a multiple of the sinc stride (see forward_common.cpp): the raw
// filter outputs of the whole span + the tap sums.  The segmentation model's only.
PA_INTERNAL void sincnet_plan_span(int sinc_stride, int B, int N, int64_t chunk_stride, Bump* ws, SincNetPlan* p);
// The two halves of sincnet_run, for a caller that joins the chunks of several waveforms (pa_seg_forward_files):
// the waveform statistics + the sinc layer of the B chunks of ONE waveform -> p.wav_mean, p.wav_rstd, p.s1 (the
// only stage whose values depend on which chunks share a launch: the span is re-centred by chunk 0) ...
PA_INTERNAL int sincnet_sinc_stage(const SincNetView& w, const SincNetPlan& p, const float* wav, int64_t wav_len,
                                   int64_t chunk_stride, int B, int N, float* ws, void* stream);
// ... and everything behind p.s1, chunk by chunk, for all B chunks of the plan
PA_INTERNAL int sincnet_after_sinc(const SincNetView& w, const SincNetPlan& p, int B, float* ws, float* x0,
                                   void* stream);
// x0: rows [(tile, t, b16)][64] of ceil(B / 16) tiles
PA_INTERNAL int sincnet_run(const SincNetView& w, const SincNetPlan& p, const float* wav, int64_t wav_len,
                            int64_t chunk_stride, int B, int N, float* ws, float* x0, void* stream);

// ---- LSTM stack, feed-forward head and classifier (PyanNet.py:226-240, SSeRiouSS.py:315-328):
//      pa_seg_forward, pa_sser_forward
struct LstmHeadView {   // the fields of pa_seg_weights / pa_sser_weights that carry the same names
  int lstm_layers, lstm_hidden, lstm_bidir, num_linear, linear_hidden, num_classes, num_speakers;
  const float* const* lstm_wih;
  const float* const* lstm_bias;
  const float* const* lstm_whh;
  const float* const* lin_w;
  const float* const* lin_b;
  const float *cls_w, *cls_b;
  const uint8_t* powerset_map;
};
template <class W>
LstmHeadView lstm_head_of(const W* w) {
  return {w->lstm_layers, w->lstm_hidden, w->lstm_bidir, w->num_linear, w->linear_hidden, w->num_classes,
          w->num_speakers, w->lstm_wih,   w->lstm_bias,  w->lstm_whh,   w->lin_w,         w->lin_b,
          w->cls_w,        w->cls_b,      w->powerset_map};
}

struct LstmHeadPlan {
  int ntiles;
  long M;   // tile_rows(B, T)
  // gate pre-activations (ndir * 4H columns), two layer outputs (ndir * H), two head activations
  size_t xproj, h0, h1, l0, l1;
};
// the sizes the kernels take; otherwise the error of entry point `who` is set and false returned
PA_INTERNAL bool lstm_head_check(const LstmHeadView& w, const char* who);
PA_INTERNAL void lstm_head_plan(const LstmHeadView& w, int B, int T, Bump* ws, LstmHeadPlan* p);
// x0: M rows of `kin` floats in the (tile, t, b16) order
PA_INTERNAL int lstm_head_run(const LstmHeadView& w, const LstmHeadPlan& p, const float* x0, int kin, int B, int T,
                              float* ws, float* logp, uint8_t* multilabel, void* stream);

}  // namespace pa
