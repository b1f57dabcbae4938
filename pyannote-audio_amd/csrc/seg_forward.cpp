// pa_seg_forward: sequences the segmentation kernels on one stream out of a caller workspace.
// Replaces PyanNet.forward + hard Powerset conversion (PyanNet.py:211-240, powerset.py:115-140).
#include "forward_common.h"

namespace {

struct SegPlan {
  pa::SincNetPlan sinc;
  pa::LstmHeadPlan head;
  size_t x0, total;   // offsets in floats
};

bool make_plan(const pa_seg_weights* w, int B, int N, int64_t chunk_stride, SegPlan* p) {
  pa::Bump ws;
  if (!pa::sincnet_plan(w->sinc_stride, B, N, &ws, &p->sinc)) return false;
  p->x0 = ws.take((size_t)pa::tile_rows(B, p->sinc.T) * 64);
  pa::lstm_head_plan(pa::lstm_head_of(w), B, p->sinc.T, &ws, &p->head);
  pa::sincnet_plan_span(w->sinc_stride, B, N, chunk_stride, &ws, &p->sinc);
  p->total = ws.o;
  return true;
}

}  // namespace

extern "C" {

int pa_seg_num_frames(int num_samples, int sinc_stride) {
  pa::SincNetPlan p;
  return pa::sincnet_frames(sinc_stride, num_samples, &p) ? p.T : 0;
}

size_t pa_seg_workspace_bytes_strided(const pa_seg_weights* w, int num_chunks, int num_samples,
                                      int64_t chunk_stride) {
  SegPlan p;
  if (!make_plan(w, num_chunks, num_samples, chunk_stride, &p)) return 0;
  return p.total * sizeof(float);
}

size_t pa_seg_workspace_bytes(const pa_seg_weights* w, int num_chunks, int num_samples) {
  return pa_seg_workspace_bytes_strided(w, num_chunks, num_samples, num_samples);
}

int pa_seg_forward(const pa_seg_weights* w, const float* wav, int64_t wav_len, int64_t chunk_stride,
                   int num_chunks, int num_samples, float* logp, uint8_t* multilabel, void* workspace,
                   size_t workspace_bytes, void* stream) {
  if (num_chunks <= 0) return 0;
  SegPlan p;
  if (!make_plan(w, num_chunks, num_samples, chunk_stride, &p)) {
    pa::set_error("pa_seg_forward: chunk of %d samples is too short for SincNet", num_samples);
    return 3;
  }
  if (p.sinc.span_pos > 0 && workspace_bytes < p.total * sizeof(float)) {
    // a workspace sized without the stride (pa_seg_workspace_bytes): the per-chunk sinc layer
    make_plan(w, num_chunks, num_samples, num_samples, &p);
  }
  const pa::LstmHeadView head = pa::lstm_head_of(w);
  if (!pa::lstm_head_check(head, "pa_seg_forward")) return 3;
  if (workspace_bytes < p.total * sizeof(float)) {
    pa::set_error("pa_seg_forward: workspace too small (%zu < %zu bytes)", workspace_bytes,
                  p.total * sizeof(float));
    return 3;
  }
  float* ws = (float*)workspace;
  PA_RUN(pa::sincnet_run(pa::sincnet_of(w), p.sinc, wav, wav_len, chunk_stride, num_chunks, num_samples, ws,
                         ws + p.x0, stream));
  return pa::lstm_head_run(head, p.head, ws + p.x0, 64, num_chunks, p.sinc.T, ws, logp, multilabel, stream);
}

}  // extern "C"
