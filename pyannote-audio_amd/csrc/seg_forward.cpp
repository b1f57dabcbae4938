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

// pa_seg_forward_files: the chunks of several waveforms as ONE chunk axis.  The buffers of `sinc` / `head` hold all
// chunks; the span scratch holds the longest file's span and is reused file after file on the stream.
struct FilesPlan {
  SegPlan seg;
  long chunks;        // all files'
  size_t span_base;   // where every file's span scratch begins
};

// the span scratch of a file of B chunks, taken at `base`: what a single-file plan would add behind its other buffers
size_t plan_file_span(const pa_seg_weights* w, int B, int N, int64_t chunk_stride, size_t base, pa::SincNetPlan* p) {
  pa::Bump at;
  at.o = base;
  p->span = p->span_pos = 0;
  p->span_s = p->tap_sums = 0;
  pa::sincnet_plan_span(w->sinc_stride, B, N, chunk_stride, &at, p);
  return at.o;
}

// 0: planned, 1: a negative chunk count or more than 65 535 chunks, 2: chunks too short for SincNet
int make_files_plan(const pa_seg_weights* w, int num_files, const int* chunks_per_file, int N, int64_t chunk_stride,
                    FilesPlan* p) {
  p->chunks = 0;
  for (int f = 0; f < num_files; ++f) {
    if (chunks_per_file[f] < 0) return 1;
    p->chunks += chunks_per_file[f];
  }
  if (num_files < 0 || p->chunks > 65535) return 1;   // (the chunk axis is a grid's y dimension)
  pa::Bump ws;
  const int B = (int)p->chunks;
  if (!pa::sincnet_plan(w->sinc_stride, B, N, &ws, &p->seg.sinc)) return 2;
  p->seg.x0 = ws.take((size_t)pa::tile_rows(B, p->seg.sinc.T) * 64);
  pa::lstm_head_plan(pa::lstm_head_of(w), B, p->seg.sinc.T, &ws, &p->seg.head);
  p->span_base = p->seg.total = ws.o;
  for (int f = 0; f < num_files; ++f) {
    pa::SincNetPlan one = p->seg.sinc;
    const size_t end = plan_file_span(w, chunks_per_file[f], N, chunk_stride, p->span_base, &one);
    if (end > p->seg.total) p->seg.total = end;
  }
  return 0;
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

size_t pa_seg_files_workspace_bytes(const pa_seg_weights* w, int num_files, const int* chunks_per_file,
                                    int num_samples, int64_t chunk_stride) {
  FilesPlan p;
  if (make_files_plan(w, num_files, chunks_per_file, num_samples, chunk_stride, &p) != 0) return 0;
  return p.seg.total * sizeof(float);
}

int pa_seg_forward_files(const pa_seg_weights* w, const float* const* wavs, const int64_t* wav_lens,
                         const int* chunks_per_file, int num_files, int64_t chunk_stride, int num_samples,
                         float* logp, uint8_t* multilabel, void* workspace, size_t workspace_bytes, void* stream) {
  FilesPlan p;
  const int bad = make_files_plan(w, num_files, chunks_per_file, num_samples, chunk_stride, &p);
  if (bad == 1) {
    pa::set_error("pa_seg_forward_files: a negative chunk count, or more than 65535 chunks in one launch group");
    return 3;
  }
  if (bad != 0) {
    pa::set_error("pa_seg_forward_files: chunk of %d samples is too short for SincNet", num_samples);
    return 3;
  }
  if (p.chunks == 0) return 0;
  const pa::LstmHeadView head = pa::lstm_head_of(w);
  if (!pa::lstm_head_check(head, "pa_seg_forward_files")) return 3;
  if (workspace_bytes < p.seg.total * sizeof(float)) {
    pa::set_error("pa_seg_forward_files: workspace too small (%zu < %zu bytes)", workspace_bytes,
                  p.seg.total * sizeof(float));
    return 3;
  }
  float* ws = (float*)workspace;
  const pa::SincNetView sinc = pa::sincnet_of(w);
  const int B = (int)p.chunks;
  // the sinc stage file by file, with the arguments pa_seg_forward passes for that file alone (the span path from two
  // chunks on, re-centred by the FILE's chunk 0), writing at the file's chunk offset ...
  long c0 = 0;
  for (int f = 0; f < num_files; ++f) {
    const int Bf = chunks_per_file[f];
    if (Bf == 0) continue;
    pa::SincNetPlan one = p.seg.sinc;
    one.wav_mean += c0;
    one.wav_rstd += c0;
    one.s1 += (size_t)c0 * 80 * one.P1;
    plan_file_span(w, Bf, num_samples, chunk_stride, p.span_base, &one);
    PA_RUN(pa::sincnet_sinc_stage(sinc, one, wavs[f], wav_lens[f], chunk_stride, Bf, num_samples, ws, stream));
    c0 += Bf;
  }
  // ... and everything behind it once over all chunks: none of it looks past its own chunk
  PA_RUN(pa::sincnet_after_sinc(sinc, p.seg.sinc, B, ws, ws + p.seg.x0, stream));
  return pa::lstm_head_run(head, p.seg.head, ws + p.seg.x0, 64, B, p.seg.sinc.T, ws, logp, multilabel, stream);
}

}  // extern "C"
