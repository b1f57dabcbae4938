/* pyannote_amd.h -- C ABI of libpyannote_amd.so (gfx950 / MI355X kernels for the
 * speaker-diarization-3.1 hot path).
 *
 * The reference (pyannote.audio 4.0.x) is 100 % Python and has NO C/FFI boundary of its own
 * (SURVEY.md section 8b); the boundary below is what the reference's Python objects would bind with
 * `ctypes` (see INTEGRATION.md for the stubs).  Each group cites the reference interface it
 * replaces, relative to src/pyannote/audio/.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless its name ends in `_host` or it is uint8;
 *     (`tensor.data_ptr()` of a contiguous torch-ROCm tensor is what callers pass)
 *   - `stream` is a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); nothing synchronises: a call enqueues
 *     kernels on `stream` (zero fills included: csrc/fill.hip, no hipMemsetAsync), on no other stream, and returns --
 *     so it can be captured into a graph and replayed (tests/test_stream_contract_gpu.py does that with every one).  The exceptions say so again in their own comment, wait
 *     for `stream` before they return because a result or a table crosses the host, and cannot be captured:
 *     pa_binarize_regions, pa_regions_sweep_count, pa_regions_sweep_emit, pa_binarize_regions_files_count,
 *     pa_binarize_regions_files_emit, and pa_kmeans_f64 when round_iterations > 0
 *   - no hidden allocation: scratch comes from the caller (`*_workspace_bytes`).  One exception, once per process and
 *     device: the FIRST launch of a persistent 3x3 convolution kernel (the convolution entry points, and the embedding
 *     forwards built on them) allocates the 256-KB pool of tile counters with hipMalloc, zeroes it on the null stream
 *     and waits for the null stream.  That first launch must therefore not be made inside a stream capture: warm up
 *     with one eager call per device; every later launch only takes a block of the pool
 *   - return 0 = OK, 1 = launch/runtime failure, 2 = out of memory, 3 = invalid argument;
 *     pa_last_error() returns a thread-local message.  Python maps 2 -> MemoryError, which is the
 *     convention of Inference.infer (core/inference.py:199-208).
 *   - all arithmetic is IEEE fp32 (f32-input MFMA; the reference disables TF32,
 *     utils/reproducibility.py:68-73); the clustering distance kernels are fp64 like SciPy.
 *
 * Workspaces (every `workspace` / `ws` argument with its `*_workspace_bytes` query)
 *   - the contents on entry may be ANYTHING -- NaN, huge values, the left-over of another call or of a larger
 *     batch -- and are unspecified on return.  Every block a call reads, it has written before on the same stream (a
 *     kernel, the fill kernel included), or the read cannot reach an output: DESIGN.md section 31 lists the blocks;
 *   - nothing outside [workspace, workspace + workspace_bytes) is touched, and a call given the bytes its query
 *     returned uses no more than those;
 *   - no output depends on the contents: the same arguments give the same output BYTES whatever the workspace held
 *     (tests/test_hostile_workspace_gpu.py).  One exception, by design: pa_vbx_iteration with first == 0 continues the
 *     call before it and reads rho and G from the workspace that call left;
 *   - the pointer must be 256-byte aligned, which every `tensor.data_ptr()` of a fresh torch allocation is: the blocks
 *     are carved at multiples of 256 bytes from it and the kernels rely on 16-byte aligned rows.  The annotation-count
 *     and regions-sweep entry points align the pointer themselves (their queries include the 256 bytes that may cost).
 */
#ifndef PYANNOTE_AMD_H
#define PYANNOTE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int pa_version(void);
const char* pa_last_error(void);

/* Built-in kernel profiler (measurement aid, no reference counterpart): while enabled every launcher
 * brackets its kernel with two hipEvents on the launch stream.  pa_prof_report synchronises and writes
 * a JSON object {"kernel": {"launches", "ms", "flops", "bytes"}} (algorithmic flops/bytes) into buf,
 * clears the records and returns the size needed. */
void pa_prof_enable(int on);
size_t pa_prof_report(char* buf, size_t cap);

/* ------------------------------------------------------------------------------------------
 * Segmentation model: replaces PyanNet.forward (models/segmentation/PyanNet.py:211-240) +
 * Powerset.to_multilabel(hard) (utils/powerset.py:115-140) as called from Inference.infer
 * (core/inference.py:182-215).
 * ---------------------------------------------------------------------------------------- */
#define PA_MAX_LSTM_LAYERS 8
#define PA_MAX_LINEAR 4

typedef struct pa_seg_weights {
  int32_t sinc_stride;   /* 10 */
  int32_t lstm_layers;   /* L */
  int32_t lstm_hidden;   /* multiple of 16 (32 when unidirectional), <= 512; 128 + bidirectional = register-resident kernel */
  int32_t lstm_bidir;    /* 1 / 0 */
  int32_t num_linear;    /* 0..PA_MAX_LINEAR */
  int32_t linear_hidden; /* multiple of 32 */
  int32_t num_classes;   /* powerset classes (7) */
  int32_t num_speakers;  /* multilabel width (3) */
  float wav_gamma, wav_beta;  /* sincnet.wav_norm1d.{weight,bias} */
  const float* sinc_filt; /* [5][63][64]  MFMA B image of the 80x251 sinc taps (tap 251 = 0) */
  const float* norm0;     /* [2][80] gamma | beta  (sincnet.norm1d.0) */
  const float* conv1_w;   /* [4][100][64] MFMA B image of sincnet.conv1d.1.weight (60,80,5) */
  const float* conv1_b;   /* [64] (60 real) */
  const float* norm1;     /* [2][60] */
  const float* conv2_w;   /* [4][75][64]  image of sincnet.conv1d.2.weight (60,60,5) */
  const float* conv2_b;   /* [64] */
  const float* norm2;     /* [2][60] */
  const float* lstm_wih[PA_MAX_LSTM_LAYERS];  /* [ndir * 4H][Kin] rows permuted (pa_lstm_rec / pa_lstm_rec_h column
                                               * order), Kin = 64 (layer 0) / ndir * H */
  const float* lstm_bias[PA_MAX_LSTM_LAYERS]; /* [ndir * 4H] b_ih + b_hh, permuted */
  const float* lstm_whh[PA_MAX_LSTM_LAYERS];  /* MFMA B image of weight_hh: [2][4][8][32][64] (H = 128, bidirectional)
                                               * or the layout of pa_lstm_rec_h */
  const float* lin_w[PA_MAX_LINEAR];          /* [out][in] as torch */
  const float* lin_b[PA_MAX_LINEAR];
  const float* cls_w;                         /* [num_classes][in] */
  const float* cls_b;
  const uint8_t* powerset_map;                /* [num_classes][num_speakers] 0/1 */
} pa_seg_weights;

/* frames per chunk for `num_samples` (SincNet.num_frames, models/blocks/sincnet.py:82-107) */
int pa_seg_num_frames(int num_samples, int sinc_stride);
size_t pa_seg_workspace_bytes(const pa_seg_weights* w, int num_chunks, int num_samples);
/* The same for callers that know the chunk stride: identical to pa_seg_workspace_bytes unless the
 * shared sinc layer applies (overlapping chunks whose stride is a multiple of 10 samples; PA_SEG_SHARED_SINC=0
 * in the environment switches it off), which needs 320 B per span position more.  pa_seg_forward falls back to the per-chunk
 * layer when the workspace it is given is the smaller one. */
size_t pa_seg_workspace_bytes_strided(const pa_seg_weights* w, int num_chunks, int num_samples,
                                      int64_t chunk_stride);
/* Chunk b is wav[b*chunk_stride : b*chunk_stride + num_samples], zero beyond wav_len
 * (Inference.slide's unfold + zero-padded last chunk, core/inference.py:261-278).
 * logp: (num_chunks, F, num_classes) log-probabilities or NULL;
 * multilabel: (num_chunks, F, num_speakers) uint8 {0,1} or NULL. */
int pa_seg_forward(const pa_seg_weights* w, const float* wav, int64_t wav_len, int64_t chunk_stride,
                   int num_chunks, int num_samples, float* logp, uint8_t* multilabel, void* workspace,
                   size_t workspace_bytes, void* stream);

/* The chunks of SEVERAL waveforms in one launch group (short files: the LSTM recurrence takes the same time for 21
 * chunks as for 2 048).  wavs / wav_lens / chunks_per_file: HOST arrays of num_files entries; wavs[f] is a device
 * pointer (read as zeros from wav_lens[f] on, never concatenated with its neighbours).  File f contributes
 * chunks_per_file[f] chunks at chunk_stride, as pa_seg_forward would take them; logp / multilabel cover the
 * concatenation of all files' chunks in file order, and every chunk's rows are bit for bit those of pa_seg_forward
 * on its file alone: the waveform statistics and the sinc layer (whose span is re-centred by the file's first chunk)
 * run per file, everything behind them once over all chunks.  A file of 0 chunks contributes nothing; 0 chunks in
 * all: returns 0, nothing is launched.  Returns 3 (pa_last_error) for a negative chunk count, more than 65 535
 * chunks, chunks too short for a frame, or a workspace below pa_seg_files_workspace_bytes (0 = invalid arguments):
 * the common buffers for all chunks + the span scratch of the longest file, reused file after file. */
size_t pa_seg_files_workspace_bytes(const pa_seg_weights* w, int num_files, const int* chunks_per_file,
                                    int num_samples, int64_t chunk_stride);
int pa_seg_forward_files(const pa_seg_weights* w, const float* const* wavs, const int64_t* wav_lens,
                         const int* chunks_per_file, int num_files, int64_t chunk_stride, int num_samples,
                         float* logp, uint8_t* multilabel, void* workspace, size_t workspace_bytes, void* stream);

/* building blocks of pa_seg_forward (exported for unit parity tests) */
int pa_row_stats(const float* x, long row_stride, long total_len, int rows, int len, float eps,
                 float* mean, float* rstd, void* stream);
int pa_sinc_fir_pool(const float* wav, long wav_len, long chunk_stride, int B, int N, int stride,
                     const float* mean, const float* rstd, float gamma, float beta,
                     const float* filt_packed, float* out, void* stream);
/* The sinc layer once per span of overlapping chunks (what pa_seg_forward runs when the chunk stride allows it).  pa_sinc_fir_span: S (80, Pc) = raw filter outputs of wav[0, span) (zeros past wav_len),
 * Pc = (span - 251) / 10 + 1.  pa_sinc_fix_pool: chunk b starts `positions_per_chunk_step` positions after chunk
 * b - 1; per-chunk affine fix-up of the waveform InstanceNorm, magnitude, maxpool3 -> out (B, 80, P) exactly what
 * pa_sinc_fir_pool writes (up to float rounding: 1e-6 of the peak); tap_sums: 80 floats of scratch. */
int pa_sinc_fir_span(const float* wav, long wav_len, long span, const float* filt_packed, float* S, void* stream);
int pa_sinc_fix_pool(const float* S, long Pc, int positions_per_chunk_step, int B, int P, const float* mean,
                     const float* rstd, float gamma, float beta, const float* filt_packed, float* tap_sums,
                     float* out, void* stream);
/* The same with the span re-centred, what pa_seg_forward runs: a DC offset that is large against the level of the
 * recording cancels in the fix-up above (the error grows like sqrt(1 + (mean / std)^2)).  mean / rstd: the chunk
 * statistics on the device, chunk 0 first (pa_sinc_fir_span_centred reads chunk 0's only).  m0 = mean[0] if
 * |mean[0]| rstd[0] > 0.5, else 0 (then S and the fix-up are those of the functions above, bit for bit) is taken off
 * the samples on load, and a chunk with |mean[b] - m0| rstd[b] > 0.5 is computed from wav (wav_len, N as in
 * pa_sinc_fir_pool, stride 10) by the per-chunk kernel instead of being fixed up. */
int pa_sinc_fir_span_centred(const float* wav, long wav_len, long span, const float* mean0, const float* rstd0,
                             const float* filt_packed, float* S, void* stream);
int pa_sinc_fix_pool_centred(const float* S, long Pc, int positions_per_chunk_step, int B, int P, const float* wav,
                             long wav_len, int N, const float* mean, const float* rstd, float gamma, float beta,
                             const float* filt_packed, float* tap_sums, float* out, void* stream);
int pa_conv5_pool(const float* xin, int B, int cin, int Lin, const float* in_mean,
                  const float* in_rstd, const float* gam, const float* bet, const float* w_packed,
                  const float* bias64, float* out, void* stream);
int pa_norm_transpose(const float* xin, int B, int T, const float* in_mean, const float* in_rstd,
                      const float* gam, const float* bet, float* X0, void* stream);
/* + act 2 = ReLU and an optional residual laid out like C (out_mode 0): C = act(A W^T + bias + Res) */
int pa_gemm_tn_ex(const float* A, int lda, const float* W, int ldw, const float* bias, const float* Res,
                  float* C, long ldc, int M, int N, int K, int act, int out_mode, void* stream);
int pa_gemm_tn(const float* A, int lda, const float* W, int ldw, const float* bias, float* C, long ldc,
               int M, int N, int K, int act, int out_mode, void* stream);
/* the 1x1 stride-2 shortcut convolution + BatchNorm of a BasicBlock / Bottleneck (resnet.py:109-118) as the same GEMM
 * reading pixel (2y, 2x) of the NHWC map X (B, H, W, cin) in place: C[(b, y, x)][n] = sum_c X[b][2y][2x][c] W[n][c]
 * + bias[n]; cin % 32 == 0 */
int pa_gemm_tn_s2(const float* X, int B, int H, int W, int cin, const float* Wt, int ldw, const float* bias, float* C,
                  long ldc, int N, void* stream);
int pa_lstm_rec(const float* xproj, const float* whh_packed, float* out, int ntiles, int ndir, int T,
                void* stream);
/* the recurrence for any hidden size H (multiple of 16, <= 512) and ndir in {1, 2} (PyanNet.py:64-72 accepts any
 * nn.LSTM configuration).  H == 128 && ndir == 2: pa_lstm_rec with its operand layouts.  Otherwise
 *   xproj : [tile][t][ndir * 4H][16], column dir * 4H + (4 u + q) * 16 + n  <->  torch gate row q H + 16 u + n (q: i,f,g,o)
 *   whh   : [dir][u][q][k4][lane][j] = weight_hh[q H + 16 u + (lane & 15)][16 k4 + 4 j + (lane >> 4)]
 *   out   : [m][ndir * H], m = (tile * T + t) * 16 + b16, columns dir * H + j */
int pa_lstm_rec_h(const float* xproj, const float* whh_packed, float* out, int ntiles, int ndir, int T, int H,
                  void* stream);
int pa_classifier(const float* X, int ldx, int K, int ntiles, int T, int B, const float* cw,
                  const float* cb, int NC, const unsigned char* mapping, int S, float* logp,
                  unsigned char* multilabel, void* stream);

/* ------------------------------------------------------------------------------------------
 * Embedding model: replaces WeSpeakerResNet34.forward (models/embedding/wespeaker/__init__.py:
 * 324-343: compute_fbank :113-139 -> ResNet.forward resnet.py:399-430 -> TSTP/StatsPool
 * resnet.py:49-66, blocks/pooling.py:30-130 -> seg_1) as called from
 * PyannoteAudioPretrainedSpeakerEmbedding.__call__ (pipelines/speaker_verification.py:704-716).
 * The backbone runs once per chunk and is pooled for all S masks (forward_frames /
 * forward_embedding split, wespeaker/__init__.py:288-322).
 * ---------------------------------------------------------------------------------------- */
#define PA_MAX_RES_BLOCKS 128   /* ResNet293: 10 + 20 + 64 + 3 = 97 blocks */

typedef struct pa_emb_weights {
  int32_t num_mel;       /* 80 */
  int32_t embed_dim;     /* 256 */
  int32_t num_layers;    /* 4 */
  int32_t num_blocks[4]; /* 3,4,6,3 (ResNet34); 3,8,36,3 / 6,16,48,3 / 10,20,64,3 (ResNet152/221/293) */
  int32_t planes[4];     /* 32,64,128,256 */
  int32_t bottleneck;    /* 0: BasicBlock (resnet.py:84-145); 1: Bottleneck, expansion 4 (resnet.py:148-212) */
  /* fbank tables */
  const float* fb_window;   /* [400] hamming (periodic=False) */
  const float* fb_tw256;    /* [256][2] exp(-2 pi i m/256) */
  const float* fb_tw512;    /* [257][2] exp(-2 pi i k/512) */
  const float* fb_mel_w;    /* [num_mel][257] */
  const int32_t* fb_mel_lo; /* [num_mel] first / last FFT bin with non-zero weight */
  const int32_t* fb_mel_hi;
  /* BatchNorm folded: w *= gamma/sqrt(var+eps), shift = beta - mean*gamma/sqrt(var+eps) */
  const float* stem_w;     /* [9][32]  (tap = 3*dmel + dtime) */
  const float* stem_shift; /* [32] */
  const float* blk_w1[PA_MAX_RES_BLOCKS];     /* [9][cout][cin] */
  const float* blk_shift1[PA_MAX_RES_BLOCKS]; /* [cout] */
  const float* blk_w2[PA_MAX_RES_BLOCKS];     /* [9][cout][cout] */
  const float* blk_shift2[PA_MAX_RES_BLOCKS];
  const float* blk_u1[PA_MAX_RES_BLOCKS];     /* [16][cout][cin] Winograd F(2x2,3x3) image G g G^T of w1, or NULL */
  const float* blk_u2[PA_MAX_RES_BLOCKS];     /* same for w2; used for stride-1 convolutions when not NULL */
  const float* blk_wsc[PA_MAX_RES_BLOCKS];    /* [cout][cin] 1x1 shortcut (stride 2, or stride 1 for the first Bottleneck) or NULL */
  const float* blk_shiftsc[PA_MAX_RES_BLOCKS];
  /* Bottleneck only: w1 = [planes][cin] 1x1, w2 / u2 = the 3x3 (stride s), w3 = [4 planes][planes] 1x1 */
  const float* blk_w3[PA_MAX_RES_BLOCKS];
  const float* blk_shift3[PA_MAX_RES_BLOCKS];
  const float* seg1_w; /* [embed_dim][2 * expansion * planes[3] * num_mel/8] */
  const float* seg1_b;
  /* Winograd F(4x4,3x3) images of w1 / w2 (pa_winograd4_pack_host), or NULL: when set, a stride-1 3x3 convolution
   * runs through pa_conv3x3_wino4 instead of pa_conv3x3_wino (blk_u*) / pa_conv3x3 (blk_w*) */
  const float* blk_v1[PA_MAX_RES_BLOCKS];
  const float* blk_v2[PA_MAX_RES_BLOCKS];
  /* fbank centring (wespeaker/__init__.py:137-157): 0 = subtract the mean over all frames of the chunk
   * (fbank_centering_span=None); odd K >= 1 = subtract the running mean of K frames (pa_fbank_center_span) */
  int32_t fb_center_kernel;
} pa_emb_weights;

/* fbank frames for num_samples (25 ms / 10 ms, snip_edges) and frames after the 3 stride-2 stages */
int pa_emb_num_fbank_frames(int num_samples);
int pa_emb_num_pool_frames(const pa_emb_weights* w, int num_samples);
size_t pa_emb_workspace_bytes(const pa_emb_weights* w, int num_chunks, int num_samples, int num_masks);
/* chunk b = wav[b*chunk_stride : +num_samples] (zero past wav_len);
 * masks: (num_chunks, S, mask_frames) fp32 or NULL (S = 1, unweighted);
 * nearest_idx: (pool_frames) int32 source index of F.interpolate(mode="nearest"), ignored if !masks;
 * emb: (num_chunks, S, embed_dim). */
int pa_emb_forward(const pa_emb_weights* w, const float* wav, int64_t wav_len, int64_t chunk_stride,
                   int num_chunks, int num_samples, const float* masks, int num_masks, int mask_frames,
                   const int32_t* nearest_idx, float* emb, void* workspace, size_t workspace_bytes,
                   void* stream);

/* Ragged batch: utterance b = wav[offsets[b] : offsets[b] + lengths[b]] (device int64 / int32 arrays, lengths[b] >= 400,
 * max_samples = max lengths[b]).  The maps are padded to max_samples and zeroed past each utterance's valid columns
 * (see emb_forward.cpp), so emb[b] is what pa_emb_forward computes for that utterance alone (up to rounding).
 * masks: (num_utterances, pa_emb_num_pool_frames(w, max_samples)) fp32 weights at pool resolution, or NULL (unweighted);
 * columns past an utterance's own pool frames are ignored.  emb: (num_utterances, embed_dim).
 * Checkpoints with fbank_centering_span are refused (return 3): run them one length at a time. */
size_t pa_emb_ragged_workspace_bytes(const pa_emb_weights* w, int num_utterances, int max_samples);
int pa_emb_forward_ragged(const pa_emb_weights* w, const float* wav, int64_t wav_len, const int64_t* offsets,
                          const int32_t* lengths, int num_utterances, int max_samples, const float* masks, float* emb,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Numerical guard of the Winograd paths (weights.EmbeddingPack runs it once per loaded checkpoint; the reference has
 * no counterpart: its convolutions are torch's direct fp32 ones, resnet.py:92-107).  The chunks go through a
 * BasicBlock network in which every stride-1 3x3 convolution is evaluated by the DIRECT kernel (whose output feeds
 * the next layer) and, beside it, by every Winograd image the block carries.
 * report (device, 8 * PA_MAX_RES_BLOCKS floats, zeroed by the call): for block b, convolution j in {0, 1}:
 *   report[4 (2 b + j) + 0] = max |direct|,  [+1] = max |F(4x4) - direct|   (both 0: no F(4x4) image)
 *   report[4 (2 b + j) + 2] = max |direct|,  [+3] = max |F(2x2) - direct|   (both 0: no F(2x2) image)
 * over the whole output map (after shift, residual and ReLU).  emb: (num_chunks, embed_dim) from the direct path. */
size_t pa_emb_calibrate_workspace_bytes(const pa_emb_weights* w, int num_chunks, int num_samples);
int pa_emb_calibrate_winograd(const pa_emb_weights* w, const float* wav, int64_t wav_len, int64_t chunk_stride,
                              int num_chunks, int num_samples, float* report, float* emb, void* workspace,
                              size_t workspace_bytes, void* stream);
/* out2[0] = max(out2[0], max |ref|), out2[1] = max(out2[1], max |got - ref|) over n floats (out2 >= 0 on entry) */
int pa_absmax_diff(const float* got, const float* ref, long n, float* out2, void* stream);

int pa_fbank(const float* wav, long wav_len, long chunk_stride, int B, int N, const float* window,
             const float* tw256, const float* tw512, const float* mel_w, const int* mel_lo,
             const int* mel_hi, int nmel, float* out, int center, void* stream);
/* Running-mean centring of fbank features, out of place (wespeaker/__init__.py:141-157): for every chunk b, frame t and
 * mel bin m,  out[b][t][m] = fb[b][t][m] - mean(fb[b][t - K/2 .. t + K/2][m] inside [0, T)),  the mean being the float32
 * sum in ascending frame order divided by the number of frames inside -- F.avg_pool1d(kernel K, stride 1, padding K / 2,
 * count_include_pad=False).  fb, out: (B, T, nmel) float32, out != fb; K odd >= 1; min(K, 2 T - 1) <= 2049. */
int pa_fbank_center_span(const float* fb, int B, int T, int nmel, int kernel, float* out, void* stream);
int pa_resnet_stem(const float* fbank, int B, int T, int F, const float* w9, const float* shift,
                   float* out, void* stream);
int pa_conv3x3(const float* X, int B, int H, int W, int cin, const float* Wg, const float* shift,
               const float* R, float* Y, int cout, int stride, int relu, void* stream);
/* The entry of a stride-2 BasicBlock in one launch: Y = [relu](conv3x3_s2(X) + shift), bit-identical to
 * pa_conv3x3(..., stride 2, ...), and the 1x1 stride-2 shortcut Ysc = conv1x1_s2(X) + shift_sc (pa_gemm_tn_s2's result
 * up to the summation order), whose pixel (2y, 2x) is the 3x3 convolution's centre tap.  Wg: [9][cout][cin], Wsc: the
 * plain [cout][cin] image.  Refused (return 3, nothing written) unless cin % 16 == 0, cout % 64 == 0, the map has at
 * least 16 output rows and Y and Ysc do not overlap; pa_conv3x3_s2_sc_supported tells the first three in advance. */
int pa_conv3x3_s2_sc_supported(int H, int cin, int cout);
int pa_conv3x3_s2_sc(const float* X, int B, int H, int W, int cin, const float* Wg, const float* shift,
                     const float* Wsc, const float* shift_sc, float* Y, float* Ysc, int cout, int relu,
                     void* stream);
/* the same stride-1 convolution through Winograd F(2x2,3x3).  U is NOT a plain [16][cout][cin] array: it is
 * G g G^T packed as one contiguous 32-KB slab per (32-cout slice, 16-cin stage),
 * [cout/32][cin/16][row = 32 xi + (cout % 32)][slot][4] with xi = 4a + b and channel quad q of the stage at
 * slot (q + 2 ((row >> 2) & 1)) & 3 -- build it with pa_winograd_pack_host (cout % 32 == 0, cin % 16 == 0). */
int pa_winograd_pack_host(const float* conv_weight /* (cout, cin, 3, 3), resnet.py:92-107 */,
                          const float* bn_scale /* (cout) gamma / sqrt(var + eps), or NULL */, int cout, int cin,
                          float* U_slabs /* HOST buffer, 16 * cout * cin floats */);
int pa_conv3x3_wino(const float* X, int B, int H, int W, int cin, const float* U, const float* shift,
                    const float* R, float* Y, int cout, int relu, void* stream);
/* the same stride-1 convolution through Winograd F(4x4,3x3) (csrc/emb_winograd4.hip: 36 instead of 64 multiplies per
 * 16 outputs; error ~1e-5 of max |Y| per convolution, tools/probes/winograd_f4_numerics.py).  U: G g G^T packed as
 * one contiguous 36-KB slab per (32-cout slice, 8-cin stage), [cout/32][cin/8][row = 32 xi + (cout % 32)][8] with
 * xi = 6a + b -- build it with pa_winograd4_pack_host (cout % 32 == 0, cin % 8 == 0, cin >= 32). */
int pa_winograd4_pack_host(const float* conv_weight /* (cout, cin, 3, 3), resnet.py:92-107 */,
                           const float* bn_scale /* (cout) gamma / sqrt(var + eps), or NULL */, int cout, int cin,
                           float* U_slabs /* HOST buffer, 36 * cout * cin floats */);
int pa_conv3x3_wino4(const float* X, int B, int H, int W, int cin, const float* U, const float* shift,
                     const float* R, float* Y, int cout, int relu, void* stream);
/* row ranges of one convolution (the maps X, R, Y are whole in every call): output rows 0 .. rows - 1 through F(4x4)
 * (rows == H or a multiple of 4 below it) and rows y_first .. H - 1 through F(2x2) (y_first even).  pa_emb_forward
 * splits a map whose height is 2 (mod 4) this way instead of padding its last F(4x4) tile row. */
int pa_conv3x3_wino4_rows(const float* X, int B, int H, int W, int cin, const float* U, const float* shift,
                          const float* R, float* Y, int cout, int relu, int rows, void* stream);
int pa_conv3x3_wino_rows(const float* X, int B, int H, int W, int cin, const float* U, const float* shift,
                         const float* R, float* Y, int cout, int relu, int y_first, void* stream);
int pa_stats_pool(const float* feat, int B, int Fh, int Tp, int C, const float* masks, int S, int Fm,
                  const int* nearest_idx, float* stats, void* stream);
/* Pieces of pa_emb_forward_ragged.  Valid width of utterance b at a map with `halvings` stride-2 stages behind it:
 * Wv_b = 1 + (lengths[b] - 400) / 160, then (Wv - 1) / 2 + 1 per stage.
 * pa_fbank_ragged: (B, T, nmel) out, T = frames of max_samples; each utterance centred on its own mean, frames past
 *   its own zero.  pa_zero_tail_cols: x (B, H, W, C) NHWC, C % 4 == 0, 16-byte aligned: columns [Wv_b, W) <- 0.
 *   pa_stats_pool_ragged: pa_stats_pool with S = 1 over columns [0, Wv_b) of utterance b; masks (B, ld_masks) at
 *   pool resolution or NULL. */
int pa_fbank_ragged(const float* wav, long wav_len, const int64_t* offsets, const int32_t* lengths, int B,
                    int max_samples, const float* window, const float* tw256, const float* tw512, const float* mel_w,
                    const int* mel_lo, const int* mel_hi, int nmel, float* out, void* stream);
int pa_zero_tail_cols(float* x, int B, int H, int W, int C, const int32_t* lengths, int halvings, void* stream);
int pa_stats_pool_ragged(const float* feat, int B, int Fh, int W, int C, const int32_t* lengths, int halvings,
                         const float* masks, int ld_masks, float* stats, void* stream);

/* ------------------------------------------------------------------------------------------
 * SSeRiouSS segmentation model: replaces SSeRiouSS.forward (models/segmentation/SSeRiouSS.py:289-328) =
 * torchaudio wav2vec 2.0 / WavLM `extract_features` -> (softmax-weighted mix of | one of) the transformer
 * layer outputs -> bi-LSTM stack -> Linear head -> classifier, as called from Inference.infer.
 * Weight layouts (all [out][in] row-major like torch unless stated):
 * ---------------------------------------------------------------------------------------- */
#define PA_W2V_MAX_CONV 8
#define PA_W2V_MAX_LAYERS 24
typedef struct pa_w2v_layer {
  const float* qk_w;   /* [2D][D] q rows then k rows (in_proj_weight[:2D] / q_proj, k_proj) */
  const float* qk_b;   /* [2D] */
  const float* v_w;    /* [D][D]; its bias is folded into out_b (soft-max rows sum to 1) */
  const float* out_w;  /* [D][D] */
  const float* out_b;  /* [D] = out_proj.bias + out_proj.weight @ v_bias */
  const float* ln1_g;  /* layer_norm */
  const float* ln1_b;
  const float* ff1_w;  /* [F][D] feed_forward.intermediate_dense */
  const float* ff1_b;
  const float* ff2_w;  /* [D][F] feed_forward.output_dense */
  const float* ff2_b;
  const float* ln2_g;  /* final_layer_norm */
  const float* ln2_b;
  const float* gate_w;     /* WavLM only: gru_rel_pos_linear [8][D/H] */
  const float* gate_b;     /* [8] */
  const float* gate_const; /* gru_rel_pos_const [H] */
} pa_w2v_layer;

typedef struct pa_sser_weights {
  int32_t num_conv;                        /* feature extractor layers (7) */
  int32_t conv_channels[PA_W2V_MAX_CONV];  /* multiples of 32 */
  int32_t conv_kernel[PA_W2V_MAX_CONV];    /* 10, 3, 3, 3, 3, 2, 2 (first <= 16) */
  int32_t conv_stride[PA_W2V_MAX_CONV];    /* 5, 2, 2, 2, 2, 2, 2 */
  int32_t extractor_layer_norm;            /* 0: "group_norm" (GroupNorm on layer 0 only), 1: "layer_norm" */
  int32_t embed_dim, num_layers, num_heads, ff_dim, layer_norm_first;
  int32_t pos_kernel, pos_groups;          /* 128, 16 */
  int32_t wavlm;                           /* gated relative position bias (rel_bias argument of the call) */
  int32_t use_layer;                       /* wav2vec_layer: < 0 = weighted mix of all layers */
  int32_t lstm_layers, lstm_hidden, lstm_bidir, num_linear, linear_hidden, num_classes, num_speakers;
  const float* conv_w[PA_W2V_MAX_CONV];      /* layer 0: [C0][K0]; layer l: [C_l][k * C_{l-1}], index j * C + c */
  const float* conv_b[PA_W2V_MAX_CONV];      /* or NULL (extractor_conv_bias = False) */
  const float* conv_norm_g[PA_W2V_MAX_CONV]; /* GroupNorm (layer 0) / LayerNorm (every layer) affine */
  const float* conv_norm_b[PA_W2V_MAX_CONV];
  const float* proj_ln_g; /* encoder.feature_projection.layer_norm */
  const float* proj_ln_b;
  const float* proj_w;    /* [D][C_last] */
  const float* proj_b;
  const float* pos_w;     /* [groups][kernel][D/groups (in)][D/groups (out)], weight_norm materialised */
  const float* pos_b;     /* [D] */
  const float* enc_ln_g;  /* encoder.transformer.layer_norm: in front of the layers iff !layer_norm_first (post-LN) */
  const float* enc_ln_b;
  pa_w2v_layer layers[PA_W2V_MAX_LAYERS];
  float layer_mix[PA_W2V_MAX_LAYERS];      /* softmax(wav2vec_weights) */
  const float* lstm_wih[PA_MAX_LSTM_LAYERS]; /* as in pa_seg_weights (layer 0: Kin = embed_dim) */
  const float* lstm_bias[PA_MAX_LSTM_LAYERS];
  const float* lstm_whh[PA_MAX_LSTM_LAYERS];
  const float* lin_w[PA_MAX_LINEAR];
  const float* lin_b[PA_MAX_LINEAR];
  const float* cls_w;
  const float* cls_b;
  const uint8_t* powerset_map;             /* NULL = multi-label head (sigmoid scores) */
} pa_sser_weights;

/* frames per chunk (SSeRiouSS.num_frames, SSeRiouSS.py:217-241); 0 = too short */
int pa_sser_num_frames(const pa_sser_weights* w, int num_samples);
size_t pa_sser_workspace_bytes(const pa_sser_weights* w, int num_chunks, int num_samples);
/* chunks and outputs as pa_seg_forward; rel_bias: [H][T][T] fp32 = rel_attn_embed[bucket(k - q)] for the
 * T = pa_sser_num_frames(num_samples) frames of a chunk (WavLM), NULL for a wav2vec 2.0 encoder */
int pa_sser_forward(const pa_sser_weights* w, const float* wav, int64_t wav_len, int64_t chunk_stride,
                    int num_chunks, int num_samples, const float* rel_bias, float* logp, uint8_t* multilabel,
                    void* workspace, size_t workspace_bytes, void* stream);
/* building blocks of pa_sser_forward (exported for unit parity tests): the encoder kernels that are not GEMMs.
 * Layout: channels-last rows; row (b, t) of a stage is row b * P + t of its buffer, P >= T the per-chunk row pitch.
 * Rows T .. P - 1 of a chunk are padding: never read as data (pa_w2v_conv0 writes zeros there, the others leave them
 * alone).  Every function checks its arguments before it computes with them and returns 3, having launched nothing,
 * when one is refused; B <= 0, rows <= 0 and n <= 0 are an empty success (0).
 *
 * pa_w2v_conv0: out[b * P + t][c] = bias[c] + sum_j w[c * K0 + j] * chunk_b[t * S0 + j] for t < T, 0 for T <= t < P;
 *   chunk_b = wav[b * chunk_stride, + N), zeros from wav_len on; w: [C][K0]; bias: [C] or NULL; 1 <= K0, S0 <= 16;
 *   P >= T >= 1, C >= 1, chunk_stride >= 0.  The caller passes T = (N - K0) / S0 + 1. */
int pa_w2v_conv0(const float* wav, long wav_len, long chunk_stride, int B, int N, int T, int P, int C, int K0, int S0,
                 const float* w, const float* bias, float* out, void* stream);
/* GroupNorm(num_groups = C) + GELU (exact erf) in place: per (chunk, channel) mean and biased variance over the T valid
 * rows of x [B * P][C], eps 1e-5; gamma, beta: [C]; mean_scratch, rstd_scratch: [B][C] floats, left holding the
 * statistics.  P >= T >= 1, C >= 1. */
int pa_w2v_group_norm_gelu(float* x, int B, int T, int P, int C, const float* gamma, const float* beta,
                           float* mean_scratch, float* rstd_scratch, void* stream);
/* LayerNorm over the C channels of each of `rows` contiguous rows [rows][C] (eps 1e-5, biased variance), then GELU if
 * gelu != 0; out may be in.  1 <= C <= 1024. */
int pa_w2v_layernorm(const float* in, float* out, long rows, int C, const float* gamma, const float* beta, int gelu,
                     void* stream);
/* convolutional positional embedding: out = x + gelu(grouped conv1d(x, padding KW / 2) + bias) on the frames 0 .. T - 1
 * of each chunk (the last frame of an even kernel is dropped), zero padding outside [0, T) of the chunk.  x, out:
 * [B * P][D], distinct buffers; w3: [g][j][ci][co] (groups, taps, input channel, output channel of the group; co
 * fastest) = torch's weight (D, D / groups, KW) as weight.reshape(groups, CG, CG, KW).permute(0, 3, 2, 1); bias: [D].
 * groups >= 1, KW >= 1, D % groups == 0, P >= T >= 1, (16 + KW - 1) * D / groups floats within 64 KiB of LDS. */
int pa_w2v_posconv(const float* x, int B, int T, int P, int D, int groups, int KW, const float* w3, const float* bias,
                   float* out, void* stream);
/* attention soft-max in place: S [B][H][T][Tp] (row pitch Tp >= T) <- softmax_k(S * scale + gate[b][h][t] * bias[h][t][k])
 * over k < T; columns T .. Tp - 1 are set to 0.  bias: [H][T][T] or NULL (no gate; xin, gate_* are then unused).
 * gate (WavLM): q = xin[b * P + t][h * hd, + hd), hd = D / H; u = gate_w q + gate_b (gate_w [8][hd], gate_b [8]);
 * gate = ga * (gb * gate_const[h] - 1) + 2 with ga = sigmoid(u0 + .. + u3), gb = sigmoid(u4 + .. + u7).
 * Tp >= T >= 1, H >= 1, D % H == 0, hd <= 128; with a bias xin, gate_w, gate_b, gate_const non-NULL and P >= T. */
int pa_w2v_softmax(float* S, int B, int H, int T, int Tp, float scale, const float* bias, const float* xin, int P, int D,
                   const float* gate_w, const float* gate_b, const float* gate_const, void* stream);
/* acc[i] = (first ? 0 : acc[i]) + w * x[i], i < n (one fma); n % 4 == 0, both 16-byte aligned */
int pa_w2v_axpy(float* acc, const float* x, float w, long n, int first, void* stream);
/* rows [b * P + t][D] -> LSTM input rows out[((b >> 4) * T + t) * 16 + (b & 15)][D]; the chunks B .. 16 * ceil(B / 16) - 1
 * are zero.  P >= T >= 1, D >= 1. */
int pa_w2v_to_tiles(const float* x, int B, int T, int P, int D, float* out, void* stream);
/* outer x inner independent TN GEMMs in one launch (operand z = (zo, zi) starts zo * s?o + zi * s?i floats
 * after its base pointer); act 0 or 3 (GELU) */
int pa_gemm_tn_batched(const float* A, int lda, long sAo, long sAi, const float* W, int ldw, long sWo, long sWi,
                       const float* bias, float* C, long ldc, long sCo, long sCi, int M, int N, int K,
                       int outer, int inner, int act, void* stream);

/* ------------------------------------------------------------------------------------------
 * XVectorSincNet embedding model: replaces XVectorSincNet.forward (models/embedding/xvector.py:330-349) =
 * SincNet -> 5 x (Conv1d(k, dilation) + LeakyReLU + BatchNorm1d) -> StatsPool(weights) -> Linear, as called
 * by PyannoteAudioPretrainedSpeakerEmbedding (pipelines/speaker_verification.py:704-716).
 * ---------------------------------------------------------------------------------------- */
#define PA_XVEC_TDNN 5
typedef struct pa_xvec_weights {
  int32_t sinc_stride;                 /* 10 */
  int32_t dimension;                   /* embedding size (512) */
  int32_t tdnn_channels[PA_XVEC_TDNN]; /* 512, 512, 512, 512, 1500 (multiples of 4) */
  int32_t tdnn_kernel[PA_XVEC_TDNN];   /* 5, 3, 3, 1, 1 */
  int32_t tdnn_dilation[PA_XVEC_TDNN]; /* 1, 2, 3, 1, 1 */
  float wav_gamma, wav_beta;           /* SincNet fields: exactly those of pa_seg_weights */
  const float* sinc_filt;
  const float* norm0;
  const float* conv1_w;
  const float* conv1_b;
  const float* norm1;
  const float* conv2_w;
  const float* conv2_b;
  const float* norm2;
  /* [k][cout][cin_pad] per layer (cin_pad = 64 for layer 0), the PREVIOUS layer's BatchNorm folded in */
  const float* tdnn_w[PA_XVEC_TDNN];
  const float* tdnn_b[PA_XVEC_TDNN];
  const float* bn_scale; /* [channels[4]] the LAST BatchNorm as an affine map, applied inside the pooling */
  const float* bn_shift;
  const float* emb_w; /* [dimension][ld] ld = 2 * channels[4] rounded up to 32 (zero padded) */
  const float* emb_b;
} pa_xvec_weights;

/* frames left after SincNet and the TDNN stack (XVectorSincNet.num_frames, xvector.py:264-287); 0 = too short */
int pa_xvec_num_frames(const pa_xvec_weights* w, int num_samples);
size_t pa_xvec_workspace_bytes(const pa_xvec_weights* w, int num_chunks, int num_samples, int num_masks);
/* chunks addressed like pa_seg_forward; masks (num_chunks, num_masks, mask_frames) fp32 or NULL (unweighted
 * pooling), nearest_idx (frames) = F.interpolate(mode="nearest") source index of every pooled frame;
 * emb: (num_chunks * num_masks, dimension) */
int pa_xvec_forward(const pa_xvec_weights* w, const float* wav, int64_t wav_len, int64_t chunk_stride,
                    int num_chunks, int num_samples, const float* masks, int num_masks, int mask_frames,
                    const int32_t* nearest_idx, float* emb, void* workspace, size_t workspace_bytes,
                    void* stream);
/* ------------------------------------------------------------------------------------------
 * XVectorMFCC embedding model: replaces XVectorMFCC.forward (models/embedding/xvector.py:185-202) =
 * torchaudio MFCC -> the same TDNN stack, pooling and Linear as XVectorSincNet.  The front end (csrc/mfcc.hip)
 * is built for n_fft = win_length = 400, reflect padding, power 2, not normalized; the filter bank, window and DCT
 * matrix are data (the checkpoint's torchaudio buffers).
 * ---------------------------------------------------------------------------------------- */
typedef struct pa_xvec_mfcc_weights {
  int32_t n_fft;                       /* 400 */
  int32_t hop_length;                  /* 1 .. 400 */
  int32_t center;                      /* 1: frames reflect-padded by n_fft / 2 on each side of the chunk */
  int32_t log_mels;                    /* 1: log(mel + 1e-6); 0: dB, clamped at the chunk's max - 80 dB */
  int32_t n_mels;                      /* <= 256 */
  int32_t n_mfcc;                      /* <= 64 */
  int32_t dimension;                   /* embedding size */
  int32_t tdnn_channels[PA_XVEC_TDNN]; /* as pa_xvec_weights */
  int32_t tdnn_kernel[PA_XVEC_TDNN];
  int32_t tdnn_dilation[PA_XVEC_TDNN];
  const float* window;                 /* [400] */
  const float* fft_tw;                 /* complex [200] exp(-2 pi i m / 200), then [201] exp(-2 pi i k / 400) */
  const float* mel_w;                  /* [n_mels][201] = torchaudio's fb transposed */
  const int32_t* mel_lo;               /* [n_mels] first / last non-zero bin of each filter (lo > hi: none) */
  const int32_t* mel_hi;
  const float* dct;                    /* [n_mels][64] torchaudio's dct_mat, zero past n_mfcc */
  const float* tdnn_w[PA_XVEC_TDNN];   /* as pa_xvec_weights (cin_pad = 64 for layer 0) */
  const float* tdnn_b[PA_XVEC_TDNN];
  const float* bn_scale;
  const float* bn_shift;
  const float* emb_w;
  const float* emb_b;
} pa_xvec_mfcc_weights;

/* frames left after the MFCC front end and the TDNN stack (XVectorMFCC.num_frames, xvector.py:96-126; 0 = too short,
 * which includes a centred chunk of at most n_fft / 2 samples: torch's reflect padding refuses it) */
int pa_xvec_mfcc_num_frames(const pa_xvec_mfcc_weights* w, int num_samples);
size_t pa_xvec_mfcc_workspace_bytes(const pa_xvec_mfcc_weights* w, int num_chunks, int num_samples, int num_masks);
/* the contract of pa_xvec_forward; samples past wav_len read as zero */
int pa_xvec_mfcc_forward(const pa_xvec_mfcc_weights* w, const float* wav, int64_t wav_len, int64_t chunk_stride,
                         int num_chunks, int num_samples, const float* masks, int num_masks, int mask_frames,
                         const int32_t* nearest_idx, float* emb, void* workspace, size_t workspace_bytes,
                         void* stream);
/* the MFCC front end alone: out (num_chunks, frames, n_mfcc) = torchaudio's MFCC of each chunk, transposed;
 * workspace: pa_xvec_mfcc_workspace_bytes(w, num_chunks, num_samples, 1) bytes suffice */
int pa_mfcc_features(const pa_xvec_mfcc_weights* w, const float* wav, int64_t wav_len, int64_t chunk_stride,
                     int num_chunks, int num_samples, float* out, void* workspace, size_t workspace_bytes,
                     void* stream);

/* StatsPool over the rows of a (tile, t, b16)-ordered activation matrix (models/blocks/pooling.py:64-130) */
int pa_stats_pool_rows(const float* feat, int B, int T0, int Tp, int C, int ld, const float* masks, int S,
                       int Fm, const int* nearest_idx, float* stats, int ld_stats,
                       const float* aff_scale /* (C) or NULL: x -> scale x + shift on load */,
                       const float* aff_shift, void* stream);

/* ------------------------------------------------------------------------------------------
 * Clustering distances (fp64, bit-identical to SciPy): replace the pdist inside
 * scipy.cluster.hierarchy.linkage(X, "centroid", "euclidean") (pipelines/clustering.py:374-382) and
 * scipy.spatial.distance.cdist(E, centroids, "cosine") (pipelines/clustering.py:190-200).
 * ---------------------------------------------------------------------------------------- */
/* out: condensed (N*(N-1)/2) upper triangle, pair order (0,1),(0,2),...,(N-2,N-1) */
int pa_pdist_f64(const double* X, int N, int D, double* out, void* stream);
/* out: (NA, NB); norms: scratch of NA + NB doubles */
int pa_cdist_cosine_f64(const double* A, int NA, const double* B, int NB, int D, double* out,
                        double* norms, void* stream);

/* Cluster centroids, bit-identical to np.mean(X[rows of cluster k], axis=0) (pipelines/clustering.py:182-187,
 * :462-472: float32 row-order sums divided in float32).  X: (., D) float32 rows; rows: row numbers grouped by
 * cluster, original order inside a cluster; offsets: K + 1 group boundaries into `rows`; out: (K, D) float32, NaN
 * rows for empty clusters. */
int pa_centroid_means(const float* X, int D, const int* rows, const int* offsets, int K, float* out, void* stream);

/* Centroid-linkage dendrogram, bit-identical to scipy.cluster.hierarchy.linkage(y, "centroid")
 * (pipelines/clustering.py:374-382).  D: condensed distances (n*(n-1)/2 doubles, e.g. straight from
 * pa_pdist_f64), OVERWRITTEN when the heap kernel runs;  Z: (n-1, 4) doubles in SciPy's layout [id_a, id_b,
 * height, size].  Two kernels behind one call (csrc/linkage_fast.hip, csrc/linkage.hip): a heap-free merge on a
 * square copy of the matrix over 1 / 8 / 16 workgroups, and -- only when two rows ever tie for the smallest lower
 * bound, i.e. when SciPy's heap order would matter -- the exact replay of SciPy's heap on the condensed matrix
 * by ONE workgroup.  The number of workgroups of the heap-free merge only depends on n (PA_LINKAGE_FAST_WGS
 * overrides it for experiments).
 * The workspace holds the square copy (8 n^2 bytes; PA_LINKAGE_FAST_MAX_GB caps it, default 96). */
size_t pa_linkage_workspace_bytes(int n);
int pa_linkage_centroid_f64(double* D, int n, double* Z, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * Single, complete, average, weighted and Ward linkage (csrc/linkage_chain.hip), bit-identical to
 * scipy.cluster.hierarchy.linkage(y, method): the other values of AgglomerativeClustering.method
 * (pipelines/clustering.py:292-480).  What runs where: these five and centroid on the device; median -- and any size
 * whose square matrix exceeds the cap below -- on the host in SciPy.
 * ---------------------------------------------------------------------------------------- */
enum {
  PA_LINKAGE_SINGLE = 0,   /* _hierarchy.mst_single_linkage */
  PA_LINKAGE_COMPLETE = 1, /* _hierarchy.nn_chain with max(a, b) */
  PA_LINKAGE_AVERAGE = 2,  /* ... (nx a + ny b) / (nx + ny) */
  PA_LINKAGE_WEIGHTED = 3, /* ... 0.5 (a + b) */
  PA_LINKAGE_WARD = 4      /* ... sqrt(((ni + nx) a^2 + (ni + ny) b^2 - ni c^2) / (nx + ny + ni)) */
};
/* scipy.spatial.distance.pdist(X, "cosine") with the arithmetic of the cosine cdist above.  out: condensed, the
 * layout of the Euclidean pdist;  norms: scratch of N doubles.  A zero row yields NaN, as in SciPy. */
int pa_pdist_cosine_f64(const double* X, int N, int D, double* out, double* norms, void* stream);
/* *flag (one int in device memory) = 1 when any of the `count` doubles is NaN or infinite, else 0: the check SciPy's
 * linkage makes on its input ("The condensed distance matrix must contain only finite values."), to be read by the
 * caller BEFORE the merge is launched. */
int pa_nonfinite_flag_f64(const double* v, long count, int* flag, void* stream);
/* The unsorted merge list of SciPy's algorithm from a condensed matrix D (n*(n-1)/2 doubles, left intact).
 * raw: (n-1, 4) doubles [x, y, height, size of the merger], x < y cluster slots in merge order for the chain
 * methods; [x, y, height, 0] in Prim's order for single.  SciPy's dendrogram is the stable sort of these rows by
 * height followed by its union-find relabelling (distance.linkage_finish).  One persistent workgroup on a square
 * copy of the matrix in the workspace (8 n^2 bytes; PA_LINKAGE_FAST_MAX_GB caps it, default 96: the workspace query
 * returns 0 for n < 2 or above the cap).  After the kernel the first int of the workspace is 0; anything else means
 * that a loop bound of the algorithm was exceeded and `raw` is incomplete.  Refused with return code 3, nothing
 * written: n < 2, unknown method, null pointer, workspace too small, square matrix above the cap. */
size_t pa_linkage_chain_workspace_bytes(int n);
int pa_linkage_chain_f64(const double* D, int n, int method, double* raw, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Frame-domain stages (uint8 hard segmentations in, per-frame decisions out).  Replace the Python
 * loops of Inference.aggregate (core/inference.py:589-611), speaker_count
 * (pipelines/utils/diarization.py:150-185), SpeakerDiarization.reconstruct
 * (pipelines/speaker_diarization.py:480-528), to_diarization (pipelines/utils/diarization.py:
 * 221-268) and the numpy reductions of filter_embeddings (pipelines/clustering.py:109-116) and
 * get_embeddings' mask selection (pipelines/speaker_diarization.py:375-427).
 * seg: (C, F, S) uint8 {0,1};  start_frame: (C) int32 = closest_frame(chunk.start + frame.duration/2)
 * (core/inference.py:596), computed by the caller in float64 exactly as the reference does.
 * ---------------------------------------------------------------------------------------- */
/* Dense chunk buffer from several device-resident waveforms (csrc/gather.hip): out (num_chunks, num_samples) fp32,
 * out[c][i] = file_ptr[chunk_file[c]][chunk_start[c] + i], 0 where chunk_start[c] + i >= file_len[chunk_file[c]].
 * All four tables are DEVICE arrays: per file its base pointer and length in samples, per chunk its file index and
 * first sample (>= 0).  What a launch group of the embedding network reads when its chunks come from several
 * files; 16-byte accesses where base + start and the output row are 16-byte aligned. */
int pa_gather_chunks(const float* const* file_ptr, const int64_t* file_len, const int32_t* chunk_file,
                     const int64_t* chunk_start, int num_chunks, int num_samples, float* out, void* stream);
/* active[c][s] = sum_f seg;  clean[c][s] = sum_f seg * [sum_s' seg == 1]   (both (C,S) int32) */
int pa_seg_chunk_stats(const uint8_t* seg, int C, int F, int S, int32_t* active, int32_t* clean,
                       void* stream);
/* masks (C,S,F) fp32: the overlap-free mask where exclude_overlap && clean[c][s] > min_num_frames,
 * the full mask otherwise */
int pa_embedding_masks(const uint8_t* seg, int C, int F, int S, const int32_t* clean,
                       int exclude_overlap, int min_num_frames, float* masks, void* stream);
/* count (T) uint8 = rint( overlap-add average of sum_s seg );  scratch: 2*T int32 */
int pa_speaker_count(const uint8_t* seg, int C, int F, int S, const int32_t* start_frame, int T,
                     uint8_t* count, int32_t* scratch, void* stream);
/* act (T,K) int32 = overlap-add SUM over chunks of max_{s: hard[c][s]==k} seg[c][f][s];
 * hard: (C,S) int32, negative = unassigned / inactive */
int pa_cluster_activations(const uint8_t* seg, int C, int F, int S, const int32_t* start_frame,
                           const int32_t* hard, int K, int T, int32_t* act, void* stream);
/* out (T,K) uint8: the min(count[t], cap, K) most active clusters per frame, ties to the lowest index;
 * tie (T) uint8: 1 where equal activations straddle the selection boundary (the reference's
 * np.argsort order among equals is host-dependent: the caller re-decides those frames with numpy) */
int pa_topk_binarize(const int32_t* act, const uint8_t* count, int T, int K, int cap, uint8_t* out,
                     uint8_t* tie, void* stream);

/* Soft-score (non-powerset segmentation) forms of the same stages:
 * hysteresis thresholding = `binarize` (utils/signal.py:78-140; pipelines/speaker_diarization.py:599-606):
 * scores (C,F,K) fp32 -> out (C,F,K) uint8; on where score > onset, off where score < offset, unchanged in
 * between, NaN = 0; initial_state 0 / 1, or -1 for `scores[:, 0] >= midpoint`.  `midpoint` is the reference's
 * threshold for that comparison: 0.5 * (onset + offset) formed in double precision from the caller's double
 * thresholds and rounded once to fp32 (numpy compares fp32 scores with the Python float that way).  It is an argument
 * because the two fp32 thresholds cannot carry it: 0.5f * (onset + offset) in fp32 is one ulp off for some pairs,
 * (0.4, 0.3) among them.  Read only when initial_state is -1. */
int pa_binarize_hysteresis(const float* scores, int C, int F, int K, float onset, float offset, float midpoint,
                           int initial_state, uint8_t* out, void* stream);
/* out (C,F,K) fp32 = max_{s: hard[c][s]==k} scores[c][f][s], NaN when chunk c has no speaker in cluster k
 * (pipelines/speaker_diarization.py:506-522); overlap-add it with pa_aggregate(skip_average = 1). */
int pa_cluster_max(const float* scores, int C, int F, int S, const int32_t* hard, int K, float* out,
                   void* stream);
/* pa_topk_binarize on fp32 activations (>= 0, no NaN) */
int pa_topk_binarize_f32(const float* act, const uint8_t* count, int T, int K, int cap, uint8_t* out,
                         uint8_t* tie, void* stream);

/* General overlap-add aggregation, replaces Inference.aggregate (core/inference.py:498-620):
 * scores (C,F,K) fp32 (NaN = missing), window (F) fp64 = Hamming or ones, warm (F) fp64 = warm-up
 * window, start_frame (C) non-decreasing -> out (T,K) fp32 = sum / max(weight sum, epsilon) (or the plain sum), `missing` where
 * nothing voted.  Bit-identical to the reference's chunk loop (same accumulation order and dtypes). */
int pa_aggregate(const float* scores, int C, int F, int K, const int32_t* start_frame, int T,
                 const double* window, const double* warm, float epsilon, float missing, int skip_average,
                 float* out, void* stream);

/* pa_aggregate for a ragged list of files in ONE launch (detection pipelines on a list of files, DESIGN.md section
 * 32).  scores (total_chunks, F, S) on the device: the chunks of all files in file order, as pa_seg_forward_files
 * leaves them; fp32, or (scores_uint8) the uint8 hard multilabel output, whose values count as 0.f / 1.f.  DEVICE
 * tables: chunk0 (num_files + 1) int32, file f owns chunks chunk0[f] .. chunk0[f + 1] - 1; row0 (num_files + 1) int32
 * non-decreasing, file f owns rows row0[f] .. row0[f + 1] - 1 of `out`; T (num_files) int32 <= row0[f + 1] - row0[f],
 * the frames kept for the file.  All files share the chunk grid: start_frame (max_chunks) int32 is indexed by a
 * chunk's position in its file, max_chunks >= every file's chunk count.  window, warm, epsilon, missing,
 * skip_average: as for pa_aggregate.  any = 0: K = S (fp32 scores only); any = 1: K = 1 and a chunk's value at a frame
 * is the maximum of its S columns, NaN when one of them is (np.max).
 * out (rows, K) fp32, rows = row0[num_files]: rows row0[f] .. row0[f] + T[f] - 1 equal, bit for bit, the first T[f]
 * rows pa_aggregate gives for file f's chunks alone (collapsed first, with `any`); every other row is NaN.  A file
 * without chunks owns no rows.  uint8 scores with any = 0 are refused (3). */
int pa_aggregate_files(const void* scores, int scores_uint8, int total_chunks, int F, int S, int any, int num_files,
                       const int32_t* chunk0, const int32_t* row0, const int32_t* T, const int32_t* start_frame,
                       int max_chunks, const double* window, const double* warm, float epsilon, float missing,
                       int skip_average, long rows, float* out, void* stream);

/* Hysteresis thresholding of an aggregated score array into per-class region lists, replaces `Binarize.__call__`
 * (utils/signal.py:254-318) applied to every class, `Annotation.support(collar)` and the min_duration_on deletion:
 * scores (T,K) fp32 row-major on the device (as pa_aggregate leaves it), K <= 16.  onset / offset (K) fp32 and
 * min_duration_on / min_duration_off (K) fp64 are HOST arrays.  State rule per class: inactive -> active iff
 * score > onset, active -> inactive iff score < offset (fp32 comparisons, NaN changes nothing); state of frame 0 =
 * score > onset.  A region runs from the middle of the frame that switched on to the middle of the frame that
 * switched off (or of the last frame); middle of frame i = 0.5 * (s + (s + duration)), s = start + i * step, fp64,
 * bit-identical to the host.  Regions not longer than 1e-6 do not exist; with min_duration_off > 0 neighbours whose gap
 * is shorter are merged, then with min_duration_on > 0 shorter regions are removed.
 * Outputs (device): counts (K) int32; regions (K, capacity, 2) fp64 start / end in time order, class k's at
 * regions + k * capacity * 2; tracks (K, capacity) int32, optional (NULL): index of every region among the class's
 * regions after merging and before removal when min_duration_off > 0, else 0 (its track name in the reference).
 * `capacity` bounds a class's regions BEFORE merging (at most T / 2): if a class needs more, nothing is written past
 * capacity, the call returns 3 and pa_last_error says which class.  T < 2 gives zero regions.  The call waits for the
 * stream (it reads the counts back to check the capacity). */
size_t pa_binarize_regions_workspace_bytes(int T, int K, int capacity);
int pa_binarize_regions(const float* scores, int T, int K, const float* onset, const float* offset,
                        const double* min_duration_on, const double* min_duration_off, double start,
                        double duration, double step, int capacity, int32_t* counts, double* regions,
                        int32_t* tracks, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the regions of many detectors from one pass over the scores (tuning onset / offset / min_duration_on /
 *      min_duration_off of a detection pipeline on a corpus; csrc/regions_sweep.hip) ---- */

/* scores (T,K) fp32 on the device, K <= 16, as for pa_binarize_regions.  HOST arrays: L LANES (lane_class int32 in
 * 0..K-1, onset, offset fp32) and M JOBS (job_lane int32 in 0..L-1, min_duration_on / min_duration_off fp64), jobs in
 * any order, any number of jobs per lane, lanes may repeat.  Job j's region list and track positions are, bit for
 * bit, what pa_binarize_regions gives for column lane_class[job_lane[j]] with the job's four parameters.
 * Lanes of one class are grouped sixteen to a map word (classes ascending, lanes in order): the scores are read per
 * group, the hysteresis runs once per lane.  Two phases, because the row buffers are sized from counts:
 *   pa_regions_sweep_count   n_raw (L) int32, HOST, overwritten: the regions of every lane before any clean-up.
 *   pa_regions_sweep_emit    takes those counts back; regions (rows, 2) fp64 and tracks (rows) int32 (optional, NULL)
 *                            on the device: job after job, each in time order; job_off (M + 1) int32 on the device:
 *                            job j owns rows job_off[j] .. job_off[j + 1].  rows >= sum over jobs of
 *                            n_raw[job_lane[j]] (the bound a job's list has before merging).
 * `workspace` (device): pa_regions_sweep_workspace_bytes(T, groups, groups_per_launch, L, M, raw_rows, job_rows) with
 * groups = pa_regions_sweep_groups(K, L, lane_class) (-1: K or a class out of range), raw_rows = sum of n_raw,
 * job_rows as above (M = raw_rows = job_rows = 0 for the counting phase).  A workspace smaller than
 * groups_per_launch = groups asks for (at least groups_per_launch = 1) splits the groups over several launch
 * sequences; results do not depend on the split.  launches (optional, HOST): how many sequences ran.
 * T < 2, L == 0 or M == 0 give zero counts / an all-zero offset table.  K outside 1..16, a lane's class outside
 * 0..K-1, a job's lane outside 0..L-1 and NaN thresholds or durations are refused before any launch (3,
 * pa_last_error).  No workgroup waits for another, no floating-point atomics.  Both calls wait for the stream. */
int pa_regions_sweep_groups(int K, int L, const int32_t* lane_class);
size_t pa_regions_sweep_workspace_bytes(int T, int groups, int groups_per_launch, int L, int M, long raw_rows,
                                        long job_rows);
int pa_regions_sweep_count(const float* scores, int T, int K, int L, const int32_t* lane_class, const float* onset,
                           const float* offset, int32_t* n_raw, int32_t* launches, void* workspace,
                           size_t workspace_bytes, void* stream);
int pa_regions_sweep_emit(const float* scores, int T, int K, int L, const int32_t* lane_class, const float* onset,
                          const float* offset, const int32_t* n_raw, int M, const int32_t* job_lane,
                          const double* min_duration_on, const double* min_duration_off, double start, double duration,
                          double step, long rows, double* regions, int32_t* tracks, int32_t* job_off,
                          int32_t* launches, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the regions of every (file, class) of a ragged list of files from one pass (csrc/regions_files.hip, DESIGN.md
 *      section 32) ---- */

/* scores (rows, K) fp32 on the device as pa_aggregate_files leaves it, K <= 16.  HOST arrays: row0 (num_files + 1)
 * int32, row0[0] = 0, non-decreasing multiples of 64, rows = row0[num_files]; T (num_files) int32, 0 <= T[f] <=
 * row0[f + 1] - row0[f]; onset / offset (K) fp32 and min_duration_on / min_duration_off (K) fp64, one set for all
 * files.  For every file f and class k the region list and the track positions are, bit for bit, what
 * pa_binarize_regions gives on rows row0[f] .. row0[f] + T[f] - 1 alone with the same parameters: times are counted
 * from the file's own frame 0, nothing is merged across files, T[f] < 2 gives empty lists.  Two phases, because the
 * row buffers are sized from counts:
 *   pa_binarize_regions_files_count   n_raw (K) int32, HOST, overwritten: the regions of every class, over all files,
 *                                     before any clean-up.
 *   pa_binarize_regions_files_emit    takes those counts back (other counts than the scores have: 3); regions
 *                                     (rows_out, 2) fp64 and tracks (rows_out) int32 (optional, NULL) on the device,
 *                                     list after list in (file, class) order, each in time order; list_off
 *                                     (num_files K + 1) int32 on the device: list f K + k owns rows list_off[f K + k]
 *                                     .. list_off[f K + k + 1].  rows_out >= the sum of n_raw.
 * `workspace` (device): pa_binarize_regions_files_workspace_bytes(rows, K, num_files, raw_rows), raw_rows = the sum of
 * n_raw (0 for the counting phase).  K outside 1..16, NaN thresholds, durations or grid, row0 that decreases or is no
 * multiple of 64, T[f] outside its file's rows, more than 65 535 files and a workspace below the stated size are
 * refused before any launch (3, pa_last_error) with every output untouched.  No workgroup waits for another, no
 * floating-point atomics, every loop is bounded by an argument.  Both calls wait for the stream. */
size_t pa_binarize_regions_files_workspace_bytes(long rows, int K, int num_files, long raw_rows);
int pa_binarize_regions_files_count(const float* scores, int K, int num_files, const int32_t* row0, const int32_t* T,
                                    const float* onset, const float* offset, int32_t* n_raw, void* workspace,
                                    size_t workspace_bytes, void* stream);
int pa_binarize_regions_files_emit(const float* scores, int K, int num_files, const int32_t* row0, const int32_t* T,
                                   const float* onset, const float* offset, const double* min_duration_on,
                                   const double* min_duration_off, double start, double duration, double step,
                                   const int32_t* n_raw, long rows_out, double* regions, int32_t* tracks,
                                   int32_t* list_off, void* workspace, size_t workspace_bytes, void* stream);

/* ---- audio front door (core/io.py:223-265) ---- */

/* Polyphase windowed-sinc resampling, replaces torchaudio.functional.resample in
 * Audio.downmix_and_resample (core/io.py:258-262): x (n) fp32 -> out (n_out) fp32,
 * out[q P + p] = sum_k taps[p][k] x[q L - width + k], K = 2 width + L taps per phase, zeros outside x. */
int pa_resample_poly(const float* x, long n, const float* taps, int L, int P, int K, int width, float* out,
                     long n_out, void* stream);

/* ---- VBx clustering + PLDA (pipelines/clustering.py:550-669, utils/vbx.py:27-218, core/plda.py:33-60) ---- */

/* x-vector -> PLDA space, replaces PLDA.__call__ (core/plda.py:47-60) = plda_tf(xvec_tf(x))
 * (utils/vbx.py:205-217): X (n, din) fp32 -> fea (n, dout) fp64.  lda [din][dmid], trT [dmid][dout]. */
int pa_plda_transform(const float* X, int n, int din, int dmid, int dout, const double* mean1,
                      const double* lda, const double* mean2, const double* mu, const double* trT,
                      double* fea, void* stream);
size_t pa_vbx_workspace_bytes(int n, int s, int d);
/* one iteration of VBx (utils/vbx.py:106-133): M step (16)(17), E step (23) + GMM responsibilities,
 * ELBO (25) -> elbo_out[0].  gamma (n, s) fp64 is updated in place. */
int pa_vbx_iteration(const double* fea, const double* Phi, int n, int s, int d, double Fa, double Fb,
                     int first, double* gamma, double* elbo_out, void* workspace, size_t workspace_bytes,
                     void* stream);
/* bytes of `workspace` below, from the number of jobs, n, the largest S of the call and d (0: an argument is
 * not positive) */
size_t pa_vbx_batch_workspace_bytes(int jobs, int n, int smax, int d);
/* Whole VB inferences for `jobs` jobs over the same features fea (n, d), d = 128: no read-back, no host
 * synchronisation.  Job j starts from the (n, S_j) responsibilities at gamma0 + job_init[2 j] (an offset in
 * doubles; gamma0 holds gamma0_len doubles and is only read, several jobs may name the same ones), with
 * S_j = job_init[2 j + 1] <= smax, Fa = job_f[2 j] and Fb = job_f[2 j + 1]; both tables are device arrays.  rho and
 * G are computed once and shared.  Every round is the three steps of pa_vbx_iteration launched once for all jobs;
 * after the ELBO of round `it` a job's ELBO workgroup applies `it > 0 && elbo[it] - elbo[it - 1] < epsilon` in
 * double and, if it holds, retires the job, whose workgroups return at entry from then on.  max_iterations rounds
 * are enqueued.  gamma (jobs, n * smax): the final (n, S_j) responsibilities of job j, contiguous at the start of
 * its slab; elbo (jobs, max_iterations): its history, valid up to iterations[j] (jobs; 0 for a job whose table
 * entry is out of range, which is left alone).  Per job, bit for bit what max_iterations calls of
 * pa_vbx_iteration followed by that test on the host give. */
int pa_vbx_run_batch(const double* fea, const double* Phi, int n, int d, int jobs, const double* gamma0,
                     long gamma0_len, const int64_t* job_init, const double* job_f, int smax,
                     int max_iterations, double epsilon, double* gamma, double* elbo, int32_t* iterations,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- constrained assignment of local speakers to clusters (pipelines/clustering.py:127-140) ---- */

/* limits of pa_constrained_assign: local speakers per chunk (4) and clusters (64) */
int pa_constrained_assign_max_speakers(void);
int pa_constrained_assign_max_clusters(void);
/* soft (chunks, speakers, clusters) fp64 and silent (chunks, speakers) uint8 on the device.  Per chunk: the
 * injective map of the non-silent rows into the clusters with the largest sum (a partial map of `clusters` rows
 * when there are fewer clusters than non-silent rows), found by exhaustive search over each row's best columns.
 * hard (chunks, speakers) int8: the cluster of every row, -2 for a silent or unassigned row.  flagged (chunks)
 * uint8: 1 where the optimum is not safely unique -- a non-silent row holds a non-finite value; another map comes
 * within 1e-9 of the best total; or, with more clusters than non-silent rows A, the A-th and (A+1)-th best value of
 * a row lie within 1e-9 (the search keeps A columns per row, and a map through a dropped column loses at least that
 * gap, so a larger gap proves that no unseen map is a runner-up); the rows of such a chunk are all -2 and the caller solves it with the solver
 * whose tie-breaking it wants to reproduce. */
int pa_constrained_assign(const double* soft, const unsigned char* silent, int chunks, int speakers, int clusters,
                          signed char* hard, unsigned char* flagged, void* stream);

/* ---- frame-level diarization error rates (utils/metric.py:41-93,
 *      torchmetrics/functional/audio/diarization_error_rate.py:33-162) ---- */

/* File mode: ref (T, Sr) and hyp (T, Sh) uint8 (non-zero = on), row-major, 1 <= Sr, Sh <= 32, T < 2^31;
 * keep (T) uint8 optional (NULL): frames with 0 are ignored.  One pass, exact integer sums.
 * out, int64, Sr*Sh + Sr + Sh + 4 values, overwritten:
 *   cooc (Sr, Sh)   frames in which reference speaker i and hypothesis speaker j are both on
 *   ref_frames (Sr), hyp_frames (Sh)
 *   total = sum Nr, false_alarm = sum max(0, Nh - Nr), missed = sum max(0, Nr - Nh), both = sum min(Nr, Nh)
 * (Nr / Nh = speakers on in a frame).  Under a one-to-one speaker mapping pi, correct = sum_i cooc[i][pi(i)] and
 * confusion = both - correct; the reference's mapping maximises `correct` (csrc/metrics.hip). */
int pa_der_counts(const uint8_t* ref, const uint8_t* hyp, const uint8_t* keep, long T, int Sr, int Sh,
                  int64_t* out, void* stream);

/* Chunk mode: preds (B, S, F) fp32 scores, target (B, S, F) 0/1 as uint8 or (target_is_f32) fp32, thresholds (Q)
 * fp32, 1 <= Q <= 64, 1 <= S <= 32.  perm (B, S) int32: score row perm[b][i] plays target speaker i (outside
 * 0..S-1: nobody does); NULL with S <= 4: the kernel takes the permutation with the smallest summed squared
 * error (fp64), the first in lexicographic order among equals.  Hypothesis at threshold q = score > thresholds[q]
 * (fp32 comparison).  counts (B, Q, 3) int32 = false alarm, missed detection, confusion; total (B) int32 = target
 * speech frames.  Nothing of size F * Q is allocated or written. */
int pa_der_chunks(const float* preds, const void* target, int target_is_f32, int B, int S, int F,
                  const float* thresholds, int Q, const int32_t* perm, int32_t* counts, int32_t* total,
                  void* stream);
/* bytes of the per-chunk tables (`counts` and `total` above) that a caller who only wants the batch sums
 * allocates as scratch: 4 B (3 Q + 1), whatever F is */
size_t pa_der_chunks_workspace_bytes(int B, int Q);
/* out (3 Q + 1) int64, overwritten: sums over the B chunks of counts (Q, 3), then of total */
int pa_der_chunks_sum(const int32_t* counts, const int32_t* total, int B, int Q, int64_t* out, void* stream);

/* ---- speaker-verification trials (pipelines/speaker_verification.py:858-895,
 *      torchmetrics/classification/equal_error_rate.py) ---- */

/* out[t] = scipy.spatial.distance.cdist(E[idx1[t]:idx1[t]+1], E[idx2[t]:idx2[t]+1], "cosine")[0, 0], bit for bit
 * (the arithmetic of pa_cdist_cosine_f64).  E: (N, D) float64 rows; idx1, idx2: (T) int32, each in 0..N-1 (the
 * CALLER checks the range: the kernel does not); T < 2^31; norms_scratch: N doubles. */
int pa_trial_cosine_f64(const double* E, int N, int D, const int32_t* idx1, const int32_t* idx2, long T,
                        double* out, double* norms_scratch, void* stream);

/* the sizes at which the curve kernels change path: scores per workgroup, and workgroup sums per chunk of the
 * two-level scan (a list of more than block * chunk scores fills a second chunk) */
int pa_det_block_elements(void);
int pa_det_scan_chunk(void);
/* bytes of `workspace` below for T scores (0: T outside 1..2^31-1) */
size_t pa_det_workspace_bytes(long T);
/* sklearn.metrics.roc_curve(drop_intermediate=True) + det_curve's fnr = 1 - tpr, first crossing and equal error
 * rate, in exact integers and single float64 divisions (csrc/verification.hip).
 * sorted_keys (T) float64 ASCENDING from a stable sort, labels (T) uint8 (non-zero = target trial) in the same
 * order; the curve is walked from the far end.  negate: the keys are negated distances; thresholds are negated back.
 * fps, tps: (T + 1) int32, required; thresholds, fpr, fnr: (T + 1) float64, all three or all NULL (only the
 * equal error rate is wanted).  Point 0 is (0, 0) at threshold +inf (-inf when negate).
 * status, 8 int64, overwritten: [0] non-finite keys, [1] targets P, [2] non-targets N, [3] points written,
 * [4] k = first point with fpr > fnr (-1: none), [5] the bits of the float64 eer =
 * 0.25 * (((fpr[k-1] + fpr[k]) + fnr[k-1]) + fnr[k]) (NaN without a crossing), [6] tie groups.
 * With status[0] != 0 or P == 0 or N == 0 the curve is meaningless and the caller must refuse it.
 * Several launches on `stream`, none of which waits for another workgroup; results are bit-reproducible. */
int pa_det_curve_f64(const double* sorted_keys, const uint8_t* labels, long T, int negate, int32_t* fps,
                     int32_t* tps, double* thresholds, double* fpr, double* fnr, int64_t* status, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- time-based diarization and detection error rates on segments in seconds (pyannote.metrics'
 *      DiarizationErrorRate / IdentificationErrorRate / DetectionErrorRate, restated: DESIGN.md section 21) ---- */

/* bytes of `ws` below (0: a negative count, or more cuts than the quadratic sort accepts) */
size_t pa_annot_counts_workspace_bytes(int Nr, int Nh, int Nu);
/* ref_seg (Nr, 2), hyp_seg (Nh, 2), uem_seg (Nu, 2) fp64 start / end in seconds, in any order; ref_label (Nr),
 * hyp_label (Nh) int32 in 0..Kr-1 / 0..Kh-1 (a label outside is ignored), 0 <= Kr, Kh <= 64; every N may be 0.
 * A label is on or off at a time t (overlapping tracks of one label count once).  Evaluated time = the union of
 * the uem segments, minus, when collar > 0, the intervals (t - collar/2, t + collar/2) around the start and the end
 * of every reference segment as given, minus, when skip_overlap, every instant at which two reference segments with
 * different labels are on.  With Nr(t), Nh(t) the numbers of labels on at t and all integrals over the evaluated
 * time, out, fp64, Kr*Kh + Kr + Kh + 7 values, overwritten:
 *   cooc (Kr, Kh)   seconds in which reference label i and hypothesis label j are both on
 *   ref_dur (Kr), hyp_dur (Kh)
 *   total = int Nr, false_alarm = int max(0, Nh - Nr), missed = int max(0, Nr - Nh), both = int min(Nr, Nh),
 *   ref_speech = int [Nr > 0], hyp_speech = int [Nh > 0], both_speech = int [Nr > 0 and Nh > 0]
 * Under a one-to-one mapping pi of hypothesis labels onto reference labels, correct = sum_j cooc[pi(j)][j] and
 * confusion = both - correct (the identity of pa_der_counts).  Intervals are taken exactly (no 1e-6 rule); the
 * additions have a fixed order (no floating-point atomics), so results are bit-reproducible, and exact whenever
 * every boundary is a multiple of one power of two.  The caller refuses NaN and end < start: the kernels stay in
 * bounds for them but the result is meaningless.  Four launches on `stream`; nothing is copied back. */
int pa_annot_counts(const double* ref_seg, const int32_t* ref_label, int Nr, int Kr, const double* hyp_seg,
                    const int32_t* hyp_label, int Nh, int Kh, const double* uem_seg, int Nu, double collar,
                    int skip_overlap, double* out, void* ws, size_t ws_bytes, void* stream);

/* ---- the same sums for W windows of one file in one call (the reference's SlidingDiarizationErrorRate,
 *      utils/metric.py:245-286, crops and scores every window by itself) ---- */

/* bytes of `ws` below (0: a negative count, or more cuts than the quadratic sort accepts, the 2 W window cuts
 * included) */
size_t pa_annot_window_counts_workspace_bytes(int Nr, int Nh, int Nu, int W);
/* The arrays of pa_annot_counts, and win_seg (W, 2) fp64 start / end on the device.  Windows come in any order; they
 * may overlap, touch, lie partly or wholly outside the uem, or have zero length.
 * out, (W, Kr*Kh + Kr + Kh + 7) fp64, overwritten: row w holds, in exact arithmetic, the values pa_annot_counts
 * defines for (ref, hyp, uem intersected with [win_start, win_end], collar, skip_overlap), labels indexed file-wide
 * (a label that is silent in the window has zeros).  COLLARS ARE THOSE OF THE FILE: around the reference boundaries
 * as given, not around the edges a crop of the reference to the window would create.
 * The cut list of pa_annot_counts is extended by the 2 W window boundaries (cuts only: nothing starts or ends
 * there); rank sort and interval sweep run once, window w is the rank range [rank of its start, rank of its end) of
 * the sorted intervals, and one workgroup per (window, value) sums that range in a fixed order: no floating-point
 * atomics, no workgroup waits for another, the same input gives the same bits, and inputs whose boundaries (the
 * windows' included) are multiples of one power of two give exact sums.  The sort is quadratic in
 * 2 (Nr + Nh + Nu + W) [+ 4 Nr] cuts.
 * Refused before any launch (3): a negative count, a K above 64, more cuts than the sort accepts, a workspace that
 * is too small, collar negative or NaN.  W == 0 launches nothing and returns 0.  The caller refuses NaN and
 * end < start: the kernels stay in bounds for them but the result is meaningless.  Four launches on `stream`;
 * nothing is copied back. */
int pa_annot_window_counts(const double* ref_seg, const int32_t* ref_label, int Nr, int Kr, const double* hyp_seg,
                           const int32_t* hyp_label, int Nh, int Kh, const double* uem_seg, int Nu,
                           const double* win_seg, int W, double collar, int skip_overlap, double* out, void* ws,
                           size_t ws_bytes, void* stream);

/* ---- a corpus of files at once, with the within-speaker gaps of every hypothesis filled on the device (the
 *      reference's MinDurationOffOptimizer, __main__.py:430-510, evaluates all files again for every candidate gap:
 *      the turns are uploaded once and only `fill` changes between calls) ---- */

/* The turns of F files, concatenated file after file.  Everything but the h_* tables lies on the DEVICE and is only
 * read; the h_* tables are HOST copies of the device tables of the same name, from which the call checks the sizes
 * and sizes its launches before anything runs (the caller keeps both equal: the kernels trust the device tables).
 * Offsets are int32 with F + 1 entries, offset[0] = 0, file f owns [offset[f], offset[f + 1]).
 *   ref_seg / hyp_seg / uem_seg   (N, 2) fp64 start / end, as in pa_annot_counts, in any order within a file
 *   ref_label / hyp_label         int32 label index WITHIN the file, 0..Kr[f]-1 / 0..Kh[f]-1
 *   cut_off[f + 1] - cut_off[f] = 2 (Nr + Nh + Nu) + 4 Nr of file f (its cuts with a collar and no row merged)
 *   out_off[f + 1] - out_off[f] = Kr Kh + Kr + Kh + 7 of file f
 *   run_first                     F + 1: run_first[f] = Kh[0] + .. + Kh[f - 1]; run run_first[f] + j holds the
 *                                 hypothesis rows of label j of file f; R = run_first[F]
 *   run_off                       R + 1 offsets into run_rows (a file's runs follow each other, files in order)
 *   run_rows                      per run, the indices into hyp_seg (rows of ALL files counted from 0) of its rows
 *                                 sorted by (start, end); every hypothesis row appears once */
typedef struct {
  int32_t F, R;
  const double *ref_seg, *hyp_seg, *uem_seg;
  const int32_t *ref_label, *hyp_label;
  const int32_t *ref_off, *hyp_off, *uem_off, *cut_off, *out_off;
  const int32_t *Kr, *Kh;
  const int32_t *run_first, *run_off, *run_rows;
  const int32_t *h_ref_off, *h_hyp_off, *h_uem_off, *h_Kr, *h_Kh;
} pa_annot_corpus;

/* bytes of `ws` below, from the host tables (0 for what pa_annot_corpus_counts refuses: missing host tables, more
 * than 65535 files, a K above 64, a file with more cuts than the quadratic sort accepts, R != sum of Kh) */
size_t pa_annot_corpus_workspace_bytes(const pa_annot_corpus* corpus);
/* For every file f: replace its hypothesis by `Annotation.support(fill)` of it, then the sums of pa_annot_counts.
 * support, per label, rows sorted by (start, end), with the current merged turn (a, E) and the next row (c, d), in
 * float64: lo = min(E, d); the rows MERGE (E = max(E, d)) iff lo - c > 1e-6, or g < fill with g = c - lo taken as 0
 * unless g > 1e-6; otherwise (a, E) is emitted -- if E - a > 1e-6: a shorter turn is no segment and is dropped, as
 * an Annotation drops it -- and (c, d) becomes the current turn.  (Strict: touching turns merge
 * for every fill > 0 and never for fill = 0; E is the largest end of the current turn, not of the label.)
 * merged_rows (F) int32, device, overwritten: the rows of each supported hypothesis.
 * out, device, overwritten: at out_off[f] the Kr Kh + Kr + Kh + 7 values of pa_annot_counts for file f, BIT FOR BIT
 * what pa_annot_counts writes for (the file's reference rows, its supported hypothesis rows in any order, its uem
 * rows, collar, skip_overlap): the same device functions on the same multiset of cuts.
 * fill or collar negative or NaN and everything pa_annot_corpus_workspace_bytes answers 0 for are refused before any
 * launch.  Six launches on `stream` (two when no file has a cut), none waits for another workgroup, no
 * floating-point atomics, nothing is copied back. */
int pa_annot_corpus_counts(const pa_annot_corpus* corpus, double fill, double collar, int skip_overlap, double* out,
                           int32_t* merged_rows, void* ws, size_t ws_bytes, void* stream);

/* ---- every flat cut of one dendrogram (scipy.cluster.hierarchy.fcluster(Z, t, "distance") for many t: what tuning
 *      `clustering.threshold` on a corpus asks for, __main__.py:116-283) ---- */

/* HOST function, once per dendrogram.  Z: (n - 1, 4) float64 SciPy linkage matrix in host memory, 2 <= n <= 2^30.
 * Nodes 0..n-1 are the leaves, n + i is merge i.  With MD[i] the largest height in the subtree of merge i (SciPy's
 * get_max_dist_for_each_cluster), own_md = MD for a merge and -inf for a leaf, parent_md = own_md of the parent and
 * +inf for the root, the outputs (host, written in full) list the 2n - 1 nodes by their slot on the timeline on
 * which SciPy's cluster_monocrit hands out cluster numbers -- a merge when the depth-first walk (left internal child,
 * then right internal child) enters it, a leaf when the walk leaves its parent, left leaf before right leaf:
 *   tl_own, tl_parent (2n - 1) float64;  tl_lo (2n - 1) int32 = first position of the node's leaves in left-first leaf
 *   order;  leaf_lo (n) int32 = the position of leaf l.  Every position lies in 0..n-1.
 * No recursion (a chain is n - 1 deep).  Returns 3 when Z is no tree (a child id that is no integer, out of range,
 * not yet formed or used twice). */
int pa_dendrogram_plan(const double* Z, int n, double* tl_own, double* tl_parent, int32_t* tl_lo, int32_t* leaf_lo);
/* thresholds per launch of pa_dendrogram_cuts; a longer list is cut in several launches */
int pa_dendrogram_cuts_chunk(void);
/* bytes of `ws` below: one int32 row of n positions per threshold of a launch (0: n or T out of range) */
size_t pa_dendrogram_cuts_workspace_bytes(int n, long T);
/* The four plan arrays on the DEVICE, thresholds (T) float64 on the device, none NaN (the caller checks).
 * labels (T, n) int32, row k = fcluster(Z, thresholds[k], "distance") - 1, numbering included; num_clusters (T) int32.
 * Node v starts a flat cluster iff own_md[v] <= t < parent_md[v] (float64 comparisons; a threshold of +inf counts as
 * the largest finite double, so that the root, whose parent_md is +inf, starts the one cluster); its number is the inclusive
 * prefix sum of those flags along the timeline, written at tl_lo; a second scan over the leaf positions ("last
 * non-zero wins") carries it across the node's leaves.  One workgroup per threshold, O(n) each, no atomics, no
 * workgroup waits for another; `ws` may be smaller than pa_dendrogram_cuts_workspace_bytes says (at least one row):
 * the launches then take fewer thresholds each.  Nothing is copied back. */
int pa_dendrogram_cuts(const double* tl_own, const double* tl_parent, const int32_t* tl_lo, const int32_t* leaf_lo,
                       int n, const double* thresholds, long T, int32_t* labels, int32_t* num_clusters, void* ws,
                       size_t ws_bytes, void* stream);

/* ---- KMeans (pipelines/clustering.py:483-547 and 624-645: sklearn.cluster.KMeans, dense, k-means++, lloyd) ---- */

/* the largest K and D pa_kmeans_f64 takes */
int pa_kmeans_max_clusters(void);
int pa_kmeans_max_dim(void);
/* bytes of `workspace` below (0: a size pa_kmeans_f64 refuses) */
size_t pa_kmeans_workspace_bytes(int N, int D, int K, int n_init);
/* scikit-learn 1.7.2's KMeans(n_clusters=K, init="k-means++", algorithm="lloyd") with unit sample weights on the
 * float64 rows X (N, D), for n_init initialisations at once (they are jobs of one set of launches), in float64 with a
 * fixed order of additions (no floating-point atomics, no dependence on the grid): bit-reproducible from call to call.
 * The random draws are the caller's, taken in sklearn's order from one RandomState: first (n_init) int32 = the first
 * centre's row, uniforms (n_init, K - 1, T) float64 with T = 2 + int(log(K)) = the draws of every further centre.
 * X is centred on its column means; tolv = tol * mean of the column variances.  k-means++ per centre: candidates
 * min(searchsorted(cumsum(closest), u * pot), N - 1), the one with the smallest potential (the first of equals) wins.
 * Lloyd: label = first argmin_j |C_j|^2 - 2 x.C_j; centres = member means; the centres are replaced, then: the same
 * labels as in the iteration before -> strict stop; else sum |C_new - C|^2 <= tolv -> tol stop; after a tol stop or
 * max_iter iterations the rows are assigned once more.  inertia = sum |x - C_label|^2.
 * round_iterations > 0: the iterations are enqueued that many at a time, the jobs' done flags are read back after
 * every round (one stream synchronisation each) and the loop ends once every job has stopped; <= 0: all max_iter
 * iterations are enqueued without a read-back (the workgroups of a stopped job return at entry).
 * Outputs, on the device, per initialisation: labels (n_init, N) int32; centers (n_init, K, D) float64 in the
 * caller's coordinates; inertia (n_init); picks (n_init, K) int32 = the rows k-means++ chose; status (n_init, 4) int32
 * = iterations, stop kind (0 strict, 1 tol, 2 max_iter), empty-cluster flag, non-finite flag.  A job whose cluster
 * comes up empty stops there with its flag raised (sklearn would relocate points: the caller falls back); non-finite
 * input raises the last flag of every job and nothing else is written.  With a flag set, labels, centers and inertia of
 * that job are not meaningful.  Returns 3, before any launch, for K < 2, K > pa_kmeans_max_clusters(), D outside
 * 1..pa_kmeans_max_dim(), N < K, N >= 2^24, n_init outside 1..65535, max_iter < 1 or a workspace that is too small. */
int pa_kmeans_f64(const double* X, int N, int D, int K, int n_init, const int32_t* first, const double* uniforms,
                  int max_iter, double tol, int round_iterations, int32_t* labels, double* centers, double* inertia,
                  int32_t* picks, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---- batched linear sum assignment (scipy.optimize.linear_sum_assignment; csrc/lsap.hip) ---- */

/* the largest number of rows and of columns pa_lsap_batch takes (64) */
int pa_lsap_max_size(void);
/* `batch` assignment problems in one launch, each with the result of scipy.optimize.linear_sum_assignment(problem,
 * maximize) -- the SAME optimum where there are several: the kernel does the additions, subtractions and comparisons
 * of SciPy's shortest augmenting path solver in SciPy's order (tests/lsap_model.py restates them).
 * cost: float64 on the device, element (b, r, c) at cost[b * batch_stride + r * row_stride + c * col_stride]; the
 * strides are in elements and may describe a transposed view.  rows, cols <= pa_lsap_max_size().
 * row_mask, col_mask: (batch) each on the device, or NULL = every row / column: problem b is the submatrix of the rows
 * and columns whose bits are set, in ascending order (bits at or above rows / cols are ignored).
 * col4row (batch, rows) int32: the column of every row, numbered as in `cost`; -1 for a row that is masked out, left
 * unassigned (more rows than columns) or part of a problem that was not solved.
 * total (batch), or NULL: cost[r][col4row[r]] added over the assigned rows in ascending r, starting from 0.0.
 * status (batch): 0 solved; 1 invalid entry, what SciPy refuses with "matrix contains invalid numeric entries": a NaN,
 * or -inf after the negation of `maximize`, anywhere in the problem; 2 infeasible: +inf (after the negation) forbids
 * a pair, and no complete assignment avoids those.  With a status other than 0 the problem's col4row is -1 and its
 * total 0.0.  A problem without a row or without a column is solved, with total 0.0.
 * One 64-lane workgroup per problem; no workspace, no allocation, no synchronisation; every loop of the kernel has a
 * bound known on entry.  batch == 0 returns at once.  Returns 3, before the launch, for more than 64 rows or columns. */
int pa_lsap_batch(const double* cost, long batch_stride, long row_stride, long col_stride, int batch, int rows,
                  int cols, const uint64_t* row_mask, const uint64_t* col_mask, int maximize, int32_t* col4row,
                  double* total, uint8_t* status, void* stream);
/* The cost matrices `permutate` (utils/permutation.py:99-196) hands to the solver, for y1 (batch, frames, C1) and
 * y2 (batch, frames, C2) of one dtype (float32, or float64 with is_f64) on the device, given by their element strides
 * (y2_batch_stride 0: one y2 for the whole batch): cost (batch, R, C2) float64, contiguous, R = max(C1, C2);
 * rows < C1: the mean over the frames of (y1[.., i] - y2[.., j])^2, or of the absolute difference with `mae`, computed
 * as numpy computes np.mean(.., axis=0) in the input dtype -- the frames added one after the other from frame 0, the
 * product rounded before the sum, one division by `frames` -- and converted exactly; rows >= C1 (C2 > C1 only):
 * the largest of those plus 1, both in the input dtype.  1 <= C1, C2 <= 64, frames >= 1. */
int pa_pair_costs(const void* y1, long y1_batch_stride, long y1_frame_stride, long y1_class_stride, const void* y2,
                  long y2_batch_stride, long y2_frame_stride, long y2_class_stride, int is_f64, int batch, int frames,
                  int C1, int C2, int mae, double* cost, void* stream);
/* out (batch, frames, C1), contiguous, of y2's dtype: out[b, f, i] = y2[b, f, perm[b * perm_stride + i]], 0 where that
 * entry of perm is -1 (y2 by its element strides, as above) */
int pa_permute_classes(const void* y2, long y2_batch_stride, long y2_frame_stride, long y2_class_stride, int is_f64,
                       const int32_t* perm, long perm_stride, int batch, int frames, int C1, int C2, void* out,
                       void* stream);

/* ---- open-set speaker identification against an enrolled gallery (identification.py; csrc/identify.hip, DESIGN.md
 *      section 33; no reference counterpart: the reference stops at DiarizeOutput.speaker_embeddings) ---- */

/* Everything below is float64 on the device.  The distance of two rows is scipy.spatial.distance.cdist(., ., "cosine")
 * bit for bit (the arithmetic of pa_cdist_cosine_f64), and the (rows, rows) matrix is never written: the second table is
 * walked in tiles of pa_identify_tile() rows, whose values are merged into each row's running best.  The workspace holds
 * of the two selecting calls holds the row norms of both tables and a transposed copy of the second one.
 * Order of two values wherever one is selected: np.sort's -- by value, -0.0 equal to 0.0, NaN last -- and, among equal
 * values, the lower row of the second table first (np.argsort(kind="stable")). */
int pa_identify_tile(void);      /* rows of the second table per tile (256) */
int pa_identify_max_top(void);   /* the largest K of pa_cohort_stats_f64 (512) */
int pa_identify_max_k(void);     /* the largest k of pa_gallery_topk_f64 (64) */
/* bytes of `workspace` of pa_cohort_stats_f64 (0: sizes it refuses) */
size_t pa_cohort_stats_workspace_bytes(int M, int N, int D);
/* The two statistics of adaptive score normalisation.  X (M, D), C (N, D) cohort rows.  Per row of X, with s[0..K) its K
 * smallest distances to the cohort rows in ascending order:
 *   mean[i] = (((s0 + s1) + s2) + ...) / K          stdev[i] = sqrt((((e0 + e1) + e2) + ...) / K), e = (s - mean) * (s - mean)
 * -- np.cumsum(.)[-1], not np.sum: the additions run left to right and every operation is rounded on its own.
 * 1 <= K <= min(N, pa_identify_max_top()): clipping K to the cohort is the caller's business.
 * status (M) int32: 1 for a row of X whose norm is zero or not finite, whose mean and stdev are NaN; else 0.  A cohort
 * row without a direction gives NaN distances, which sort last.  Four launches (norms, transposition, selection), no
 * synchronisation. */
int pa_cohort_stats_f64(const double* X, int M, const double* C, int N, int D, int K, double* mean, double* stdev,
                        int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
/* bytes of `workspace` of pa_gallery_topk_f64 (0: sizes it refuses) */
size_t pa_gallery_workspace_bytes(int M, int Ng, int D);
/* Q (M, D) queries, G (Ng, D) gallery.  q_mean, q_std (M) and g_mean, g_std (Ng): all NULL or all given.  The value of
 * pair (i, j) is its distance d without them and 0.5 * ((d - q_mean[i]) / q_std[i] + (d - g_mean[j]) / g_std[j]) with
 * them, in that order of operations.  Per query: values (M, k) = the k smallest values, ascending, and indices (M, k)
 * int32 = their gallery rows: np.argsort(row, kind="stable")[:k].  1 <= k <= min(Ng, pa_identify_max_k()). */
int pa_gallery_topk_f64(const double* Q, int M, const double* G, int Ng, int D, const double* q_mean,
                        const double* q_std, const double* g_mean, const double* g_std, int k, double* values,
                        int32_t* indices, void* workspace, size_t workspace_bytes, void* stream);
/* out[p] = the value of pair (iq[p], ig[p]) as pa_gallery_topk_f64 defines it, for P pairs; iq, ig (P) int32 on the
 * device.  An index outside its table gives NaN.  One thread per pair takes the two norms and the dot product: one
 * launch, no workspace. */
int pa_gallery_pairs_f64(const double* Q, int M, const double* G, int Ng, int D, const double* q_mean,
                         const double* q_std, const double* g_mean, const double* g_std, const int32_t* iq,
                         const int32_t* ig, long P, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PYANNOTE_AMD_H */
