/* pyannote_amd_online.h -- C ABI of the ONLINE (streaming) speaker-diarization step on gfx950.
 *
 * These entry points live in libpyannote_amd.so next to those of pyannote_amd.h.  They have a header and a prefix of
 * their own (`pao_`) because the main header's table of stream contracts (tests/stream_contract.py) has one row per
 * function of that header and was not to change with the change that added them; tests/test_online_contract_gpu.py
 * holds them to the same two contracts.  Folding them into pyannote_amd.h (as `pa_online_*`) together with their rows
 * of that table is left to a later change that may edit the table.
 *
 * Conventions (those of pyannote_amd.h)
 *   - every pointer is a DEVICE pointer unless its name ends in `_host`;
 *   - `stream` is a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); nothing synchronises: a call enqueues
 *     ONE kernel on `stream`, on no other stream, and returns -- so it can be captured into a graph and replayed;
 *   - no hidden allocation; neither call takes a workspace.  The bank state is in / out: its contents on entry are
 *     the state.  Outputs (`map`, `out`) may hold anything on entry and are written whole;
 *   - return 0 = OK, 1 = launch failure, 3 = invalid argument; pa_last_error() (pyannote_amd.h) has the message;
 *   - distances are fp64 with the arithmetic of pa_cdist_cosine_f64 (scipy.spatial.distance.cdist(., ., "cosine") bit
 *     for bit); everything else is integer arithmetic.
 *
 * Bank state, for N stream slots, K global speakers, D embedding dimensions, a ring of R frames:
 *   centroid_sum (N, K, D) float64   per-speaker sums of embeddings
 *   centroid_n   (N, K)    int32     number of embeddings in the sum; 0 = free
 *   acc_sum      (N, R, K) int32     ring over the global frame index g mod R: covering chunks in which k was on
 *   acc_cnt      (N, R)    int32     ring: chunks that covered the frame
 * A call touches the slots it lists and no other.  `slots` must be distinct: one workgroup owns one stream.  The
 * values that decide whether a call is valid live on the device, so a caller hands a host copy along (`*_host`); a
 * NULL host copy means the caller vouches for them (out-of-range slots are still skipped on the device).
 */
#ifndef PYANNOTE_AMD_ONLINE_H
#define PYANNOTE_AMD_ONLINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* limits of pao_cluster_step: *max_local = 4 local speakers per chunk (S), *max_speakers = 32 global speakers (K) */
int pao_cluster_step_limits(int* max_local_host, int* max_speakers_host);

/* One incremental clustering step (Coria et al., ASRU 2021) for M streams of a bank, one chunk each, in one launch.
 *   slots (M) int32 distinct, in [0, N); slots_host: the same on the host, or NULL
 *   emb (M, S, D) float32; active, clean (M, S) int32 (pa_seg_chunk_stats)
 *   -> map (M, S) int32 in [-1, K), centroid_sum / centroid_n of the listed slots updated.
 * Per stream, in this order:
 *   1. s is PRESENT iff active >= min_active_frames, its row is all finite and its fp64 norm is > 0;
 *   2. LONG iff present and clean >= min_update_frames;
 *   3. d[s][k] = cosine distance of double(emb[s]) and centroid_sum[k] for the occupied k (centroid_n > 0);
 *   4. the optimal map sends exactly min(P, K_occ) present speakers injectively to occupied centroids with the
 *      smallest total (distances added in increasing s); ties -> the lexicographically smallest (k_0 .. k_{S-1}),
 *      "unmapped" after every index.  Exhaustive, split over the workgroup: the rule is total, no host exit;
 *   5. a mapped pair with d > delta_new is un-mapped, the others are MATCHED;
 *   6. unmatched present speakers in increasing s: long and a free slot exists -> it FOUNDS the lowest free slot
 *      (sum = double(emb[s]), n = 1); otherwise it is FORCED onto the occupied centroid of smallest d[s][k] that no
 *      other speaker of the chunk holds (matched, founded, earlier forced; ties -> lower k; no update); none -> -1.
 *      A centroid founded in this step is always held by its founder, so it never takes a forced speaker;
 *   7. matched AND long speakers update: sum[k] += double(emb[s]), n[k] += 1;
 *   8. not-present speakers get -1.
 * S <= 4, K <= 32, D >= 1, else 3.  3 as well for duplicate or out-of-range slots_host. */
int pao_cluster_step(const int32_t* slots, const int32_t* slots_host, int M, int N, const float* emb,
                     const int32_t* active, const int32_t* clean, int S, int D, int K, int min_active_frames,
                     int min_update_frames, double delta_new, double* centroid_sum, int32_t* centroid_n,
                     int32_t* map, void* stream);

/* Rolling overlap-add and emission for M streams of a bank in one launch.
 *   seg (M, F, S) uint8 hard decisions; map (M, S) int32 (entries outside [0, K) count as -1)
 *   start_frame, emit_from, emit_to (M) int64; frames_host (3, M) int64 = those three rows on the host, or NULL
 *   -> out (M, E, K) uint8, acc_sum / acc_cnt of the listed slots updated.
 * For f in [0, F), g = start_frame + f, g >= emit_from (a frame below emit_from was emitted by an earlier call and
 * its ring row belongs to frame g + R now): acc_cnt[g mod R] += 1 and, for each s with map[s] >= 0 and seg[f][s],
 * acc_sum[g mod R][map[s]] += 1.  A stream with start_frame < 0 adds nothing: a flush at the end of a stream.  Then
 * out[g - emit_from][k] = (2 acc_sum > acc_cnt) for g in [emit_from, emit_to) -- a frame no chunk covered gives 0 --
 * zero rows behind, and the emitted ring rows are cleared.
 * 3 if R < F + E, S > 4, K > 32, duplicate or out-of-range slots_host, or a range of frames_host is inconsistent:
 * 0 <= emit_from <= emit_to, emit_to - emit_from <= E and, unless start_frame < 0, start_frame + F - emit_from <= R
 * (the frames not yet emitted fit the ring).  On the device an inconsistent stream gets zero rows and keeps its state. */
int pao_emit(const int32_t* slots, const int32_t* slots_host, int M, int N, const uint8_t* seg, int F, int S,
             const int32_t* map, const int64_t* start_frame, const int64_t* emit_from, const int64_t* emit_to,
             const int64_t* frames_host, int R, int K, int E, int32_t* acc_sum, int32_t* acc_cnt, uint8_t* out,
             void* stream);

#ifdef __cplusplus
}
#endif
#endif
