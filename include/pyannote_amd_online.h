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

/* Replay of recorded files through the rule above: J jobs in ONE launch, one workgroup per job, no host in the loop.
 * A job is a file and a threshold triple; files of a list and candidates of a tuning grid are jobs of one launch.
 * The front ends of the files are concatenated along the chunk axis:
 *   emb (num_chunks, S, D) float32; active, clean (num_chunks, S) int32; seg (num_chunks, F, S) uint8
 *   files (num_files, 4) int64: per file its chunk offset, its chunk count C, its schedule offset (in rows) and its
 *     frame total
 *   sched (num_sched, 3) int64: rows of (start_frame, emit_from, emit_to); a file owns C + 1 consecutive rows, row c
 *     for chunk c and the FLUSH row last
 *   jobs (J, 3) int32: per job its file, min_active_frames, min_update_frames; delta_new (J) float64
 *   offsets (J, 2) int64: per job its first row of `map` and its first row of `out`
 *   files_host, sched_host, jobs_host, offsets_host: the same tables on the host.  They are REQUIRED (a NULL one is
 *     refused with 3): the loop bounds come from them.  This is the one departure from "NULL = the caller vouches".
 * State, in / out, one row per JOB (not per file): centroid_sum (J, K, D) float64, centroid_n (J, K) int32,
 * acc_sum (J, R, K) int32, acc_cnt (J, R) int32.  The contents on entry are the state -- a fresh replay passes
 * zeros, a continued one what an earlier call left -- and on return they hold the final state.
 * For c = 0 .. C - 1 a job applies items 1-8 of pao_cluster_step to chunk c with its own thresholds, then the
 * overlap-add, emission and ring clearing of pao_emit with schedule row c; then pao_emit with the flush row (nothing
 * is added).  The arithmetic is that of the two calls -- the same device functions -- so the result is what they give
 * called once per chunk, bit for bit.
 *   -> map (map_rows, S) int32: rows [offset, offset + C) of a job hold the maps of its chunks
 *   -> out (out_rows, K) uint8: rows [offset, offset + frame total) of a job; row g - (emit_from of the file's first
 *      schedule row) holds frame g.
 * Every row a job owns is written whatever it held; rows no job owns are not touched.
 * 3 (nothing written) if S > 4, K > 32, D < 1, F < 1 or R < F; a NULL host table; a file whose chunks or schedule
 * rows run past num_chunks / num_sched or whose frame total exceeds INT_MAX / 32; a job whose file is outside
 * [0, num_files); a job whose rows run past map_rows / out_rows or overlap another job's; a schedule that is
 * inconsistent: every row has 0 <= emit_from <= emit_to and, unless start_frame < 0, start_frame + F - emit_from <= R;
 * each emit_from equals the previous row's emit_to; the last row has start_frame < 0; the last emit_to minus the first
 * emit_from equals the file's frame total.
 * The device checks the same conditions again: a job whose rows cannot be located (file out of range, rows past the
 * totals or under another job's) writes nothing; a job with an inconsistent schedule leaves its state alone and
 * writes zero rows and -1 maps.
 * One kernel on `stream`, no other stream, no synchronisation, no allocation on the device, no workspace: it can be
 * captured into a graph and replayed. */
int pao_replay(const float* emb, const int32_t* active, const int32_t* clean, const uint8_t* seg, int64_t num_chunks,
               int F, int S, int D, const int64_t* files, const int64_t* files_host, int num_files,
               const int64_t* sched, const int64_t* sched_host, int64_t num_sched, const int32_t* jobs,
               const int32_t* jobs_host, const double* delta_new, const int64_t* offsets,
               const int64_t* offsets_host, int J, int64_t map_rows, int64_t out_rows, int K, int R,
               double* centroid_sum, int32_t* centroid_n, int32_t* acc_sum, int32_t* acc_cnt, int32_t* map,
               uint8_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Online DETECTION (voice activity, multi-label events): csrc/online_detect.hip.  No embeddings and no clustering; the
 * arithmetic of the OFFLINE detection path carried across pushes, so that a stream's regions at full latency are bit
 * for bit those of pa_aggregate_files + pa_binarize_regions on the same samples.
 *
 * limits of pao_detect_step: *max_classes = 16 classes (K, and score columns S); *max_emit_values = the most E * K one
 * emission may hold (the workgroup keeps it in LDS) */
int pao_detect_limits(int* max_classes_host, int* max_emit_values_host);

/* One detection step of M streams of an N-slot bank in one launch, one workgroup per stream.
 *   slots (M) int32 distinct, in [0, N); slots_host: the same on the host, or NULL
 *   scores (M, F, S): float32, or with scores_uint8 the uint8 hard decisions (0 -> 0.f, anything else -> 1.f, as
 *     pa_aggregate_files reads them; with any = 1 only, else 3)
 *   any: K = 1 and the value of a frame is the maximum of its S columns, NaN if one of them is (np.max); else K = S
 *   window, warm (F) float64 on the device; epsilon, missing: as pa_aggregate
 *   start_frame, emit_from, emit_to, closing (M) int64 on the device; frames_host (4, M) int64 = those four rows on
 *     the host, or NULL.  Consistent as for pao_emit: 0 <= emit_from <= emit_to, emit_to - emit_from <= E and, unless
 *     start_frame < 0, start_frame + F - emit_from <= R; closing is 0 or 1
 *   start, duration, step: the frame grid (the time of frame g is 0.5 * (s + (s + duration)), s = start + g * step)
 *   onset_host, offset_host (K) float32, min_duration_on_host, min_duration_off_host (K) float64: host arrays, read
 *     before the call returns and handed to the kernel by value; one set for the whole bank
 * State, in / out, touched for the listed slots only; zeros are a fresh stream:
 *   acc, cnt (N, R, K) float32   ring over the global frame index g mod R: weighted sum of scores, sum of weights
 *   msk (N, R, K) uint8          ring: a chunk gave the frame a value that is not NaN
 *   on (N, K) uint8              hysteresis state behind the last emitted frame
 *   open_start (N, K) float64    where the open region started (meaningful while `on`)
 *   pend (N, K, 2) float64, has_pend (N, K) uint8   the last merged region, not final yet
 *   n_merged (N, K) int32        merged regions so far, the pending one included
 * Per stream, in this order:
 *   1. OVERLAP-ADD.  For f in [0, F), g = start_frame + f, g >= emit_from (a frame below emit_from was emitted by an
 *      earlier call), x the frame's value, m = 0 if x is NaN else 1, row g mod R of the ring:
 *        acc = (float)((double)acc + (((double)(m ? x : 0) * m) * window[f]) * warm[f])
 *        cnt = (float)((double)cnt + ((double)m * window[f]) * warm[f]),   msk = max(msk, m)
 *      -- pa_aggregate's expressions, one chunk per call in ascending chunk order.  start_frame < 0 adds nothing: a
 *      flush at the end of a stream.
 *   2. EMISSION.  For g in [emit_from, emit_to): v = acc / fmaxf(cnt, epsilon), v = missing where msk == 0;
 *      values[g - emit_from] = v and the ring row is cleared.
 *   3. HYSTERESIS on the emitted values, float32 comparisons, continuing from `on`: frame 0 of the stream finds the
 *      state inactive whatever `on` held; inactive -> active iff v > onset, active -> inactive iff v < offset (NaN
 *      changes nothing; offset > onset is legal).  active[g - emit_from] = the state behind frame g.  Going active at
 *      frame g sets open_start = t(g); going inactive at frame g closes the raw region (open_start, t(g)).
 *   4. A raw region (s, e) that closes is dropped unless e - s > 1e-6.  Otherwise, with d(a, b) = b - a if that is
 *      > 1e-6 else 0 (pyannote.core's Segment.duration): if a region is pending, min_off > 0 and d(pend.e, s) <
 *      min_off, it is merged (pend.e = e); else the pending region, if any, is FINALISED and (s, e) becomes the pending
 *      region, n_merged += 1.  Without min_off > 0 nothing ever merges and the pending region is finalised at once.
 *      A pending region is also finalised when the stream goes active at a time t with not d(pend.e, t) < min_off: no
 *      later region can merge with it.  FINALISE: the region is written to this call's list unless min_on > 0 and
 *      d(pend.s, pend.e) < min_on; its track is n_merged - 1 (its index among the merged regions, counted whether or
 *      not they were written) when min_off > 0, else 0.
 *   5. CLOSING (closing = 1, the last call of a stream).  Behind the emitted frames a region still open closes at
 *      t(emit_to - 1) by item 4, the state becomes inactive, and the pending region is finalised.
 *   -> values (M, E, K) float32, active (M, E, K) uint8: rows behind emit_to - emit_from are NaN / 0
 *   -> counts (M, K) int32, regions (M, K, cap, 2) float64, tracks (M, K, cap) int32: the regions this call finalised,
 *      in time order; rows behind a count are NaN / -1.  Every output is written whole.
 * Why the regions of a whole stream are pa_binarize_regions' on the concatenated values (T frames): items 3 - 4 are
 * its rule frame by frame -- the same comparisons, the same t(g), empty regions dropped before merging, merging before
 * the min_on deletion, tracks numbered over the merged list -- and a merged region is final exactly when no later raw
 * region can extend it, which is what the finality conditions of item 4 say.  Offline, the LAST frame is special: it
 * closes what is open and opens nothing.  Item 5 gives the same list: a region open before frame T - 1 closes at
 * t(T - 1) whether frame T - 1 switched it off (item 3 closed it there) or not (item 5 does); a region that item 3
 * opens AT frame T - 1 is closed by item 5 at its own start and dropped as empty; T = 1 is that case and T = 0 has no
 * frame, so T < 2 gives no region.
 * 3 (nothing launched, nothing written) if S or K is outside 1..16, F < 1, E < 1, R < F + E, E * K exceeds
 * pao_detect_limits, cap < E / 2 + 2 (an emission of E frames finalises at most E / 2 + 1 regions that close in it and
 * the one pending on entry), uint8 scores without `any`, a NaN threshold, duration or grid value, duplicate or
 * out-of-range slots_host, or an inconsistent entry of frames_host.  On the device a stream whose slot or frames are
 * inconsistent gets NaN values, zero states, zero counts, NaN / -1 region rows and keeps its state.
 * One kernel on `stream`, no synchronisation, no allocation, no workspace: it can be captured into a graph. */
int pao_detect_step(const int32_t* slots, const int32_t* slots_host, int M, int N, const void* scores,
                    int scores_uint8, int F, int S, int any, const double* window, const double* warm, float epsilon,
                    float missing, const int64_t* start_frame, const int64_t* emit_from, const int64_t* emit_to,
                    const int64_t* closing, const int64_t* frames_host, double start, double duration, double step,
                    const float* onset_host, const float* offset_host, const double* min_duration_on_host,
                    const double* min_duration_off_host, int R, int E, int cap, float* acc, float* cnt, uint8_t* msk,
                    uint8_t* on, double* open_start, double* pend, uint8_t* has_pend, int32_t* n_merged, float* values,
                    uint8_t* active, int32_t* counts, double* regions, int32_t* tracks, void* stream);

#ifdef __cplusplus
}
#endif
#endif
