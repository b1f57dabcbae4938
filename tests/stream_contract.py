"""One row per stream-taking entry point of include/pyannote_amd.h (TEST INFRASTRUCTURE ONLY).

The header opens with two promises that cover the whole C ABI: "`stream` is a hipStream_t; nothing synchronises" and "no
hidden allocation".  Every function with a `void* stream` parameter is classified here:

  async   the call enqueues on `stream` and does nothing else: it can be captured into a graph on a side stream, nothing
          runs until the graph is replayed, and the replay is the whole operation (tests/test_stream_contract_gpu.py);
  waits   the function's own header comment says that it waits for the stream or reads back: it is run on a side stream
          and must give the default-stream bytes, its host-side results valid on return.

tests/test_stream_contract_cpu.py holds the table against the header: the set of row names is the set of declarations
with a `void* stream` parameter, and a `waits` row needs the words in its comment and its name in the Conventions
paragraph.  There is no escape list: every row has a case (tests/entry_cases.py)."""
import re
from collections import namedtuple
from pathlib import Path

import entry_cases as ec

HEADER = Path(__file__).resolve().parent.parent / "include" / "pyannote_amd.h"

ASYNC, WAITS = "async", "waits"

#: name: the entry point; variant: which of its cases ("" when there is one); cls: ASYNC / WAITS; build(device) -> Entry
Row = namedtuple("Row", "name variant cls build")


def _row(name, build, variant="", cls=ASYNC):
    return Row(name, variant, cls, build)


def _stage(stage):
    return lambda dev: ec.seg_stage(dev, stage)


def _conv(case_name):
    return lambda dev: ec.conv3x3_family(dev, case_name)


ROWS = [
    # ---- segmentation networks: B = 1 and 17 (a last tile of one chunk), the shared span path, the generic LSTM
    _row("pa_seg_forward", lambda d: ec.seg_forward(d, "h128", 1, ec.N1, 0, "strided"), "h128-B1"),
    _row("pa_seg_forward", lambda d: ec.seg_forward(d, "h128", 17, ec.N1, 0, "strided"), "h128-B17"),
    _row("pa_seg_forward", lambda d: ec.seg_forward(d, "h128", 17, 1600, ec.N1 - 700, "strided"), "h128-B17-span-short"),
    _row("pa_seg_forward", lambda d: ec.seg_forward(d, "generic", 17, ec.N1, 0, "strided"), "generic-B17"),
    _row("pa_seg_forward_files", ec.seg_forward_files),
    _row("pa_row_stats", _stage("row_stats")),
    _row("pa_sinc_fir_pool", _stage("sinc_fir_pool")),
    _row("pa_sinc_fir_span", _stage("sinc_fir_span")),
    _row("pa_sinc_fix_pool", _stage("sinc_fix_pool")),
    _row("pa_sinc_fir_span_centred", _stage("sinc_fir_span_centred")),
    _row("pa_sinc_fix_pool_centred", _stage("sinc_fix_pool_centred")),
    _row("pa_conv5_pool", _stage("conv5_pool")),
    _row("pa_norm_transpose", _stage("norm_transpose")),
    _row("pa_gemm_tn_ex", _stage("gemm_tn_ex")),
    _row("pa_gemm_tn", _stage("gemm_tn")),
    _row("pa_gemm_tn_s2", ec.gemm_tn_s2),
    _row("pa_lstm_rec", _stage("lstm_rec")),
    _row("pa_lstm_rec_h", ec.lstm_rec_h),
    _row("pa_classifier", _stage("classifier")),
    # ---- embedding networks
    _row("pa_emb_forward", lambda d: ec.emb_forward(d, "basic", 1, 1, 32160), "basic-B1"),
    _row("pa_emb_forward", lambda d: ec.emb_forward(d, "basic", 17, 3, 32000), "basic-B17-S3"),
    _row("pa_emb_forward", lambda d: ec.emb_forward(d, "bottleneck", 3, 3, 32160), "bottleneck-B3-S3"),
    _row("pa_emb_forward", lambda d: ec.emb_forward(d, "span39", 3, 3, 32160), "span39-B3-S3"),
    _row("pa_emb_forward_ragged", lambda d: ec.emb_forward_ragged(d, [12000, 8000, 33000])),
    _row("pa_emb_calibrate_winograd", ec.emb_calibrate_winograd),
    _row("pa_absmax_diff", ec.absmax_diff),
    _row("pa_fbank", ec.fbank),
    _row("pa_fbank_center_span", ec.fbank_center_span),
    _row("pa_resnet_stem", ec.resnet_stem),
    # the persistent convolutions: every claiming workgroup takes at least two tiles (the tile counters of the second
    # replay are those of the first), and the row-range forms on a small map
    _row("pa_conv3x3", _conv("direct_16to32_3x5_B1024"), "s1-many-tiles"),
    _row("pa_conv3x3", _conv("direct_16to64_31x3_B128_s2"), "s2-many-tiles"),
    _row("pa_conv3x3_s2_sc", ec.conv3x3_s2_sc),
    _row("pa_conv3x3_wino", _conv("wino_32to32_5x3_B1024"), "wino32-many-tiles"),
    _row("pa_conv3x3_wino", _conv("wino_16to32_4x33_B1024"), "2x2-many-tiles"),
    _row("pa_conv3x3_wino4", _conv("wino4_32to32_1x53_B2048"), "rows-many-tiles"),
    _row("pa_conv3x3_wino4", _conv("wino4_32to256_7x22_B9"), "runs"),
    _row("pa_conv3x3_wino4_rows", _conv("wino4_64to64_10x70_B3_rows8")),
    _row("pa_conv3x3_wino_rows", _conv("wino_64to64_6x40_B3_yfirst4")),
    _row("pa_stats_pool", ec.stats_pool),
    _row("pa_fbank_ragged", ec.fbank_ragged),
    _row("pa_zero_tail_cols", ec.zero_tail_cols),
    _row("pa_stats_pool_ragged", ec.stats_pool_ragged),
    # ---- SSeRiouSS
    _row("pa_sser_forward", lambda d: ec.sser_forward(d, 1), "B1"),
    _row("pa_sser_forward", lambda d: ec.sser_forward(d, 17), "B17"),
    _row("pa_w2v_conv0", ec.w2v_conv0),
    _row("pa_w2v_group_norm_gelu", ec.w2v_group_norm_gelu),
    _row("pa_w2v_layernorm", ec.w2v_layernorm),
    _row("pa_w2v_posconv", ec.w2v_posconv),
    _row("pa_w2v_softmax", ec.w2v_softmax),
    _row("pa_w2v_axpy", ec.w2v_axpy),
    _row("pa_w2v_to_tiles", ec.w2v_to_tiles),
    _row("pa_gemm_tn_batched", ec.gemm_tn_batched),
    # ---- x-vectors
    _row("pa_xvec_forward", lambda d: ec.xvec_forward(d, 1, 1), "B1"),
    _row("pa_xvec_forward", lambda d: ec.xvec_forward(d, 17, 3), "B17-S3"),
    _row("pa_xvec_mfcc_forward", lambda d: ec.xvec_mfcc_forward(d, "centred", 1, 1), "centred-B1"),
    _row("pa_xvec_mfcc_forward", lambda d: ec.xvec_mfcc_forward(d, "uncentred_hop160", 17, 3), "uncentred-B17-S3"),
    _row("pa_mfcc_features", ec.mfcc_features),
    _row("pa_stats_pool_rows", ec.stats_pool_rows),
    # ---- clustering
    _row("pa_pdist_f64", ec.pdist_f64),
    _row("pa_cdist_cosine_f64", ec.cdist_cosine_f64),
    _row("pa_centroid_means", ec.centroid_means),
    _row("pa_linkage_centroid_f64", lambda d: ec.linkage_centroid(d, 65, 0), "n65"),
    _row("pa_linkage_centroid_f64", lambda d: ec.linkage_centroid(d, 65, 13), "n65-ties-heap"),
    _row("pa_pdist_cosine_f64", ec.pdist_cosine_f64),
    _row("pa_nonfinite_flag_f64", ec.nonfinite_flag_f64),
    _row("pa_linkage_chain_f64", lambda d: ec.linkage_chain(d, 130, "single"), "n130-single"),
    _row("pa_linkage_chain_f64", lambda d: ec.linkage_chain(d, 130, "ward"), "n130-ward"),
    # ---- frame-domain stages
    _row("pa_gather_chunks", ec.gather_chunks),
    _row("pa_seg_chunk_stats", ec.seg_chunk_stats),
    _row("pa_embedding_masks", ec.embedding_masks),
    _row("pa_speaker_count", ec.speaker_count),
    _row("pa_cluster_activations", ec.cluster_activations),
    _row("pa_topk_binarize", lambda d: ec.topk_binarize(d, False)),
    _row("pa_binarize_hysteresis", ec.binarize_hysteresis),
    _row("pa_cluster_max", ec.cluster_max),
    _row("pa_topk_binarize_f32", lambda d: ec.topk_binarize(d, True)),
    _row("pa_aggregate", ec.aggregate),
    _row("pa_aggregate_files", ec.aggregate_files),
    # ---- regions: every one of these reads counts back, or hands host tables to asynchronous copies and waits
    _row("pa_binarize_regions", ec.binarize_regions, cls=WAITS),
    _row("pa_regions_sweep_count", ec.regions_sweep_count, cls=WAITS),
    _row("pa_regions_sweep_emit", ec.regions_sweep_emit, cls=WAITS),
    _row("pa_binarize_regions_files_count", ec.regions_files_count, cls=WAITS),
    _row("pa_binarize_regions_files_emit", ec.regions_files_emit, cls=WAITS),
    # ---- front door, VBx, assignment
    _row("pa_resample_poly", ec.resample_poly),
    _row("pa_plda_transform", ec.plda_transform),
    _row("pa_vbx_iteration", ec.vbx_iteration_small, "first"),          # (first = 0 reads the call before it, by contract)
    _row("pa_vbx_run_batch", lambda d: ec.vbx_run_batch(d, 130)),
    _row("pa_constrained_assign", ec.constrained_assign),
    # ---- metrics
    _row("pa_der_counts", ec.der_counts),
    _row("pa_der_chunks", ec.der_chunks),
    _row("pa_der_chunks_sum", ec.der_chunks_sum),
    _row("pa_trial_cosine_f64", ec.trial_cosine_f64),
    _row("pa_det_curve_f64", lambda d: ec.det_curve(d, "rounded", 1)),
    _row("pa_annot_counts", ec.annot_counts),
    _row("pa_annot_window_counts", ec.annot_window_counts),
    _row("pa_annot_corpus_counts", ec.annot_corpus_counts),
    _row("pa_dendrogram_cuts", ec.dendrogram_cuts),
    _row("pa_kmeans_f64", lambda d: ec.kmeans(d, "70x16-k5", 0, 40), "no-read-back"),
    _row("pa_kmeans_f64", lambda d: ec.kmeans(d, "70x16-k5", 8, 300), "rounds-of-8", cls=WAITS),
    _row("pa_lsap_batch", ec.lsap_batch),
    _row("pa_pair_costs", ec.pair_costs),
    _row("pa_permute_classes", ec.permute_classes),
    # ---- identification
    _row("pa_cohort_stats_f64", ec.cohort_stats),
    _row("pa_gallery_topk_f64", ec.gallery_topk),
    _row("pa_gallery_pairs_f64", ec.gallery_pairs),
]

#: what a `waits` function's own comment must say (lower case, white space collapsed), any one of these
WAITS_WORDS = ("waits for the stream", "wait for the stream", "read back")


def row_id(row) -> str:
    return row.name + (f"[{row.variant}]" if row.variant else "")


# ------------------------------------------------------------------------------------------------ the header, parsed
Declaration = namedtuple("Declaration", "name params comment")


def _squash(text: str) -> str:
    return re.sub(r"[\s*]+", " ", text).strip().lower()


def parse_header(text: str):
    """-> [Declaration] of every function declared in the header, each with the comment block(s) that precede it since
    the declaration before (a comment may cover several functions that follow it: `covering` below)"""
    body = text[text.index('extern "C" {'):]
    token = re.compile(r"/\*.*?\*/|typedef\s+struct[^{;]*\{.*?\}\s*\w*\s*;|enum\s*\{.*?\}\s*;|#[^\n]*|"
                       r"(?P<decl>[A-Za-z_][\w\s\*]*?\b(?P<name>pa_\w+)\s*\((?P<params>[^;{]*?)\)\s*;)", re.S)
    out, pending = [], []
    for m in token.finditer(body):
        if m.group("decl"):
            params = re.sub(r"/\*.*?\*/", " ", m.group("params"), flags=re.S)
            out.append(Declaration(m.group("name"), " ".join(params.split()), " ".join(pending)))
            pending = []
        elif m.group(0).startswith("/*"):
            pending.append(m.group(0))
    return out


def stream_taking(decls):
    return [d.name for d in decls if re.search(r"\bvoid\s*\*\s*stream\b", d.params)]


def covering_comment(decls, name: str) -> str:
    """the comment that speaks for `name`: its own, or -- for a declaration without one -- the nearest comment above it
    (one comment in front of a group of declarations covers the group)"""
    i = next(k for k, d in enumerate(decls) if d.name == name)
    while i > 0 and not decls[i].comment:
        i -= 1
    return decls[i].comment


def conventions(text: str) -> str:
    """the Conventions paragraph of the header's opening comment"""
    head = text[:text.index("#ifndef PYANNOTE_AMD_H")]
    start = head.index("Conventions")
    return head[start:head.index("Workspaces (every", start)]
