"""Every entry point that takes a caller workspace, run on hostile workspace contents (tests/hostile_workspace.py).

The launch sequences lean on claims like "rows past a chunk hold garbage and are never read" and "written before it is
read"; DESIGN.md, "What the launch sequences assume about their workspace", walks every carve and says, block by block,
who writes first and why no uncovered element reaches an output.  The runs here confirm that table: each case calls its
entry point through the C ABI on a workspace of exactly pa_*_workspace_bytes bytes between guard blocks, filled with
0x00 (twice), 0xFF and +-1e30, and requires byte-identical outputs and untouched guards (run_under_fills).  On the
outputs of the 0xFF run it then makes the ONE value assertion the entry point's own test module makes -- the float32
oracle at north_star_ratio <= 1 for the networks, `==` against SciPy / the Python model / the exact truth for the
float64 and integer kernels -- so that a sequence that is wrong in the same way under every fill does not pass.  No
tolerance is introduced here.  The shapes are the smallest at which the padding in question exists.

The last four tests are the production form of a stale workspace: an engine that keeps its buffer runs a larger call,
then a smaller one, whose result must equal, byte for byte, that of a freshly constructed engine.

The calls themselves are built by tests/entry_cases.py, which tests/stream_contract.py shares."""
import numpy as np
import pytest
import torch

import entry_cases as ec
from conftest import north_star_ratio
from entry_cases import N1
from hostile_workspace import FILLS, HostileWorkspace, run_under_fills

pytestmark = pytest.mark.gpu


def _log(what, need):
    """the size a case ran at goes to the test's output (`pytest -rA` shows it)"""
    print(f"hostile_workspace[{what}]: workspace {int(need)} bytes")


def _fills(what, call, need, outputs, device, initial=None):
    _log(what, need)
    with torch.cuda.device(device):
        return run_under_fills(call, need, outputs, device, what, initial)


def _case(what, entry, device):
    """an entry_cases.Entry under the four fills -> the outputs of the 0xFF run"""
    return _fills(what, entry.call, entry.need, entry.outputs, device, entry.initial or None)


_wave = ec.wave


def _chunks(wav, stride, B, N):
    """the reference's chunks: zero-padded past the end of the waveform -> (B, 1, N)"""
    out = torch.zeros(B, 1, N)
    for b in range(B):
        seg = wav[b * stride:b * stride + N]
        out[b, 0, :seg.numel()] = seg
    return out


def _hard_decisions_match(ml, ref):
    """the powerset decisions, wherever the oracle's top-2 gap is above the tolerance (tests/test_seg_gpu.py)"""
    from oracle import Powerset
    top2 = ref.topk(2, dim=-1).values
    safe = (top2[..., 0] - top2[..., 1]) > 1e-4
    return torch.equal(ml[safe], Powerset(3, 2)(ref).to(torch.uint8)[safe])


# =========================================================================================== segmentation networks
@pytest.fixture(scope="module")
def seg_models(gpu_device):
    """the 4-layer H = 128 bidirectional model of tests/test_seg_gpu.py (register-resident LSTM kernel) and one whose
    LSTM takes the generic kernel: H = 64, unidirectional, a 96-wide head"""
    return ec.seg_models(gpu_device)


SEG_CASES = [
    # (model, B, chunk_stride, samples the waveform lacks at its end, workspace query)
    ("h128", 1, N1, 0, "strided"),
    ("h128", 17, N1, 0, "strided"),                      # a last tile of 1 real chunk and 15 pad slots
    ("h128", 33, N1, 0, "strided"),                      # three tiles
    ("h128", 17, 1603, 0, "strided"),                    # overlapping, no multiple of 10: the per-chunk sinc layer
    ("h128", 17, 1600, N1 - 700, "strided"),             # the shared span path; the audio ends 700 samples into chunk 16
    ("h128", 17, 1600, N1 - 700, "plain"),               # ... in the smaller workspace: falls back to the per-chunk layer
    ("generic", 17, N1, 0, "strided"),                   # k_lstm_rec_gen: one workgroup, two tiles
    ("generic", 33, N1, 0, "strided"),                   # ... its last workgroup owns a single tile
]


@pytest.mark.parametrize("name,B,stride,short,query", SEG_CASES,
                         ids=[f"{c[0]}-B{c[1]}-s{c[2]}-{c[4]}{'-short' if c[3] else ''}" for c in SEG_CASES])
def test_seg_forward(seg_models, gpu_device, name, B, stride, short, query):
    e = ec.seg_forward(gpu_device, name, B, stride, short, query)
    model, wav, F, strided, plain = (e.extra[k] for k in ("model", "wav", "F", "strided", "plain"))
    assert F == 56
    if stride == 1600:
        assert strided > plain, "the shared sinc layer asks for its span scratch"
    else:
        assert strided == plain
    assert e.need == (strided if query == "strided" else plain)
    assert e.outputs == [((B, F, 7), torch.float32), ((B, F, 3), torch.uint8)]
    logp, ml = _case(f"pa_seg_forward {name} B={B} stride={stride} {query}", e, gpu_device)
    with torch.inference_mode():
        ref = model(_chunks(wav, stride, B, N1))
    assert north_star_ratio(f"hostile_seg_{name}_B{B}_s{stride}_{query}", logp, ref) <= 1.0
    assert _hard_decisions_match(ml, ref)


def test_seg_forward_files(seg_models, gpu_device):
    """chunks_per_file = [3, 0, 1, 13] at stride 1600: a file of no chunks, a one-chunk file (the per-chunk sinc layer),
    a file that ends 900 samples before its chunks do, 17 chunks in all (a tile boundary inside the last file)"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    e = ec.seg_forward_files(gpu_device)
    model, w, stride, counts, waves, dev_waves, F = (e.extra[k] for k in ("model", "w", "stride", "counts", "waves",
                                                                           "dev_waves", "F"))
    assert (stride, counts, F) == (1600, [3, 0, 1, 13], 56)
    assert e.outputs == [((17, F, 7), torch.float32), ((17, F, 3), torch.uint8)]
    logp, ml = _case("pa_seg_forward_files [3, 0, 1, 13]", e, gpu_device)
    # the header's promise: every file's rows are, byte for byte, those of pa_seg_forward on that file alone
    alone_logp, alone_ml = [], []
    for x, c in zip(dev_waves, counts):
        if c == 0:
            continue
        one = lib.pa_seg_workspace_bytes_strided(w, c, N1, stride)

        def alone(ws, nbytes, lp, m, x=x, c=c):
            return lib.pa_seg_forward(w, ffi.ptr(x), x.numel(), stride, c, N1, lp, m, ws, nbytes, ffi.stream())

        a, b = _fills(f"pa_seg_forward alone, {c} chunks", alone, one,
                      [((c, F, 7), torch.float32), ((c, F, 3), torch.uint8)], gpu_device)
        alone_logp.append(a)
        alone_ml.append(b)
    assert torch.equal(logp.view(torch.int32), torch.cat(alone_logp).view(torch.int32))
    assert torch.equal(ml, torch.cat(alone_ml))
    with torch.inference_mode():
        ref = model(torch.cat([_chunks(x, stride, c, N1) for x, c in zip(waves, counts) if c]))
    assert north_star_ratio("hostile_seg_forward_files", logp, ref) <= 1.0
    assert _hard_decisions_match(ml, ref)


@pytest.fixture(scope="module")
def sser(gpu_device):
    """the small configuration of tests/test_sseriouss_gpu.py"""
    return ec.sser_model(gpu_device)


@pytest.mark.parametrize("B", [1, 17])
def test_sser_forward(sser, gpu_device, B):
    e = ec.sser_forward(gpu_device, B)
    model, wav, F = e.extra["model"], e.extra["wav"], e.extra["F"]
    assert model is sser[0] and e.outputs == [((B, F, 7), torch.float32), ((B, F, 3), torch.uint8)]
    logp, ml = _case(f"pa_sser_forward B={B}", e, gpu_device)
    with torch.inference_mode():
        ref = model(wav.view(B, 1, N1))
    assert north_star_ratio(f"hostile_sser_B{B}", logp, ref) <= 1.0
    assert _hard_decisions_match(ml, ref)


# ============================================================================================== embedding networks
_masks = ec.masks_01


def _masked_embeddings(oracle, chunks, masks):
    with torch.inference_mode():
        if masks is None:
            return oracle(chunks)[:, None]
        return torch.stack([oracle(chunks, weights=masks[:, s]) for s in range(masks.shape[1])], dim=1)


def _embedding_case(what, forward, workspace_bytes, engine, oracle, dim, B, S, N, device, seed):
    """one pa_*_forward of the embedding family: B chunks of N samples side by side, S masks per chunk (S = 1: none)"""
    e = ec.embedding_forward(device, forward, workspace_bytes, engine, dim, B, S, N, seed)
    wav, masks = e.extra["wav"], e.extra["masks"]
    assert e.outputs == [((B, S, dim), torch.float32)] and (masks is None) == (S == 1)
    (emb,) = _case(what, e, device)
    want = _masked_embeddings(oracle, wav.view(B, 1, N), masks)
    assert north_star_ratio("hostile_" + what.replace(" ", "_"), emb, want) <= 1.0


@pytest.fixture(scope="module")
def xvec(gpu_device):
    return ec.xvec_model(gpu_device)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("B", [1, 5, 17])
def test_xvec_forward(xvec, gpu_device, B, S):
    model, eng = xvec
    _embedding_case(f"pa_xvec_forward B={B} S={S}", "pa_xvec_forward", "pa_xvec_workspace_bytes", eng, model, 512,
                    B, S, N1, gpu_device, seed=10 * B + S)


@pytest.fixture(scope="module")
def xvec_mfcc(gpu_device):
    return ec.xvec_mfcc_models(gpu_device)


@pytest.mark.parametrize("config", ["centred", "uncentred_hop160"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("B", [1, 5, 17])
def test_xvec_mfcc_forward(xvec_mfcc, gpu_device, B, S, config):
    oracle, eng = xvec_mfcc[config]
    assert bool(eng.pack.struct.center) == (config == "centred")
    _embedding_case(f"pa_xvec_mfcc_forward {config} B={B} S={S}", "pa_xvec_mfcc_forward",
                    "pa_xvec_mfcc_workspace_bytes", eng, oracle, 512, B, S, N1, gpu_device, seed=20 * B + S)


@pytest.fixture(scope="module")
def emb_models(gpu_device):
    """ResNet34 of BasicBlocks (seeded as in tests/test_emb_gpu.py), the Bottleneck network, and the ResNet34 with
    fbank_centering_span = 0.4 s (an odd running-mean kernel of 39 frames)"""
    return ec.emb_models(gpu_device)


# 32 000 / 32 160 samples: 198 / 199 fbank frames, 2 / 3 (mod 4) -- partial F(4x4) tile rows, an odd F(2x2) column, odd
# widths into the stride-2 stages (99 / 100, 50, 25)
EMB_CASES = [(name, B, S, N) for name in ("basic", "bottleneck") for B in (1, 3) for S in (1, 3)
             for N in (32000, 32160)] + [("span39", 3, 3, 32160)]


@pytest.mark.parametrize("name,B,S,N", EMB_CASES, ids=[f"{c[0]}-B{c[1]}-S{c[2]}-N{c[3]}" for c in EMB_CASES])
def test_emb_forward(emb_models, gpu_device, name, B, S, N):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    oracle, eng = emb_models[name]
    assert lib.pa_emb_num_fbank_frames(N) == (198 if N == 32000 else 199)
    assert eng.pack.struct.fb_center_kernel == (39 if name == "span39" else 0)
    _embedding_case(f"pa_emb_forward {name} B={B} S={S} N={N}", "pa_emb_forward", "pa_emb_workspace_bytes", eng,
                    oracle, 256, B, S, N, gpu_device, seed=B + S + N)


def _five_ragged_lengths():
    """five of the lengths of tests/test_embedding_inference_gpu.py: the shortest (0.5 s), the longest (20 s) and three
    in between whose frame counts differ mod 8"""
    from test_embedding_inference_gpu import _ragged_lengths
    lengths = sorted(_ragged_lengths())
    frames = [1 + (n - 400) // 160 for n in lengths]
    picked, residues = [lengths[0], lengths[-1]], {frames[0] % 8, frames[-1] % 8}
    for n, t in zip(lengths[3:-1:3], frames[3:-1:3]):
        if t % 8 not in residues and len(picked) < 5:
            picked.append(n)
            residues.add(t % 8)
    assert len(picked) == 5 and len(residues) == 5, (picked, residues)
    return [picked[i] for i in (2, 0, 4, 1, 3)]            # (not in length order)


def test_emb_forward_ragged(emb_models, gpu_device):
    """the guards and the bit comparison that the NaN-workspace run of tests/test_embedding_inference_gpu.py lacks"""
    lengths = _five_ragged_lengths()
    e = ec.emb_forward_ragged(gpu_device, lengths)
    oracle, waves, masks = e.extra["oracle"], e.extra["waves"], e.extra["masks"]
    assert oracle is emb_models["basic"][0] and e.outputs == [((len(lengths), 256), torch.float32)]
    (emb,) = _case(f"pa_emb_forward_ragged {lengths}", e, gpu_device)
    with torch.inference_mode():
        want = torch.cat([oracle(x[None, None], weights=m[None]) for x, m in zip(waves, masks)])
    assert north_star_ratio("hostile_emb_forward_ragged", emb, want) <= 1.0


def test_emb_calibrate_winograd(emb_models, gpu_device):
    """report (zeroed by the call) and the embeddings of the direct path"""
    e = ec.emb_calibrate_winograd(gpu_device)
    oracle, wav, B, N = (e.extra[k] for k in ("oracle", "wav", "B", "N"))
    assert oracle is emb_models["basic"][0] and (B, N) == (2, 32000)
    assert e.outputs == [((2 * 128, 4), torch.float32), ((B, 256), torch.float32)]
    report, emb = _case("pa_emb_calibrate_winograd", e, gpu_device)
    with torch.inference_mode():
        want = oracle(wav.view(B, 1, N))
    assert north_star_ratio("hostile_emb_calibrate_direct_path", emb, want) <= 1.0
    # 29 of the 32 convolutions have stride 1: all carry an F(2x2) image, those of layers 2 - 4 an F(4x4) image too
    f4, f2 = report[report[:, 0] > 0], report[report[:, 2] > 0]
    assert len(f2) == 29 and 0 < len(f4) < 29 and torch.isfinite(report).all()
    assert (f4[:, 1] < f4[:, 0]).all() and (f2[:, 3] < f2[:, 2]).all()


# ============================================================================================ exact kernels: linkage
# (n, duplicated rows, PA_LINKAGE_FAST): without ties the heap-free merge on the square copy finishes (65 and 300 have
# square_ld(n) > n); with ties it hands over to the heap kernel; n = 2 is below its smallest size; n <= 1024 is one
# workgroup, no mailbox
CENTROID_CASES = [(2, 0, None), (3, 0, None), (65, 0, None), (65, 13, None), (300, 0, None), (300, 60, None),
                  (1000, 0, None), (1000, 25, None), (300, 60, "0")]


@pytest.mark.parametrize("n,dup,fast", CENTROID_CASES,
                         ids=[f"n{c[0]}-dup{c[1]}" + ("-fast0" if c[2] else "") for c in CENTROID_CASES])
def test_linkage_centroid(gpu_device, monkeypatch, n, dup, fast):
    from scipy.cluster.hierarchy import linkage
    if fast is not None:
        monkeypatch.setenv("PA_LINKAGE_FAST", fast)          # (as tests/test_pipeline_gpu.py switches it)
    e = ec.linkage_centroid(gpu_device, n, dup)              # (every call works on a fresh copy of the matrix)
    y = e.extra["y"]
    assert e.outputs == [((n - 1, 4), torch.float64)]
    (Z,) = _case(f"pa_linkage_centroid_f64 n={n} dup={dup} fast={fast}", e, gpu_device)
    got, want = Z.numpy(), linkage(y, method="centroid")
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"first differing merge {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


@pytest.mark.parametrize("method", ["single", "complete", "average", "weighted", "ward"])
@pytest.mark.parametrize("n", [2, 130])
def test_linkage_chain(gpu_device, n, method):
    from linkage_chain_model import raw_merges
    e = ec.linkage_chain(gpu_device, n, method)
    y, D = e.extra["y"], e.extra["D"]
    assert e.outputs == [((n - 1, 4), torch.float64)]
    (raw,) = _case(f"pa_linkage_chain_f64 n={n} {method}", e, gpu_device)
    got, want = raw.numpy(), raw_merges(y, n, method)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"first differing raw merge {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
    assert torch.equal(D.cpu(), torch.from_numpy(y))


# ============================================================================================= exact kernels: KMeans
@pytest.mark.parametrize("rounds,max_iter", [(8, 300), (0, 40)])
@pytest.mark.parametrize("row", ["70x16-k5", "table4"])
def test_kmeans(gpu_device, row, rounds, max_iter):
    import kmeans_model as km
    e = ec.kmeans(gpu_device, row, rounds, max_iter)
    X, n, d, k = (e.extra[name] for name in ("X", "n", "d", "k"))
    n_init = 3
    assert e.outputs == [((n_init, n), torch.int32, -77), ((n_init, k, d), torch.float64), ((n_init,), torch.float64),
                         ((n_init, k), torch.int32, -77), ((n_init, 4), torch.int32, -77)]
    labels, centers, inertia, picks, status = _case(f"pa_kmeans_f64 n={n} d={d} k={k} round_iterations={rounds}", e,
                                                    gpu_device)
    model = km.kmeans(X, k, max_iter=max_iter)
    assert np.array_equal(status.numpy(), model["status"])
    assert np.array_equal(picks.numpy(), model["picks"])
    assert np.array_equal(labels.numpy(), model["labels"])
    # centres and inertia as tests/test_kmeans_gpu.py holds them (unit-norm rows: max |X| <= 1; another order of sums)
    assert np.allclose(centers.numpy(), model["centers"], rtol=0, atol=2.0 * n * 2.0 ** -53)
    rel = np.abs(inertia.numpy() - model["inertia"]) / np.maximum(model["inertia"], 1e-300)
    assert (rel <= 4.0 * n * d * 2.0 ** -53).all()


# ========================================================================================== exact kernels: DET curve
@pytest.fixture(scope="module")
def det_cases():
    from verification_truth import B, CHUNK, scan_case, small_cases
    scan = scan_case()
    assert len(scan[1]) == B * CHUNK + 1                 # a second chunk of workgroup sums: every scan level is used
    return {"rounded": small_cases()["rounded"], "scan": scan}


@pytest.mark.parametrize("negate", [0, 1])
@pytest.mark.parametrize("name", ["rounded", "scan"])
def test_det_curve(gpu_device, det_cases, name, negate):
    from verification_truth import det_curve_truth
    e = ec.det_curve(gpu_device, name, negate)
    y_true, scores, T = e.extra["y_true"], e.extra["scores"], e.extra["T"]
    assert T == len(det_cases[name][1]) and np.array_equal(scores, det_cases[name][1])
    assert e.outputs == [((T + 1,), torch.int32, -77), ((T + 1,), torch.int32, -77), ((T + 1,), torch.float64),
                         ((T + 1,), torch.float64), ((T + 1,), torch.float64), ((8,), torch.int64, -77)]
    fps, tps, thr, fpr, fnr, status = _case(f"pa_det_curve_f64 {name} T={T} negate={negate}", e, gpu_device)
    want = det_curve_truth(y_true, scores, bool(negate))
    status = status.numpy()
    points = int(status[3])
    assert status[0] == 0 and points == len(want[0]) and int(status[4]) == want[4]
    assert np.array_equal(fpr.numpy()[:points], want[0]) and np.array_equal(fnr.numpy()[:points], want[1])
    assert np.array_equal(thr.numpy()[:points], want[2])
    assert np.array_equal(np.signbit(thr.numpy()[:points]), np.signbit(want[2]))
    assert float(status[5:6].view(np.float64)[0]) == want[3]
    assert torch.isnan(fpr[points:]).all() and (fps[points:] == -77).all()      # nothing behind the last point


# ===================================================================================== exact kernels: dendrogram cuts
def test_dendrogram_cuts(gpu_device):
    """65 leaves, more thresholds than two launches take"""
    from scipy.cluster.hierarchy import fcluster
    import pyannote_audio_amd.ffi as ffi
    e = ec.dendrogram_cuts(gpu_device, 65)
    Z, thresholds, T, n = (e.extra[k] for k in ("Z", "thresholds", "T", "n"))
    assert n == 65 and T == 2 * ffi.load().pa_dendrogram_cuts_chunk() + 3
    assert e.outputs == [((T, n), torch.int32, -77), ((T,), torch.int32, -77)]
    labels, counts = _case(f"pa_dendrogram_cuts n={n} T={T}", e, gpu_device)
    want = np.stack([fcluster(Z, t, criterion="distance") - 1 for t in thresholds])
    assert (labels.numpy() == want).all()
    assert (counts.numpy() == want.max(axis=1) + 1).all()


# ================================================================================== exact kernels: annotation counts
def test_annot_counts(gpu_device):
    from fractions import Fraction
    import annotation_metrics_truth as truth
    e = ec.annot_counts(gpu_device)
    case = e.extra["case"]
    Kr, Kh = case["Kr"], case["Kh"]
    assert e.outputs == [((Kr * Kh + Kr + Kh + 7,), torch.float64)]
    (out,) = _case("pa_annot_counts", e, gpu_device)
    assert [Fraction(v) for v in out.tolist()] == truth.flat(truth.case_truth(case))
    assert out[-7].item() > 0.0                          # `total`: something was evaluated


def test_annot_window_counts(gpu_device):
    from fractions import Fraction
    import annotation_metrics_truth as truth
    import window_counts_cases as cases
    e = ec.annot_window_counts(gpu_device)
    case, W = e.extra["case"], e.extra["W"]
    Kr, Kh = case["Kr"], case["Kh"]
    assert W == 9 and e.outputs == [((W, Kr * Kh + Kr + Kh + 7), torch.float64)]
    (out,) = _case("pa_annot_window_counts", e, gpu_device)
    for w, (row, want) in enumerate(zip(out.tolist(), cases.window_truths(case))):
        assert [Fraction(v) for v in row] == truth.flat(want), (w, case["windows"][w])
    assert out[:, -7].count_nonzero().item() >= 3


def test_annot_corpus_counts(gpu_device):
    """three files, gaps filled on the device: every file's block equals, bit for bit, the per-file path
    (host `support`, pa_annot_counts), as tests/test_corpus_counts_gpu.py holds it"""
    from test_corpus_counts_gpu import per_file
    e = ec.annot_corpus_counts(gpu_device)
    files, out_off, fill, collar, skip = (e.extra[k] for k in ("files", "out_off", "fill", "collar", "skip"))
    assert (fill, collar, skip) == (0.25, 0.25, 1) and len(files) == 3
    assert e.outputs == [((int(out_off[-1]),), torch.float64), ((len(files),), torch.int32, -77)]
    out, merged = _case("pa_annot_corpus_counts", e, gpu_device)
    out = out.numpy()
    for f, file in enumerate(files):
        want = per_file(file, fill, collar, bool(skip), gpu_device)
        flat = np.concatenate([want["cooc"].ravel(), want["ref_dur"], want["hyp_dur"],
                               [want[name] for name in ("total", "false_alarm", "missed", "both", "ref_speech",
                                                        "hyp_speech", "both_speech")]]).astype(np.float64)
        assert out[out_off[f]:out_off[f + 1]].tobytes() == flat.tobytes(), f
        assert int(merged[f]) == len(list(file["speaker_diarization"].support(fill).itertracks())), f
    assert int(merged[1]) == 30                          # (the 0.125 s gaps of file b were filled)


# ============================================================================================ exact kernels: regions
def test_binarize_regions(gpu_device):
    """T = 2001, K = 2 of tests/test_multilabel_gpu.py, with room for class 0's 1000 regions"""
    import multilabel_oracle as mo
    e = ec.binarize_regions(gpu_device)
    scores, K, FRAMES = e.extra["scores"], e.extra["K"], e.extra["FRAMES"]
    assert scores.shape == (2001, 2) and K == 2
    assert e.outputs == [((K,), torch.int32, -77), ((K, 1000, 2), torch.float64), ((K, 1000), torch.int32, -77)]
    counts, regions, tracks = _case("pa_binarize_regions T=2001 K=2", e, gpu_device)
    assert counts.tolist() == [1000, 3]
    for k in range(K):
        want, positions = mo.class_regions(scores[:, k], *FRAMES, 0.5, 0.5)
        got = regions[k, :counts[k]].numpy()
        assert np.array_equal(got.view(np.int64), np.array(want, dtype=np.float64).reshape(-1, 2).view(np.int64)), k
        assert tracks[k, :counts[k]].tolist() == [0] * len(want), k     # (no merging: every track position is 0)
    assert torch.isnan(regions[1, 3:]).all() and (tracks[1, 3:] == -77).all()


def test_regions_sweep(gpu_device):
    """one group of three lanes of one class; the counting phase answers on the host, so its fills are compared here"""
    import regions_sweep_cases as rs
    c = ec.regions_sweep_case(gpu_device)
    scores, lane_class, onset, offset, job_lane, d_on, d_off = c["case"]
    assert (c["T"], c["K"], c["L"], c["M"], c["groups"]) == (1025, 1, 3, 6, 1)
    M = c["M"]
    count = ec.regions_sweep_count(gpu_device, c)
    counted = {}
    _log("pa_regions_sweep_count", count.need)
    with torch.cuda.device(gpu_device):
        for fill in FILLS:
            ws = HostileWorkspace(count.need, gpu_device, fill)
            rc = count.call(ws.ptr, ws.nbytes)
            n_raw, launches = (a.copy() for a in count.host)
            assert rc == 0 and launches[0] == 1
            ws.check(f"pa_regions_sweep_count ({fill})")
            counted[fill] = n_raw
    assert all(np.array_equal(counted["zeros"], counted[fill]) for fill in FILLS) and counted["zeros"].min() > 0
    e = ec.regions_sweep_emit(gpu_device, c, counted["ones"])
    rows = e.extra["rows"]
    assert rows == int(counted["ones"][job_lane].sum())
    assert e.outputs == [((rows, 2), torch.float64), ((rows,), torch.int32, -77), ((M + 1,), torch.int32, -77)]
    regions, tracks, job_off = _case("pa_regions_sweep_emit", e, gpu_device)
    off = job_off.tolist()
    got = ([regions[a:b].numpy() for a, b in zip(off[:-1], off[1:])],
           [tracks[a:b].numpy() for a, b in zip(off[:-1], off[1:])])
    rs.assert_same(got, rs.truth(scores, lane_class, onset, offset, job_lane, d_on, d_off), "one group")


# ================================================================================================ exact kernels: VBx
def test_vbx_iteration(gpu_device):
    """one first = 1 iteration of the (257, 5, 129) shape of tests/vbx_truth.py through the harness (the NaN-filled
    runs of tests/test_vbx_kernels_gpu.py stay): gamma is read and updated in place.  (first = 0 is the one call that
    reads its workspace on purpose: rho and G of the first = 1 call before it, as the header says.)"""
    from test_vbx_kernels_gpu import assert_parity64
    from vbx_truth import FA_FB, VBX_SHAPES, elbo_ratio, gamma_ratio, vbx_steps
    (N, S, D), (Fa, Fb) = VBX_SHAPES[4], FA_FB[0]
    assert (N, S, D) == (257, 5, 129)
    fea, Phi, steps = vbx_steps(N, S, D, Fa, Fb, 400)
    tag, first, gamma_in, (truth_gamma, truth_elbo), (np_gamma, np_elbo) = steps[0]
    assert first == 1
    e = ec.vbx_iteration(gpu_device, N, S, D, Fa, Fb, fea, Phi, gamma_in)
    assert e.outputs == [((N, S), torch.float64), ((1,), torch.float64)] and list(e.initial) == [0]
    gamma, elbo = _case(f"pa_vbx_iteration N={N} S={S} D={D}", e, gpu_device)
    assert_parity64("hostile vbx gamma", gamma_ratio(gamma.numpy(), truth_gamma), gamma_ratio(np_gamma, truth_gamma))
    assert_parity64("hostile vbx ELBO", elbo_ratio(float(elbo[0]), truth_elbo), elbo_ratio(np_elbo, truth_elbo))


def test_vbx_run_batch(gpu_device):
    """two jobs over the same features; per job, bit for bit what the loop of pa_vbx_iteration with the convergence
    test on the host gives (tests/test_vbx_batch_gpu.py)"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    e = ec.vbx_run_batch(gpu_device, 150)
    N, S, D, iters, eps, factors, fea_d, phi_d, g0 = (e.extra[k] for k in ("N", "S", "D", "iters", "eps", "factors",
                                                                            "fea_d", "phi_d", "g0"))
    J = len(factors)
    assert (N, S, D, iters, eps, J) == (150, 4, 128, 8, 1e-4, 2)
    assert e.outputs == [((J, N * S), torch.float64), ((J, iters), torch.float64), ((J,), torch.int32, -77)]
    gamma, elbo, iterations = _case(f"pa_vbx_run_batch J={J} N={N} S={S}", e, gpu_device)
    one = lib.pa_vbx_workspace_bytes(N, S, D)
    with torch.cuda.device(gpu_device):
        for j, (Fa, Fb) in enumerate(factors):
            ws = HostileWorkspace(one, gpu_device, "ones")
            q, history = g0.clone(), []
            value = torch.zeros(1, dtype=torch.float64, device=gpu_device)
            for it in range(iters):
                ffi.check(lib.pa_vbx_iteration(ffi.ptr(fea_d), ffi.ptr(phi_d), N, S, D, Fa, Fb, int(it == 0), ffi.ptr(q),
                                               ffi.ptr(value), ws.ptr, ws.nbytes, ffi.stream()), "pa_vbx_iteration")
                history.append(float(value.item()))
                if it > 0 and history[-1] - history[-2] < eps:
                    break
            ws.check("pa_vbx_iteration loop")
            assert int(iterations[j]) == len(history), j
            assert elbo[j, :len(history)].tolist() == history, j
            assert torch.equal(gamma[j].view(torch.int64), q.cpu().view(-1).view(torch.int64)), j


# ======================================================================================================== engines
def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(a.cpu().contiguous().view(-1).view(torch.uint8), b.cpu().contiguous().view(-1).view(torch.uint8))


def test_segmentation_engine_small_call_after_a_large_one(seg_models, gpu_device):
    from pyannote_audio_amd.segmentation import SegmentationEngine
    _, pack = seg_models["h128"]
    big, small = _wave(32 * 1600 + N1, seed=1).to(gpu_device), _wave(N1 + 1600, seed=2).to(gpu_device)
    used = SegmentationEngine(pack)
    used.forward_strided(big, 1600, 33, N1)
    held = used._ws.data_ptr()
    got = used.forward_strided(small, 1600, 2, N1)
    assert used._ws.data_ptr() == held, "the engine kept its workspace: the small call ran on the large one's state"
    want = SegmentationEngine(pack).forward_strided(small, 1600, 2, N1)
    assert _same_bytes(got[0], want[0]) and _same_bytes(got[1], want[1])


def test_sseriouss_engine_small_call_after_a_large_one(sser, gpu_device):
    _, pack, Engine = sser
    g = torch.Generator().manual_seed(3)
    big = (0.1 * torch.randn(33 * N1, generator=g)).clamp(-1, 1).to(gpu_device)
    small = (0.1 * torch.randn(2 * N1, generator=g)).clamp(-1, 1).to(gpu_device)
    used = Engine(pack)
    used.forward_strided(big, N1, 33, N1)
    held = used._ws.data_ptr()
    got = used.forward_strided(small, N1, 2, N1)
    assert used._ws.data_ptr() == held
    want = Engine(pack).forward_strided(small, N1, 2, N1)
    assert _same_bytes(got[0], want[0]) and _same_bytes(got[1], want[1])


def test_embedding_engine_small_call_after_a_large_one(emb_models, gpu_device):
    from pyannote_audio_amd.embedding import EmbeddingEngine
    _, eng = emb_models["basic"]
    pack = eng.pack
    big, small = _wave(3 * 32160, seed=4).to(gpu_device), _wave(32000, seed=5).to(gpu_device)
    masks = _masks(3, 3, 115, seed=6).to(gpu_device)
    used = EmbeddingEngine(pack)
    used.forward_strided(big, 32160, 3, 32160, masks)
    held = used._ws.data_ptr()
    got = used.forward_strided(small, 32000, 1, 32000)
    assert used._ws.data_ptr() == held
    assert _same_bytes(got, EmbeddingEngine(pack).forward_strided(small, 32000, 1, 32000))


def test_xvector_engine_small_call_after_a_large_one(xvec, gpu_device):
    from pyannote_audio_amd.embedding import XVectorEngine
    _, eng = xvec
    pack = eng.pack
    big, small = _wave(17 * 32000, seed=7).to(gpu_device), _wave(N1, seed=8).to(gpu_device)
    used = XVectorEngine(pack)
    used.forward_strided(big, 32000, 17, 32000)
    held = used._ws.data_ptr()
    got = used.forward_strided(small, N1, 1, N1)
    assert used._ws.data_ptr() == held
    assert _same_bytes(got, XVectorEngine(pack).forward_strided(small, N1, 1, N1))
