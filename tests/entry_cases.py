"""Small calls of the C ABI's entry points, built once and run many times (TEST INFRASTRUCTURE ONLY).

A builder takes the device and returns an `Entry`: the call as a closure of the workspace pointer, the workspace size and
the output pointers, which reads `ffi.stream()` when it is CALLED, never when it is built; the outputs as
(shape, dtype[, untouched value]) specifications of `kernel_parity.Guarded` buffers; the bytes of workspace the matching
query asked for (None: the entry point takes none); the inputs, whose bits a call must leave alone.  Two users:

  * tests/test_hostile_workspace_gpu.py runs the workspace-taking ones under hostile workspace contents and makes its
    value assertion from `Entry.extra`;
  * tests/stream_contract.py gives every stream-taking entry point of include/pyannote_amd.h a row and
    tests/test_stream_contract_gpu.py captures, replays and side-streams each row.

Nothing here asserts a value.  Shapes are the smallest at which the launch sequence is complete: a partial last tile, more
than one tile per workgroup where a kernel is persistent, B = 1 and 17 for the forwards."""
import ctypes as C
import functools

import numpy as np
import torch

N1 = 16000            # one second: 56 SincNet frames, 49 wav2vec frames, 42 / 101 x-vector frames
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


class Entry:
    """call(ws_ptr, ws_bytes, *output_ptrs) -> return code; outputs: [(shape, dtype) or (shape, dtype, untouched)];
    need: workspace bytes or None; initial: {output index: tensor} for outputs the call reads as well; inputs: device
    tensors the call only reads; host: numpy arrays the call writes on the HOST (results of the entry points that
    wait for the stream); extra: whatever the caller's value assertion wants"""

    def __init__(self, call, outputs, need=None, initial=None, inputs=(), host=(), **extra):
        self.call, self.outputs, self.need = call, list(outputs), None if need is None else int(need)
        self.initial, self.inputs, self.host, self.extra = dict(initial or {}), list(inputs), list(host), extra


def _ffi():
    import pyannote_audio_amd.ffi as ffi
    return ffi, ffi.load()


def p(t):
    """device pointer of a tensor (None -> NULL); an int is a pointer already"""
    if t is None:
        return None
    return C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def off(ptr, nbytes):
    return C.c_void_p(int(ptr) + nbytes)


def randn(dev, *shape, seed=0, dtype=F32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g, dtype=torch.float64)).to(dtype).contiguous().to(dev)


def rand(dev, *shape, seed=0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64).to(dtype).contiguous().to(dev)


def randint(dev, lo, hi, *shape, seed=0, dtype=I32):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g).to(dtype).contiguous().to(dev)


def wave(n, seed):
    """noise + a tone + a DC offset, as the forward tests of the networks use"""
    g = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(n, generator=g) + 0.05 * torch.sin(torch.arange(n) * 0.01) + 0.02
    return x.clamp(-1, 1)


def masks_01(B, S, Fm, seed):
    """(B, S, Fm) 0 / 1 weights, one mask all zero (its embedding is the bias path)"""
    g = torch.Generator().manual_seed(seed)
    masks = (torch.rand(B, S, Fm, generator=g) < 0.6).float()
    masks[0, S - 1] = 0.0
    return masks


# =================================================================================================== the models
@functools.lru_cache(maxsize=None)
def seg_models(dev):
    """the 4-layer H = 128 bidirectional model of tests/test_seg_gpu.py (register-resident LSTM kernel) and one whose
    LSTM takes the generic kernel: H = 64, unidirectional, a 96-wide head"""
    from oracle import seeded_pyannet
    from oracle.models import PyanNet
    from pyannote_audio_amd.weights import SegmentationPack
    std = seeded_pyannet(seed=1234, num_layers=4)
    torch.manual_seed(77)
    lstm = {"hidden_size": 64, "num_layers": 2, "bidirectional": False, "monolithic": False}
    linear = {"hidden_size": 96, "num_layers": 2}
    gen = PyanNet(num_classes=7, lstm=lstm, linear=linear).eval()
    return {"h128": (std, SegmentationPack(std.state_dict(), {"lstm": {"num_layers": 4}}, 7, 3, 2, dev)),
            "generic": (gen, SegmentationPack(gen.state_dict(), {"lstm": lstm, "linear": linear}, 7, 3, 2, dev))}


@functools.lru_cache(maxsize=None)
def sser_model(dev):
    """the small configuration of tests/test_sseriouss_gpu.py"""
    from oracle import seeded_sseriouss
    from oracle.models import TINY_WAV2VEC2
    from pyannote_audio_amd.segmentation import SSeRiouSSEngine
    from pyannote_audio_amd.weights import SSeRiouSSPack
    model = seeded_sseriouss(wav2vec=dict(TINY_WAV2VEC2), num_layers=2)
    hparams = {"wav2vec": dict(TINY_WAV2VEC2), "wav2vec_layer": -1, "lstm": {"num_layers": 2}}
    return model, SSeRiouSSPack(model.state_dict(), hparams, 7, 3, 2, dev), SSeRiouSSEngine


@functools.lru_cache(maxsize=None)
def xvec_model(dev):
    from oracle import seeded_xvector
    from pyannote_audio_amd.embedding import XVectorEngine
    from pyannote_audio_amd.weights import XVectorPack
    model = seeded_xvector()
    return model, XVectorEngine(XVectorPack(model.state_dict(), {"sincnet": {"stride": 10}}, dev))


@functools.lru_cache(maxsize=None)
def xvec_mfcc_models(dev):
    import pyannote_audio_amd as pa
    import xvector_mfcc_oracle as xo
    out = {}
    for name, mfcc in (("centred", None), ("uncentred_hop160", {"melkwargs": {"center": False, "hop_length": 160}})):
        oracle = xo.seeded_xvector_mfcc(seed=3579, mfcc=mfcc)
        model = pa.XVectorMFCC(oracle.state_dict(), xo.xvector_mfcc_hparams(oracle), pa.model.embedding_specifications())
        out[name] = (oracle, model.to(dev).engine)
    return out


def bottleneck_oracle():
    """the shallow Bottleneck network of tests/test_emb_gpu.py and tests/test_embedding_inference_gpu.py"""
    from oracle.models import Bottleneck, WeSpeakerResNet34 as OracleNet
    torch.manual_seed(11)
    model = OracleNet(num_blocks=(1, 1, 1, 1), block=Bottleneck).eval()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.6, 1.2)
                m.bias.normal_(0, 0.1)
    return model


@functools.lru_cache(maxsize=None)
def emb_models(dev):
    """ResNet34 of BasicBlocks (seeded as in tests/test_emb_gpu.py), the Bottleneck network, and the ResNet34 with
    fbank_centering_span = 0.4 s (an odd running-mean kernel of 39 frames)"""
    from oracle import seeded_wespeaker
    from pyannote_audio_amd.embedding import EmbeddingEngine
    from pyannote_audio_amd.weights import EmbeddingPack
    basic, bottleneck, span = seeded_wespeaker(seed=4321), bottleneck_oracle(), seeded_wespeaker(seed=4321)
    span.fbank_centering_span = 0.4
    return {"basic": (basic, EmbeddingEngine(EmbeddingPack(basic.state_dict(), dev))),
            "bottleneck": (bottleneck, EmbeddingEngine(EmbeddingPack(bottleneck.state_dict(), dev))),
            "span39": (span, EmbeddingEngine(EmbeddingPack(span.state_dict(), dev, center_kernel=39)))}


# ====================================================================================== segmentation networks
def seg_forward(dev, name, B, stride, short, query):
    """pa_seg_forward on B chunks of one second; `short`: samples the waveform lacks at its end; `query`: which
    workspace query sizes the workspace ("strided" / "plain")"""
    ffi, lib = _ffi()
    model, pack = seg_models(dev)[name]
    w = pack.struct
    wav = wave((B - 1) * stride + N1 - short, seed=B + stride)
    wd = wav.to(dev)
    F = lib.pa_seg_num_frames(N1, 10)
    strided = lib.pa_seg_workspace_bytes_strided(w, B, N1, stride)
    plain = lib.pa_seg_workspace_bytes(w, B, N1)

    def call(ws, nbytes, logp, ml):
        return lib.pa_seg_forward(w, p(wd), wd.numel(), stride, B, N1, logp, ml, ws, nbytes, ffi.stream())

    return Entry(call, [((B, F, 7), F32), ((B, F, 3), U8)], strided if query == "strided" else plain, inputs=[wd],
                 wav=wav, model=model, F=F, strided=strided, plain=plain)


def seg_forward_files(dev):
    """chunks_per_file = [3, 0, 1, 13] at stride 1600: a file of no chunks, a one-chunk file (the per-chunk sinc layer),
    a file that ends 900 samples before its chunks do, 17 chunks in all (a tile boundary inside the last file)"""
    ffi, lib = _ffi()
    model, pack = seg_models(dev)["h128"]
    w = pack.struct
    stride, counts = 1600, [3, 0, 1, 13]
    lengths = [2 * stride + N1, 5000, N1, 12 * stride + N1 - 900]
    waves = [wave(n, seed=40 + i) for i, n in enumerate(lengths)]
    dev_waves = [x.to(dev) for x in waves]
    n, total, F = len(counts), sum(counts), 56
    ptrs = (C.c_void_p * n)(*[x.data_ptr() for x in dev_waves])
    lens = (C.c_int64 * n)(*lengths)
    cnts = (C.c_int * n)(*counts)
    need = lib.pa_seg_files_workspace_bytes(w, n, cnts, N1, stride)

    def call(ws, nbytes, logp, ml):
        return lib.pa_seg_forward_files(w, ptrs, lens, cnts, n, stride, N1, logp, ml, ws, nbytes, ffi.stream())

    return Entry(call, [((total, F, 7), F32), ((total, F, 3), U8)], need, inputs=dev_waves, waves=waves,
                 dev_waves=dev_waves, counts=counts, stride=stride, model=model, w=w, F=F)


def sser_forward(dev, B):
    ffi, lib = _ffi()
    model, pack, _ = sser_model(dev)
    w = pack.struct
    g = torch.Generator().manual_seed(B)
    wav = (0.1 * torch.randn(B * N1, generator=g)).clamp(-1, 1)
    wd = wav.to(dev)
    F = lib.pa_sser_num_frames(w, N1)
    bias = pack.relative_bias(F)
    need = lib.pa_sser_workspace_bytes(w, B, N1)

    def call(ws, nbytes, logp, ml):
        return lib.pa_sser_forward(w, p(wd), wd.numel(), N1, B, N1, p(bias), logp, ml, ws, nbytes, ffi.stream())

    return Entry(call, [((B, F, 7), F32), ((B, F, 3), U8)], need, inputs=[wd], wav=wav, model=model, F=F)


# ========================================================================================== embedding networks
def embedding_forward(dev, forward, workspace_bytes, engine, dim, B, S, N, seed):
    """one pa_*_forward of the embedding family (named by `forward` / `workspace_bytes`): B chunks of N samples side by
    side, S masks per chunk (S = 1: none)"""
    ffi, lib = _ffi()
    forward, workspace_bytes = getattr(lib, forward), getattr(lib, workspace_bytes)
    w = engine.pack.struct
    g = torch.Generator().manual_seed(seed)
    wav = (0.1 * torch.randn(B * N, generator=g) + 0.03 * torch.sin(torch.arange(B * N) * 0.02)).clamp(-1, 1)
    wd = wav.to(dev)
    Tp = engine.num_pool_frames(N)
    Fm = lib.pa_seg_num_frames(N, 10)                    # masks at the segmentation model's frame rate
    masks = masks_01(B, S, Fm, seed) if S > 1 else None
    md = masks.to(dev) if masks is not None else None
    idx = engine.nearest_index(Fm, Tp) if masks is not None else None
    need = workspace_bytes(w, B, N, S)

    def call(ws, nbytes, emb):
        return forward(w, p(wd), wd.numel(), N, B, N, p(md), S, Fm if masks is not None else 0, p(idx), emb, ws,
                       nbytes, ffi.stream())

    return Entry(call, [((B, S, dim), F32)], need, inputs=[t for t in (wd, md, idx) if t is not None], wav=wav,
                 masks=masks)


def xvec_forward(dev, B, S):
    _, eng = xvec_model(dev)
    return embedding_forward(dev, "pa_xvec_forward", "pa_xvec_workspace_bytes", eng, 512, B, S, N1, seed=10 * B + S)


def xvec_mfcc_forward(dev, config, B, S):
    _, eng = xvec_mfcc_models(dev)[config]
    return embedding_forward(dev, "pa_xvec_mfcc_forward", "pa_xvec_mfcc_workspace_bytes", eng, 512, B, S, N1,
                             seed=20 * B + S)


def emb_forward(dev, name, B, S, N):
    _, eng = emb_models(dev)[name]
    return embedding_forward(dev, "pa_emb_forward", "pa_emb_workspace_bytes", eng, 256, B, S, N, seed=B + S + N)


def emb_forward_ragged(dev, lengths):
    ffi, lib = _ffi()
    oracle, eng = emb_models(dev)["basic"]
    w = eng.pack.struct
    B, n_max = len(lengths), max(lengths)
    waves = [wave(n, seed=60 + i) for i, n in enumerate(lengths)]
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    wd = torch.cat(waves).to(dev)
    off_d = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    len_d = torch.tensor(lengths, dtype=I32, device=dev)
    g = torch.Generator().manual_seed(17)
    masks = [(torch.rand(eng.num_pool_frames(n) + 9, generator=g) < 0.7).float() for n in lengths]
    pooled = torch.ones((B, eng.num_pool_frames(n_max)), dtype=F32, device=dev)
    for b, (m, n) in enumerate(zip(masks, lengths)):
        q = eng.pool_weights(m.to(dev), n)
        pooled[b, :q.numel()] = q
    need = lib.pa_emb_ragged_workspace_bytes(w, B, n_max)

    def call(ws, nbytes, emb):
        return lib.pa_emb_forward_ragged(w, p(wd), wd.numel(), p(off_d), p(len_d), B, n_max, p(pooled), emb, ws, nbytes,
                                         ffi.stream())

    return Entry(call, [((B, 256), F32)], need, inputs=[wd, off_d, len_d, pooled], oracle=oracle, waves=waves,
                 masks=masks)


def emb_calibrate_winograd(dev):
    """report (zeroed by the call) and the embeddings of the direct path"""
    ffi, lib = _ffi()
    from pyannote_audio_amd.weights import EmbeddingPack
    oracle, _ = emb_models(dev)["basic"]
    # every Winograd image in place.  (`pack` stays in the closure: the struct holds raw pointers into its tensors.)
    pack = EmbeddingPack(oracle.state_dict(), dev, guard=False)
    w = pack.struct
    B, N = 2, 32000
    wav = wave(B * N, seed=70)
    wd = wav.to(dev)
    need = lib.pa_emb_calibrate_workspace_bytes(w, B, N)

    def call(ws, nbytes, report, emb, pack=pack):
        return lib.pa_emb_calibrate_winograd(w, p(wd), wd.numel(), N, B, N, report, emb, ws, nbytes, ffi.stream())

    return Entry(call, [((2 * 128, 4), F32), ((B, 256), F32)], need, inputs=[wd], oracle=oracle, wav=wav, B=B, N=N)


def mfcc_features(dev, B=3):
    ffi, lib = _ffi()
    _, eng = xvec_mfcc_models(dev)["centred"]
    w = eng.pack.struct
    N = N1
    T = 1 + N // w.hop_length if w.center else 1 + (N - w.n_fft) // w.hop_length
    wd = wave(B * N, seed=81).to(dev)
    need = lib.pa_xvec_mfcc_workspace_bytes(w, B, N, 1)

    def call(ws, nbytes, out):
        return lib.pa_mfcc_features(w, p(wd), wd.numel(), N, B, N, out, ws, nbytes, ffi.stream())

    return Entry(call, [((B, T, w.n_mfcc), F32)], need, inputs=[wd])


# =================================================================================================== clustering
def clustered_unit(n, d, seed, dup):
    """clustered points with duplicated rows (exact ties), as tests/test_pipeline_gpu.py builds them"""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((5, d))
    X = (centers[rng.integers(0, 5, n)] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)
    if dup:
        X[rng.integers(0, n, dup)] = X[rng.integers(0, n, dup)]
    return X / np.linalg.norm(X, axis=1, keepdims=True)


def linkage_centroid(dev, n, dup):
    """D is overwritten when the heap kernel runs: every call works on a fresh copy of the condensed matrix (the copy is
    stream-ordered work of torch on the current stream, so it is captured and replayed with the call)"""
    from scipy.spatial.distance import pdist
    ffi, lib = _ffi()
    y = pdist(clustered_unit(n, 16, seed=n + dup, dup=dup))
    cond = torch.from_numpy(y).to(dev)
    work = torch.empty_like(cond)
    need = lib.pa_linkage_workspace_bytes(n)

    def call(ws, nbytes, Z):
        work.copy_(cond)
        return lib.pa_linkage_centroid_f64(p(work), n, Z, ws, nbytes, ffi.stream())

    return Entry(call, [((n - 1, 4), F64)], need, inputs=[cond], y=y)


def linkage_chain(dev, n, method):
    from scipy.spatial.distance import pdist
    from pyannote_audio_amd import distance
    from test_linkage_methods_gpu import clustered
    ffi, lib = _ffi()
    y = pdist(clustered(n, 8, seed=n, dup=n // 6), "euclidean")
    D = torch.from_numpy(y).to(dev)
    need = lib.pa_linkage_chain_workspace_bytes(n)

    def call(ws, nbytes, raw):
        return lib.pa_linkage_chain_f64(p(D), n, distance.CHAIN_METHODS[method], raw, ws, nbytes, ffi.stream())

    return Entry(call, [((n - 1, 4), F64)], need, inputs=[D], y=y, D=D)


def kmeans(dev, row, rounds, max_iter):
    import kmeans_model as km
    import pyannote_audio_amd.distance as distance
    ffi, lib = _ffi()
    n, d, g, k, noise = (70, 16, 5, 5, 0.7) if row == "70x16-k5" else km.TABLE[4]
    n_init = 3
    X = km.data(n, d, g, noise, 0, np.float64)
    first, uniforms = distance.kmeans_draws(n, k, n_init, 42)
    Xd = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
    first_d, uniforms_d = torch.from_numpy(first).to(dev), torch.from_numpy(uniforms).to(dev)
    need = lib.pa_kmeans_workspace_bytes(n, d, k, n_init)

    def call(ws, nbytes, labels, centers, inertia, picks, status):
        return lib.pa_kmeans_f64(p(Xd), n, d, k, n_init, p(first_d), p(uniforms_d), max_iter, 1e-4, rounds, labels,
                                 centers, inertia, picks, status, ws, nbytes, ffi.stream())

    outputs = [((n_init, n), I32, -77), ((n_init, k, d), F64), ((n_init,), F64), ((n_init, k), I32, -77),
               ((n_init, 4), I32, -77)]
    return Entry(call, outputs, need, inputs=[Xd, first_d, uniforms_d], X=X, n=n, d=d, k=k)


def det_curve(dev, name, negate):
    from verification_truth import scan_case, small_cases
    ffi, lib = _ffi()
    y_true, scores = scan_case() if name == "scan" else small_cases()[name]
    T = len(scores)
    keys = torch.from_numpy(np.asarray(scores, dtype=np.float64)).to(dev)
    keys, order = torch.sort(-keys if negate else keys, stable=True)
    labels = (torch.from_numpy(np.asarray(y_true)).to(dev) != 0).to(U8)[order].contiguous()
    need = lib.pa_det_workspace_bytes(T)

    def call(ws, nbytes, fps, tps, thr, fpr, fnr, status):
        return lib.pa_det_curve_f64(p(keys), p(labels), T, negate, fps, tps, thr, fpr, fnr, status, ws, nbytes,
                                    ffi.stream())

    outputs = [((T + 1,), I32, -77), ((T + 1,), I32, -77), ((T + 1,), F64), ((T + 1,), F64), ((T + 1,), F64),
               ((8,), I64, -77)]
    return Entry(call, outputs, need, inputs=[keys, labels], y_true=y_true, scores=scores, T=T)


def dendrogram_cuts(dev, n=65):
    """65 leaves, more thresholds than two launches take"""
    from scipy.cluster.hierarchy import linkage
    from pyannote_audio_amd.clustering import Dendrogram
    from test_dendrogram_cuts_cpu import points
    from test_dendrogram_cuts_gpu import many_thresholds
    ffi, lib = _ffi()
    Z = linkage(points("random", n, seed=n), method="centroid")
    T = 2 * lib.pa_dendrogram_cuts_chunk() + 3
    thresholds = many_thresholds(Z, T, seed=9)
    plan = [torch.from_numpy(a).to(dev) for a in Dendrogram(Z).plan()]
    t_dev = torch.from_numpy(thresholds).to(dev)
    need = lib.pa_dendrogram_cuts_workspace_bytes(n, T)

    def call(ws, nbytes, labels, counts):
        return lib.pa_dendrogram_cuts(*(p(a) for a in plan), n, p(t_dev), T, labels, counts, ws, nbytes, ffi.stream())

    return Entry(call, [((T, n), I32, -77), ((T,), I32, -77)], need, inputs=plan + [t_dev], Z=Z, thresholds=thresholds,
                 T=T, n=n)


# ============================================================================================ annotation counts
def annot_arrays(case, dev):
    def f64(rows):
        return torch.tensor([[r[0], r[1]] for r in rows], dtype=F64).reshape(-1, 2).to(dev)

    def i32(rows):
        return torch.tensor([r[2] for r in rows], dtype=I32).to(dev)

    return f64(case["ref"]), i32(case["ref"]), f64(case["hyp"]), i32(case["hyp"]), f64(case["uem"])


def annot_case():
    """dyadic boundaries (exact sums), a uem of three regions, 2 reference and 4 hypothesis labels, a collar"""
    import annotation_metrics_truth as truth
    case = truth.random_dyadic_case(21, Nr=40, Nh=50, Nu=3, Kr=2, Kh=4, collar=0.25)
    assert len(case["uem"]) == 3 and case["Kh"] > case["Kr"]
    return case


def annot_counts(dev):
    ffi, lib = _ffi()
    case = annot_case()
    ref_seg, ref_lab, hyp_seg, hyp_lab, uem_seg = arrays = annot_arrays(case, dev)
    Nr, Nh, Nu, Kr, Kh = len(case["ref"]), len(case["hyp"]), len(case["uem"]), case["Kr"], case["Kh"]
    need = lib.pa_annot_counts_workspace_bytes(Nr, Nh, Nu)

    def call(ws, nbytes, out):
        return lib.pa_annot_counts(p(ref_seg), p(ref_lab), Nr, Kr, p(hyp_seg), p(hyp_lab), Nh, Kh, p(uem_seg), Nu,
                                   case["collar"], 0, out, ws, nbytes, ffi.stream())

    return Entry(call, [((Kr * Kh + Kr + Kh + 7,), F64)], need, inputs=arrays, case=case)


def annot_window_counts(dev):
    import window_counts_cases as cases
    ffi, lib = _ffi()
    case = cases.with_windows(annot_case(), cases.random_windows(5, 9))
    cases.assert_dyadic(case)
    ref_seg, ref_lab, hyp_seg, hyp_lab, uem_seg = arrays = annot_arrays(case, dev)
    win = torch.tensor(case["windows"], dtype=F64).reshape(-1, 2).to(dev)
    Nr, Nh, Nu, Kr, Kh, W = len(case["ref"]), len(case["hyp"]), len(case["uem"]), case["Kr"], case["Kh"], 9
    need = lib.pa_annot_window_counts_workspace_bytes(Nr, Nh, Nu, W)

    def call(ws, nbytes, out):
        return lib.pa_annot_window_counts(p(ref_seg), p(ref_lab), Nr, Kr, p(hyp_seg), p(hyp_lab), Nh, Kh, p(uem_seg), Nu,
                                          p(win), W, case["collar"], 0, out, ws, nbytes, ffi.stream())

    return Entry(call, [((W, Kr * Kh + Kr + Kh + 7), F64)], need, inputs=list(arrays) + [win], case=case, W=W)


def annot_corpus_counts(dev):
    """three files, gaps filled on the device"""
    import random
    import evaluation_truth as et
    from pyannote_audio_amd.evaluation import Corpus
    from test_corpus_counts_gpu import make_file, split_turns
    ffi, lib = _ffi()
    rng = random.Random(5)
    files = [make_file("a", et.random_rows(rng, 30, ["a", "b"], 40.0, True),
                       et.random_rows(rng, 40, ["x", "y", "z"], 40.0, True), uem=((0.5, 30.0), (32.0, 50.0))),
             make_file("b", split_turns(20, ["a", "b"]), split_turns(30, ["x", "y", "z", "w"], start=0.5)),
             make_file("c", et.random_rows(rng, 12, ["a"], 20.0, True), et.random_rows(rng, 25, ["x", "y"], 20.0, True))]
    corpus = Corpus(files, device=dev)
    struct, out_off = corpus._call.struct, corpus._call.out_off
    need = lib.pa_annot_corpus_workspace_bytes(C.byref(struct))
    fill, collar, skip = 0.25, 0.25, 1

    def call(ws, nbytes, out, merged, corpus=corpus):
        return lib.pa_annot_corpus_counts(C.byref(struct), fill, collar, skip, out, merged, ws, nbytes, ffi.stream())

    return Entry(call, [((int(out_off[-1]),), F64), ((len(files),), I32, -77)], need, files=files, out_off=out_off,
                 fill=fill, collar=collar, skip=skip)


# ====================================================================================================== regions
def binarize_regions(dev):
    """T = 2001, K = 2 of tests/test_multilabel_gpu.py, with room for class 0's 1000 regions"""
    from test_multilabel_gpu import FRAMES
    ffi, lib = _ffi()
    T, K, cap = 2001, 2, 1000
    scores = np.full((T, K), 0.1, dtype=np.float32)
    scores[0::2, 0] = 0.9
    for a, b in ((10, 40), (500, 520), (1500, 1990)):
        scores[a:b, 1] = 0.9
    x = torch.from_numpy(scores).to(dev)
    on, zero = np.full(K, 0.5, dtype=np.float32), np.zeros(K, dtype=np.float64)
    need = lib.pa_binarize_regions_workspace_bytes(T, K, cap)

    def call(ws, nbytes, counts, regions, tracks):
        return lib.pa_binarize_regions(p(x), T, K, on.ctypes.data, on.ctypes.data, zero.ctypes.data, zero.ctypes.data,
                                       *FRAMES, cap, counts, regions, tracks, ws, nbytes, ffi.stream())

    return Entry(call, [((K,), I32, -77), ((K, cap, 2), F64), ((K, cap), I32, -77)], need, inputs=[x], scores=scores,
                 K=K, FRAMES=FRAMES)


def regions_sweep_case(dev):
    """one group of three lanes of one class"""
    import regions_sweep_cases as rs
    ffi, lib = _ffi()
    T, K = 1025, 1
    scores, lane_class, onset, offset, job_lane, d_on, d_off = case = rs.make_case(91, T, K, 3, 0.02)
    L, M = len(lane_class), len(job_lane)
    groups = int(lib.pa_regions_sweep_groups(K, L, lane_class.ctypes.data))
    assert groups == 1 and L == 3 and M == 6
    return dict(case=case, T=T, K=K, L=L, M=M, groups=groups, x=torch.from_numpy(scores).to(dev), rs=rs)


def regions_sweep_count(dev, c=None):
    """the counting phase answers on the host: n_raw and launches are `Entry.host`"""
    ffi, lib = _ffi()
    c = c or regions_sweep_case(dev)
    scores, lane_class, onset, offset, job_lane, d_on, d_off = c["case"]
    T, K, L, groups, x = c["T"], c["K"], c["L"], c["groups"], c["x"]
    need = int(lib.pa_regions_sweep_workspace_bytes(T, groups, groups, L, 0, 0, 0))
    n_raw, launches = np.full(L, -7, dtype=np.int32), np.zeros(1, dtype=np.int32)

    def call(ws, nbytes):
        n_raw[:], launches[:] = -7, 0
        return lib.pa_regions_sweep_count(p(x), T, K, L, lane_class.ctypes.data, onset.ctypes.data, offset.ctypes.data,
                                          n_raw.ctypes.data, launches.ctypes.data, ws, nbytes, ffi.stream())

    return Entry(call, [], need, inputs=[x], host=[n_raw, launches], c=c)


def regions_sweep_emit(dev, c=None, n_raw=None):
    """`n_raw`: the counts of the counting phase (run here, on the current stream, when not given)"""
    ffi, lib = _ffi()
    from hostile_workspace import HostileWorkspace
    c = c or regions_sweep_case(dev)
    scores, lane_class, onset, offset, job_lane, d_on, d_off = c["case"]
    T, K, L, M, groups, x, rs = c["T"], c["K"], c["L"], c["M"], c["groups"], c["x"], c["rs"]
    if n_raw is None:
        count = regions_sweep_count(dev, c)
        ws = HostileWorkspace(count.need, dev, "ones")
        assert count.call(ws.ptr, ws.nbytes) == 0
        n_raw = count.host[0].copy()
    raw_rows, rows = int(n_raw.sum()), int(n_raw[job_lane].sum())
    need = int(lib.pa_regions_sweep_workspace_bytes(T, groups, groups, L, M, raw_rows, rows))
    launches = np.zeros(1, dtype=np.int32)

    def call(ws, nbytes, regions, tracks, job_off):
        launches[:] = 0
        return lib.pa_regions_sweep_emit(p(x), T, K, L, lane_class.ctypes.data, onset.ctypes.data, offset.ctypes.data,
                                         n_raw.ctypes.data, M, job_lane.ctypes.data, d_on.ctypes.data, d_off.ctypes.data,
                                         *rs.FRAMES, rows, regions, tracks, job_off, launches.ctypes.data, ws, nbytes,
                                         ffi.stream())

    return Entry(call, [((rows, 2), F64), ((rows,), I32, -77), ((M + 1,), I32, -77)], need, inputs=[x],
                 host=[launches], c=c, rows=rows)


def regions_files_case(dev):
    """three files of 76, 0 and 96 frames in rows that are multiples of 64, two classes"""
    import multilabel_oracle as mo
    from detection_batch_cases import FRAMES
    K, row0, T = 2, np.array([0, 128, 128, 256], dtype=np.int32), np.array([76, 0, 96], dtype=np.int32)
    rng = np.random.default_rng(55)
    scores = np.full((256, K), np.nan, dtype=np.float32)
    for f in (0, 2):
        scores[row0[f]:row0[f] + T[f]] = mo.smooth_scores(rng, int(T[f]), K, width=3)
    onset, offset = np.array([0.55, 0.5], dtype=np.float32), np.array([0.45, 0.5], dtype=np.float32)
    d_on, d_off = np.array([0.02, 0.0]), np.array([0.03, 0.0])
    return dict(K=K, row0=row0, T=T, x=torch.from_numpy(scores).to(dev), onset=onset, offset=offset, d_on=d_on,
                d_off=d_off, FRAMES=FRAMES)


def regions_files_count(dev, c=None):
    ffi, lib = _ffi()
    c = c or regions_files_case(dev)
    K, row0, T, x, onset, offset = c["K"], c["row0"], c["T"], c["x"], c["onset"], c["offset"]
    need = lib.pa_binarize_regions_files_workspace_bytes(int(row0[-1]), K, len(T), 0)
    n_raw = np.full(K, -7, dtype=np.int32)

    def call(ws, nbytes):
        n_raw[:] = -7
        return lib.pa_binarize_regions_files_count(p(x), K, len(T), row0.ctypes.data, T.ctypes.data, onset.ctypes.data,
                                                   offset.ctypes.data, n_raw.ctypes.data, ws, nbytes, ffi.stream())

    return Entry(call, [], need, inputs=[x], host=[n_raw], c=c)


def regions_files_emit(dev):
    ffi, lib = _ffi()
    from hostile_workspace import HostileWorkspace
    c = regions_files_case(dev)
    K, row0, T, x, onset, offset = c["K"], c["row0"], c["T"], c["x"], c["onset"], c["offset"]
    count = regions_files_count(dev, c)
    ws = HostileWorkspace(count.need, dev, "ones")
    assert count.call(ws.ptr, ws.nbytes) == 0
    n_raw = count.host[0].copy()
    assert n_raw.min() >= 0 and n_raw.sum() > 0
    rows_out, lists = int(n_raw.sum()), len(T) * K
    need = lib.pa_binarize_regions_files_workspace_bytes(int(row0[-1]), K, len(T), rows_out)

    def call(ws, nbytes, regions, tracks, list_off):
        return lib.pa_binarize_regions_files_emit(p(x), K, len(T), row0.ctypes.data, T.ctypes.data, onset.ctypes.data,
                                                  offset.ctypes.data, c["d_on"].ctypes.data, c["d_off"].ctypes.data,
                                                  *c["FRAMES"], n_raw.ctypes.data, rows_out, regions, tracks, list_off,
                                                  ws, nbytes, ffi.stream())

    return Entry(call, [((rows_out, 2), F64), ((rows_out,), I32, -77), ((lists + 1,), I32, -77)], need, inputs=[x])


# ========================================================================================================== VBx
def vbx_iteration(dev, N, S, D, Fa, Fb, fea, Phi, gamma_in):
    """one first = 1 iteration: gamma is read and updated in place"""
    ffi, lib = _ffi()
    fea_d, phi_d = torch.from_numpy(np.ascontiguousarray(fea)).to(dev), torch.from_numpy(Phi.copy()).to(dev)
    need = lib.pa_vbx_workspace_bytes(N, S, D)

    def call(ws, nbytes, gamma, elbo):
        return lib.pa_vbx_iteration(p(fea_d), p(phi_d), N, S, D, float(Fa), float(Fb), 1, gamma, elbo, ws, nbytes,
                                    ffi.stream())

    return Entry(call, [((N, S), F64), ((1,), F64)], need, inputs=[fea_d, phi_d],
                 initial={0: torch.from_numpy(np.ascontiguousarray(gamma_in, dtype=np.float64))})


def vbx_iteration_small(dev):
    from vbx_truth import vbx_inputs
    N, S, D = 130, 4, 128
    fea, Phi, gamma0 = vbx_inputs(N, S, D, seed=3)
    return vbx_iteration(dev, N, S, D, 0.07, 0.8, fea, Phi, gamma0)


def vbx_run_batch(dev, N=150):
    """two jobs over the same features"""
    from vbx_truth import vbx_inputs
    ffi, lib = _ffi()
    S, D, iters, eps = 4, 128, 8, 1e-4
    fea, Phi, gamma0 = vbx_inputs(N, S, D, seed=3)
    factors = [(0.07, 0.8), (0.4, 0.05)]
    J = len(factors)
    fea_d, phi_d = torch.from_numpy(np.ascontiguousarray(fea)).to(dev), torch.from_numpy(Phi.copy()).to(dev)
    g0 = torch.from_numpy(np.ascontiguousarray(gamma0, dtype=np.float64)).to(dev)
    job_init = torch.tensor([[0, S]] * J, dtype=I64, device=dev)
    job_f = torch.tensor(factors, dtype=F64, device=dev)
    need = lib.pa_vbx_batch_workspace_bytes(J, N, S, D)

    def call(ws, nbytes, gamma, elbo, iterations):
        return lib.pa_vbx_run_batch(p(fea_d), p(phi_d), N, D, J, p(g0), g0.numel(), p(job_init), p(job_f), S, iters, eps,
                                    gamma, elbo, iterations, ws, nbytes, ffi.stream())

    return Entry(call, [((J, N * S), F64), ((J, iters), F64), ((J,), I32, -77)], need,
                 inputs=[fea_d, phi_d, g0, job_init, job_f], N=N, S=S, D=D, iters=iters, eps=eps, factors=factors,
                 fea_d=fea_d, phi_d=phi_d, g0=g0)


# =========================================================================== entry points WITHOUT a workspace
def _plain(fn):
    """call(*outs) of an entry point without a workspace -> the Entry call signature"""
    return lambda ws, nbytes, *outs: fn(*outs)


@functools.lru_cache(maxsize=None)
def seg_chain(dev):
    """The building blocks of pa_seg_forward on B = 17 chunks of one second (two tiles, the second with one chunk), each
    stage fed by the stage before it: the functions are only meaningful in sequence.  Run once, on the current stream,
    when the first row asks for it; the rows then call ONE stage each on these operands."""
    ffi, lib = _ffi()
    _, pack = seg_models(dev)["h128"]
    w = pack.struct
    B, N, step = 17, N1, 1600
    ntiles = (B + 15) // 16
    P1 = ((N - 251) // 10 + 1) // 3
    P2 = (P1 - 4) // 3
    T = (P2 - 4) // 3
    M = ntiles * T * 16
    z = lambda *s: torch.zeros(*s, dtype=F32, device=dev)
    c = dict(w=w, pack=pack, B=B, N=N, step=step, ntiles=ntiles, P1=P1, P2=P2, T=T, M=M)
    c["wav"] = wave(B * N, seed=5).to(dev)
    c["mean"], c["rstd"] = z(B), z(B)
    c["s1"], c["m1"], c["r1"] = z(B, 80, P1), z(B * 80), z(B * 80)
    c["s2"], c["m2"], c["r2"] = z(B, 60, P2), z(B * 60), z(B * 60)
    c["s3"], c["m3"], c["r3"] = z(B, 60, T), z(B * 60), z(B * 60)
    c["X0"], c["xproj"], c["h"] = z(M, 64), z(M * 1024), z(M, 256)
    # overlapping chunks: the shared span
    span = (B - 1) * step + N
    c["span"], c["Pc"] = span, (span - 251) // 10 + 1
    c["wav_span"] = wave(span - 700, seed=6).to(dev)                    # the audio ends 700 samples into the last chunk
    c["mean_s"], c["rstd_s"] = z(B), z(B)
    c["S"], c["Sc"] = z(80, c["Pc"]), z(80, c["Pc"])
    c["lin_w"], c["lin_b"], c["res"] = randn(dev, 128, 256, seed=1, scale=0.06), randn(dev, 128, seed=2), \
        randn(dev, M, 128, seed=3)
    c["cls_x"] = randn(dev, M, 128, seed=4)
    c["cls_w"], c["cls_b"] = randn(dev, 7, 128, seed=5, scale=0.2), randn(dev, 7, seed=6)
    c["calls"] = calls = {}
    st = ffi.stream
    calls["row_stats"] = lambda mean, rstd: lib.pa_row_stats(p(c["wav"]), N, c["wav"].numel(), B, N, 1e-5, mean, rstd, st())
    calls["sinc_fir_pool"] = lambda out: lib.pa_sinc_fir_pool(p(c["wav"]), c["wav"].numel(), N, B, N, 10, p(c["mean"]),
                                                              p(c["rstd"]), w.wav_gamma, w.wav_beta, w.sinc_filt, out, st())
    calls["conv5_pool"] = lambda out: lib.pa_conv5_pool(p(c["s1"]), B, 80, P1, p(c["m1"]), p(c["r1"]), w.norm0,
                                                        off(w.norm0, 80 * 4), w.conv1_w, w.conv1_b, out, st())
    conv2 = lambda out: lib.pa_conv5_pool(p(c["s2"]), B, 60, P2, p(c["m2"]), p(c["r2"]), w.norm1, off(w.norm1, 60 * 4),
                                          w.conv2_w, w.conv2_b, out, st())
    calls["norm_transpose"] = lambda out: lib.pa_norm_transpose(p(c["s3"]), B, T, p(c["m3"]), p(c["r3"]), w.norm2,
                                                                off(w.norm2, 60 * 4), out, st())
    calls["gemm_tn"] = lambda out: lib.pa_gemm_tn(p(c["X0"]), 64, w.lstm_wih[0], 64, w.lstm_bias[0], out, 0, M, 1024, 64,
                                                  0, 1, st())
    calls["lstm_rec"] = lambda out: lib.pa_lstm_rec(p(c["xproj"]), w.lstm_whh[0], out, ntiles, 2, T, st())
    calls["gemm_tn_ex"] = lambda out: lib.pa_gemm_tn_ex(p(c["h"]), 256, p(c["lin_w"]), 256, p(c["lin_b"]), p(c["res"]),
                                                        out, 128, M, 128, 256, 2, 0, st())
    calls["classifier"] = lambda logp, ml: lib.pa_classifier(p(c["cls_x"]), 128, 128, ntiles, T, B, p(c["cls_w"]),
                                                             p(c["cls_b"]), 7, w.powerset_map, 3, logp, ml, st())
    stats_s = lambda mean, rstd: lib.pa_row_stats(p(c["wav_span"]), step, c["wav_span"].numel(), B, N, 1e-5, mean, rstd, st())
    calls["sinc_fir_span"] = lambda S: lib.pa_sinc_fir_span(p(c["wav_span"]), c["wav_span"].numel(), span, w.sinc_filt, S,
                                                            st())
    calls["sinc_fix_pool"] = lambda taps, out: lib.pa_sinc_fix_pool(
        p(c["S"]), c["Pc"], step // 10, B, P1, p(c["mean_s"]), p(c["rstd_s"]), w.wav_gamma, w.wav_beta, w.sinc_filt, taps,
        out, st())
    calls["sinc_fir_span_centred"] = lambda S: lib.pa_sinc_fir_span_centred(
        p(c["wav_span"]), c["wav_span"].numel(), span, p(c["mean_s"]), p(c["rstd_s"]), w.sinc_filt, S, st())
    calls["sinc_fix_pool_centred"] = lambda taps, out: lib.pa_sinc_fix_pool_centred(
        p(c["Sc"]), c["Pc"], step // 10, B, P1, p(c["wav_span"]), c["wav_span"].numel(), N, p(c["mean_s"]),
        p(c["rstd_s"]), w.wav_gamma, w.wav_beta, w.sinc_filt, taps, out, st())
    rs = lambda x, rows, n, m, r: lib.pa_row_stats(p(x), n, x.numel(), rows, n, 1e-5, p(m), p(r), st())
    for rc in (calls["row_stats"](p(c["mean"]), p(c["rstd"])), calls["sinc_fir_pool"](p(c["s1"])),
               rs(c["s1"], B * 80, P1, c["m1"], c["r1"]), calls["conv5_pool"](p(c["s2"])),
               rs(c["s2"], B * 60, P2, c["m2"], c["r2"]), conv2(p(c["s3"])), rs(c["s3"], B * 60, T, c["m3"], c["r3"]),
               calls["norm_transpose"](p(c["X0"])), calls["gemm_tn"](p(c["xproj"])), calls["lstm_rec"](p(c["h"])),
               stats_s(p(c["mean_s"]), p(c["rstd_s"])), calls["sinc_fir_span"](p(c["S"])),
               calls["sinc_fir_span_centred"](p(c["Sc"]))):
        ffi.check(rc, "seg_chain")
    torch.cuda.synchronize()
    return c


def seg_stage(dev, stage):
    c = seg_chain(dev)
    B, P1, P2, T, M, Pc = c["B"], c["P1"], c["P2"], c["T"], c["M"], c["Pc"]
    outputs = {"row_stats": [((B,), F32), ((B,), F32)], "sinc_fir_pool": [((B, 80, P1), F32)],
               "conv5_pool": [((B, 60, P2), F32)], "norm_transpose": [((M, 64), F32)], "gemm_tn": [((M * 1024,), F32)],
               "lstm_rec": [((M, 256), F32)], "gemm_tn_ex": [((M, 128), F32)],
               "classifier": [((B, T, 7), F32), ((B, T, 3), U8)], "sinc_fir_span": [((80, Pc), F32)],
               "sinc_fix_pool": [((80,), F32), ((B, 80, P1), F32)], "sinc_fir_span_centred": [((80, Pc), F32)],
               "sinc_fix_pool_centred": [((80,), F32), ((B, 80, P1), F32)]}[stage]
    inputs = [v for v in c.values() if isinstance(v, torch.Tensor)]
    return Entry(_plain(c["calls"][stage]), outputs, inputs=inputs, chain=c)


def lstm_rec_h(dev):
    """the generic recurrence: H = 64, one direction, two tiles"""
    ffi, lib = _ffi()
    H, ndir, ntiles, T = 64, 1, 2, 9
    xproj = randn(dev, ntiles, T, ndir * 4 * H, 16, seed=11)
    whh = randn(dev, ndir * 4 * H * H, seed=12, scale=0.1)
    call = lambda out: lib.pa_lstm_rec_h(p(xproj), p(whh), out, ntiles, ndir, T, H, ffi.stream())
    return Entry(_plain(call), [((ntiles * T * 16, ndir * H), F32)], inputs=[xproj, whh])


def gemm_tn_s2(dev):
    ffi, lib = _ffi()
    B, H, W, cin, N = 2, 9, 7, 32, 64
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    X, Wt, bias = randn(dev, B, H, W, cin, seed=13), randn(dev, N, cin, seed=14, scale=0.2), randn(dev, N, seed=15)
    call = lambda out: lib.pa_gemm_tn_s2(p(X), B, H, W, cin, p(Wt), cin, p(bias), out, N, N, ffi.stream())
    return Entry(_plain(call), [((B * Ho * Wo, N), F32)], inputs=[X, Wt, bias])


def gemm_tn_batched(dev):
    ffi, lib = _ffi()
    M, N, K, outer, inner = 40, 48, 64, 2, 3
    A, W, bias = randn(dev, outer, inner, M, K, seed=16), randn(dev, outer, inner, N, K, seed=17, scale=0.1), \
        randn(dev, N, seed=18)
    call = lambda out: lib.pa_gemm_tn_batched(p(A), K, inner * M * K, M * K, p(W), K, inner * N * K, N * K, p(bias), out, N,
                                              inner * M * N, M * N, M, N, K, outer, inner, 3, ffi.stream())
    return Entry(_plain(call), [((outer, inner, M, N), F32)], inputs=[A, W, bias])


# ---- embedding pieces
def _fb(dev):
    return emb_models(dev)["basic"][1].pack.struct


def absmax_diff(dev):
    ffi, lib = _ffi()
    n = 5000
    got, ref = randn(dev, n, seed=20), randn(dev, n, seed=21)
    call = lambda out2: lib.pa_absmax_diff(p(got), p(ref), n, out2, ffi.stream())
    return Entry(_plain(call), [((2,), F32)], inputs=[got, ref], initial={0: torch.zeros(2)})


def fbank(dev):
    ffi, lib = _ffi()
    w, B, N = _fb(dev), 3, 4000
    T = lib.pa_emb_num_fbank_frames(N)
    wd = wave(B * N - 300, seed=22).to(dev)
    call = lambda out: lib.pa_fbank(p(wd), wd.numel(), N, B, N, w.fb_window, w.fb_tw256, w.fb_tw512, w.fb_mel_w,
                                    w.fb_mel_lo, w.fb_mel_hi, 80, out, 1, ffi.stream())
    return Entry(_plain(call), [((B, T, 80), F32)], inputs=[wd])


def fbank_center_span(dev):
    ffi, lib = _ffi()
    B, T, nmel, K = 3, 50, 80, 39
    fb = randn(dev, B, T, nmel, seed=23)
    call = lambda out: lib.pa_fbank_center_span(p(fb), B, T, nmel, K, out, ffi.stream())
    return Entry(_plain(call), [((B, T, nmel), F32)], inputs=[fb])


def resnet_stem(dev):
    ffi, lib = _ffi()
    B, T, Fb = 2, 37, 80
    fb, w9, shift = randn(dev, B, T, Fb, seed=24), randn(dev, 9, 32, seed=25, scale=0.3), randn(dev, 32, seed=26)
    call = lambda out: lib.pa_resnet_stem(p(fb), B, T, Fb, p(w9), p(shift), out, ffi.stream())
    return Entry(_plain(call), [((B, Fb, T, 32), F32)], inputs=[fb, w9, shift])


def conv3x3_family(dev, name):
    """a case of tests/conv_truth.py by name, with its float inputs, a residual and ReLU, through the entry point the
    case is for.  The `many` cases: every claiming workgroup takes at least two tiles."""
    import conv_truth as T
    from pyannote_audio_amd.weights import winograd4_pack, winograd4_weights, winograd_pack, winograd_weights
    ffi, lib = _ffi()
    case = next(c for c in T.CASES if c["name"] == name)
    x, w, shift, R = T.float_inputs(case, T.float_seed(case))
    image = T.direct_image(w) if case["algo"] == "direct" else \
        winograd_pack(winograd_weights(w)) if case["algo"] == "wino" else winograd4_pack(winograd4_weights(w))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev)
    xd, wd, shd, rd = nhwc(x), image.contiguous().to(dev), shift.to(dev), nhwc(R)
    Ho, Wo = T.out_hw(case["H"], case["W"], case["stride"])
    head = (p(xd), case["B"], case["H"], case["W"], case["cin"], p(wd), p(shd), p(rd))

    def call(out):
        if case["algo"] == "direct":
            return lib.pa_conv3x3(*head, out, case["cout"], case["stride"], 1, ffi.stream())
        if case["algo"] == "wino":
            if case["y_first"] == 0:
                return lib.pa_conv3x3_wino(*head, out, case["cout"], 1, ffi.stream())
            return lib.pa_conv3x3_wino_rows(*head, out, case["cout"], 1, case["y_first"], ffi.stream())
        if case["rows"] == case["H"]:
            return lib.pa_conv3x3_wino4(*head, out, case["cout"], 1, ffi.stream())
        return lib.pa_conv3x3_wino4_rows(*head, out, case["cout"], 1, case["rows"], ffi.stream())

    return Entry(_plain(call), [((case["B"], Ho, Wo, case["cout"]), F32)], inputs=[xd, wd, shd, rd], case=case)


def conv3x3_s2_sc(dev):
    ffi, lib = _ffi()
    B, H, W, cin, cout = 2, 32, 10, 32, 64
    assert lib.pa_conv3x3_s2_sc_supported(H, cin, cout)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    X, Wg, shift = randn(dev, B, H, W, cin, seed=27), randn(dev, 9, cout, cin, seed=28, scale=0.06), randn(dev, cout, seed=29)
    Wsc, shsc = randn(dev, cout, cin, seed=30, scale=0.2), randn(dev, cout, seed=31)
    call = lambda Y, Ysc: lib.pa_conv3x3_s2_sc(p(X), B, H, W, cin, p(Wg), p(shift), p(Wsc), p(shsc), Y, Ysc, cout, 1,
                                               ffi.stream())
    return Entry(_plain(call), [((B, Ho, Wo, cout), F32), ((B, Ho, Wo, cout), F32)], inputs=[X, Wg, shift, Wsc, shsc])


def _nearest_idx(Fm, Tp, dev):
    ramp = torch.arange(Fm, dtype=F32).view(1, 1, -1)
    return torch.nn.functional.interpolate(ramp, size=Tp, mode="nearest").view(-1).to(I32).to(dev)


def stats_pool(dev):
    ffi, lib = _ffi()
    B, Fh, Tp, Cc, S, Fm = 3, 2, 17, 32, 2, 24
    feat, masks, idx = randn(dev, B, Fh, Tp, Cc, seed=32), rand(dev, B, S, Fm, seed=33), _nearest_idx(Fm, Tp, dev)
    call = lambda out: lib.pa_stats_pool(p(feat), B, Fh, Tp, Cc, p(masks), S, Fm, p(idx), out, ffi.stream())
    return Entry(_plain(call), [((B, S, 2 * Cc * Fh), F32)], inputs=[feat, masks, idx])


def stats_pool_rows(dev):
    ffi, lib = _ffi()
    B, T0, Tp, Cc, ld, S, Fm, ld_stats = 17, 20, 18, 32, 36, 2, 25, 64
    mat = randn(dev, 2, T0, 16, ld, seed=34)
    masks, idx = rand(dev, B, S, Fm, seed=35), _nearest_idx(Fm, Tp, dev)
    scale, shift = 0.5 + rand(dev, Cc, seed=36), randn(dev, Cc, seed=37)
    call = lambda out: lib.pa_stats_pool_rows(p(mat), B, T0, Tp, Cc, ld, p(masks), S, Fm, p(idx), out, ld_stats, p(scale),
                                              p(shift), ffi.stream())
    return Entry(_plain(call), [((B, S, ld_stats), F32)], inputs=[mat, masks, idx, scale, shift])


RAGGED_LENGTHS = [8000, 16000, 12000]


def fbank_ragged(dev):
    ffi, lib = _ffi()
    w, lengths = _fb(dev), RAGGED_LENGTHS
    B, nmax = len(lengths), max(lengths)
    T = lib.pa_emb_num_fbank_frames(nmax)
    wd = wave(sum(lengths), seed=38).to(dev)
    od = torch.tensor(np.concatenate([[0], np.cumsum(lengths)[:-1]]), dtype=I64, device=dev)
    ld = torch.tensor(lengths, dtype=I32, device=dev)
    call = lambda out: lib.pa_fbank_ragged(p(wd), wd.numel(), p(od), p(ld), B, nmax, w.fb_window, w.fb_tw256, w.fb_tw512,
                                           w.fb_mel_w, w.fb_mel_lo, w.fb_mel_hi, 80, out, ffi.stream())
    return Entry(_plain(call), [((B, T, 80), F32)], inputs=[wd, od, ld])


def _ragged_width(n, halvings):
    wv = 1 + (n - 400) // 160
    for _ in range(halvings):
        wv = (wv - 1) // 2 + 1
    return wv


def zero_tail_cols(dev):
    ffi, lib = _ffi()
    lengths, halvings, H, Cc = RAGGED_LENGTHS, 2, 3, 8
    B, W = len(lengths), max(_ragged_width(n, halvings) for n in lengths)
    x0 = randn("cpu", B, H, W, Cc, seed=39)
    ld = torch.tensor(lengths, dtype=I32, device=dev)
    call = lambda x: lib.pa_zero_tail_cols(x, B, H, W, Cc, p(ld), halvings, ffi.stream())
    return Entry(_plain(call), [((B, H, W, Cc), F32)], inputs=[ld], initial={0: x0})


def stats_pool_ragged(dev):
    ffi, lib = _ffi()
    lengths, Fh, Cc = RAGGED_LENGTHS, 2, 32
    B, W = len(lengths), max(_ragged_width(n, 3) for n in lengths)
    feat, masks = randn(dev, B, Fh, W, Cc, seed=40), rand(dev, B, W, seed=41)
    ld = torch.tensor(lengths, dtype=I32, device=dev)
    call = lambda out: lib.pa_stats_pool_ragged(p(feat), B, Fh, W, Cc, p(ld), 3, p(masks), W, out, ffi.stream())
    return Entry(_plain(call), [((B, 2 * Cc * Fh), F32)], inputs=[feat, masks, ld])


# ---- wav2vec pieces
def w2v_conv0(dev):
    ffi, lib = _ffi()
    B, N, K0, S0, Cc = 3, 400, 10, 5, 32
    T = (N - K0) // S0 + 1
    P = T + 1
    wd = wave(B * N - 50, seed=42).to(dev)
    w, bias = randn(dev, Cc, K0, seed=43, scale=0.3), randn(dev, Cc, seed=44)
    call = lambda out: lib.pa_w2v_conv0(p(wd), wd.numel(), N, B, N, T, P, Cc, K0, S0, p(w), p(bias), out, ffi.stream())
    return Entry(_plain(call), [((B * P, Cc), F32)], inputs=[wd, w, bias])


def w2v_group_norm_gelu(dev):
    ffi, lib = _ffi()
    B, T, P, Cc = 3, 79, 80, 32
    x0 = randn("cpu", B * P, Cc, seed=45)
    g, b = 0.5 + rand(dev, Cc, seed=46), randn(dev, Cc, seed=47)
    call = lambda x, mean, rstd: lib.pa_w2v_group_norm_gelu(x, B, T, P, Cc, p(g), p(b), mean, rstd, ffi.stream())
    return Entry(_plain(call), [((B * P, Cc), F32), ((B, Cc), F32), ((B, Cc), F32)], inputs=[g, b], initial={0: x0})


def w2v_layernorm(dev):
    ffi, lib = _ffi()
    rows, Cc = 37, 96
    x, g, b = randn(dev, rows, Cc, seed=48), 0.5 + rand(dev, Cc, seed=49), randn(dev, Cc, seed=50)
    call = lambda out: lib.pa_w2v_layernorm(p(x), out, rows, Cc, p(g), p(b), 1, ffi.stream())
    return Entry(_plain(call), [((rows, Cc), F32)], inputs=[x, g, b])


def w2v_posconv(dev):
    ffi, lib = _ffi()
    B, T, P, D, groups, KW = 2, 19, 20, 64, 4, 8
    CG = D // groups
    x, w3, bias = randn(dev, B * P, D, seed=51), randn(dev, groups, KW, CG, CG, seed=52, scale=0.1), randn(dev, D, seed=53)
    call = lambda out: lib.pa_w2v_posconv(p(x), B, T, P, D, groups, KW, p(w3), p(bias), out, ffi.stream())
    return Entry(_plain(call), [((B * P, D), F32)], inputs=[x, w3, bias])


def w2v_softmax(dev):
    """the gated (WavLM) form"""
    ffi, lib = _ffi()
    B, H, T, Tp, P, D = 2, 2, 19, 24, 20, 64
    S0 = randn("cpu", B, H, T, Tp, seed=54)
    bias, xin = randn(dev, H, T, T, seed=55), randn(dev, B * P, D, seed=56)
    gw, gb, gc = randn(dev, 8, D // H, seed=57, scale=0.2), randn(dev, 8, seed=58), rand(dev, H, seed=59)
    call = lambda S: lib.pa_w2v_softmax(S, B, H, T, Tp, 0.125, p(bias), p(xin), P, D, p(gw), p(gb), p(gc), ffi.stream())
    return Entry(_plain(call), [((B, H, T, Tp), F32)], inputs=[bias, xin, gw, gb, gc], initial={0: S0})


def w2v_axpy(dev):
    ffi, lib = _ffi()
    n = 1028
    x, acc0 = randn(dev, n, seed=60), randn("cpu", n, seed=61)
    call = lambda acc: lib.pa_w2v_axpy(acc, p(x), 0.37, n, 0, ffi.stream())
    return Entry(_plain(call), [((n,), F32)], inputs=[x], initial={0: acc0})


def w2v_to_tiles(dev):
    ffi, lib = _ffi()
    B, T, P, D = 17, 5, 6, 32
    x = randn(dev, B * P, D, seed=62)
    call = lambda out: lib.pa_w2v_to_tiles(p(x), B, T, P, D, out, ffi.stream())
    return Entry(_plain(call), [((2 * T * 16, D), F32)], inputs=[x])


# ---- distances
def pdist_f64(dev):
    ffi, lib = _ffi()
    N, D = 65, 16
    X = randn(dev, N, D, seed=63, dtype=F64)
    call = lambda out: lib.pa_pdist_f64(p(X), N, D, out, ffi.stream())
    return Entry(_plain(call), [((N * (N - 1) // 2,), F64)], inputs=[X])


def cdist_cosine_f64(dev):
    ffi, lib = _ffi()
    NA, NB, D = 40, 7, 16
    A, B = randn(dev, NA, D, seed=64, dtype=F64), randn(dev, NB, D, seed=65, dtype=F64)
    call = lambda out, norms: lib.pa_cdist_cosine_f64(p(A), NA, p(B), NB, D, out, norms, ffi.stream())
    return Entry(_plain(call), [((NA, NB), F64), ((NA + NB,), F64)], inputs=[A, B])


def pdist_cosine_f64(dev):
    ffi, lib = _ffi()
    N, D = 65, 16
    X = randn(dev, N, D, seed=66, dtype=F64)
    call = lambda out, norms: lib.pa_pdist_cosine_f64(p(X), N, D, out, norms, ffi.stream())
    return Entry(_plain(call), [((N * (N - 1) // 2,), F64), ((N,), F64)], inputs=[X])


def centroid_means(dev):
    """four clusters, one of them empty (a NaN row)"""
    ffi, lib = _ffi()
    n, D, K = 50, 16, 4
    X = randn(dev, n, D, seed=67)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(68)).to(I32).to(dev)
    offsets = torch.tensor([0, 10, 10, 30, 50], dtype=I32, device=dev)
    call = lambda out: lib.pa_centroid_means(p(X), D, p(rows), p(offsets), K, out, ffi.stream())
    return Entry(_plain(call), [((K, D), F32, 1e30)], inputs=[X, rows, offsets])


def nonfinite_flag_f64(dev):
    ffi, lib = _ffi()
    n = 3000
    v = randn(dev, n, seed=69, dtype=F64)
    v[2017] = float("inf")
    call = lambda flag: lib.pa_nonfinite_flag_f64(p(v), n, flag, ffi.stream())
    return Entry(_plain(call), [((1,), I32, -77)], inputs=[v])


# ---- frame-domain kernels: 7 chunks of 56 frames, 10 frames apart, 3 local speakers, 4 clusters
FR = dict(C=7, F=56, S=3, K=4, step=10)
FR["T"] = (FR["C"] - 1) * FR["step"] + FR["F"]


def _frames(dev):
    c = dict(FR)
    c["seg"] = randint(dev, 0, 2, c["C"], c["F"], c["S"], seed=70, dtype=U8)
    c["start"] = (torch.arange(c["C"], dtype=I32) * c["step"]).to(dev)
    hard = randint("cpu", -1, c["K"], c["C"], c["S"], seed=71)
    hard[3] = -1                                                     # a chunk without any assigned speaker
    c["hard"] = hard.to(dev)
    c["scores"] = rand(dev, c["C"], c["F"], c["S"], seed=72)
    return c


def gather_chunks(dev):
    ffi, lib = _ffi()
    files = [wave(5000, seed=73).to(dev), wave(7000, seed=74).to(dev)]
    ptrs = torch.tensor([f.data_ptr() for f in files], dtype=I64, device=dev)
    lens = torch.tensor([5000, 7000], dtype=I64, device=dev)
    chunk_file = torch.tensor([0, 0, 1, 1, 1], dtype=I32, device=dev)
    chunk_start = torch.tensor([0, 4001, 16, 3000, 6000], dtype=I64, device=dev)
    n, N = 5, 1600
    call = lambda out: lib.pa_gather_chunks(p(ptrs), p(lens), p(chunk_file), p(chunk_start), n, N, out, ffi.stream())
    return Entry(_plain(call), [((n, N), F32)], inputs=files + [ptrs, lens, chunk_file, chunk_start])


def seg_chunk_stats(dev):
    ffi, lib = _ffi()
    c = _frames(dev)
    call = lambda active, clean: lib.pa_seg_chunk_stats(p(c["seg"]), c["C"], c["F"], c["S"], active, clean, ffi.stream())
    return Entry(_plain(call), [((c["C"], c["S"]), I32, -77), ((c["C"], c["S"]), I32, -77)], inputs=[c["seg"]])


def embedding_masks(dev):
    ffi, lib = _ffi()
    c = _frames(dev)
    clean = randint(dev, 0, c["F"], c["C"], c["S"], seed=75)
    call = lambda masks: lib.pa_embedding_masks(p(c["seg"]), c["C"], c["F"], c["S"], p(clean), 1, 20, masks, ffi.stream())
    return Entry(_plain(call), [((c["C"], c["S"], c["F"]), F32)], inputs=[c["seg"], clean])


def speaker_count(dev):
    ffi, lib = _ffi()
    c = _frames(dev)
    call = lambda count, scratch: lib.pa_speaker_count(p(c["seg"]), c["C"], c["F"], c["S"], p(c["start"]), c["T"], count,
                                                       scratch, ffi.stream())
    return Entry(_plain(call), [((c["T"],), U8), ((2 * c["T"],), I32, -77)], inputs=[c["seg"], c["start"]])


def cluster_activations(dev):
    ffi, lib = _ffi()
    c = _frames(dev)
    call = lambda act: lib.pa_cluster_activations(p(c["seg"]), c["C"], c["F"], c["S"], p(c["start"]), p(c["hard"]), c["K"],
                                                  c["T"], act, ffi.stream())
    return Entry(_plain(call), [((c["T"], c["K"]), I32, -77)], inputs=[c["seg"], c["start"], c["hard"]])


def topk_binarize(dev, f32):
    ffi, lib = _ffi()
    T, K, cap = 3001, 5, 3
    act = randint(dev, 0, 4, T, K, seed=76)                          # many equal activations: ties at the boundary
    if f32:
        act = act.float()
    count = randint(dev, 0, 5, T, seed=77, dtype=U8)
    fn = lib.pa_topk_binarize_f32 if f32 else lib.pa_topk_binarize
    call = lambda out, tie: fn(p(act), p(count), T, K, cap, out, tie, ffi.stream())
    return Entry(_plain(call), [((T, K), U8), ((T,), U8)], inputs=[act, count])


def binarize_hysteresis(dev):
    ffi, lib = _ffi()
    c = _frames(dev)
    call = lambda out: lib.pa_binarize_hysteresis(p(c["scores"]), c["C"], c["F"], c["S"], 0.6, 0.4, 0.5, -1, out,
                                                  ffi.stream())
    return Entry(_plain(call), [((c["C"], c["F"], c["S"]), U8)], inputs=[c["scores"]])


def cluster_max(dev):
    """NaN is a correct value here (a chunk without a speaker in the cluster): the untouched value is 1e30"""
    ffi, lib = _ffi()
    c = _frames(dev)
    call = lambda out: lib.pa_cluster_max(p(c["scores"]), c["C"], c["F"], c["S"], p(c["hard"]), c["K"], out, ffi.stream())
    return Entry(_plain(call), [((c["C"], c["F"], c["K"]), F32, 1e30)], inputs=[c["scores"], c["hard"]])


def aggregate(dev):
    ffi, lib = _ffi()
    c = _frames(dev)
    scores = c["scores"].clone()
    scores[2, :, 1] = float("nan")
    window = torch.from_numpy(np.hamming(c["F"])).to(dev)
    warm = torch.ones(c["F"], dtype=F64)
    warm[:5] = warm[-5:] = 1e-12
    warm = warm.to(dev)
    call = lambda out: lib.pa_aggregate(p(scores), c["C"], c["F"], c["S"], p(c["start"]), c["T"], p(window), p(warm), 1e-12,
                                        float("nan"), 0, out, ffi.stream())
    return Entry(_plain(call), [((c["T"], c["S"]), F32, 1e30)], inputs=[scores, c["start"], window, warm])


def aggregate_files(dev):
    """three files of 3, 0 and 5 chunks in rows that are multiples of 64; every row outside a file's frames is NaN"""
    ffi, lib = _ffi()
    F, S, step = 56, 3, 10
    chunk0 = torch.tensor([0, 3, 3, 8], dtype=I32, device=dev)
    row0 = torch.tensor([0, 128, 128, 256], dtype=I32, device=dev)
    T = torch.tensor([76, 0, 96], dtype=I32, device=dev)
    start = (torch.arange(5, dtype=I32) * step).to(dev)
    scores = rand(dev, 8, F, S, seed=78)
    window, warm = torch.ones(F, dtype=F64, device=dev), torch.ones(F, dtype=F64, device=dev)
    call = lambda out: lib.pa_aggregate_files(p(scores), 0, 8, F, S, 0, 3, p(chunk0), p(row0), p(T), p(start), 5, p(window),
                                              p(warm), 1e-12, float("nan"), 0, 256, out, ffi.stream())
    return Entry(_plain(call), [((256, S), F32, 1e30)], inputs=[scores, chunk0, row0, T, start, window, warm])


def resample_poly(dev):
    import resample_truth as RT
    ffi, lib = _ffi()
    taps, L, P, width = RT.bank(48000, 16000)
    n = 3001
    n_out = RT.num_out(n, L, P)
    x, tp = wave(n, seed=79).to(dev), torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float32)).to(dev)
    K = taps.shape[1]
    call = lambda out: lib.pa_resample_poly(p(x), n, p(tp), L, P, K, width, out, n_out, ffi.stream())
    return Entry(_plain(call), [((n_out,), F32)], inputs=[x, tp])


def plda_transform(dev):
    ffi, lib = _ffi()
    n, din, dmid, dout = 37, 64, 32, 16
    X = randn(dev, n, din, seed=80)
    mean1, lda = randn(dev, din, seed=81, dtype=F64, scale=0.1), randn(dev, din, dmid, seed=82, dtype=F64, scale=0.2)
    mean2, mu = randn(dev, dmid, seed=83, dtype=F64, scale=0.1), randn(dev, dmid, seed=84, dtype=F64, scale=0.1)
    trT = randn(dev, dmid, dout, seed=85, dtype=F64, scale=0.2)
    call = lambda fea: lib.pa_plda_transform(p(X), n, din, dmid, dout, p(mean1), p(lda), p(mean2), p(mu), p(trT), fea,
                                             ffi.stream())
    return Entry(_plain(call), [((n, dout), F64)], inputs=[X, mean1, lda, mean2, mu, trT])


def constrained_assign(dev):
    ffi, lib = _ffi()
    chunks, speakers, clusters = 70, 3, 5
    soft = rand(dev, chunks, speakers, clusters, seed=86, dtype=F64)
    silent = (rand(dev, chunks, speakers, seed=87) < 0.2).to(U8)
    call = lambda hard, flagged: lib.pa_constrained_assign(p(soft), p(silent), chunks, speakers, clusters, hard, flagged,
                                                           ffi.stream())
    return Entry(_plain(call), [((chunks, speakers), torch.int8, -91), ((chunks,), U8)], inputs=[soft, silent])


# ---- metrics
def der_counts(dev):
    ffi, lib = _ffi()
    T, Sr, Sh = 3001, 3, 4
    ref, hyp, keep = randint(dev, 0, 2, T, Sr, seed=88, dtype=U8), randint(dev, 0, 2, T, Sh, seed=89, dtype=U8), \
        randint(dev, 0, 2, T, seed=90, dtype=U8)
    call = lambda out: lib.pa_der_counts(p(ref), p(hyp), p(keep), T, Sr, Sh, out, ffi.stream())
    return Entry(_plain(call), [((Sr * Sh + Sr + Sh + 4,), I64, -77)], inputs=[ref, hyp, keep])


def _der_chunks(dev):
    B, S, F, Q = 5, 3, 293, 4
    return dict(B=B, S=S, F=F, Q=Q, preds=rand(dev, B, S, F, seed=91), target=randint(dev, 0, 2, B, S, F, seed=92, dtype=U8),
                thr=torch.tensor([0.2, 0.4, 0.6, 0.8], dtype=F32, device=dev))


def der_chunks(dev):
    ffi, lib = _ffi()
    c = _der_chunks(dev)
    call = lambda counts, total: lib.pa_der_chunks(p(c["preds"]), p(c["target"]), 0, c["B"], c["S"], c["F"], p(c["thr"]),
                                                   c["Q"], None, counts, total, ffi.stream())
    return Entry(_plain(call), [((c["B"], c["Q"], 3), I32, -77), ((c["B"],), I32, -77)],
                 inputs=[c["preds"], c["target"], c["thr"]])


def der_chunks_sum(dev):
    ffi, lib = _ffi()
    B, Q = 300, 4
    counts, total = randint(dev, 0, 100, B, Q, 3, seed=93), randint(dev, 0, 300, B, seed=94)
    call = lambda out: lib.pa_der_chunks_sum(p(counts), p(total), B, Q, out, ffi.stream())
    return Entry(_plain(call), [((3 * Q + 1,), I64, -77)], inputs=[counts, total])


def trial_cosine_f64(dev):
    ffi, lib = _ffi()
    N, D, T = 20, 16, 300
    E = randn(dev, N, D, seed=95, dtype=F64)
    i1, i2 = randint(dev, 0, N, T, seed=96), randint(dev, 0, N, T, seed=97)
    call = lambda out, norms: lib.pa_trial_cosine_f64(p(E), N, D, p(i1), p(i2), T, out, norms, ffi.stream())
    return Entry(_plain(call), [((T,), F64), ((N,), F64)], inputs=[E, i1, i2])


# ---- assignment
def lsap_batch(dev):
    ffi, lib = _ffi()
    batch, rows, cols = 5, 6, 7
    cost = rand(dev, batch, rows, cols, seed=98, dtype=F64)
    call = lambda col4row, total, status: lib.pa_lsap_batch(p(cost), rows * cols, cols, 1, batch, rows, cols, None, None, 0,
                                                            col4row, total, status, ffi.stream())
    return Entry(_plain(call), [((batch, rows), I32, -77), ((batch,), F64), ((batch,), U8)], inputs=[cost])


def pair_costs(dev):
    ffi, lib = _ffi()
    batch, frames, C1, C2 = 3, 50, 3, 4
    y1, y2 = rand(dev, batch, frames, C1, seed=99), rand(dev, batch, frames, C2, seed=100)
    call = lambda cost: lib.pa_pair_costs(p(y1), frames * C1, C1, 1, p(y2), frames * C2, C2, 1, 0, batch, frames, C1, C2, 0,
                                          cost, ffi.stream())
    return Entry(_plain(call), [((batch, C2, C2), F64)], inputs=[y1, y2])


def permute_classes(dev):
    ffi, lib = _ffi()
    batch, frames, C1, C2 = 3, 50, 3, 4
    y2 = rand(dev, batch, frames, C2, seed=101)
    perm = torch.tensor([[2, 0, 3], [1, -1, 0], [3, 2, 1]], dtype=I32, device=dev)
    call = lambda out: lib.pa_permute_classes(p(y2), frames * C2, C2, 1, 0, p(perm), C1, batch, frames, C1, C2, out,
                                              ffi.stream())
    return Entry(_plain(call), [((batch, frames, C1), F32)], inputs=[y2, perm])


# ---- identification: a second table of more than one tile of 256 rows
def cohort_stats(dev):
    ffi, lib = _ffi()
    M, N, D, K = 10, 300, 16, 20
    X, Cc = randn(dev, M, D, seed=102, dtype=F64), randn(dev, N, D, seed=103, dtype=F64)
    need = lib.pa_cohort_stats_workspace_bytes(M, N, D)

    def call(ws, nbytes, mean, stdev, status):
        return lib.pa_cohort_stats_f64(p(X), M, p(Cc), N, D, K, mean, stdev, status, ws, nbytes, ffi.stream())

    return Entry(call, [((M,), F64), ((M,), F64), ((M,), I32, -77)], need, inputs=[X, Cc])


def _gallery(dev):
    M, Ng, D = 10, 300, 16
    return dict(M=M, Ng=Ng, D=D, Q=randn(dev, M, D, seed=104, dtype=F64), G=randn(dev, Ng, D, seed=105, dtype=F64),
                qm=rand(dev, M, seed=106, dtype=F64), qs=0.5 + rand(dev, M, seed=107, dtype=F64),
                gm=rand(dev, Ng, seed=108, dtype=F64), gs=0.5 + rand(dev, Ng, seed=109, dtype=F64))


def gallery_topk(dev):
    ffi, lib = _ffi()
    c, k = _gallery(dev), 5
    need = lib.pa_gallery_workspace_bytes(c["M"], c["Ng"], c["D"])

    def call(ws, nbytes, values, indices):
        return lib.pa_gallery_topk_f64(p(c["Q"]), c["M"], p(c["G"]), c["Ng"], c["D"], p(c["qm"]), p(c["qs"]), p(c["gm"]),
                                       p(c["gs"]), k, values, indices, ws, nbytes, ffi.stream())

    return Entry(call, [((c["M"], k), F64), ((c["M"], k), I32, -77)], need,
                 inputs=[c[n] for n in ("Q", "G", "qm", "qs", "gm", "gs")])


def gallery_pairs(dev):
    ffi, lib = _ffi()
    c, P = _gallery(dev), 300
    iq, ig = randint(dev, 0, c["M"], P, seed=110), randint(dev, 0, c["Ng"], P, seed=111)
    call = lambda out: lib.pa_gallery_pairs_f64(p(c["Q"]), c["M"], p(c["G"]), c["Ng"], c["D"], p(c["qm"]), p(c["qs"]),
                                                p(c["gm"]), p(c["gs"]), p(iq), p(ig), P, out, ffi.stream())
    return Entry(_plain(call), [((P,), F64)], inputs=[c[n] for n in ("Q", "G", "qm", "qs", "gm", "gs")] + [iq, ig])
