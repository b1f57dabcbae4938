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
then a smaller one, whose result must equal, byte for byte, that of a freshly constructed engine."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import north_star_ratio
from hostile_workspace import FILLS, HostileWorkspace, run_under_fills

pytestmark = pytest.mark.gpu

N1 = 16000            # one second: 56 SincNet frames, 49 wav2vec frames, 42 / 101 x-vector frames


def _log(what, need):
    """the size a case ran at goes to the test's output (`pytest -rA` shows it)"""
    print(f"hostile_workspace[{what}]: workspace {int(need)} bytes")


def _fills(what, call, need, outputs, device, initial=None):
    _log(what, need)
    with torch.cuda.device(device):
        return run_under_fills(call, need, outputs, device, what, initial)


def _wave(n, seed):
    """noise + a tone + a DC offset, as the forward tests of the networks use"""
    g = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(n, generator=g) + 0.05 * torch.sin(torch.arange(n) * 0.01) + 0.02
    return x.clamp(-1, 1)


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
    from oracle import seeded_pyannet
    from oracle.models import PyanNet
    from pyannote_audio_amd.weights import SegmentationPack
    std = seeded_pyannet(seed=1234, num_layers=4)
    torch.manual_seed(77)
    lstm = {"hidden_size": 64, "num_layers": 2, "bidirectional": False, "monolithic": False}
    linear = {"hidden_size": 96, "num_layers": 2}
    gen = PyanNet(num_classes=7, lstm=lstm, linear=linear).eval()
    return {"h128": (std, SegmentationPack(std.state_dict(), {"lstm": {"num_layers": 4}}, 7, 3, 2, gpu_device)),
            "generic": (gen, SegmentationPack(gen.state_dict(), {"lstm": lstm, "linear": linear}, 7, 3, 2, gpu_device))}


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
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    model, pack = seg_models[name]
    w = pack.struct
    wav = _wave((B - 1) * stride + N1 - short, seed=B + stride)
    wd = wav.to(gpu_device)
    F = lib.pa_seg_num_frames(N1, 10)
    assert F == 56
    strided = lib.pa_seg_workspace_bytes_strided(w, B, N1, stride)
    plain = lib.pa_seg_workspace_bytes(w, B, N1)
    if stride == 1600:
        assert strided > plain, "the shared sinc layer asks for its span scratch"
    else:
        assert strided == plain
    need = strided if query == "strided" else plain

    def call(ws, nbytes, logp, ml):
        return lib.pa_seg_forward(w, ffi.ptr(wd), wd.numel(), stride, B, N1, logp, ml, ws, nbytes, ffi.stream())

    logp, ml = _fills(f"pa_seg_forward {name} B={B} stride={stride} {query}", call, need,
                      [((B, F, 7), torch.float32), ((B, F, 3), torch.uint8)], gpu_device)
    with torch.inference_mode():
        ref = model(_chunks(wav, stride, B, N1))
    assert north_star_ratio(f"hostile_seg_{name}_B{B}_s{stride}_{query}", logp, ref) <= 1.0
    assert _hard_decisions_match(ml, ref)


def test_seg_forward_files(seg_models, gpu_device):
    """chunks_per_file = [3, 0, 1, 13] at stride 1600: a file of no chunks, a one-chunk file (the per-chunk sinc layer),
    a file that ends 900 samples before its chunks do, 17 chunks in all (a tile boundary inside the last file)"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    model, pack = seg_models["h128"]
    w = pack.struct
    stride, counts = 1600, [3, 0, 1, 13]
    lengths = [2 * stride + N1, 5000, N1, 12 * stride + N1 - 900]
    waves = [_wave(n, seed=40 + i) for i, n in enumerate(lengths)]
    dev_waves = [x.to(gpu_device) for x in waves]
    n, total, F = len(counts), sum(counts), 56
    ptrs = (C.c_void_p * n)(*[x.data_ptr() for x in dev_waves])
    lens = (C.c_int64 * n)(*lengths)
    cnts = (C.c_int * n)(*counts)
    need = lib.pa_seg_files_workspace_bytes(w, n, cnts, N1, stride)

    def call(ws, nbytes, logp, ml):
        return lib.pa_seg_forward_files(w, ptrs, lens, cnts, n, stride, N1, logp, ml, ws, nbytes, ffi.stream())

    outputs = [((total, F, 7), torch.float32), ((total, F, 3), torch.uint8)]
    logp, ml = _fills("pa_seg_forward_files [3, 0, 1, 13]", call, need, outputs, gpu_device)
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
    from oracle import seeded_sseriouss
    from oracle.models import TINY_WAV2VEC2
    from pyannote_audio_amd.segmentation import SSeRiouSSEngine
    from pyannote_audio_amd.weights import SSeRiouSSPack
    model = seeded_sseriouss(wav2vec=dict(TINY_WAV2VEC2), num_layers=2)
    hparams = {"wav2vec": dict(TINY_WAV2VEC2), "wav2vec_layer": -1, "lstm": {"num_layers": 2}}
    return model, SSeRiouSSPack(model.state_dict(), hparams, 7, 3, 2, gpu_device), SSeRiouSSEngine


@pytest.mark.parametrize("B", [1, 17])
def test_sser_forward(sser, gpu_device, B):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    model, pack, _ = sser
    w = pack.struct
    g = torch.Generator().manual_seed(B)
    wav = (0.1 * torch.randn(B * N1, generator=g)).clamp(-1, 1)
    wd = wav.to(gpu_device)
    F = lib.pa_sser_num_frames(w, N1)
    bias = pack.relative_bias(F)
    need = lib.pa_sser_workspace_bytes(w, B, N1)

    def call(ws, nbytes, logp, ml):
        return lib.pa_sser_forward(w, ffi.ptr(wd), wd.numel(), N1, B, N1, ffi.ptr(bias), logp, ml, ws, nbytes,
                                   ffi.stream())

    logp, ml = _fills(f"pa_sser_forward B={B}", call, need, [((B, F, 7), torch.float32), ((B, F, 3), torch.uint8)],
                      gpu_device)
    with torch.inference_mode():
        ref = model(wav.view(B, 1, N1))
    assert north_star_ratio(f"hostile_sser_B{B}", logp, ref) <= 1.0
    assert _hard_decisions_match(ml, ref)


# ============================================================================================== embedding networks
def _masks(B, S, Fm, seed):
    """(B, S, Fm) 0 / 1 weights, one mask all zero (its embedding is the bias path)"""
    g = torch.Generator().manual_seed(seed)
    masks = (torch.rand(B, S, Fm, generator=g) < 0.6).float()
    masks[0, S - 1] = 0.0
    return masks


def _masked_embeddings(oracle, chunks, masks):
    with torch.inference_mode():
        if masks is None:
            return oracle(chunks)[:, None]
        return torch.stack([oracle(chunks, weights=masks[:, s]) for s in range(masks.shape[1])], dim=1)


def _embedding_case(what, forward, workspace_bytes, engine, oracle, dim, B, S, N, device, seed):
    """one pa_*_forward of the embedding family: B chunks of N samples side by side, S masks per chunk (S = 1: none)"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    w = engine.pack.struct
    g = torch.Generator().manual_seed(seed)
    wav = (0.1 * torch.randn(B * N, generator=g) + 0.03 * torch.sin(torch.arange(B * N) * 0.02)).clamp(-1, 1)
    wd = wav.to(device)
    Tp = engine.num_pool_frames(N)
    Fm = lib.pa_seg_num_frames(N, 10)                    # masks at the segmentation model's frame rate
    masks = _masks(B, S, Fm, seed) if S > 1 else None
    md = masks.to(device) if masks is not None else None
    idx = engine.nearest_index(Fm, Tp) if masks is not None else None
    need = workspace_bytes(w, B, N, S)

    def call(ws, nbytes, emb):
        return forward(w, ffi.ptr(wd), wd.numel(), N, B, N, ffi.ptr(md), S, Fm if masks is not None else 0,
                       ffi.ptr(idx), emb, ws, nbytes, ffi.stream())

    (emb,) = _fills(what, call, need, [((B, S, dim), torch.float32)], device)
    want = _masked_embeddings(oracle, wav.view(B, 1, N), masks)
    assert north_star_ratio("hostile_" + what.replace(" ", "_"), emb, want) <= 1.0


@pytest.fixture(scope="module")
def xvec(gpu_device):
    from oracle import seeded_xvector
    from pyannote_audio_amd.embedding import XVectorEngine
    from pyannote_audio_amd.weights import XVectorPack
    model = seeded_xvector()
    return model, XVectorEngine(XVectorPack(model.state_dict(), {"sincnet": {"stride": 10}}, gpu_device))


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("B", [1, 5, 17])
def test_xvec_forward(xvec, gpu_device, B, S):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    model, eng = xvec
    _embedding_case(f"pa_xvec_forward B={B} S={S}", lib.pa_xvec_forward, lib.pa_xvec_workspace_bytes, eng, model, 512,
                    B, S, N1, gpu_device, seed=10 * B + S)


@pytest.fixture(scope="module")
def xvec_mfcc(gpu_device):
    import pyannote_audio_amd as pa
    import xvector_mfcc_oracle as xo
    out = {}
    for name, mfcc in (("centred", None), ("uncentred_hop160", {"melkwargs": {"center": False, "hop_length": 160}})):
        oracle = xo.seeded_xvector_mfcc(seed=3579, mfcc=mfcc)
        model = pa.XVectorMFCC(oracle.state_dict(), xo.xvector_mfcc_hparams(oracle), pa.model.embedding_specifications())
        out[name] = (oracle, model.to(gpu_device).engine)
    return out


@pytest.mark.parametrize("config", ["centred", "uncentred_hop160"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("B", [1, 5, 17])
def test_xvec_mfcc_forward(xvec_mfcc, gpu_device, B, S, config):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    oracle, eng = xvec_mfcc[config]
    assert bool(eng.pack.struct.center) == (config == "centred")
    _embedding_case(f"pa_xvec_mfcc_forward {config} B={B} S={S}", lib.pa_xvec_mfcc_forward,
                    lib.pa_xvec_mfcc_workspace_bytes, eng, oracle, 512, B, S, N1, gpu_device, seed=20 * B + S)


def _bottleneck_oracle():
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


@pytest.fixture(scope="module")
def emb_models(gpu_device):
    """ResNet34 of BasicBlocks (seeded as in tests/test_emb_gpu.py), the Bottleneck network, and the ResNet34 with
    fbank_centering_span = 0.4 s (an odd running-mean kernel of 39 frames)"""
    from oracle import seeded_wespeaker
    from pyannote_audio_amd.embedding import EmbeddingEngine
    from pyannote_audio_amd.weights import EmbeddingPack
    basic, bottleneck, span = seeded_wespeaker(seed=4321), _bottleneck_oracle(), seeded_wespeaker(seed=4321)
    span.fbank_centering_span = 0.4
    return {"basic": (basic, EmbeddingEngine(EmbeddingPack(basic.state_dict(), gpu_device))),
            "bottleneck": (bottleneck, EmbeddingEngine(EmbeddingPack(bottleneck.state_dict(), gpu_device))),
            "span39": (span, EmbeddingEngine(EmbeddingPack(span.state_dict(), gpu_device, center_kernel=39)))}


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
    _embedding_case(f"pa_emb_forward {name} B={B} S={S} N={N}", lib.pa_emb_forward, lib.pa_emb_workspace_bytes, eng,
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
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    oracle, eng = emb_models["basic"]
    w = eng.pack.struct
    lengths = _five_ragged_lengths()
    B, n_max = len(lengths), max(lengths)
    waves = [_wave(n, seed=60 + i) for i, n in enumerate(lengths)]
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    wd = torch.cat(waves).to(gpu_device)
    off_d = torch.from_numpy(offsets.astype(np.int64)).to(gpu_device)
    len_d = torch.tensor(lengths, dtype=torch.int32, device=gpu_device)
    g = torch.Generator().manual_seed(17)
    masks = [(torch.rand(eng.num_pool_frames(n) + 9, generator=g) < 0.7).float() for n in lengths]
    pooled = torch.ones((B, eng.num_pool_frames(n_max)), dtype=torch.float32, device=gpu_device)
    for b, (m, n) in enumerate(zip(masks, lengths)):
        p = eng.pool_weights(m.to(gpu_device), n)
        pooled[b, :p.numel()] = p
    need = lib.pa_emb_ragged_workspace_bytes(w, B, n_max)

    def call(ws, nbytes, emb):
        return lib.pa_emb_forward_ragged(w, ffi.ptr(wd), wd.numel(), ffi.ptr(off_d), ffi.ptr(len_d), B, n_max,
                                         ffi.ptr(pooled), emb, ws, nbytes, ffi.stream())

    (emb,) = _fills(f"pa_emb_forward_ragged {lengths}", call, need, [((B, 256), torch.float32)], gpu_device)
    with torch.inference_mode():
        want = torch.cat([oracle(x[None, None], weights=m[None]) for x, m in zip(waves, masks)])
    assert north_star_ratio("hostile_emb_forward_ragged", emb, want) <= 1.0


def test_emb_calibrate_winograd(emb_models, gpu_device):
    """report (zeroed by the call) and the embeddings of the direct path"""
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd.weights import EmbeddingPack
    lib = ffi.load()
    oracle, _ = emb_models["basic"]
    # every Winograd image in place.  (`pack` stays in scope: the struct holds raw pointers into the pack's tensors.)
    pack = EmbeddingPack(oracle.state_dict(), gpu_device, guard=False)
    w = pack.struct
    B, N = 2, 32000
    wav = _wave(B * N, seed=70)
    wd = wav.to(gpu_device)
    need = lib.pa_emb_calibrate_workspace_bytes(w, B, N)

    def call(ws, nbytes, report, emb):
        return lib.pa_emb_calibrate_winograd(w, ffi.ptr(wd), wd.numel(), N, B, N, report, emb, ws, nbytes, ffi.stream())

    report, emb = _fills("pa_emb_calibrate_winograd", call, need,
                         [((2 * 128, 4), torch.float32), ((B, 256), torch.float32)], gpu_device)
    with torch.inference_mode():
        want = oracle(wav.view(B, 1, N))
    assert north_star_ratio("hostile_emb_calibrate_direct_path", emb, want) <= 1.0
    # 29 of the 32 convolutions have stride 1: all carry an F(2x2) image, those of layers 2 - 4 an F(4x4) image too
    f4, f2 = report[report[:, 0] > 0], report[report[:, 2] > 0]
    assert len(f2) == 29 and 0 < len(f4) < 29 and torch.isfinite(report).all()
    assert (f4[:, 1] < f4[:, 0]).all() and (f2[:, 3] < f2[:, 2]).all()


# ============================================================================================ exact kernels: linkage
def _clustered_unit(n, d, seed, dup):
    """clustered points with duplicated rows (exact ties), as tests/test_pipeline_gpu.py builds them"""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((5, d))
    X = (centers[rng.integers(0, 5, n)] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)
    if dup:
        X[rng.integers(0, n, dup)] = X[rng.integers(0, n, dup)]
    return X / np.linalg.norm(X, axis=1, keepdims=True)


# (n, duplicated rows, PA_LINKAGE_FAST): without ties the heap-free merge on the square copy finishes (65 and 300 have
# square_ld(n) > n); with ties it hands over to the heap kernel; n = 2 is below its smallest size; n <= 1024 is one
# workgroup, no mailbox
CENTROID_CASES = [(2, 0, None), (3, 0, None), (65, 0, None), (65, 13, None), (300, 0, None), (300, 60, None),
                  (1000, 0, None), (1000, 25, None), (300, 60, "0")]


@pytest.mark.parametrize("n,dup,fast", CENTROID_CASES,
                         ids=[f"n{c[0]}-dup{c[1]}" + ("-fast0" if c[2] else "") for c in CENTROID_CASES])
def test_linkage_centroid(gpu_device, monkeypatch, n, dup, fast):
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import pdist
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    if fast is not None:
        monkeypatch.setenv("PA_LINKAGE_FAST", fast)          # (as tests/test_pipeline_gpu.py switches it)
    y = pdist(_clustered_unit(n, 16, seed=n + dup, dup=dup))
    cond = torch.from_numpy(y).to(gpu_device)
    need = lib.pa_linkage_workspace_bytes(n)

    def call(ws, nbytes, Z):
        D = cond.clone()                                     # (overwritten when the heap kernel runs)
        return lib.pa_linkage_centroid_f64(ffi.ptr(D), n, Z, ws, nbytes, ffi.stream())

    (Z,) = _fills(f"pa_linkage_centroid_f64 n={n} dup={dup} fast={fast}", call, need, [((n - 1, 4), torch.float64)],
                  gpu_device)
    got, want = Z.numpy(), linkage(y, method="centroid")
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"first differing merge {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


@pytest.mark.parametrize("method", ["single", "complete", "average", "weighted", "ward"])
@pytest.mark.parametrize("n", [2, 130])
def test_linkage_chain(gpu_device, n, method):
    from scipy.spatial.distance import pdist
    import pyannote_audio_amd.ffi as ffi
    from linkage_chain_model import raw_merges
    from pyannote_audio_amd import distance
    from test_linkage_methods_gpu import clustered
    lib = ffi.load()
    y = pdist(clustered(n, 8, seed=n, dup=n // 6), "euclidean")
    D = torch.from_numpy(y).to(gpu_device)
    need = lib.pa_linkage_chain_workspace_bytes(n)

    def call(ws, nbytes, raw):
        return lib.pa_linkage_chain_f64(ffi.ptr(D), n, distance.CHAIN_METHODS[method], raw, ws, nbytes, ffi.stream())

    (raw,) = _fills(f"pa_linkage_chain_f64 n={n} {method}", call, need, [((n - 1, 4), torch.float64)], gpu_device)
    got, want = raw.numpy(), raw_merges(y, n, method)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"first differing raw merge {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
    assert torch.equal(D.cpu(), torch.from_numpy(y))


# ============================================================================================= exact kernels: KMeans
@pytest.mark.parametrize("rounds,max_iter", [(8, 300), (0, 40)])
@pytest.mark.parametrize("row", ["70x16-k5", "table4"])
def test_kmeans(gpu_device, row, rounds, max_iter):
    import kmeans_model as km
    import pyannote_audio_amd.distance as distance
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    n, d, g, k, noise = (70, 16, 5, 5, 0.7) if row == "70x16-k5" else km.TABLE[4]
    n_init = 3
    X = km.data(n, d, g, noise, 0, np.float64)
    first, uniforms = distance.kmeans_draws(n, k, n_init, 42)
    Xd = torch.from_numpy(np.ascontiguousarray(X)).to(gpu_device)
    first_d, uniforms_d = torch.from_numpy(first).to(gpu_device), torch.from_numpy(uniforms).to(gpu_device)
    need = lib.pa_kmeans_workspace_bytes(n, d, k, n_init)

    def call(ws, nbytes, labels, centers, inertia, picks, status):
        return lib.pa_kmeans_f64(ffi.ptr(Xd), n, d, k, n_init, ffi.ptr(first_d), ffi.ptr(uniforms_d), max_iter, 1e-4,
                                 rounds, labels, centers, inertia, picks, status, ws, nbytes, ffi.stream())

    labels, centers, inertia, picks, status = _fills(
        f"pa_kmeans_f64 n={n} d={d} k={k} round_iterations={rounds}", call, need,
        [((n_init, n), torch.int32, -77), ((n_init, k, d), torch.float64), ((n_init,), torch.float64),
         ((n_init, k), torch.int32, -77), ((n_init, 4), torch.int32, -77)], gpu_device)
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
    import pyannote_audio_amd.ffi as ffi
    from verification_truth import det_curve_truth
    lib = ffi.load()
    y_true, scores = det_cases[name]
    T = len(scores)
    keys = torch.from_numpy(np.asarray(scores, dtype=np.float64)).to(gpu_device)
    keys, order = torch.sort(-keys if negate else keys, stable=True)
    labels = (torch.from_numpy(np.asarray(y_true)).to(gpu_device) != 0).to(torch.uint8)[order].contiguous()
    need = lib.pa_det_workspace_bytes(T)

    def call(ws, nbytes, fps, tps, thr, fpr, fnr, status):
        return lib.pa_det_curve_f64(ffi.ptr(keys), ffi.ptr(labels), T, negate, fps, tps, thr, fpr, fnr, status, ws,
                                    nbytes, ffi.stream())

    fps, tps, thr, fpr, fnr, status = _fills(
        f"pa_det_curve_f64 {name} T={T} negate={negate}", call, need,
        [((T + 1,), torch.int32, -77), ((T + 1,), torch.int32, -77), ((T + 1,), torch.float64),
         ((T + 1,), torch.float64), ((T + 1,), torch.float64), ((8,), torch.int64, -77)], gpu_device)
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
    from scipy.cluster.hierarchy import fcluster, linkage
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd.clustering import Dendrogram
    from test_dendrogram_cuts_cpu import points
    from test_dendrogram_cuts_gpu import many_thresholds
    lib = ffi.load()
    n = 65
    Z = linkage(points("random", n, seed=n), method="centroid")
    T = 2 * lib.pa_dendrogram_cuts_chunk() + 3
    thresholds = many_thresholds(Z, T, seed=9)
    plan = [torch.from_numpy(a).to(gpu_device) for a in Dendrogram(Z).plan()]
    t_dev = torch.from_numpy(thresholds).to(gpu_device)
    need = lib.pa_dendrogram_cuts_workspace_bytes(n, T)

    def call(ws, nbytes, labels, counts):
        return lib.pa_dendrogram_cuts(*(ffi.ptr(a) for a in plan), n, ffi.ptr(t_dev), T, labels, counts, ws, nbytes,
                                      ffi.stream())

    labels, counts = _fills(f"pa_dendrogram_cuts n={n} T={T}", call, need,
                            [((T, n), torch.int32, -77), ((T,), torch.int32, -77)], gpu_device)
    want = np.stack([fcluster(Z, t, criterion="distance") - 1 for t in thresholds])
    assert (labels.numpy() == want).all()
    assert (counts.numpy() == want.max(axis=1) + 1).all()


# ================================================================================== exact kernels: annotation counts
def _annot_arrays(case, device):
    def f64(rows):
        return torch.tensor([[r[0], r[1]] for r in rows], dtype=torch.float64).reshape(-1, 2).to(device)

    def i32(rows):
        return torch.tensor([r[2] for r in rows], dtype=torch.int32).to(device)

    return f64(case["ref"]), i32(case["ref"]), f64(case["hyp"]), i32(case["hyp"]), f64(case["uem"])


def _annot_case():
    """dyadic boundaries (exact sums), a uem of three regions, 2 reference and 4 hypothesis labels, a collar"""
    import annotation_metrics_truth as truth
    case = truth.random_dyadic_case(21, Nr=40, Nh=50, Nu=3, Kr=2, Kh=4, collar=0.25)
    assert len(case["uem"]) == 3 and case["Kh"] > case["Kr"]
    return case


def test_annot_counts(gpu_device):
    from fractions import Fraction
    import annotation_metrics_truth as truth
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    case = _annot_case()
    ref_seg, ref_lab, hyp_seg, hyp_lab, uem_seg = _annot_arrays(case, gpu_device)
    Nr, Nh, Nu, Kr, Kh = len(case["ref"]), len(case["hyp"]), len(case["uem"]), case["Kr"], case["Kh"]
    need = lib.pa_annot_counts_workspace_bytes(Nr, Nh, Nu)

    def call(ws, nbytes, out):
        return lib.pa_annot_counts(ffi.ptr(ref_seg), ffi.ptr(ref_lab), Nr, Kr, ffi.ptr(hyp_seg), ffi.ptr(hyp_lab), Nh,
                                   Kh, ffi.ptr(uem_seg), Nu, case["collar"], 0, out, ws, nbytes, ffi.stream())

    (out,) = _fills("pa_annot_counts", call, need, [((Kr * Kh + Kr + Kh + 7,), torch.float64)], gpu_device)
    assert [Fraction(v) for v in out.tolist()] == truth.flat(truth.case_truth(case))
    assert out[-7].item() > 0.0                          # `total`: something was evaluated


def test_annot_window_counts(gpu_device):
    from fractions import Fraction
    import annotation_metrics_truth as truth
    import pyannote_audio_amd.ffi as ffi
    import window_counts_cases as cases
    lib = ffi.load()
    case = cases.with_windows(_annot_case(), cases.random_windows(5, 9))
    cases.assert_dyadic(case)
    ref_seg, ref_lab, hyp_seg, hyp_lab, uem_seg = _annot_arrays(case, gpu_device)
    win = torch.tensor(case["windows"], dtype=torch.float64).reshape(-1, 2).to(gpu_device)
    Nr, Nh, Nu, Kr, Kh, W = len(case["ref"]), len(case["hyp"]), len(case["uem"]), case["Kr"], case["Kh"], 9
    need = lib.pa_annot_window_counts_workspace_bytes(Nr, Nh, Nu, W)

    def call(ws, nbytes, out):
        return lib.pa_annot_window_counts(ffi.ptr(ref_seg), ffi.ptr(ref_lab), Nr, Kr, ffi.ptr(hyp_seg),
                                          ffi.ptr(hyp_lab), Nh, Kh, ffi.ptr(uem_seg), Nu, ffi.ptr(win), W,
                                          case["collar"], 0, out, ws, nbytes, ffi.stream())

    (out,) = _fills("pa_annot_window_counts", call, need, [((W, Kr * Kh + Kr + Kh + 7), torch.float64)], gpu_device)
    for w, (row, want) in enumerate(zip(out.tolist(), cases.window_truths(case))):
        assert [Fraction(v) for v in row] == truth.flat(want), (w, case["windows"][w])
    assert out[:, -7].count_nonzero().item() >= 3


def test_annot_corpus_counts(gpu_device):
    """three files, gaps filled on the device: every file's block equals, bit for bit, the per-file path
    (host `support`, pa_annot_counts), as tests/test_corpus_counts_gpu.py holds it"""
    import random
    import evaluation_truth as et
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd.evaluation import Corpus
    from test_corpus_counts_gpu import make_file, per_file, split_turns
    lib = ffi.load()
    rng = random.Random(5)
    files = [make_file("a", et.random_rows(rng, 30, ["a", "b"], 40.0, True),
                       et.random_rows(rng, 40, ["x", "y", "z"], 40.0, True), uem=((0.5, 30.0), (32.0, 50.0))),
             make_file("b", split_turns(20, ["a", "b"]), split_turns(30, ["x", "y", "z", "w"], start=0.5)),
             make_file("c", et.random_rows(rng, 12, ["a"], 20.0, True), et.random_rows(rng, 25, ["x", "y"], 20.0, True))]
    corpus = Corpus(files, device=gpu_device)
    struct, out_off = corpus._call.struct, corpus._call.out_off
    need = lib.pa_annot_corpus_workspace_bytes(C.byref(struct))
    fill, collar, skip = 0.25, 0.25, 1

    def call(ws, nbytes, out, merged):
        return lib.pa_annot_corpus_counts(C.byref(struct), fill, collar, skip, out, merged, ws, nbytes, ffi.stream())

    out, merged = _fills("pa_annot_corpus_counts", call, need,
                         [((int(out_off[-1]),), torch.float64), ((len(files),), torch.int32, -77)], gpu_device)
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
    import pyannote_audio_amd.ffi as ffi
    from test_multilabel_gpu import FRAMES
    lib = ffi.load()
    T, K, cap = 2001, 2, 1000
    scores = np.full((T, K), 0.1, dtype=np.float32)
    scores[0::2, 0] = 0.9
    for a, b in ((10, 40), (500, 520), (1500, 1990)):
        scores[a:b, 1] = 0.9
    x = torch.from_numpy(scores).to(gpu_device)
    on, zero = np.full(K, 0.5, dtype=np.float32), np.zeros(K, dtype=np.float64)
    need = lib.pa_binarize_regions_workspace_bytes(T, K, cap)

    def call(ws, nbytes, counts, regions, tracks):
        return lib.pa_binarize_regions(ffi.ptr(x), T, K, on.ctypes.data, on.ctypes.data, zero.ctypes.data,
                                       zero.ctypes.data, *FRAMES, cap, counts, regions, tracks, ws, nbytes, ffi.stream())

    counts, regions, tracks = _fills("pa_binarize_regions T=2001 K=2", call, need,
                                     [((K,), torch.int32, -77), ((K, cap, 2), torch.float64),
                                      ((K, cap), torch.int32, -77)], gpu_device)
    assert counts.tolist() == [1000, 3]
    for k in range(K):
        want, positions = mo.class_regions(scores[:, k], *FRAMES, 0.5, 0.5)
        got = regions[k, :counts[k]].numpy()
        assert np.array_equal(got.view(np.int64), np.array(want, dtype=np.float64).reshape(-1, 2).view(np.int64)), k
        assert tracks[k, :counts[k]].tolist() == [0] * len(want), k     # (no merging: every track position is 0)
    assert torch.isnan(regions[1, 3:]).all() and (tracks[1, 3:] == -77).all()


def test_regions_sweep(gpu_device):
    """one group of three lanes of one class; the counting phase answers on the host, so its fills are compared here"""
    import pyannote_audio_amd.ffi as ffi
    import regions_sweep_cases as rs
    lib = ffi.load()
    T, K = 1025, 1
    scores, lane_class, onset, offset, job_lane, d_on, d_off = rs.make_case(91, T, K, 3, 0.02)
    L, M = len(lane_class), len(job_lane)
    groups = int(lib.pa_regions_sweep_groups(K, L, lane_class.ctypes.data))
    assert groups == 1 and L == 3 and M == 6
    x = torch.from_numpy(scores).to(gpu_device)
    counted = {}
    need = int(lib.pa_regions_sweep_workspace_bytes(T, groups, groups, L, 0, 0, 0))
    _log("pa_regions_sweep_count", need)
    with torch.cuda.device(gpu_device):
        for fill in FILLS:
            ws = HostileWorkspace(need, gpu_device, fill)
            n_raw, launches = np.full(L, -7, dtype=np.int32), np.zeros(1, dtype=np.int32)
            rc = lib.pa_regions_sweep_count(ffi.ptr(x), T, K, L, lane_class.ctypes.data, onset.ctypes.data,
                                            offset.ctypes.data, n_raw.ctypes.data, launches.ctypes.data, ws.ptr,
                                            ws.nbytes, ffi.stream())
            assert rc == 0 and launches[0] == 1
            ws.check(f"pa_regions_sweep_count ({fill})")
            counted[fill] = n_raw
    assert all(np.array_equal(counted["zeros"], counted[fill]) for fill in FILLS) and counted["zeros"].min() > 0
    n_raw = counted["ones"]
    raw_rows, rows = int(n_raw.sum()), int(n_raw[job_lane].sum())
    need = int(lib.pa_regions_sweep_workspace_bytes(T, groups, groups, L, M, raw_rows, rows))

    def call(ws, nbytes, regions, tracks, job_off):
        launches = np.zeros(1, dtype=np.int32)
        return lib.pa_regions_sweep_emit(ffi.ptr(x), T, K, L, lane_class.ctypes.data, onset.ctypes.data,
                                         offset.ctypes.data, n_raw.ctypes.data, M, job_lane.ctypes.data,
                                         d_on.ctypes.data, d_off.ctypes.data, *rs.FRAMES, rows, regions, tracks, job_off,
                                         launches.ctypes.data, ws, nbytes, ffi.stream())

    regions, tracks, job_off = _fills("pa_regions_sweep_emit", call, need,
                                      [((rows, 2), torch.float64), ((rows,), torch.int32, -77),
                                       ((M + 1,), torch.int32, -77)], gpu_device)
    off = job_off.tolist()
    got = ([regions[a:b].numpy() for a, b in zip(off[:-1], off[1:])],
           [tracks[a:b].numpy() for a, b in zip(off[:-1], off[1:])])
    rs.assert_same(got, rs.truth(scores, lane_class, onset, offset, job_lane, d_on, d_off), "one group")


# ================================================================================================ exact kernels: VBx
def test_vbx_iteration(gpu_device):
    """one first = 1 iteration of the (257, 5, 129) shape of tests/vbx_truth.py through the harness (the NaN-filled
    runs of tests/test_vbx_kernels_gpu.py stay): gamma is read and updated in place.  (first = 0 is the one call that
    reads its workspace on purpose: rho and G of the first = 1 call before it, as the header says.)"""
    import pyannote_audio_amd.ffi as ffi
    from test_vbx_kernels_gpu import assert_parity64
    from vbx_truth import FA_FB, VBX_SHAPES, elbo_ratio, gamma_ratio, vbx_steps
    lib = ffi.load()
    (N, S, D), (Fa, Fb) = VBX_SHAPES[4], FA_FB[0]
    assert (N, S, D) == (257, 5, 129)
    fea, Phi, steps = vbx_steps(N, S, D, Fa, Fb, 400)
    tag, first, gamma_in, (truth_gamma, truth_elbo), (np_gamma, np_elbo) = steps[0]
    assert first == 1
    fea_d, phi_d = torch.from_numpy(np.ascontiguousarray(fea)).to(gpu_device), torch.from_numpy(Phi.copy()).to(gpu_device)
    need = lib.pa_vbx_workspace_bytes(N, S, D)

    def call(ws, nbytes, gamma, elbo):
        return lib.pa_vbx_iteration(ffi.ptr(fea_d), ffi.ptr(phi_d), N, S, D, float(Fa), float(Fb), 1, gamma, elbo, ws,
                                    nbytes, ffi.stream())

    gamma, elbo = _fills(f"pa_vbx_iteration N={N} S={S} D={D}", call, need,
                         [((N, S), torch.float64), ((1,), torch.float64)], gpu_device,
                         initial={0: torch.from_numpy(np.ascontiguousarray(gamma_in, dtype=np.float64))})
    assert_parity64("hostile vbx gamma", gamma_ratio(gamma.numpy(), truth_gamma), gamma_ratio(np_gamma, truth_gamma))
    assert_parity64("hostile vbx ELBO", elbo_ratio(float(elbo[0]), truth_elbo), elbo_ratio(np_elbo, truth_elbo))


def test_vbx_run_batch(gpu_device):
    """two jobs over the same features; per job, bit for bit what the loop of pa_vbx_iteration with the convergence
    test on the host gives (tests/test_vbx_batch_gpu.py)"""
    import pyannote_audio_amd.ffi as ffi
    from vbx_truth import vbx_inputs
    lib = ffi.load()
    N, S, D, iters, eps = 150, 4, 128, 8, 1e-4
    fea, Phi, gamma0 = vbx_inputs(N, S, D, seed=3)
    factors = [(0.07, 0.8), (0.4, 0.05)]
    J = len(factors)
    fea_d, phi_d = torch.from_numpy(np.ascontiguousarray(fea)).to(gpu_device), torch.from_numpy(Phi.copy()).to(gpu_device)
    g0 = torch.from_numpy(np.ascontiguousarray(gamma0, dtype=np.float64)).to(gpu_device)
    job_init = torch.tensor([[0, S]] * J, dtype=torch.int64, device=gpu_device)
    job_f = torch.tensor(factors, dtype=torch.float64, device=gpu_device)
    need = lib.pa_vbx_batch_workspace_bytes(J, N, S, D)

    def call(ws, nbytes, gamma, elbo, iterations):
        return lib.pa_vbx_run_batch(ffi.ptr(fea_d), ffi.ptr(phi_d), N, D, J, ffi.ptr(g0), g0.numel(),
                                    ffi.ptr(job_init), ffi.ptr(job_f), S, iters, eps, gamma, elbo, iterations, ws,
                                    nbytes, ffi.stream())

    gamma, elbo, iterations = _fills(f"pa_vbx_run_batch J={J} N={N} S={S}", call, need,
                                     [((J, N * S), torch.float64), ((J, iters), torch.float64),
                                      ((J,), torch.int32, -77)], gpu_device)
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
