"""The size and frame functions of the forward entry points (csrc/*_forward.cpp) return what they returned before the
entry points shared their SincNet, LSTM-head and TDNN plans: tests/golden/forward_plans_v1.json holds the values of
`table()` below as the library at the commit before that change computed them
(tests/golden/make_forward_plans_golden.py).
None of these functions takes a device pointer, so the weight structs carry their integer fields only and no GPU is
needed."""
import itertools
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_plans_v1.json")

BATCHES = (1, 16, 17, 33)
FIXED_SAMPLES = (16000, 80000, 160000)
SINC_STRIDES = (10, 5, 16)
LSTMS = ((128, 1, 4), (48, 1, 2), (32, 0, 1), (512, 1, 1))     # (hidden, bidirectional, layers)
LINEARS = ((2, 128), (0, 0))                                    # (layers, width)
MASKS = (1, 3)
TDNN = ((512, 512, 512, 512, 1500), (5, 3, 3, 1, 1), (1, 2, 3, 1, 1))   # channels, kernel, dilation (weights.py)
# (extractor convolutions (channels, kernel, stride), embed_dim, heads, ff_dim, layers) of tests/test_sseriouss_gpu.py
_TINY_CONV = ((64, 10, 5), (64, 3, 2), (64, 3, 2), (64, 2, 2))
ENCODERS = {
    "wavlm_base": (((512, 10, 5),) + ((512, 3, 2),) * 4 + ((512, 2, 2),) * 2, 768, 12, 3072, 12),
    "tiny": (_TINY_CONV, 128, 4, 256, 3),
    "tiny_group_norm_post_ln": (_TINY_CONV, 96, 3, 256, 3),
}
# (bottleneck, blocks per layer, planes) as tests/test_emb_gpu.py builds its networks
RESNETS = {
    "resnet34": (0, (3, 4, 6, 3), (32, 64, 128, 256)),
    "bottleneck_1111": (1, (1, 1, 1, 1), (32, 64, 128, 256)),
    "bottleneck_2322": (1, (2, 3, 2, 2), (32, 64, 128, 256)),
}


def _head(w, lstm, linear):
    w.lstm_hidden, w.lstm_bidir, w.lstm_layers = lstm
    w.num_linear, w.linear_hidden = linear
    w.num_classes, w.num_speakers = 7, 3
    return w


def seg_weights(ffi, sinc_stride, lstm, linear):
    w = ffi.SegWeights()
    w.sinc_stride = sinc_stride
    return _head(w, lstm, linear)


def sser_weights(ffi, name, lstm, linear):
    conv, dim, heads, ff, layers = ENCODERS[name]
    w = ffi.SserWeights()
    w.num_conv = len(conv)
    for i, (c, k, s) in enumerate(conv):
        w.conv_channels[i], w.conv_kernel[i], w.conv_stride[i] = c, k, s
    w.embed_dim, w.num_heads, w.ff_dim, w.num_layers = dim, heads, ff, layers
    return _head(w, lstm, linear)


def _tdnn(w):
    for l in range(5):
        w.tdnn_channels[l], w.tdnn_kernel[l], w.tdnn_dilation[l] = (TDNN[i][l] for i in range(3))
    w.dimension = 512
    return w


def xvec_weights(ffi, sinc_stride):
    w = ffi.XvecWeights()
    w.sinc_stride = sinc_stride
    return _tdnn(w)


def mfcc_weights(ffi, center):
    w = ffi.XvecMfccWeights()
    w.n_fft, w.hop_length, w.center, w.log_mels, w.n_mels, w.n_mfcc = 400, 200, center, 0, 128, 40
    return _tdnn(w)


def emb_weights(ffi, name):
    bottleneck, blocks, planes = RESNETS[name]
    w = ffi.EmbWeights()
    w.num_mel, w.embed_dim, w.num_layers, w.bottleneck = 80, 256, 4, bottleneck
    for l in range(4):
        w.num_blocks[l], w.planes[l] = blocks[l], planes[l]
    return w


def first_accepted(frames):
    """the smallest sample count with at least one output frame (bisection: `frames` is monotone)"""
    lo, hi = 1, 160000
    assert frames(lo) == 0 and frames(hi) > 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if frames(mid) > 0 else (mid, hi)
    return hi


def samples(frames):
    """[smallest accepted, the one below it (the largest refused), 16 000, 80 000, 160 000]"""
    n = first_accepted(frames)
    return (n, n - 1) + FIXED_SAMPLES


def chunk_strides(n):
    """the chunk itself, a tenth of it, a stride that is no multiple of 10, none"""
    odd = n // 10 + 5 if (n // 10 + 5) % 10 else n // 10 + 6
    return (n, n // 10, odd, 0)


def table(lib, ffi):
    """{function: [[arguments ..., value], ...]}; weight structs appear as the names / tuples they were built from"""
    from ctypes import byref
    t = {name: [] for name in (
        "pa_seg_num_frames", "pa_seg_workspace_bytes", "pa_seg_workspace_bytes_strided", "pa_sser_num_frames",
        "pa_sser_workspace_bytes", "pa_xvec_num_frames", "pa_xvec_workspace_bytes", "pa_xvec_mfcc_num_frames",
        "pa_xvec_mfcc_workspace_bytes", "pa_emb_num_pool_frames", "pa_emb_workspace_bytes",
        "pa_emb_ragged_workspace_bytes", "pa_emb_calibrate_workspace_bytes")}
    heads = list(itertools.product(LSTMS, LINEARS))
    for s in SINC_STRIDES:
        for n in samples(lambda n: lib.pa_seg_num_frames(n, s)):
            t["pa_seg_num_frames"].append([n, s, lib.pa_seg_num_frames(n, s)])
            for (lstm, linear), B in itertools.product(heads, BATCHES):
                w = seg_weights(ffi, s, lstm, linear)
                t["pa_seg_workspace_bytes"].append([s, lstm, linear, B, n, lib.pa_seg_workspace_bytes(byref(w), B, n)])
                for stride in chunk_strides(n):
                    t["pa_seg_workspace_bytes_strided"].append(
                        [s, lstm, linear, B, n, stride, lib.pa_seg_workspace_bytes_strided(byref(w), B, n, stride)])
        w = xvec_weights(ffi, s)
        for n in samples(lambda n: lib.pa_xvec_num_frames(byref(w), n)):
            t["pa_xvec_num_frames"].append([s, n, lib.pa_xvec_num_frames(byref(w), n)])
            for B, S in itertools.product(BATCHES, MASKS):
                t["pa_xvec_workspace_bytes"].append([s, B, n, S, lib.pa_xvec_workspace_bytes(byref(w), B, n, S)])
    for name in ENCODERS:
        w = sser_weights(ffi, name, LSTMS[0], LINEARS[0])
        for n in samples(lambda n: lib.pa_sser_num_frames(byref(w), n)):
            t["pa_sser_num_frames"].append([name, n, lib.pa_sser_num_frames(byref(w), n)])
            for (lstm, linear), B in itertools.product(heads, BATCHES):
                wh = sser_weights(ffi, name, lstm, linear)
                t["pa_sser_workspace_bytes"].append(
                    [name, lstm, linear, B, n, lib.pa_sser_workspace_bytes(byref(wh), B, n)])
    for center in (1, 0):
        w = mfcc_weights(ffi, center)
        for n in samples(lambda n: lib.pa_xvec_mfcc_num_frames(byref(w), n)):
            t["pa_xvec_mfcc_num_frames"].append([center, n, lib.pa_xvec_mfcc_num_frames(byref(w), n)])
            for B, S in itertools.product(BATCHES, MASKS):
                t["pa_xvec_mfcc_workspace_bytes"].append(
                    [center, B, n, S, lib.pa_xvec_mfcc_workspace_bytes(byref(w), B, n, S)])
    for name in RESNETS:
        w = emb_weights(ffi, name)
        for n in samples(lambda n: lib.pa_emb_num_pool_frames(byref(w), n)):
            t["pa_emb_num_pool_frames"].append([name, n, lib.pa_emb_num_pool_frames(byref(w), n)])
            for B in BATCHES:
                for S in MASKS:
                    t["pa_emb_workspace_bytes"].append([name, B, n, S, lib.pa_emb_workspace_bytes(byref(w), B, n, S)])
                t["pa_emb_ragged_workspace_bytes"].append(
                    [name, B, n, lib.pa_emb_ragged_workspace_bytes(byref(w), B, n)])
                t["pa_emb_calibrate_workspace_bytes"].append(
                    [name, B, n, lib.pa_emb_calibrate_workspace_bytes(byref(w), B, n)])
    return json.loads(json.dumps(t))     # tuples -> lists, as the golden file holds them


@pytest.fixture(scope="module")
def library():
    import __graft_entry__
    __graft_entry__.build()
    import pyannote_audio_amd.ffi as ffi
    return ffi.load(), ffi


@pytest.fixture(scope="module")
def plans(library):
    return table(*library)


with open(GOLDEN) as _fp:
    _GOLDEN = json.load(_fp)


@pytest.mark.parametrize("function", sorted(_GOLDEN))
def test_plan_function_returns_the_recorded_values(plans, function):
    want, got = _GOLDEN[function], plans[function]
    assert len(got) == len(want) and len(want) > 0
    # the same cases (the smallest accepted sample counts included), then the same values
    assert [row[:-1] for row in got] == [row[:-1] for row in want]
    wrong = [(g, w[-1]) for g, w in zip(got, want) if g[-1] != w[-1]]
    assert not wrong, f"{len(wrong)} of {len(want)} differ; first (case + got, recorded): {wrong[:3]}"


def test_the_sample_below_the_smallest_is_refused_by_every_function(plans):
    """per model the table holds the first sample count with a frame and the one below it: there every size function
    returns 0, and nowhere else"""
    assert sorted(plans) == sorted(_GOLDEN)
    # (function prefix, its frame function, column of the sample count in the frame / the size functions)
    families = (("pa_seg_", "pa_seg_num_frames", 0, 4), ("pa_sser_", "pa_sser_num_frames", 1, 4),
                ("pa_xvec_mfcc_", "pa_xvec_mfcc_num_frames", 1, 2), ("pa_xvec_", "pa_xvec_num_frames", 1, 2),
                ("pa_emb_", "pa_emb_num_pool_frames", 1, 2))
    seen = set()
    for prefix, frame_function, col, size_col in families:
        model = lambda row, c: row[1] if frame_function == "pa_seg_num_frames" and c == 0 else row[0]
        frames = {(model(row, col), row[col]): row[-1] for row in plans[frame_function]}
        small = [(m, n) for m, n in frames if n not in FIXED_SAMPLES]
        assert small and all((frames[m, n] == 0) == ((m, n + 1) in frames and frames[m, n + 1] > 0) for m, n in small)
        for function in plans:
            if function.startswith(prefix) and function != frame_function and function not in seen:
                seen.add(function)
                for row in plans[function]:
                    assert (row[-1] == 0) == (frames[row[0], row[size_col]] == 0), (function, row)
        seen.add(frame_function)
    assert seen == set(plans)


@pytest.mark.parametrize("sinc_stride", SINC_STRIDES)
def test_seg_num_frames_is_the_conv_arithmetic(library, sinc_stride):
    from pyannote_audio_amd.model import multi_conv_num_frames
    lib, _ = library
    conv = ([251, 3, 5, 3, 5, 3], [sinc_stride, 3, 1, 3, 1, 3], [0] * 6, [1] * 6)
    for n in range(240, 2001):
        assert lib.pa_seg_num_frames(n, sinc_stride) == max(0, multi_conv_num_frames(n, *conv)), n
