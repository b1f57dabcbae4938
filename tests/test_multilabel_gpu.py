"""pa_binarize_regions, the device-resident aggregate and MultiLabelSegmentation on the GPU.

Region times are compared BIT FOR BIT everywhere; nothing is excused for sitting near a threshold: the end-to-end test
compares the pipeline's regions with the frame-by-frame helper applied to the pipeline's own hooked scores."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import multilabel_oracle as mo  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multilabel_v1.npz")
CLASSES = ["speech", "music", "noise"]
FRAMES = (0.0, 0.0619375, 0.016875)
TILE = 1024            # frames per workgroup in csrc/regions.hip


def run_kernel(device, scores, frames, onset, offset, d_on, d_off):
    from pyannote_audio_amd import frames as frame_ops
    from pyannote_audio_amd.core import SlidingWindow
    window = SlidingWindow(start=frames[0], duration=frames[1], step=frames[2])
    return frame_ops.binarize_regions(torch.from_numpy(scores).to(device), window, onset, offset, d_on, d_off,
                                      return_tracks=True)


def assert_same_regions(got, want, where):
    regions, positions = got
    for k, (want_regions, want_positions) in enumerate(want):
        w = np.array(want_regions, dtype=np.float64).reshape(-1, 2)
        assert regions[k].shape == w.shape, (where, k, regions[k].shape, w.shape)
        assert regions[k].dtype == np.float64
        assert np.array_equal(regions[k].view(np.int64), w.view(np.int64)), (where, k)
        assert positions[k].tolist() == list(want_positions), (where, k)


def test_kernel_reproduces_the_reference_recording(gpu_device):
    g = np.load(GOLDEN)
    for name in [str(c) for c in g["cases"]]:
        got = run_kernel(gpu_device, g[f"{name}/scores"], g[f"{name}/frames"], g[f"{name}/onset"], g[f"{name}/offset"],
                         g[f"{name}/min_duration_on"], g[f"{name}/min_duration_off"])
        for k in range(3):
            want = g[f"{name}/binarize{k}_times"]
            assert len(got[0][k]) == len(want), (name, k)
            assert np.array_equal(got[0][k].view(np.int64), want.view(np.int64)), (name, k)
            assert [mo.track_name(p) for p in got[1][k]] == [str(t) for t in g[f"{name}/binarize{k}_tracks"]], (name, k)


def grid_parameters(rng, K, order):
    low, high = rng.uniform(0.3, 0.45, K), rng.uniform(0.55, 0.7, K)
    onset, offset = (high, low) if order == "offset_below_onset" else (low, high)
    d_on = rng.choice([0.0, 0.05, 0.12], K)
    d_off = rng.choice([0.0, 0.04, 0.1], K)
    return onset, offset, d_on, d_off


@pytest.mark.parametrize("K", [1, 3, 4, 16])
def test_kernel_matches_the_helper_on_a_grid(gpu_device, K):
    rng = np.random.default_rng(100 + K)
    for T in (2, 3, TILE - 1, TILE, TILE + 1, 3 * TILE - 1, 3 * TILE + 1):
        for order in ("offset_below_onset", "offset_above_onset"):
            for nan_fraction in (0.0, 0.02, 1.0):
                scores = mo.smooth_scores(rng, T, K, width=int(rng.integers(1, 12)), nan_fraction=nan_fraction)
                onset, offset, d_on, d_off = grid_parameters(rng, K, order)
                want = mo.all_regions(scores, *FRAMES, onset, offset, d_on, d_off)
                got = run_kernel(gpu_device, scores, FRAMES, onset, offset, d_on, d_off)
                assert_same_regions(got, want, (T, K, order, nan_fraction))


@pytest.mark.parametrize("K,order", [(4, "offset_below_onset"), (16, "offset_above_onset")])
def test_kernel_matches_the_helper_on_an_audio_hour(gpu_device, K, order):
    rng = np.random.default_rng(7 + K)
    T = 213334
    scores = mo.smooth_scores(rng, T, K, width=25, nan_fraction=0.02 if K == 4 else 0.0)
    onset, offset, d_on, d_off = grid_parameters(rng, K, order)
    want = mo.all_regions(scores, *FRAMES, onset, offset, d_on, d_off)
    assert sum(len(r) for r, _ in want) > 1000
    assert_same_regions(run_kernel(gpu_device, scores, FRAMES, onset, offset, d_on, d_off), want, (T, K))


def test_fewer_than_two_frames_give_no_region(gpu_device):
    for T in (0, 1):
        regions, positions = run_kernel(gpu_device, np.full((T, 3), 0.9, dtype=np.float32), FRAMES, 0.5, 0.5, 0.0, 0.0)
        assert [len(r) for r in regions] == [0, 0, 0] and [len(p) for p in positions] == [0, 0, 0]


def test_capacity_too_small_is_reported_and_nothing_is_written_past_it(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    T, K, cap, guard = 2001, 2, 100, 64
    scores = np.full((T, K), 0.1, dtype=np.float32)
    scores[0::2, 0] = 0.9                       # class 0: 1000 regions; class 1: three
    for a, b in ((10, 40), (500, 520), (1500, 1990)):
        scores[a:b, 1] = 0.9
    x = torch.from_numpy(scores).to(gpu_device)
    sentinel = -12345.5
    regions = torch.full((K * cap * 2 + guard,), sentinel, dtype=torch.float64, device=gpu_device)
    tracks = torch.full((K * cap + guard,), -7, dtype=torch.int32, device=gpu_device)
    counts = torch.full((K + guard,), -7, dtype=torch.int32, device=gpu_device)
    nbytes = int(lib.pa_binarize_regions_workspace_bytes(T, K, cap))
    # (0xFF bytes, the `ones` fill of tests/hostile_workspace.py: NaN / -1 wherever the kernels read before they write)
    from hostile_workspace import fill_bytes
    workspace = fill_bytes("ones", nbytes + 8 * guard, gpu_device)
    workspace[nbytes:] = 0xA5
    on = np.full(K, 0.5, dtype=np.float32)
    zero = np.zeros(K, dtype=np.float64)
    rc = lib.pa_binarize_regions(ffi.ptr(x), T, K, on.ctypes.data, on.ctypes.data, zero.ctypes.data, zero.ctypes.data,
                                 *FRAMES, cap, ffi.ptr(counts), ffi.ptr(regions), ffi.ptr(tracks), ffi.ptr(workspace),
                                 nbytes, ffi.stream())
    torch.cuda.synchronize()
    assert rc != 0
    message = lib.pa_last_error().decode()
    assert "class 0" in message and "1000" in message and "capacity" in message
    with pytest.raises(ValueError, match="capacity"):
        ffi.check(rc, "pa_binarize_regions")
    r, t, c = regions.cpu().numpy(), tracks.cpu().numpy(), counts.cpu().numpy()
    assert (r[K * cap * 2:] == sentinel).all() and (t[K * cap:] == -7).all() and (c[K:] == -7).all()
    assert (workspace[nbytes:].cpu().numpy() == 0xA5).all()
    # class 1 starts right after class 0's `cap` slots: its three regions are intact and the rest of its slots untouched
    want, _ = mo.class_regions(scores[:, 1], *FRAMES, 0.5, 0.5)
    assert c[1] == 3 and c[0] <= cap
    second = r[cap * 2:K * cap * 2].reshape(cap, 2)
    assert np.array_equal(second[:3].view(np.int64), np.array(want).view(np.int64))
    assert (second[3:] == sentinel).all() and (t[cap + 3:K * cap] == -7).all()
    # the same call with room for everything succeeds
    from pyannote_audio_amd import frames as frame_ops
    from pyannote_audio_amd.core import SlidingWindow
    full = frame_ops.binarize_regions(x, SlidingWindow(*FRAMES[1:], FRAMES[0]), 0.5, 0.5)
    assert [len(f) for f in full] == [1000, 3]
    with pytest.raises(ValueError, match="capacity"):
        frame_ops.binarize_regions(x, SlidingWindow(*FRAMES[1:], FRAMES[0]), 0.5, 0.5, capacity=999)


# ------------------------------------------------------------------------------------------- model and pipeline
@pytest.fixture(scope="module")
def multilabel_setup(tmp_path_factory, gpu_device):
    """a multi-label checkpoint (three named classes, not permutation invariant) with the calibrated read-out of
    oracle.synthetic.calibrated_multilabel_pyannet, written in the reference's format, and its pipeline"""
    import yaml
    import pyannote_audio_amd as pa
    from conftest import PYANNET_HPARAMS
    from oracle.synthetic import calibrated_multilabel_pyannet
    from pyannote_audio_amd.model import Problem, PyanNet, Resolution, Specifications, save_checkpoint
    seg_o = calibrated_multilabel_pyannet(calib_seconds=40.0)
    root = tmp_path_factory.mktemp("multilabel")
    os.makedirs(root / "segmentation")
    spec = Specifications(problem=Problem.MULTI_LABEL_CLASSIFICATION, resolution=Resolution.FRAME, duration=10.0,
                          min_duration=None, warm_up=(0.0, 0.0), classes=list(CLASSES), permutation_invariant=False)
    save_checkpoint(str(root / "segmentation" / "pytorch_model.bin"), seg_o.state_dict(), PYANNET_HPARAMS,
                    PyanNet.ARCHITECTURE, spec)
    thresholds = {"speech": {"onset": 0.6, "offset": 0.4, "min_duration_on": 0.0, "min_duration_off": 0.0},
                  "music": {"onset": 0.4, "offset": 0.6, "min_duration_on": 0.05, "min_duration_off": 0.1},
                  "noise": {"onset": 0.5, "offset": 0.5, "min_duration_on": 0.1, "min_duration_off": 0.0}}
    config = {"version": "3.1.0",
              "pipeline": {"name": "pyannote.audio.pipelines.MultiLabelSegmentation",
                           "params": {"segmentation": "$model/segmentation"}},
              "params": {"thresholds": thresholds}}
    with open(root / "config.yaml", "w") as fp:
        yaml.safe_dump(config, fp)
    pipeline = pa.Pipeline.from_pretrained(str(root)).to(gpu_device)
    return seg_o, pipeline, thresholds


@pytest.mark.parametrize("seconds", [23.0, 27.43])      # without / with a last, zero-padded chunk
def test_device_aggregate_is_the_host_aggregate(multilabel_setup, gpu_device, seconds):
    from oracle.synthetic import synth_conversation
    _, pipeline, _ = multilabel_setup
    inference = pipeline._segmentation
    wav, _ = synth_conversation(seconds, seed=21)
    host = inference.slide(wav, 16000)
    device, frames = inference.slide_device(wav, 16000)
    assert device.is_cuda and device.dtype == torch.float32 and device.is_contiguous()
    got = device.cpu().numpy()
    assert got.shape == host.data.shape
    assert np.array_equal(got.view(np.int32), np.ascontiguousarray(host.data).view(np.int32))
    window = host.sliding_window
    assert (frames.start, frames.duration, frames.step) == (window.start, window.duration, window.step)
    n, has_last = inference.num_chunks(wav.shape[1], 160000, 16000)
    assert has_last == (seconds != 23.0)
    # frames.aggregate (host result) and frames.aggregate_device on the same chunk scores
    from pyannote_audio_amd import frames as frame_ops
    from pyannote_audio_amd.core import SlidingWindow
    chunks = SlidingWindow(start=0.0, duration=10.0, step=1.0)
    scores = inference.last_device_output
    a = frame_ops.aggregate(scores, chunks, inference.model.receptive_field, gpu_device, hamming=True, missing=0.0)
    b, _ = frame_ops.aggregate_device(scores, chunks, inference.model.receptive_field, gpu_device, hamming=True,
                                      missing=0.0)
    assert np.array_equal(a.data.view(np.int32), b.cpu().numpy().view(np.int32))


@pytest.mark.parametrize("seconds,seed", [(23.0, 14), (27.43, 5)])
def test_pipeline_end_to_end(multilabel_setup, gpu_device, seconds, seed):
    from conftest import north_star_ratio
    from oracle.pipeline import SW, aggregate, receptive_field, slide
    from oracle.synthetic import synth_conversation
    seg_o, pipeline, thresholds = multilabel_setup
    wav, _ = synth_conversation(seconds, seed=seed)
    file = {"waveform": wav, "sample_rate": 16000, "uri": f"conv{seed}"}
    seen, progress = {}, []

    def hook(name, artefact, file=None, **kw):
        if artefact is not None:
            seen[name] = artefact
        else:
            progress.append((kw.get("completed"), kw.get("total")))

    hooked = pipeline(dict(file), hook=hook)
    scores = seen["segmentation"]
    assert isinstance(scores.data, np.ndarray) and scores.data.dtype == np.float32 and scores.data.shape[1] == 3
    assert progress and progress[-1][0] == progress[-1][1]

    # (a) the aggregated scores against the oracle's slide -> aggregate
    chunk_scores = slide(seg_o, wav, 16000, 10.0, 1.0)
    want, want_frames = aggregate(chunk_scores, SW(0.0, 10.0, 1.0), receptive_field(seg_o), hamming=True, missing=0.0)
    window = scores.sliding_window
    assert (window.start, window.duration, window.step) == (want_frames.start, want_frames.duration, want_frames.step)
    assert len(scores.data) <= len(want) and len(want) - len(scores.data) < 589
    assert north_star_ratio(f"multilabel_aggregate_{seconds:g}s", scores.data, want[:len(scores.data)]) <= 1.0

    # (b) the regions against the helper on the pipeline's own scores: exactly
    order = [thresholds[c] for c in CLASSES]
    assert any(t["offset"] > t["onset"] for t in order)
    per_class = mo.all_regions(scores.data, window.start, window.duration, window.step,
                               [t["onset"] for t in order], [t["offset"] for t in order],
                               [t["min_duration_on"] for t in order], [t["min_duration_off"] for t in order])
    rows = mo.annotation_rows(hooked)
    assert rows == mo.triples(per_class, CLASSES)
    assert hooked.uri == file["uri"] and len(rows) >= 3
    assert set(hooked.labels()) <= set(CLASSES) and len(set(hooked.labels())) >= 2

    # without a hook: the same annotation, and no score array handed out
    plain = pipeline(dict(file))
    assert mo.annotation_rows(plain) == rows and plain.uri == hooked.uri


def test_training_mode_caches_the_scores(multilabel_setup):
    from oracle.synthetic import synth_conversation
    _, pipeline, _ = multilabel_setup
    wav, _ = synth_conversation(12.5, seed=2)
    file = {"waveform": wav, "sample_rate": 16000, "uri": "cached"}
    want = mo.annotation_rows(pipeline(dict(file)))
    pipeline.training = True
    try:
        first = pipeline.apply(file)
        cached = file[pipeline.CACHED_SEGMENTATION]
        assert isinstance(cached.data, np.ndarray)
        file["waveform"] = None                              # the second run must not need the audio
        second = pipeline.apply(file)
    finally:
        pipeline.training = False
    assert mo.annotation_rows(first) == want and mo.annotation_rows(second) == want
