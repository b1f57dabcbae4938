"""GPU: VoiceActivityDetection and MultiLabelSegmentation on a list of files in packed launches.

Every comparison is exact (`==`, `torch.equal`, `np.array_equal` on the bit patterns); there are no tolerances:

* `frames.aggregate_files` (`pa_aggregate_files`) against `frames.aggregate_device` file by file;
* `frames.binarize_regions_files` (`pa_binarize_regions_files_count` / `_emit`) against `frames.binarize_regions` file
  by file and against tests/multilabel_oracle.py file by file;
* hostile workspace contents and the refusals of the C ABI;
* `SegmentationEngine.forward_files` on a multi-label checkpoint against `forward_strided` file by file;
* `pipeline(files, pack=...)` against `[pipeline(f) for f in files]` for both pipelines, the groups it formed and the
  calls that take the per-file loop."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import detection_batch_cases as cases  # noqa: E402
import multilabel_oracle as mo  # noqa: E402
import regions_files_model as model  # noqa: E402

pytestmark = pytest.mark.gpu

SECONDS = [0.7, 10.0, 10.5, 23.0, 27.43]
CLASSES = ["speech", "music", "noise"]


def _window(triple):
    from pyannote_audio_amd.core import SlidingWindow
    return SlidingWindow(start=triple[0], duration=triple[1], step=triple[2])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ aggregate_files
@pytest.fixture(scope="module")
def aggregate_layout():
    """chunk0, row0, T of the four files: T is what the chunks cover, and a strict prefix of it for files 1 and 2"""
    from pyannote_audio_amd import frames as frame_ops
    chunks, frames = _window(cases.AGG_CHUNKS), _window(cases.FRAMES)
    covered = [frame_ops.frame_geometry(chunks, frames, c)[1] for c in cases.AGG_COUNTS]
    T = np.array([covered[0], covered[1] - 37, covered[2] - 290, covered[3]], dtype=np.int32)
    chunk0 = np.concatenate([[0], np.cumsum(cases.AGG_COUNTS)]).astype(np.int32)
    return chunk0, model.layout(T), T, covered


@pytest.mark.parametrize("kind", ["classes", "any", "hard"])
def test_aggregate_files_is_aggregate_device_per_file(gpu_device, aggregate_layout, kind):
    from pyannote_audio_amd import frames as frame_ops
    chunk0, row0, T, covered = aggregate_layout
    chunks, frames = _window(cases.AGG_CHUNKS), _window(cases.FRAMES)
    kw = dict(warm_up=cases.AGG_WARM_UP, hamming=True, missing=0.0)
    host = cases.aggregate_scores(kind)
    collapse = kind != "classes"
    if kind == "any":
        assert np.isnan(host).any(axis=-1).any() and not np.isnan(host).all(axis=-1).all()
    x = torch.from_numpy(host.copy()).to(gpu_device)

    def alone(f, scores):
        """file f by the single-file kernel, collapsed first as VoiceActivityDetection's hook does it"""
        mine = scores[chunk0[f]:chunk0[f + 1]].astype(np.float32)
        if collapse:
            mine = np.max(mine, axis=-1, keepdims=True)
        out, grid = frame_ops.aggregate_device(mine, chunks, frames, gpu_device, **kw)
        assert out.shape[0] == covered[f]
        return out.cpu().numpy(), grid

    packed, grid = frame_ops.aggregate_files(x, chunk0, row0, T, chunks, frames, any=collapse, packed=True, **kw)
    assert packed.shape == (int(row0[-1]), 1 if collapse else cases.AGG_S) and packed.dtype == torch.float32
    got = packed.cpu().numpy()
    owned = np.zeros(len(got), dtype=bool)
    for f in range(len(T)):
        want, want_grid = alone(f, host)
        assert np.array_equal(_bits(got[row0[f]:row0[f] + T[f]]), _bits(want[:T[f]])), (kind, f)
        assert (grid.start, grid.duration, grid.step) == (want_grid.start, want_grid.duration, want_grid.step)
        owned[row0[f]:row0[f] + T[f]] = True
    assert (~owned).any() and np.isnan(got[~owned]).all() and (kind == "hard" or (got[owned] == 0.0).any())
    # the per-file views are the same rows
    views, _ = frame_ops.aggregate_files(x, chunk0, row0, T, chunks, frames, any=collapse, **kw)
    assert [tuple(v.shape) for v in views] == [(t, packed.shape[1]) for t in T]
    assert all(torch.equal(v, packed[a:a + t]) for v, a, t in zip(views, row0[:-1], T))
    # file f + 1 does not depend on file f: every file in turn replaced by NaN (zeros for the hard decisions)
    for f in range(len(T) - 1):
        other = host.copy()
        other[chunk0[f]:chunk0[f + 1]] = 0 if kind == "hard" else np.nan
        again, _ = frame_ops.aggregate_files(torch.from_numpy(other).to(gpu_device), chunk0, row0, T, chunks, frames,
                                             any=collapse, packed=True, **kw)
        again = again.cpu().numpy()
        keep = np.ones(len(got), dtype=bool)
        keep[row0[f]:row0[f + 1]] = False
        assert np.array_equal(_bits(again[keep]), _bits(got[keep])), (kind, f)
        if kind != "hard":
            assert (again[row0[f]:row0[f] + T[f]] == 0.0).all()         # nobody voted: `missing`


def test_aggregate_files_refusals(gpu_device, aggregate_layout):
    from pyannote_audio_amd import frames as frame_ops
    chunk0, row0, T, _ = aggregate_layout
    chunks, frames = _window(cases.AGG_CHUNKS), _window(cases.FRAMES)
    hard = torch.from_numpy(cases.aggregate_scores("hard").copy()).to(gpu_device)
    with pytest.raises(ValueError, match="any"):
        frame_ops.aggregate_files(hard, chunk0, row0, T, chunks, frames)
    soft = torch.from_numpy(cases.aggregate_scores("classes").copy()).to(gpu_device)
    with pytest.raises(ValueError, match="chunk0"):
        frame_ops.aggregate_files(soft, chunk0[:-1], row0, T, chunks, frames)
    with pytest.raises(ValueError, match="cover fewer"):
        frame_ops.aggregate_files(soft, chunk0, row0 + np.arange(5, dtype=np.int32) * 64, T + 1, chunks, frames)
    with pytest.raises(ValueError, match="multiples of 64"):
        frame_ops.aggregate_files(soft, chunk0, row0 + 1, T, chunks, frames)


# ----------------------------------------------------------------------------------------- binarize_regions_files
@pytest.fixture(scope="module")
def region_inputs(gpu_device):
    """per K: the files, their layout and the packed device scores (0.95 in the padding: a padding row that counted
    would open or extend a region)"""
    out = {}
    for K in (1, 3, 16):
        files = cases.region_files(K)
        T = np.array([len(x) for x in files], dtype=np.int32)
        row0 = model.layout(T)
        out[K] = (files, row0, T, torch.from_numpy(model.pack(files, row0, fill=0.95)).to(gpu_device))
    return out


@pytest.mark.parametrize("name", [p[0] for p in cases.REGION_PARAMETERS])
@pytest.mark.parametrize("K", [1, 3, 16])
def test_binarize_regions_files_against_two_truths(gpu_device, region_inputs, K, name):
    from pyannote_audio_amd import frames as frame_ops
    files, row0, T, packed = region_inputs[K]
    window = _window(cases.FRAMES)
    params = cases.region_parameters(name, K)
    got = frame_ops.binarize_regions_files(packed, row0, T, window, *params, return_tracks=True)
    # (a) the per-file helper, written from the rule
    cases.assert_same_lists(got, cases.oracle_per_file(files, *params), ("oracle", K, name))
    # (b) the single-file kernel on every file's rows alone
    for f, x in enumerate(files):
        regions, positions = frame_ops.binarize_regions(torch.from_numpy(np.array(x)).to(gpu_device), window, *params,
                                                        return_tracks=True)
        for k in range(K):
            assert got[0][f][k].dtype == np.float64 and got[0][f][k].shape == regions[k].shape, (K, name, f, k)
            assert np.array_equal(_bits(got[0][f][k]), _bits(regions[k])), (K, name, f, k)
            assert got[1][f][k].tolist() == positions[k].tolist(), (K, name, f, k)
    # without tracks: the same rows
    plain = frame_ops.binarize_regions_files(packed, row0, T, window, *params)
    assert all(np.array_equal(_bits(a), _bits(b)) for fa, fb in zip(plain, got[0]) for a, b in zip(fa, fb))
    # neighbours: file 3 ends active, file 4 starts active -- two regions, each in its own file's time
    if name != "offset_above_onset":
        assert got[0][3][0][-1, 1] == mo.frame_middle(63, *cases.FRAMES)
        assert got[0][4][0][0, 0] == mo.frame_middle(0, *cases.FRAMES)
    assert all(len(r) == 0 for r in got[0][0] + got[0][6]) and len(got[0][2][0]) == 0


def test_no_file_and_files_without_frames(gpu_device):
    from pyannote_audio_amd import frames as frame_ops
    window = _window(cases.FRAMES)
    empty = torch.zeros((0, 2), dtype=torch.float32, device=gpu_device)
    assert frame_ops.binarize_regions_files(empty, [0], [], window, 0.5, 0.5) == []
    regions, tracks = frame_ops.binarize_regions_files(empty, [0, 0, 0], [0, 0], window, 0.5, 0.5, return_tracks=True)
    assert [[len(r) for r in f] for f in regions] == [[0, 0], [0, 0]] == [[len(t) for t in f] for f in tracks]
    # a file without frames between two that have some
    x = np.full((192, 1), 0.9, dtype=np.float32)
    regions = frame_ops.binarize_regions_files(torch.from_numpy(x).to(gpu_device), [0, 64, 128, 192], [40, 0, 64],
                                               window, 0.5, 0.5)
    want = [[mo.frame_middle(0, *cases.FRAMES), mo.frame_middle(t - 1, *cases.FRAMES)] for t in (40, 64)]
    assert regions[0][0].tolist() == [want[0]] and len(regions[1][0]) == 0 and regions[2][0].tolist() == [want[1]]


def _regions_call(lib, ffi, x, K, row0, T, params, n_raw, rows_out, nbytes_of=None):
    """-> emit(ws, nbytes, regions, tracks, list_off) on host tables that outlive the call"""
    onset, offset, d_on, d_off = (np.ascontiguousarray(p, dtype=t) for p, t in
                                  zip(params, (np.float32, np.float32, np.float64, np.float64)))
    row0, T = np.ascontiguousarray(row0, dtype=np.int32), np.ascontiguousarray(T, dtype=np.int32)
    n_raw = np.ascontiguousarray(n_raw, dtype=np.int32)
    keep = (onset, offset, d_on, d_off, row0, T, n_raw)

    def emit(ws, nbytes, regions, tracks, list_off, grid=cases.FRAMES):
        assert keep
        return lib.pa_binarize_regions_files_emit(
            ffi.ptr(x), K, len(T), row0.ctypes.data, T.ctypes.data, onset.ctypes.data, offset.ctypes.data,
            d_on.ctypes.data, d_off.ctypes.data, *[float(g) for g in grid], n_raw.ctypes.data, rows_out, regions,
            tracks, list_off, ws, nbytes, ffi.stream())

    def count(ws, nbytes, out):
        return lib.pa_binarize_regions_files_count(ffi.ptr(x), K, len(T), row0.ctypes.data, T.ctypes.data,
                                                   onset.ctypes.data, offset.ctypes.data, out.ctypes.data, ws, nbytes,
                                                   ffi.stream())
    return count, emit


def _counted(lib, ffi, x, K, row0, T, params):
    count, _ = _regions_call(lib, ffi, x, K, row0, T, params, np.zeros(16), 0)
    nbytes = int(lib.pa_binarize_regions_files_workspace_bytes(x.shape[0], K, len(T), 0))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    n_raw = np.full(K, -1, dtype=np.int32)
    assert count(ffi.ptr(ws), nbytes, n_raw) == 0
    return n_raw


def test_hostile_workspace_contents(gpu_device, region_inputs):
    import pyannote_audio_amd.ffi as ffi
    from hostile_workspace import HostileWorkspace, run_under_fills
    lib = ffi.load()
    K = 3
    files, row0, T, x = region_inputs[K]
    params = cases.region_parameters("offset_is_onset", K)
    # the counting phase: the same counts whatever the workspace held
    need = int(lib.pa_binarize_regions_files_workspace_bytes(x.shape[0], K, len(T), 0))
    count, _ = _regions_call(lib, ffi, x, K, row0, T, params, np.zeros(16), 0)
    seen = []
    for fill in ("zeros", "ones", "huge"):
        ws = HostileWorkspace(need, gpu_device, fill)
        n_raw = np.full(K, -1, dtype=np.int32)
        assert count(ws.ptr, ws.nbytes, n_raw) == 0
        ws.check(f"pa_binarize_regions_files_count ({fill})")
        seen.append(n_raw.tolist())
    assert seen[0] == seen[1] == seen[2] and min(seen[0]) > 0
    raw = cases.oracle_per_file(files, params[0], params[1], 0.0, 0.0)       # (before clean-up: nothing is empty here)
    assert seen[0] == [sum(len(per_class[k][0]) for per_class in raw) for k in range(K)]
    # the emitting phase
    n_raw = np.array(seen[0], dtype=np.int32)
    rows = int(n_raw.sum())
    need = int(lib.pa_binarize_regions_files_workspace_bytes(x.shape[0], K, len(T), rows))
    _, emit = _regions_call(lib, ffi, x, K, row0, T, params, n_raw, rows)
    lists = len(T) * K
    regions, tracks, list_off = run_under_fills(
        emit, need, [((rows, 2), torch.float64), ((rows,), torch.int32, -7), ((lists + 1,), torch.int32, -7)],
        gpu_device, "pa_binarize_regions_files_emit")
    off = list_off.numpy()
    got = ([[regions.numpy()[off[f * K + k]:off[f * K + k + 1]] for k in range(K)] for f in range(len(T))],
           [[tracks.numpy()[off[f * K + k]:off[f * K + k + 1]] for k in range(K)] for f in range(len(T))])
    cases.assert_same_lists(got, cases.oracle_per_file(files, *params), "hostile workspace")
    assert (tracks.numpy()[off[-1]:] == -7).all() and np.isnan(regions.numpy()[off[-1]:]).all()


def test_refusals_leave_the_outputs_untouched(gpu_device, region_inputs):
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd import frames as frame_ops
    from kernel_parity import Guarded
    lib = ffi.load()
    K = 3
    files, row0, T, x = region_inputs[K]
    good = cases.region_parameters("offset_is_onset", K)
    n_raw = _counted(lib, ffi, x, K, row0, T, good)
    rows = int(n_raw.sum())
    need = int(lib.pa_binarize_regions_files_workspace_bytes(x.shape[0], K, len(T), rows))
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    nan = float("nan")

    def with_nan(which):
        p = [np.array(v, dtype=np.float64) for v in good]
        p[which][1] = nan
        return p

    wide = np.concatenate([row0, row0[-1] + 64 * np.arange(1, 65536 - len(T) + 1, dtype=np.int64)]).astype(np.int32)
    shifted = row0.copy()
    shifted[4] -= 32                                               # still non-decreasing, no multiple of 64
    swapped = row0.copy()
    swapped[5] = swapped[3]                                        # decreases
    long_file = T.copy()
    long_file[2] = 65                                              # file 2 owns 64 rows
    refused = {
        "no class": dict(K=0), "17 classes": dict(K=17),
        "NaN onset": dict(params=with_nan(0)), "NaN offset": dict(params=with_nan(1)),
        "NaN min_duration_on": dict(params=with_nan(2)), "NaN min_duration_off": dict(params=with_nan(3)),
        "row0 decreases": dict(row0=swapped), "row0 no multiple of 64": dict(row0=shifted),
        "a file keeps more than it owns": dict(T=long_file), "negative T": dict(T=np.where(T == 63, -1, T)),
        "65536 files": dict(row0=wide, T=np.zeros(65536, dtype=np.int32)),
        "small workspace": dict(nbytes=need - 1),
    }
    for what, change in refused.items():
        k = change.get("K", K)
        pad = lambda p: [np.resize(np.asarray(v), max(k, 1)) for v in p]
        use_row0, use_T = change.get("row0", row0), change.get("T", T)
        count, emit = _regions_call(lib, ffi, x, k, use_row0, use_T, pad(change.get("params", good)),
                                    np.resize(n_raw, 17), rows)
        outs = [Guarded(2 * rows, gpu_device, torch.float64), Guarded(rows, gpu_device, torch.int32),
                Guarded(len(use_T) * max(k, 1) + 1, gpu_device, torch.int32)]
        rc = emit(ffi.ptr(ws), change.get("nbytes", need), *[g.ptr for g in outs])
        assert rc == 3, (what, rc)
        with pytest.raises(ValueError):
            ffi.check(rc, what)
        assert all(g.untouched() for g in outs), what
        # the counting phase refuses the same tables (it takes no durations)
        if "min_duration" not in what:
            counted = np.full(17, -5, dtype=np.int32)
            small = int(lib.pa_binarize_regions_files_workspace_bytes(x.shape[0], K, len(T), 0))
            rc = count(ffi.ptr(ws), small - 1 if what == "small workspace" else need, counted)
            assert rc == 3 and (counted == -5).all(), (what, rc)
    # a NaN in the frame grid, and counts that are not those of the scores
    _, emit = _regions_call(lib, ffi, x, K, row0, T, good, n_raw, rows)
    outs = [Guarded(2 * rows, gpu_device, torch.float64), Guarded(rows, gpu_device, torch.int32),
            Guarded(len(T) * K + 1, gpu_device, torch.int32)]
    assert emit(ffi.ptr(ws), need, *[g.ptr for g in outs], grid=(0.0, nan, 0.016875)) == 3
    assert all(g.untouched() for g in outs)
    fewer = n_raw.copy()
    fewer[1] -= 1
    _, emit = _regions_call(lib, ffi, x, K, row0, T, good, fewer, rows)
    rc = emit(ffi.ptr(ws), need, *[g.ptr for g in outs])
    torch.cuda.synchronize()
    assert rc == 3 and "class 1" in lib.pa_last_error().decode()
    assert lib.pa_binarize_regions_files_workspace_bytes(64, 17, 1, 0) == 0
    # the Python layer refuses the same before it calls
    window = _window(cases.FRAMES)
    for bad in (dict(row0=swapped), dict(row0=shifted), dict(T=long_file)):
        with pytest.raises(ValueError):
            frame_ops.binarize_regions_files(x, bad.get("row0", row0), bad.get("T", T), window, *good)
    with pytest.raises(ValueError, match="NaN"):
        frame_ops.binarize_regions_files(x, row0, T, window, *with_nan(2))
    with pytest.raises(ValueError, match="classes"):
        frame_ops.binarize_regions_files(torch.zeros((64, 17), device=gpu_device), [0, 64], [64], window, 0.5, 0.5)


# --------------------------------------------------------------------------------------------- model and pipelines
@pytest.fixture(scope="module")
def multilabel_setup(tmp_path_factory, gpu_device):
    """the recipe of tests/test_multilabel_gpu.py: a multi-label checkpoint (three named classes, not permutation
    invariant) with a calibrated read-out, written in the reference's format, and its pipeline"""
    import yaml
    import pyannote_audio_amd as pa
    from conftest import PYANNET_HPARAMS
    from oracle.synthetic import calibrated_multilabel_pyannet
    from pyannote_audio_amd.model import Problem, PyanNet, Resolution, Specifications, save_checkpoint
    seg_o = calibrated_multilabel_pyannet(calib_seconds=40.0)
    root = tmp_path_factory.mktemp("multilabel_batch")
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


@pytest.fixture(scope="module")
def audio_files():
    from oracle.synthetic import synth_conversation
    return [{"waveform": synth_conversation(seconds, seed=40 + i)[0], "sample_rate": 16000, "uri": f"file{i}"}
            for i, seconds in enumerate(SECONDS)]


def _copies(files):
    return [dict(f) for f in files]


def _rows(annotation):
    return list(annotation.itertracks(yield_label=True))


def _assert_same_annotations(got, files, want):
    assert [f["uri"] for f, _ in got] == [f["uri"] for f in files]
    for (file, annotation), alone in zip(got, want):
        assert _rows(annotation) == _rows(alone), file["uri"]
        assert annotation.uri == alone.uri == file["uri"]


def test_forward_files_on_a_multilabel_checkpoint(multilabel_setup, gpu_device):
    _, pipeline, _ = multilabel_setup
    engine = pipeline._segmentation.model.engine
    assert engine.PACKS_FILES and not engine.pack.powerset
    g = torch.Generator().manual_seed(3)
    counts = [1, 3, 13]
    waves = [(0.1 * torch.randn(160000 + (c - 1) * 16000, generator=g)).to(gpu_device) for c in counts]
    scores, multilabel = engine.forward_files(waves, 16000, counts, 160000)
    assert multilabel is None and scores.shape[0] == sum(counts) and scores.shape[2] == len(CLASSES)
    at = 0
    for wave, count in zip(waves, counts):
        alone, none = engine.forward_strided(wave, 16000, count, 160000)
        assert none is None and torch.equal(scores[at:at + count], alone), count
        at += count


@pytest.fixture(scope="module")
def vad(pipeline_dir, gpu_device):
    import pyannote_audio_amd as pa
    return pa.VoiceActivityDetection(segmentation=os.path.join(pipeline_dir, "segmentation")).to(gpu_device)


@pytest.mark.parametrize("durations", [(0.0, 0.0), (0.2, 0.15)])
def test_voice_activity_detection_packed_is_apply_per_file(vad, audio_files, durations):
    vad.instantiate({"min_duration_on": durations[0], "min_duration_off": durations[1]})
    want = [vad(dict(f)) for f in audio_files]
    assert sum(len(_rows(a)) for a in want) >= 2 and all(a.labels() in ([], ["SPEECH"]) for a in want)
    got = list(vad(_copies(audio_files), pack=True))
    _assert_same_annotations(got, audio_files, want)
    assert vad.last_pack_groups == [[f["uri"] for f in audio_files]]
    # several groups, one of them a file larger than the budget (chunks per file: 1, 1, 2, 14, 19)
    got = list(vad(_copies(audio_files), pack=3))
    _assert_same_annotations(got, audio_files, want)
    assert vad.last_pack_groups == [["file0", "file1"], ["file2"], ["file3"], ["file4"]]


def test_pack_false_never_packs(vad, audio_files, monkeypatch):
    vad.instantiate({"min_duration_on": 0.0, "min_duration_off": 0.0})
    want = [vad(dict(f)) for f in audio_files[:3]]
    engine = vad._segmentation.model.engine

    def never(*args, **kwargs):
        raise AssertionError("forward_files was called")

    monkeypatch.setattr(engine, "forward_files", never)
    for kwargs in ({}, {"pack": False}):
        got = list(vad(_copies(audio_files[:3]), **kwargs))
        _assert_same_annotations(got, audio_files[:3], want)
        assert vad.last_pack_groups == []
    with pytest.raises(AssertionError, match="forward_files"):
        list(vad(_copies(audio_files[:3]), pack=True))


def test_multilabel_segmentation_packed_is_apply_per_file(multilabel_setup, audio_files):
    _, pipeline, thresholds = multilabel_setup
    assert any(t["offset"] > t["onset"] for t in thresholds.values())
    want = [pipeline(dict(f)) for f in audio_files]
    assert sum(len(_rows(a)) for a in want) >= 3 and len({l for a in want for l in a.labels()}) >= 2
    got = list(pipeline(_copies(audio_files), pack=True))
    _assert_same_annotations(got, audio_files, want)
    assert pipeline.last_pack_groups == [[f["uri"] for f in audio_files]]
    got = list(pipeline(_copies(audio_files), pack=3))
    _assert_same_annotations(got, audio_files, want)
    assert pipeline.last_pack_groups == [["file0", "file1"], ["file2"], ["file3"], ["file4"]]


def test_hook_and_training_take_the_per_file_loop(vad, multilabel_setup, audio_files, monkeypatch):
    vad.instantiate({"min_duration_on": 0.0, "min_duration_off": 0.0})
    _, multilabel, _ = multilabel_setup
    files = audio_files[1:4]
    for pipeline in (vad, multilabel):
        want = [pipeline(dict(f)) for f in files]
        engine = pipeline._segmentation.model.engine

        def never(*args, **kwargs):
            raise AssertionError("forward_files was called")

        monkeypatch.setattr(engine, "forward_files", never)
        seen = []
        hook = lambda name, artefact, file=None, **kw: seen.append((file["uri"], name)) if artefact is not None else None
        got = list(pipeline(_copies(files), pack=True, hook=hook))
        _assert_same_annotations(got, files, want)
        assert pipeline.last_pack_groups == [] and [u for u, _ in seen] == [f["uri"] for f in files]
        pipeline.training = True
        try:
            got = list(pipeline(_copies(files), pack=True))
            _assert_same_annotations(got, files, want)
            assert pipeline.last_pack_groups == []
            assert all(isinstance(f[pipeline.CACHED_SEGMENTATION].data, np.ndarray) for f, _ in got)
        finally:
            pipeline.training = False
