"""Host side of the detection pipelines on a list of files (no GPU):

* `frames.files_layout` against the shapes `Inference.slide` produces, with the engine replaced by a stub and the
  aggregation by the host chunk loop;
* the numpy model of the scan over the concatenation (tests/regions_files_model.py) against the per-file helper
  (tests/multilabel_oracle.py), bit for bit, on the cases the GPU test runs -- and those cases tell the model's
  deliberate errors from the right one, so they cannot pass vacuously;
* which calls of `apply_batch` form groups and which take the per-file loop, with the launches replaced by recorders."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import detection_batch_cases as cases  # noqa: E402
import multilabel_oracle as mo  # noqa: E402
import regions_files_model as model  # noqa: E402

from pyannote_audio_amd import frames as frame_ops  # noqa: E402
from pyannote_audio_amd.core import SlidingWindow, SlidingWindowFeature  # noqa: E402
from pyannote_audio_amd.detection_batch import PackedDetection  # noqa: E402
from pyannote_audio_amd.inference import Inference  # noqa: E402
from pyannote_audio_amd.model import Resolution  # noqa: E402
from pyannote_audio_amd.pipeline import Pipeline  # noqa: E402

SECONDS = [0.7, 10.0, 10.5, 23.0, 27.43]
NUM_FRAMES = 589                      # frames of a 10 s chunk of the PyanNet front end


class _Engine:
    PACKS_FILES = True
    max_chunks = 4096

    def __init__(self):
        self.counts = []

    def forward_strided(self, wav, stride, count, window, want_logp=True, want_multilabel=True):
        self.counts.append(count)
        return torch.full((count, NUM_FRAMES, 3), 0.25), None


class _Model:
    def __init__(self, engine):
        self.engine = engine
        self.specifications = SimpleNamespace(duration=10.0, warm_up=(0.0, 0.0), powerset=False,
                                              permutation_invariant=False, resolution=Resolution.FRAME)
        self.audio = SimpleNamespace(sample_rate=16000,
                                     get_num_samples=lambda duration, sample_rate=None: round(duration * 16000))
        self.device = torch.device("cpu")
        self.receptive_field = SlidingWindow(start=0.0, duration=0.0619375, step=0.016875)

    def eval(self):
        return self

    def to(self, device):
        return self


def _host_aggregate(scores, chunks, frames, device, **kw):
    return Inference.aggregate(SlidingWindowFeature(np.asarray(scores), chunks), frames, **kw)


# --------------------------------------------------------------------------------------------------- files_layout
def test_files_layout_gives_the_shapes_of_slide(monkeypatch):
    monkeypatch.setattr(frame_ops, "aggregate", _host_aggregate)
    engine = _Engine()
    inference = Inference(_Model(engine))
    samples = [int(s * 16000) for s in SECONDS]
    counts, chunk0, row0, T = frame_ops.files_layout(samples, inference)
    for n, count, kept in zip(samples, counts, T):
        out = inference.slide(torch.zeros(1, n), 16000)
        assert engine.counts[-1] == count, n
        assert out.data.shape == (kept, 3), (n, out.data.shape, kept)
    assert counts.tolist() == [1, 1, 2, 14, 19]
    assert chunk0.tolist() == [0, 1, 2, 4, 18, 37]
    # 0.7 s and 10.5 s end in a zero-padded chunk whose padding the loose crop cuts off; 10.0 s and 23.0 s do not
    whole = frame_ops.frame_geometry(SlidingWindow(start=0.0, duration=10.0, step=1.0), inference.model.receptive_field, 1)
    assert T[0] < T[1] == whole[1] < T[2] < T[3] < T[4]
    assert row0[0] == 0 and (row0 % 64 == 0).all() and (np.diff(row0) >= T).all() and (np.diff(row0) < T + 64).all()
    assert all(a.dtype == np.int32 for a in (counts, chunk0, row0, T))
    empty = frame_ops.files_layout([], inference)
    assert [len(a) for a in empty] == [0, 1, 1, 0]


def test_row_tables_are_checked_on_the_host():
    check = frame_ops._files_tables
    check([0, 64, 64, 192], [64, 0, 100], "t")
    for row0, T in (([0, 64, 32], [1, 1]), ([0, 60], [1]), ([0, 64], [65]), ([64, 128], [1]), ([0, 64], [1, 1]),
                    ([0, 64], [-1])):
        with pytest.raises(ValueError):
            check(row0, T, "t")
    with pytest.raises(ValueError, match="65535"):
        check(np.zeros(65537, dtype=np.int32), np.zeros(65536, dtype=np.int32), "t")


# ------------------------------------------------------------------------------------- the model of the one scan
@pytest.mark.parametrize("K", [1, 3, 16])
def test_scan_over_the_concatenation_is_the_rule_per_file(K):
    files = cases.region_files(K)
    T = [len(x) for x in files]
    row0 = model.layout(T)
    assert (row0 % 64 == 0).all()
    # the padding's contents do not matter, and neither does what it holds next to a file's last frame
    for fill in (np.nan, 0.95):
        scores = model.pack(files, row0, fill=fill)
        for name, *_ in cases.REGION_PARAMETERS:
            params = cases.region_parameters(name, K)
            want = cases.oracle_per_file(files, *params)
            got = model.regions_files(scores, row0, T, *cases.FRAMES, *params)
            pairs = [[rows for rows, _ in per_class] for per_class in got]
            positions = [[p for _, p in per_class] for per_class in got]
            cases.assert_same_lists((pairs, positions), want, (K, name, fill))


def test_the_cases_cannot_pass_vacuously():
    for K in (1, 3, 16):
        files = cases.region_files(K)
        T = [len(x) for x in files]
        row0 = model.layout(T)
        scores = model.pack(files, row0)
        plain = cases.oracle_per_file(files, *cases.region_parameters("offset_below_onset", K))
        # somewhere, every class has at least three regions; T < 2 gives none; the NaN column gives none
        assert all(max(len(per_class[k][0]) for per_class in plain) >= 3 for k in range(K))
        assert all(len(rows) == 0 for per_class in plain[:1] for rows, _ in per_class)
        assert plain[2][0] == ([], [])
        # file 3 ends active, file 4 starts active, file 6 is inactive between two active ones
        last, first = plain[3][0][0][-1], plain[4][0][0][0]
        assert last[1] == mo.frame_middle(63, *cases.FRAMES) and first[0] == mo.frame_middle(0, *cases.FRAMES)
        assert all(len(rows) == 0 for rows, _ in plain[6])
        assert plain[5][0][0][-1][1] == mo.frame_middle(1022, *cases.FRAMES) and plain[7][0][0][0][0] == first[0]
        # minimum durations: at least one region merged away and one dropped
        onset, offset, d_on, d_off = cases.region_parameters("offset_is_onset", K)
        raw = cases.oracle_per_file(files, onset, offset, 0.0, 0.0)
        merged = cases.oracle_per_file(files, onset, offset, 0.0, d_off)
        both = cases.oracle_per_file(files, onset, offset, d_on, d_off)
        count = lambda lists: sum(len(rows) for per_class in lists for rows, _ in per_class)
        assert count(raw) > count(merged) > count(both) > 0
        # every deliberate error of the model is told from the right one by some case
        for wrong in model.WRONG:
            told = False
            for name, *_ in cases.REGION_PARAMETERS:
                params = cases.region_parameters(name, K)
                got = model.regions_files(scores, row0, T, *cases.FRAMES, *params, wrong=wrong)
                want = cases.oracle_per_file(files, *params)
                told = told or any(list(map(tuple, g[0])) != list(map(tuple, w[0])) or list(g[1]) != list(w[1])
                                   for gf, wf in zip(got, want) for g, w in zip(gf, wf))
            assert told, (K, wrong)


# ------------------------------------------------------------------------------------ grouping and fallbacks
class _Detector(PackedDetection, Pipeline):
    """the mixin over a stub Inference: `apply` and `_detect_group` record what they were asked"""

    def __init__(self, **inference_kwargs):
        super().__init__()
        self._segmentation = Inference(_Model(_Engine()), **inference_kwargs)
        self.applied, self.groups, self.detector = [], [], {"any": True}

    def _packed_detector(self):
        return self.detector

    def apply(self, file, hook=None):
        self.applied.append((file["uri"], hook))
        return "apply:" + file["uri"]

    def _detect_group(self, files, waveforms, detector):
        assert detector is self.detector and [w.shape[0] for w in waveforms] == [1] * len(files)
        self.groups.append([f["uri"] for f in files])
        return ["packed:" + f["uri"] for f in files]


def _files():
    return [{"waveform": torch.zeros(1, int(s * 16000)), "sample_rate": 16000, "uri": f"f{i}"}
            for i, s in enumerate(SECONDS)]


def test_groups_follow_the_chunk_budget():
    p = _Detector()
    out = list(p(_files(), pack=True))
    assert [o for _, o in out] == [f"packed:f{i}" for i in range(5)] and [f["uri"] for f, _ in out] == p.groups[0]
    assert p.groups == [["f0", "f1", "f2", "f3", "f4"]] == p.last_pack_groups and p.applied == []
    # chunks per file: 1, 1, 2, 14, 19; a file larger than the budget is a group of its own
    p = _Detector()
    out = list(p(_files(), pack=3))
    assert p.last_pack_groups == [["f0", "f1"], ["f2"], ["f3"], ["f4"]] == p.groups
    assert [o for _, o in out] == [f"packed:f{i}" for i in range(5)]
    p = _Detector()
    list(p(_files(), pack=16))
    assert p.last_pack_groups == [["f0", "f1", "f2"], ["f3"], ["f4"]]
    for bad in (0, -2):
        with pytest.raises(ValueError, match="pack"):
            list(_Detector()(_files(), pack=bad))


def test_the_per_file_loop_is_the_default_and_the_fallback():
    def loop_taken(p, files=None, **kwargs):
        out = list(p(files or _files(), **kwargs))
        assert [o for _, o in out] == [f"apply:f{i}" for i in range(5)]
        assert p.groups == [] and p.last_pack_groups == [] and [u for u, _ in p.applied] == [f"f{i}" for i in range(5)]
        return p

    loop_taken(_Detector())
    loop_taken(_Detector(), pack=False)
    hook = lambda *a, **k: None
    assert all(h is hook for _, h in loop_taken(_Detector(), pack=True, hook=hook).applied)
    p = _Detector()
    p.training = True
    loop_taken(p, pack=True)
    p = _Detector()
    p._segmentation.model.engine.PACKS_FILES = False
    loop_taken(p, pack=True)
    with pytest.warns(UserWarning):
        whole = _Detector(window="whole")
    loop_taken(whole, pack=True)
    loop_taken(_Detector(skip_aggregation=True), pack=True)
    p = _Detector()
    p.detector = None                                     # the pipeline's own configuration asks for the loop
    loop_taken(p, pack=True)
    # a file's own pipeline_kwargs reach its `apply`, as in the loop of a pipeline without apply_batch
    files = _files()
    files[2]["pipeline_kwargs"] = {"hook": hook}
    p = loop_taken(_Detector(), files=files, pack=True)
    assert [h for _, h in p.applied] == [None, None, hook, None, None]


def test_what_the_pipelines_ask_of_the_packed_route():
    from pyannote_audio_amd.multilabel import MultiLabelSegmentation
    from pyannote_audio_amd.voice_activity_detection import VoiceActivityDetection, any_speaker

    def vad(onset, offset, powerset=True, hook=any_speaker, skip_conversion=False):
        inference = SimpleNamespace(pre_aggregation_hook=hook, skip_conversion=skip_conversion,
                                    model=SimpleNamespace(specifications=SimpleNamespace(powerset=powerset)))
        return VoiceActivityDetection._packed_detector(SimpleNamespace(
            _segmentation=inference, onset=onset, offset=offset, min_duration_on=0.2, min_duration_off=0.15))

    d = vad(0.5, 0.5)
    assert d == {"any": True, "hard": True, "onset": 0.5, "offset": 0.5, "min_duration_on": 0.2,
                 "min_duration_off": 0.15, "classes": ["SPEECH"]}
    assert vad(0.6, 0.4, powerset=False)["hard"] is False and vad(0.5, 0.5, skip_conversion=True)["hard"] is False
    assert vad(0.6, 0.0)["offset"] == 0.6                 # Binarize: `offset or onset`
    assert vad(0.4, 0.6, powerset=False) is None          # the host Binarize is another rule there
    assert vad(0.5, 0.5, hook=lambda x: x) is None

    pipeline = SimpleNamespace(_segmentation=SimpleNamespace(pre_aggregation_hook=None), _onset=[0.4], _offset=[0.6],
                               _min_duration_on=[0.0], _min_duration_off=[0.1], _classes=["speech"])
    d = MultiLabelSegmentation._packed_detector(pipeline)
    assert d["any"] is False and d["hard"] is False and d["offset"] == [0.6] and d["classes"] == ["speech"]
    pipeline._segmentation.pre_aggregation_hook = lambda x: x
    assert MultiLabelSegmentation._packed_detector(pipeline) is None
