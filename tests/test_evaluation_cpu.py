"""CPU: `annotation_metrics.JaccardErrorRate`, the support rule the corpus kernel is held to, `evaluation`'s
`Corpus` / `MinDurationOffOptimizer` / `benchmark` on the host path, and the RTTM / UEM readers.

Boundaries are on the dyadic grid of tests/annotation_metrics_truth.py (every sum is exact), so comparisons with the
exact truths of tests/evaluation_truth.py use `==`."""
import os
import warnings
from fractions import Fraction

import numpy as np
import pytest
import yaml

import annotation_metrics_truth as truth
import evaluation_truth as et
from evaluation_truth import annotation, bare_annotation, corpus_files, indexed, timeline

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRID = truth.GRID


# ------------------------------------------------------------------------------------------------- jaccard
def _jer_case(ref, hyp, uem, collar=0.0, skip_overlap=False):
    from pyannote_audio_amd.annotation_metrics import JaccardErrorRate
    metric = JaccardErrorRate(collar=collar, skip_overlap=skip_overlap)
    got = metric(annotation(ref), annotation(hyp), uem=timeline(uem), detailed=True)
    (Kr, r), (Kh, h) = indexed(ref), indexed(hyp)
    count, errors = et.jaccard_truth(r, h, uem, Kr, Kh, collar=collar, skip_overlap=skip_overlap)
    assert got["speaker count"] == count
    assert got["speaker error"] == et.float_sum(errors)
    assert got["jaccard error rate"] == (et.float_sum(errors) / count if count else 0.0)
    return got, errors


REF = [(1.0, 5.0, "a"), (6.0, 9.0, "b"), (8.5, 12.0, "a"), (13.0, 14.0, "c")]
HYP = [(1.25, 5.0, "x"), (6.0, 8.0, "y"), (8.75, 12.5, "x"), (13.0, 13.5, "z")]
UEM = [(0.0, 16.0)]


def test_jaccard_matched_pair_is_zero():
    got, errors = _jer_case([(1.0, 3.0, "a"), (4.0, 6.0, "b")], [(1.0, 3.0, "x"), (4.0, 6.0, "y")], UEM)
    assert errors == [0, 0] and got["jaccard error rate"] == 0.0 and got["speaker count"] == 2


def test_jaccard_against_exact_truth():
    got, errors = _jer_case(REF, HYP, UEM)
    assert got["speaker count"] == 3 and all(0 < e < 1 for e in errors)


def test_jaccard_unmapped_reference_adds_one():
    base, _ = _jer_case(REF, HYP, UEM)
    more, errors = _jer_case(REF + [(14.5, 15.5, "d")], HYP, UEM)          # nobody speaks where "d" does
    assert errors[-1] == 1
    assert more["speaker count"] == base["speaker count"] + 1
    assert more["speaker error"] == base["speaker error"] + 1.0


def test_jaccard_extra_hypothesis_label_changes_nothing_unless_mapped():
    base, _ = _jer_case(REF, HYP, UEM)
    # a fourth hypothesis speaker that overlaps "b" less than "y" does: it stays unmapped
    same, _ = _jer_case(REF, HYP + [(8.0, 8.25, "w")], UEM)
    assert same == base
    # the same speaker once it overlaps "c" more than "z" does: it is mapped, and the error of "c" changes
    other, _ = _jer_case(REF, HYP + [(13.0, 13.75, "w")], UEM)
    assert other["speaker count"] == base["speaker count"] and other["speaker error"] != base["speaker error"]


def test_jaccard_reference_label_outside_uem_is_not_counted():
    inside, _ = _jer_case(REF, HYP, [(0.0, 12.5)])                           # "c" speaks after the uem ends
    assert inside["speaker count"] == 2
    everything, _ = _jer_case(REF, HYP, UEM)
    assert everything["speaker count"] == 3


@pytest.mark.parametrize("collar,skip_overlap", [(0.5, False), (0.0, True), (0.25, True)])
def test_jaccard_collar_and_skip_overlap(collar, skip_overlap):
    _jer_case(REF, HYP, UEM, collar=collar, skip_overlap=skip_overlap)


def test_jaccard_accumulates_components():
    from pyannote_audio_amd.annotation_metrics import JaccardErrorRate
    metric = JaccardErrorRate()
    cases = [(REF, HYP), (REF + [(14.5, 15.5, "d")], HYP), ([(1.0, 3.0, "a")], [(1.0, 3.0, "x")])]
    count, error = 0, 0.0
    for k, (ref, hyp) in enumerate(cases):
        file = metric(annotation(ref, uri=f"f{k}"), annotation(hyp), uem=timeline(UEM), detailed=True)
        count += file["speaker count"]
        error += file["speaker error"]
    assert metric["speaker count"] == count == 8 and metric["speaker error"] == error
    assert abs(metric) == error / count
    report = metric.report()
    assert list(report) == ["f0", "f1", "f2", "TOTAL"] and report["TOTAL"]["jaccard error rate"] == error / count
    assert JaccardErrorRate()(annotation([]), annotation(HYP), uem=timeline(UEM)) == 0.0     # no speaker: 0


def test_components_from_counts_is_compute_components():
    """the split every class got: counts, then components from the counts"""
    from pyannote_audio_amd import annotation_metrics as am
    ref, hyp, uem = annotation(REF), annotation(HYP), timeline(UEM)
    for cls in (am.DiarizationErrorRate, am.GreedyDiarizationErrorRate, am.IdentificationErrorRate,
                am.DetectionErrorRate, am.DetectionPrecisionRecallFMeasure, am.JaccardErrorRate):
        metric = cls(collar=0.25)
        counts = am.annotation_counts(ref, hyp, uem=uem, collar=0.25)
        assert metric.components_from_counts(counts) == metric.compute_components(ref, hyp, uem=uem)
        assert metric.add_counts(counts, uri="x") == cls(collar=0.25)(ref, hyp, uem=uem)


# ------------------------------------------------------------------------------------------------- support
def _support_of(rows, fill):
    return sorted((s.start, s.end, l) for s, _, l in bare_annotation(rows).support(fill).itertracks(yield_label=True))


@pytest.mark.parametrize("name", list(et.SUPPORT_EDGES))
def test_support_rule_edges(name):
    pairs, expected = et.SUPPORT_EDGES[name]
    rows = [(a, b, "x") for a, b in pairs] + [(1.5, 2.5, "y")]          # (another label never interferes)
    for fill, turns in expected.items():
        want = et.support_rows(rows, fill, num=Fraction)
        assert len(want) == turns + 1, (name, fill)
        assert sorted(et.support_rows(rows, fill, num=float)) == sorted(want) == _support_of(rows, fill)


def test_support_rule_short_row_inside_a_turn():
    pairs, expected = et.SHORT_ROW_INSIDE
    rows = [(a, b, "x") for a, b in pairs]
    for fill, turns in expected.items():
        want = et.support_rows(rows, fill, num=float)
        assert len(want) == turns and sorted(want) == _support_of(rows, fill)
    assert sorted(et.support_rows(rows, 0.0)) == [(1.0, 5.0, "x"), (3.0, 6.0, "x")]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("fill", [0.0, 0.125, 0.5])
def test_support_rule_random(seed, fill):
    import random
    rows = et.random_rows(random.Random(seed), 120, ["x", "y", "z"], 40.0, dyadic=True)
    want = et.support_rows(rows, fill, num=Fraction)
    assert sorted(want) == sorted(et.support_rows(rows, fill)) == _support_of(rows, fill)


# ---------------------------------------------------------------------------------- corpus and optimizer
def reference_loop(files, metric, bounds=(0.0, 1.0)):
    """the reference's MinDurationOffOptimizer, transcribed: `support` per file, the metric per file,
    scipy's bounded scalar minimisation, 0.0 when nothing beats it"""
    from scipy.optimize import minimize_scalar
    state = {"best": float("inf"), "reports": {}}

    def objective(collar):
        metric.reset()
        for file in files:
            file["temporary"] = file["speaker_diarization"].support(collar)
            metric(file["annotation"], file["temporary"], uem=file["annotated"])
        state["reports"][collar] = {uri: dict(c) for uri, c in metric.results_}
        state["reports"][collar]["TOTAL"] = {**metric[:], metric.metric_name_: abs(metric)}
        value = abs(metric)
        if value < state["best"]:
            state["best"] = value
            for file in files:
                file["expected_best"] = file.pop("temporary")
        return value

    without = objective(0.0)
    found = minimize_scalar(objective, bounds=bounds, method="Bounded")
    best = 0.0 if without == state["best"] else float(found.x)
    return best, state["reports"][best]


@pytest.mark.parametrize("maker,zero_wins", [(et.split_gap_turns, False), (et.zero_wins_turns, True)])
def test_optimizer_host_path_equals_the_reference_loop(maker, zero_wins):
    from pyannote_audio_amd.annotation_metrics import DiarizationErrorRate
    from pyannote_audio_amd.evaluation import MinDurationOffOptimizer
    files = corpus_files(maker)
    want_best, want_report = reference_loop(files, DiarizationErrorRate())
    optimizer = MinDurationOffOptimizer()
    best, report = optimizer(files, DiarizationErrorRate())
    assert best == want_best and report == want_report
    assert (best == 0.0) == zero_wins and (zero_wins or best > 0.25)
    assert set(optimizer._reports) >= {0.0, best} and len(optimizer._reports) > 2       # one report per candidate
    for file in files:
        assert file["best_speaker_diarization"] == file["expected_best"]
        assert file["best_speaker_diarization"] == file["speaker_diarization"].support(best)
    if not zero_wins:
        assert report["TOTAL"]["missed detection"] == 0.0 < optimizer._reports[0.0]["TOTAL"]["missed detection"]


def test_optimizer_takes_the_literal_loop_for_other_metrics():
    """a metric object that is not one of the count-based classes is called file by file"""
    from pyannote_audio_amd.annotation_metrics import DiarizationErrorRate
    from pyannote_audio_amd.evaluation import MinDurationOffOptimizer

    class Wrapped:
        def __init__(self):
            self.inner, self.calls = DiarizationErrorRate(), 0

        def reset(self):
            self.inner.reset()

        def __call__(self, reference, hypothesis, uem=None):
            self.calls += 1
            return self.inner(reference, hypothesis, uem=uem)

        def __abs__(self):
            return abs(self.inner)

        def report(self):
            return self.inner.report()

    files = corpus_files(et.split_gap_turns)
    metric = Wrapped()
    best, report = MinDurationOffOptimizer()(files, metric)
    assert metric.calls > 0 and metric.calls % len(files) == 0
    assert (best, report) == MinDurationOffOptimizer()(corpus_files(et.split_gap_turns), DiarizationErrorRate())


def test_corpus_counts_on_the_host():
    """the per-file dicts of `annotation_counts` on the supported hypothesis; the extent rule with one warning;
    no dependence on earlier calls; refusals"""
    from pyannote_audio_amd.annotation_metrics import annotation_counts
    from pyannote_audio_amd.evaluation import Corpus
    files = corpus_files(et.split_gap_turns, uem=False)
    with pytest.warns(UserWarning) as caught:
        corpus = Corpus(files)
    assert len(caught) == 1

    def same(a, b):
        return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)

    first = corpus.counts(0.5, collar=0.25)
    zero = corpus.counts(0.0, collar=0.25)
    again = corpus.counts(0.5, collar=0.25)
    for f, file in enumerate(files):
        for fill, got in ((0.5, first[f]), (0.0, zero[f]), (0.5, again[f])):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = annotation_counts(file["annotation"], file["speaker_diarization"].support(fill), collar=0.25)
            assert same(got, want)
    assert corpus.merged_rows_ == [len(file["speaker_diarization"].support(0.5)) for file in files]
    for bad in (-0.125, float("nan")):
        with pytest.raises(ValueError):
            corpus.counts(bad)
        with pytest.raises(ValueError):
            corpus.counts(0.0, collar=bad)


@pytest.mark.parametrize("files", [
    [],                                                          # F = 0: the alignment slack alone
    [(0, 0, 0, 0, 0)],                                           # an empty file
    [(5, 7, 1, 2, 3), (0, 0, 0, 0, 0), (12, 1, 2, 4, 1)],
    [(3, 0, 1, 2, 0), (0, 9, 1, 0, 64), (1000, 2000, 3, 64, 64), (1, 1, 1, 1, 1)],
], ids=["no-file", "empty-file", "three-files", "four-files"])
def test_workspace_formula_is_the_library_s(files):
    """`evaluation.corpus_workspace_bytes` (callers size their chunks with it before any table exists) against
    `pa_annot_corpus_workspace_bytes`, which reads F, R and the five host tables only.  Per file: reference,
    hypothesis, uem rows, reference and hypothesis labels."""
    import ctypes
    from pyannote_audio_amd import ffi
    from pyannote_audio_amd.evaluation import corpus_workspace_bytes, cut_slots
    struct = ffi.AnnotCorpus()
    struct.F, struct.R = len(files), sum(f[4] for f in files)
    columns = np.array(files, dtype=np.int64).reshape(len(files), 5).T
    tables = [np.concatenate([[0], np.cumsum(column)]).astype(np.int32) for column in columns[:3]] + \
             [np.ascontiguousarray(column, dtype=np.int32) for column in columns[3:]]
    for name, table in zip(("ref_off", "hyp_off", "uem_off", "Kr", "Kh"), tables):
        setattr(struct, "h_" + name, table.ctypes.data)
    want = int(ffi.load().pa_annot_corpus_workspace_bytes(ctypes.byref(struct)))
    assert want > 0
    assert corpus_workspace_bytes(sum(f[1] for f in files), sum(cut_slots(f[0], f[1], f[2]) for f in files)) == want


# ----------------------------------------------------------------------------------------------- benchmark
class StubOutput:
    def __init__(self, speaker_diarization):
        self.speaker_diarization = speaker_diarization

    def serialize(self):
        return {"diarization": [[a, b, l] for a, b, _, l in self.speaker_diarization.flat_rows()]}


class StubPipeline:
    """yields fixed annotations; `serialize` only when asked for"""

    def __init__(self, predictions, serialize=False):
        self.predictions, self.serialize = predictions, serialize

    def __call__(self, files):
        for file in files:
            prediction = self.predictions[file["uri"]]
            yield file, (StubOutput(prediction) if self.serialize else prediction)


def two_files():
    ref0, hyp0 = et.split_gap_turns(0)                                     # 2 speakers, 2 predicted
    ref1, hyp1 = et.split_gap_turns(1, speakers=3)                         # 3 speakers ...
    hyp1 = [(a, b, "h0" if l == "h2" else l) for a, b, l in hyp1]          # ... 2 predicted
    files, predictions = [], {}
    for uri, ref, hyp in (("one", ref0, hyp0), ("two", ref1, hyp1)):
        files.append({"uri": uri, "annotation": annotation(ref, uri=uri), "annotated": timeline([(0.0, 120.0)]),
                      "duration": 120.0})
        predictions[uri] = annotation(hyp, uri=uri)
    return files, predictions


def test_benchmark_artefacts(tmp_path):
    from pyannote_audio_amd.annotation_metrics import DiarizationErrorRate
    from pyannote_audio_amd.core import load_rttm
    from pyannote_audio_amd.evaluation import benchmark
    files, predictions = two_files()
    result = benchmark(StubPipeline(predictions, serialize=True), files, tmp_path, optimize=True, name="stub")
    names = ["stub.rttm", "stub.json", "stub.yml", "stub.csv", "stub.txt", "stub.SpeakerCount.csv",
             "stub.OptimizedMinDurationOff.csv", "stub.OptimizedMinDurationOff.txt",
             "stub.OptimizedMinDurationOff.yml", "stub.OptimizedMinDurationOff.rttm"]
    assert sorted(p.name for p in result["files"]) == sorted(names) == sorted(os.listdir(tmp_path))
    assert (tmp_path / "stub.rttm").read_text() == predictions["one"].to_rttm() + predictions["two"].to_rttm()
    speed = yaml.safe_load((tmp_path / "stub.yml").read_text())
    assert set(speed) == {"seconds_per_hour", "times_faster_than_realtime", "total_processing_time"}
    assert speed["times_faster_than_realtime"] == pytest.approx(240.0 / speed["total_processing_time"])
    # the metric's table: one line per file and the total, in full precision
    metric = DiarizationErrorRate()
    for file in files:
        metric(file["annotation"], predictions[file["uri"]], uem=file["annotated"])
    lines = (tmp_path / "stub.csv").read_text().splitlines()
    assert lines[0] == "item,diarization error rate,total,correct,false alarm,missed detection,confusion"
    assert [line.split(",")[0] for line in lines[1:]] == ["one", "two", "TOTAL"]
    assert float(lines[-1].split(",")[1]) == abs(metric) == result["value"]
    assert "TOTAL" in (tmp_path / "stub.txt").read_text()
    # 2 reference speakers -> 2 predicted, 3 -> 2
    count = (tmp_path / "stub.SpeakerCount.csv").read_text().splitlines()
    assert [[int(v) for v in line.split(",")] for line in count[:-1]] == [[0, 0, 0], [0, 0, 0], [0, 0, 1], [0, 0, 1]]
    assert count[-1] == "# Accuracy = 50.0% / Average error = 0.50 speakers off"
    # the optimised half
    best = yaml.safe_load((tmp_path / "stub.OptimizedMinDurationOff.yml").read_text())["min_duration_off"]
    assert best == result["min_duration_off"] > 0.25
    filled = load_rttm(tmp_path / "stub.OptimizedMinDurationOff.rttm")
    assert {uri: len(a) for uri, a in filled.items()} == {"one": 12, "two": 12}
    assert (tmp_path / "stub.OptimizedMinDurationOff.rttm").read_text() == \
        "".join(file["best_speaker_diarization"].to_rttm() for file in files)
    optimised = (tmp_path / "stub.OptimizedMinDurationOff.csv").read_text().splitlines()
    assert float(optimised[-1].split(",")[1]) == result["optimized_report"]["TOTAL"]["diarization error rate"] \
        < result["value"]
    # existing output is not overwritten
    with pytest.raises(FileExistsError):
        benchmark(StubPipeline(predictions), files, tmp_path, name="stub")


def test_benchmark_per_file_oracle_and_missing_annotation(tmp_path):
    from pyannote_audio_amd.evaluation import benchmark
    files, predictions = two_files()
    result = benchmark(StubPipeline(predictions, serialize=True), files, tmp_path, per_file=True, optimize=True,
                       num_speakers="oracle", name="stub")
    assert [file["pipeline_kwargs"] for file in files] == [{"num_speakers": 2}, {"num_speakers": 3}]
    root = tmp_path / "stub.OracleNumSpeakers"
    assert sorted(os.listdir(root / "rttm")) == ["one.OptimizedMinDurationOff.rttm", "one.rttm",
                                                 "two.OptimizedMinDurationOff.rttm", "two.rttm"]
    assert sorted(os.listdir(root / "json")) == ["one.json", "two.json"]
    assert (root / "rttm" / "two.rttm").read_text() == predictions["two"].to_rttm()
    assert (tmp_path / "stub.OracleNumSpeakers.csv").exists() and all(p.exists() for p in result["files"])
    with pytest.raises(FileExistsError):
        benchmark(StubPipeline(predictions), files, tmp_path, per_file=True, num_speakers="oracle", name="stub")
    # a file without annotation: predictions and speed only
    files, predictions = two_files()
    del files[1]["annotation"]
    result = benchmark(StubPipeline(predictions), files, tmp_path, optimize=True, name="bare")
    assert sorted(p.name for p in result["files"]) == ["bare.rttm", "bare.yml"]
    assert sorted(n for n in os.listdir(tmp_path) if n.startswith("bare")) == ["bare.rttm", "bare.yml"]
    assert "value" not in result


# ------------------------------------------------------------------------------------------------- readers
def test_load_rttm_round_trip():
    from pyannote_audio_amd.core import load_rttm
    path = os.path.join(GOLDEN, "sample.rttm")
    loaded = load_rttm(path)
    assert list(loaded) == ["sample"] and loaded["sample"].uri == "sample"
    with open(path) as fp:
        text = fp.read()
    assert loaded["sample"].to_rttm() == text
    assert len(loaded["sample"]) == len(text.splitlines()) and loaded["sample"].labels() == ["speaker90", "speaker91"]


def test_load_rttm_and_uem_several_uris_and_malformed(tmp_path):
    from pyannote_audio_amd.core import Segment, load_rttm, load_uem
    rttm = tmp_path / "two.rttm"
    rttm.write_text("SPEAKER a 1 0.500 1.250 <NA> <NA> x <NA> <NA>\n"
                    "SPEAKER b 1 2.000 1.000 <NA> <NA> y <NA> <NA>\n"
                    "\n"
                    "SPEAKER a 1 0.500 1.250 <NA> <NA> y <NA> <NA>\n")
    loaded = load_rttm(rttm)
    assert sorted(loaded) == ["a", "b"]
    assert [(s.start, s.end, l) for s, _, l in loaded["a"].itertracks(yield_label=True)] == \
        [(0.5, 1.75, "x"), (0.5, 1.75, "y")]
    assert [(s.start, s.end, l) for s, _, l in loaded["b"].itertracks(yield_label=True)] == [(2.0, 3.0, "y")]
    uem = tmp_path / "two.uem"
    uem.write_text("a 1 0.000 10.000\nb 1 0.000 4.000\na 1 12.000 20.000\n")
    regions = load_uem(uem)
    assert list(regions["a"]) == [Segment(0.0, 10.0), Segment(12.0, 20.0)] and list(regions["b"]) == [Segment(0.0, 4.0)]
    for bad in ("SPEAKER a 1 0.500 <NA> <NA> x\n", "SPEAKER a 1 zero 1.0 <NA> <NA> x <NA> <NA>\n",
                "LEXEME a 1 0.5 1.0 <NA> <NA> x <NA> <NA>\n", "SPEAKER a 1 0.5 -1.0 <NA> <NA> x <NA> <NA>\n"):
        rttm.write_text(bad)
        with pytest.raises(ValueError):
            load_rttm(rttm)
    for bad in ("a 1 0.0\n", "a 1 zero 1.0\n", "a 1 2.0 1.0\n"):
        uem.write_text(bad)
        with pytest.raises(ValueError):
            load_uem(uem)
