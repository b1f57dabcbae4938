"""GPU: `pa_annot_corpus_counts` (csrc/annot_metrics.hip) through `evaluation.Corpus`, and what is built on it.

The contract is bit equality with the per-file path: for every file,
`annotation_counts(reference, hypothesis.support(fill), uem, collar, skip_overlap, device=cuda)` (host `support`,
`pa_annot_counts`), compared value by value on the bytes.  On the dyadic grid of tests/annotation_metrics_truth.py the
results are also compared with the exact truth (`truth_counts` on the rows of tests/evaluation_truth.py's
`support_rows` in Fractions)."""
import ctypes
import os
import random
import warnings
from fractions import Fraction

import numpy as np
import pytest

import annotation_metrics_truth as truth
import evaluation_truth as et
from evaluation_truth import annotation, bare_annotation, corpus_files, indexed, timeline

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRID = truth.GRID


def bits(counts: dict) -> dict:
    return {k: v if k.endswith("labels") else np.asarray(v, dtype=np.float64).tobytes() for k, v in counts.items()}


def per_file(file, fill, collar, skip_overlap, device, key="speaker_diarization"):
    from pyannote_audio_amd.annotation_metrics import annotation_counts
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return annotation_counts(file["annotation"], file[key].support(fill), uem=file.get("annotated"),
                                 collar=collar, skip_overlap=skip_overlap, device=device)


def check(corpus, fill, collar=0.0, skip_overlap=False, exact=False):
    """every file of `corpus` against the per-file path (bits), the merged rows against the host `support`, and on
    request against the exact truth -> the corpus' results"""
    got = corpus.counts(fill, collar=collar, skip_overlap=skip_overlap)
    assert len(got) == len(corpus.files)
    for f, file in enumerate(corpus.files):
        want = per_file(file, fill, collar, skip_overlap, corpus.device)
        assert bits(got[f]) == bits(want), (f, fill, collar, skip_overlap)
        hyp = file["speaker_diarization"]
        assert corpus.merged_rows_[f] == len(list(hyp.support(fill).itertracks())), (f, fill)
        if exact:
            (Kr, ref), (Kh, rows) = indexed(rows_of(file["annotation"])), indexed(rows_of(hyp))
            names = sorted({l for _, _, l in rows_of(hyp)}, key=str)
            merged = [(float(a), float(b), names.index(l)) for a, b, l in
                      et.support_rows(rows_of(hyp), fill, num=Fraction)]
            uem = [(s.start, s.end) for s in file["annotated"]]
            t = truth.truth_counts(ref, merged, uem, Kr, Kh, collar=collar, skip_overlap=skip_overlap)
            flat = np.concatenate([got[f]["cooc"].ravel(), got[f]["ref_dur"], got[f]["hyp_dur"],
                                   [got[f][name] for name in truth.SCALARS]])
            assert [Fraction(v) for v in flat.tolist()] == truth.flat(t), (f, fill, collar, skip_overlap)
    return got


def rows_of(annotation_):
    return [(s.start, s.end, l) for s, _, l in annotation_.itertracks(yield_label=True)]


def make_file(uri, ref, hyp, uem=((0.0, 64.0),)):
    file = {"uri": uri, "annotation": annotation(ref, uri=uri), "speaker_diarization": annotation(hyp, uri=uri)}
    if uem is not None:
        file["annotated"] = timeline(uem)
    return file


def split_turns(n, labels, fill_gap=0.125, start=1.0):
    """n turns of 0.5 s, one every second, each split in two by a gap of `fill_gap`: 2 n rows, n turns once gaps of
    that length are filled; labels in turn"""
    rows = []
    for k in range(n):
        t = start + k * 1.0
        rows += [(t, t + 0.25, labels[k % len(labels)]), (t + 0.25 + fill_gap, t + 0.625, labels[k % len(labels)])]
    return rows


# --------------------------------------------------------------------------------------------------- cases
def test_one_file_equals_the_per_file_call(gpu_device):
    from pyannote_audio_amd.evaluation import Corpus
    rng = random.Random(5)
    file = make_file("one", et.random_rows(rng, 40, ["a", "b", "c"], 40.0, True),
                     et.random_rows(rng, 50, ["x", "y"], 40.0, True), uem=((0.5, 30.0), (32.0, 50.0)))
    corpus = Corpus([file], device=gpu_device)
    for fill, collar, skip_overlap in ((0.0, 0.0, False), (0.25, 0.0, False), (0.5, 0.5, True)):
        check(corpus, fill, collar, skip_overlap, exact=True)


def test_five_files_of_every_kind(gpu_device):
    """an empty hypothesis, an empty reference, a file whose uem has no rows, a file with 64 hypothesis labels, rows
    in `flat_rows` order with the labels interleaved; three of the files have 254, 256 and 258 cuts once the gaps are
    filled (the number of cuts is even: these are the counts around the workgroup size of 256, with 253, 255 and 257
    elementary intervals), so that the files' offsets are no multiples of the workgroup size"""
    from pyannote_audio_amd.evaluation import Corpus
    rng = random.Random(7)
    many = [f"s{j:02d}" for j in range(64)]
    files = [
        # 2 (126 + 0 + 1) = 254 cuts
        make_file("no hypothesis", split_turns(63, ["a", "b", "c"]), []),
        # 2 (0 + 127 + 1) = 256 cuts when the 0.125 s gaps are filled
        make_file("no reference", [], split_turns(127, ["x", "y"], start=0.5), uem=((0.0, 200.0),)),
        make_file("no uem rows", et.random_rows(rng, 30, ["a", "b"], 20.0, True),
                  et.random_rows(rng, 30, ["x"], 20.0, True), uem=()),
        # 2 (32 + 96 + 1) = 258 cuts when the gaps are filled: 64 labels, the first 32 have two turns
        make_file("64 labels", et.random_rows(rng, 32, ["a", "b", "c"], 90.0, True), split_turns(96, many),
                  uem=((0.0, 128.0),)),
        make_file("interleaved", et.random_rows(rng, 70, ["a", "b", "c", "d"], 30.0, True),
                  et.random_rows(rng, 90, ["x", "y", "z"], 30.0, True)),
    ]
    assert len(files[3]["speaker_diarization"].labels()) == 64
    labels = [l for _, _, _, l in files[4]["speaker_diarization"].flat_rows()]
    assert len({tuple(labels[i:i + 2]) for i in range(len(labels) - 1)}) > 3            # (interleaved indeed)
    corpus = Corpus(files, device=gpu_device)
    got = check(corpus, 0.25, exact=True)
    cuts = [2 * (len(list(f["annotation"].itertracks())) + m + len(f["annotated"]))
            for f, m in zip(files, corpus.merged_rows_)]
    assert cuts[0] == 254 and cuts[1] == 256 and cuts[3] == 258
    assert corpus.merged_rows_[:2] == [0, 127] and corpus.merged_rows_[3] == 96
    assert not got[2]["cooc"].any() and got[2]["total"] == 0.0
    assert got[0]["total"] > 0 and got[1]["false_alarm"] > 0 and got[3]["hyp_dur"].all()
    check(corpus, 0.0, exact=True)                          # (none of the 0.125 s gaps is filled)
    check(corpus, 0.25, collar=0.5, skip_overlap=True, exact=True)


def test_support_edges(gpu_device):
    """every edge of the support rule (tests/evaluation_truth.py), each as the hypothesis of a file of its own, at every
    fill its table lists; the short row inside a turn is off the grid and has no exact truth"""
    from pyannote_audio_amd.evaluation import Corpus
    ref = [(0.5, 3.0, "a"), (2.5, 12.0, "b")]
    edges = dict(et.SUPPORT_EDGES)
    files = [make_file(name, ref, [(a, b, "x") for a, b in pairs]) for name, (pairs, _) in edges.items()]
    corpus = Corpus(files, device=gpu_device)
    for fill in sorted({fill for _, expected in edges.values() for fill in expected}):
        check(corpus, fill, exact=True)
        for (name, (_, expected)), rows in zip(edges.items(), corpus.merged_rows_):
            if fill in expected:
                assert rows == expected[fill], (name, fill)
    check(corpus, et.FILL, collar=0.25, skip_overlap=True, exact=True)

    pairs, expected = et.SHORT_ROW_INSIDE
    file = make_file("short row", ref, [])
    file["speaker_diarization"] = bare_annotation([(a, b, "x") for a, b in pairs])
    short = Corpus([files[0], file], device=gpu_device)
    for fill, turns in expected.items():
        check(short, fill)
        assert short.merged_rows_[1] == turns


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_corpora_off_the_grid(gpu_device, seed):
    """boundaries that are no multiples of anything: the bits still equal the per-file path's"""
    from pyannote_audio_amd.evaluation import Corpus
    rng = random.Random(100 + seed)
    files = []
    for f in range(4):
        nr, nh = rng.randrange(1, 301), rng.randrange(1, 301)
        files.append(make_file(f"f{f}", et.random_rows(rng, nr, ["a", "b", "c", "d"][:1 + f], 200.0, False),
                               et.random_rows(rng, nh, ["x", "y", "z", "w", "v"][:2 + f], 200.0, False),
                               uem=((rng.uniform(0, 5), rng.uniform(90, 100)), (rng.uniform(101, 110), 250.0))))
    corpus = Corpus(files, device=gpu_device)
    for fill in (0.0, 0.1, 0.37):
        check(corpus, fill, collar=0.25)
        check(corpus, fill, skip_overlap=True)


def test_results_do_not_depend_on_earlier_calls(gpu_device):
    from pyannote_audio_amd.evaluation import Corpus
    files = corpus_files(et.split_gap_turns)
    corpus = Corpus(files, device=gpu_device)
    first, between, third = corpus.counts(0.5), corpus.counts(0.0), corpus.counts(0.5)
    fresh = Corpus(files, device=gpu_device).counts(0.5)
    for a, b, c, d in zip(first, between, third, fresh):
        assert bits(a) == bits(c) == bits(d) != bits(b)


def test_refusals(gpu_device):
    """refused on the Python side or by the entry point's checks, before any launch"""
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd.evaluation import Corpus
    files = corpus_files(et.split_gap_turns)
    corpus = Corpus(files, device=gpu_device)
    for bad in (-0.125, float("nan")):
        with pytest.raises(ValueError):
            corpus.counts(bad)
        with pytest.raises(ValueError):
            corpus.counts(0.25, collar=bad)
        with pytest.raises(ValueError):                      # (the entry point's own check)
            corpus.device_counts(bad)
    # 65 labels on a side: that file goes through the host, the others through the device
    wide = make_file("wide", [(1.0, 40.0, "a")], split_turns(65, [f"s{j:02d}" for j in range(65)]))
    mixed = Corpus([files[0], wide], device=gpu_device)
    assert mixed._device_files == [0]
    check(mixed, 0.25)
    # what the workspace query answers 0 for is refused by the call, from the host tables alone
    lib = ffi.load()

    def table(*values):
        return np.array(values, dtype=np.int32)

    def refused(hyp_rows, Kh, files=1):
        host = {"h_ref_off": table(*[0] * (files + 1)), "h_hyp_off": table(*[0] * files, hyp_rows),
                "h_uem_off": table(*[0] * (files + 1)), "h_Kr": table(*[0] * files), "h_Kh": table(*[0] * (files - 1), Kh)}
        struct = ffi.AnnotCorpus()
        struct.F, struct.R = files, Kh
        for name, array in host.items():
            setattr(struct, name, array.ctypes.data)
        assert lib.pa_annot_corpus_workspace_bytes(ctypes.byref(struct)) == 0
        with pytest.raises(ValueError):
            ffi.check(lib.pa_annot_corpus_counts(ctypes.byref(struct), 0.0, 0.0, 0, None, None, None, 0, None),
                      "pa_annot_corpus_counts")

    refused((1 << 21) + 1, 1)           # 2^22 + 2 cuts in one file
    refused(10, 65)                     # 65 labels
    refused(10, 1, files=65536)         # more files than a launch has rows


def test_optimizer_on_the_device_equals_its_host_path(gpu_device):
    from pyannote_audio_amd.annotation_metrics import DiarizationErrorRate, JaccardErrorRate
    from pyannote_audio_amd.evaluation import MinDurationOffOptimizer
    for cls in (DiarizationErrorRate, JaccardErrorRate):
        host_files, device_files = corpus_files(et.split_gap_turns), corpus_files(et.split_gap_turns)
        host, device = MinDurationOffOptimizer(), MinDurationOffOptimizer()
        want = host(host_files, cls())
        got = device(device_files, cls(device=gpu_device))
        assert got == want and got[0] > 0.25
        assert device._reports == host._reports
        for a, b in zip(host_files, device_files):
            assert a["best_speaker_diarization"] == b["best_speaker_diarization"]


def test_benchmark_end_to_end(pipeline_dir, gpu_device, tmp_path):
    """the seeded SpeakerDiarization pipeline on the reference's sample with its RTTM as the annotation,
    optimize=True.  The table's value is the pipeline's metric on the prediction, exactly; evaluated on the WRITTEN
    RTTM read back it can differ by the RTTM's resolution: a start is rounded to 1 ms (off by <= 0.5 ms) and an end
    is the sum of a rounded start and a rounded duration (off by <= 1 ms); moving one hypothesis boundary by d
    changes each of false alarm, missed detection, matched and correctly matched time by at most d and leaves the
    total alone, so the rate moves by at most 4 * 2 * rows * 1 ms / total (the mapping is the same unless two
    speakers tie within that)."""
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.core import load_rttm
    from pyannote_audio_amd.evaluation import benchmark
    sample = os.path.join(GOLDEN, "sample.wav")
    reference = load_rttm(os.path.join(GOLDEN, "sample.rttm"))["sample"]
    pipeline = pa.Pipeline.from_pretrained(pipeline_dir).to(gpu_device)
    files = [{"uri": "sample", "audio": sample, "annotation": reference}]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        result = benchmark(pipeline, files, tmp_path, metric=pipeline.get_metric(), optimize=True, name="sample")
    names = {p.name for p in result["files"]}
    assert names == set(os.listdir(tmp_path))
    speed = [n for n in names if n.endswith(".yml") and "Optimized" not in n]
    assert len(speed) == 1 and speed[0] != "sample.yml"                     # (named after the device)
    assert names - set(speed) == {"sample.rttm", "sample.json", "sample.csv", "sample.txt", "sample.SpeakerCount.csv",
                                  "sample.OptimizedMinDurationOff.csv", "sample.OptimizedMinDurationOff.txt",
                                  "sample.OptimizedMinDurationOff.yml", "sample.OptimizedMinDurationOff.rttm"}
    import yaml
    logged = yaml.safe_load((tmp_path / speed[0]).read_text())
    assert {"seconds_per_hour", "times_faster_than_realtime", "total_processing_time", "device"} == set(logged)
    assert logged["device"]["name"]
    prediction = files[0]["speaker_diarization"]
    assert (tmp_path / "sample.rttm").read_text() == prediction.to_rttm()
    lines = (tmp_path / "sample.csv").read_text().splitlines()
    value = float(lines[-1].split(",")[1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        assert value == result["value"] == pipeline.get_metric()(reference, prediction)
        written = load_rttm(tmp_path / "sample.rttm")["sample"]
        read_back = pipeline.get_metric()(reference, written, detailed=True)
    rows = len(prediction.flat_rows())
    assert abs(read_back["diarization error rate"] - value) <= 4 * 2 * rows * 1e-3 / read_back["total"]
    assert 0.0 <= result["min_duration_off"] <= 1.0
    optimised = (tmp_path / "sample.OptimizedMinDurationOff.csv").read_text().splitlines()
    assert float(optimised[-1].split(",")[1]) <= value
    assert (tmp_path / "sample.OptimizedMinDurationOff.rttm").read_text() == \
        prediction.support(result["min_duration_off"]).to_rttm()
