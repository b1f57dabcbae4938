"""The training cache of `SpeakerDiarization` and `pyannote_audio_amd.tuning.ClusteringTuner` on the GPU: a cached
front end launches neither network and changes no output, and a sweep over `clustering.threshold` x
`min_cluster_size` gives, candidate by candidate, the loss and the annotations of the literal loop --
`pipeline.instantiate(params)`, `pipeline(file)` for every file, a fresh metric -- on tests/golden/sample.wav and two
crops of it."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CROPS = ((0.0, 30.0), (0.0, 18.0), (9.0, 30.0))


@pytest.fixture(scope="module")
def pipeline(pipeline_dir, gpu_device):
    import pyannote_audio_amd as pa
    return pa.Pipeline.from_pretrained(pipeline_dir).to(gpu_device)


def corpus():
    """fresh file dicts: sample.wav and two crops of it, each with its part of sample.rttm"""
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.audio import Audio
    from pyannote_audio_amd.core import Segment, load_rttm
    waveform, rate = Audio(16000, mono="downmix")(os.path.join(GOLDEN, "sample.wav"))
    reference = load_rttm(os.path.join(GOLDEN, "sample.rttm"))["sample"]
    files = []
    for start, end in CROPS:
        uri = f"sample_{int(start)}_{int(end)}"
        part = pa.Annotation(uri=uri)
        for segment, track, label in reference.itertracks(yield_label=True):
            a, b = max(segment.start, start), min(segment.end, end)
            if b > a:
                part[Segment(a - start, b - start), track] = label
        files.append({"waveform": waveform[:, int(start * rate):int(end * rate)].clone(), "sample_rate": rate,
                      "uri": uri, "annotation": part, "annotated": [Segment(0.0, end - start)]})
    return files


def literal_loop(pipeline, files, candidates):
    """what the parent commit can do: every candidate through the whole pipeline, file by file"""
    assert pipeline.training is False
    losses, outputs = [], []
    for params in candidates:
        pipeline.instantiate(params)
        metric = pipeline.get_metric()
        outputs.append([])
        for file in files:
            diarization = pipeline(file).speaker_diarization
            metric(file["annotation"], diarization, uem=file.get("annotated"))
            outputs[-1].append(diarization)
        losses.append(abs(metric))
    return losses, outputs


def count_networks(pipeline, monkeypatch):
    calls = {"segmentation": 0, "embedding": 0}
    segmentation, engine = pipeline._segmentation, pipeline._embedding.model_.engine
    seg_forward, emb_forward = segmentation._forward, engine.forward_strided

    def counted_segmentation(*args, **kwargs):
        calls["segmentation"] += 1
        return seg_forward(*args, **kwargs)

    def counted_embedding(*args, **kwargs):
        calls["embedding"] += 1
        return emb_forward(*args, **kwargs)

    monkeypatch.setattr(segmentation, "_forward", counted_segmentation)
    monkeypatch.setattr(engine, "forward_strided", counted_embedding)
    return calls


def same_output(a, b) -> bool:
    return (a.speaker_diarization == b.speaker_diarization
            and a.exclusive_speaker_diarization == b.exclusive_speaker_diarization
            and np.array_equal(a.speaker_embeddings, b.speaker_embeddings))


def test_training_cache(pipeline, monkeypatch):
    pipeline.instantiate(pipeline.default_parameters())
    calls = count_networks(pipeline, monkeypatch)
    file = corpus()[0]
    keys = set(file)
    assert pipeline.training is False
    before = pipeline(file)
    assert set(file) == keys and calls == {"segmentation": 1, "embedding": 1}
    assert len(before.speaker_diarization.labels()) >= 1
    pipeline.training = True
    try:
        first = pipeline(file)
        assert calls == {"segmentation": 2, "embedding": 2}
        assert set(file) - keys == {"training_cache/segmentation", "training_cache/embeddings",
                                    "training_cache/front_end"}
        assert file["training_cache/segmentation"].data.shape[2] == 3
        assert set(file["training_cache/embeddings"]) == {"embeddings"}           # a powerset model: no threshold
        assert file["training_cache/embeddings"]["embeddings"].shape[:2] == file["training_cache/segmentation"].data.shape[::2]
        front = file["training_cache/front_end"]
        assert front.dev_seg.is_cuda and front.dev_emb.is_cuda and front.count is not None
        assert front.active.shape == front.clean.shape == tuple(front.dev_emb.shape[:2])
        enqueued = pipeline._segmentation.last_enqueued
        second = pipeline(file)
        assert calls == {"segmentation": 2, "embedding": 2}                        # neither network was launched
        assert pipeline._segmentation.last_enqueued == enqueued
        assert same_output(first, second) and same_output(before, first)
        # another candidate on the cached front end = the same candidate on a fresh one
        params = pipeline.parameters(instantiated=True)
        params["clustering"].update(threshold=0.3, min_cluster_size=1)
        pipeline.instantiate(params)
        cached = pipeline(file)
        assert calls == {"segmentation": 2, "embedding": 2}
    finally:
        pipeline.training = False
    fresh_file = corpus()[0]
    fresh = pipeline(fresh_file)
    assert same_output(cached, fresh) and set(fresh_file) == keys
    # a file that carries a cache is not served from it once `training` is off, and is left as it is
    cached_keys = set(file)
    again = pipeline(file)
    assert calls == {"segmentation": 4, "embedding": 4} and same_output(again, fresh) and set(file) == cached_keys


def quantile_thresholds(tuner, levels) -> list:
    """thresholds from the merge heights of the files' own dendrograms, so that the cuts differ by construction"""
    heights = np.concatenate([tuner._tree(item).tree.Z[:, 2] for item in tuner.prepared])
    return [float(t) for t in np.quantile(heights, levels)]


@pytest.mark.parametrize("forced", [False, True])
def test_sweep_equals_the_literal_loop(pipeline, monkeypatch, forced):
    from pyannote_audio_amd.tuning import ClusteringTuner, best_entry
    pipeline.instantiate(pipeline.default_parameters())
    files = corpus()
    if forced:      # the forced-count walk on cut labels
        files[1]["pipeline_kwargs"] = {"num_speakers": 2}
    calls = count_networks(pipeline, monkeypatch)
    tuner = ClusteringTuner(pipeline).prepare(files)
    assert pipeline.training is False and calls == {"segmentation": 3, "embedding": 3}
    assert all("training_cache/front_end" in file for file in files)
    sizes_of_training_sets = [tuner._tree(item).train.shape[0] for item in tuner.prepared]
    print("training embeddings per file:", sizes_of_training_sets)
    assert min(sizes_of_training_sets) >= 8
    levels = np.linspace(0.15, 0.97, 4 if forced else 9)
    thresholds = quantile_thresholds(tuner, levels)
    result = tuner.sweep(thresholds, [1, 12])
    assert calls == {"segmentation": 3, "embedding": 3}                 # the sweep itself runs no network
    entries = result["entries"]
    assert len(entries) == 2 * len(thresholds) and result["evaluations"] == 3 * len(entries)
    assert [(e["params"]["clustering"]["threshold"], e["params"]["clustering"]["min_cluster_size"])
            for e in entries] == [(t, m) for t in thresholds for m in (1, 12)]
    counts = {row[0] for row, e in zip(tuner.train_clusters, entries)
              if e["params"]["clustering"]["min_cluster_size"] == 1}
    print("clusters of file 0 over the thresholds:", sorted(counts), "shared:", result["shared_evaluations"])
    assert len(counts) >= 3

    hypotheses = [list(row) for row in tuner.hypotheses]
    losses, outputs = literal_loop(pipeline, corpus_like(files), [e["params"] for e in entries])
    for c, entry in enumerate(entries):
        print(c, entry["params"]["clustering"], entry["loss"], losses[c])
        assert entry["loss"] == losses[c], c
        for f in range(len(files)):
            assert hypotheses[c][f] == outputs[c][f], (c, f)
    assert result["best"] is best_entry(entries) and result["best"] is entries[int(np.argmin(losses))]
    if forced:
        assert all(len(row[1].labels()) <= 2 for row in hypotheses)


def corpus_like(files) -> list:
    """the same files without their caches (and as the dicts a user would pass)"""
    return [{key: value for key, value in file.items() if not key.startswith("training_cache/")} for file in files]


def test_thresholds_between_the_same_heights_share_their_evaluation(pipeline):
    from pyannote_audio_amd.tuning import ClusteringTuner
    pipeline.instantiate(pipeline.default_parameters())
    files = corpus()
    tuner = ClusteringTuner(pipeline).prepare(files)
    heights = np.unique(np.concatenate([tuner._tree(item).tree.Z[:, 2] for item in tuner.prepared]))
    i = int(np.argmax(np.diff(heights[:-1])))            # the widest gap between two adjacent heights of any file
    low, high = heights[i], heights[i + 1]
    inside = [float(low + (high - low) / 3), float(low + 2 * (high - low) / 3)]
    result = tuner.sweep(inside, [1])
    assert result["evaluations"] == 6 and result["shared_evaluations"] == 3
    assert result["entries"][0]["loss"] == result["entries"][1]["loss"]
    assert all(a is b for a, b in zip(*tuner.hypotheses))
    losses, _ = literal_loop(pipeline, corpus_like(files), [e["params"] for e in result["entries"]])
    assert losses == [e["loss"] for e in result["entries"]]
    # the host cut gives the same sweep
    tuner.cut_on = "host"
    again = tuner.sweep(inside + [float(high)], [1])
    assert [e["loss"] for e in again["entries"][:2]] == losses and again["shared_evaluations"] >= 3


def test_another_clustering_runs_through_the_pipeline(pipeline_dir, gpu_device, monkeypatch):
    """no dendrogram to cut: the candidates go through the pipeline's own call, on cached front ends"""
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.tuning import ClusteringTuner
    kmeans = pa.SpeakerDiarization(segmentation=os.path.join(pipeline_dir, "segmentation"),
                                   embedding=os.path.join(pipeline_dir, "embedding"),
                                   clustering="KMeansClustering").to(gpu_device)
    kmeans.instantiate({"segmentation": {"min_duration_off": 0.0}, "clustering": {}})
    calls = count_networks(kmeans, monkeypatch)
    files = corpus()[1:]
    tuner = ClusteringTuner(kmeans).prepare(files)
    assert calls == {"segmentation": 2, "embedding": 2}

    result = tuner.evaluate([{"segmentation": {"min_duration_off": gap}, "clustering": {}} for gap in (0.0, 0.5)])
    assert calls == {"segmentation": 2, "embedding": 2} and len(result["entries"]) == 2
    assert all(np.isfinite(e["loss"]) for e in result["entries"])
