"""GPU: `ClusteringTuner.sweep_vbx` on a `VBxClustering` pipeline -- per file one linkage, one PLDA projection, one
`Dendrogram.cuts` call and the VB inferences of all candidates from batched launches -- gives, candidate by candidate,
the loss, the annotations and the VB iteration counts of the literal loop (`pipeline.instantiate(params)`,
`pipeline(file)` for every file, a fresh metric) on tests/golden/sample.wav and two crops of it, with `==`."""
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CROPS = ((0.0, 30.0), (0.0, 18.0), (9.0, 30.0))
#: within the ranges `VBxClustering` declares; on this corpus Fb = 0.8 collapses every file into one speaker after 2 to 7
#: iterations and Fb = 0.01 keeps 1 to 5 speakers after 16 to 20 (the oracle's cluster_vbx on the pipeline's own
#: embeddings; no ELBO step of any job lies within 1e-5 of the 1e-4 threshold)
FAS, FBS = (0.07, 0.5), (0.8, 0.01)
CONFIG = {}       # "yml": the config.yaml of the pipeline fixture


@pytest.fixture(scope="module")
def pipeline(tmp_path_factory, synthetic_models, gpu_device):
    """the community-1 layout of tests/test_vbx_gpu.py::test_pipeline_with_vbx_clustering"""
    import pyannote_audio_amd as pa
    from conftest import write_pipeline_dir
    from oracle.vbx import synth_plda
    root = str(tmp_path_factory.mktemp("community"))
    write_pipeline_dir(root, *synthetic_models, config_extra={
        "pipeline": {"name": "pyannote.audio.pipelines.SpeakerDiarization",
                     "params": {"clustering": "VBxClustering", "embedding": "$model/embedding",
                                "embedding_batch_size": 32, "embedding_exclude_overlap": True,
                                "plda": "$model/plda", "segmentation": "$model/segmentation",
                                "segmentation_batch_size": 32}},
        "params": {"clustering": {"threshold": 0.6, "Fa": 0.07, "Fb": 0.8},
                   "segmentation": {"min_duration_off": 0.0}}})
    shutil.copytree(synth_plda(str(tmp_path_factory.mktemp("plda"))), os.path.join(root, "plda"))
    pipeline = pa.Pipeline.from_pretrained(root).to(gpu_device)
    assert isinstance(pipeline.clustering, pa.VBxClustering)
    CONFIG["yml"] = os.path.join(root, "config.yaml")
    return pipeline


def corpus():
    """fresh file dicts: sample.wav and two crops of it, each with its part of sample.rttm (tests/test_tuning_gpu.py)"""
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


def corpus_like(files) -> list:
    """the same files without their caches (and as the dicts a user would pass)"""
    return [{key: value for key, value in file.items() if not key.startswith("training_cache/")} for file in files]


def literal_loop(pipeline, files, candidates):
    """the `literal_loop` of tests/test_tuning_gpu.py -- every candidate through the whole pipeline, file by file --
    which also notes the VB iterations of every call"""
    assert pipeline.training is False
    losses, outputs, iterations = [], [], []
    for params in candidates:
        pipeline.instantiate(params)
        metric = pipeline.get_metric()
        outputs.append([])
        iterations.append([])
        for file in files:
            diarization = pipeline(file).speaker_diarization
            metric(file["annotation"], diarization, uem=file.get("annotated"))
            outputs[-1].append(diarization)
            iterations[-1].append(pipeline.clustering.timings.get("vbx_iterations"))
        losses.append(abs(metric))
    return losses, outputs, iterations


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


@pytest.mark.parametrize("capped", [False, True])
def test_sweep_vbx_equals_the_literal_loop(pipeline, monkeypatch, capped):
    from pyannote_audio_amd.tuning import ClusteringTuner, best_entry, write_config
    pipeline.instantiate({"clustering": {"threshold": 0.6, "Fa": 0.07, "Fb": 0.8},
                          "segmentation": {"min_duration_off": 0.0}})
    files = corpus()
    if capped:      # VBx finds more than one speaker: KMeans with one cluster, no assignment constraint
        files[1]["pipeline_kwargs"] = {"max_speakers": 1}
    calls = count_networks(pipeline, monkeypatch)
    tuner = ClusteringTuner(pipeline).prepare(files)
    assert pipeline.training is False and calls == {"segmentation": 3, "embedding": 3}
    plans = [tuner._vbx_front(item) for item in tuner.prepared]
    assert all(plan is not None for plan in plans)
    print("training embeddings per file:", [plan.train.shape[0] for plan in plans])
    heights = np.concatenate([plan.tree.Z[:, 2] for plan in plans])
    thresholds = [float(t) for t in np.quantile(heights, (0.35, 0.75, 0.95))]

    result = tuner.sweep_vbx(thresholds, FAS, FBS)
    assert calls == {"segmentation": 3, "embedding": 3}                 # the sweep itself runs no network
    entries = result["entries"]
    assert len(entries) == 12 and result["evaluations"] == 36
    assert [(e["params"]["clustering"]["threshold"], e["params"]["clustering"]["Fa"], e["params"]["clustering"]["Fb"])
            for e in entries] == [(t, a, b) for t in thresholds for a in FAS for b in FBS]
    shared = dict(tuner.vbx_shared)
    print("shared:", shared, "evaluations shared:", result["shared_evaluations"])
    print("speakers VBx kept:", tuner.train_clusters)
    # the thresholds cut the files differently, and no (cut, Fa, Fb) ran twice
    assert shared["candidates"] == 36 and 3 < shared["initialisations"] <= 9
    assert shared["jobs"] == 4 * shared["initialisations"] and shared["calls"] == 3
    assert all(kept is not None and kept >= 1 for row in tuner.train_clusters for kept in row)
    assert len({kept for row in tuner.train_clusters for kept in row}) >= 3        # from one speaker to several

    hypotheses = [list(row) for row in tuner.hypotheses]
    iterations = [list(row) for row in tuner.vbx_iterations]
    losses, outputs, loop_iterations = literal_loop(pipeline, corpus_like(files), [e["params"] for e in entries])
    for c, entry in enumerate(entries):
        print(c, entry["params"]["clustering"], entry["loss"], losses[c], iterations[c], loop_iterations[c])
        assert entry["loss"] == losses[c], c
        assert iterations[c] == loop_iterations[c], c
        for f in range(len(files)):
            assert hypotheses[c][f] == outputs[c][f], (c, f)
    assert result["best"] is best_entry(entries) and result["best"] is entries[int(np.argmin(losses))]
    if capped:
        assert all(len(row[1].labels()) <= 1 for row in hypotheses)

    # a smaller budget: more calls, the same sweep
    tuner.workspace_bytes = 1
    again = tuner.sweep_vbx(thresholds, FAS, FBS)
    assert tuner.vbx_shared["calls"] == shared["jobs"] and [e["loss"] for e in again["entries"]] == losses
    assert [list(row) for row in tuner.vbx_iterations] == loop_iterations

    import yaml
    written = write_config(CONFIG["yml"], result, "dev")
    with open(written) as fp:
        config = yaml.load(fp, Loader=yaml.SafeLoader)
    assert config["params"] == result["best"]["params"]
    assert config["optimization"]["status"]["best_loss"] == float(result["best"]["loss"])
