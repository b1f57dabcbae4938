"""The REFERENCE'S OWN PIPELINE against the oracle -- stage by stage and end to end.

What the reference returned on the seeded inputs below is stored in tests/golden/reference_cpu_v1.npz (generator:
tests/golden/make_reference_cpu_golden.py, which loads pyannote.audio 4.0.7 through tests/refharness.py with stand-ins
for the absent third-party packages (lightning, pyannote.core / .pipeline, asteroid_filterbanks, torchaudio's kaldi.fbank:
ours on both sides of the comparison, i.e. still unpinned).  Everything else that runs below is the
reference's code: `Model.from_pretrained`, `PyanNet` / `SincNet`, `WeSpeakerResNet34`, `Inference.slide /
aggregate`, `SpeakerDiarization.apply` (speaker_count, get_embeddings, reconstruct, to_diarization),
`AgglomerativeClustering` / `VBxClustering` / `PLDA`, `Binarize`, the label mapping.

The checkpoints are the seeded synthetic ones, written by the PRODUCT's `save_checkpoint` and read by the
REFERENCE's loader -- which also pins the checkpoint format.  All comparisons are
bit for bit, on the generator's host thread count (conftest.GOLDEN_THREADS); an array too large for a fixture is
compared through its `conftest.digest`."""
import os

import numpy as np
import pytest
import torch

from conftest import digest, turn_strings

pytestmark = pytest.mark.usefixtures("golden_threads")

AHC_PARAMS = {"clustering": {"method": "centroid", "min_cluster_size": 12, "threshold": 0.7045654963945799},
              "segmentation": {"min_duration_off": 0.0}}


@pytest.fixture(scope="module")
def models():
    from oracle.synthetic import calibrated_pyannet, calibrated_wespeaker
    return calibrated_pyannet(calib_seconds=40.0), calibrated_wespeaker(calib_seconds=12.0)


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory, models):
    import oracle.vbx as ov
    from conftest import write_pipeline_dir
    d = str(tmp_path_factory.mktemp("ref_sd31"))
    write_pipeline_dir(d, *models)
    ov.synth_plda(os.path.join(d, "plda"))
    return d


@pytest.fixture(scope="module")
def ref():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_cpu_v1.npz")) as z:
        return {k: z[k] for k in z.files}


def test_reference_loader_reads_product_checkpoints(ref, model_dir, models):
    """core/model.py:497-655 on checkpoints written by pyannote_audio_amd.model.save_checkpoint: the right
    classes, specifications and hyper-parameters come back; PyanNet / WeSpeakerResNet34 forward equal the
    oracle modules bit for bit (PyanNet.py:211-240, sincnet.py:163-184, wespeaker/__init__.py:324-372)."""
    seg_o, emb_o = models
    seg_class, seg_module, emb_class = ref["loader_classes"]
    assert seg_class == "PyanNet" and emb_class == "WeSpeakerResNet34"
    assert seg_module.startswith("pyannote.audio.models.segmentation")
    powerset, duration, num_powerset_classes, num_classes, powerset_max_classes = ref["loader_spec"]
    assert powerset and duration == 10.0 and num_powerset_classes == 7
    assert num_classes == 3 and powerset_max_classes == 2
    rf_duration, rf_step, rf_start = ref["loader_rf"]
    assert (round(rf_duration), round(rf_step)) == (991, 270) and rf_start == 0.0
    g = torch.Generator().manual_seed(5)
    wav = (0.1 * torch.randn(3, 1, 160000, generator=g)).clamp(-1, 1)
    masks = (torch.rand(3, 589, generator=g) < 0.6).float()
    with torch.inference_mode():
        assert digest(seg_o(wav)) == ref["loader_seg"]
        assert np.array_equal(emb_o(wav[:, :, :48000], weights=masks).numpy(), ref["loader_emb_weighted"])
        assert np.array_equal(emb_o(wav[:2]).numpy(), ref["loader_emb"])
    assert list(ref["loader_num_frames"]) == [589, 293]


@pytest.mark.parametrize("span", [None, 0.4, 1.0, 3.0, 30.0])
def test_reference_compute_fbank_centering_span_equals_oracle(ref, span):
    """wespeaker/__init__.py:113-157 executed from the reference's file: global mean (`None`) and the running mean of
    `fbank_centering_span` seconds (a window shorter than the chunk, about the chunk, far longer than the chunk) --
    the oracle's restatement is bit-identical, and so is the embedding of the whole model.  The stock classes do not
    take `fbank_centering_span` (:346-372): the reference-side model is what a user of the reference would write, a
    subclass that forwards it to `BaseWeSpeakerResNet`.  It was built after torch.manual_seed(21), and so is the
    oracle's model: the generator checked that both draw the same initial weights."""
    import oracle.models as om
    i = [None, 0.4, 1.0, 3.0, 30.0].index(span)
    assert list(ref[f"centering_{i}_hparams"]) == [str(span), "hamming"]
    torch.manual_seed(21)
    ours = om.WeSpeakerResNet34(fbank_centering_span=span).eval()
    g = torch.Generator().manual_seed(9)
    wav = (0.1 * torch.randn(2, 1, 40000, generator=g)).clamp(-1, 1)
    want = ref[f"centering_{i}_fbank"]
    with torch.inference_mode():
        got = ours.compute_fbank(wav)
        assert got.shape == (2, 248, 80) and digest(got) == want
        assert np.array_equal(ours(wav).numpy(), ref[f"centering_{i}_embedding"])
        plain = om.WeSpeakerResNet34().compute_fbank(wav)
    # (a window that covers the chunk from every frame is the global mean up to the order of the float32 sums)
    assert (span is None) == (digest(plain) == want)
    if span == 30.0:
        assert torch.allclose(plain, got, atol=1e-4)


def test_reference_loader_drops_hyper_parameters_its_classes_do_not_take(ref, model_dir, tmp_path):
    """A WeSpeakerResNet34 checkpoint that SAYS fbank_centering_span = 3.0 / snip_edges = False: the reference's class
    does not take either (wespeaker/__init__.py:346-372), its loader drops them (Lightning's `_load_state`, restated in
    tests/refharness.py -- Lightning itself is absent: unpinned) and computes the defaults.  The product does the same
    and says so; a hyper-parameter that counts and that the HIP front end is not built for is refused."""
    import warnings
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.model import load_checkpoint, save_checkpoint
    src = os.path.join(model_dir, "embedding", "pytorch_model.bin")
    ckpt = load_checkpoint(src)
    odd = dict(ckpt["hyper_parameters"], fbank_centering_span=3.0, snip_edges=False)
    path = str(tmp_path / "odd.bin")
    save_checkpoint(path, ckpt["state_dict"], odd, ("pyannote.audio.models.embedding.wespeaker", "WeSpeakerResNet34"),
                    ckpt["pyannote.audio"]["specifications"])
    assert list(ref["dropped_hparams"]) == ["None", "True"]   # what the reference's loader made of the same file
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        ours = pa.Model.from_pretrained(path)
    assert ours.fbank_center_kernel == 0
    text = " ".join(str(w.message) for w in seen)
    assert "fbank_centering_span = 3.0" in text and "snip_edges = False" in text and "as in the reference" in text


def test_reference_inference_on_sample_wav(ref, model_dir, models):
    """BASELINE configs[0] on the reference's own `Inference` (core/inference.py:217-373) over its own
    30 s fixture: (21, 589, 3) hard multilabel chunks, equal to oracle.pipeline.slide."""
    from oracle import pipeline as op
    from pyannote_audio_amd.audio import Audio
    seg_o, _ = models
    wav, sr = Audio(16000, mono="downmix")(os.path.join(os.path.dirname(__file__), "golden", "sample.wav"))
    got = op.slide(seg_o, wav, sr, 10.0, 1.0, 8)
    assert got.shape == (21, 589, 3)
    assert tuple(ref["inference_window"]) == (10.0, 1.0)
    assert digest(got) == ref["inference_sample"]
    # a file that ends in an orphan chunk (core/inference.py:270-278)
    short = wav[:, : 16000 * 13 + 4321]
    got = op.slide(seg_o, short, sr, 10.0, 1.0, 8)
    assert got.shape == (5, 589, 3) and digest(got) == ref["inference_short"]


@pytest.mark.parametrize("seconds,seed,kwargs", [
    (17.0, 3, {}),
    (19.5, 8, {"num_speakers": 2}),
    (16.0, 5, {"min_speakers": 2, "max_speakers": 3}),
])
def test_reference_speaker_diarization_equals_oracle(ref, model_dir, models, seconds, seed, kwargs):
    """`SpeakerDiarization.apply` (pipelines/speaker_diarization.py:530-784) with the 3.1 configuration:
    every artefact the hook sees and the final annotations equal oracle.pipeline.diarize."""
    from oracle.pipeline import diarize
    from oracle.synthetic import synth_conversation
    seg_o, emb_o = models
    conv, _ = synth_conversation(seconds, seed=seed)
    key = f"diarization_{[17.0, 19.5, 16.0].index(seconds)}"
    want = diarize(seg_o, emb_o, conv, exclude_overlap=True, **kwargs)
    assert digest(np.asarray(want.segmentations, dtype=np.float32)) == ref[key + "_segmentation"]
    assert np.array_equal(ref[key + "_count"], want.count.reshape(-1))
    assert digest(np.asarray(want.embeddings, dtype=np.float32)) == ref[key + "_embeddings"]
    assert list(ref[key + "_turns"]) == turn_strings(want.diarization)
    assert list(ref[key + "_exclusive_turns"]) == turn_strings(want.exclusive_diarization)
    assert np.array_equal(ref[key + "_centroids"], want.centroids)
    assert len(want.diarization) > 5 and len({l for _, _, l in want.diarization}) >= 2


def test_reference_clustering_classes_equal_oracle(ref, models):
    """`AgglomerativeClustering.__call__` and `VBxClustering.__call__` (pipelines/clustering.py:214-480,
    :550-669) on seeded embeddings: hard clusters, soft scores and centroids equal the oracle's."""
    import oracle.vbx as ov
    from oracle.pipeline import clustering as oracle_ahc
    rng = np.random.default_rng(12)
    C, S, D, F = 140, 3, 256, 589
    centres = rng.standard_normal((4, D))
    who = rng.integers(0, 4, (C, S))
    emb = (centres[who] + 0.35 * rng.standard_normal((C, S, D))).astype(np.float32)
    seg = np.zeros((C, F, S), dtype=np.float32)
    for c in range(C):
        for s in range(S):
            if rng.uniform() < 0.8:
                a = rng.integers(0, 300)
                seg[c, a:a + rng.integers(60, 280), s] = 1.0
    emb[5, 1] = np.nan
    for i, kw in enumerate(({}, {"num_clusters": 3}, {"min_clusters": 5, "max_clusters": 6})):
        bounds = {"num_clusters": None, "min_clusters": 1, "max_clusters": np.inf}
        bounds.update(kw)
        if bounds["num_clusters"]:
            bounds["min_clusters"] = bounds["max_clusters"] = bounds["num_clusters"]
        ohard, osoft, ocent = oracle_ahc(emb.copy(), seg, **bounds, **AHC_PARAMS["clustering"])
        assert np.array_equal(ref[f"ahc_{i}_hard"], ohard) and digest(osoft) == ref[f"ahc_{i}_soft"]
        assert digest(ocent) == ref[f"ahc_{i}_centroids"]


def test_reference_vbx_pipeline_equals_oracle(ref, model_dir, models):
    """The 4.x / community-1 default (`clustering="VBxClustering"`, speaker_diarization.py:210, 280-285):
    the reference's pipeline with a synthetic PLDA vs the oracle's stages + oracle.vbx.vbx_clustering."""
    import oracle.vbx as ov
    seg_o, emb_o = models
    params = {"segmentation": {"min_duration_off": 0.0}, "clustering": {"threshold": 0.6, "Fa": 0.07, "Fb": 0.8}}
    plda = ov.PLDA(os.path.join(model_dir, "plda", "xvec_transform.npz"),
                   os.path.join(model_dir, "plda", "plda.npz"))
    # the reference's segmentation and embeddings of a 17 s synthetic conversation (synth_conversation(17.0, seed=11))
    seg = ref["vbx_pipeline_segmentation"].astype(np.float32)
    hard, _, cent = ov.vbx_clustering(ref["vbx_pipeline_embeddings"], seg, plda, **params["clustering"])
    # the reference's discrete diarization restated from the oracle's clusters
    from oracle import pipeline as op
    chunks = op.SW(0.0, 10.0, 1.0)
    frames = op.receptive_field(seg_o, 16000)
    count, count_frames = op.speaker_count(seg, chunks, frames)
    assert np.array_equal(ref["vbx_pipeline_count"], count.reshape(-1))
    hard = hard.copy()
    hard[np.sum(seg, axis=1) == 0] = -2
    discrete = op.reconstruct(seg, chunks, hard, count.astype(np.int8), count_frames)
    got = ref["vbx_pipeline_discrete"]
    assert got.shape == discrete.shape and np.array_equal(got, discrete)
    assert ref["vbx_pipeline_centroid_dim"] == 256 and len(ref["vbx_pipeline_turns"]) > 3


def test_reference_binarize_equals_oracle(ref):
    """`Binarize.__call__` (utils/signal.py:254-318) on a random {0,1} frame matrix vs oracle.pipeline.binarize."""
    from oracle import pipeline as op
    rng = np.random.default_rng(2)
    data = (rng.uniform(size=(4000, 3)) < 0.5).astype(np.float32)
    for k in range(3):                       # long runs instead of salt-and-pepper
        data[:, k] = np.repeat(data[::40, k], 40)
    frames = op.SW(0.0, 991 / 16000, 270 / 16000)
    want = op.binarize(data, frames)
    got = [tuple(row) for row in ref["binarize_class"]]
    assert got == sorted((s, e, int(l)) for s, e, _, l in want)


def test_reference_binarize_function_equals_oracle(ref):
    """`binarize` (utils/signal.py:78-204; hysteresis thresholding, ndarray and SlidingWindowFeature forms)
    vs oracle.pipeline.hysteresis, incl. NaN scores, scores exactly on a threshold, every initial state."""
    from oracle import pipeline as op
    rng = np.random.default_rng(6)
    scores = rng.uniform(size=(7, 120, 3)).astype(np.float32)
    scores[2, 10:14, 1] = np.nan
    scores[3, ::9, 0] = 0.6            # exactly on the onset
    scores[4, ::7, 2] = 0.4            # exactly on the offset
    for i, (onset, offset, init) in enumerate([(0.5, None, False), (0.6, 0.4, None), (0.6, 0.4, True),
                                               (0.3, None, None)]):
        want = ref[f"binarize_function_{i}"]
        got = op.hysteresis(scores, onset=onset, offset=offset, initial_state=init)
        assert want.shape == got.shape and np.array_equal(got, want)


def test_reference_non_powerset_pipeline_equals_oracle(ref, tmp_path, models):
    """a14: a multi-label (non-powerset) segmentation checkpoint through the reference's pipeline --
    `binarize(segmentations, onset=threshold, initial_state=False)` (speaker_diarization.py:599-606), counting /
    masks / clustering on the binary form, reconstruction from the RAW scores (:687-691) -- vs the oracle."""
    from oracle.pipeline import diarize
    from oracle.synthetic import calibrated_multilabel_pyannet, synth_conversation
    seg_o = calibrated_multilabel_pyannet(calib_seconds=40.0)
    _, emb_o = models
    conv, _ = synth_conversation(16.0, seed=14)
    want = diarize(seg_o, emb_o, conv, exclude_overlap=True, segmentation_threshold=0.5)
    assert want.raw_segmentations.dtype == np.float32 and 0.0 < want.raw_segmentations.min() < 0.5
    assert digest(want.raw_segmentations) == ref["multilabel_segmentation"]
    assert np.array_equal(ref["multilabel_count"], want.count.reshape(-1))
    assert digest(np.asarray(want.embeddings, dtype=np.float32)) == ref["multilabel_embeddings"]
    assert list(ref["multilabel_turns"]) == turn_strings(want.diarization)
    assert list(ref["multilabel_exclusive_turns"]) == turn_strings(want.exclusive_diarization)
    assert len(want.diarization) > 5 and len({l for _, _, l in want.diarization}) >= 2


def test_reference_xvector_sincnet_equals_oracle(ref):
    """f3: `XVectorSincNet` (models/embedding/xvector.py:205-349) from the reference vs oracle.models.
    XVectorSincNet with the same state dict: same keys, identical embeddings with / without weights, the
    reference's frame geometry and the `min_num_samples` bisection of the pipeline wrapper
    (pipelines/speaker_verification.py:688-702) reproduced by the product's closed form."""
    import oracle.models as om
    import pyannote_audio_amd.model as pm
    ours = om.seeded_xvector()
    assert list(ref["xvector_keys"]) == list(ours.state_dict())
    g = torch.Generator().manual_seed(2)
    wav = (0.1 * torch.randn(2, 1, 48000, generator=g)).clamp(-1, 1)
    weights = (torch.rand(2, 173, generator=g) < 0.6).float()
    with torch.inference_mode():
        assert np.array_equal(ours(wav, weights=weights).numpy(), ref["xvector_weighted"])
        assert np.array_equal(ours(wav).numpy(), ref["xvector_unweighted"])
    assert ref["xvector_dimension"] == 512
    product = pm.XVectorSincNet.__new__(pm.XVectorSincNet)
    product.hparams = {"sincnet": {"stride": 10}}
    for n, want in zip((4771, 4770, 48000, 80000, 160000), ref["xvector_num_frames"]):
        assert product.num_frames(n) == want
    assert [product.receptive_field_size(1), product.receptive_field_center(0)] == list(ref["xvector_rf"])
    # the wrapper's bisection: shortest waveform the reference model embeds without raising
    from pyannote_audio_amd.speaker_verification import first_true
    assert ref["xvector_min_num_samples"] == first_true(lambda n: product.num_frames(n) > 0, 2, 8000)


@pytest.mark.parametrize("wav2vec,layer", [("WAVLM_BASE", -1), ("tiny", -1), ("tiny", 2)])
def test_reference_sseriouss_equals_oracle(ref, tmp_path, wav2vec, layer):
    """f3: the reference's `SSeRiouSS` (models/segmentation/SSeRiouSS.py:42-328 -- layer weighting :307-313,
    LSTM :315-322, head :324-328, frame geometry :217-287), loaded by the reference's loader from a checkpoint
    the product wrote, vs oracle.models.SSeRiouSS.  BOTH run on oracle/wav2vec2.py, the (unpinned) restatement
    of torchaudio's wav2vec 2.0 / WavLM encoder: this pins the reference's own file, not torchaudio."""
    import oracle.models as om
    from pyannote_audio_amd.model import save_checkpoint, segmentation_specifications
    config = "WAVLM_BASE" if wav2vec == "WAVLM_BASE" else dict(om.TINY_WAV2VEC2)
    ours = om.seeded_sseriouss(wav2vec=config, num_layers=2, wav2vec_layer=layer)
    hparams = {"wav2vec": config, "wav2vec_frozen": False, "wav2vec_layer": layer,
               "lstm": {"hidden_size": 128, "num_layers": 2, "bidirectional": True, "monolithic": True,
                        "dropout": 0.0}, "linear": {"hidden_size": 128, "num_layers": 2},
               "sample_rate": 16000, "num_channels": 1}
    key = f"sseriouss_{[('WAVLM_BASE', -1), ('tiny', -1), ('tiny', 2)].index((wav2vec, layer))}"
    # (the reference's loader read this checkpoint, written by the product, when the golden file was made)
    save_checkpoint(os.path.join(str(tmp_path), "pytorch_model.bin"), ours.state_dict(), hparams,
                    ("pyannote.audio.models.segmentation.SSeRiouSS", "SSeRiouSS"), segmentation_specifications(10.0))
    assert ref[key + "_class"] == "SSeRiouSS" and list(ref[key + "_keys"]) == list(ours.state_dict())
    g = torch.Generator().manual_seed(4)
    wav = (0.1 * torch.randn(2, 1, 24000, generator=g)).clamp(-1, 1)
    with torch.inference_mode():
        want, got = ref[key + "_output"], ours(wav).numpy()
    assert want.shape == got.shape and np.array_equal(got, want)
    import pyannote_audio_amd.model as pm
    product = pm.SSeRiouSS.__new__(pm.SSeRiouSS)
    product.hparams = hparams
    for n, want_n in zip((24000, 160000, 80000, 400, 399), ref[key + "_num_frames"]):
        assert product.num_frames(n) == want_n
    assert [product.receptive_field_size(1), product.receptive_field_size(2),
            product.receptive_field_center(0)] == list(ref[key + "_rf"])
