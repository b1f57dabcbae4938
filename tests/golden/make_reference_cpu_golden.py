"""Regenerates tests/golden/reference_cpu_v1.npz: what the REFERENCE'S OWN CODE returns in the CPU parity tests
tests/test_oracle_vs_reference_files.py and tests/test_reference_pipeline.py, on their seeded inputs.

pyannote.audio 4.0.7 is loaded by tests/refharness.py (stand-ins only for the absent third-party packages, see that
file); the reference's source tree is needed here and nowhere else: the tests compare the oracle and the product with
this file.  Arrays are stored as they are where they are small, and as `digest` (dtype, shape, SHA-256 of the bytes:
the tests compare bit for bit) where they are not.  Torch runs on GOLDEN_THREADS host threads here and in the tests,
so that a float32 sum is associated the same way on both sides.

Run from the repository root:  python tests/golden/make_reference_cpu_golden.py /path/to/reference/src"""
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("PYANNOTE_SKIP_DEPENDENCY_CHECK", "1")

import refharness  # noqa: E402
from conftest import GOLDEN_THREADS, digest, turn_strings, write_pipeline_dir  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference_cpu_v1.npz")
AHC_PARAMS = {"clustering": {"method": "centroid", "min_cluster_size": 12, "threshold": 0.7045654963945799},
              "segmentation": {"min_duration_off": 0.0}}
RESNETS = [("ResNet34", 298), ("ResNet152", 67), ("ResNet221", 40), ("ResNet293", 33)]
POWERSETS = [(3, 2), (4, 2), (3, 3), (2, 1)]
SPANS = [None, 0.4, 1.0, 3.0, 30.0]
DIARIZATIONS = [(17.0, 3, {}), (19.5, 8, {"num_speakers": 2}), (16.0, 5, {"min_speakers": 2, "max_speakers": 3})]
SSERIOUSS = [("WAVLM_BASE", -1), ("tiny", -1), ("tiny", 2)]


def randomise_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
                m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))


def turns(annotation):
    return turn_strings((s.start, s.end, l) for s, _, l in annotation.itertracks(yield_label=True))


def hooked():
    seen = {}

    def hook(name, artefact, file=None, **kw):
        if artefact is not None:      # (copied: apply() later caps `count.data` in place)
            seen[name] = np.array(getattr(artefact, "data", artefact), copy=True)
    return seen, hook


def reference_files(out):
    """tests/test_oracle_vs_reference_files.py"""
    import oracle.vbx as ov
    with refharness.reference_modules() as r:
        resnet = r.load("pyannote.audio.models.embedding.wespeaker.resnet")
        pooling = r.load("pyannote.audio.models.blocks.pooling")
        powerset = r.load("pyannote.audio.utils.powerset")
        rf = r.load("pyannote.audio.utils.receptive_field")
        vbx = r.load("pyannote.audio.utils.vbx")

    for name, frames in RESNETS:
        torch.manual_seed(11)
        theirs = getattr(resnet, name)(80, 256, pooling_func="TSTP", two_emb_layer=False)
        randomise_bn(theirs, 5)
        theirs.eval()
        out[f"resnet_{name}_keys"] = np.array(list(theirs.state_dict()))
        g = torch.Generator().manual_seed(3)
        fbank = torch.randn(2, frames, 80, generator=g)
        weights = (torch.rand(2, 589, generator=g) < 0.7).float()
        with torch.inference_mode():
            out[f"resnet_{name}_weighted"] = theirs(fbank.clone(), weights=weights)[1].numpy()
            out[f"resnet_{name}_unweighted"] = theirs(fbank.clone())[1].numpy()

    theirs = pooling.StatsPool()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 40, 125, generator=g)
    cases = [None, torch.rand(3, 125, generator=g), (torch.rand(3, 589, generator=g) < 0.6).float(),
             torch.rand(3, 3, 589, generator=g), torch.zeros(3, 589)]
    for i, w in enumerate(cases):
        out[f"stats_pool_{i}"] = theirs(x, weights=w).numpy()
    tstp = resnet.TSTP(in_dim=2560)
    f = torch.randn(2, 256, 10, 38, generator=g)
    w = (torch.rand(2, 589, generator=g) < 0.5).float()
    out["tstp"] = tstp(f, weights=w).numpy()
    out["tstp_out_dim"] = np.array(tstp.get_out_dim())

    for n, k in POWERSETS:
        theirs = powerset.Powerset(n, k)
        key = f"powerset_{n}_{k}"
        out[key + "_classes"] = np.array(theirs.num_powerset_classes)
        out[key + "_mapping"] = theirs.mapping.numpy()
        g = torch.Generator().manual_seed(1)
        logp = torch.log_softmax(torch.randn(4, 57, theirs.num_powerset_classes, generator=g), dim=-1)
        ml = theirs.to_multilabel(logp)
        out[key + "_hard"] = ml.numpy()
        out[key + "_soft"] = theirs.to_multilabel(logp, soft=True).numpy()
        out[key + "_forward"] = theirs(logp).numpy()
        out[key + "_to_powerset"] = theirs.to_powerset(ml).numpy()

    ks, ss, ps, ds = [251, 3, 5, 3, 5, 3], [10, 3, 1, 3, 1, 3], [0] * 6, [1] * 6
    size = rf.multi_conv_receptive_field_size(1, ks, ss, padding=ps, dilation=ds)
    step = rf.multi_conv_receptive_field_size(2, ks, ss, padding=ps, dilation=ds) - size
    center = rf.multi_conv_receptive_field_center(0, ks, ss, padding=ps, dilation=ds)
    out["rf_sincnet"] = np.array([size, step, center])
    out["rf_sincnet_num_frames"] = np.array([rf.multi_conv_num_frames(n, ks, ss, padding=ps, dilation=ds)
                                             for n in (160000, 80000, 48000, 16000, 991, 1261, 123457)])
    ks2, ss2, ps2 = [3, 3, 3, 3, 1, 3], [1, 1, 1, 2, 1, 2], [1, 1, 1, 1, 0, 1]
    out["rf_resnet"] = np.array([(rf.multi_conv_receptive_field_center(f, ks2, ss2, padding=ps2, dilation=[1] * 6),
                                  rf.multi_conv_receptive_field_size(f + 1, ks2, ss2, padding=ps2, dilation=[1] * 6))
                                 for f in (0, 1, 7)])
    out["rf_fbank_num_frames"] = np.array([rf.conv1d_num_frames(n, kernel_size=400, stride=160, padding=0, dilation=1)
                                           for n in (48000, 160000)])

    d = ov.synth_plda(tempfile.mkdtemp(), seed=9)
    xvec_tf, plda_tf, plda_psi = vbx.vbx_setup(os.path.join(d, "xvec_transform.npz"), os.path.join(d, "plda.npz"))
    rng = np.random.default_rng(4)
    centres = rng.standard_normal((4, 256))
    labels = rng.integers(0, 4, 300)
    emb = (centres[labels] + 0.3 * rng.standard_normal((300, 256))).astype(np.float32)
    fea = plda_tf(xvec_tf(emb), lda_dim=128)
    out["vbx_fea"] = digest(fea)
    out["vbx_phi"] = plda_psi[:128]
    init = (labels + rng.integers(0, 2, 300)) % 5
    from scipy.special import softmax
    for i, (Fa, Fb) in enumerate([(0.07, 0.8), (0.3, 2.0)]):
        q, pi = vbx.cluster_vbx(init, fea, plda_psi[:128], Fa=Fa, Fb=Fb, maxIters=20)
        out[f"vbx_q_{i}"], out[f"vbx_pi_{i}"] = q, pi
        q0 = np.zeros((300, 5))
        q0[range(300), init] = 1.0
        q0 = softmax(q0 * 7.0, axis=1)
        out[f"vbx_elbo_{i}"] = np.asarray(vbx.VBx(fea, plda_psi[:128], Fa=Fa, Fb=Fb, pi=5, gamma=q0, maxIters=20)[2])


def reference_pipeline(out):
    """tests/test_reference_pipeline.py"""
    import oracle.models as om
    import oracle.vbx as ov
    from oracle.synthetic import calibrated_multilabel_pyannet, calibrated_pyannet, calibrated_wespeaker
    from oracle.synthetic import synth_conversation
    from pyannote_audio_amd.audio import Audio
    from pyannote_audio_amd.model import load_checkpoint, save_checkpoint, segmentation_specifications
    seg_o, emb_o = calibrated_pyannet(calib_seconds=40.0), calibrated_wespeaker(calib_seconds=12.0)
    model_dir = tempfile.mkdtemp()
    write_pipeline_dir(model_dir, seg_o, emb_o)
    ov.synth_plda(os.path.join(model_dir, "plda"))
    with refharness.reference_modules(third_party=True) as r:
        r.load_pipelines()
        Model = sys.modules["pyannote.audio"].Model
        Inference = sys.modules["pyannote.audio"].Inference
        SpeakerDiarization = sys.modules["pyannote.audio.pipelines"].SpeakerDiarization
        clustering = sys.modules["pyannote.audio.pipelines.clustering"]
        signal = r.load("pyannote.audio.utils.signal")
        core = sys.modules["pyannote.core"]

        def pipeline(d, clustering="AgglomerativeClustering", params=AHC_PARAMS):
            return SpeakerDiarization(
                segmentation=os.path.join(d, "segmentation"), embedding=os.path.join(d, "embedding"),
                plda=os.path.join(d, "plda"), clustering=clustering, embedding_exclude_overlap=True,
                segmentation_batch_size=32, embedding_batch_size=32).instantiate(params)

        # -- the reference's loader on the product's checkpoints
        seg_r = Model.from_pretrained(os.path.join(model_dir, "segmentation"))
        emb_r = Model.from_pretrained(os.path.join(model_dir, "embedding"))
        spec = seg_r.specifications
        rf = seg_r.receptive_field
        out["loader_classes"] = np.array([type(seg_r).__name__, type(seg_r).__module__, type(emb_r).__name__])
        out["loader_spec"] = np.array([spec.powerset, spec.duration, spec.num_powerset_classes, len(spec.classes),
                                       spec.powerset_max_classes], dtype=np.float64)
        out["loader_rf"] = np.array([rf.duration * 16000, rf.step * 16000, rf.start])
        out["loader_num_frames"] = np.array([seg_r.num_frames(160000), seg_r.num_frames(80000)])
        g = torch.Generator().manual_seed(5)
        wav = (0.1 * torch.randn(3, 1, 160000, generator=g)).clamp(-1, 1)
        masks = (torch.rand(3, 589, generator=g) < 0.6).float()
        with torch.inference_mode():
            out["loader_seg"] = digest(seg_r(wav))
            out["loader_emb_weighted"] = emb_r(wav[:, :, :48000], weights=masks).numpy()
            out["loader_emb"] = emb_r(wav[:2]).numpy()

        # -- compute_fbank with fbank_centering_span, from the reference's file
        wespeaker = r.load("pyannote.audio.models.embedding.wespeaker")
        resnet = r.load("pyannote.audio.models.embedding.wespeaker.resnet")

        class Centred(wespeaker.BaseWeSpeakerResNet):
            def __init__(self, fbank_centering_span=None):
                super().__init__(fbank_centering_span=fbank_centering_span)
                self.resnet = resnet.ResNet34(80, 256, pooling_func="TSTP", two_emb_layer=False)

        for i, span in enumerate(SPANS):
            torch.manual_seed(21)
            theirs = Centred(fbank_centering_span=span).eval()
            torch.manual_seed(21)
            ours = om.WeSpeakerResNet34(fbank_centering_span=span).eval()
            # (the test builds the oracle model from the same seed instead of loading this one's weights)
            assert all(torch.equal(a, b) for a, b in zip(theirs.state_dict().values(), ours.state_dict().values()))
            out[f"centering_{i}_hparams"] = np.array([str(theirs.hparams.fbank_centering_span),
                                                      theirs.hparams.window_type])
            g = torch.Generator().manual_seed(9)
            w = (0.1 * torch.randn(2, 1, 40000, generator=g)).clamp(-1, 1)
            with torch.inference_mode():
                out[f"centering_{i}_fbank"] = digest(theirs.compute_fbank(w))
                out[f"centering_{i}_embedding"] = theirs(w).numpy()

        # -- hyper-parameters the reference's classes do not take
        ckpt = load_checkpoint(os.path.join(model_dir, "embedding", "pytorch_model.bin"))
        path = os.path.join(tempfile.mkdtemp(), "odd.bin")
        save_checkpoint(path, ckpt["state_dict"], dict(ckpt["hyper_parameters"], fbank_centering_span=3.0,
                                                       snip_edges=False),
                        ("pyannote.audio.models.embedding.wespeaker", "WeSpeakerResNet34"),
                        ckpt["pyannote.audio"]["specifications"])
        theirs = Model.from_pretrained(path)
        out["dropped_hparams"] = np.array([str(theirs.hparams.fbank_centering_span), str(theirs.hparams.snip_edges)])

        # -- Inference on the 30 s fixture
        sample, sr = Audio(16000, mono="downmix")(os.path.join(ROOT, "tests", "golden", "sample.wav"))
        inference = Inference(seg_r, skip_aggregation=True, batch_size=8)
        swf = inference({"waveform": sample, "sample_rate": sr})
        out["inference_window"] = np.array([swf.sliding_window.duration, swf.sliding_window.step])
        out["inference_sample"] = digest(swf.data)
        out["inference_short"] = digest(inference({"waveform": sample[:, : 16000 * 13 + 4321], "sample_rate": sr}).data)

        # -- SpeakerDiarization.apply, AHC
        for i, (seconds, seed, kwargs) in enumerate(DIARIZATIONS):
            conv, _ = synth_conversation(seconds, seed=seed)
            seen, hook = hooked()
            res = pipeline(model_dir)({"waveform": conv, "sample_rate": 16000, "uri": "conv"}, hook=hook, **kwargs)
            key = f"diarization_{i}"
            out[key + "_segmentation"] = digest(seen["segmentation"])
            out[key + "_count"] = seen["speaker_counting"].reshape(-1)
            out[key + "_embeddings"] = digest(seen["embeddings"])
            out[key + "_turns"] = turns(res.speaker_diarization)
            out[key + "_exclusive_turns"] = turns(res.exclusive_speaker_diarization)
            out[key + "_centroids"] = np.asarray(res.speaker_embeddings)

        # -- the clustering classes on seeded embeddings
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
        swf = core.SlidingWindowFeature(seg, core.SlidingWindow(start=0.0, duration=10.0, step=1.0))
        for i, kw in enumerate(({}, {"num_clusters": 3}, {"min_clusters": 5, "max_clusters": 6})):
            ahc = clustering.AgglomerativeClustering(metric="cosine").instantiate(AHC_PARAMS["clustering"])
            bounds = {"num_clusters": None, "min_clusters": 1, "max_clusters": np.inf}
            bounds.update(kw)
            if bounds["num_clusters"]:
                bounds["min_clusters"] = bounds["max_clusters"] = bounds["num_clusters"]
            hard, soft, cent = ahc(embeddings=emb.copy(), segmentations=swf, **bounds)
            out[f"ahc_{i}_hard"], out[f"ahc_{i}_soft"], out[f"ahc_{i}_centroids"] = hard, digest(soft), digest(cent)

        # -- VBxClustering pipeline
        conv, _ = synth_conversation(17.0, seed=11)
        seen, hook = hooked()
        params = {"segmentation": {"min_duration_off": 0.0}, "clustering": {"threshold": 0.6, "Fa": 0.07, "Fb": 0.8}}
        res = pipeline(model_dir, clustering="VBxClustering", params=params)(
            {"waveform": conv, "sample_rate": 16000, "uri": "conv"}, hook=hook)
        assert np.array_equal(seen["segmentation"], seen["segmentation"].astype(np.uint8))
        out["vbx_pipeline_segmentation"] = seen["segmentation"].astype(np.uint8)
        out["vbx_pipeline_embeddings"] = seen["embeddings"]
        out["vbx_pipeline_count"] = seen["speaker_counting"].reshape(-1)
        out["vbx_pipeline_discrete"] = seen["discrete_diarization"]
        out["vbx_pipeline_centroid_dim"] = np.array(res.speaker_embeddings.shape[1])
        out["vbx_pipeline_turns"] = turns(res.speaker_diarization)

        # -- Binarize (class) and binarize (function)
        rng = np.random.default_rng(2)
        data = (rng.uniform(size=(4000, 3)) < 0.5).astype(np.float32)
        for k in range(3):
            data[:, k] = np.repeat(data[::40, k], 40)
        sw = core.SlidingWindow(start=0.0, duration=991 / 16000, step=270 / 16000)
        ann = signal.Binarize(onset=0.5, offset=0.5, min_duration_on=0.0, min_duration_off=0.0)(
            core.SlidingWindowFeature(data, sw))
        out["binarize_class"] = np.array(sorted((s.start, s.end, int(l)) for s, _, l in
                                                ann.itertracks(yield_label=True)), dtype=np.float64)
        rng = np.random.default_rng(6)
        scores = rng.uniform(size=(7, 120, 3)).astype(np.float32)
        scores[2, 10:14, 1] = np.nan
        scores[3, ::9, 0] = 0.6
        scores[4, ::7, 2] = 0.4
        swf = core.SlidingWindowFeature(scores, core.SlidingWindow(start=0.0, duration=10.0, step=1.0))
        for i, (onset, offset, init) in enumerate([(0.5, None, False), (0.6, 0.4, None), (0.6, 0.4, True),
                                                   (0.3, None, None)]):
            out[f"binarize_function_{i}"] = signal.binarize(swf, onset=onset, offset=offset, initial_state=init).data

        # -- a multi-label (non-powerset) segmentation checkpoint
        seg_m = calibrated_multilabel_pyannet(calib_seconds=40.0)
        d = tempfile.mkdtemp()
        write_pipeline_dir(d, seg_m, emb_o, powerset=False)
        ov.synth_plda(os.path.join(d, "plda"))
        params = {"clustering": AHC_PARAMS["clustering"], "segmentation": {"threshold": 0.5, "min_duration_off": 0.0}}
        conv, _ = synth_conversation(16.0, seed=14)
        seen, hook = hooked()
        res = pipeline(d, params=params)({"waveform": conv, "sample_rate": 16000, "uri": "conv"}, hook=hook)
        out["multilabel_segmentation"] = digest(seen["segmentation"])
        out["multilabel_count"] = seen["speaker_counting"].reshape(-1)
        out["multilabel_embeddings"] = digest(seen["embeddings"])
        out["multilabel_turns"] = turns(res.speaker_diarization)
        out["multilabel_exclusive_turns"] = turns(res.exclusive_speaker_diarization)

        # -- XVectorSincNet
        xv = r.load("pyannote.audio.models.embedding.xvector")
        ours = om.seeded_xvector()
        theirs = xv.XVectorSincNet()
        out["xvector_keys"] = np.array(list(theirs.state_dict()))
        theirs.load_state_dict(ours.state_dict())
        theirs.eval()
        g = torch.Generator().manual_seed(2)
        wav = (0.1 * torch.randn(2, 1, 48000, generator=g)).clamp(-1, 1)
        weights = (torch.rand(2, 173, generator=g) < 0.6).float()
        with torch.inference_mode():
            out["xvector_weighted"] = theirs(wav, weights=weights).numpy()
            out["xvector_unweighted"] = theirs(wav).numpy()
        out["xvector_dimension"] = np.array(theirs.dimension)
        out["xvector_num_frames"] = np.array([theirs.num_frames(n) for n in (4771, 4770, 48000, 80000, 160000)])
        out["xvector_rf"] = np.array([theirs.receptive_field_size(1), theirs.receptive_field_center(0)])
        lower, upper = 2, 8000
        with torch.inference_mode():
            while lower + 1 < upper:
                middle = (lower + upper) // 2
                try:
                    theirs(torch.randn(1, 1, middle))
                    upper = middle
                except Exception:
                    lower = middle
        out["xvector_min_num_samples"] = np.array(upper)

        # -- SSeRiouSS
        for i, (wav2vec, layer) in enumerate(SSERIOUSS):
            config = "WAVLM_BASE" if wav2vec == "WAVLM_BASE" else dict(om.TINY_WAV2VEC2)
            ours = om.seeded_sseriouss(wav2vec=config, num_layers=2, wav2vec_layer=layer)
            hparams = {"wav2vec": config, "wav2vec_frozen": False, "wav2vec_layer": layer,
                       "lstm": {"hidden_size": 128, "num_layers": 2, "bidirectional": True, "monolithic": True,
                                "dropout": 0.0}, "linear": {"hidden_size": 128, "num_layers": 2},
                       "sample_rate": 16000, "num_channels": 1}
            path = os.path.join(tempfile.mkdtemp(), "pytorch_model.bin")
            save_checkpoint(path, ours.state_dict(), hparams,
                            ("pyannote.audio.models.segmentation.SSeRiouSS", "SSeRiouSS"),
                            segmentation_specifications(10.0))
            theirs = Model.from_pretrained(path)
            out[f"sseriouss_{i}_class"] = np.array(type(theirs).__name__)
            out[f"sseriouss_{i}_keys"] = np.array(list(theirs.state_dict()))
            g = torch.Generator().manual_seed(4)
            wav = (0.1 * torch.randn(2, 1, 24000, generator=g)).clamp(-1, 1)
            with torch.inference_mode():
                out[f"sseriouss_{i}_output"] = theirs(wav).numpy()
            out[f"sseriouss_{i}_num_frames"] = np.array([theirs.num_frames(n) for n in (24000, 160000, 80000, 400, 399)])
            out[f"sseriouss_{i}_rf"] = np.array([theirs.receptive_field_size(1), theirs.receptive_field_size(2),
                                                 theirs.receptive_field_center(0)])


def main():
    if len(sys.argv) > 1:
        refharness.REF_SRC = sys.argv[1]
        refharness.REF_PKG = os.path.join(sys.argv[1], "pyannote", "audio")
    warnings.simplefilter("ignore")
    torch.set_num_threads(GOLDEN_THREADS)
    out = {}
    reference_files(out)
    reference_pipeline(out)
    np.savez_compressed(OUT, **out)
    print("written", OUT, len(out), "arrays,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
