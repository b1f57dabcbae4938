"""The oracle against the REFERENCE'S OWN CODE.

Five files of pyannote.audio 4.0.7 need nothing but torch / numpy / scipy / einops; what they return on the seeded
inputs below is stored in tests/golden/reference_cpu_v1.npz (generator: tests/golden/make_reference_cpu_golden.py,
which runs them through tests/refharness.py):

    models/embedding/wespeaker/resnet.py   ResNet34 / 152 / 221 / 293, BasicBlock, Bottleneck, TSTP
    models/blocks/pooling.py               StatsPool
    utils/powerset.py                      Powerset
    utils/receptive_field.py               frame geometry
    utils/vbx.py                           VBx, cluster_vbx, vbx_setup

Every comparison is BIT FOR BIT on seeded inputs (same host thread count as the generator: conftest.GOLDEN_THREADS);
an array too large for a fixture is compared through its `conftest.digest`."""
import os

import numpy as np
import pytest
import torch

from conftest import digest

pytestmark = pytest.mark.usefixtures("golden_threads")


@pytest.fixture(scope="module")
def ref():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_cpu_v1.npz")) as z:
        return {k: z[k] for k in z.files}


def _randomise_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
                m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))


@pytest.mark.parametrize("name,blocks,bottleneck,frames", [
    ("ResNet34", (3, 4, 6, 3), False, 298),
    ("ResNet152", (3, 8, 36, 3), True, 67),
    ("ResNet221", (6, 16, 48, 3), True, 40),
    ("ResNet293", (10, 20, 64, 3), True, 33),
])
def test_wespeaker_resnets(ref, name, blocks, bottleneck, frames):
    """wespeaker/resnet.py:84-145 (BasicBlock), :148-212 (Bottleneck), :215-260, :399-430 (ResNet),
    :37-66 (TSTP) with the wrapper's arguments (`two_emb_layer=False`, wespeaker/__init__.py:370-372):
    same state-dict keys, identical embeddings with and without pooling weights.
    The reference's model was built after torch.manual_seed(11): the oracle's, built the same way, draws the same
    initial weights (same modules in the same order)."""
    import oracle.models as om
    torch.manual_seed(11)
    ours = om.ResNet(blocks, 32, 80, 256, block=om.Bottleneck if bottleneck else om.BasicBlock)
    assert list(ours.state_dict()) == list(ref[f"resnet_{name}_keys"])
    _randomise_bn(ours, 5)
    ours.eval()
    g = torch.Generator().manual_seed(3)
    fbank = torch.randn(2, frames, 80, generator=g)
    weights = (torch.rand(2, 589, generator=g) < 0.7).float()
    with torch.inference_mode():
        got = ours(fbank.clone(), weights=weights).numpy()
        got_u = ours(fbank.clone()).numpy()
    want, want_u = ref[f"resnet_{name}_weighted"], ref[f"resnet_{name}_unweighted"]
    assert want.shape == (2, 256) and np.array_equal(got, want)
    assert np.array_equal(got_u, want_u)


def test_stats_pool(ref):
    """models/blocks/pooling.py:30-130: unweighted, (B,T) weights, (B,S,T) weights, weights on another
    time grid (nearest interpolation), all-zero weights."""
    import oracle.models as om
    ours = om.StatsPool()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 40, 125, generator=g)
    cases = [None,
             torch.rand(3, 125, generator=g),
             (torch.rand(3, 589, generator=g) < 0.6).float(),
             torch.rand(3, 3, 589, generator=g),
             torch.zeros(3, 589)]
    for i, w in enumerate(cases):
        want = ref[f"stats_pool_{i}"]
        got = ours(x, weights=w).numpy()
        assert got.shape == want.shape and np.array_equal(got, want)
    f = torch.randn(2, 256, 10, 38, generator=g)
    w = (torch.rand(2, 589, generator=g) < 0.5).float()
    assert np.array_equal(om.TSTP()(f, weights=w).numpy(), ref["tstp"])
    assert ref["tstp_out_dim"] == 5120


@pytest.mark.parametrize("num_classes,max_set_size", [(3, 2), (4, 2), (3, 3), (2, 1)])
def test_powerset(ref, num_classes, max_set_size):
    """utils/powerset.py:37-140: mapping, hard and soft `to_multilabel`, `to_powerset`."""
    import oracle.models as om
    key = f"powerset_{num_classes}_{max_set_size}"
    ours = om.Powerset(num_classes, max_set_size)
    assert ours.num_powerset_classes == ref[key + "_classes"]
    assert np.array_equal(ours.mapping.numpy(), ref[key + "_mapping"])
    g = torch.Generator().manual_seed(1)
    logp = torch.log_softmax(torch.randn(4, 57, ours.num_powerset_classes, generator=g), dim=-1)
    assert np.array_equal(ours.to_multilabel(logp).numpy(), ref[key + "_hard"])
    assert np.array_equal(ours.to_multilabel(logp, soft=True).numpy(), ref[key + "_soft"])
    assert np.array_equal(ours(logp).numpy(), ref[key + "_forward"])
    ml = torch.from_numpy(ref[key + "_hard"])
    assert np.array_equal(ours.to_powerset(ml).numpy(), ref[key + "_to_powerset"])


def test_powerset_product_lut(ref):
    """The product's hard conversion is an arg-max -> look-up table (k_classifier): the table must be
    the reference's mapping (utils/powerset.py:80-109) for the 3.1 model's (3, 2)."""
    from pyannote_audio_amd.weights import powerset_mapping
    want = ref["powerset_3_2_mapping"]
    assert np.array_equal(np.asarray(powerset_mapping(3, 2)), want)


def test_receptive_field(ref):
    """utils/receptive_field.py:26-165 with SincNet's kernels / strides (models/blocks/sincnet.py:82-161):
    oracle.pipeline.receptive_field and the product's frame geometry."""
    import oracle.models as om
    from oracle.pipeline import receptive_field
    ks, ss, ps, ds = [251, 3, 5, 3, 5, 3], [10, 3, 1, 3, 1, 3], [0] * 6, [1] * 6
    size, step, center = (int(v) for v in ref["rf_sincnet"])
    assert (size, step, center) == (991, 270, 495)
    sw = receptive_field(om.seeded_pyannet(num_layers=1), 16000)
    assert sw.duration == size / 16000 and sw.step == step / 16000
    assert sw.start == (center - (size - 1) / 2) / 16000
    import pyannote_audio_amd.model as pm
    from pyannote_audio_amd.segmentation import num_frames
    for n, want in zip((160000, 80000, 48000, 16000, 991, 1261, 123457), ref["rf_sincnet_num_frames"]):
        assert num_frames(n) == want == pm.multi_conv_num_frames(n, ks, ss, ps, ds)
    assert pm.multi_conv_receptive_field_size(1, ks, ss, ps, ds) == size
    assert pm.multi_conv_receptive_field_size(2, ks, ss, ps, ds) - size == step
    assert pm.multi_conv_receptive_field_center(0, ks, ss, ps, ds) == center
    # padded / strided 2-D chains of the ResNets (wespeaker/__init__.py:160-322)
    ks2, ss2, ps2 = [3, 3, 3, 3, 1, 3], [1, 1, 1, 2, 1, 2], [1, 1, 1, 1, 0, 1]
    for f, (center2, size2) in zip((0, 1, 7), ref["rf_resnet"]):
        assert pm.multi_conv_receptive_field_center(f, ks2, ss2, ps2, [1] * 6) == center2
        assert pm.multi_conv_receptive_field_size(f + 1, ks2, ss2, ps2, [1] * 6) == size2
    # the WeSpeaker wrappers' geometry (wespeaker/__init__.py:160-230): fbank window 400 / hop 160
    assert list(ref["rf_fbank_num_frames"]) == [298, 998]


def test_vbx_setup_and_cluster_vbx(ref, tmp_path):
    """utils/vbx.py:27-157 (VBx, cluster_vbx) and :160-218 (vbx_setup): the oracle's PLDA front end,
    responsibilities, priors and ELBO trace equal the reference's bit for bit."""
    import oracle.vbx as ov
    d = ov.synth_plda(str(tmp_path), seed=9)
    plda = ov.PLDA(os.path.join(d, "xvec_transform.npz"), os.path.join(d, "plda.npz"))
    rng = np.random.default_rng(4)
    centres = rng.standard_normal((4, 256))
    labels = rng.integers(0, 4, 300)
    emb = (centres[labels] + 0.3 * rng.standard_normal((300, 256))).astype(np.float32)
    got_fea = plda(emb)
    assert digest(got_fea) == ref["vbx_fea"]
    assert np.array_equal(plda.phi, ref["vbx_phi"])
    init = (labels + rng.integers(0, 2, 300)) % 5        # a deliberately imperfect 5-cluster start
    for i, (Fa, Fb) in enumerate([(0.07, 0.8), (0.3, 2.0)]):
        gq, gpi, gL = ov.cluster_vbx(init, got_fea, plda.phi, Fa=Fa, Fb=Fb, maxIters=20)
        assert np.array_equal(gq, ref[f"vbx_q_{i}"]) and np.array_equal(gpi, ref[f"vbx_pi_{i}"])
        # the ELBO trace (and with it the stopping iteration) from VBx itself, utils/vbx.py:27-140
        wL = ref[f"vbx_elbo_{i}"]
        assert np.array_equal(np.asarray(gL), wL) and 2 <= len(gL) <= 20
