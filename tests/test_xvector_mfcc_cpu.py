"""XVectorMFCC on the host (models/embedding/xvector.py:42-202): the MFCC restatement of tests/xvector_mfcc_oracle.py
pinned by HuggingFace `transformers.audio_utils` (torchaudio is absent), the reference's own XVectorMFCC executed on
that restatement against the oracle module and the product's frame geometry, the hyper-parameter validator, and the
checkpoint round trip.  No GPU."""
import math
import sys

import numpy as np
import pytest
import torch

import xvector_mfcc_oracle as xo

pytestmark = pytest.mark.filterwarnings("ignore::UserWarning")


def _signal(seed: int, n: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(n, generator=g, dtype=torch.float64)).clamp(-1, 1)


def test_filter_bank_pinned_by_transformers():
    audio_utils = pytest.importorskip("transformers.audio_utils")
    for n_mels, f_min, f_max in ((128, 0.0, 8000.0), (40, 20.0, 7600.0), (256, 0.0, 8000.0)):
        theirs = audio_utils.mel_filter_bank(201, n_mels, f_min, f_max, 16000, norm=None, mel_scale="htk")
        exact = xo.melscale_fbanks(201, f_min, f_max, n_mels, 16000, dtype=torch.float64).numpy()
        assert exact.shape == theirs.shape == (201, n_mels)
        assert np.abs(exact - theirs).max() <= 1e-9
        if n_mels == 128:     # the stock configuration, in float32 as torchaudio builds it
            assert np.abs(xo.melscale_fbanks(201, f_min, f_max, n_mels, 16000).numpy() - theirs).max() <= 2e-5
    # with the defaults, 4 of the 128 filters are all zero (no FFT bin between their edges)
    fb = xo.melscale_fbanks(201, 0.0, 8000.0, 128, 16000)
    assert int((fb.abs().sum(dim=0) == 0).sum()) == 4
    # the product's closed form (used when a checkpoint lacks the buffer) is the oracle's, bit for bit
    from pyannote_audio_amd.weights import create_dct, melscale_fbanks
    assert torch.equal(melscale_fbanks(201, 0.0, 8000.0, 128, 16000), fb)
    assert torch.equal(melscale_fbanks(201, 20.0, 7000.0, 64, 16000, "slaney", "slaney"),
                       xo.melscale_fbanks(201, 20.0, 7000.0, 64, 16000, "slaney", "slaney"))
    assert torch.equal(create_dct(40, 128, "ortho"), xo.create_dct(40, 128, "ortho"))
    assert torch.equal(create_dct(24, 80, None), xo.create_dct(24, 80, None))


@pytest.mark.parametrize("center,hop", [(True, 200), (False, 160)])
def test_power_spectrogram_and_db_pinned_by_transformers(center, hop):
    audio_utils = pytest.importorskip("transformers.audio_utils")
    x = _signal(1, 16000 * 3 + 77)
    spec = xo._Spectrogram(400, 400, hop, 0, 2.0, False, center, "reflect", torch.float64)(x)
    window = audio_utils.window_function(400, "hann", periodic=True)
    assert np.abs(window - torch.hann_window(400, dtype=torch.float64).numpy()).max() < 1e-15
    theirs = audio_utils.spectrogram(x.numpy(), window, frame_length=400, hop_length=hop, power=2.0, center=center,
                                     pad_mode="reflect", dtype=np.float64)
    assert theirs.shape == tuple(spec.shape)
    assert np.abs(spec.numpy() - theirs).max() <= 1e-6 * np.abs(theirs).max()
    fb = xo.melscale_fbanks(201, 0.0, 8000.0, 128, 16000, dtype=torch.float64)
    mel = torch.matmul(spec.t(), fb).t()                       # (n_mels, frames) of one chunk
    ours = xo.amplitude_to_db(mel.view(1, 1, *mel.shape)).view(mel.shape)
    want = audio_utils.power_to_db(mel.numpy(), reference=1.0, min_value=1e-10, db_range=80.0)
    assert np.abs(ours.numpy() - want).max() <= 1e-9
    # the clamp is taken per chunk: a second, louder chunk does not move the first one's floor
    both = torch.stack([mel, 1e4 * mel]).unsqueeze(1)
    assert torch.equal(xo.amplitude_to_db(both)[0, 0], ours)


@pytest.mark.parametrize("n_mfcc,n_mels", [(40, 128), (64, 64), (24, 80)])
def test_create_dct_ortho_is_orthonormal(n_mfcc, n_mels):
    d = xo.create_dct(n_mfcc, n_mels, "ortho", dtype=torch.float64)
    assert d.shape == (n_mels, n_mfcc)
    assert torch.allclose(d.t() @ d, torch.eye(n_mfcc, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(xo.create_dct(n_mfcc, n_mels, None, dtype=torch.float64)[:, 1:],
                          d[:, 1:] * math.sqrt(2.0 * n_mels), atol=1e-12)


# ------------------------------------------------------------------------------------------ the reference's class
@pytest.fixture(scope="module")
def reference_xvector():
    import refharness
    if not refharness.available():
        pytest.skip("the reference sources are not on this machine")
    with refharness.reference_modules(third_party=True) as r:
        r.load_core()
        sys.modules["torchaudio.transforms"].MFCC = xo.MFCC     # the restatement stands in for torchaudio's
        yield r.load("pyannote.audio.models.embedding.xvector")


@pytest.mark.parametrize("mfcc", [None, {"melkwargs": {"center": False, "hop_length": 160}},
                                  {"log_mels": True, "n_mfcc": 24}, {"n_mfcc": 64, "melkwargs": {"hop_length": 160}}])
def test_reference_xvector_mfcc_equals_oracle(reference_xvector, mfcc):
    """the reference's XVectorMFCC (with the restated MFCC) and the oracle module: same state-dict keys, identical
    embeddings with and without weights; its num_frames / receptive field equal the product's closed forms"""
    import pyannote_audio_amd.model as pm
    ours = xo.seeded_xvector_mfcc(mfcc=mfcc)
    theirs = reference_xvector.XVectorMFCC(mfcc=mfcc)
    assert list(theirs.state_dict()) == list(ours.state_dict())
    theirs.load_state_dict(ours.state_dict())
    theirs.eval()
    g = torch.Generator().manual_seed(2)
    wav = (0.1 * torch.randn(2, 1, 48000, generator=g)).clamp(-1, 1)
    weights = (torch.rand(2, 3, 173, generator=g) < 0.6).float()
    with torch.inference_mode():
        assert torch.equal(ours(wav, weights=weights), theirs(wav, weights=weights))
        assert torch.equal(ours(wav), theirs(wav))
    assert dict(theirs.hparams["mfcc"]) == ours.hparams_mfcc
    product = pm.XVectorMFCC(ours.state_dict(), xo.xvector_mfcc_hparams(ours), pm.embedding_specifications())
    assert product.dimension == theirs.dimension == 512
    for n in (2799, 2800, 3000, 4771, 16000, 48000, 80000, 160000, 160001):
        assert product.num_frames(n) == theirs.num_frames(n), n
    for f in (1, 2, 10):
        assert product.receptive_field_size(f) == theirs.receptive_field_size(f)
    for f in (0, 3):
        assert product.receptive_field_center(f) == theirs.receptive_field_center(f)


def test_geometry_at_16khz():
    import pyannote_audio_amd.model as pm
    ours = xo.seeded_xvector_mfcc()
    product = pm.XVectorMFCC(ours.state_dict(), xo.xvector_mfcc_hparams(ours), pm.embedding_specifications())
    assert product.num_frames(160000) == 787            # 801 MFCC frames
    assert product.receptive_field_size(1) == 400 + 14 * 200
    assert product.receptive_field_center(0) == 7 * 200


# ------------------------------------------------------------------------------------------ hyper-parameters
REFUSED = [
    ({"n_mfcc": 65}, "n_mfcc"), ({"n_mfcc": 0}, "n_mfcc"), ({"dct_type": 3}, "dct_type"), ({"norm": "forward"}, "norm"),
    ({"log_mels": "yes"}, "log_mels"), ({"top_db": 60}, "top_db"),
    ({"melkwargs": {"n_fft": 512}}, "n_fft"), ({"melkwargs": {"win_length": 320}}, "win_length"),
    ({"melkwargs": {"hop_length": 0}}, "hop_length"), ({"melkwargs": {"hop_length": 401}}, "hop_length"),
    ({"melkwargs": {"center": 1}}, "center"), ({"melkwargs": {"pad_mode": "constant"}}, "pad_mode"),
    ({"melkwargs": {"pad": 10}}, "pad"), ({"melkwargs": {"power": 1.0}}, "power"),
    ({"melkwargs": {"normalized": True}}, "normalized"), ({"melkwargs": {"onesided": False}}, "onesided"),
    ({"melkwargs": {"window_fn": torch.hamming_window}}, "window_fn"), ({"melkwargs": {"wkwargs": {"a": 1}}}, "wkwargs"),
    ({"melkwargs": {"n_mels": 257}}, "n_mels"), ({"melkwargs": {"n_mels": 32}}, "n_mfcc"),
    ({"melkwargs": {"mel_scale": "bark"}}, "mel_scale"), ({"melkwargs": {"norm": "l2"}}, "norm"),
    ({"melkwargs": {"sample_rate": 8000}}, "sample_rate"), ({"melkwargs": {"f_min": "low"}}, "f_min"),
]


@pytest.mark.parametrize("mfcc,key", REFUSED, ids=[k + str(i) for i, (_, k) in enumerate(REFUSED)])
def test_validator_refuses_what_the_front_end_is_not_built_for(mfcc, key):
    from pyannote_audio_amd.weights import mfcc_config
    with pytest.raises(NotImplementedError, match=key):
        mfcc_config({"sample_rate": 16000, "mfcc": mfcc})


ACCEPTED = [None, {"n_mfcc": 64}, {"n_mfcc": 1, "norm": None, "log_mels": True},
            {"melkwargs": {"n_fft": 400, "win_length": 400, "hop_length": 1, "center": False, "pad_mode": "reflect",
                           "pad": 0, "power": 2, "normalized": False, "onesided": True, "window_fn": torch.hann_window,
                           "n_mels": 256, "f_min": 20.0, "f_max": 7600, "mel_scale": "slaney", "norm": "slaney"}},
            {"melkwargs": {"hop_length": 400, "n_mels": 40}, "n_mfcc": 40}]


@pytest.mark.parametrize("mfcc", ACCEPTED)
def test_validator_accepts_the_built_configurations(mfcc):
    from pyannote_audio_amd.weights import mfcc_config
    cfg = mfcc_config({"sample_rate": 16000, "mfcc": mfcc})
    assert cfg["n_fft"] == 400 and 1 <= cfg["hop_length"] <= 400 and cfg["n_mfcc"] <= 64


def test_model_refuses_at_load_time_without_a_device(tmp_path):
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.model import embedding_specifications, save_checkpoint
    ours = xo.seeded_xvector_mfcc()
    hp = xo.xvector_mfcc_hparams(ours)
    hp["mfcc"] = dict(hp["mfcc"], melkwargs={"n_fft": 512})
    path = tmp_path / "odd.bin"
    save_checkpoint(path, ours.state_dict(), hp, pa.XVectorMFCC.ARCHITECTURE, embedding_specifications())
    with pytest.raises(NotImplementedError, match="n_fft = 512"):
        pa.Model.from_pretrained(path)


def test_checkpoint_round_trip(tmp_path):
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.model import embedding_specifications, load_checkpoint, save_checkpoint
    ours = xo.seeded_xvector_mfcc(mfcc={"log_mels": True, "melkwargs": {"hop_length": 160}})
    hp = xo.xvector_mfcc_hparams(ours)
    path = tmp_path / "pytorch_model.bin"
    save_checkpoint(path, ours.state_dict(), hp, pa.XVectorMFCC.ARCHITECTURE, embedding_specifications())
    model = pa.Model.from_pretrained(str(tmp_path))
    assert type(model) is pa.XVectorMFCC
    assert dict(model.hparams) == hp and model.specifications == embedding_specifications()
    assert model.mfcc["hop_length"] == 160 and model.mfcc["log_mels"] and model.dimension == 512
    assert all(torch.equal(model.state_dict()[k], v) for k, v in ours.state_dict().items())
    ckpt = load_checkpoint(path)
    assert ckpt["pyannote.audio"]["architecture"] == {"module": "pyannote.audio.models.embedding.xvector",
                                                      "class": "XVectorMFCC"}
    from pyannote_audio_amd.speaker_verification import first_true
    assert hasattr(model, "_TDNN")
    assert first_true(lambda n: model.num_frames(n) > 0, 2, 8000) == 14 * 160


def test_pack_buffers_come_from_the_checkpoint_or_the_closed_forms():
    """the front end reads the checkpoint's torchaudio buffers; a state dict without them gets the closed forms
    (float32, as torchaudio builds them) -- the same tables for the stock configuration"""
    from pyannote_audio_amd.weights import mfcc_buffers, mfcc_config
    ours = xo.seeded_xvector_mfcc()
    sd = ours.state_dict()
    cfg = mfcc_config(xo.xvector_mfcc_hparams(ours))
    a = mfcc_buffers(sd, cfg)
    b = mfcc_buffers({k: v for k, v in sd.items() if not k.startswith("mfcc.")}, cfg)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    odd = dict(sd)
    odd["mfcc.MelSpectrogram.mel_scale.fb"] = 2.0 * sd["mfcc.MelSpectrogram.mel_scale.fb"]
    assert torch.equal(mfcc_buffers(odd, cfg)[1], odd["mfcc.MelSpectrogram.mel_scale.fb"])
    with pytest.raises(ValueError, match="dct_mat"):
        mfcc_buffers(dict(sd, **{"mfcc.dct_mat": sd["mfcc.dct_mat"][:, :20]}), cfg)
