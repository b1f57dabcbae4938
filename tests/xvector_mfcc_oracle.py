"""Torch-CPU restatement of torchaudio.transforms.MFCC (torchaudio is not installed; its documented behaviour, pinned
by tests/test_xvector_mfcc_cpu.py against HuggingFace `transformers.audio_utils`) and an XVectorMFCC oracle module
(models/embedding/xvector.py:42-202) built on it.  TEST INFRASTRUCTURE ONLY.

`MFCC(sample_rate, n_mfcc, dct_type, norm, log_mels, melkwargs, dtype)` takes torchaudio's arguments (so that it can
stand in for `torchaudio.transforms.MFCC` under tests/refharness.py) and computes in `dtype` (float32 = what the
reference computes, float64 = the precision yardstick).  Its buffers carry torchaudio's state-dict names:
`dct_mat`, `MelSpectrogram.spectrogram.window`, `MelSpectrogram.mel_scale.fb`."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

import oracle.models as om

MFCC_DEFAULTS = {"n_mfcc": 40, "dct_type": 2, "norm": "ortho", "log_mels": False}


def hz_to_mel(freq: float, mel_scale: str = "htk") -> float:
    if mel_scale == "htk":
        return 2595.0 * math.log10(1.0 + freq / 700.0)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return min_log_mel + math.log(freq / min_log_hz) / logstep if freq >= min_log_hz else freq / f_sp


def mel_to_hz(mels: torch.Tensor, mel_scale: str = "htk") -> torch.Tensor:
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (mels / 2595.0) - 1.0)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    freqs = f_sp * mels
    log_t = mels >= min_log_mel
    freqs[log_t] = min_log_hz * torch.exp(logstep * (mels[log_t] - min_log_mel))
    return freqs


def melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate, norm=None, mel_scale="htk",
                    dtype=torch.float32) -> torch.Tensor:
    """(n_freqs, n_mels) triangular filters between mel-spaced points (torchaudio.functional.melscale_fbanks)"""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=dtype)
    m_pts = torch.linspace(hz_to_mel(f_min, mel_scale), hz_to_mel(f_max, mel_scale), n_mels + 2, dtype=dtype)
    f_pts = mel_to_hz(m_pts, mel_scale)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = torch.max(torch.zeros(1, dtype=dtype), torch.min(down, up))
    if norm == "slaney":
        fb *= (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels])).unsqueeze(0)
    return fb


def create_dct(n_mfcc, n_mels, norm, dtype=torch.float32) -> torch.Tensor:
    """(n_mels, n_mfcc) DCT-II matrix (torchaudio.functional.create_dct)"""
    n = torch.arange(float(n_mels), dtype=dtype)
    k = torch.arange(float(n_mfcc), dtype=dtype).unsqueeze(1)
    dct = torch.cos(math.pi / float(n_mels) * (n + 0.5) * k)
    if norm is None:
        dct *= 2.0
    else:
        assert norm == "ortho"
        dct[0] *= 1.0 / math.sqrt(2.0)
        dct *= math.sqrt(2.0 / float(n_mels))
    return dct.t()


class _Spectrogram(nn.Module):
    def __init__(self, n_fft, win_length, hop_length, pad, power, normalized, center, pad_mode, dtype):
        super().__init__()
        self.n_fft, self.win_length, self.hop_length = n_fft, win_length, hop_length
        self.pad, self.power, self.normalized, self.center, self.pad_mode = pad, power, normalized, center, pad_mode
        self.register_buffer("window", torch.hann_window(win_length, dtype=dtype))

    def forward(self, x):
        shape = x.shape
        x = x.reshape(-1, shape[-1])
        spec = torch.stft(x, n_fft=self.n_fft, hop_length=self.hop_length, win_length=self.win_length,
                          window=self.window, center=self.center, pad_mode=self.pad_mode, normalized=False,
                          onesided=True, return_complex=True)
        spec = spec.abs().pow(self.power)
        return spec.reshape(shape[:-1] + spec.shape[-2:])


class _MelScale(nn.Module):
    def __init__(self, n_mels, sample_rate, f_min, f_max, n_stft, norm, mel_scale, dtype):
        super().__init__()
        self.register_buffer("fb", melscale_fbanks(n_stft, f_min, f_max, n_mels, sample_rate, norm, mel_scale,
                                                   dtype))

    def forward(self, spec):
        return torch.matmul(spec.transpose(-1, -2), self.fb).transpose(-1, -2)


class _MelSpectrogram(nn.Module):
    def __init__(self, sample_rate=16000, n_fft=400, win_length=None, hop_length=None, f_min=0.0, f_max=None, pad=0,
                 n_mels=128, window_fn=None, power=2.0, normalized=False, wkwargs=None, center=True,
                 pad_mode="reflect", onesided=None, norm=None, mel_scale="htk", dtype=torch.float32):
        super().__init__()
        win_length = win_length if win_length is not None else n_fft
        hop_length = hop_length if hop_length is not None else win_length // 2
        f_max = f_max if f_max is not None else float(sample_rate // 2)
        self.n_mels = n_mels
        self.spectrogram = _Spectrogram(n_fft, win_length, hop_length, pad, power, normalized, center, pad_mode,
                                        dtype)
        self.mel_scale = _MelScale(n_mels, sample_rate, f_min, f_max, n_fft // 2 + 1, norm, mel_scale, dtype)

    def forward(self, x):
        return self.mel_scale(self.spectrogram(x))


def amplitude_to_db(x: torch.Tensor, top_db: float = 80.0) -> torch.Tensor:
    """AmplitudeToDB("power", top_db=80): 10 log10(max(x, 1e-10)), clamped at the max over (channel, mel, time) of
    each batch item minus top_db"""
    x_db = 10.0 * torch.log10(torch.clamp(x, min=1e-10))
    shape = x_db.size()
    packed = shape[-3] if x_db.dim() > 2 else 1
    x_db = x_db.reshape(-1, packed, shape[-2], shape[-1])
    x_db = torch.max(x_db, (x_db.amax(dim=(-3, -2, -1)) - top_db).view(-1, 1, 1, 1))
    return x_db.reshape(shape)


class MFCC(nn.Module):
    """torchaudio.transforms.MFCC(sample_rate, n_mfcc, dct_type, norm, log_mels, melkwargs), in `dtype`"""

    def __init__(self, sample_rate=16000, n_mfcc=40, dct_type=2, norm="ortho", log_mels=False, melkwargs=None,
                 dtype=torch.float32):
        super().__init__()
        assert dct_type == 2
        self.n_mfcc, self.log_mels, self.top_db = n_mfcc, log_mels, 80.0
        self.MelSpectrogram = _MelSpectrogram(sample_rate=sample_rate, dtype=dtype, **(melkwargs or {}))
        if n_mfcc > self.MelSpectrogram.n_mels:
            raise ValueError("Cannot select more MFCC coefficients than # mel bins")
        self.register_buffer("dct_mat", create_dct(n_mfcc, self.MelSpectrogram.n_mels, norm, dtype))

    def forward(self, waveform):
        mel = self.MelSpectrogram(waveform)
        mel = torch.log(mel + 1e-6) if self.log_mels else amplitude_to_db(mel, self.top_db)
        return torch.matmul(mel.transpose(-1, -2), self.dct_mat).transpose(-1, -2)


class XVectorMFCC(nn.Module):
    """MFCC -> 5 x (Conv1d + LeakyReLU + BatchNorm1d) -> StatsPool -> Linear (models/embedding/xvector.py:42-202;
    pinned to that class by tests/test_xvector_mfcc_cpu.py with this MFCC on both sides)"""

    def __init__(self, sample_rate: int = 16000, mfcc: dict | None = None, dimension: int = 512,
                 dtype=torch.float32):
        super().__init__()
        cfg = dict(MFCC_DEFAULTS, **(mfcc or {}))
        cfg["sample_rate"] = sample_rate
        self.hparams_mfcc = cfg
        self.mfcc = MFCC(**cfg, dtype=dtype)
        self.tdnns = nn.ModuleList()
        in_channel = cfg["n_mfcc"]
        for out_channel, kernel_size, dilation in zip([512, 512, 512, 512, 1500], [5, 3, 3, 1, 1], [1, 2, 3, 1, 1]):
            self.tdnns.extend([nn.Conv1d(in_channel, out_channel, kernel_size, dilation=dilation),
                               nn.LeakyReLU(), nn.BatchNorm1d(out_channel)])
            in_channel = out_channel
        self.stats_pool = om.StatsPool()
        self.embedding = nn.Linear(in_channel * 2, dimension)
        self.to(dtype)

    def forward(self, waveforms, weights=None):
        outputs = self.mfcc(waveforms).squeeze(dim=1)
        for tdnn in self.tdnns:
            outputs = tdnn(outputs)
        return self.embedding(self.stats_pool(outputs, weights=weights))


def seeded_xvector_mfcc(seed: int = 3579, mfcc: dict | None = None, dimension: int = 512,
                        dtype=torch.float32) -> XVectorMFCC:
    """Default-initialised XVectorMFCC with randomised BatchNorm statistics / affine (as oracle.seeded_xvector); the
    first convolution is scaled down so that its input, MFCCs of some hundreds, gives activations of order one"""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    model = XVectorMFCC(mfcc=mfcc, dimension=dimension)
    with torch.no_grad():
        model.tdnns[0].weight.mul_(0.02)
        for m in model.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
                m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
    return model.to(dtype).eval()


def as_float64(model: XVectorMFCC) -> XVectorMFCC:
    """the same weights in float64, its MFCC buffers rebuilt in float64 from the closed forms"""
    ref = XVectorMFCC(mfcc={k: v for k, v in model.hparams_mfcc.items() if k != "sample_rate"},
                      sample_rate=model.hparams_mfcc["sample_rate"], dimension=model.embedding.out_features,
                      dtype=torch.float64)
    sd = {k: v.double() for k, v in model.state_dict().items() if not k.startswith("mfcc.")}
    missing, unexpected = ref.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("mfcc.") for k in missing)
    return ref.eval()


def xvector_mfcc_hparams(model: XVectorMFCC) -> dict:
    """the hyper-parameters the reference's XVectorMFCC saves (save_hyperparameters("mfcc", "dimension") + Model's
    sample_rate / num_channels)"""
    return {"sample_rate": model.hparams_mfcc["sample_rate"], "num_channels": 1, "mfcc": dict(model.hparams_mfcc),
            "dimension": model.embedding.out_features}
