"""Case tables, input generators and float64 truths of the wav2vec 2.0 / WavLM encoder kernels (csrc/w2v.hip: pa_w2v_conv0,
pa_w2v_group_norm_gelu, pa_w2v_layernorm, pa_w2v_posconv, pa_w2v_softmax, pa_w2v_axpy, pa_w2v_to_tiles), shared by
tests/test_w2v_kernels_gpu.py (the kernels, on an MI355X) and tests/test_w2v_truth_cpu.py (admissibility of every case and
the truths pinned to oracle.wav2vec2, without a GPU).  Pure torch on the CPU; nothing here touches the library.

Every operation is written once, as a function of a dtype: evaluated in float64 it is the truth, in float32 it is "float32
torch doing the same operation" (tests/kernel_parity.py).  Inputs are float32 tensors -- exactly what the kernel is given --
and are widened, never regenerated, for the truth.  The functions take the VALID rows only (x[:, :T]); what the padding
rows T .. P - 1 and the padding columns T .. Tp - 1 hold is the business of the GPU test, which fills them with NaN.

Kept out (and why): inputs with a heavy offset against their spread.  Float32 rounding of the input alone takes float32
torch past half the contract there, so such a case says nothing about a kernel:
    layer norm, mean 20 / std 0.05, C = 512     float32 torch at 4.6 of the contract
    layer norm, mean 5 / std 0.1, C = 1024                       0.66
    group norm, channel mean 10 / std 0.02                       3.7
The strongest offset kept is group norm at channel mean 3 / std 0.1 (0.36 with the inputs generated here).  Group norm over T = 1 row is kept out of the
admissible list as well (torch's float32 group norm was measured at 1.07 of the contract there): its truth is
gelu(beta[c]) exactly, and the GPU test holds the kernel to that closed form."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-5
NAN = float("nan")


def gelu(x):
    """exact (erf) GELU in the dtype of x"""
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def chunks_of(wav, wav_len, chunk_stride, B, N):
    """(B, N): chunk b = wav[b chunk_stride : b chunk_stride + N], zeros from wav_len on"""
    idx = torch.arange(B).view(-1, 1) * chunk_stride + torch.arange(N).view(1, -1)
    return torch.where(idx < wav_len, wav[idx.clamp(max=max(wav_len - 1, 0))], torch.zeros((), dtype=wav.dtype))


def pad_rows(x, P, value=NAN):
    """(B, T, C) -> (B, P, C) with rows T .. P - 1 set to `value`"""
    B, T, C = x.shape
    out = torch.full((B, P, C), value, dtype=x.dtype)
    out[:, :T] = x
    return out


# ---------------------------------------------------------------------------------------------------------------------
# pa_w2v_conv0
# ---------------------------------------------------------------------------------------------------------------------
def _c0(C, K0, S0, N, B, step=None, cut=0):
    step = N if step is None else step
    return dict(name=f"C{C}_K{K0}_S{S0}_N{N}_B{B}_step{step}" + (f"_cut{cut}" if cut else ""), C=C, K0=K0, S0=S0, N=N,
                B=B, step=step, T=(N - K0) // S0 + 1, end=(B - 1) * step + N, wav_len=(B - 1) * step + N - cut)


CONV0_CASES = [
    _c0(64, 10, 5, 1600, 3, 400),                 # T = 319: ten blocks of 32 rows, the last one partly
    _c0(512, 10, 5, 3200, 2, 3200, cut=700),      # two trips of the channel loop; the last chunk runs off the waveform
    _c0(32, 16, 16, 800, 2, 100),                 # the largest kernel and stride, T = 50
    _c0(96, 1, 1, 70, 1),
    _c0(64, 3, 2, 100, 5, 37),
    _c0(64, 2, 5, 163, 2, 50),                    # K0 < S0: samples between the windows are never read
    _c0(32, 10, 5, 100, 2, 60),                   # T = 19 < 32: one block, partly filled
]
#: P - T of the two runs of every case
CONV0_PADS = (0, 9)


def conv0_input(case, seed):
    """wav (wav_len,), weight (C, K0), bias (C)"""
    g = torch.Generator().manual_seed(seed)
    wav = 0.1 * torch.randn(case["wav_len"], generator=g) + 0.05 * torch.sin(torch.arange(case["wav_len"]) * 0.05)
    w = torch.randn(case["C"], case["K0"], generator=g) / math.sqrt(case["K0"])
    bias = 0.05 * torch.randn(case["C"], generator=g)
    return wav.float(), w, bias


def conv0(wav, case, w, bias, dtype):
    """conv1d of each zero-extended chunk, channels last -> (B, T, C); bias may be None"""
    c = chunks_of(wav, case["wav_len"], case["step"], case["B"], case["N"]).to(dtype)
    y = F.conv1d(c[:, None], w.to(dtype)[:, None], None if bias is None else bias.to(dtype), stride=case["S0"])
    assert y.shape[-1] == case["T"]
    return y.transpose(1, 2).contiguous()


def conv0_exact_weights(case):
    """channel c has its single tap (value 1) at j = c % K0: every tap is some channel's"""
    tap = torch.arange(case["C"]) % case["K0"]
    w = torch.zeros(case["C"], case["K0"])
    w[torch.arange(case["C"]), tap] = 1.0
    return w, tap


def conv0_exact(wav, case, tap):
    """out[b][t][c] = wav[b step + t S0 + tap_c] (zero behind wav_len), exactly"""
    c = chunks_of(wav, case["wav_len"], case["step"], case["B"], case["N"])
    pos = torch.arange(case["T"]).view(-1, 1) * case["S0"] + tap.view(1, -1)               # (T, C)
    return c[:, pos]


# ---------------------------------------------------------------------------------------------------------------------
# pa_w2v_group_norm_gelu
# ---------------------------------------------------------------------------------------------------------------------
def _gn(B, T, P, C, mean=0.0, std=0.1):
    return dict(name=f"B{B}_T{T}_P{P}_C{C}" + (f"_mean{mean:g}_std{std:g}" if mean else ""), B=B, T=T, P=P, C=C,
                mean=mean, std=std)


GN_CASES = [
    _gn(2, 499, 499, 64),
    _gn(3, 49, 64, 96),            # half of the second 64-channel block idle
    _gn(1, 5, 8, 32),              # half a block idle; row lane 0 has two rows, the others one
    _gn(2, 3, 4, 64),              # T < 4: a row lane without rows
    _gn(2, 130, 130, 512),
    _gn(2, 49, 52, 64, mean=3.0, std=0.1),
]
#: inadmissible by the rule (see the module docstring), held to gelu(beta) by the GPU test
GN_ONE_ROW = _gn(1, 1, 4, 64)


def gn_input(case, seed):
    """x (B, T, C) valid rows: per (chunk, channel) offsets of the size of case["mean"] against a spread of exactly
    case["std"] (or offsets of the size of the spread, which then varies by a factor of 3 between channels), gamma of both
    signs, beta"""
    g = torch.Generator().manual_seed(seed)
    B, T, C = case["B"], case["T"], case["C"]
    centre = case["mean"] * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)[None, None] if case["mean"] else \
        case["std"] * torch.randn(B, 1, C, generator=g)
    spread = case["std"] * (torch.ones(B, 1, C) if case["mean"] else 0.5 + torch.rand(B, 1, C, generator=g))
    x = centre + spread * torch.randn(B, T, C, generator=g)
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    beta = 0.3 * torch.randn(C, generator=g)
    return x.float(), gamma.float(), beta.float()


def group_norm_gelu(x, gamma, beta, dtype):
    """x (B, T, C) -> y (B, T, C), mean (B, C), rstd (B, C): statistics over the T rows (biased variance)"""
    x = x.to(dtype)
    T = x.shape[1]
    mean = x.sum(1) / T
    d = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((d * d).sum(1) / T + EPS)
    y = d * (rstd * gamma.to(dtype)[None])[:, None] + beta.to(dtype)[None, None]
    return gelu(y), mean, rstd


# ---------------------------------------------------------------------------------------------------------------------
# pa_w2v_layernorm
# ---------------------------------------------------------------------------------------------------------------------
LN_CHANNELS = (32, 96, 512, 768, 1000, 1024)
LN_ROWS = (1, 3, 4, 5, 37)
LN_CASES = [dict(name=f"C{C}_rows{rows}", C=C, rows=rows) for C in LN_CHANNELS for rows in LN_ROWS]


def ln_input(case, seed):
    """x (rows, C) with a per-row offset of the size of the spread, gamma of both signs, beta"""
    g = torch.Generator().manual_seed(seed)
    rows, C = case["rows"], case["C"]
    x = torch.randn(rows, 1, generator=g) + (0.5 + torch.rand(rows, 1, generator=g)) * torch.randn(rows, C, generator=g)
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    beta = 0.3 * torch.randn(C, generator=g)
    return x.float(), gamma.float(), beta.float()


def layer_norm(x, gamma, beta, with_gelu, dtype):
    x = x.to(dtype)
    C = x.shape[-1]
    d = x - x.sum(-1, keepdim=True) / C
    y = d / torch.sqrt((d * d).sum(-1, keepdim=True) / C + EPS) * gamma.to(dtype) + beta.to(dtype)
    return gelu(y) if with_gelu else y


# ---------------------------------------------------------------------------------------------------------------------
# pa_w2v_posconv
# ---------------------------------------------------------------------------------------------------------------------
def _pc(D, groups, KW, T, P, B):
    return dict(name=f"D{D}_g{groups}_k{KW}_T{T}_P{P}_B{B}", D=D, groups=groups, KW=KW, T=T, P=P, B=B, CG=D // groups)


POSCONV_CASES = [
    _pc(128, 4, 32, 49, 52, 3),
    _pc(768, 16, 128, 40, 40, 2),        # WavLM's CG = 48 and kernel; P == T: the next chunk's rows follow at once
    _pc(96, 3, 5, 17, 20, 2),            # odd kernel: no frame is dropped
    _pc(64, 2, 1, 16, 16, 1),
    _pc(64, 2, 32, 7, 9, 2),             # T < pad
    _pc(64, 1, 4, 1, 3, 2),
    _pc(128, 4, 32, 33, 33, 1),          # rows 16 | 17 and 32 | 33 are tile edges
]


def posconv_input(case, seed):
    """x (B, T, D) valid rows, weight (D, CG, KW) in the reference layout scaled by 1 / sqrt(CG KW), bias (D)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(case["B"], case["T"], case["D"], generator=g)
    w = torch.randn(case["D"], case["CG"], case["KW"], generator=g) / math.sqrt(case["CG"] * case["KW"])
    bias = 0.2 * torch.randn(case["D"], generator=g)
    return x.float(), w.float(), bias.float()


def repack_pos_weight(w, groups):
    """(D, CG, KW) -> [g][j][ci][co], the operand of pa_w2v_posconv"""
    D, CG, KW = w.shape
    return w.reshape(groups, CG, CG, KW).permute(0, 3, 2, 1).contiguous()


def posconv(x, w, bias, groups, dtype):
    """x (B, T, D) -> x + gelu(grouped conv1d(x, padding KW // 2) + bias), the last frame of an even kernel dropped"""
    KW = w.shape[-1]
    x = x.to(dtype)
    y = F.conv1d(x.transpose(1, 2), w.to(dtype), bias.to(dtype), padding=KW // 2, groups=groups)
    if KW % 2 == 0:
        y = y[..., :-1]
    return x + gelu(y).transpose(1, 2)


def posconv_single_weight(x, case, g, j, ci, co, value, dtype):
    """the one weight `value` at (g, j, ci, co), no bias: x + gelu(value x[t + j - pad, g CG + ci]) in channel g CG + co,
    x everywhere else"""
    x = x.to(dtype)
    B, T, D = x.shape
    CG, pad = case["CG"], case["KW"] // 2
    src = torch.zeros(B, T, dtype=dtype)
    t = torch.arange(T) + j - pad
    ok = (t >= 0) & (t < T)
    src[:, ok] = x[:, t[ok], g * CG + ci]
    out = x.clone()
    out[:, :, g * CG + co] += gelu(torch.tensor(value, dtype=torch.float32).to(dtype) * src)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# pa_w2v_softmax
# ---------------------------------------------------------------------------------------------------------------------
def _sm(B, H, T, Tp, hd, variant=None):
    return dict(name=f"B{B}_H{H}_T{T}_Tp{Tp}_hd{hd}" + (f"_{variant}" if variant else ""), B=B, H=H, T=T, Tp=Tp, hd=hd,
                D=H * hd, P=T + 3, variant=variant)


SOFTMAX_CASES = [
    _sm(2, 4, 49, 64, 32, "row_plus80"),     # +80 on one whole row of every (b, h): the maximum is taken off first
    _sm(1, 12, 499, 512, 64),
    _sm(2, 2, 70, 96, 128),                  # hd > 64: the second half of the gate's dot product, all 64 lanes of it
    _sm(2, 3, 65, 96, 96, "spike60"),        # ... and half of the lanes; one score 60 above the rest of its row
    _sm(3, 2, 1, 32, 32),
    _sm(1, 2, 63, 64, 64),
    _sm(1, 2, 64, 64, 64),
    _sm(1, 3, 33, 45, 32),                   # Tp no multiple of 32, 99 rows: the last block of four has three
]


def softmax_input(case, seed):
    """S (B, H, T, T) raw scores whose scaled standard deviation is 2, scale, bias (H, T, T), xin (B, T, D) valid rows,
    gate_w (8, hd), gate_b (8), gate_const (H) -- a different one per head"""
    g = torch.Generator().manual_seed(seed)
    B, H, T, hd, D = case["B"], case["H"], case["T"], case["hd"], case["D"]
    scale = hd ** -0.5
    S = (2.0 / scale) * torch.randn(B, H, T, T, generator=g)
    if case["variant"] == "row_plus80":
        S[:, :, T // 3] += 80.0 / scale
    elif case["variant"] == "spike60":
        t, k = T // 2, T - 1
        S[:, :, t, k] = S[:, :, t].amax(-1) + 60.0 / scale
    bias = torch.randn(H, T, T, generator=g)
    xin = torch.randn(B, T, D, generator=g)
    gate_w = torch.randn(8, hd, generator=g) / math.sqrt(hd)
    gate_b = 0.3 * torch.randn(8, generator=g)
    gate_const = 1.0 + 0.15 * torch.arange(H) + 0.05 * torch.randn(H, generator=g)
    return S.float(), scale, bias.float(), xin.float(), gate_w.float(), gate_b.float(), gate_const.float()


def wavlm_gate(xin, H, gate_w, gate_b, gate_const, dtype):
    """(B, H, T): from head slice h of row (b, t), u = gate_w q + gate_b (8 values); ga = sigmoid(u0 + u1 + u2 + u3),
    gb = sigmoid(u4 + u5 + u6 + u7); gate = ga (gb const[h] - 1) + 2"""
    B, T, D = xin.shape
    q = xin.to(dtype).reshape(B, T, H, D // H).permute(0, 2, 1, 3)                       # (B, H, T, hd)
    u = q @ gate_w.to(dtype).t() + gate_b.to(dtype)                                     # (B, H, T, 8)
    ga = torch.sigmoid(u[..., 0] + u[..., 1] + u[..., 2] + u[..., 3])
    gb = torch.sigmoid(u[..., 4] + u[..., 5] + u[..., 6] + u[..., 7])
    return ga * (gb * gate_const.to(dtype).view(1, H, 1) - 1.0) + 2.0


def attention_softmax(S, scale, dtype, bias=None, xin=None, gate_w=None, gate_b=None, gate_const=None):
    """softmax over the last axis of S scale (+ gate[b, h, t] bias[h, t, :]) -> (B, H, T, T)"""
    z = S.to(dtype) * torch.tensor(scale, dtype=torch.float32).to(dtype)
    if bias is not None:
        gate = wavlm_gate(xin, S.shape[1], gate_w, gate_b, gate_const, dtype)
        z = z + gate[..., None] * bias.to(dtype)[None]
    z = z - z.amax(-1, keepdim=True)
    e = torch.exp(z)
    return e / e.sum(-1, keepdim=True)


# ---------------------------------------------------------------------------------------------------------------------
# pa_w2v_axpy, pa_w2v_to_tiles
# ---------------------------------------------------------------------------------------------------------------------
AXPY_SIZES = (4, 1020, 1024, 1028, 4096 + 4)


def axpy(acc, x, w, first, dtype):
    wx = torch.tensor(w, dtype=torch.float32).to(dtype) * x.to(dtype)
    return wx if first else acc.to(dtype) + wx


TILES_CASES = [dict(name=f"B{B}_T{T}_P{P}_D{D}", B=B, T=T, P=P, D=D)
               for B, T, P, D in ((1, 1, 1, 32), (16, 7, 9, 96), (17, 7, 7, 300), (19, 3, 5, 64))]


def to_tiles(x):
    """x (B, T, D) valid rows -> (ntiles, T, 16, D): chunk b at [b // 16, :, b % 16]; the chunks from B on are zero"""
    B, T, D = x.shape
    ntiles = (B + 15) // 16
    out = torch.zeros(ntiles, T, 16, D, dtype=x.dtype)
    for b in range(B):
        out[b // 16, :, b % 16] = x[b]
    return out
