"""Case tables, input generators and float64 truths of the SincNet front-end kernels (csrc/seg_frontend.hip), shared by
tests/test_seg_frontend_gpu.py (the kernels, on an MI355X) and tests/test_seg_frontend_truth_cpu.py (admissibility of
every case, without a GPU).  Pure torch on the CPU; nothing here touches the library.

Every operation is written once, as a function of a dtype: evaluated in float64 it is the truth, in float32 it is "float32
torch doing the same operation" (tests/kernel_parity.py).  Inputs are float32 tensors -- exactly what the kernel is given --
and are widened, never regenerated, for the truth.

The means, rstds, gammas and betas a kernel takes are inputs of its case, chosen here; only the shared sinc pair
(pa_sinc_fir_span + pa_sinc_fix_pool) is given the statistics of its own chunks (float64 on the host, rounded to float32),
because what it is tested for -- cancellation against a DC offset -- exists only when the mean is the mean.

Kept out (and why): DC 0.25 / std 0.005 at N = 160 000 (DC / std = 50).  Float32 torch itself is 0.61 to 0.85 of the
contract away from the float64 truth there, so the case is inadmissible by the rule of kernel_parity; the family stops at
DC / std = 33 (DC 0.1 / std 0.003), where float32 torch stays below one half."""
import functools
import math

import torch
import torch.nn.functional as F

EPS = 1e-5
POISON = 1e30            # what surrounds (and fills the unused gaps of) every kernel input: finite, so that fmaxf keeps it
SINC_STRIDES = (1, 2, 4, 5, 8, 10, 16, 20)
SINC_DEMOTE = 0.5        # csrc/seg_frontend.hip: the shared layer re-centres a span when |mean_0| rstd_0 exceeds it, and
#                          hands a chunk back to the per-chunk kernel when |mean_b - m0| rstd_b does


def poison(n: int) -> torch.Tensor:
    """n float32 values of +-POISON, alternating in sign (|.| and max are involved: one sign could hide)"""
    s = torch.ones(n)
    s[1::2] = -1.0
    return POISON * s


def lrelu(x):
    """leaky ReLU of slope 0.01 in the dtype of x (float32: x * 0.01f, one rounding, as the kernel does it)"""
    return torch.where(x > 0, x, x * 0.01)


def pack_b_image(wk: torch.Tensor, n_tiles: int) -> torch.Tensor:
    """(16 n_tiles, K), K % 4 == 0 -> the B-operand image the kernels read, from the layout their headers state:
    image[(tile KT + kt) 64 + lane] = wk[16 tile + (lane & 15)][4 kt + (lane >> 4)], KT = K / 4"""
    n16, K = wk.shape
    assert n16 == 16 * n_tiles and K % 4 == 0
    KT = K // 4
    tile = torch.arange(n_tiles).view(-1, 1, 1)
    kt = torch.arange(KT).view(1, -1, 1)
    lane = torch.arange(64).view(1, 1, -1)
    tile, kt, lane = torch.broadcast_tensors(tile, kt, lane)
    return wk[16 * tile + (lane & 15), 4 * kt + (lane >> 4)].contiguous().view(-1)


def sinc_image(taps: torch.Tensor) -> torch.Tensor:
    """(80, 251) taps -> packed image [5][63][64]; index 251 is padding and stays zero"""
    return pack_b_image(F.pad(taps, (0, 1)), 5)


def conv5_image(weight: torch.Tensor) -> torch.Tensor:
    """(60, cin, 5) -> packed image [4][5 cin / 4][64], K order k = tap cin + c, output channels 60 .. 63 zero"""
    cout, cin, k = weight.shape
    wk = torch.zeros(64, 5 * cin)
    wk[:cout] = weight.permute(0, 2, 1).reshape(cout, 5 * cin)
    return pack_b_image(wk, 4)


@functools.lru_cache(maxsize=None)
def model_sinc(seed: int = 1234):
    """the (80, 251) sinc filters of the seeded oracle model the GPU suite packs, and the weight and bias of its
    waveform InstanceNorm"""
    from oracle import seeded_pyannet
    model = seeded_pyannet(seed=seed, num_layers=4)
    with torch.no_grad():
        taps = model.sincnet.conv1d[0].filterbank.filters()[:, 0].detach().float().contiguous()
    return taps, float(model.sincnet.wav_norm1d.weight.detach()[0]), float(model.sincnet.wav_norm1d.bias.detach()[0])


def exact_tap_positions() -> torch.Tensor:
    """filter f of the hand-made image has its single tap (value 1) here: all different, 0 and 250 among them"""
    t = (torch.arange(80) * 250) // 79
    assert t[0] == 0 and t[-1] == 250 and t.unique().numel() == 80
    return t


def exact_taps() -> torch.Tensor:
    taps = torch.zeros(80, 251)
    taps[torch.arange(80), exact_tap_positions()] = 1.0
    return taps


# ---------------------------------------------------------------------------------------------------------------------
# pa_row_stats
# ---------------------------------------------------------------------------------------------------------------------
def _rs(name, rows, length, stride, total=None, kind="noise", dc=0.02, spread=0.1):
    return dict(name=name, rows=rows, len=length, stride=stride,
                total=(rows - 1) * stride + length if total is None else total, kind=kind, dc=dc, spread=spread)


ROW_STATS_CASES = [
    _rs("len1", 5, 1, 1),
    _rs("len255_stride_eq", 4, 255, 255),
    _rs("len256_stride_lt", 4, 256, 100),                       # overlapping rows, as the sliding window reads them
    _rs("len257_stride_gt", 4, 257, 300),                       # the gaps between the rows are poisoned
    _rs("len160000_stride_lt_last_cut", 4, 160000, 16000, total=3 * 16000 + 160000 - 4000),
    _rs("len160000_stride_eq", 2, 160000, 160000),
    _rs("last_row_cut_next_wholly_behind", 4, 1000, 1000, total=2500),     # row 2 half zeros, row 3 all zeros
    _rs("stride_gt_rows_behind", 5, 300, 450, total=1000),                 # rows 3 and 4 behind total_len, row 2 cut
    _rs("constant_row", 3, 4000, 4000, kind="constant", dc=0.37),
    _rs("constant_row_cut", 2, 4000, 4000, total=6000, kind="constant", dc=-0.5),
    _rs("dc_1x_spread", 3, 4000, 4000, dc=0.01, spread=0.01),
    _rs("dc_100x_spread", 3, 4000, 4000, dc=1.0, spread=0.01),
    _rs("dc_10000x_spread", 3, 4000, 4000, dc=100.0, spread=0.01),
    _rs("dc_100x_spread_len160000_cut", 3, 160000, 16000, total=2 * 16000 + 160000 - 30000, dc=1.0, spread=0.01),
    _rs("dc_10000x_spread_len257", 6, 257, 257, dc=-100.0, spread=0.01),
]


def row_stats_input(case, seed):
    """(total,) float32; what no row covers (stride > len) is poison"""
    g = torch.Generator().manual_seed(seed)
    n = case["total"]
    if case["kind"] == "constant":
        x = torch.full((n,), case["dc"])
    else:
        x = case["dc"] + case["spread"] * torch.randn(n, generator=g)
    if case["stride"] > case["len"]:
        gap = (torch.arange(n) % case["stride"]) >= case["len"]
        x[gap] = poison(n)[gap]
    return x


def rows_of(x, total, stride, rows, length):
    """(rows, length): row r = x[r stride : r stride + length], zeros from `total` on"""
    idx = torch.arange(rows).view(-1, 1) * stride + torch.arange(length).view(1, -1)
    valid = idx < total
    return torch.where(valid, x[idx.clamp(max=max(total - 1, 0))], torch.zeros((), dtype=x.dtype))


def row_stats(x, case, dtype):
    """mean and 1 / sqrt(biased variance + eps) of the zero-extended rows"""
    r = rows_of(x, case["total"], case["stride"], case["rows"], case["len"]).to(dtype)
    mean = r.mean(-1)
    var = r.var(-1, unbiased=False) if case["len"] > 1 else torch.zeros_like(mean)
    return mean, 1.0 / torch.sqrt(var + EPS)


# ---------------------------------------------------------------------------------------------------------------------
# pa_sinc_fir_pool
# ---------------------------------------------------------------------------------------------------------------------
def chunks_of(wav, wav_len, chunk_stride, B, N):
    """(B, N): chunk b = wav[b chunk_stride : b chunk_stride + N], zeros from wav_len on"""
    return rows_of(wav, wav_len, chunk_stride, B, N)


def sinc_pool_layer(chunks, mean, rstd, gamma, beta, taps, stride, dtype):
    """normalise, filter, magnitude, maxpool3 of every chunk -> (B, 80, P); gamma / beta are taken as float32 values"""
    g32, b32 = torch.tensor(gamma, dtype=torch.float32), torch.tensor(beta, dtype=torch.float32)
    x = chunks.to(dtype)
    xn = (x - mean.to(dtype)[:, None]) * (rstd.to(dtype) * g32.to(dtype))[:, None] + b32.to(dtype)
    y = F.conv1d(xn[:, None], taps.to(dtype)[:, None], stride=stride).abs()
    if y.shape[-1] < 3:
        return y.new_zeros(y.shape[0], 80, 0)
    return F.max_pool1d(y, 3)


def sinc_pool_exact(chunks, stride):
    """the hand-made image with mean 0, rstd 1, gamma 1, beta 0: out[b][f][p] = max_j |x[b][(3 p + j) stride + t_f]|,
    exactly (products with 0 and 1, sums with 0)"""
    B, N = chunks.shape
    P = ((N - 251) // stride + 1) // 3
    t = exact_tap_positions()
    pos = (3 * torch.arange(P).view(1, -1, 1) + torch.arange(3).view(1, 1, -1)) * stride + t.view(-1, 1, 1)   # (80,P,3)
    return chunks[:, pos].abs().amax(-1)


def _sinc_pool_cases():
    cases = []
    for si, s in enumerate(SINC_STRIDES):
        for pi, P in enumerate((1, 127, 128, 129, "full")):
            k = si * 5 + pi
            if P == "full":
                N, B = (160000 if s >= 5 else 32000), 2 + k % 2
            else:
                # L = 3 P + k % 3 positions (up to two that no pooling window takes), and up to s - 1 samples no
                # position takes
                N, B = 251 + (3 * P - 1 + k % 3) * s + k % s, (1, 7, 3)[k % 3]
            step = (N, max(1, N // 3), N + 37)[(k // 2) % 3]             # chunk_stride ==, <, > N
            tail = ("inside", "partly", "wholly")[(k // 3) % 3]        # where wav_len cuts the last chunk
            if B == 1 and tail == "wholly":
                tail = "partly"                                        # (keep a sample to read)
            end = (B - 1) * step + N
            wav_len = {"inside": end, "partly": end - N // 2, "wholly": (B - 1) * step}[tail]
            cases.append(dict(name=f"s{s}_P{P}_B{B}_{'eq' if step == N else 'lt' if step < N else 'gt'}_{tail}",
                              stride=s, N=N, B=B, step=step, wav_len=max(wav_len, 0), end=end,
                              gamma=(1.3, -0.8)[k % 2], beta=0.05))
    # the smallest chunk that yields an output at all: L = 3, P = 1
    for s in SINC_STRIDES:
        cases.append(dict(name=f"s{s}_L3_P1_B2_eq_inside", stride=s, N=251 + 2 * s, B=2, step=251 + 2 * s,
                          wav_len=2 * (251 + 2 * s), end=2 * (251 + 2 * s), gamma=1.3, beta=0.05))
    return cases


SINC_POOL_CASES = _sinc_pool_cases()


def wave(n, seed, dc=0.02, std=0.1, tone=0.05):
    g = torch.Generator().manual_seed(seed)
    x = std * torch.randn(n, generator=g) + dc
    if tone:
        x = x + tone * torch.sin(torch.arange(n) * 0.01)
    return x.float()


def sinc_pool_input(case, seed):
    """wav (wav_len,) with the samples no chunk covers poisoned, mean (B,), rstd (B,)"""
    g = torch.Generator().manual_seed(seed + 1)
    wav = wave(case["wav_len"], seed)
    if case["step"] > case["N"]:
        gap = (torch.arange(case["wav_len"]) % case["step"]) >= case["N"]
        wav[gap] = poison(case["wav_len"])[gap]
    mean = 0.02 + 0.02 * torch.randn(case["B"], generator=g)
    rstd = 1.0 / (0.1 * (0.5 + torch.rand(case["B"], generator=g)))
    return wav, mean, rstd


# ---------------------------------------------------------------------------------------------------------------------
# pa_sinc_fir_span + pa_sinc_fix_pool
# ---------------------------------------------------------------------------------------------------------------------
def _span(name, B, N, step, cut=0, dc=0.02, std=0.1, dc2=None, gamma=None, beta=None, tone=0.05):
    """gamma / beta None: those of the seeded model.  dc2: the offset from the middle of the span on."""
    return dict(name=name, B=B, N=N, step=step, span=(B - 1) * step + N, wav_len=(B - 1) * step + N - cut, dc=dc,
                std=std, dc2=dc2, gamma=gamma, beta=beta, tone=tone)


SPAN_CASES = [
    _span("Pc1", 1, 257, 10, gamma=1.3, beta=0.05),                         # span 251 .. 260: one position, P = 0
    _span("Pc127", 1, 251 + 1260, 10, gamma=1.3, beta=0.05),
    _span("Pc128_B2_Q3", 2, 251 + 1270 - 30, 30, gamma=-0.8, beta=0.05),
    _span("Pc129_cut", 1, 251 + 1280 + 7, 10, cut=300, gamma=1.3, beta=0.05),
    _span("Q100_N32000_B5_cut", 5, 32000, 1000, cut=2500, gamma=-0.8, beta=0.05),
    _span("Q800_N80000_B4", 4, 80000, 8000, gamma=1.3, beta=0.05),
    _span("Q1600_N160000_B7_cut", 7, 160000, 16000, cut=4000, gamma=-0.8, beta=0.05),
]

#: (N, DC, std) of the issue's table: DC / std = 0.2, 2.5, 10, 33, the constant chunk; 4 chunks, step N / 10
DC_FAMILY = [(160000, 0.02, 0.1), (160000, 0.05, 0.02), (160000, 0.1, 0.01), (160000, 0.1, 0.003),
             (80000, 0.1, 0.01), (32000, 0.1, 0.003), (160000, 0.5, 0.0)]
DC_CASES = [_span(f"dc{dc:g}_std{std:g}_N{N}", 4, N, N // 10, dc=dc, std=std, tone=0.0) for N, dc, std in DC_FAMILY]
DC_CASES.append(_span("dc0.05_std0.02_N160000_B7_cut", 7, 160000, 16000, cut=4000, dc=0.05, std=0.02, tone=0.0))
#: the offset steps in the middle of the span, so that chunk means differ: a small step (every chunk stays within
#: SINC_DEMOTE standard deviations of chunk 0's mean) and a large one (the later chunks do not)
STEP_CASES = [_span("dcstep_0.1_to_0.102_std0.01", 7, 160000, 16000, dc=0.1, std=0.01, dc2=0.102, tone=0.0),
              _span("dcstep_0.08_to_0.1_std0.01", 7, 160000, 16000, dc=0.08, std=0.01, dc2=0.1, tone=0.0)]


def span_input(case, seed):
    """wav (wav_len,), and mean / rstd (B,) of the zero-extended chunks: float64 on the host, rounded to float32"""
    n = case["wav_len"]
    wav = wave(n, seed, dc=case["dc"], std=case["std"], tone=case["tone"])
    if case["dc2"] is not None:
        half = case["span"] // 2
        wav[half:] += torch.tensor(case["dc2"] - case["dc"], dtype=torch.float32)
    c = chunks_of(wav, n, case["step"], case["B"], case["N"]).double()
    mean = c.mean(-1)
    rstd = 1.0 / torch.sqrt(c.var(-1, unbiased=False) + EPS)
    return wav, mean.float(), rstd.float()


def span_raw(wav, wav_len, span, m0, taps, dtype):
    """S (80, Pc): the filters over the zero-extended span minus m0 (a float32 value), stride 10"""
    x = rows_of(wav, wav_len, 0, 1, span).to(dtype) - m0.to(dtype)
    return F.conv1d(x[:, None], taps.to(dtype)[:, None], stride=10)[0]


def shared_formula_f32(wav, wav_len, step, B, N, mean, rstd, gamma, beta, taps, m0=None):
    """Float32 emulation of the shared sinc layer, as a plain function: filter the span once (minus m0 when given: the
    re-centred form; None: the raw span, the formula the kernels had before), then per chunk
    |g (S - (mu - m0) S1) + beta S1| and maxpool3.  Says nothing about the kernel: the MFMA sums in another order."""
    f32 = torch.float32
    m0 = torch.zeros((), dtype=f32) if m0 is None else m0.to(f32)
    span = (B - 1) * step + N
    S = span_raw(wav, wav_len, span, m0, taps, f32)
    S1 = taps.double().sum(-1).float()
    Q, P = step // 10, ((N - 251) // 10 + 1) // 3
    out = []
    for b in range(B):
        g = rstd[b] * torch.tensor(gamma, dtype=f32)
        off = torch.tensor(beta, dtype=f32) * S1 - g * (mean[b] - m0) * S1
        v = (g * S[:, b * Q: b * Q + 3 * P] + off[:, None]).abs()
        out.append(v.view(80, P, 3).amax(-1))
    return torch.stack(out)


def span_centre(mean, rstd):
    """m0 of the re-centred pair, in float32 as the kernels evaluate it: chunk 0's mean when it lies further than
    SINC_DEMOTE of chunk 0's standard deviations from zero, else zero (the raw span, bit for bit)"""
    far = mean[0].float().abs() * rstd[0].float() > SINC_DEMOTE
    return mean[0].float() if bool(far) else torch.zeros((), dtype=torch.float32)


def demoted(mean, rstd, m0):
    """the device-side rule, in float32 as the kernels evaluate it"""
    return (mean.float() - m0.float()).abs() * rstd.float() > SINC_DEMOTE


# ---------------------------------------------------------------------------------------------------------------------
# pa_conv5_pool
# ---------------------------------------------------------------------------------------------------------------------
def _cv(name, cin, B, Lin, rows="wild", const_row=False):
    return dict(name=name, cin=cin, B=B, Lin=Lin, P=(Lin - 4) // 3, rows=rows, const_row=const_row)


def _conv5_cases():
    cases = []
    for cin, prod in ((80, 5325), (60, 1773)):           # production: 160 000 samples -> 5 325 -> 1 773 positions
        for i, P in enumerate((1, 31, 32, 33)):
            cases.append(_cv(f"cin{cin}_P{P}", cin, (1, 3, 37, 2)[i], 3 * P + 4 + i % 3, rows=("wild", "unit")[i % 2]))
        cases.append(_cv(f"cin{cin}_P{(prod - 4) // 3}_production", cin, 2, prod))
        cases.append(_cv(f"cin{cin}_P40_constant_row", cin, 3, 125, rows="unit", const_row=True))
    return cases


CONV5_CASES = _conv5_cases()


def conv5_input(case, seed):
    """x (B, cin, Lin), mean / rstd (B cin), gamma / beta (cin) of both signs, weight (60, cin, 5), bias (60).
    rows == "wild": neighbouring rows differ by up to 1e6 in scale (the element behind a row's end is the next row's
    first); the statistics follow the row, so that the normalised values stay of order one."""
    g = torch.Generator().manual_seed(seed)
    B, cin, Lin = case["B"], case["cin"], case["Lin"]
    R = B * cin
    scale = torch.ones(R)
    if case["rows"] == "wild":
        scale = 10.0 ** ((torch.arange(R) * 7) % 3 * 3.0 - 3.0)                   # 1e-3, 1, 1e3, ...
    center = scale * torch.randn(R, generator=g)
    x = center[:, None] + scale[:, None] * torch.randn(R, Lin, generator=g)
    mean = center + 0.1 * scale * torch.randn(R, generator=g)
    rstd = (0.5 + torch.rand(R, generator=g)) / scale
    if case["const_row"]:                                 # rows 1, 1 + cin, ...: constant input, the rstd of variance 0
        x[1::cin] = center[1::cin, None]
        mean[1::cin] = center[1::cin]
        rstd[1::cin] = 1.0 / math.sqrt(EPS)
    gamma = (0.5 + torch.rand(cin, generator=g)) * torch.where(torch.arange(cin) % 3 == 1, -1.0, 1.0)
    beta = 0.3 * torch.randn(cin, generator=g)
    weight = torch.randn(60, cin, 5, generator=g) / math.sqrt(5 * cin)
    bias = 0.2 * torch.randn(60, generator=g)
    return x.view(B, cin, Lin).float(), mean.float(), rstd.float(), gamma.float(), beta.float(), weight, bias


def conv5_pool(x, mean, rstd, gamma, beta, weight, bias, dtype):
    """IN + leaky ReLU on the input, conv1d k = 5, bias, maxpool3 -> (B, 60, P)"""
    B, cin, Lin = x.shape
    sc = (rstd.to(dtype).view(B, cin) * gamma.to(dtype)[None])[:, :, None]
    a = lrelu((x.to(dtype) - mean.to(dtype).view(B, cin, 1)) * sc + beta.to(dtype)[None, :, None])
    y = F.conv1d(a, weight.to(dtype), bias.to(dtype))
    if y.shape[-1] < 3:
        return y.new_zeros(B, 60, 0)
    return F.max_pool1d(y, 3)


def conv5_exact_weights(cin):
    """one weight of value 1 per output channel: channel o reads input channel (7 o + 3) % cin at tap o % 5"""
    o = torch.arange(60)
    c, t = (7 * o + 3) % cin, o % 5
    w = torch.zeros(60, cin, 5)
    w[o, c, t] = 1.0
    return w, c, t


def conv5_pool_exact(x, c, t, bias):
    """mean 0, rstd 1, gamma 1, beta 0 and conv5_exact_weights: out[b][o][p] = max_j lrelu(x[b][c_o][3 p + j + t_o]) +
    bias[o], every step one float32 operation"""
    B, cin, Lin = x.shape
    P = (Lin - 4) // 3
    pos = 3 * torch.arange(P).view(1, -1, 1) + torch.arange(3).view(1, 1, -1) + t.view(-1, 1, 1)        # (60, P, 3)
    a = lrelu(x)[:, c.view(-1, 1, 1), pos]                                                             # (B, 60, P, 3)
    return a.amax(-1) + bias.view(1, -1, 1)


# ---------------------------------------------------------------------------------------------------------------------
# pa_norm_transpose
# ---------------------------------------------------------------------------------------------------------------------
NORM_T_CASES = [dict(name=f"B{B}_T{T}", B=B, T=T, rows=("wild", "unit")[i % 2], cin=60, Lin=T, const_row=False)
                for i, (B, T) in enumerate(((1, 1), (15, 63), (16, 64), (17, 65), (37, 589), (1, 589), (37, 1),
                                            (16, 65), (17, 63), (15, 64)))]


def norm_transpose_input(case, seed):
    x, mean, rstd, gamma, beta, _, _ = conv5_input(case, seed)
    return x, mean, rstd, gamma, beta


def norm_transpose(x, mean, rstd, gamma, beta, dtype):
    """IN + leaky ReLU, as LSTM input rows (ntiles, T, 16, 64): chunk b = 16 tile + b16; channels 60 .. 63 and the
    chunks from B on are zero"""
    B, C, T = x.shape
    sc = (rstd.to(dtype).view(B, C) * gamma.to(dtype)[None])[:, :, None]
    a = lrelu((x.to(dtype) - mean.to(dtype).view(B, C, 1)) * sc + beta.to(dtype)[None, :, None])     # (B, 60, T)
    ntiles = (B + 15) // 16
    out = torch.zeros(ntiles * 16, T, 64, dtype=dtype)
    out[:B, :, :C] = a.permute(0, 2, 1)
    return out.view(ntiles, 16, T, 64).permute(0, 2, 1, 3).contiguous()
