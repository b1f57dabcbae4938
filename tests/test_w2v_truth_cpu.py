"""What tests/test_w2v_kernels_gpu.py rests on, checked where no GPU is needed:
  * admissibility of every value case (tests/kernel_parity.py): float32 torch, doing the same operation, is within HALF
    the contract (rtol 1e-4 / atol 1e-5) of the float64 truth.  A badly chosen case is found here, not on the GPU machine;
  * the truths of tests/w2v_truth.py, in float64, equal the modules of oracle.wav2vec2 run in double to 1e-12 of the
    largest value (tap order, group order, the dropped frame of an even kernel, the gate).  The oracle is itself pinned
    to HuggingFace transformers by tests/test_oracle_wav2vec2_pin.py;
  * the re-packing of the positional weight the GPU test does equals what SSeRiouSSPack uploads.
Nothing here says anything about a kernel."""
import ctypes

import numpy as np
import pytest
import torch

import w2v_truth as T
from kernel_parity import SEED_OFFSET, ratio

HALF = 0.5
F32, F64 = torch.float32, torch.float64
_ids = dict(ids=lambda c: c["name"])


def _admissible(name, ref32, truth64):
    r = ratio(ref32, truth64)
    print(f"{name}: float32 torch {r:.4f} of the contract")
    assert r <= HALF, f"{name}: inadmissible case -- float32 torch is {r:.3f} of the contract away from float64"


def _pinned(name, mine, theirs):
    assert mine.dtype == theirs.dtype == F64 and mine.shape == theirs.shape
    rel = float((mine - theirs).abs().max() / theirs.abs().max())
    print(f"{name}: {rel:.2e} of the largest value")
    assert rel <= 1e-12, f"{name}: the truth is {rel:.2e} away from the oracle module"


# ---------------------------------------------------------------------------------------------------------------------
# admissibility
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.CONV0_CASES, **_ids)
def test_conv0_cases_are_admissible(case):
    wav, w, bias = T.conv0_input(case, 100 + SEED_OFFSET)
    assert case["T"] >= 1 and (case["T"] - 1) * case["S0"] + case["K0"] <= case["N"]
    for b in (bias, None):
        truth = T.conv0(wav, case, w, b, F64)
        assert truth.shape == (case["B"], case["T"], case["C"])
        _admissible("conv0_" + case["name"], T.conv0(wav, case, w, b, F32), truth)
    # the one-tap weights: the float64 convolution IS the gather
    w1, tap = T.conv0_exact_weights(case)
    assert set(tap.tolist()) == set(range(case["K0"]))
    assert torch.equal(T.conv0(wav, case, w1, None, F64).float(), T.conv0_exact(wav, case, tap))


def test_conv0_cases_cover_the_branches():
    c = T.CONV0_CASES
    assert any(x["T"] < 32 for x in c) and any(x["T"] % 32 for x in c) and any(x["T"] > 64 for x in c)
    assert any(x["C"] > 256 for x in c) and any(x["K0"] < x["S0"] for x in c) and any(x["K0"] > x["S0"] for x in c)
    assert any(x["K0"] == 16 and x["S0"] == 16 for x in c) and any(x["K0"] == 1 for x in c)
    assert any(x["wav_len"] < x["end"] for x in c) and {0} < set(T.CONV0_PADS)


@pytest.mark.parametrize("case", T.GN_CASES, **_ids)
def test_group_norm_cases_are_admissible(case):
    x, gamma, beta = T.gn_input(case, 200 + SEED_OFFSET)
    y64, m64, r64 = T.group_norm_gelu(x, gamma, beta, F64)
    y32, m32, r32 = T.group_norm_gelu(x, gamma, beta, F32)
    _admissible("group_norm_" + case["name"], y32, y64)
    _admissible("group_norm_mean_" + case["name"], m32, m64)
    _admissible("group_norm_rstd_" + case["name"], r32, r64)
    if case["mean"]:
        assert float((m64.abs() / case["mean"] - 1).abs().max()) < 0.1
    assert bool((gamma > 0).any()) and bool((gamma < 0).any())


def test_group_norm_of_one_row_is_gelu_of_beta():
    """T = 1: the row is its own mean, whatever it holds -- the closed form the GPU test uses"""
    x, gamma, beta = T.gn_input(T.GN_ONE_ROW, 200 + SEED_OFFSET)
    y, m, r = T.group_norm_gelu(x, gamma, beta, F64)
    assert torch.equal(y, T.gelu(beta.double()).expand(1, 1, -1)) and torch.equal(m, x[:, 0].double())
    assert torch.equal(r, torch.full_like(r, 1.0 / np.sqrt(T.EPS)))
    assert T.GN_ONE_ROW not in T.GN_CASES and all(c["T"] > 1 for c in T.GN_CASES)


@pytest.mark.parametrize("case", T.LN_CASES, **_ids)
def test_layer_norm_cases_are_admissible(case):
    x, gamma, beta = T.ln_input(case, 300 + SEED_OFFSET)
    for with_gelu in (False, True):
        _admissible(f"layer_norm_{case['name']}_gelu{int(with_gelu)}", T.layer_norm(x, gamma, beta, with_gelu, F32),
                    T.layer_norm(x, gamma, beta, with_gelu, F64))


@pytest.mark.parametrize("case", T.POSCONV_CASES, **_ids)
def test_posconv_cases_are_admissible(case):
    x, w, bias = T.posconv_input(case, 400 + SEED_OFFSET)
    truth = T.posconv(x, w, bias, case["groups"], F64)
    assert truth.shape == x.shape
    _admissible("posconv_" + case["name"], T.posconv(x, w, bias, case["groups"], F32), truth)


@pytest.mark.parametrize("case", T.SOFTMAX_CASES, **_ids)
def test_softmax_cases_are_admissible(case):
    S, scale, bias, xin, gw, gb, gc = T.softmax_input(case, 500 + SEED_OFFSET)
    gated = T.attention_softmax(S, scale, F64, bias, xin, gw, gb, gc)
    plain = T.attention_softmax(S, scale, F64)
    _admissible("softmax_gated_" + case["name"], T.attention_softmax(S, scale, F32, bias, xin, gw, gb, gc), gated)
    _admissible("softmax_plain_" + case["name"], T.attention_softmax(S, scale, F32), plain)
    assert float((gated.sum(-1) - 1).abs().max()) < 1e-12
    if case["T"] >= 33:
        # several entries per row above 0.05 (an error of the gate then moves values far above atol), and the bias matters
        assert float((plain > 0.05).sum(-1).float().mean()) >= 2.0
        assert ratio(plain, gated) > 100.0
    assert gc.unique().numel() == case["H"]
    if case["variant"] == "spike60":
        assert float(plain[:, :, case["T"] // 2, -1].min()) > 1.0 - 1e-12


def test_softmax_cases_cover_the_branches():
    c = T.SOFTMAX_CASES
    assert {32, 64, 96, 128} <= {x["hd"] for x in c}
    assert any(x["Tp"] % 32 for x in c) and any((x["B"] * x["H"] * x["T"]) % 4 for x in c)
    assert any(x["T"] == 1 for x in c) and any(x["T"] > 64 * 4 for x in c) and all(x["Tp"] >= x["T"] for x in c)
    assert {"row_plus80", "spike60"} <= {x["variant"] for x in c}


def test_axpy_and_to_tiles_truths():
    g = torch.Generator().manual_seed(600 + SEED_OFFSET)
    acc, x = torch.randn(1028, generator=g), torch.randn(1028, generator=g)
    _admissible("axpy", T.axpy(acc, x, 0.37, 0, F32), T.axpy(acc, x, 0.37, 0, F64))
    assert torch.equal(T.axpy(acc, x, 0.37, 1, F32), torch.tensor(0.37) * x)
    for case in T.TILES_CASES:
        x = torch.arange(case["B"] * case["T"] * case["D"], dtype=F32).view(case["B"], case["T"], case["D"]) + 1
        tiles = T.to_tiles(x)
        assert tiles.shape == ((case["B"] + 15) // 16, case["T"], 16, case["D"])
        assert torch.equal(tiles[tiles != 0].sort().values, x.reshape(-1))
        b = case["B"] - 1
        assert torch.equal(tiles[b >> 4, :, b & 15], x[b])


# ---------------------------------------------------------------------------------------------------------------------
# the truths are the oracle's modules
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,groups,KW,Tn", [(128, 4, 32, 49), (96, 3, 5, 17), (64, 2, 1, 16), (64, 2, 32, 7)])
def test_posconv_truth_is_the_oracle_module(D, groups, KW, Tn):
    from oracle.wav2vec2 import ConvolutionalPositionalEmbedding
    torch.manual_seed(7 + SEED_OFFSET)
    m = ConvolutionalPositionalEmbedding(D, KW, groups).double()
    with torch.no_grad():
        m.conv.bias.normal_(0.0, 0.2)
        x = torch.randn(2, Tn, D, dtype=F64)
        theirs = x + m(x)
        mine = T.posconv(x, m.conv.weight.detach(), m.conv.bias.detach(), groups, F64)
    _pinned(f"posconv_D{D}_g{groups}_k{KW}", mine, theirs)


@pytest.mark.parametrize("hd,H", [(32, 4), (128, 2)])
def test_gated_softmax_truth_is_the_oracle_attention(hd, H):
    """the gate and the gated soft-max against WavLMSelfAttention: its `gate`, and the probabilities of its
    scaled_dot_product_attention read off with the identity as values"""
    import torch.nn.functional as F
    from oracle.wav2vec2 import WavLMSelfAttention
    torch.manual_seed(8 + SEED_OFFSET)
    D, B, Tn = H * hd, 2, 21
    att = WavLMSelfAttention(D, H, True, 40, 100).double()
    with torch.no_grad():
        att.gru_rel_pos_const.copy_(1.0 + 0.2 * torch.arange(H, dtype=F64).view(1, H, 1, 1))
        att.gru_rel_pos_linear.bias.normal_(0.0, 0.3)
        att.rel_attn_embed.weight.normal_(0.0, 1.0)
        x = torch.randn(B, Tn, D, dtype=F64)
        q, k = torch.randn(B, H, Tn, hd, dtype=F64), torch.randn(B, H, Tn, hd, dtype=F64)
        bias = att.compute_bias(Tn, Tn)                                                        # (H, T, T)
        their_gate = att.gate(x)                                                               # (B, H, T, 1)
        mask = (their_gate.view(B, H, -1, 1) * bias[None]).view(B, H, Tn, Tn)
        eye = torch.eye(Tn, dtype=F64).expand(B, H, Tn, Tn)
        theirs = F.scaled_dot_product_attention(q, k, eye, attn_mask=mask)
        gw, gb, gc = att.gru_rel_pos_linear.weight, att.gru_rel_pos_linear.bias, att.gru_rel_pos_const.reshape(-1)
        _pinned(f"gate_hd{hd}", T.wavlm_gate(x, H, gw, gb, gc, F64), their_gate[..., 0])
        mine = T.attention_softmax(q @ k.transpose(-1, -2), hd ** -0.5, F64, bias, x, gw, gb, gc)
        # (the scale travels as a float32 value, as the kernel takes it; hd ** -0.5 of 32 and 128 is not exact in float32)
        exact = T.attention_softmax(q @ k.transpose(-1, -2) * (hd ** -0.5), 1.0, F64, bias, x, gw, gb, gc)
    _pinned(f"gated_softmax_hd{hd}", exact, theirs)
    assert float((mine - exact).abs().max()) < 1e-6


@pytest.mark.parametrize("C,K0,S0,N", [(64, 10, 5, 1600), (32, 16, 16, 800), (64, 2, 5, 163)])
def test_conv0_group_norm_truth_is_the_oracle_block(C, K0, S0, N):
    from oracle.wav2vec2 import FeatureExtractor
    torch.manual_seed(9 + SEED_OFFSET)
    block = FeatureExtractor("group_norm", [(C, K0, S0)], False).double().conv_layers[0]
    with torch.no_grad():
        block.layer_norm.weight.normal_(1.0, 0.2)
        block.layer_norm.bias.normal_(0.0, 0.3)
        wav = 0.1 * torch.randn(2, N, dtype=F64)
        theirs = block(wav[:, None]).transpose(1, 2)                                           # (B, T, C)
        case = dict(B=2, N=N, step=N, wav_len=2 * N, S0=S0, T=(N - K0) // S0 + 1)
        y = T.conv0(wav.reshape(-1), case, block.conv.weight[:, 0], None, F64)
        mine, _, _ = T.group_norm_gelu(y, block.layer_norm.weight, block.layer_norm.bias, F64)
    _pinned(f"conv0_group_norm_C{C}_K{K0}_S{S0}", mine, theirs)


@pytest.mark.parametrize("with_gelu", [False, True])
def test_layer_norm_truth_is_torch_layer_norm(with_gelu):
    import torch.nn.functional as F
    x, gamma, beta = T.ln_input(dict(rows=5, C=1000), 300 + SEED_OFFSET)
    theirs = F.layer_norm(x.double(), (1000,), gamma.double(), beta.double(), T.EPS)
    _pinned("layer_norm", T.layer_norm(x, gamma, beta, with_gelu, F64), F.gelu(theirs) if with_gelu else theirs)


# ---------------------------------------------------------------------------------------------------------------------
# the re-packing of the positional weight
# ---------------------------------------------------------------------------------------------------------------------
def _floats(pointer, shape):
    n = int(np.prod(shape))
    addr = pointer if isinstance(pointer, int) else pointer.value
    return torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * n).from_address(addr)).reshape(shape).copy())


def test_repacking_is_that_of_the_pack():
    """[g][j][ci][co] as tests/w2v_truth.py builds it from the reference-layout weight == what SSeRiouSSPack uploads"""
    import oracle.models as om
    from pyannote_audio_amd.weights import SSeRiouSSPack
    cfg = dict(om.TINY_WAV2VEC2)
    model = om.seeded_sseriouss(wav2vec=cfg, num_layers=1)
    pack = SSeRiouSSPack(model.state_dict(), {"wav2vec": cfg, "wav2vec_layer": -1, "lstm": {"num_layers": 1}}, 7, 3, 2,
                         torch.device("cpu"))
    sd = model.state_dict()
    pc = "wav2vec.encoder.transformer.pos_conv_embed.conv.parametrizations.weight.original"
    g_, v_ = sd[pc + "0"], sd[pc + "1"]
    groups, KW, D = cfg["encoder_pos_conv_groups"], cfg["encoder_pos_conv_kernel"], cfg["encoder_embed_dim"]
    CG = D // groups
    weight = v_ * (g_ / torch.linalg.vector_norm(v_, dim=(0, 1), keepdim=True))      # weight_norm(dim=2) materialised
    assert weight.shape == (D, CG, KW)
    module = model.wav2vec.encoder.transformer.pos_conv_embed.conv.weight.detach()
    assert torch.allclose(weight, module, rtol=1e-5, atol=1e-9)
    mine = T.repack_pos_weight(weight, groups)
    assert torch.equal(mine, _floats(pack.struct.pos_w, (groups, KW, CG, CG)))
    # and index by index: [g][j][ci][co] is weight[g CG + co][ci][j]
    for g, j, ci, co in ((0, 0, 1, 2), (3, KW - 1, CG - 1, 0), (2, 5, 0, CG - 1)):
        assert mine[g, j, ci, co] == weight[g * CG + co, ci, j]
