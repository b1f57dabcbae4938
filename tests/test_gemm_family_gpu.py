"""k_gemm_tn (csrc/seg_lstm.hip) through its three entry points against a float64 product: seeded shape / stride /
epilogue fuzzing of pa_gemm_tn_ex, the batched launch of the wav2vec attention (pa_gemm_tn_batched) and the argument
refusals.  Rules of the comparison: tests/kernel_parity.py."""
import math

import pytest
import torch
import torch.nn.functional as F

from kernel_parity import SEED_OFFSET, Guarded, assert_parity, dptr, ratio

pytestmark = pytest.mark.gpu

N_PLAIN, N_MODE1 = 40, 6


def _ri(rng, lo, hi):
    return int(torch.randint(lo, hi + 1, (1,), generator=rng))


def _plain_cases():
    """the 40 out_mode-0 cases: the first 8 sit in the nn == 8 band (N in 897 .. 1024), 3 of them with more than 8 row
    tiles (M > 1024); cases 8 and 9 have fewer than 16 rows; the rest is free"""
    rng = torch.Generator().manual_seed(4100 + SEED_OFFSET)
    cases = []
    for i in range(N_PLAIN):
        M = _ri(rng, 1025, 1500) if i < 3 else _ri(rng, 1, 15) if i in (8, 9) else _ri(rng, 1, 1500)
        N = _ri(rng, 897, 1024) if i < 8 else _ri(rng, 1, 1100)
        K = 32 * _ri(rng, 1, 32)
        # the float64 truth and the float32 reference cost 2 M N K multiply-adds: ~2e9 at most (they never exceed
        # 1500 x 1100 x 1024 = 1.7e9 here)
        lda = K + (0, 4, 36)[_ri(rng, 0, 2)]
        ldw = K + (0, 4, 36)[_ri(rng, 0, 2)]
        ldc = N + (0, 1, 13)[_ri(rng, 0, 2)]
        cases.append(dict(M=M, N=N, K=K, lda=lda, ldw=ldw, ldc=ldc, act=i % 4, res=bool(_ri(rng, 0, 1)),
                          bias=i % 4 != (i // 4) % 4, seed=5000 + i + SEED_OFFSET))
    return cases


def test_case_list_covers_the_geometry():
    cases = _plain_cases()
    band = [c for c in cases if 897 <= c["N"] <= 1024]
    assert len(cases) >= 40 and len(band) >= 8 and sum(c["M"] > 1024 for c in band) >= 3
    assert any(c["M"] < 16 for c in cases) and any(c["M"] % 4 for c in cases) and any(c["M"] % 16 for c in cases)
    assert any(c["M"] % 128 for c in cases) and any(c["M"] > 1024 for c in cases)
    assert any(c["N"] % 128 for c in cases)
    assert {c["act"] for c in cases} == {0, 1, 2, 3} and {c["res"] for c in cases} == {True, False}
    assert sum(not c["bias"] for c in cases) * 4 >= len(cases)
    for key, extra in (("lda", "K"), ("ldw", "K")):
        assert {c[key] - c[extra] for c in cases} == {0, 4, 36}
    assert {c["ldc"] - c["N"] for c in cases} == {0, 1, 13}
    # every combination of activation and bias / no bias occurs
    assert {(c["act"], c["bias"]) for c in cases} == {(a, b) for a in range(4) for b in (True, False)}


def _act64(z, act):
    if act == 1:
        return torch.where(z > 0, z, 0.01 * z)
    if act == 2:
        return z.clamp_min(0)
    if act == 3:
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    return z


def _act32(z, act):
    return (z, F.leaky_relu(z, 0.01), F.relu(z), F.gelu(z))[act]


def _operands(c):
    """A (M, lda) and W (N, ldw) with NaN in the padding columns (nothing may read them), bias, residual (M, ldc)"""
    rng = torch.Generator().manual_seed(c["seed"])
    M, N, K = c["M"], c["N"], c["K"]
    A = torch.full((M, c["lda"]), float("nan"))
    W = torch.full((N, c["ldw"]), float("nan"))
    A[:, :K] = torch.randn(M, K, generator=rng)
    W[:, :K] = torch.randn(N, K, generator=rng) / K ** 0.5
    bias = torch.randn(N, generator=rng) if c["bias"] else None
    res = None
    if c.get("res"):
        res = torch.full((M, c["ldc"]), float("nan"))
        res[:, :N] = torch.randn(M, N, generator=rng)
    return A, W, bias, res


def _truth_and_reference(c, A, W, bias, res):
    M, N, K = c["M"], c["N"], c["K"]
    z64 = A[:, :K].double() @ W[:, :K].double().T
    z32 = A[:, :K] @ W[:, :K].T
    if bias is not None:
        z64, z32 = z64 + bias.double(), z32 + bias
    if res is not None:
        z64, z32 = z64 + res[:, :N].double(), z32 + res[:, :N]
    return _act64(z64, c["act"]), _act32(z32, c["act"])


@pytest.mark.parametrize("block", range(4))
def test_fuzz_gemm_tn_ex(gpu_device, block):
    """pa_gemm_tn_ex, out_mode 0: M 1 .. 1500, N 1 .. 1100, K 32 .. 1024, padded leading dimensions on all three
    matrices, the four activations, residual, NULL bias -- against float64, output inside NaN guards and gaps"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    for c in _plain_cases()[block * 10:(block + 1) * 10]:
        A, W, bias, res = _operands(c)
        truth, ref32 = _truth_and_reference(c, A, W, bias, res)
        M, N, K, ldc = c["M"], c["N"], c["K"], c["ldc"]
        Ad, Wd = A.to(gpu_device), W.to(gpu_device)
        bd = bias.to(gpu_device) if bias is not None else None
        rd = res.to(gpu_device) if res is not None else None
        out = Guarded(M * ldc, gpu_device)
        ffi.check(lib.pa_gemm_tn_ex(dptr(Ad), c["lda"], dptr(Wd), c["ldw"], dptr(bd), dptr(rd), out.ptr, ldc, M, N, K,
                                    c["act"], 0, ffi.stream()), f"gemm {c}")
        written = torch.zeros(M, ldc, dtype=torch.bool)
        written[:, :N] = True
        got = out.check(written, str(c)).view(M, ldc)[:, :N]
        tag = "gemm_ex_M{M}_N{N}_K{K}_lda{lda}_ldw{ldw}_ldc{ldc}_act{act}".format(**c) + \
              ("_res" if c["res"] else "") + ("" if c["bias"] else "_nobias")
        assert_parity(tag, got, truth, ref32)


def test_fuzz_gemm_tn_gate_layout(gpu_device):
    """out_mode 1 (the LSTM gate pre-activations): C[((m >> 4) N + n) 16 + (m & 15)], M a multiple of 16, no activation"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    rng = torch.Generator().manual_seed(4200 + SEED_OFFSET)
    for i in range(N_MODE1):
        c = dict(M=16 * _ri(rng, 1, 90), N=_ri(rng, 897, 1024) if i < 2 else _ri(rng, 1, 1100), K=32 * _ri(rng, 1, 32),
                 act=0, bias=i % 3 != 2, seed=5100 + i + SEED_OFFSET)
        c["lda"], c["ldw"], c["ldc"] = c["K"] + (0, 4, 36)[i % 3], c["K"] + (36, 0, 4)[i % 3], c["N"]
        A, W, bias, _ = _operands(c)
        truth, ref32 = _truth_and_reference(c, A, W, bias, None)
        M, N, K = c["M"], c["N"], c["K"]
        Ad, Wd = A.to(gpu_device), W.to(gpu_device)
        bd = bias.to(gpu_device) if bias is not None else None
        out = Guarded(M * N, gpu_device)
        ffi.check(lib.pa_gemm_tn(dptr(Ad), c["lda"], dptr(Wd), c["ldw"], dptr(bd), out.ptr, 0, M, N, K, 0, 1,
                                 ffi.stream()), f"gemm {c}")
        got = out.check(None, str(c)).view(M // 16, N, 16).permute(0, 2, 1).reshape(M, N)
        assert_parity(f"gemm_gates_M{M}_N{N}_K{K}_lda{c['lda']}_ldw{c['ldw']}" + ("" if c["bias"] else "_nobias"),
                      got, truth, ref32)


def _batched(lib, ffi, dev, tag, M, N, K, outer, inner, lda, sAo, sAi, ldw, sWo, sWi, ldc, sCo, sCi, act, with_bias,
             seed):
    """one launch of outer x inner products on flat NaN-filled operand buffers; every product against float64"""
    rng = torch.Generator().manual_seed(seed)
    na = (outer - 1) * sAo + (inner - 1) * sAi + (M - 1) * lda + K
    nw = (outer - 1) * sWo + (inner - 1) * sWi + (N - 1) * ldw + K
    nc = (outer - 1) * sCo + (inner - 1) * sCi + (M - 1) * ldc + N
    A, W = torch.full((na,), float("nan")), torch.full((nw,), float("nan"))
    bias = torch.randn(N, generator=rng) if with_bias else None
    written = torch.zeros(nc, dtype=torch.bool)
    rows_a = torch.arange(M).view(-1, 1) * lda + torch.arange(K).view(1, -1)
    rows_w = torch.arange(N).view(-1, 1) * ldw + torch.arange(K).view(1, -1)
    rows_c = torch.arange(M).view(-1, 1) * ldc + torch.arange(N).view(1, -1)
    prods = []
    for zo in range(outer):
        for zi in range(inner):
            a, w = torch.randn(M, K, generator=rng), torch.randn(N, K, generator=rng) / K ** 0.5
            # (operands of neighbouring products may interleave -- heads inside a row -- but never overlap)
            assert torch.isnan(A[zo * sAo + zi * sAi + rows_a]).all() and torch.isnan(W[zo * sWo + zi * sWi + rows_w]).all()
            assert not written[zo * sCo + zi * sCi + rows_c].any()
            A[zo * sAo + zi * sAi + rows_a] = a
            W[zo * sWo + zi * sWi + rows_w] = w
            written[zo * sCo + zi * sCi + rows_c] = True
            prods.append((zo, zi, a, w))
    Ad, Wd = A.to(dev), W.to(dev)
    bd = bias.to(dev) if with_bias else None
    out = Guarded(nc, dev)
    ffi.check(lib.pa_gemm_tn_batched(dptr(Ad), lda, sAo, sAi, dptr(Wd), ldw, sWo, sWi, dptr(bd), out.ptr, ldc, sCo, sCi,
                                     M, N, K, outer, inner, act, ffi.stream()), tag)
    flat = out.check(written, tag)
    got, truth, ref32 = [], [], []
    for zo, zi, a, w in prods:
        got.append(flat[zo * sCo + zi * sCi + rows_c])
        z64, z32 = a.double() @ w.double().T, a @ w.T
        if with_bias:
            z64, z32 = z64 + bias.double(), z32 + bias
        truth.append(_act64(z64, act))
        ref32.append(_act32(z32, act))
    assert_parity(tag, torch.stack(got), torch.stack(truth), torch.stack(ref32))


def test_gemm_tn_batched_attention_shapes(gpu_device):
    """the two batched products of the wav2vec encoder: scores = Q K^T per (chunk, head) straight from the (T, D)
    projections (lda = ldw = D, head stride D / H, chunk stride T D; ldc = Tp), and P V from padded probabilities"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    for i, (chunks, heads, T, Dh) in enumerate(((3, 4, 49, 64), (2, 12, 149, 64), (1, 3, 130, 32))):
        D, Tp = heads * Dh, (T + 3) // 4 * 4 + 4
        _batched(lib, ffi, gpu_device, f"gemm_batched_QK_c{chunks}_h{heads}_T{T}_d{Dh}", T, T, Dh, chunks, heads,
                 D, T * D, Dh, D, T * D, Dh, Tp, heads * T * Tp, T * Tp, 0, False, 4300 + i + SEED_OFFSET)
        # P V: A = probabilities (T, Tk) with row stride Tk (a multiple of 32 = K), W = V^T (Dh, Tk) per head,
        # output columns head * Dh of the (T, D) context
        Tk = (T + 31) // 32 * 32
        _batched(lib, ffi, gpu_device, f"gemm_batched_PV_c{chunks}_h{heads}_T{T}_d{Dh}", T, Dh, Tk, chunks, heads,
                 Tk, heads * T * Tk, T * Tk, Tk, heads * Dh * Tk, Dh * Tk, D, T * D, Dh, 0, False,
                 4350 + i + SEED_OFFSET)


def test_gemm_tn_batched_free_form(gpu_device):
    """outer, inner in 1 .. 7, six different strides (multiples of 4), GELU and none, shared and NULL bias"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    rng = torch.Generator().manual_seed(4400 + SEED_OFFSET)
    seen = set()
    for i in range(8):
        outer, inner = (1, 7) if i == 0 else (7, 1) if i == 1 else (_ri(rng, 1, 7), _ri(rng, 1, 7))
        M, N, K = _ri(rng, 1, 300), _ri(rng, 1, 300), 32 * _ri(rng, 1, 8)
        lda, ldw, ldc = K + 4 * _ri(rng, 0, 3), K + 4 * _ri(rng, 0, 3), N + _ri(rng, 0, 5)
        sAi = M * lda + 4 * (1 + i)
        sWi = N * ldw + 4 * (9 + i)
        sCi = (M * ldc + 3) // 4 * 4 + 4 * (17 + i)
        sAo, sWo, sCo = inner * sAi + 4 * 25, inner * sWi + 4 * 33, inner * sCi + 4 * 41
        assert len({sAo, sAi, sWo, sWi, sCo, sCi}) == 6
        act, with_bias = (0, 3)[i % 2], i % 4 < 2
        seen.add((act, with_bias))
        _batched(lib, ffi, gpu_device, f"gemm_batched_free_{outer}x{inner}_M{M}_N{N}_K{K}_act{act}" +
                 ("" if with_bias else "_nobias"), M, N, K, outer, inner, lda, sAo, sAi, ldw, sWo, sWi, ldc, sCo, sCi,
                 act, with_bias, 4450 + i + SEED_OFFSET)
    assert len(seen) == 4


def test_gemm_refusals_write_nothing(gpu_device):
    """invalid arguments: return 3, a message in pa_last_error(), the output untouched"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    M, N, K = 32, 40, 64
    A = torch.randn(M, K + 4, device=gpu_device)
    W = torch.randn(N, K + 4, device=gpu_device)
    b = torch.randn(N, device=gpu_device)
    R = torch.randn(M, N, device=gpu_device)
    out = Guarded(M * N, gpu_device)
    st = ffi.stream()
    calls = {
        "K % 32": lambda: lib.pa_gemm_tn_ex(dptr(A), K + 4, dptr(W), K + 4, dptr(b), None, out.ptr, N, M, N, 48, 0, 0, st),
        "lda % 4": lambda: lib.pa_gemm_tn_ex(dptr(A), K + 2, dptr(W), K + 4, dptr(b), None, out.ptr, N, M, N, K, 0, 0, st),
        "ldw % 4": lambda: lib.pa_gemm_tn(dptr(A), K + 4, dptr(W), K + 1, dptr(b), out.ptr, N, M, N, K, 0, 0, st),
        "residual with out_mode 1": lambda: lib.pa_gemm_tn_ex(dptr(A), K + 4, dptr(W), K + 4, dptr(b), dptr(R), out.ptr,
                                                              N, M, N, K, 0, 1, st),
        "unknown act": lambda: lib.pa_gemm_tn_ex(dptr(A), K + 4, dptr(W), K + 4, dptr(b), None, out.ptr, N, M, N, K, 7,
                                                 0, st),
        "act with out_mode 1": lambda: lib.pa_gemm_tn(dptr(A), K + 4, dptr(W), K + 4, dptr(b), out.ptr, N, M, N, K, 1,
                                                      1, st),
        "out_mode 1 with M % 16": lambda: lib.pa_gemm_tn(dptr(A), K + 4, dptr(W), K + 4, dptr(b), out.ptr, N, 24, N, K,
                                                         0, 1, st),
        "batched: more than 65535 products": lambda: lib.pa_gemm_tn_batched(
            dptr(A), K + 4, 0, 0, dptr(W), K + 4, 0, 0, dptr(b), out.ptr, N, 0, 0, M, N, K, 256, 256, 0, st),
        "batched: K % 32": lambda: lib.pa_gemm_tn_batched(
            dptr(A), K + 4, 0, 0, dptr(W), K + 4, 0, 0, dptr(b), out.ptr, N, 0, 0, M, N, 48, 1, 1, 0, st),
        "batched: stride % 4": lambda: lib.pa_gemm_tn_batched(
            dptr(A), K + 4, 0, 2, dptr(W), K + 4, 0, 0, dptr(b), out.ptr, N, 0, 0, M, N, K, 1, 1, 0, st),
        "batched: unknown act": lambda: lib.pa_gemm_tn_batched(
            dptr(A), K + 4, 0, 0, dptr(W), K + 4, 0, 0, dptr(b), out.ptr, N, 0, 0, M, N, K, 1, 1, 2, st),
    }
    for what, call in calls.items():
        assert call() == 3, what
        assert lib.pa_last_error().decode().strip(), what
        assert out.untouched(), what
        with pytest.raises(ValueError):
            ffi.check(3, what)
    # ... and the same operands are accepted once the arguments are right
    ffi.check(lib.pa_gemm_tn_ex(dptr(A), K + 4, dptr(W), K + 4, dptr(b), dptr(R), out.ptr, N, M, N, K, 2, 0, st), "gemm")
    got = out.check(None, "accepted call").view(M, N)
    a, w = A.cpu()[:, :K], W.cpu()[:, :K]
    truth = (a.double() @ w.double().T + b.cpu().double() + R.cpu().double()).clamp_min(0)
    assert_parity("gemm_after_refusals", got, truth, F.relu(a @ w.T + b.cpu() + R.cpu()))
    assert ratio(got, truth) <= 1.0
