"""Case tables, input families, float64 truths, float32 host replays and integer weight images of the three 3x3
convolution families (csrc/emb_resnet.hip: pa_conv3x3; csrc/emb_winograd.hip: pa_conv3x3_wino[_rows];
csrc/emb_winograd4.hip: pa_conv3x3_wino4[_rows]), shared by tests/test_conv_kernels_gpu.py (the kernels, on an MI355X)
and tests/test_conv_truth_cpu.py (everything that can be pinned without a GPU).  Pure torch on the CPU; nothing here
touches the library.  Tensors are NCHW here; the GPU test permutes to the kernels' NHWC.

Four parts:
  * the launchers' dispatch, restated (`direct_instantiation`, `wino_instantiation`, `wino4_mode`, `xcd_ranges`) with the
    number of workgroup tiles of a launch; every case CLAIMS the instantiation it is there for and the CPU test holds
    the claim against the restated rule;
  * float cases: `float_inputs` draws one of five seeded families, `conv_of` / `finish` are the float64 truth and, in
    float32, "float32 torch doing the same operation" of tests/kernel_parity.py;
  * `wino4_replay` / `wino2_replay`: the Winograd arithmetic in float32 on the host, vectorised over tiles -- the
    recipes of tests/test_winograd4_cpu.py (bt, at, point order xi = 6a + b, U read back from the slab image) and of
    tests/test_winograd_cpu.py, input channels accumulated one by one in ascending order, a product rounded before it
    is added.  F(4x4) is held to max(1, 2 x the replay's distance from the truth): by design its element-wise error is
    not that of a direct convolution, so float32 torch is no stand-in for it;
  * exact cases: small integers and sparse integer weights, with weight images chosen so that EVERY float32 intermediate
    of every algorithm is an integer below 2^24 (`exact_proof` computes the largest one) -- the kernel must then
    reproduce the integer convolution bit for bit, whatever its summation order.

Kept out (and why): whole inputs scaled by 10 (x = 10 randn and its post-ReLU twins).  Float32 torch itself measured 0.30 to
0.56 of the contract away from the float64 truth there, so the family is inadmissible by the rule of kernel_parity; the
per-channel factors of `cin-scale` / `cout-scale` reach the same decade on SOME channels and stay admissible."""
import math

import torch
import torch.nn.functional as F

CUS = 256                 # compute units of an MI355X
COST_CAP = 2e9            # multiply-adds of one case's float64 truth (the cap of tests/test_fuzz_gpu.py)
EXACT_LIMIT = 1 << 24     # integers of smaller magnitude are float32 values, and so are their sums and differences
FAMILIES = ("randn", "relu", "relu+2", "cin-scale", "cout-scale")


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------
# the launchers' dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------
#: k_conv3x3<S, TH, TWT, BN>: stride, tile rows, 32-pixel tile columns, output channels of a workgroup tile
DIRECT_INSTANTIATIONS = ((1, 8, 1, 32), (1, 8, 1, 64), (1, 4, 2, 64), (1, 2, 2, 64), (2, 4, 1, 32), (2, 2, 2, 32))
#: k_conv3x3_wino32, k_conv3x3_wino<TR, TCG>
WINO_INSTANTIATIONS = ("wino32", (4, 1), (2, 2), (1, 4))
#: k_conv3x3_wino4<MODE>: row-shaped, tile-private, run-shaped units
WINO4_MODES = (0, 1, 2)
#: workgroups (F(2x2) 32 -> 32: halves of a workgroup) that claim tiles of one launch on CUS compute units
CLAIMERS = {"direct": 2 * CUS, "wino": 2 * CUS, "wino4": CUS}


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def direct_instantiation(cout, H, stride):
    """pa_conv3x3 (csrc/emb_resnet.hip)"""
    Ho = (H - 1) // stride + 1
    if stride == 1:
        if cout == 32:
            return (1, 8, 1, 32)
        return (1, 8, 1, 64) if Ho >= 32 else (1, 4, 2, 64) if Ho >= 16 else (1, 2, 2, 64)
    if stride == 2:
        return (2, 4, 1, 32) if Ho >= 16 else (2, 2, 2, 32)
    raise ValueError(f"stride {stride}")


def wino_instantiation(cin, cout, H, W, y_first=0):
    """pa_conv3x3_wino_rows (csrc/emb_winograd.hip): the workgroup tile that pads the rows of the launch the least, ties
    to the taller tile; the two-halves kernel for 32 -> 32 whole maps where the 8 x 32 tile is chosen"""
    Hr = H - y_first

    def padded(tr, tcg):
        return cdiv(Hr, 2 * tr) * 2 * tr * cdiv(W, 32 * tcg) * 32 * tcg
    a41, a22, a14 = padded(4, 1), padded(2, 2), padded(1, 4)
    if a41 <= a22 and a41 <= a14:
        return "wino32" if (cin == 32 and cout == 32 and y_first == 0) else (4, 1)
    return (2, 2) if a22 <= a14 else (1, 4)


def wino4_mode(B, H, W, rows):
    """wino4_unit_mode (csrc/emb_winograd4.hip) without PA_WINO4_LINEAR"""
    if rows != H:
        return 0
    tcols, trows = cdiv(W, 4), cdiv(H, 4)
    lin_units, row_units = cdiv(B * trows * tcols, 16), B * trows * cdiv(W, 64)
    if tcols >= 5 and lin_units * 118 <= row_units * 100:
        return 2
    return 1 if lin_units * 120 <= row_units * 100 else 0


def xcd_ranges(case) -> bool:
    """tile order of a launch without PA_XCD_RANGES: contiguous ranges per XCD everywhere but F(4x4) at 256 output
    channels (xcd_ranges_wanted(n_tiles < 8))"""
    return case["algo"] != "wino4" or case["cout"] // 32 < 8


def instantiation(case):
    if case["algo"] == "direct":
        return direct_instantiation(case["cout"], case["H"], case["stride"])
    if case["algo"] == "wino":
        return wino_instantiation(case["cin"], case["cout"], case["H"], case["W"], case["y_first"])
    return wino4_mode(case["B"], case["H"], case["W"], case["rows"])


def workgroup_tiles(case) -> int:
    """tiles a launch hands out through its tile queue (holes of the padded index space not counted)"""
    B, H, W, cout = case["B"], case["H"], case["W"], case["cout"]
    inst = instantiation(case)
    if case["algo"] == "direct":
        S, TH, TWT, BN = inst
        Ho, Wo = out_hw(H, W, S)
        return cdiv(Wo, 32 * TWT) * cdiv(Ho, TH) * (cout // BN) * B
    if case["algo"] == "wino":
        tr, tcg = (4, 1) if inst == "wino32" else inst
        return cdiv(W, 32 * tcg) * cdiv(H - case["y_first"], 2 * tr) * B * (cout // 32)
    tiles = (cdiv(W, 4) if inst else cdiv(W, 64)) * cdiv(case["rows"], 4) * B
    units = cdiv(tiles, 16) if inst else tiles
    return cdiv(units, 4) * (cout // 32)


def cost(case) -> int:
    """multiply-adds of the float64 truth (the whole map, also for a row range)"""
    Ho, Wo = out_hw(case["H"], case["W"], case["stride"])
    return case["B"] * Ho * Wo * 9 * case["cin"] * case["cout"]


def written_rows(case):
    """output rows [lo, hi) a launch writes"""
    Ho, _ = out_hw(case["H"], case["W"], case["stride"])
    if case["algo"] == "wino":
        return case["y_first"], Ho
    if case["algo"] == "wino4":
        return 0, case["rows"]
    return 0, Ho


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def _case(algo, claims, B, H, W, cin, cout, stride=1, y_first=0, rows=None, many=False, tag=""):
    name = f"{algo}_{cin}to{cout}_{H}x{W}_B{B}"
    if stride != 1:
        name += f"_s{stride}"
    if y_first:
        name += f"_yfirst{y_first}"
    if rows is not None:
        name += f"_rows{rows}"
    return dict(name=name + tag, algo=algo, claims=claims, B=B, H=H, W=W, cin=cin, cout=cout, stride=stride,
                y_first=y_first, rows=H if rows is None else rows, many=many)


def _cases():
    D, W2, W4 = "direct", "wino", "wino4"
    cases = [
        # ---- pa_conv3x3: the smallest maps that reach each instantiation, a map wider than one tile for both widths
        _case(D, (1, 8, 1, 32), 2, 5, 9, 32, 32),
        _case(D, (1, 8, 1, 32), 2, 9, 35, 64, 32),
        _case(D, (1, 8, 1, 64), 1, 33, 7, 32, 64),
        _case(D, (1, 4, 2, 64), 2, 17, 9, 64, 64),
        _case(D, (1, 4, 2, 64), 1, 17, 70, 64, 64),
        _case(D, (1, 2, 2, 64), 3, 3, 5, 128, 128),
        _case(D, (1, 2, 2, 64), 2, 1, 1, 128, 128),
        _case(D, (2, 4, 1, 32), 2, 31, 9, 32, 64, stride=2),          # Ho = 16 from an odd ...
        _case(D, (2, 4, 1, 32), 2, 32, 10, 32, 64, stride=2),         # ... and from an even input
        _case(D, (2, 2, 2, 32), 2, 9, 7, 128, 256, stride=2),
        _case(D, (2, 2, 2, 32), 2, 10, 8, 128, 256, stride=2),
        _case(D, (2, 2, 2, 32), 1, 30, 131, 16, 64, stride=2),        # Ho = 15: the last height of this one; Wo = 66
        # ---- every workgroup claims at least two tiles (cin = 16: the smallest the kernel accepts)
        _case(D, (1, 8, 1, 32), 1024, 3, 5, 16, 32, many=True),
        _case(D, (1, 8, 1, 64), 205, 33, 2, 16, 64, many=True),
        _case(D, (1, 4, 2, 64), 205, 17, 3, 16, 64, many=True),
        _case(D, (1, 2, 2, 64), 256, 3, 2, 16, 128, many=True),
        _case(D, (2, 4, 1, 32), 128, 31, 3, 16, 64, stride=2, many=True),
        _case(D, (2, 2, 2, 32), 256, 5, 4, 16, 64, stride=2, many=True),
        # ---- pa_conv3x3_wino: each tile shape on a map that fills it, and on its ragged twin
        _case(W2, "wino32", 2, 8, 32, 32, 32),
        _case(W2, "wino32", 3, 7, 33, 32, 32),
        _case(W2, (4, 1), 2, 8, 32, 64, 64),
        _case(W2, (4, 1), 2, 7, 33, 32, 64),
        _case(W2, (2, 2), 2, 4, 64, 128, 128),
        _case(W2, (2, 2), 2, 3, 65, 64, 128),
        _case(W2, (1, 4), 1, 2, 128, 256, 256),
        _case(W2, (1, 4), 2, 1, 129, 128, 256),
        # ---- pa_conv3x3_wino_rows with y_first > 0: the rows above stay untouched
        _case(W2, (1, 4), 2, 10, 125, 256, 256, y_first=8),
        _case(W2, (2, 2), 3, 6, 40, 64, 64, y_first=4),
        _case(W2, (4, 1), 3, 7, 30, 32, 32, y_first=4),               # (32 -> 32, yet not the two-halves kernel)
        _case(W2, "wino32", 1024, 5, 3, 32, 32, many=True),
        _case(W2, (4, 1), 1024, 5, 3, 16, 32, many=True),
        _case(W2, (2, 2), 1024, 4, 33, 16, 32, many=True),
        _case(W2, (1, 4), 1024, 2, 65, 16, 32, many=True),
        # ---- pa_conv3x3_wino4, row-shaped units (5 x 129 with one image takes RUN-shaped units: see below)
        _case(W4, 0, 1, 4, 128, 64, 64),
        _case(W4, 0, 1, 5, 125, 32, 256),
        # ---- tile-private patches: maps under 5 tiles wide, several images per 16-tile unit (units straddle images),
        #      a map smaller than one unit, cin % 8 == 0 but not % 16
        _case(W4, 1, 8, 8, 12, 32, 256),
        _case(W4, 1, 37, 3, 3, 256, 256),
        _case(W4, 1, 5, 5, 9, 40, 32),
        _case(W4, 1, 2, 8, 16, 128, 128),
        # ---- run-shaped units: at least 5 tiles per row
        _case(W4, 2, 8, 8, 20, 64, 64),
        _case(W4, 2, 9, 7, 22, 32, 256),
        _case(W4, 2, 1, 5, 129, 32, 32),
        # ---- pa_conv3x3_wino4_rows below H: groups of 4 units straddle images
        _case(W4, 0, 3, 6, 70, 40, 64, rows=4),
        _case(W4, 0, 3, 10, 70, 64, 64, rows=8),
        _case(W4, 0, 2, 10, 38, 32, 256, rows=8),
        # ---- every workgroup claims at least two (group of 4 units, 32 output channels) tiles
        _case(W4, 0, 2048, 1, 53, 32, 32, many=True),
        _case(W4, 1, 32768, 2, 2, 32, 32, many=True),
        _case(W4, 2, 6560, 1, 17, 32, 32, many=True),
    ]
    for i, c in enumerate(cases):
        c["index"] = i
        c["family"] = FAMILIES[i % len(FAMILIES)]
        # variant 0 / 1 of a case: (residual, ReLU); both launches share inputs and the convolution of the truth
        c["variants"] = ((True, True), (False, False)) if i % 2 == 0 else ((True, False), (False, True))
    return cases


CASES = _cases()


def float_seed(case, offset=0):
    return 7000 + case["index"] + offset


def exact_seed(case, variant, offset=0):
    return 9000 + 2 * case["index"] + variant + offset


def _family_cases():
    """all five families on one geometry per kernel family (the issue's 2 x 256 x 8 x 16 map for F(4x4))"""
    out = []
    for base in (_case("direct", (1, 4, 2, 64), 2, 17, 9, 64, 64), _case("direct", (2, 4, 1, 32), 2, 31, 9, 32, 64, stride=2),
                 _case("wino", (4, 1), 2, 7, 33, 64, 64), _case("wino4", 1, 2, 8, 16, 256, 256),
                 _case("wino4", 2, 4, 6, 38, 128, 128)):
        for k, fam in enumerate(FAMILIES):
            c = dict(base, name=f"{base['name']}_{fam}", family=fam, index=len(CASES) + len(out),
                     variants=(((True, True), (False, False)) if k % 2 == 0 else ((True, False), (False, True))))
            out.append(c)
    return out


FAMILY_CASES = _family_cases()
FLOAT_CASES = CASES + FAMILY_CASES
EXACT_CASES = CASES


# ---------------------------------------------------------------------------------------------------------------------
# float cases: inputs and truth
# ---------------------------------------------------------------------------------------------------------------------
def float_inputs(case, seed):
    """x (B, cin, H, W), w (cout, cin, 3, 3), shift (cout), R (B, cout, Ho, Wo) of the case's family, all float32"""
    g = torch.Generator().manual_seed(seed)
    B, H, W, cin, cout, fam = case["B"], case["H"], case["W"], case["cin"], case["cout"], case["family"]
    assert fam in FAMILIES
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3 * math.sqrt(cin))
    shift = torch.randn(cout, generator=g)
    Ho, Wo = out_hw(H, W, case["stride"])
    R = torch.randn(B, cout, Ho, Wo, generator=g)
    if fam != "randn":
        x = F.relu(x)                                                    # what a ResNet feeds its convolutions
    if fam == "relu+2":
        x = x + 2.0                                                      # ... with a large mean
    if fam == "cin-scale":
        x = x * (10.0 ** (2 * torch.rand(cin, generator=g) - 1)).view(1, -1, 1, 1)
    if fam == "cout-scale":
        w = w * (10.0 ** (2 * torch.rand(cout, generator=g) - 1)).view(-1, 1, 1, 1)      # folded BatchNorm
    return x.contiguous(), w.contiguous(), shift, R


def conv_of(x, w, stride, dtype):
    """the convolution alone in `dtype` from float32 (or integer-valued) operands, widened, never regenerated"""
    return F.conv2d(x.to(dtype), w.to(dtype), stride=stride, padding=1)


def finish(conv, shift, R, use_res, relu):
    """relu?(conv + shift [+ R]) in the dtype of conv, in the kernels' order"""
    y = conv + shift.to(conv.dtype).view(1, -1, 1, 1)
    if use_res:
        y = y + R.to(conv.dtype)
    return F.relu(y) if relu else y


# ---------------------------------------------------------------------------------------------------------------------
# weight images
# ---------------------------------------------------------------------------------------------------------------------
def direct_image(w):
    """(cout, cin, 3, 3) -> [9][cout][cin], tap = 3 dy + dx"""
    cout, cin = w.shape[:2]
    return w.permute(2, 3, 0, 1).reshape(9, cout, cin).float().contiguous()


def wino2_unpack(P):
    """weights.winograd_pack's image [cout/32][cin/16][512][4 slots][4] -> U [16][cout][cin], read at the kernel's
    addresses: row r = 32 xi + n holds channel quad g at slot (g + 2 ((r >> 2) & 1)) & 3"""
    no, nc = P.shape[:2]
    r = torch.arange(512)
    slot_of_quad = (torch.arange(4)[None, :] + 2 * ((r >> 2) & 1)[:, None]) & 3
    A = torch.gather(P, 3, slot_of_quad.view(1, 1, 512, 4, 1).expand(no, nc, 512, 4, 4))
    return A.reshape(no, nc, 16, 32, 16).permute(2, 0, 3, 1, 4).reshape(16, 32 * no, 16 * nc).contiguous()


def wino4_unpack(P):
    """weights.winograd4_pack's image [cout/32][cin/8][32 xi + n][8] -> U [36][cout][cin], read at the kernel's
    addresses: rows whose n has bit 3 set hold their two channel quads swapped"""
    no, nc = P.shape[:2]
    A = P.reshape(no, nc, 36, 32, 8)
    swapped = torch.cat([A[..., 4:], A[..., :4]], dim=-1)
    A = torch.where(((torch.arange(32) >> 3) & 1).bool().view(1, 1, 1, 32, 1), swapped, A)
    return A.permute(2, 0, 3, 1, 4).reshape(36, 32 * no, 8 * nc).contiguous()


#: 24 G of F(4x4, 3x3): integral
G24 = torch.tensor([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]], dtype=torch.int64)


def wino4_int_image(w):
    """(24 G) w (24 G)^T in int64 for integer w -> [36][cout][cin] int64 = 576 times the F(4x4) weight image, every
    entry exact (weights.winograd4_weights goes through float64 1/6 and 1/24 and leaves 1e-13 where the entry is 0)"""
    w = w.to(torch.int64)
    U = torch.einsum("ap,oipq,bq->aboi", G24, w, G24)
    return U.reshape(36, w.shape[0], w.shape[1]).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# float32 host replays of the Winograd kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def bt4(x):
    """the kernel's wino4_bt as tests/test_winograd4_cpu.py::bt spells it, on a sequence of six tensors"""
    a = x[4] - 4 * x[2]
    b = x[3] - 4 * x[1]
    c = x[4] - x[2]
    d = x[3] - x[1]
    return [4 * x[0] + (x[4] - 5 * x[2]), a + b, a - b, c + 2 * d, c - 2 * d, 4 * x[1] + (x[5] - 5 * x[3])]


def at4(m):
    """tests/test_winograd4_cpu.py::at, on a sequence of six tensors -> four"""
    s1, d1, s2, d2 = m[1] + m[2], m[1] - m[2], m[3] + m[4], m[3] - m[4]
    return [m[0] + s1 + s2, d1 + 2 * d2, s1 + 4 * s2, d1 + 8 * d2 + m[5]]


def bt2(x):
    """B^T of F(2x2): csrc/emb_winograd.hip and tests/test_winograd_cpu.py"""
    return [x[0] - x[2], x[1] + x[2], x[2] - x[1], x[1] - x[3]]


def at2(m):
    return [m[0] + m[1] + m[2], m[1] - m[2] - m[3]]


def _along(recipe, t, dim):
    return torch.stack(recipe(t.unbind(dim)), dim)


def _patches(x, m):
    """(B, cin, H, W) -> (B, cin, th, tw, m + 2, m + 2): the zero-padded input patches of the m x m output tiles"""
    H, W = x.shape[2:]
    th, tw = cdiv(H, m), cdiv(W, m)
    xp = F.pad(x, (1, m * tw + 1 - W, 1, m * th + 1 - H))
    return xp.unfold(2, m + 2, m).unfold(3, m + 2, m)


def _replay(x, U, m, bt, at, dtype, chunk_tiles=2048):
    """Y = A^T [ sum_c U_c . (B^T d B)_c ] A over all tiles in `dtype`: columns then rows of the patch through `bt`, the
    input channels one by one in ascending order (a rounded product, then a rounded sum), point rows then point columns
    through `at`.  x (B, cin, H, W), U [(m + 2)^2][cout][cin] -> (B, cout, H, W)."""
    B, cin, H, W = x.shape
    n, cout = m + 2, U.shape[1]
    th, tw = cdiv(H, m), cdiv(W, m)
    d = _patches(x.to(dtype), m)
    Ut = U.to(dtype).permute(2, 0, 1).contiguous()                            # [cin][points][cout]
    out = torch.empty(B, cout, m * th, m * tw, dtype=dtype)
    step = max(1, chunk_tiles // (th * tw))
    for b0 in range(0, B, step):
        v = _along(bt, _along(bt, d[b0:b0 + step], 4), 5)                     # (b, cin, th, tw, a, b)
        nb = v.shape[0]
        v = v.permute(1, 0, 2, 3, 4, 5).reshape(cin, nb * th * tw, n * n, 1)
        M = torch.zeros(nb * th * tw, n * n, cout, dtype=dtype)
        for c in range(cin):
            M += Ut[c] * v[c]
        y = _along(at, _along(at, M.view(-1, n, n, cout), 1), 2)              # (tiles, p, q, cout)
        out[b0:b0 + nb] = y.view(nb, th, tw, m, m, cout).permute(0, 5, 1, 3, 2, 4).reshape(nb, cout, m * th, m * tw)
    return out[:, :, :H, :W]


def wino4_replay(x, slabs, dtype=torch.float32):
    """the F(4x4) convolution alone, from the packed weight image the kernel is given"""
    return _replay(x, wino4_unpack(slabs), 4, bt4, at4, dtype)


def wino2_replay(x, slabs, dtype=torch.float32):
    """the F(2x2) convolution alone, from the packed weight image the kernel is given"""
    return _replay(x, wino2_unpack(slabs), 2, bt2, at2, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------------
#: variant -> (input range, nz input channels per output channel, taps in [-k, k]): signed inputs, and a post-ReLU
#: twin.  F(4x4) multiplies by 576 and its inverse transform, bounded with absolute values, by up to 19^2 more: fewer
#: and smaller taps keep it below 2^24 (measured by exact_proof: 0.8 of 2^24 already at (-4, 4, 4, 2))
EXACT_VARIANTS = {"direct": ((-4, 4, 4, 2), (0, 8, 8, 3)), "wino": ((-4, 4, 4, 2), (0, 8, 8, 3)),
                  "wino4": ((-4, 4, 2, 2), (0, 8, 2, 1))}
#: what the weight image multiplies the convolution by: 4 makes G (4 w) G^T of F(2x2) integral (G is dyadic, halves
#: only), 576 = 24^2 clears the 1/6 and 1/24 of F(4x4)'s G
EXACT_GAIN = {"direct": 4, "wino": 4, "wino4": 576}


def exact_inputs(case, seed, variant):
    """integer-valued float32 operands: x in [lo, hi], w sparse with nz input channels per output channel and taps in
    [-k, k], shift in [-8, 8], R in [-16, 16]; `variant`: an index into EXACT_VARIANTS, or (lo, hi, nz, k) itself"""
    lo, hi, nz, k = EXACT_VARIANTS[case["algo"]][variant] if isinstance(variant, int) else variant
    g = torch.Generator().manual_seed(seed)
    B, H, W, cin, cout = case["B"], case["H"], case["W"], case["cin"], case["cout"]
    x = torch.randint(lo, hi + 1, (B, cin, H, W), generator=g).float()
    chans = torch.rand(cout, cin, generator=g).argsort(1)[:, :nz]            # nz different input channels each
    taps = torch.randint(-k, k + 1, (cout, nz, 3, 3), generator=g).float()
    w = torch.zeros(cout, cin, 3, 3)
    w.scatter_(1, chans.view(cout, nz, 1, 1).expand(cout, nz, 3, 3), taps)
    shift = torch.randint(-8, 9, (cout,), generator=g).float()
    Ho, Wo = out_hw(H, W, case["stride"])
    R = torch.randint(-16, 17, (B, cout, Ho, Wo), generator=g).float()
    return x, w, shift, R


def exact_image(case, w):
    """what the kernel is given for integer weights w: -> (the unpacked integer image as float32, the packed image)"""
    from pyannote_audio_amd.weights import winograd4_pack, winograd_pack, winograd_weights
    if case["algo"] == "direct":
        img = direct_image(4 * w)
        return img, img
    if case["algo"] == "wino":
        U = winograd_weights(4 * w)
        return U, winograd_pack(U)
    U = wino4_int_image(w).float()
    return U, winograd4_pack(U)


def exact_truth(case, x, w, shift, R, use_res, relu):
    """gain x (integer convolution) + shift [+ R], in float64 (every value an integer far below 2^53), as float32"""
    conv = EXACT_GAIN[case["algo"]] * conv_of(x, w, case["stride"], torch.float64)
    y = finish(conv, shift, R, use_res, relu)
    assert bool((y == y.round()).all()) and float(y.abs().max()) < EXACT_LIMIT
    return y.float()


_BT = {2: torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64),
       4: torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0],
                        [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=torch.float64)}
_AT = {2: torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64),
       4: torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]],
                       dtype=torch.float64)}


def exact_proof(case, x, w, shift, R):
    """Largest magnitude any float32 intermediate of the case's algorithm can take, whatever the order of its sums: every
    product and partial sum is bounded by the same expression with absolute values throughout.  Integer arithmetic,
    carried in float64 (exact: every value is an integer below 2^53, asserted) so that the contractions run at GEMM
    speed; the weight images themselves are built in int64.
      direct:   sum over taps and channels of |4 w| |x|, + |shift| + |R|
      Winograd: |B^T| |d| |B| (the input transform), sum over channels of |U| |V| (the accumulators),
                |A^T| (that) |A| (both stages of the inverse transform), + |shift| + |R|
    -> dict of the stage maxima (int)"""
    tail = int(shift.abs().max()) + int(R.abs().max())
    if case["algo"] == "direct":
        acc = conv_of(x.abs(), (4 * w).abs(), case["stride"], torch.float64)
        stages = dict(accumulate=acc.max().item())
        stages["epilogue"] = stages["accumulate"] + tail
    else:
        m = 2 if case["algo"] == "wino" else 4
        U, _ = exact_image(case, w)
        Ua = U.double().abs()                                                  # [points][cout][cin]
        d = _patches(x.double().abs(), m)                                      # (B, cin, th, tw, n, n)
        Ba, Aa = _BT[m].abs(), _AT[m].abs()
        stages = dict(weights=Ua.max().item(), transform=0.0, accumulate=0.0, inverse=0.0)
        B = x.shape[0]
        tiles = d.shape[2] * d.shape[3]
        step = max(1, 4096 // tiles)
        for b0 in range(0, B, step):
            V = torch.einsum("ai,bcyxij,dj->adbyxc", Ba, d[b0:b0 + step], Ba)  # bounds |V| and the stage in between
            n = m + 2
            V = V.reshape(n * n, -1, V.shape[-1])                              # [points][tiles][cin]
            M = torch.bmm(V, Ua.transpose(1, 2))                               # [points][tiles][cout]: sum |U| |V|
            Y = torch.einsum("pa,abto,qb->pqto", Aa, M.view(n, n, -1, M.shape[-1]), Aa)
            stages["transform"] = max(stages["transform"], V.max().item())
            stages["accumulate"] = max(stages["accumulate"], M.max().item())
            stages["inverse"] = max(stages["inverse"], Y.max().item())
        stages["epilogue"] = stages["inverse"] + tail
    assert all(v < 2.0 ** 53 and v == int(v) for v in stages.values())
    return {k: int(v) for k, v in stages.items()}


def exact_replay(case, x, packed, shift, R, use_res, relu):
    """the float32 host evaluation of an exact case from the image the kernel is given"""
    if case["algo"] == "direct":
        cout, cin = packed.shape[1:]
        conv = conv_of(x, packed.view(3, 3, cout, cin).permute(2, 3, 0, 1), case["stride"], torch.float32)
    elif case["algo"] == "wino":
        conv = wino2_replay(x, packed)
    else:
        conv = wino4_replay(x, packed)
    return finish(conv, shift, R, use_res, relu)
