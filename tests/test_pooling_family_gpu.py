"""The statistics-pooling kernels (csrc/emb_pool.hip, csrc/emb_ragged.hip), the ragged-batch helpers and the ResNet
stem, each through its own entry point against float64: the formula in the header of csrc/emb_pool.hip
(v1 = sum w + 1e-8; mean = sum(x w) / v1; var = sum((x - mean)^2 w) / (v1 - sum(w^2) / v1 + 1e-8)), torch's
std(correction = 1) for the unweighted row form, F.conv2d for the stem, the oracle's kaldi fbank in float64.
Rules of the comparison: tests/kernel_parity.py.

One trap in the truth itself: when a single frame carries weight, both 1e-8 terms are below float32 resolution --
float32 gives mean = x and std = 0 exactly, where the float64 formula gives std of about 6e-5 |x|.  Such rows (counted
from the weights, before any output is looked at) are held to the float32 StatsPool of the oracle, as the reference's
own known-answer tests do."""
import pytest
import torch
import torch.nn.functional as F

from kernel_parity import GUARD, SEED_OFFSET, Guarded, assert_parity, dptr, ratio

pytestmark = pytest.mark.gpu

KINDS = ("fractional", "zero", "one_frame", "ones", "small", "binary")


def _weights(rng, kind, Fm):
    if kind == "fractional":
        return torch.rand(Fm, generator=rng)
    if kind == "zero":
        return torch.zeros(Fm)
    if kind == "one_frame":
        w = torch.zeros(Fm)
        w[int(torch.randint(Fm, (1,), generator=rng))] = 1.0
        return w
    if kind == "ones":
        return torch.ones(Fm)
    if kind == "small":
        return 1e-6 * (0.5 + torch.rand(Fm, generator=rng))
    return (torch.rand(Fm, generator=rng) < 0.6).float()


def _single_frame_rows_get_weight_one(masks, idx):
    """masks (B, S, Fm) in place: a row that, after nearest interpolation, weights exactly ONE frame gets weight 1 there.
    With a fractional weight w the case is ill-posed in float32 -- x w / (w + 1e-8) need not return x, and
    v1 - w^2 / v1 + 1e-8 is an ulp of w against 1e-8, of either sign: float32 torch returns rounding noise over 1e-8 for
    the std there (1e-3 |x| where float64 says 6e-5 |x|), the kernel the same or NaN when that denominator rounds
    below zero.  An input rule, applied before anything is computed."""
    w = masks[:, :, idx.long()]
    single = (w != 0).sum(-1) == 1
    masks[single] = (masks[single] != 0).float()
    return masks


def _nearest_idx(Fm, Tp):
    """source index of F.interpolate(mode="nearest") from Fm to Tp frames"""
    ramp = torch.arange(Fm, dtype=torch.float32).view(1, 1, Fm)
    return F.interpolate(ramp, size=Tp, mode="nearest").view(-1).to(torch.int32)


def _pool(x, w, dtype):
    """x (..., D, T), w (..., T) already at pool resolution -> (..., 2 D): the weighted formula in `dtype`"""
    x, w = x.to(dtype), w.to(dtype).unsqueeze(-2)
    v1 = w.sum(-1) + 1e-8
    mean = (x * w).sum(-1) / v1
    var = ((x - mean.unsqueeze(-1)) ** 2 * w).sum(-1) / (v1 - (w * w).sum(-1) / v1 + 1e-8)
    return torch.cat([mean, var.sqrt()], -1)


def _compare_rows(tag, got, truth, ref32, single):
    """rows (leading dimensions) flagged `single` -- one weighted frame -- against float32, all others against float64"""
    single = single.reshape(-1)
    got, truth, ref32 = (t.reshape(single.numel(), -1) for t in (got, truth, ref32))
    if bool((~single).any()):
        assert_parity(tag, got[~single], truth[~single], ref32[~single])
    if bool(single.any()):
        assert_parity(tag + "_single_frame_vs_float32", got[single], ref32[single].double(), ref32[single])


def _stats_pool_case(lib, ffi, dev, tag, B, Fh, C, Tp, S, Fm, kinds, seed, offset=0.0, spread=1.0, masks_null=False):
    rng = torch.Generator().manual_seed(seed)
    feat = offset + spread * torch.randn(B, Fh, Tp, C, generator=rng)            # NHWC map of layer 4
    seq = feat.permute(0, 3, 1, 2).reshape(B, C * Fh, Tp)                        # d = c Fh + f
    if masks_null:
        S, masks, idx = 1, None, None
        w = torch.ones(B, 1, Tp)
    else:
        masks = torch.stack([torch.stack([_weights(rng, kinds[(b * S + s) % len(kinds)], Fm) for s in range(S)])
                             for b in range(B)])
        idx = _nearest_idx(Fm, Tp)
        w = _single_frame_rows_get_weight_one(masks, idx)[:, :, idx.long()]
        assert Fm == Tp or torch.equal(w, F.interpolate(masks, size=Tp, mode="nearest"))
    truth = _pool(seq.unsqueeze(1), w, torch.float64)                            # (B, S, 2 D)
    ref32 = _pool(seq.unsqueeze(1), w, torch.float32)
    single = (w != 0).sum(-1) == 1
    fd = feat.to(dev)
    md = masks.to(dev) if masks is not None else None
    idd = idx.to(dev) if idx is not None else None
    out = Guarded(B * S * 2 * C * Fh, dev)
    ffi.check(lib.pa_stats_pool(dptr(fd), B, Fh, Tp, C, dptr(md), S, Fm, dptr(idd), out.ptr, ffi.stream()), tag)
    got = out.check(None, tag).view(B, S, 2 * C * Fh)
    _compare_rows(tag, got, truth, ref32, single)


@pytest.mark.parametrize("Fh", [1, 10])
@pytest.mark.parametrize("C", [32, 256, 320, 1024])
def test_stats_pool(gpu_device, Fh, C):
    """pa_stats_pool at every pool length (1, 2, 15 / 16 / 17 around the load batch, 125, the 512 limit), 1 .. 4
    speakers, masks at pool resolution and at other resolutions (nearest), all kinds of weights, and no masks at all"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    for i, Tp in enumerate((1, 2, 15, 16, 17, 125, 512)):
        S = 1 + (i + C // 32 + Fh) % 4
        Fm = (Tp, 3 * Tp + 1, max(1, Tp // 2), Tp + 7)[(i + Fh) % 4]
        B = 3 if Tp < 512 else 2
        kinds = KINDS[i % len(KINDS):] + KINDS[:i % len(KINDS)]
        _stats_pool_case(lib, ffi, gpu_device, f"stats_pool_Fh{Fh}_C{C}_Tp{Tp}_S{S}_Fm{Fm}", B, Fh, C, Tp, S, Fm, kinds,
                         9000 + 16 * i + Fh + C + SEED_OFFSET)
        if i % 3 == (C // 32) % 3:
            _stats_pool_case(lib, ffi, gpu_device, f"stats_pool_Fh{Fh}_C{C}_Tp{Tp}_nomasks", B, Fh, C, Tp, 1, Tp, kinds,
                             9500 + 16 * i + Fh + C + SEED_OFFSET, masks_null=True)


@pytest.mark.parametrize("offset", [1e2, 1e3])
def test_stats_pool_constant_offset(gpu_device, offset):
    """features = offset + 0.01 randn: a channel offset 1e4 / 1e5 times the spread.  The two-pass variance survives it
    (x - mean is exact to an ulp of x, and a shifted mean only adds its square): float32 torch stays within half the
    contract on both halves at either offset, so both are kept.  Weights of 1e-6 are left out here: with them the 1e-8 in
    v1 biases the float64 mean by 8e-5 of the offset -- as much as the spread -- and the std becomes a statement about
    that bias (float32 torch: 1.06 of the contract at offset 1e2, 10.8 at 1e3)."""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    for i, (Tp, S, C) in enumerate(((125, 3, 256), (512, 4, 320), (17, 2, 32))):
        _stats_pool_case(lib, ffi, gpu_device, f"stats_pool_offset{offset:g}_Tp{Tp}_S{S}_C{C}", 2, 10, C, Tp, S, Tp,
                         ("fractional", "binary", "ones"), 9700 + i + SEED_OFFSET, offset=offset, spread=0.01)


def test_stats_pool_refusals(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    feat = torch.randn(1, 1, 513, 32, device=gpu_device)
    masks = torch.ones(1, 5, 513, device=gpu_device)
    idx = torch.arange(513, dtype=torch.int32, device=gpu_device)
    out = Guarded(5 * 64, gpu_device)
    for what, (Tp, S) in (("T' = 513", (513, 1)), ("S = 5", (16, 5))):
        assert lib.pa_stats_pool(dptr(feat), 1, 1, Tp, 32, dptr(masks), S, Tp, dptr(idx), out.ptr, ffi.stream()) == 3, what
        assert lib.pa_last_error().decode().strip() and out.untouched(), what


def _rows_case(lib, ffi, dev, tag, B, T0, Tp, C, ld, S, Fm, ld_stats, affine, kinds, seed, masks_null=False,
               expect_nan_std=False, offset=0.0, spread=1.0, affine_values=None):
    """`offset` + `spread` randn in the matrix; `affine_values` = (scale, shift): the same for every channel, in place
    of random ones"""
    rng = torch.Generator().manual_seed(seed)
    ntiles = (B + 15) // 16
    mat = torch.full((ntiles, T0, 16, ld), float("nan"))
    mat[..., :C] = offset + spread * torch.randn(ntiles, T0, 16, C, generator=rng)
    x = mat.permute(0, 2, 1, 3).reshape(ntiles * 16, T0, ld)[:B, :Tp, :C]           # (B, Tp, C)
    scale = 0.5 + torch.rand(C, generator=rng) if affine else None
    shift = torch.randn(C, generator=rng) if affine else None
    if affine_values is not None:
        assert affine
        scale, shift = torch.full((C,), affine_values[0]), torch.full((C,), affine_values[1])
    x64, x32 = x.double(), x
    if affine:
        x64, x32 = x64 * scale.double() + shift.double(), x * scale + shift
    if affine_values is not None:
        # A shift of 1e3 on a spread of 0.01 leaves float32 a grid of 6e-5 for the shifted values.  That rounding is no
        # property of the pooling, and it is correlated with the data enough to move the std of 125 frames by 9e-4 of
        # itself: against the unrounded float64 values, float32 torch is at 0.83 of the contract.  So the truth pools, in
        # float64, the float32 values the kernel loads -- fma(x, scale, shift), rounded once (formed exactly enough in
        # float64: the product is exact there).
        x32 = (x.double() * scale.double() + shift.double()).float()
        x64 = x32.double()
    if masks_null:
        S, masks, idx = 1, None, None
        truth = torch.cat([x64.mean(1), x64.std(1, correction=1)], -1).unsqueeze(1)
        ref32 = torch.cat([x32.mean(1), x32.std(1, correction=1)], -1).unsqueeze(1)
        single = torch.zeros(B, 1, dtype=torch.bool)
    else:
        masks = torch.stack([torch.stack([_weights(rng, kinds[(b * S + s) % len(kinds)], Fm) for s in range(S)])
                             for b in range(B)])
        idx = _nearest_idx(Fm, Tp)
        w = _single_frame_rows_get_weight_one(masks, idx)[:, :, idx.long()]
        truth = _pool(x64.transpose(1, 2).unsqueeze(1), w, torch.float64)
        ref32 = _pool(x32.transpose(1, 2).unsqueeze(1), w, torch.float32)
        single = (w != 0).sum(-1) == 1
    md, idd = (masks.to(dev), idx.to(dev)) if masks is not None else (None, None)
    sd, hd = (scale.to(dev), shift.to(dev)) if affine else (None, None)
    matd = mat.to(dev)
    out = Guarded(B * S * ld_stats, dev)
    ffi.check(lib.pa_stats_pool_rows(dptr(matd), B, T0, Tp, C, ld, dptr(md), S, Fm, dptr(idd), out.ptr, ld_stats,
                                     dptr(sd), dptr(hd), ffi.stream()), tag)
    if expect_nan_std:             # a single unweighted frame: mean = x, std = NaN like torch.std(correction=1)
        written = torch.ones(B, S, ld_stats, dtype=torch.bool)
        written[..., C:2 * C] = False
        got = out.check(written, tag).view(B, S, ld_stats)
        assert torch.isnan(truth[..., C:]).all() and torch.isnan(got[..., C:2 * C]).all(), tag
        assert_parity(tag + "_mean", got[..., :C], truth[..., :C], ref32[..., :C])
        assert bool((got[..., 2 * C:] == 0).all()), tag
        return
    got = out.check(None, tag).view(B, S, ld_stats)
    assert bool((got[..., 2 * C:] == 0).all()), f"{tag}: padding columns of the statistics are not exact zeros"
    if not masks_null:
        zero = (w != 0).sum(-1) == 0          # nobody speaks: the pooled affine map is 0, not `shift`
        assert bool((got[zero][..., :2 * C] == 0).all()), tag
    _compare_rows(tag, got[..., :2 * C], truth, ref32, single)


def test_stats_pool_rows(gpu_device):
    """pa_stats_pool_rows on a (tile, t, b16)-ordered matrix: T0 > Tp, ld > C, padded statistics rows, the BatchNorm
    affine map on load, weighted and unweighted, up to the 640-frame limit"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    i = 0
    for B in (1, 17, 37):
        for C, ld in ((1500, 1504), (64, 100), (512, 516)):
            for affine in (False, True):
                Tp = (1, 37, 293, 640, 125, 16)[i % 6]
                T0 = Tp + (3, 1, 11)[i % 3]
                S = 1 + i % 4
                Fm = (Tp, 2 * Tp + 3, max(1, Tp // 3))[i % 3]
                ld_stats = 2 * C if i % 2 else (2 * C + 31) // 32 * 32 + 32
                kinds = KINDS[i % len(KINDS):] + KINDS[:i % len(KINDS)]
                _rows_case(lib, ffi, gpu_device, f"stats_pool_rows_B{B}_C{C}_Tp{Tp}_T0{T0}_S{S}_Fm{Fm}_lds{ld_stats}" +
                           ("_affine" if affine else ""), B, T0, Tp, C, ld, S, Fm, ld_stats, affine, kinds,
                           9800 + i + SEED_OFFSET)
                if i % 4 == 1:
                    _rows_case(lib, ffi, gpu_device, f"stats_pool_rows_B{B}_C{C}_Tp{Tp}_nomasks" +
                               ("_affine" if affine else ""), B, T0, max(Tp, 2), C, ld, 1, Tp, ld_stats, affine, kinds,
                               9900 + i + SEED_OFFSET, masks_null=True)
                i += 1
    # one unweighted frame: std is NaN, as torch's
    _rows_case(lib, ffi, gpu_device, "stats_pool_rows_nomasks_Tp1", 17, 4, 1, 64, 68, 1, 1, 160, True, KINDS,
               9990 + SEED_OFFSET, masks_null=True, expect_nan_std=True)
    # 640 frames are accepted (above), 641 refused
    feat = torch.randn(700 * 16, 64, device=gpu_device)
    out = Guarded(128, gpu_device)
    assert lib.pa_stats_pool_rows(dptr(feat), 1, 700, 641, 64, 64, None, 1, 641, None, out.ptr, 128, None, None,
                                  ffi.stream()) == 3
    assert lib.pa_last_error().decode().strip() and out.untouched()


@pytest.mark.parametrize("where", ["in_the_data", "in_aff_shift"])
@pytest.mark.parametrize("offset", [1e2, 1e3])
def test_stats_pool_rows_constant_offset(gpu_device, offset, where):
    """the offset cases of test_stats_pool_constant_offset for the row form, whose input has an offset by construction
    (the last BatchNorm's shift, applied on load): offset + 0.01 randn in the matrix, and randn in the matrix with
    aff_scale = 0.01 and aff_shift = offset, which is how the offset arrives in production.  125, 293 and 640 frames, 64
    channels in rows of 68, 17 chunks, ones / binary / fractional weights for every chunk (`small` left out for the
    reason given there)."""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    for i, Tp in enumerate((125, 293, 640)):
        kw = dict(offset=offset, spread=0.01) if where == "in_the_data" else dict(affine_values=(0.01, offset))
        _rows_case(lib, ffi, gpu_device, f"stats_pool_rows_offset{offset:g}_{where}_Tp{Tp}", 17, Tp + 3, Tp, 64, 68, 3, Tp,
                   160, where == "in_aff_shift", ("ones", "binary", "fractional"), 9750 + i + SEED_OFFSET, **kw)


#: running_mean (of either sign) of the last BatchNorm in test_stats_pool_rows_long_through_the_forward
LONG_SHIFT = 0.03125


def _long_pool_case(shift=LONG_SHIFT):
    """(oracle, wav (2, 1, 160000), weights (2, 3, 787): fractional | binary | ones, float64 truth, float32 oracle) of a
    seeded XVectorMFCC whose last BatchNorm has running_var = 1e-4 and running_mean = +-shift -- on the CPU"""
    import xvector_mfcc_oracle as xo
    oracle = xo.seeded_xvector_mfcc(seed=3579)
    bn = oracle.tdnns[14]
    g = torch.Generator().manual_seed(4300 + SEED_OFFSET)
    with torch.no_grad():
        sign = (torch.rand(bn.running_mean.shape, generator=g) < 0.5).float() * 2 - 1
        bn.running_mean.copy_(shift * sign)
        bn.running_var.fill_(1e-4)
    B, N, Tp = 2, 160000, 787
    wav = (0.1 * torch.randn(B, 1, N, generator=g)).clamp(-1, 1)
    w = torch.stack([torch.rand(B, Tp, generator=g), (torch.rand(B, Tp, generator=g) < 0.6).float(),
                     torch.ones(B, Tp)], dim=1)
    exact = xo.as_float64(oracle)
    with torch.inference_mode():
        want64 = torch.stack([exact(wav.double(), weights=w[:, s].double()) for s in range(3)], dim=1)
        want32 = torch.stack([oracle(wav, weights=w[:, s]) for s in range(3)], dim=1)
    return oracle, wav, w, want64, want32


def test_stats_pool_rows_long_through_the_forward(gpu_device):
    """k_stats_pool_rows_long has no entry point of its own (pa_stats_pool_rows refuses 641 frames): 787 pool frames of
    10 s chunks at hop 200 through pa_xvec_mfcc_forward, B = 2, S = 3, against the float64 oracle.  The last BatchNorm
    has running_var = 1e-4 and running_mean = +-LONG_SHIFT: its shift on load is LONG_SHIFT / sqrt(1e-4 + 1e-5), about
    95 x LONG_SHIFT, against a spread of 0.1 in the features it pools.  A running_mean of +-30 (a shift of 2860) is not
    admissible end to end: the float32 oracle is then 0.86 of the contract away from float64, 4.7 at +-10, 1.8 at +-1,
    0.68 at +-0.5, 0.34 to 0.62 at +-0.125 depending on the CPU -- the embedding layer sums 1500 means of either sign to
    outputs near zero, which no float32 Linear holds to 1e-5 -- so the shift was shrunk until the float32 oracle is
    within half the contract with room to spare (0.16): +-0.03125, a shift of 3 against a spread of 0.1.  (The large
    offsets are held by test_stats_pool_rows_constant_offset, up to 640 frames.)"""
    import xvector_mfcc_oracle as xo
    import pyannote_audio_amd as pa
    oracle, wav, w, want64, want32 = _long_pool_case()
    model = pa.XVectorMFCC(oracle.state_dict(), xo.xvector_mfcc_hparams(oracle),
                           pa.model.embedding_specifications()).to(gpu_device)
    assert model.num_frames(wav.shape[-1]) == w.shape[-1] == 787 > 640
    got = model(wav.to(gpu_device), w.to(gpu_device))
    assert got.shape == want64.shape == (2, 3, 512)
    assert_parity(f"stats_pool_rows_long_Tp787_shift{LONG_SHIFT:g}", got, want64, want32)


def _columns(n, halvings):
    w = 1 + (n - 400) // 160
    for _ in range(halvings):
        w = (w - 1) // 2 + 1
    return w


@pytest.mark.parametrize("with_masks", [False, True])
def test_stats_pool_ragged(gpu_device, with_masks):
    """pa_stats_pool_ragged: utterances of one column (400 samples), a few seconds, and widths of 600 and 1025 columns
    after three halvings (two and three 512-column LDS tiles); every utterance equals the pooling of its own valid columns;
    NaN behind them in the features (and in the masks) never reaches the output"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    rng = torch.Generator().manual_seed(10100 + SEED_OFFSET)
    lengths = [400, 48000, 400 + 160 * 8 * 599 + 77, 84321, 400 + 160 * 8 * 1024, 23456, 400 + 160 * 8 * 512]
    widths = [_columns(n, 3) for n in lengths]
    assert widths[0] == 1 and widths[2] == 600 and widths[4] == 1025 and widths[6] == 513
    B, Fh, C, W = len(lengths), 3, 300, max(widths)
    feat = torch.full((B, Fh, W, C), float("nan"))
    ld_masks = W + 5
    masks = torch.full((B, ld_masks), float("nan")) if with_masks else None
    kinds = ("binary", "fractional", "binary", "zero", "fractional", "one_frame", "small")
    truth, ref32, single = [], [], []
    for b, wv in enumerate(widths):
        feat[b, :, :wv] = torch.randn(Fh, wv, C, generator=rng)
        w = _weights(rng, kinds[b], wv) if with_masks else torch.ones(wv)
        if (w != 0).sum() == 1:
            w = (w != 0).float()          # (the input rule of _single_frame_rows_get_weight_one)
        if with_masks:
            masks[b, :wv] = w
        seq = feat[b, :, :wv].permute(2, 0, 1).reshape(C * Fh, wv)
        truth.append(_pool(seq, w, torch.float64))
        ref32.append(_pool(seq, w, torch.float32))
        single.append(bool((w != 0).sum() == 1))
    fd, ld = feat.to(gpu_device), torch.tensor(lengths, dtype=torch.int32, device=gpu_device)
    md = masks.to(gpu_device) if with_masks else None
    out = Guarded(B * 2 * C * Fh, gpu_device)
    tag = "stats_pool_ragged_" + ("masks" if with_masks else "nomasks")
    ffi.check(lib.pa_stats_pool_ragged(dptr(fd), B, Fh, W, C, dptr(ld), 3, dptr(md), ld_masks if with_masks else 0,
                                       out.ptr, ffi.stream()), tag)
    got = out.check(None, tag).view(B, 2 * C * Fh)
    _compare_rows(tag, got, torch.stack(truth), torch.stack(ref32), torch.tensor(single))


def test_stats_pool_ragged_constant_offset(gpu_device):
    """pa_stats_pool_ragged has no limit on the width: features = 1e3 + 0.01 randn over 600 and 1025 valid columns (two
    and three LDS tiles), fractional and binary weights; admissibility is ruled per utterance"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    rng = torch.Generator().manual_seed(10150 + SEED_OFFSET)
    cases = [(400 + 160 * 8 * 599 + 77, "fractional"), (400 + 160 * 8 * 1024, "fractional"),
             (400 + 160 * 8 * 599 + 77, "binary"), (400 + 160 * 8 * 1024, "binary")]
    widths = [_columns(n, 3) for n, _ in cases]
    assert widths == [600, 1025, 600, 1025]
    B, Fh, C, W = len(cases), 3, 64, max(widths)
    feat = torch.full((B, Fh, W, C), float("nan"))
    ld_masks = W + 5
    masks = torch.full((B, ld_masks), float("nan"))
    truth, ref32 = [], []
    for b, (wv, (_, kind)) in enumerate(zip(widths, cases)):
        feat[b, :, :wv] = 1e3 + 0.01 * torch.randn(Fh, wv, C, generator=rng)
        w = _weights(rng, kind, wv)
        masks[b, :wv] = w
        seq = feat[b, :, :wv].permute(2, 0, 1).reshape(C * Fh, wv)
        truth.append(_pool(seq, w, torch.float64))
        ref32.append(_pool(seq, w, torch.float32))
    fd, md = feat.to(gpu_device), masks.to(gpu_device)
    ld = torch.tensor([n for n, _ in cases], dtype=torch.int32, device=gpu_device)
    out = Guarded(B * 2 * C * Fh, gpu_device)
    ffi.check(lib.pa_stats_pool_ragged(dptr(fd), B, Fh, W, C, dptr(ld), 3, dptr(md), ld_masks, out.ptr, ffi.stream()),
              "stats_pool_ragged_offset")
    got = out.check(None, "stats_pool_ragged_offset").view(B, 2 * C * Fh)
    for b, (wv, (_, kind)) in enumerate(zip(widths, cases)):
        assert_parity(f"stats_pool_ragged_offset1000_W{wv}_{kind}", got[b], truth[b], ref32[b])


@pytest.mark.parametrize("C", [4, 32, 256])
def test_zero_tail_cols(gpu_device, C):
    """pa_zero_tail_cols: columns behind an utterance's valid width become exact zeros, everything else keeps its bits"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    rng = torch.Generator().manual_seed(10200 + C + SEED_OFFSET)
    lengths = [400, 16000, 5000, 31999, 32000, 719]
    for halvings in range(4):
        widths = [_columns(n, halvings) for n in lengths]
        B, H, W = len(lengths), (5, 3, 2, 1)[halvings], max(widths)
        x = torch.randn(B, H, W, C, generator=rng)
        buf = Guarded(x.numel(), gpu_device)
        buf.buf[GUARD:GUARD + x.numel()] = x.view(-1).to(gpu_device)
        ld = torch.tensor(lengths, dtype=torch.int32, device=gpu_device)
        ffi.check(lib.pa_zero_tail_cols(buf.ptr, B, H, W, C, dptr(ld), halvings, ffi.stream()), "zero_tail")
        got = buf.check(None, f"zero_tail C{C} halvings {halvings}").view(B, H, W, C)
        for b, wv in enumerate(widths):
            assert torch.equal(got[b, :, :wv], x[b, :, :wv]), (C, halvings, b)
            assert bool((got[b, :, wv:] == 0).all()) and not torch.signbit(got[b, :, wv:]).any(), (C, halvings, b)


def test_fbank_ragged(gpu_device):
    """pa_fbank_ragged: every utterance against the float64 kaldi fbank of the oracle (energy domain, the bound of
    test_fuzz_fbank_lengths), each centred on its own mean; frames behind an utterance's own count are exact zeros"""
    import pyannote_audio_amd.ffi as ffi
    from oracle import seeded_wespeaker
    from pyannote_audio_amd.weights import EmbeddingPack
    lib = ffi.load()
    model = seeded_wespeaker(seed=4321)
    pack = EmbeddingPack(model.state_dict(), gpu_device, guard=False)
    w = pack.struct
    rng = torch.Generator().manual_seed(10300 + SEED_OFFSET)
    lengths = [400, 561, 4800, 16000, 23456, 719, 48001]
    gap = 37                                           # samples between utterances that belong to nobody
    offsets, pieces, pos = [], [], 0
    for n in lengths:
        offsets.append(pos)
        pieces.append((0.1 * torch.randn(n + gap, generator=rng)).clamp(-1, 1))
        pos += n + gap
    wav = torch.cat(pieces)
    B, nmax = len(lengths), max(lengths)
    T = lib.pa_emb_num_fbank_frames(nmax)
    wd = wav.to(gpu_device)
    od = torch.tensor(offsets, dtype=torch.int64, device=gpu_device)
    ld = torch.tensor(lengths, dtype=torch.int32, device=gpu_device)
    out = Guarded(B * T * 80, gpu_device)
    ffi.check(lib.pa_fbank_ragged(dptr(wd), wd.numel(), dptr(od), dptr(ld), B, nmax, w.fb_window, w.fb_tw256, w.fb_tw512,
                                  w.fb_mel_w, w.fb_mel_lo, w.fb_mel_hi, 80, out.ptr, ffi.stream()), "fbank_ragged")
    got = out.check(None, "fbank_ragged").view(B, T, 80)
    for b, n in enumerate(lengths):
        x = wav[offsets[b]:offsets[b] + n].view(1, 1, n)
        with torch.inference_mode():
            ref = model.compute_fbank(x)
            ref64 = model.double().compute_fbank(x.double())
            model.float()
        Tb = ref.shape[1]
        assert Tb == 1 + (n - 400) // 160
        assert bool((got[b, Tb:] == 0).all()), n
        e64 = torch.exp(ref64)
        scale = torch.maximum(e64, 1e-3 * e64.amax(dim=(1, 2), keepdim=True))
        rel = ((torch.exp(got[b:b + 1, :Tb].double()) - e64).abs() / scale).max().item()
        rel_oracle = ((torch.exp(ref.double()) - e64).abs() / scale).max().item()
        print(f"fbank_ragged_N{n}: energy-domain error {rel:.3e}, float32 oracle {rel_oracle:.3e}")
        assert rel < max(2e-4, 2.0 * rel_oracle) and rel < 4e-4, (n, rel, rel_oracle)


@pytest.mark.parametrize("Fbins", [80, 8])
@pytest.mark.parametrize("B", [1, 5])
def test_resnet_stem(gpu_device, Fbins, B):
    """pa_resnet_stem against float64 conv2d(1 -> 32, 3x3, padding 1) + shift + ReLU, NHWC output inside guards"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    rng = torch.Generator().manual_seed(10400 + Fbins + B + SEED_OFFSET)
    wt = torch.randn(32, 1, 3, 3, generator=rng) / 3           # [c][0][dmel][dtime]
    shift = torch.randn(32, generator=rng)
    w9 = wt[:, 0].permute(1, 2, 0).reshape(9, 32).contiguous().to(gpu_device)       # tap = 3 dmel + dtime
    sd = shift.to(gpu_device)
    for T in (1, 2, 3, 7, 298, 998):
        fb = 3.0 * torch.randn(B, T, Fbins, generator=rng)
        x = fb.permute(0, 2, 1).unsqueeze(1)                    # (B, 1, F, T)
        truth = F.relu(F.conv2d(x.double(), wt.double(), padding=1) + shift.double().view(1, -1, 1, 1))
        ref32 = F.relu(F.conv2d(x, wt, padding=1) + shift.view(1, -1, 1, 1))
        fd = fb.to(gpu_device)
        out = Guarded(B * Fbins * T * 32, gpu_device)
        ffi.check(lib.pa_resnet_stem(dptr(fd), B, T, Fbins, dptr(w9), dptr(sd), out.ptr, ffi.stream()), "stem")
        got = out.check(None, f"stem T{T}").view(B, Fbins, T, 32).permute(0, 3, 1, 2)
        assert_parity(f"resnet_stem_B{B}_F{Fbins}_T{T}", got, truth, ref32)
        assert ratio(got, truth) <= 1.0
