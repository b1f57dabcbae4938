"""Everything of tests/test_conv_kernels_gpu.py that can be pinned without a GPU (tests/conv_truth.py): the case list
reaches every instantiation the three launchers can pick -- with and without a residual, with ReLU on and off -- and
every case takes the instantiation it claims; no float64 truth costs more than 2e9 multiply-adds; every float case is
admissible (float32 torch within half the contract of the float64 truth, exactly what kernel_parity.assert_parity demands
before it looks at a kernel); the integer weight images are integral; every exact case stays below 2^24 in every
intermediate and its float32 host replay equals the integer truth bit for bit; the vectorised F(4x4) replay is the loop
of tests/test_winograd4_cpu.py.  Nothing here says anything about a kernel."""
import numpy as np
import pytest
import torch

import conv_truth as T
from kernel_parity import SEED_OFFSET, ratio

HALF = 0.5
_ids = dict(ids=lambda c: c["name"])


def float_seed(case):
    return T.float_seed(case, SEED_OFFSET)


def exact_seed(case, variant):
    return T.exact_seed(case, variant, SEED_OFFSET)


# ---------------------------------------------------------------------------------------------------------------------
# dispatch coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_every_case_takes_the_instantiation_it_claims():
    for c in T.FLOAT_CASES:
        assert T.instantiation(c) == c["claims"], (c["name"], T.instantiation(c))
        lo, hi = T.written_rows(c)
        assert 0 <= lo < hi <= T.out_hw(c["H"], c["W"], c["stride"])[0], c["name"]
        if c["algo"] == "wino":
            assert c["y_first"] % 2 == 0 and c["cin"] % 16 == 0 and c["cout"] % 32 == 0 and c["stride"] == 1
        elif c["algo"] == "wino4":
            assert c["rows"] == c["H"] or (c["rows"] < c["H"] and c["rows"] % 4 == 0)
            assert c["cin"] % 8 == 0 and c["cin"] >= 32 and c["cout"] % 32 == 0 and c["stride"] == 1
        else:
            assert c["cin"] % 16 == 0 and c["cout"] % (32 if c["stride"] == 1 else 64) == 0
            # 64-channel tiles write whole tiles only
            assert c["claims"][3] == 32 or c["cout"] % 64 == 0


@pytest.mark.parametrize("algo,instantiations", [("direct", T.DIRECT_INSTANTIATIONS), ("wino", T.WINO_INSTANTIATIONS),
                                                 ("wino4", T.WINO4_MODES)])
def test_every_instantiation_is_reached(algo, instantiations):
    """... with and without a residual (a template parameter of every kernel), with ReLU on and off, and once by a
    launch in which every claimer of tiles gets at least two (>= 2 x the compute units, as the issue asks; in fact
    2 x the workgroups -- or halves -- that claim tiles)"""
    cases = [c for c in T.CASES if c["algo"] == algo]
    assert {c["claims"] for c in cases} == set(instantiations)
    for inst in instantiations:
        mine = [c for c in cases if c["claims"] == inst]
        variants = {v for c in mine for v in c["variants"]}
        assert {res for res, _ in variants} == {True, False}, inst
        assert {relu for _, relu in variants} == {True, False}, inst
        assert {(res, relu) for res, relu in variants} == {(True, True), (True, False), (False, True), (False, False)}
        many = [c for c in mine if c["many"]]
        assert many, inst
        for c in many:
            assert T.workgroup_tiles(c) >= 2 * T.CLAIMERS[algo] >= 2 * T.CUS, (c["name"], T.workgroup_tiles(c))
            assert c["cin"] == (32 if algo == "wino4" or inst == "wino32" else 16)        # the smallest accepted
        assert any(not c["many"] and T.workgroup_tiles(c) > 1 for c in mine), inst       # more than one block


def test_the_forms_only_a_row_range_or_a_tile_order_reaches():
    wino = [c for c in T.CASES if c["algo"] == "wino"]
    assert {c["claims"] for c in wino if c["y_first"] > 0} == {(4, 1), (2, 2), (1, 4)}
    assert {(c["H"], c["y_first"]) for c in wino if c["y_first"] > 0} == {(10, 8), (6, 4), (7, 4)}
    # 32 -> 32 with y_first > 0 is NOT the two-halves kernel
    assert any(c["cin"] == c["cout"] == 32 and c["y_first"] > 0 and c["claims"] == (4, 1) for c in wino)
    f4 = [c for c in T.CASES if c["algo"] == "wino4"]
    assert {(c["H"], c["rows"]) for c in f4 if c["rows"] < c["H"]} >= {(6, 4), (10, 8)}
    assert any(c["cin"] == 40 for c in f4 if c["rows"] < c["H"]) and any(c["cin"] == 40 for c in f4 if c["rows"] == c["H"])
    for mode in T.WINO4_MODES:            # both tile orders: cout < 256 and cout == 256
        assert {T.xcd_ranges(c) for c in f4 if c["claims"] == mode} == {True, False}, mode
    # units of 16 tiles that straddle images, a map smaller than one unit, several runs per unit
    assert any(c["claims"] == 1 and 1 < T.cdiv(c["H"], 4) * T.cdiv(c["W"], 4) < 16 and c["B"] > 1 for c in f4)
    assert any(c["claims"] == 1 and c["H"] <= 4 and c["W"] <= 4 for c in f4)
    assert any(c["claims"] == 2 and 5 <= T.cdiv(c["W"], 4) < 16 for c in f4)
    # the issue's own examples, verified rather than trusted: 5 x 129 with one image is run-shaped, not row-shaped
    assert T.wino4_mode(1, 4, 128, 4) == 0 and T.wino4_mode(1, 5, 129, 5) == 2 and T.wino4_mode(1, 5, 125, 5) == 0
    assert T.wino4_mode(8, 8, 12, 8) == 1 and T.wino4_mode(37, 3, 3, 3) == 1
    assert T.wino4_mode(8, 8, 20, 8) == 2 and T.wino4_mode(9, 7, 22, 7) == 2
    # ragged edges: a map that is no multiple of the tile in either direction, for every kernel family
    for algo in ("direct", "wino", "wino4"):
        assert any(c["H"] % 2 and c["W"] % 2 for c in T.CASES if c["algo"] == algo)
    names = [c["name"] for c in T.FLOAT_CASES]
    assert len(set(names)) == len(names)
    assert {c["family"] for c in T.CASES} == set(T.FAMILIES)
    for algo in ("direct", "wino", "wino4"):
        assert {c["family"] for c in T.FAMILY_CASES if c["algo"] == algo} == set(T.FAMILIES)


def test_no_truth_costs_more_than_the_cap():
    for c in T.FLOAT_CASES:
        assert T.cost(c) <= T.COST_CAP, (c["name"], T.cost(c))


# ---------------------------------------------------------------------------------------------------------------------
# admissibility of the float cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.FLOAT_CASES, **_ids)
def test_float_cases_are_admissible(case):
    x, w, shift, R = T.float_inputs(case, float_seed(case))
    c64, c32 = T.conv_of(x, w, case["stride"], torch.float64), T.conv_of(x, w, case["stride"], torch.float32)
    for use_res, relu in case["variants"]:
        r = ratio(T.finish(c32, shift, R, use_res, relu), T.finish(c64, shift, R, use_res, relu))
        print(f"{case['name']} res={use_res} relu={relu}: float32 torch {r:.3f} of the contract")
        assert r <= HALF, f"{case['name']}: inadmissible case -- float32 torch is {r:.3f} of the contract from float64"
    if case["family"] != "randn":
        assert float(x.min()) >= 0.0
    if case["family"] == "relu+2":
        assert float(x.mean()) > 2.0


# ---------------------------------------------------------------------------------------------------------------------
# the host replays
# ---------------------------------------------------------------------------------------------------------------------
def test_recipes_are_those_of_test_winograd4_cpu():
    import test_winograd4_cpu as ref
    g = torch.Generator().manual_seed(5 + SEED_OFFSET)
    x = torch.randn(6, 7, 3, generator=g)
    assert np.array_equal(torch.stack(T.bt4(x.unbind(0))).numpy(), ref.bt(x.numpy()))
    assert np.array_equal(torch.stack(T.at4(x.unbind(0))).numpy(), ref.at(x.numpy()))


def test_unpackers_invert_the_packers():
    from pyannote_audio_amd.weights import winograd4_pack, winograd_pack
    U4 = torch.arange(36 * 64 * 40, dtype=torch.float32).reshape(36, 64, 40)
    assert torch.equal(T.wino4_unpack(winograd4_pack(U4)), U4)
    U2 = torch.arange(16 * 64 * 48, dtype=torch.float32).reshape(16, 64, 48)
    assert torch.equal(T.wino2_unpack(winograd_pack(U2)), U2)


def test_vectorised_f4_replay_is_the_loop_of_test_winograd4_cpu():
    """one small case (two images, ragged map, cin % 8 == 0 but not % 16, two cout slices), bit for bit against the loop
    of test_winograd4_cpu.test_kernel_arithmetic_replayed_on_the_host: its bt / at, its slab addresses and quad swap,
    its point order.  The 8-channel product `u @ v` of that loop is spelled out here channel by channel (a BLAS may sum
    the eight products in any order; the replay fixes one: ascending)."""
    import test_winograd4_cpu as ref
    from pyannote_audio_amd.weights import winograd4_pack, winograd4_weights
    B, H, W, cin, cout = 2, 5, 7, 40, 64
    g = torch.Generator().manual_seed(35 + SEED_OFFSET)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    packed = winograd4_pack(winograd4_weights(w))
    slabs = packed.numpy()
    th, tw = -(-H // 4), -(-W // 4)
    out = np.zeros((B, cout, 4 * th, 4 * tw), dtype=np.float32)
    for b in range(B):
        xp = np.zeros((cin, 4 * th + 2, 4 * tw + 2), dtype=np.float32)
        xp[:, 1:H + 1, 1:W + 1] = x[b].numpy()
        for ty in range(th):
            for tx in range(tw):
                d = xp[:, 4 * ty:4 * ty + 6, 4 * tx:4 * tx + 6]
                tt = ref.bt(d.transpose(1, 2, 0))
                v = ref.bt(tt.transpose(1, 0, 2)).transpose(1, 0, 2)
                M = np.zeros((36, cout), dtype=np.float32)
                for xi in range(36):
                    for ns in range(cout // 32):
                        for st in range(cin // 8):
                            u = slabs[ns, st, 32 * xi:32 * xi + 32, :].copy()
                            sw = ((np.arange(32) >> 3) & 1).astype(bool)
                            u[sw] = np.concatenate([u[sw, 4:], u[sw, :4]], axis=1)
                            for k in range(8):
                                M[xi, 32 * ns:32 * ns + 32] += u[:, k] * v[xi // 6, xi % 6, 8 * st + k]
                z = ref.at(M.reshape(6, 6, cout))
                y = ref.at(z.transpose(1, 0, 2))
                out[b, :, 4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4] = y.transpose(2, 1, 0)
    got = T.wino4_replay(x, packed)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), out[:, :, :H, :W])
    # and it is a convolution: the bound of that test, against float64
    truth = T.conv_of(x, w, 1, torch.float64)
    assert float((got.double() - truth).abs().max()) <= 1e-4 * float(truth.abs().max())


def test_f2_replay_is_a_convolution():
    from pyannote_audio_amd.weights import winograd_pack, winograd_weights
    g = torch.Generator().manual_seed(36 + SEED_OFFSET)
    x = torch.randn(2, 32, 5, 7, generator=g)
    w = torch.randn(64, 32, 3, 3, generator=g) / (3 * 32 ** 0.5)
    got = T.wino2_replay(x, winograd_pack(winograd_weights(w)))
    assert ratio(got, T.conv_of(x, w, 1, torch.float64)) <= 1.0


@pytest.mark.parametrize("case", [c for c in T.FAMILY_CASES if c["algo"] == "wino4"], **_ids)
def test_f4_replay_on_network_statistics(case):
    """what the F(4x4) bound of the GPU test rests on: the replay is a convolution by the project's per-convolution
    bound on every family, while its element-wise ratio leaves the contract on some (printed; the issue: 5.8 on
    `cout-scale` at 256 channels) -- which is why the kernel is held to 2 x the replay and not to a constant"""
    from pyannote_audio_amd.weights import winograd4_pack, winograd4_weights
    x, w, shift, R = T.float_inputs(case, float_seed(case))
    truth = T.finish(T.conv_of(x, w, 1, torch.float64), shift, R, True, False)
    rep = T.finish(T.wino4_replay(x, winograd4_pack(winograd4_weights(w))), shift, R, True, False)
    print(f"{case['name']}: replay {ratio(rep, truth):.3f} of the contract")
    assert float((rep.double() - truth).abs().max()) <= 1e-4 * float(truth.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------------
def test_integer_weight_images_are_integral():
    from pyannote_audio_amd.weights import winograd4_weights, winograd_weights
    for variant, (_, _, nz, k) in enumerate(T.EXACT_VARIANTS["wino"]):
        case = dict(B=1, H=7, W=10, cin=64, cout=128, stride=1, algo="wino")
        _, w, _, _ = T.exact_inputs(case, 77 + variant + SEED_OFFSET, variant)
        assert bool((w == w.round()).all()) and float(w.abs().max()) == k
        assert bool(((w != 0).flatten(2).any(-1).sum(1) <= nz).all())             # nz input channels per output channel
        U2 = winograd_weights(4 * w)
        assert bool((U2 == U2.round()).all()) and float(U2.abs().max()) > 0      # G is dyadic: 4 w clears its halves
        # the image in closed form: 4 G w G^T = (2 G) w (2 G)^T
        G2 = torch.tensor([[2, 0, 0], [1, 1, 1], [1, -1, 1], [0, 0, 2]], dtype=torch.int64)
        want = torch.einsum("ap,oipq,bq->aboi", G2, w.to(torch.int64), G2).reshape(16, 128, 64)
        assert torch.equal(U2, want.float())
        U4 = T.wino4_int_image(w)
        assert U4.dtype == torch.int64 and int(U4.abs().max()) < T.EXACT_LIMIT
        # weights.winograd4_weights reaches the same image only up to the float32 rounding of its float64 residues
        # (1/6 and 1/24 are not dyadic: 1e-13 where the exact entry is 0)
        V = winograd4_weights(576 * w)
        assert bool(((V - U4.float()).abs() <= 1.2e-7 * U4.float().abs() + 1e-9).all())


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("case", T.EXACT_CASES, **_ids)
def test_exact_cases_are_exact(case, variant):
    """the proof each exact case carries: the largest magnitude any float32 intermediate can take is below 2^24, and the
    float32 host replay of the algorithm, from the image the kernel is given, IS the integer truth"""
    x, w, shift, R = T.exact_inputs(case, exact_seed(case, variant), variant)
    stages = T.exact_proof(case, x, w, shift, R)
    print(f"{case['name']} v{variant}: {stages}")
    assert max(stages.values()) < T.EXACT_LIMIT, stages
    U, packed = T.exact_image(case, w)
    assert bool((U == U.round()).all())
    use_res, relu = case["variants"][variant]
    truth = T.exact_truth(case, x, w, shift, R, use_res, relu)
    assert torch.equal(T.exact_replay(case, x, packed, shift, R, use_res, relu), truth)
    assert float(truth.abs().max()) > 0


def test_the_issues_table_of_exact_cases():
    """(cin, cout, nz, |x|, k) of the issue on a 7 x 10 map: sum |U| |V| of F(4x4) stays below 2^24 (the issue measured
    5.8e5, 7.5e5, 3.1e6, 5.5e6) and the replay is the truth.  The inverse transform bounded with absolute values is NOT
    below 2^24 for the larger two -- which is why EXACT_VARIANTS takes fewer and smaller taps for F(4x4)."""
    from pyannote_audio_amd.weights import winograd4_pack
    for cin, cout, nz, xmax, k in ((32, 32, 4, 4, 2), (256, 256, 4, 4, 2), (256, 256, 8, 8, 3), (64, 128, 16, 8, 3)):
        c = dict(B=1, H=7, W=10, stride=1, algo="wino4", cin=cin, cout=cout)
        x, w, shift, R = T.exact_inputs(c, 88 + SEED_OFFSET, (-xmax, xmax, nz, k))
        stages = T.exact_proof(c, x, w, shift, R)
        print(cin, cout, nz, xmax, k, stages)
        assert stages["accumulate"] < T.EXACT_LIMIT
        assert (stages["inverse"] < T.EXACT_LIMIT) == (xmax == 4)
        got = T.finish(T.wino4_replay(x, winograd4_pack(T.wino4_int_image(w).float())), shift, R, True, False)
        assert torch.equal(got, T.exact_truth(c, x, w, shift, R, True, False))


@pytest.mark.parametrize("name", ["direct_32to64_31x9_B2_s2", "wino_32to64_7x33_B2", "wino4_40to32_5x9_B5"])
def test_a_wrong_image_entry_changes_an_exact_case(name):
    """what the exact cases are for, shown on the host replay: one entry of the weight image dropped (a tap of the direct
    kernel, a transform-domain weight of the others) or doubled moves some output by at least 1, and the comparison is
    torch.equal.  (An entry off by ONE ULP is a non-integer product that a large partial sum can round away: 103 of 120
    such images differed from the truth in the F(4x4) replay of this case.)"""
    case = next(c for c in T.CASES if c["name"] == name)
    x, w, shift, R = T.exact_inputs(case, exact_seed(case, 0), 0)
    U, _ = T.exact_image(case, w)
    truth = T.exact_truth(case, x, w, shift, R, True, False)
    from pyannote_audio_amd.weights import winograd4_pack, winograd_pack
    pack = {"direct": lambda u: u, "wino": winograd_pack, "wino4": winograd4_pack}[case["algo"]]
    assert torch.equal(T.exact_replay(case, x, pack(U), shift, R, True, False), truth)
    entries = (U != 0).nonzero()
    g = torch.Generator().manual_seed(3 + SEED_OFFSET)
    for i in torch.randperm(len(entries), generator=g)[:6].tolist():
        for factor in (0.0, 2.0):
            wrong = U.clone()
            wrong[tuple(entries[i].tolist())] *= factor
            got = T.exact_replay(case, x, pack(wrong), shift, R, True, False)
            assert float((got - truth).abs().max()) >= 1.0, (entries[i].tolist(), factor)
