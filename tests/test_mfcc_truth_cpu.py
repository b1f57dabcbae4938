"""tests/mfcc_truth.py on the CPU: the truth equals the float64 oracle, every (configuration, signal) pair in use is
admissible (the float32 oracle within half the tolerance, decided before any kernel output exists), every signal and
configuration is what it claims to be, the square DCT tables invert, and the tolerance sees a band that is wrong by
1 dB."""
import numpy as np
import pytest
import torch

import fbank_truth as ft
import mfcc_truth as mt


def _chunk(case, b):
    return ft.chunk_of(case["data"], b, case["N"], case["stride"], case["wav_len"])


@pytest.mark.parametrize("config", list(mt.CONFIGS))
def test_truth_equals_the_float64_oracle(config):
    """the oracle in float64 with the pack's tables against the truth written out in mfcc_truth.py: the same numbers up
    to float64 rounding, on a signal with floor cells and silent frames"""
    for name in ("harmonic_envelope", "tone_440_m30dB", "zeros_then_loud"):
        case = mt.layout_case(config, name)
        for b, ch in enumerate(case["chunks"]):
            want = mt.oracle(config, _chunk(case, b), torch.float64).numpy()
            assert want.shape == ch["c"].shape == (mt.num_frames(config, case["N"]), mt.tables(config)["cfg"]["n_mfcc"])
            assert np.abs(want - ch["c"]).max() <= 1e-7, (config, name, b)


@pytest.mark.parametrize("config", list(mt.CONFIGS))
def test_every_pair_in_use_is_admissible(config):
    assert mt.PAIRS[config], f"{config}: no admissible signal"
    for name in mt.PAIRS[config]:
        case = mt.layout_case(config, name)
        assert case["wav_len"] < (case["B"] - 1) * case["stride"] + case["N"]
        assert case["wav_len"] > (case["B"] - 1) * case["stride"] + mt.PAD        # the last chunk reflects zeros
        worst = max(ch["r_oracle"] for ch in case["chunks"])
        print(f"mfcc_truth {config} {name}: float32 oracle {worst:.3f}")
        assert worst <= 0.5, f"{config} {name}: inadmissible -- the float32 oracle is at {worst:.3f} of the tolerance"


def test_every_configuration_is_covered():
    assert set(mt.PAIRS) == set(mt.CONFIGS) and not mt.EXCLUDED
    for config in mt.CONFIGS:
        assert set(mt.PAIRS[config]) | {s for c, s in mt.EXCLUDED if c == config} == set(mt.SIGNALS)


@pytest.mark.parametrize("config", list(mt.EDGE_LENGTHS))
def test_edge_cases_are_admissible(config):
    for name in mt.EDGE_SIGNALS:
        for n in mt.EDGE_LENGTHS[config]:
            assert mt.num_frames(config, n) >= 1
            for ch in mt.edge_case(config, name, n)["chunks"]:
                assert ch["r_oracle"] <= 0.5, (config, name, n, ch["r_oracle"])


def test_edge_lengths_are_the_edges():
    for config, lengths in mt.EDGE_LENGTHS.items():
        cfg = mt.tables(config)["cfg"]
        hop = cfg["hop_length"]
        if cfg["center"]:
            want = {201, 202, 399, 400, 401, hop - 1, hop, hop + 1, 16 * hop - 1, 16 * hop + 1}
            assert set(lengths) == {n for n in want if n > mt.PAD}, config
        else:
            assert set(lengths) == {400, 401, 400 + hop - 1, 400 + hop}, config
    hops = {mt.tables(c)["cfg"]["hop_length"] for c in mt.EDGE_LENGTHS if mt.tables(c)["cfg"]["center"]}
    assert any(h - 1 > mt.PAD for h in hops)                    # hop - 1, hop, hop + 1 all exist for one of them


def test_configurations_are_what_they_claim():
    for config in mt.CONFIGS:
        tb = mt.tables(config)
        fb = tb["fb"]
        assert fb.shape == (mt.NBIN, tb["cfg"]["n_mels"]) and (fb >= 0).all()
    empty = {c: int((mt.tables(c)["fb"].sum(axis=0) == 0).sum()) for c in mt.CONFIGS}
    assert empty["m256_c64"] >= 8 and empty["m256_c64"] > 2 * empty["default"] > 0      # many empty filters
    assert empty["m23_c13"] == 0 and empty["m40_c40"] == 0
    narrow = mt.tables("band_300_3400")["fb"]
    assert (narrow[:7] == 0).all() and (narrow[86:] == 0).all()               # 40 Hz bins: below 280 Hz, above 3440 Hz
    assert not np.array_equal(mt.tables("slaney")["fb"], mt.tables("default")["fb"])
    assert np.allclose(mt.tables("dct_none")["D"][:, 0], 2.0)
    assert mt.tables("log_mels")["cfg"]["log_mels"] and not mt.tables("default")["cfg"]["log_mels"]
    assert [mt.tables(c)["cfg"]["hop_length"] for c in ("hop1", "hop399", "hop400")] == [1, 399, 400]
    assert not mt.tables("m64_c64_hop160_uncentred")["cfg"]["center"]


def test_signals_are_what_they_claim():
    d = {name: mt.layout_case("default", name)["chunks"] for name in mt.SIGNALS}
    tone = d["tone_440_m30dB"][0]
    assert tone["on_floor"].mean() >= 0.25, "at least a quarter of the cells of the tone sit on the top_db floor"
    assert any((ch["E"] <= 1e-10).all(axis=1).any() for ch in d["silence_burst"]), "frames wholly at 1e-10"
    assert any((ch["E"] <= 1e-10).all(axis=1).any() and ch["E"].max() > 1.0 for ch in d["harmonic_envelope"])
    assert (d["zeros_then_loud"][0]["E"] == 0).all() and (d["zeros_then_loud"][0]["P"] == 0).all()
    assert d["zeros_then_loud"][2]["E"].max() > 1e3 * 1e-10 and d["zeros_then_loud"][2]["E"].max() > 1.0
    assert all(np.isfinite(ch["c"]).all() for chunks in d.values() for ch in chunks)
    # the chunk's loudest cell -- the one that sets the floor -- is in frame 0, whose first half is reflected padding
    first = d["loud_in_reflection"][0]
    assert np.unravel_index(np.argmax(first["v"]), first["v"].shape)[0] == 0
    assert first["E"][0].max() > 2.0 * first["E"][1:].max()          # the burst is in its window twice
    # the last chunk of every signal ends in zeros that the reflection mirrors: its last frame is silent
    for name, chunks in d.items():
        assert (chunks[-1]["P"][-1] == 0).all(), name
    # a quiet band beside a loud one, in the same frame: speech and the harmonic stack have cells 50 dB below the
    # loudest cell of their own frame that are above the floor; the bin-centred tone has nine cells in ten on the floor
    for name in ("speech", "harmonic_envelope"):
        for ch in d[name]:
            assert ((ch["v"] < ch["v"].max(axis=1, keepdims=True) - 50.0) & ~ch["on_floor"]).sum() >= 100, name
    assert d["tone_bin"][0]["on_floor"].mean() >= 0.9


@pytest.mark.parametrize("config", mt.SQUARE)
def test_square_dct_inverts(config):
    tb = mt.tables(config)
    D, n = tb["D"], tb["D"].shape[0]
    assert D.shape == (n, n) and tb["cfg"]["dct_norm"] == "ortho"
    # orthonormal up to the float32 rounding of the table.  create_dct forms the angle pi / n (m + 0.5) k in float32:
    # three roundings, 1.5 eps32 of an angle of up to pi n, which cos passes on at most one to one; every entry of D is
    # sqrt(2 / n) cos at the most, so |dD| <= 1.5 pi n eps32 sqrt(2 / n), and an entry of D D^T, a sum of n products, is
    # off by 2 n sqrt(2 / n) |dD| = 6 pi n eps32.  (That is why mfcc_truth carries coefficients back with the inverse of
    # the table as it is, not with its transpose.)
    assert np.abs(D @ D.T - np.eye(n)).max() <= 6.0 * np.pi * n * mt.EPS32
    assert np.abs(D @ tb["Dinv"] - np.eye(n)).max() <= 1e-12
    case = mt.layout_case(config, "speech")
    for ch in case["chunks"]:
        assert np.abs(ch["c"] @ tb["Dinv"] - ch["v"]).max() <= 1e-9


@pytest.mark.parametrize("config", ["default", "m40_c40", "m256_c64", "log_mels"])
def test_one_band_wrong_by_1_dB_is_seen(config):
    """what the peak-relative bound could not see: ONE mel cell of a quiet band, wrong by 1 dB (26 % in energy), moves
    the ratio far above 1 -- in every frame and band tried"""
    case = mt.layout_case(config, "speech")
    tb, ch = mt.tables(config), case["chunks"][0]
    step = 1.0 if not tb["cfg"]["log_mels"] else np.log(10.0) / 10.0
    rng = np.random.default_rng(0)
    for _ in range(50):
        t, m = int(rng.integers(ch["v"].shape[0])), int(rng.integers(ch["v"].shape[1]))
        if tb["fb"][:, m].sum() == 0:
            continue                                              # an empty filter holds no energy to get wrong
        v = ch["v"].copy()
        v[t, m] += step
        assert mt.ratio(config, v @ tb["D"], ch) > 3.0, (config, t, m)
