"""What tests/test_fbank_kernel_gpu.py rests on, checked without a GPU (tests/fbank_truth.py): the float64 truth against
the oracle's kaldi fbank, the admissibility of every signal (the float32 oracle and the float32 step model of k_fbank,
each within half the tolerance), that every signal is what it claims to be, and the order of the centring sums."""
import numpy as np
import pytest
import torch

import fbank_truth as ft


def _raw_chunks(data):
    B = 1 + (ft.TOTAL - ft.N) // ft.STRIDE
    return [ft.chunk_of(data, b, ft.N, ft.STRIDE, ft.TOTAL) for b in range(B)]


@pytest.mark.parametrize("name", list(ft.SIGNALS))
def test_truth_is_the_oracle_in_float64_above_the_floor(name):
    """log Ef == kaldi_fbank in float64 wherever E64 >= 2^-23 (below it the two floors differ: -15.94 and -36)"""
    from oracle.models import kaldi_fbank
    x = ft.signal(name, ft.TOTAL)
    tr = ft.truth(x)
    want = kaldi_fbank((torch.from_numpy(x).double() * 32768.0).unsqueeze(0)).numpy()
    above = tr["E64"] >= ft.EPS32
    assert tr["Ef"].shape == want.shape == (ft.num_frames(ft.TOTAL), ft.NMEL)
    assert above.any()
    assert np.abs(np.log(tr["Ef"]) - want)[above].max() <= 1e-9
    assert (tr["Ef"][~above] == ft.EPS32).all()
    # a silent frame: the float32 floor, not the float64 one
    silent = ft.truth(np.zeros(ft.WIN, dtype=np.float32))
    assert (silent["Ef"] == ft.EPS32).all() and silent["floor"].all() and (silent["tol"] == 1e-4 * ft.EPS32).all()


def test_every_signal_is_admissible():
    """the float32 oracle and the step model, each <= 0.5 of the tolerance at KAPPA = 1, on every chunk the GPU module
    runs: the three-chunk layout of every signal and both framing-edge signals at every length"""
    assert ft.KAPPA == 1.0
    cases = [(name, ft.layout_case(name)["chunks"]) for name in ft.SIGNALS]
    cases += [(f"{name}_N{n}", ft.edge_case(name, n)["chunks"])
              for name in ("harmonic_envelope", "silence_burst") for n in ft.EDGE_LENGTHS]
    worst = 0.0
    print(f"\n{'signal':28s} float32 oracle   step model")
    for name, chunks in cases:
        r_oracle, r_model = max(c["r_oracle"] for c in chunks), max(c["r_model"] for c in chunks)
        print(f"{name:28s} {r_oracle:14.3f} {r_model:12.3f}")
        worst = max(worst, r_oracle, r_model)
    assert worst <= 0.5, "an inadmissible signal (see the table): choose other inputs"


@pytest.mark.parametrize("name", list(ft.SIGNALS))
def test_every_signal_is_what_it_claims(name):
    data = ft.signal(name, ft.TOTAL)
    floor_frames = int(ft.truth(data)["floor"].sum())
    assert (floor_frames > 0) == (name in ft.HAS_FLOOR_FRAMES), floor_frames
    ranges = [10.0 * np.log10(t["Ef"].max() / t["Ef"].min()) for t in map(ft.truth, _raw_chunks(data))]
    print(f"\n{name}: {floor_frames} frames at the floor, range of Ef per chunk {[round(r, 1) for r in ranges]} dB")
    if name in ft.HAS_100_DB:
        assert min(ranges) >= 100.0
    if name == "dc025_envelope":
        # the stretches of exactly 0.25: there, and only there, a non-zero constant frame -- and float32 agrees exactly
        fr = np.lib.stride_tricks.sliding_window_view(data, ft.WIN)[::ft.SHIFT]
        const = (fr == 0.25).all(axis=1)
        assert const.sum() >= 10 and ft.truth(data)["floor"][const].all()
        assert (ft.oracle32(data)[const] == ft.LOG_EPS32).all()
        assert (ft.step_model(data)[const] == np.float32(ft.EPS32)).all()
    else:
        fr = np.lib.stride_tricks.sliding_window_view(data, ft.WIN)[::ft.SHIFT]
        constant = (fr == fr[:, :1]).all(axis=1)
        assert not (constant & (fr[:, 0] != 0)).any(), "a non-zero constant frame: ill-posed in float32 (input rule)"


def test_signals_follow_the_seed_and_are_not_each_other():
    a = {name: ft.signal(name, 4800) for name in ft.SIGNALS}
    assert all(np.array_equal(a[name], ft.signal(name, 4800)) for name in ft.SIGNALS)
    names = list(ft.SIGNALS)
    assert all(not np.array_equal(a[p], a[q]) for i, p in enumerate(names) for q in names[i + 1:])


def test_step_model_runs_in_float32_and_tracks_the_truth_on_a_tone():
    """the model's FFT is a DFT: a tone exactly on bin 40 puts its energy into the bands that hold bin 40"""
    x = ft.signal("tone_bin40", 4800)
    e = ft.step_model(x)
    tr = ft.truth(x)
    assert e.dtype == np.float32 and e.shape == tr["Ef"].shape
    assert (np.argmax(e, axis=1) == np.argmax(tr["Ef"], axis=1)).all()
    assert ft.mel_table()[np.argmax(e[0]), 40] > 0


def test_centring_order():
    """the four strided sequential partial sums of k_fbank_center on features 12 +- 4: accumulated in float32 (the
    kernel as it was) they drift past the contract's atol of 1e-5 with the frame count; accumulated in float64 (the
    kernel as it is) the mean is the float64 mean rounded once.  torch's float32 mean, the `ref32` of the GPU test,
    stays admissible (half of 1e-5)"""
    print(f"\n{'T':>6s} {'float32 order':>14s} {'float64 order':>14s} {'torch float32':>14s}")
    for T in (298, 998, 6000, 60000):
        g = torch.Generator().manual_seed(4242 + T + ft.SEED_OFFSET)
        x = (12.0 + 8.0 * (torch.rand(T, ft.NMEL, generator=g) - 0.5)).float()
        mean64 = x.double().mean(dim=0).numpy()
        d32 = np.abs(ft.kernel_order_mean(x.numpy()).astype(np.float64) - mean64).max()
        d64 = np.abs(ft.kernel_order_mean(x.numpy(), np.float64).astype(np.float64) - mean64).max()
        dtorch = np.abs(x.mean(dim=0).double().numpy() - mean64).max()
        print(f"{T:6d} {d32:14.2e} {d64:14.2e} {dtorch:14.2e}")
        assert d64 <= 2.0 ** -21 + 1e-9   # half an ulp of a float32 in [8, 16), and a little for the double sums
        assert dtorch <= 5e-6
    # a chunk of identical frames (silence): the float64 sums of T float32 values are exact, so is the mean
    for T in (1, 3, 148, 298, 6000):
        x = np.full((T, ft.NMEL), ft.LOG_EPS32, dtype=np.float32)
        assert (ft.kernel_order_mean(x, np.float64) == ft.LOG_EPS32).all()
