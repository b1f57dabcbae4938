"""GPU: `permutation.permutate_batch` -- the cost matrices (`pa_pair_costs`), SciPy's assignment (`pa_lsap_batch`)
and the re-ordering (`pa_permute_classes`) of csrc/lsap.hip -- against the host `permutate` on the same values, with
`==` on the re-ordered values, the permutations and the costs.  Silent (all-zero) classes give equal columns, so
most assignments here have several optima and only SciPy's own choice passes."""
import ctypes

import numpy as np
import pytest
import torch

import lsap_model

pytestmark = pytest.mark.gpu

ALL_3 = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def as_rows(permutations) -> np.ndarray:
    """the host's list of tuples with None -> what the device returns"""
    return np.array([[-1 if j is None else j for j in row] for row in permutations], dtype=np.int32)


def activations(seed, batch, frames, c1, c2, dtype):
    """y1 (batch, frames, c1), y2 (batch, frames, c2): y1 is a noisy shuffle of y2's classes; a class a side is silent
    in most items, and two of y2 where it has the room"""
    rng = np.random.default_rng(seed)
    y2 = rng.random((batch, frames, c2))
    y1 = np.zeros((batch, frames, c1))
    for b in range(batch):
        order = rng.permutation(max(c1, c2))
        for i in range(c1):
            if order[i] < c2:
                y1[b, :, i] = np.clip(y2[b, :, order[i]] + 0.05 * rng.standard_normal(frames), 0, 1)
        if b % 4 != 3:
            y1[b, :, rng.integers(0, c1)] = 0
            y2[b, :, rng.integers(0, c2)] = 0
            if c2 > 2:
                y2[b, :, rng.integers(0, c2)] = 0
    return y1.astype(dtype), y2.astype(dtype)


def check(y1, y2, device_y1, device_y2, cost_func):
    from pyannote_audio_amd.permutation import permutate, permutate_batch
    want, want_perm, want_cost = permutate(y1, y2, cost_func=cost_func, return_cost=True)
    got, perm, cost = permutate_batch(device_y1, device_y2, cost_func=cost_func, return_cost=True)
    assert got.device == perm.device == cost.device == device_y1.device
    assert got.dtype == device_y2.dtype and perm.dtype == torch.int32 and cost.dtype == device_y1.dtype
    assert got.is_contiguous() and perm.is_contiguous()
    assert np.array_equal(perm.cpu().numpy(), as_rows(want_perm))
    assert np.array_equal(cost.cpu().numpy(), want_cost)
    assert np.array_equal(got.cpu().numpy(), want)
    pair = permutate_batch(device_y1, device_y2, cost_func=cost_func)
    assert len(pair) == 2 and torch.equal(pair[0], got) and torch.equal(pair[1], perm)
    return as_rows(want_perm), want_cost


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("cost_func", ["mse", "mae"])
@pytest.mark.parametrize("c1,c2,frames", [(3, 3, 589), (3, 5, 293), (5, 3, 293), (7, 2, 17), (1, 5, 64), (8, 8, 100)])
def test_permutate_batch_equals_permutate(gpu_device, dtype, cost_func, c1, c2, frames):
    y1, y2 = activations(frames + c1, 8, frames, c1, c2, dtype)
    d1, d2 = torch.from_numpy(y1).to(gpu_device), torch.from_numpy(y2).to(gpu_device)
    perm, cost = check(y1, y2, d1, d2, cost_func)
    # ties are there: some item has two equal columns of costs, and with fewer classes in y2 somebody gets None
    assert any((cost[b][:, :, None] == cost[b][:, None, :]).all(axis=0).sum() > c2 for b in range(8)) or c2 < 3
    assert (perm == -1).any() == (c2 < c1)
    # the (batch, classes, frames) layout of metrics.py, seen through a transposed view
    s1 = torch.from_numpy(np.ascontiguousarray(y1.transpose(0, 2, 1))).to(gpu_device).transpose(1, 2)
    s2 = torch.from_numpy(np.ascontiguousarray(y2.transpose(0, 2, 1))).to(gpu_device).transpose(1, 2)
    assert not s1.is_contiguous() or c1 == 1
    check(y1, y2, s1, s2, cost_func)
    # one y2 for the whole batch
    check(y1, y2[0], d1, d2[0], cost_func)
    check(y1, y2[0], s1, s2[0], cost_func)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("frames,c1,c2", [(589, 3, 3), (293, 4, 7), (64, 1, 5), (17, 7, 2), (2000, 8, 8)])
def test_pair_costs_equal_the_numpy_model(gpu_device, dtype, frames, c1, c2):
    """`pa_pair_costs` directly: the padded float64 matrix the solver sees, padding rows included"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    y1, y2 = activations(frames, 5, frames, c1, c2, dtype)
    d1, d2 = torch.from_numpy(y1).to(gpu_device), torch.from_numpy(y2).to(gpu_device)
    rows = max(c1, c2)
    for mae in (0, 1):
        out = torch.full((5 + 2, rows, c2), -7.0, dtype=torch.float64, device=gpu_device)
        ffi.check(lib.pa_pair_costs(ctypes.c_void_p(d1.data_ptr()), *d1.stride(), ctypes.c_void_p(d2.data_ptr()),
                                    *d2.stride(), int(dtype == np.float64), 5, frames, c1, c2, mae, ffi.ptr(out[1:]),
                                    ffi.stream()), "pa_pair_costs")
        out = out.cpu().numpy()
        assert (out[0] == -7.0).all() and (out[-1] == -7.0).all()
        want = np.stack([lsap_model.padded_costs(y1[b], y2[b], "mae" if mae else "mse") for b in range(5)])
        assert np.array_equal(out[1:-1], want)


def test_the_reference_s_own_cases_on_the_device(gpu_device):
    """tests/utils/test_permutation.py of the reference (tests/test_permutation_cpu.py), through the device route"""
    from pyannote_audio_amd.permutation import permutate_batch
    torch.manual_seed(0)
    y2 = torch.randn((10, 3))
    y1 = torch.stack([y2[:, p] for p in ALL_3])
    permutated, permutations = permutate_batch(y1.to(gpu_device), y2.to(gpu_device))
    assert permutations.cpu().tolist() == [list(p) for p in ALL_3]
    assert torch.equal(permutated.cpu(), y1)
    # fewer speakers in y2
    rng = np.random.default_rng(1)
    wanted = [(0, 1, None), (0, None, 1), (1, 0, None), (1, None, 0), (None, 0, 1), (None, 1, 0)]
    y2 = rng.standard_normal((10, 2))
    y1 = np.zeros((len(wanted), 10, 3))
    for k, p in enumerate(wanted):
        for i, j in enumerate(p):
            if j is not None:
                y1[k, :, i] = y2[:, j]
    _, permutations = permutate_batch(torch.from_numpy(y1).to(gpu_device), torch.from_numpy(y2).to(gpu_device))
    assert np.array_equal(permutations.cpu().numpy(), as_rows(wanted))
    # more speakers in y2
    rng = np.random.default_rng(2)
    wanted = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    y2 = rng.standard_normal((10, 3))
    y1 = np.stack([np.stack([y2[:, j] for j in p], axis=1) for p in wanted])
    permutated, permutations = permutate_batch(torch.from_numpy(y1).to(gpu_device), torch.from_numpy(y2).to(gpu_device))
    assert np.array_equal(permutations.cpu().numpy(), as_rows(wanted))
    assert np.array_equal(permutated.cpu().numpy(), y1)


def test_what_has_no_device_route_goes_through_permutate(gpu_device):
    from pyannote_audio_amd.permutation import permutate, permutate_batch
    y1, y2 = activations(3, 4, 50, 3, 3, np.float32)
    d1, d2 = torch.from_numpy(y1).to(gpu_device), torch.from_numpy(y2).to(gpu_device)
    mae = lambda Y, y, **kw: torch.mean(torch.abs(Y - y), axis=0)      # noqa: E731  (utils/permutation.py:84-96)
    want, want_perm, want_cost = permutate(torch.from_numpy(y1), torch.from_numpy(y2), cost_func=mae, return_cost=True)
    got, perm, cost = permutate_batch(d1, d2, cost_func=mae, return_cost=True)
    assert got.device == perm.device == cost.device == d1.device
    assert torch.equal(got.cpu(), want) and torch.equal(cost.cpu(), want_cost)
    assert np.array_equal(perm.cpu().numpy(), as_rows(want_perm))
    # one class a side: numpy adds that single column pairwise
    got, perm = permutate_batch(d1[:, :, :1], d2[:, :, :1])
    assert perm.cpu().tolist() == [[0]] * 4 and torch.equal(got, d2[:, :, :1])
    # the host function keeps its behaviour for device tensors: host tensors out
    host, _ = permutate(d1, d2)
    assert not host.is_cuda


def test_more_than_four_speakers_stay_on_the_device(gpu_device, monkeypatch):
    """`diarization_error_rate` with 5 speakers takes its permutation from `permutate_batch`: the host solver is not
    called, and the counts are those of the host `permutate`'s permutation"""
    import metrics_truth
    from pyannote_audio_amd import metrics, permutation
    from test_metrics_gpu import seeded_chunks
    preds, target = seeded_chunks(6, 5, 293, seed=41)
    target[1, 2] = 0
    target[1, 4] = 0                          # two silent speakers: equal rows of costs
    thresholds = torch.linspace(0.0, 1.0, 11)
    _, found = permutation.permutate(np.transpose(target, (0, 2, 1)).astype(np.float32), np.transpose(preds, (0, 2, 1)))
    want_counts, want_total = metrics_truth.chunk_components(preds, target, thresholds.numpy(),
                                                             perm=np.array(found, dtype=np.int32))

    def refuse(*args, **kwargs):
        raise AssertionError("the host solver was called")

    monkeypatch.setattr(permutation, "linear_sum_assignment", refuse)
    monkeypatch.setattr(permutation, "permutate", refuse)
    monkeypatch.setattr(metrics, "permutate", refuse)
    _, (fa, md, conf, tot) = metrics.diarization_error_rate(
        torch.from_numpy(preds).to(gpu_device), torch.from_numpy(target).to(gpu_device), threshold=thresholds,
        reduce="chunk", return_components=True)
    assert np.array_equal(torch.stack([fa, md, conf], dim=-1).cpu().numpy(), want_counts)
    assert np.array_equal(tot.cpu().numpy(), want_total)
