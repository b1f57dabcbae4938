"""GPU: `pa_vbx_run_batch` (whole VB inferences for a batch of jobs, csrc/vbx.hip) against the per-file loop of
`VBxClustering._vbx` -- `pa_vbx_iteration` plus the convergence test on the host -- bit for bit; and
`pa_constrained_assign` (csrc/assign.hip) through `BaseClustering.constrained_argmax_device` against the host's
`constrained_argmax`.

The yardstick is `==`: the batched kernels call the very `__device__` bodies of the per-file kernels, with the same
reduction trees and the same row split, and the file is compiled with -ffp-contract=off.  The per-file kernels
themselves are held to the oracle and to extended-precision truths by tests/test_vbx_gpu.py and
tests/test_vbx_kernels_gpu.py."""
import numpy as np
import pytest

from assign_model import CAP_COUNTS_PLANTED, FLAGGED_CAP, SHAPES, assign_model, host_assign, random_case

pytestmark = pytest.mark.gpu

#: the corners of Fa / Fb of tests/test_vbx_gpu.py (they stop after about 3 and about 16 iterations on the first case)
#: and its default
FACTORS = ((0.4, 0.05), (0.02, 12.0), (0.07, 0.8))
#: (chunks, speakers, noise, seed, quantiles of the merge heights the two cuts are taken at); 165 and 442 training
#: embeddings; the oracle runs the jobs of the first case for 3, 16, 3 / 3, 18, 5 iterations, those of the second
#: for 20, 9, 4 / 12, 10, 4 (oracle.vbx.cluster_vbx on the host)
CASES = ((350, 5, 0.45, 5, (0.978, 0.97)), (900, 7, 1.2, 1, (0.97, 0.9)))


@pytest.fixture(scope="module")
def plda_dir(tmp_path_factory):
    from oracle.vbx import synth_plda
    return synth_plda(str(tmp_path_factory.mktemp("plda")))


def _embeddings(C, K, noise, seed, D_=256, F=60, S=3):
    """as in tests/test_vbx_gpu.py"""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((K, D_))
    who = rng.integers(0, K, size=(C, S))
    emb = (centers[who] + noise * rng.standard_normal((C, S, D_))).astype(np.float32)
    emb[rng.integers(0, C), rng.integers(0, S)] = np.nan
    seg = (rng.uniform(size=(C, F, S)) < 0.45).astype(np.float32)
    seg[rng.integers(0, C, C // 8), :, rng.integers(0, S, C // 8)] = 0.0
    return emb, seg


@pytest.fixture(scope="module", params=CASES, ids=lambda case: f"C{case[0]}")
def problem(request, plda_dir, gpu_device):
    """the features of one file, two cuts with different S and the cut into one cluster, the jobs of the batch, and
    -- computed once -- what the per-file loop gives for every job"""
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.clustering import Dendrogram
    from pyannote_audio_amd.core import SlidingWindow, SlidingWindowFeature
    C, K, noise, seed, levels = request.param
    emb, seg = _embeddings(C, K, noise, seed)
    clu = pa.VBxClustering(plda=plda_dir).instantiate({"threshold": 0.6, "Fa": 0.07, "Fb": 0.8}).to(gpu_device)
    chunks = SlidingWindow(start=0.0, duration=10.0, step=1.0)
    train, unit, Z, fea = clu.before_cut(emb, SlidingWindowFeature(seg, chunks))
    assert 150 <= len(train) <= 450 and tuple(fea.shape) == (len(train), 128)
    thresholds = [float(t) for t in np.quantile(Z[:, 2], levels)] + [float(Z[:, 2].max()) + 1.0]
    cuts = Dendrogram(Z).cuts(thresholds)
    labels = [np.unique(row, return_inverse=True)[1] for row in cuts]
    sizes = [int(row.max()) + 1 for row in labels]
    print(f"N = {len(train)}, clusters of the cuts: {sizes}")
    assert sizes[2] == 1 and len({sizes[0], sizes[1], 1}) == 3
    inits = [clu.initial_responsibilities(row) for row in labels]
    # three (Fa, Fb) per cut, interleaved so that neighbours differ in S, and one job with S = 1
    jobs = [(i, Fa, Fb) for Fa, Fb in FACTORS for i in (0, 1)] + [(2, 0.07, 0.8)]
    loop = []
    for i, Fa, Fb in jobs:
        clu.instantiate({"threshold": 0.6, "Fa": Fa, "Fb": Fb})
        q, _ = clu._vbx(fea, labels[i])
        loop.append((q, list(clu.last_elbo_history)))
        assert clu.timings["vbx_iterations"] == len(loop[-1][1])
    print("iterations of the loop:", [len(history) for _, history in loop])
    return clu, fea, inits, jobs, loop


def same(results, loop) -> None:
    assert len(results) == len(loop)
    for j, ((q, history), (want_q, want_history)) in enumerate(zip(results, loop)):
        assert len(history) == len(want_history), j                    # the iteration count
        assert history == want_history, j                              # the ELBO history up to the stop, `==`
        assert q.shape == want_q.shape and q.dtype == want_q.dtype and np.array_equal(q, want_q), j


def test_batch_equals_the_loop_bit_for_bit(problem):
    clu, fea, inits, jobs, loop = problem
    counts = [len(history) for _, history in loop]
    assert len(set(counts)) >= 3 and min(counts) < 6 and max(counts) >= 16     # jobs finish in different rounds
    same(clu.vbx_batch(fea, inits, jobs), loop)
    assert clu.last_vbx_calls == 1


def test_a_budget_that_splits_the_batch_gives_the_same_bits(problem):
    import pyannote_audio_amd.ffi as ffi
    clu, fea, inits, jobs, loop = problem
    n, smax = fea.shape[0], max(q0.shape[1] for q0 in inits)
    budget = int(ffi.load().pa_vbx_batch_workspace_bytes(3, n, smax, 128))
    same(clu.vbx_batch(fea, inits, jobs, workspace_bytes=budget), loop)
    assert clu.last_vbx_calls >= 2
    same(clu.vbx_batch(fea, inits, jobs, workspace_bytes=1), loop)                # every job on its own
    assert clu.last_vbx_calls == len(jobs)


def test_reversed_job_order_gives_the_same_bits_per_job(problem):
    clu, fea, inits, jobs, loop = problem
    same(clu.vbx_batch(fea, inits, jobs[::-1]), loop[::-1])


def test_batch_limits_are_refused(problem, gpu_device):
    import torch
    import pyannote_audio_amd.ffi as ffi
    clu, fea, inits, jobs, _ = problem
    lib = ffi.load()
    assert lib.pa_vbx_batch_workspace_bytes(0, 10, 3, 128) == 0
    narrow = fea[:, :64].contiguous()
    with pytest.raises(ValueError):                 # D = 128
        clu.vbx_batch(narrow, inits, jobs[:1])
    word = torch.zeros(8, dtype=torch.float64, device=gpu_device)
    table = torch.zeros(2, dtype=torch.int64, device=gpu_device)
    rc = lib.pa_vbx_run_batch(ffi.ptr(fea), ffi.ptr(word), fea.shape[0], 128, 1, ffi.ptr(word), 8, ffi.ptr(table),
                              ffi.ptr(word), 8192, 20, 1e-4, ffi.ptr(word), ffi.ptr(word), ffi.ptr(word),
                              ffi.ptr(word), 64, ffi.stream())
    assert rc == 3                                  # (d + s) * 8 <= 64 KiB, before anything is launched


# ---------------------------------------------------------------------------------------------- assignment
def device_assign(gpu_device, soft, silent):
    from pyannote_audio_amd.clustering import BaseClustering
    clustering = BaseClustering().to(gpu_device)
    return clustering.constrained_argmax_device(soft, silent), clustering


@pytest.mark.parametrize("C,S,K", SHAPES)
def test_assignment_equals_the_masked_host_result(gpu_device, C, S, K):
    import torch
    import pyannote_audio_amd.ffi as ffi
    soft, silent, must = random_case(C, S, K, seed=C + 10 * S + K)
    want = host_assign(soft, silent)
    got, clustering = device_assign(gpu_device, soft, silent)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(want, np.where(silent, -2, clustering.constrained_argmax(soft)))
    # the kernel alone: its flags are the model's, and where it decides it has decided like the host
    dev_soft, dev_silent = torch.from_numpy(soft).to(gpu_device), torch.from_numpy(silent.astype(np.uint8)).to(gpu_device)
    hard = torch.full((C, S), 99, dtype=torch.int8, device=gpu_device)
    flags = torch.full((C,), 99, dtype=torch.uint8, device=gpu_device)
    ffi.check(ffi.load().pa_constrained_assign(ffi.ptr(dev_soft), ffi.ptr(dev_silent), C, S, K, ffi.ptr(hard),
                                               ffi.ptr(flags), ffi.stream()), "pa_constrained_assign")
    hard, flags = hard.cpu().numpy(), flags.cpu().numpy().astype(bool)
    model_hard, model_flags = assign_model(soft, silent)
    assert np.array_equal(flags, model_flags) and np.array_equal(hard, model_hard)
    assert flags[must].all()                                           # the NaN chunk and the tie chunk
    assert np.array_equal(hard[~flags], want[~flags])
    share = (int(flags.sum()) - len(must)) / C
    print(f"(C, S, K) = {(C, S, K)}: {int(flags.sum())} of {C} chunks flagged ({len(must)} planted), "
          f"share beyond the planted ones {share:.3f}")
    assert share <= FLAGGED_CAP
    if (C, S, K) in CAP_COUNTS_PLANTED:
        assert int(flags.sum()) / C <= FLAGGED_CAP
    assert clustering.last_flagged_chunks == int(flags.sum())


def test_nan_silencing_of_the_pipeline(gpu_device):
    """`soft[silent] = soft.min() - 1` with a NaN embedding in the file: `soft.min()` is NaN, so `nan_to_num` lifts
    the silent rows to the smallest finite value, where they no longer lie below every active row"""
    rng = np.random.default_rng(3)
    soft = rng.uniform(0.0, 2.0, size=(40, 3, 2))
    silent = rng.uniform(size=(40, 3)) < 0.4
    silent[5] = [False, False, True]
    soft[9, 1] = np.nan
    silent[9, 1] = False
    low = np.unravel_index(np.nanargmin(np.where(silent[:, :, None], np.nan, soft)), soft.shape)
    silent[low[0]] = [s != low[1] for s in range(3)]          # the smallest value sits beside two silent rows
    soft[silent] = soft.min() - 1.0
    assert np.isnan(soft[silent]).all()
    got, clustering = device_assign(gpu_device, soft.copy(), silent)
    assert np.array_equal(got, np.where(silent, -2, clustering.constrained_argmax(soft)))
    assert clustering.last_flagged_chunks >= 2


@pytest.mark.parametrize("C,S,K", [(12, 5, 3), (12, 3, 65)])
def test_beyond_the_kernel_limits_the_host_solves(gpu_device, C, S, K):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    assert (lib.pa_constrained_assign_max_speakers(), lib.pa_constrained_assign_max_clusters()) == (4, 64)
    soft, silent, _ = random_case(C, S, K, seed=S + K)
    got, clustering = device_assign(gpu_device, soft, silent)
    assert np.array_equal(got, host_assign(soft, silent))
    assert clustering.last_flagged_chunks == C
