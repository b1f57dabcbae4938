"""CPU: what the VBx route of `ClusteringTuner` decides on the host -- which candidates share an initialisation and
a VB inference, and how a batch is split at a workspace budget -- and the numpy model of `pa_constrained_assign`
(tests/assign_model.py) against SciPy.  No GPU, no library call."""
import numpy as np
import pytest

from assign_model import CAP_COUNTS_PLANTED, FLAGGED_CAP, SHAPES, assign_model, host_assign, random_case


def test_equal_cut_rows_share_an_initialisation():
    from pyannote_audio_amd.tuning import plan_vbx_jobs
    rows = np.array([[0, 1, 2, 0], [0, 1, 2, 0], [0, 1, 1, 0], [0, 0, 0, 0], [0, 1, 1, 0]], dtype=np.int32)
    picks = [(t, 0.07, 0.8) for t in range(5)]
    inits, jobs, job_of = plan_vbx_jobs(rows, picks)
    assert inits == [0, 2, 3]                       # the first row of every distinct cut, in row order
    assert jobs == [(0, 0.07, 0.8), (1, 0.07, 0.8), (2, 0.07, 0.8)]
    assert job_of == [0, 0, 1, 2, 1]


def test_duplicate_jobs_collapse_and_the_candidate_order_is_kept():
    from pyannote_audio_amd.tuning import plan_vbx_jobs
    rows = np.array([[0, 0, 1], [0, 1, 2], [0, 0, 1]], dtype=np.int32)
    picks = [(1, 0.4, 0.05), (0, 0.4, 0.05), (2, 0.4, 0.05), (1, 0.02, 12.0), (1, 0.4, 0.05), (2, 0.02, 12.0),
             (0, 0.02, 12.0)]
    inits, jobs, job_of = plan_vbx_jobs(rows, picks)
    assert inits == [0, 1]
    # jobs in order of first use; rows 0 and 2 are one initialisation
    assert jobs == [(1, 0.4, 0.05), (0, 0.4, 0.05), (1, 0.02, 12.0), (0, 0.02, 12.0)]
    assert job_of == [0, 1, 1, 2, 0, 3, 3]
    assert [jobs[j] for j in job_of] == [({0: 0, 1: 1, 2: 0}[t], a, b) for t, a, b in picks]
    # an integer and a float that compare equal name one job
    assert plan_vbx_jobs(rows, [(0, 1, 2), (0, 1.0, 2.0)])[2] == [0, 0]


def test_budget_splitting():
    from pyannote_audio_amd.clustering import split_vbx_jobs
    sizes = [3, 9, 2, 2, 12, 1]
    bytes_of = lambda jobs, smax: 1000 + 100 * jobs * smax          # noqa: E731  (shared part + per-job part)
    assert split_vbx_jobs(sizes, bytes_of, None) == [[0, 1, 2, 3, 4, 5]]
    assert split_vbx_jobs(sizes, bytes_of, 10 ** 9) == [[0, 1, 2, 3, 4, 5]]
    runs = split_vbx_jobs(sizes, bytes_of, 1000 + 100 * 4 * 9)
    assert runs == [[0, 1, 2, 3], [4, 5]]
    for run in runs:                                                  # every run fits, none could take the next job
        assert bytes_of(len(run), max(sizes[j] for j in run)) <= 1000 + 100 * 4 * 9
    assert [j for run in runs for j in run] == list(range(len(sizes)))
    # a job that exceeds the budget on its own still runs, alone
    assert split_vbx_jobs(sizes, bytes_of, 1) == [[j] for j in range(len(sizes))]
    assert split_vbx_jobs([], bytes_of, 1) == []


def test_sweep_vbx_wants_a_vbx_pipeline():
    from pyannote_audio_amd.tuning import ClusteringTuner

    class NotVBx:
        clustering = object()
        get_metric = None

    with pytest.raises(TypeError):
        ClusteringTuner(NotVBx()).sweep_vbx([0.6], [0.07], [0.8])


@pytest.mark.parametrize("S,K", [(1, 1), (2, 1), (3, 1), (3, 2), (3, 3), (4, 2), (4, 4), (2, 7), (3, 8), (4, 9)])
def test_model_equals_scipy_outside_the_flagged_set(S, K):
    """40 random chunks per shape (400 in all): rows silent at random, fewer clusters than active rows included"""
    soft, silent, _ = random_case(40, S, K, seed=100 * S + K, planted=False)
    hard, flagged = assign_model(soft, silent)
    want = host_assign(soft, silent)
    assert not flagged.all()
    assert np.array_equal(hard[~flagged], want[~flagged])
    assert (hard[flagged] == -2).all()


def test_model_flags_what_it_cannot_decide():
    soft, silent, must = random_case(16, 3, 4, seed=5)
    hard, flagged = assign_model(soft, silent)
    assert must == [1, 2] and flagged[must].all()
    assert not flagged[0] and (hard[0] == -2).all()              # a fully silent chunk is decided: nothing to assign
    # a runner-up just inside / just outside the margin
    tie = np.array([[[1.0, 0.75], [0.75, 0.5 + 5e-10]]])          # 1.5 + 5e-10 against 1.5
    clear = np.array([[[1.0, 0.75], [0.75, 0.5 + 5e-9]]])         # 1.5 + 5e-9 against 1.5
    none = np.zeros((1, 2), dtype=bool)
    assert assign_model(tie, none)[1][0] and not assign_model(clear, none)[1][0]
    assert np.array_equal(assign_model(clear, none)[0], [[0, 1]])
    # the gap between the last kept and the first dropped column of a row
    dropped = np.array([[[1.0, 0.2, 0.2 - 5e-10], [0.1, 0.9, 0.0]]])
    assert assign_model(dropped, none)[1][0]


@pytest.mark.parametrize("C,S,K", SHAPES)
def test_gpu_test_inputs_stay_under_the_flag_cap(C, S, K):
    """the seeds of tests/test_vbx_batch_gpu.py: at most 5 % of the chunks go to the host.  The chunks planted to be
    flagged (one NaN row, one exact tie) are counted apart: they are flagged by construction, and two of them are
    more than 5 % of the smaller cases."""
    soft, silent, must = random_case(C, S, K, seed=C + 10 * S + K)
    _, flagged = assign_model(soft, silent)
    assert flagged[must].all()
    share = (int(flagged.sum()) - len(must)) / C
    print(f"(C, S, K) = {(C, S, K)}: {int(flagged.sum())} of {C} chunks flagged, {len(must)} of them planted")
    assert share <= FLAGGED_CAP
    if (C, S, K) in CAP_COUNTS_PLANTED:
        assert int(flagged.sum()) / C <= FLAGGED_CAP
