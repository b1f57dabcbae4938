"""GPU: speaker identification (pyannote_audio_amd/identification.py, csrc/identify.hip) against its numpy truth
(tests/identify_model.py).  Every comparison is `==` (NaN equal to NaN): the distances are SciPy's `cdist` bits, the
statistics add in ascending order with one rounding per operation, a selection is a stable argsort, and the assignment is
SciPy's, tie for tie.  Shapes are the smallest at which a path changes: dimensions around the two-way dot product's pair
and tail, tables of one row, of K and K + 1 rows, of one tile, one tile and a row, and three tiles; one query row and
more than a workgroup's four; duplicated rows across the K-th boundary."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import identify_model as model  # noqa: E402
from hostile_workspace import run_under_fills  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=want.dtype.kind == "f")


@pytest.fixture(scope="module")
def geometry(gpu_device):
    from pyannote_audio_amd.identification import identify_geometry
    tile, max_top, max_k = identify_geometry()
    assert tile >= 1 and max_top >= 512 and max_k >= 8
    return tile, max_top, max_k


def _stats_on_device(X, C, K, device):
    from pyannote_audio_amd.identification import cohort_stats
    mean, std, status = cohort_stats(torch.from_numpy(X).to(device), torch.from_numpy(C).to(device), K)
    return mean.cpu().numpy(), std.cpu().numpy(), status.cpu().numpy()


# ------------------------------------------------------------------------------------------------ cohort statistics
@pytest.mark.parametrize("D", [1, 2, 255, 256])
def test_cohort_statistics_equal_the_model(gpu_device, geometry, D):
    tile, max_top, _ = geometry
    rng = np.random.default_rng(100 + D)
    pool = rng.standard_normal((2 * tile + 3 + max_top + 1, D))
    queries = rng.standard_normal((65, D))
    seen = set()
    for top in (1, 2, 300, max_top):
        for N in (1, top, top + 1, tile, tile + 1, 2 * tile + 3):
            K = min(top, N)                      # (the clipping is the caller's business)
            for M in (1, 65):
                if (N, K, M) in seen:
                    continue
                seen.add((N, K, M))
                X, C = queries[:M], pool[:N]
                got = _stats_on_device(X, C, K, gpu_device)
                want = model.cohort_stats(X, C, K)
                for g, w, what in zip(got, want, ("mean", "std", "status")):
                    assert _same(g, w), f"{what}: D={D} N={N} K={K} M={M}"
                assert not got[2].any()


def test_cohort_statistics_with_duplicated_rows_and_rows_without_direction(gpu_device, geometry):
    tile, max_top, _ = geometry
    rng = np.random.default_rng(7)
    D, N = 24, 2 * tile + 3
    base = rng.standard_normal((N // 3, D))
    C = base[rng.permutation(N) % (N // 3)]          # every row three times (or four), spread over the tiles
    X = rng.standard_normal((65, D))
    X[3] = 0.0
    X[17, 5] = np.nan
    X[40] = 1e200                                    # a norm that overflows
    X[64] = C[11]                                    # distance 0 (or an ulp) to four cohort rows
    for K in (1, 2, 3, 4, 299, 300, 301, max_top):
        mean, std, status = _stats_on_device(X, C, K, gpu_device)
        want = model.cohort_stats(X, C, K)
        assert _same(mean, want[0]) and _same(std, want[1]) and _same(status, want[2]), K
        assert status.tolist() == [1 if i in (3, 17, 40) else 0 for i in range(65)]
        assert np.isnan(mean[[3, 17, 40]]).all() and np.isnan(std[[3, 17, 40]]).all()
        assert np.isfinite(np.delete(mean, [3, 17, 40])).all()
    # a constant cohort: every distance the same; with K = 2 the mean is exact ((s + s) / 2) and std exactly 0
    mean, std, _ = _stats_on_device(X[:2], np.repeat(C[:1], 10, axis=0), 2, gpu_device)
    assert (std == 0).all() and _same(mean, model.cohort_stats(X[:2], np.repeat(C[:1], 10, axis=0), 2)[0])


def test_cohort_statistics_refusals(gpu_device, geometry):
    from pyannote_audio_amd.identification import cohort_stats
    _, max_top, _ = geometry
    X = torch.ones((2, 4), dtype=torch.float64, device=gpu_device)
    C = torch.ones((max_top + 5, 4), dtype=torch.float64, device=gpu_device)
    for K in (0, max_top + 1):
        with pytest.raises(ValueError, match="K = "):
            cohort_stats(X, C, K)
    with pytest.raises(ValueError, match="K = 4"):
        cohort_stats(X, C[:3], 4)


# ------------------------------------------------------------------------------------------------------------ top-k
def _gallery_case(rng, M, Ng, D, with_stats):
    """queries, a gallery in which every row appears at least twice (equal values: the lower index wins), and statistics
    that are equal for equal rows so that the normalised values tie as well"""
    distinct = max(1, Ng // 2)
    base = rng.standard_normal((distinct, D))
    pick = rng.permutation(Ng) % distinct
    G = base[pick]
    Q = rng.standard_normal((M, D))
    stats = None
    if with_stats:
        g_mean, g_std = rng.random(distinct) + 0.5, rng.random(distinct) + 0.1
        stats = (rng.random(M) + 0.5, rng.random(M) + 0.1, g_mean[pick], g_std[pick])
    return Q, G, stats


def _to_device(device, *arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays)


@pytest.mark.parametrize("with_stats", [False, True], ids=["distances", "normalised"])
def test_topk_equals_the_model(gpu_device, geometry, with_stats):
    from pyannote_audio_amd.identification import gallery_topk
    tile, _, max_k = geometry
    rng = np.random.default_rng(11 + with_stats)
    for k in (1, 8, max_k):
        for Ng in (k, tile + 1):
            for M, D in ((1, 3), (65, 3), (65, 256)):
                Q, G, stats = _gallery_case(rng, M, Ng, D, with_stats)
                Qd, Gd = _to_device(gpu_device, Q, G)
                stats_d = None if stats is None else _to_device(gpu_device, *stats)
                values, indices = gallery_topk(Qd, Gd, k, stats_d)
                values, indices = values.cpu().numpy(), indices.cpu().numpy()
                want_values, want_indices = model.topk(Q, G, k, stats)
                assert indices.dtype == np.int32 and _same(indices, want_indices), (k, Ng, M, D)
                assert _same(values, want_values), (k, Ng, M, D)
                if Ng > 1 and k > 1:
                    assert (np.diff(values, axis=1) == 0).any(), "the case has ties"
                if not with_stats:   # the raw values are SciPy's distances
                    from scipy.spatial.distance import cdist
                    assert _same(values, np.take_along_axis(cdist(Q, G, "cosine"), indices.astype(np.int64), axis=1))


def test_topk_refusals(gpu_device, geometry):
    from pyannote_audio_amd.identification import gallery_topk
    _, _, max_k = geometry
    Q = torch.ones((2, 4), dtype=torch.float64, device=gpu_device)
    G = torch.ones((max_k + 5, 4), dtype=torch.float64, device=gpu_device)
    for k in (0, max_k + 1):
        with pytest.raises(ValueError, match="k = "):
            gallery_topk(Q, G, k)
    with pytest.raises(ValueError, match="k = 3"):
        gallery_topk(Q, G[:2], 3)
    with pytest.raises(ValueError, match="all four or None"):
        gallery_topk(Q, G, 1, (Q[:, 0], Q[:, 0], None, None))


# ------------------------------------------------------------------------------------------------------------ pairs
@pytest.mark.parametrize("with_stats", [False, True], ids=["distances", "normalised"])
def test_pairs_equal_the_full_matrix(gpu_device, with_stats):
    from pyannote_audio_amd.identification import gallery_pairs
    rng = np.random.default_rng(21 + with_stats)
    for M, Ng, D, P in ((1, 1, 1, 1), (7, 300, 255, 1000), (65, 130, 256, 129)):
        Q, G, stats = _gallery_case(rng, M, Ng, D, with_stats)
        iq, ig = rng.integers(0, M, P).astype(np.int32), rng.integers(0, Ng, P).astype(np.int32)
        Qd, Gd, iqd, igd = _to_device(gpu_device, Q, G, iq, ig)
        stats_d = None if stats is None else _to_device(gpu_device, *stats)
        got = gallery_pairs(Qd, Gd, iqd, igd, stats_d).cpu().numpy()
        assert _same(got, model.pairs(Q, G, iq, ig, stats)), (M, Ng, D, P)
    # an index outside its table gives NaN and touches nothing
    iq, ig = np.array([0, M, -1, 0], dtype=np.int32), np.array([Ng, 0, 0, 1], dtype=np.int32)
    got = gallery_pairs(Qd, Gd, *_to_device(gpu_device, iq, ig), stats_d).cpu().numpy()
    assert np.isnan(got[:3]).all() and got[3] == model.values(Q, G, stats)[0, 1]


# --------------------------------------------------------------------------------------------------------- identify
@pytest.fixture(scope="module")
def identify_case():
    """a gallery of 400 voiceprints and four files: S = 1, 3 (one row a padded centroid, one row a NaN), 9 and 0.
    Some speakers are gallery entries plus noise, the rest are strangers."""
    rng = np.random.default_rng(31)
    D, G = 32, 400
    table = rng.standard_normal((G, D)).astype(np.float32)

    def speakers(S, enrolled):
        rows = rng.standard_normal((S, D)).astype(np.float32)
        for r, g in enrolled.items():
            rows[r] = table[g] + 0.3 * rng.standard_normal(D).astype(np.float32)
        return rows

    files = [speakers(1, {0: 17}), speakers(5, {0: 3, 2: 250}), speakers(9, {0: 8, 1: 9, 2: 399}),
             np.zeros((0, D), dtype=np.float32)]
    files[1][1] = 0.0            # a padded centroid
    files[1][4, 7] = np.nan
    cohort = rng.standard_normal((350, D)).astype(np.float32)
    return table, files, cohort


def _same_results(got, want):
    assert len(got) == len(want)
    for f, ((gi, gv), (wi, wv)) in enumerate(zip(got, want)):
        assert gi.dtype == np.int64 and _same(gi, wi), f"file {f}: {gi} != {wi}"
        assert _same(gv, wv), f"file {f}: {gv} != {wv}"


@pytest.mark.parametrize("with_cohort", [False, True], ids=["distances", "normalised"])
def test_identify_equals_the_model(gpu_device, identify_case, with_cohort):
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd.identification import Gallery, identify
    table, files, cohort = identify_case
    gallery = Gallery([f"speaker_{g}" for g in range(len(table))], table)
    kwargs = {}
    if with_cohort:
        gallery.normalise(cohort, top=300)
        want_mean, want_std, _ = model.cohort_stats(table, cohort, 300)
        assert _same(gallery.g_mean, want_mean) and _same(gallery.g_std, want_std)
        kwargs = {"cohort": cohort, "top": 300}
    # the S = 9 file is solved on the host: its candidates exceed what the device solver takes
    cost = model.values(files[2].astype(np.float64), table.astype(np.float64),
                        None if not with_cohort else
                        model.cohort_stats(files[2], cohort, 300)[:2] + (gallery.g_mean, gallery.g_std))
    assert len(model.restricted_assignment(cost)[1]) > ffi.load().pa_lsap_max_size()

    everyone = identify(files, gallery, **kwargs)
    want = model.identify(files, table, **kwargs)
    _same_results(everyone, want)
    index, value = everyone[1]
    assert index[1] == -1 and index[4] == -1 and np.isnan(value[[1, 4]]).all(), "rows without direction stay anonymous"
    assert everyone[0][0][0] == 17 and index[0] == 3 and index[2] == 250 and everyone[2][0][:3].tolist() == [8, 9, 399]
    assert (np.concatenate([i for i, _ in everyone]) >= 0).sum() == 1 + 3 + 9, "without a threshold every pair is accepted"
    # a threshold between the enrolled speakers' values and the strangers'
    scored = np.concatenate([v[~np.isnan(v)] for _, v in everyone])
    threshold = float(np.sort(scored)[6])
    some = identify(files, gallery, threshold=threshold, **kwargs)
    _same_results(some, model.identify(files, table, threshold=threshold, **kwargs))
    accepted = np.concatenate([i for i, _ in some]) >= 0
    assert accepted.sum() == 7 and _same(np.concatenate([v for _, v in some]), np.concatenate([v for _, v in everyone]))
    # file by file is the batched call
    for f, table_f in enumerate(files):
        _same_results(identify([table_f], gallery, threshold=threshold, **kwargs), [some[f]])
    # more speakers than gallery entries: some stay without a partner
    small = Gallery(["a", "b"], table[[3, 250]])
    _same_results(identify(files[:3], small), model.identify(files[:3], table[[3, 250]]))
    if with_cohort:
        with pytest.raises(ValueError, match="not normalised over this cohort"):
            identify(files, gallery, cohort=cohort[:340], top=300)
        constant = np.repeat(cohort[:1], 5, axis=0)
        with pytest.raises(ValueError, match="std == 0"):
            Gallery(["a", "b"], table[:2]).normalise(constant, top=2)     # (s + s) / 2 is exact
        with pytest.warns(UserWarning, match="every cohort row is used"):
            clipped = Gallery(["a", "b"], table[:2]).normalise(cohort[:40], top=300)
        assert clipped.top == 40 and _same(clipped.g_mean, model.cohort_stats(table[:2], cohort[:40], 40)[0])


# -------------------------------------------------------------------------------------------------------- enrolment
def test_enroll_takes_the_mean_of_each_speakers_files(gpu_device):
    """every file embedded once, in batches; a voiceprint is np.mean of its speaker's float32 embeddings, bit for bit"""
    import pyannote_audio_amd.model as pm
    from conftest import WESPEAKER_HPARAMS
    from oracle import seeded_wespeaker
    from pyannote_audio_amd import Gallery, SpeakerEmbedding
    model = pm.WeSpeakerResNet34(seeded_wespeaker(seed=4321).state_dict(), WESPEAKER_HPARAMS,
                                 pm.embedding_specifications()).to(gpu_device)
    pipeline = SpeakerEmbedding(embedding=model)
    g = torch.Generator().manual_seed(61)
    files = [{"waveform": 0.1 * torch.randn(1, n, generator=g), "sample_rate": 16000, "uri": f"u{i}"}
             for i, n in enumerate((16000, 24000, 20000, 16000))]
    speakers = {"ann": [files[0], files[2], files[3]], "ben": [files[1]]}
    gallery = Gallery.enroll(pipeline, speakers, batch_size=3)
    assert gallery.names == ["ann", "ben"] and gallery.voiceprints.shape == (2, 256)
    order = [files[0], files[2], files[3], files[1]]
    embedded = np.concatenate(pipeline.apply_batch(order[:3]) + pipeline.apply_batch(order[3:]))
    assert embedded.dtype == np.float32
    assert _same(gallery.voiceprints, np.stack([np.mean(embedded[:3], axis=0), embedded[3]]).astype(np.float64))
    with pytest.raises(ValueError, match="no enrolment file"):
        Gallery.enroll(pipeline, {"ann": []})


# ------------------------------------------------------------------------------------------------------- end to end
def _turns(annotation):
    return [(s.start, s.end, label) for s, _, label in annotation.itertracks(yield_label=True)]


def _on_binary_grid(annotation):
    """the same turns with their times rounded to multiples of 2^-10 s: every duration and every sum of durations is then
    exact in float64, so a metric that is 0 in exact arithmetic is 0.0 (see the end-to-end test)"""
    import pyannote_audio_amd as pa
    out = pa.Annotation(uri=annotation.uri)
    for segment, track, label in annotation.itertracks(yield_label=True):
        out[pa.Segment(round(segment.start * 1024) / 1024, round(segment.end * 1024) / 1024), track] = label
    return out


def test_speaker_identification_end_to_end(pipeline_dir, gpu_device):
    import pyannote_audio_amd as pa
    from oracle.synthetic import synth_conversation
    from pyannote_audio_amd.identification import IdentifiedOutput, valid_rows
    diarization = pa.Pipeline.from_pretrained(pipeline_dir).to(gpu_device)
    files = [{"waveform": synth_conversation(sec, seed=seed)[0], "sample_rate": 16000, "uri": f"f{seed}"}
             for sec, seed in ((33.0, 5), (12.0, 3))]
    plain = diarization(files[0])
    labels = plain.speaker_diarization.labels()
    centroids = plain.speaker_embeddings
    known = np.flatnonzero(valid_rows(centroids))
    assert len(labels) == len(centroids) and len(known) >= 1
    # the gallery: the file's own centroids in another order among distractors
    rng = np.random.default_rng(41)
    order = rng.permutation(len(known))
    distractors = rng.standard_normal((20, centroids.shape[1])).astype(np.float32)
    table = np.concatenate([distractors[:7], centroids[known][order], distractors[7:]])
    names = [f"stranger {i}" for i in range(7)] + [f"voice of row {known[o]}" for o in order] + \
            [f"stranger {i}" for i in range(7, 20)]
    gallery = pa.Gallery(names, table)
    cohort = rng.standard_normal((60, centroids.shape[1])).astype(np.float32)
    expected = {labels[r]: f"voice of row {r}" for r in known}
    reference = plain.speaker_diarization.rename_labels(mapping=expected)

    for kwargs in ({}, {"cohort": cohort, "top": 50}):
        enrolled = pa.Gallery(names, table)
        if kwargs:
            with pytest.raises(ValueError, match="not normalised over this cohort"):
                pa.SpeakerIdentification(diarization, enrolled, **kwargs).instantiate({"threshold": 0.5})(files[0])
            enrolled.normalise(cohort, top=50)
        pipeline = pa.SpeakerIdentification(diarization, enrolled, **kwargs)
        pipeline.instantiate({"threshold": 0.5})
        named = pipeline(files[0])
        assert isinstance(named, IdentifiedOutput)
        assert {label: name for label, (name, _) in named.matches.items()} == expected
        assert _turns(named.speaker_diarization) == _turns(reference)
        assert _turns(named.exclusive_speaker_diarization) == \
            _turns(plain.exclusive_speaker_diarization.rename_labels(mapping=expected))
        assert np.array_equal(named.speaker_embeddings, centroids)
        want = model.identify([centroids], table, threshold=0.5, **kwargs)[0]
        assert [named.matches[labels[r]][1] for r in known] == want[1][known].tolist()
        # IdentificationErrorRate against the renamed reference is 0.  The metric takes false alarm, miss and confusion as
        # differences of sums of the same durations added in different orders (`both - correct`), so on the pipeline's
        # own times, which are no binary fractions, identical annotations leave a rounding residue (-1.4e-16 here) where
        # exact arithmetic says 0.  Each of the sums has at most `cuts` terms no larger than `total`, so each carries at
        # most cuts * 2^-53 * total of rounding and a difference of two at most twice that: that, and nothing wider, is
        # what the components may show.  On a binary time grid every sum is exact and the rate is 0.0.
        metric = pipeline.get_metric()
        rate = metric(reference, named.speaker_diarization)
        cuts = 2 * (len(_turns(reference)) + len(_turns(named.speaker_diarization)))
        slack = 2 * cuts * 2.0 ** -53 * metric["total"]
        assert metric["total"] > 0
        for component in ("false alarm", "missed detection", "confusion"):
            assert abs(metric[component]) <= slack, (component, metric[component], slack)
        assert abs(metric["total"] - metric["correct"]) <= slack and abs(rate) <= 3 * slack / metric["total"]
        metric = pipeline.get_metric()
        assert metric(_on_binary_grid(reference), _on_binary_grid(named.speaker_diarization)) == 0.0
        assert metric["correct"] == metric["total"] > 0
        # a list of files: one set of launches for all of them, the results of the per-file calls
        batch = list(pipeline(files, pack=True))
        assert [f["uri"] for f, _ in batch] == ["f5", "f3"]
        for (f, got), file in zip(batch, files):
            alone = pipeline(file)
            assert _turns(got.speaker_diarization) == _turns(alone.speaker_diarization), f["uri"]
            assert _turns(got.exclusive_speaker_diarization) == _turns(alone.exclusive_speaker_diarization)
            assert got.matches == alone.matches and np.array_equal(got.speaker_embeddings, alone.speaker_embeddings)
    with pytest.raises(ValueError, match="joint_clustering"):
        list(pipeline(files, joint_clustering=True))
    # a threshold nobody meets: every speaker keeps its label, the values are still reported
    strict = pa.SpeakerIdentification(diarization, gallery).instantiate({"threshold": -1.0})(files[0])
    assert _turns(strict.speaker_diarization) == _turns(plain.speaker_diarization)
    assert all(name is None for name, _ in strict.matches.values()) and len(strict.matches) == len(known)
    # a gallery entry named like a label the file keeps: the first speaker is accepted under the last speaker's label,
    # the last speaker finds only strangers and keeps it
    if len(known) >= 2:
        first, last = known[0], known[-1]
        clash = pa.Gallery([labels[last]] + [f"stranger {i}" for i in range(20)],
                           np.concatenate([centroids[first:first + 1], distractors]))
        with pytest.raises(ValueError, match="equal anonymous speaker label"):
            pa.SpeakerIdentification(diarization, clash).instantiate({"threshold": 0.5})(files[0])


# ------------------------------------------------------------------------------------------------ hostile workspace
def test_hostile_workspace(gpu_device, geometry):
    """the two workspace-taking entry points on workspaces of exactly the queried size filled with 0x00, 0xFF and +-1e30:
    the same output bytes, untouched guards, and the model's values on the 0xFF run"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    tile, _, _ = geometry
    rng = np.random.default_rng(51)
    M, N, D, K, k = 9, tile + 5, 19, 37, 8
    Q, G, stats = _gallery_case(rng, M, N, D, True)
    Qd, Gd = _to_device(gpu_device, Q, G)
    sd = _to_device(gpu_device, *stats)

    with torch.cuda.device(gpu_device):
        def stats_call(ws, nbytes, mean, std, status):
            return lib.pa_cohort_stats_f64(ffi.ptr(Qd), M, ffi.ptr(Gd), N, D, K, mean, std, status, ws, nbytes,
                                           ffi.stream())
        need = lib.pa_cohort_stats_workspace_bytes(M, N, D)
        mean, std, status = run_under_fills(stats_call, need, [((M,), torch.float64), ((M,), torch.float64),
                                                               ((M,), torch.int32)], gpu_device, "pa_cohort_stats_f64")
        want = model.cohort_stats(Q, G, K)
        assert _same(mean.numpy(), want[0]) and _same(std.numpy(), want[1]) and _same(status.numpy(), want[2])

        def topk_call(ws, nbytes, values, indices):
            return lib.pa_gallery_topk_f64(ffi.ptr(Qd), M, ffi.ptr(Gd), N, D, *[ffi.ptr(s) for s in sd], k, values,
                                           indices, ws, nbytes, ffi.stream())
        need = lib.pa_gallery_workspace_bytes(M, N, D)
        values, indices = run_under_fills(topk_call, need, [((M, k), torch.float64), ((M, k), torch.int32)], gpu_device,
                                          "pa_gallery_topk_f64")
        want = model.topk(Q, G, k, stats)
        assert _same(values.numpy(), want[0]) and _same(indices.numpy(), want[1])

        # the pairs call takes no workspace; a selecting call given one byte less than it asked for is refused
        work = torch.empty(need, dtype=torch.uint8, device=gpu_device)
        values = torch.empty((M, k), dtype=torch.float64, device=gpu_device)
        indices = torch.empty((M, k), dtype=torch.int32, device=gpu_device)
        assert lib.pa_gallery_topk_f64(ffi.ptr(Qd), M, ffi.ptr(Gd), N, D, None, None, None, None, k, ffi.ptr(values),
                                       ffi.ptr(indices), ffi.ptr(work), need - 1, ffi.stream()) == 3
