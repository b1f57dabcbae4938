"""GPU: csrc/metrics.hip through the C entry points and through pyannote_audio_amd.metrics, against the truth
(tests/metrics_truth.py, numpy int64) with `==`, and against the reference's own outputs (tests/golden/metrics_v1.npz)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import metrics_truth  # noqa: E402
from test_metrics_cpu import KEYS, chunk_case  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "metrics_v1.npz")))


def c_der_counts(ref, hyp, keep=None):
    """pa_der_counts itself -> the int64 output block on the host"""
    import pyannote_audio_amd.ffi as ffi
    Sr, Sh = ref.shape[1], hyp.shape[1]
    out = torch.full((Sr * Sh + Sr + Sh + 4,), -7, dtype=torch.int64, device=ref.device)
    ffi.check(ffi.load().pa_der_counts(ffi.ptr(ref), ffi.ptr(hyp), ffi.ptr(keep), ref.shape[0], Sr, Sh, ffi.ptr(out),
                                       ffi.stream()), "pa_der_counts")
    return out.cpu().numpy()


def flat(counts):
    return np.concatenate([np.asarray(counts["cooc"]).reshape(-1), counts["ref_frames"], counts["hyp_frames"],
                           [counts["total"], counts["false_alarm"], counts["missed"], counts["both"]]])


FILE_SHAPES = [(1, 3, 3), (63, 1, 7), (64, 3, 3), (65, 7, 3), (589, 3, 7), (589, 32, 1), (65, 32, 32),
               (213334, 3, 3), (213334, 7, 32), (213334, 32, 32)]


@pytest.mark.parametrize("T,Sr,Sh", FILE_SHAPES)
def test_file_mode_counts_equal_truth(gpu_device, T, Sr, Sh):
    from pyannote_audio_amd import metrics
    rng = np.random.default_rng(T * 1000 + Sr * 33 + Sh)
    density = 0.3 if max(Sr, Sh) <= 7 else 0.12
    ref = (rng.random((T, Sr)) < density).astype(np.uint8)
    hyp = (rng.random((T, Sh)) < density).astype(np.uint8)
    hyp[:, : min(Sr, Sh)] = np.where(rng.random((T, min(Sr, Sh))) < 0.7, ref[:, : min(Sr, Sh)], hyp[:, : min(Sr, Sh)])
    keep = (rng.random(T) < 0.6).astype(np.uint8)
    d_ref, d_hyp, d_keep = (torch.from_numpy(a).to(gpu_device) for a in (ref, hyp, keep))
    for mask, d_mask in ((None, None), (keep, d_keep), (np.zeros(T, np.uint8), torch.zeros_like(d_keep))):
        want = metrics_truth.der_counts(ref, hyp, keep=mask)
        first = c_der_counts(d_ref, d_hyp, d_mask)
        assert np.array_equal(first, flat(want))
        assert np.array_equal(c_der_counts(d_ref, d_hyp, d_mask), first)          # bit-identical when repeated
        got = metrics.der_counts(d_ref, d_hyp, keep=d_mask)
        assert np.array_equal(flat(got), flat(want))
        assert metrics.components_from_counts(got) == metrics_truth.file_components(ref, hyp, keep=mask)
    if T == 213334:
        assert want["total"] == 0 and metrics_truth.der_counts(ref, hyp)["total"] > 65504   # beyond np.half's largest
    # the public function: host arrays and device tensors alike, Python ints and a float64 quotient
    der, components = metrics.discrete_diarization_error_rate(ref, hyp)
    assert components == metrics_truth.file_components(ref, hyp)
    assert all(type(v) is int for v in components.values()) and type(der) is float
    der2, components2 = metrics.discrete_diarization_error_rate(d_ref, d_hyp.to(torch.float32))
    assert components2 == components and (der2 == der or (np.isnan(der) and np.isnan(der2)))
    if components["total"]:
        errors = components["false alarm"] + components["missed detection"] + components["confusion"]
        assert der == errors / components["total"]


@pytest.mark.parametrize("T,S", [(64, 3), (65, 32), (213334, 7)])
def test_file_mode_all_zero_and_all_one(gpu_device, T, S):
    for value in (0, 1):
        a = np.full((T, S), value, dtype=np.uint8)
        want = flat(metrics_truth.der_counts(a, a))
        got = c_der_counts(torch.from_numpy(a).to(gpu_device), torch.from_numpy(a).to(gpu_device))
        assert np.array_equal(got, want)
        assert got[-4] == value * T * S


def test_file_mode_equals_the_reference(gpu_device, golden):
    from pyannote_audio_amd import metrics
    metric = metrics.DiscreteDiarizationErrorRate()
    for name in golden["file_cases"]:
        reference, hypothesis = golden[f"file/{name}/reference"], golden[f"file/{name}/hypothesis"]
        got = metric.compute_components(reference, torch.from_numpy(hypothesis).to(gpu_device))
        assert [got[k] for k in KEYS] == golden[f"file/{name}/components"].tolist(), name


def c_der_chunks(preds, target, thresholds, perm=None):
    import pyannote_audio_amd.ffi as ffi
    B, S, F = preds.shape
    Q = thresholds.shape[0]
    counts = torch.full((B, Q, 3), -7, dtype=torch.int32, device=preds.device)
    total = torch.full((B,), -7, dtype=torch.int32, device=preds.device)
    ffi.check(ffi.load().pa_der_chunks(ffi.ptr(preds), ffi.ptr(target), int(target.dtype == torch.float32), B, S, F,
                                       ffi.ptr(thresholds), Q, ffi.ptr(perm), ffi.ptr(counts), ffi.ptr(total),
                                       ffi.stream()), "pa_der_chunks")
    return counts.cpu().numpy().astype(np.int64), total.cpu().numpy().astype(np.int64)


def seeded_chunks(B, S, F, seed):
    """0/1 targets in runs, scores that follow a shuffled copy of them with 15 % of the frames flipped"""
    rng = np.random.default_rng(seed)
    change = rng.random((B, S, F)) < 0.01
    target = ((np.cumsum(change, axis=2) + rng.integers(0, 2, (B, S, 1))) % 2).astype(np.uint8)
    on = np.where(rng.random(target.shape) < 0.15, 1 - target, target)
    preds = np.where(on == 1, rng.uniform(0.4, 1.0, target.shape), rng.uniform(0.0, 0.6, target.shape))
    order = np.argsort(rng.random((B, S)), axis=1)
    preds = np.take_along_axis(preds, order[:, :, None], axis=1).astype(np.float32)
    return preds, target


@pytest.mark.parametrize("S,F,Q", [(1, 589, 51), (2, 589, 1), (3, 589, 51), (4, 589, 64), (3, 293, 51), (4, 77, 1),
                                   (1, 1, 64)])
def test_chunk_mode_counts_equal_truth(gpu_device, S, F, Q):
    preds, target = seeded_chunks(37, S, F, seed=S * 1000 + F + Q)
    thresholds = np.linspace(0.0, 1.0, Q).astype(np.float32) if Q > 1 else np.array([0.5], np.float32)
    # scores exactly on thresholds: `>` is strict
    rng = np.random.default_rng(F)
    sel = rng.random(preds.shape) < 0.2
    preds[sel] = thresholds[rng.integers(0, Q, int(sel.sum()))]
    want_counts, want_total = metrics_truth.chunk_components(preds, target, thresholds)
    _, gap, tied = metrics_truth.chunk_permutations(preds, target)
    # float64 on both sides, so no chunk is left out: permutations that do not tie are far apart, and the exact ties
    # (two target rows that are equal, e.g. both silent) give the same counts whichever is taken
    assert gap.min() > 1e-9
    d = [torch.from_numpy(a).to(gpu_device) for a in (preds, target, thresholds)]
    counts, total = c_der_chunks(*d)
    assert np.array_equal(counts, want_counts) and np.array_equal(total, want_total)
    again = c_der_chunks(*d)
    assert np.array_equal(again[0], counts) and np.array_equal(again[1], total)
    # float32 targets take the other instantiation
    counts, total = c_der_chunks(d[0], d[1].to(torch.float32), d[2])
    assert np.array_equal(counts, want_counts) and np.array_equal(total, want_total)
    # a permutation from the caller
    perm = metrics_truth.chunk_permutations(preds, target)[0]
    counts, total = c_der_chunks(*d, perm=torch.from_numpy(perm).to(gpu_device))
    assert np.array_equal(counts, want_counts) and np.array_equal(total, want_total)


@pytest.mark.parametrize("S,F", [(5, 589), (8, 2000), (32, 589)])
def test_chunk_mode_with_a_passed_permutation(gpu_device, S, F):
    """more than 4 speakers: the permutation comes from the existing `permutate`; (8, 2000) and (32, 589) do not fit
    the LDS stage and read the chunk again through the L2"""
    from pyannote_audio_amd import metrics
    from pyannote_audio_amd.permutation import permutate
    preds, target = seeded_chunks(9, S, F, seed=S + F)
    thresholds = torch.linspace(0.0, 1.0, 51)
    _, found = permutate(np.transpose(target, (0, 2, 1)).astype(np.float32), np.transpose(preds, (0, 2, 1)))
    perm = np.array(found, dtype=np.int32)
    want_counts, want_total = metrics_truth.chunk_components(preds, target, thresholds.numpy(), perm=perm)
    d_preds, d_target = torch.from_numpy(preds).to(gpu_device), torch.from_numpy(target).to(gpu_device)
    counts, total = c_der_chunks(d_preds, d_target, thresholds.to(gpu_device), torch.from_numpy(perm).to(gpu_device))
    assert np.array_equal(counts, want_counts) and np.array_equal(total, want_total)
    der, (fa, md, conf, tot) = metrics.diarization_error_rate(d_preds, d_target, threshold=thresholds,
                                                              reduce="chunk", return_components=True)
    assert np.array_equal(torch.stack([fa, md, conf], dim=-1).cpu().numpy(), want_counts)
    assert np.array_equal(tot.cpu().numpy(), want_total)
    # without a permutation the C entry point refuses more than four speakers
    import pyannote_audio_amd.ffi as ffi
    with pytest.raises(ValueError, match="need a permutation"):
        c_der_chunks(d_preds, d_target, thresholds.to(gpu_device))
    assert ffi.load().pa_last_error()


def test_chunk_mode_equals_the_reference(gpu_device, golden):
    """components == the reference's on every chunk that is not a near-tie of its float32 permutation cost; the rate
    within float32 rounding of the reference's float32 quotient"""
    from pyannote_audio_amd import metrics
    # the reference computes fl32(errors / fl32(total + 1e-8)) from exactly represented sums; ours is the float64
    # quotient with a float64 1e-8.  Three roundings separate them: fl32 of total + 1e-8 (relative <= 2^-24; it
    # also absorbs the 1e-8, relative <= 1e-8 for total >= 1), the float32 division (<= 2^-24), and the float32
    # value of the constant 1e-8 when total = 0 (<= 2^-24): 3 * 2^-24 relative, with room for ours (2^-52).
    bound = 3 * 2.0 ** -24 + 1e-8
    for name in golden["chunk_cases"]:
        preds, target, thresholds, scalar, near = chunk_case(golden, name)
        raw_preds = torch.from_numpy(golden[f"chunk/{name}/preds"].astype(np.float32)).to(gpu_device)
        raw_target = torch.from_numpy(golden[f"chunk/{name}/target"]).to(gpu_device)
        threshold = float(golden[f"chunk/{name}/thresholds"]) if scalar else torch.from_numpy(thresholds)
        keep = ~near
        for reduce in ("batch", "chunk"):
            der, components = metrics.diarization_error_rate(raw_preds, raw_target, threshold=threshold,
                                                             reduce=reduce, return_components=True)
            assert der.dtype == torch.float64 and all(c.dtype == torch.int64 for c in components)
            for key, value in zip(("false_alarm", "missed_detection", "confusion", "total"), components):
                want = golden[f"chunk/{name}/{reduce}_{key}"]
                assert tuple(value.shape) == want.shape, (name, reduce, key)
                if reduce == "chunk":
                    assert np.array_equal(value.cpu().numpy()[keep], want[keep]), (name, reduce, key)
                elif not near.any() or key == "total":
                    assert np.array_equal(value.cpu().numpy(), want), (name, reduce, key)
            if f"chunk/{name}/{reduce}_der" in golden and not near.any():
                want = golden[f"chunk/{name}/{reduce}_der"].astype(np.float64)
                got = der.cpu().numpy()
                assert got.shape == want.shape
                assert (np.abs(got - want) <= bound * np.abs(got)).all(), (name, reduce)
        if not scalar:
            opt, at = metrics.optimal_diarization_error_rate(raw_preds, raw_target, threshold=torch.from_numpy(thresholds))
            batch = metrics.diarization_error_rate(raw_preds, raw_target, threshold=torch.from_numpy(thresholds))
            assert opt == batch.min() and at == torch.from_numpy(thresholds).to(gpu_device)[batch.argmin()]
    # exact ties were part of it and none of them was left out
    assert not golden["chunk/duplicate_rows_S3_F293_Q51/near_tie"].any()


def test_chunk_mode_one_audio_hour_inside_the_memory_bound(gpu_device):
    """B = 7 176 chunks of 3 x 589 scores at 51 thresholds: every reduction equals the truth, the calls repeat
    bit for bit, and device memory rises by the outputs plus the workspace the library reports -- nothing of the
    size of the (B, S, F, Q) arrays of the definition (2.6 GB each in float32)"""
    from pyannote_audio_amd import metrics
    B, S, F, Q = 7176, 3, 589, 51
    preds, target = seeded_chunks(B, S, F, seed=7176)
    thresholds = torch.linspace(0.0, 1.0, Q)
    want_counts, want_total = metrics_truth.chunk_components(preds, target, thresholds.numpy())
    d_preds, d_target = torch.from_numpy(preds).to(gpu_device), torch.from_numpy(target).to(gpu_device)
    d_thresholds = thresholds.to(gpu_device)
    metrics.diarization_error_rate(d_preds[:2], d_target[:2], threshold=d_thresholds)      # (library loaded, warm)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()          # (a cached block larger than a request would be counted at its own size)
    torch.cuda.reset_peak_memory_stats(gpu_device)
    before = torch.cuda.memory_allocated(gpu_device)
    der, (fa, md, conf, tot) = metrics.diarization_error_rate(d_preds, d_target, threshold=d_thresholds,
                                                              return_components=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(gpu_device) - before
    workspace = metrics.chunk_workspace_bytes(B, Q)
    assert workspace == 4 * B * (3 * Q + 1)                       # grows with B * Q, not with F * Q
    # outputs: the (3 Q + 1) int64 sums and the (Q,) float64 rate; on the way to the rate at most eight more tensors
    # of at most Q 64-bit values are alive.  The allocator hands out multiples of 512 bytes.
    block = lambda n: -(-n // 512) * 512                                              # noqa: E731
    outputs = block(8 * (3 * Q + 1)) + block(8 * Q)
    assert rise <= block(workspace) + outputs + 8 * block(8 * Q), (rise, workspace, outputs)
    assert rise < 2 * workspace and workspace < B * S * F * Q * 4 // 500
    assert np.array_equal(torch.stack([fa, md, conf], dim=-1).cpu().numpy(), want_counts.sum(axis=0))
    assert int(tot) == int(want_total.sum())
    errors = want_counts.sum(axis=0).sum(axis=1)
    assert np.array_equal(der.cpu().numpy(), errors.astype(np.float64) / (np.float64(want_total.sum()) + 1e-8))
    again = metrics.diarization_error_rate(d_preds, d_target, threshold=d_thresholds, return_components=True)
    assert torch.equal(again[0], der) and all(torch.equal(a, b) for a, b in zip(again[1], (fa, md, conf, tot)))
    # per chunk
    der_c, (fa, md, conf, tot) = metrics.diarization_error_rate(d_preds, d_target, threshold=d_thresholds,
                                                                reduce="chunk", return_components=True)
    assert np.array_equal(torch.stack([fa, md, conf], dim=-1).cpu().numpy(), want_counts)
    assert np.array_equal(tot.cpu().numpy(), want_total) and der_c.shape == (B, Q)
    # scalar threshold: the last axis goes
    der_s, parts = metrics.diarization_error_rate(d_preds, d_target, threshold=0.5, return_components=True)
    assert der_s.shape == () and all(p.shape == () for p in parts)
    mid = metrics_truth.chunk_components(preds, target, np.array([0.5], np.float32))[0].sum(axis=0)[0]
    assert [int(p) for p in parts[:3]] == mid.tolist()
    # more than 64 thresholds: split over launches
    wide = torch.linspace(0.0, 1.0, 101)
    got = metrics.diarization_error_rate(d_preds[:50], d_target[:50], threshold=wide, return_components=True)[1]
    want = metrics_truth.chunk_components(preds[:50], target[:50], wide.numpy())
    assert np.array_equal(torch.stack(got[:3], dim=-1).cpu().numpy(), want[0].sum(axis=0))
    assert int(got[3]) == int(want[1].sum())


def test_stateful_classes(gpu_device):
    from pyannote_audio_amd import metrics
    preds, target = seeded_chunks(60, 3, 293, seed=11)
    d_preds, d_target = torch.from_numpy(preds).to(gpu_device), torch.from_numpy(target).to(gpu_device)
    counts, total = metrics_truth.chunk_components(preds, target, np.array([0.5], np.float32))
    fa, md, conf = (int(v) for v in counts.sum(axis=0)[0])
    tot = float(total.sum()) + 1e-8
    want = {metrics.DiarizationErrorRate: (fa + md + conf) / tot, metrics.SpeakerConfusionRate: conf / tot,
            metrics.FalseAlarmRate: fa / tot, metrics.MissedDetectionRate: md / tot,
            metrics.DetectionErrorRate: (fa + md) / tot,
            metrics.DiarizationPrecision: (total.sum() - md - conf) / (float(total.sum() - md) + 1e-8),
            metrics.DiarizationRecall: (total.sum() - md - conf) / tot}
    for klass, value in want.items():
        metric = klass(threshold=0.5)
        for lo in range(0, 60, 20):                      # three batches accumulate into integer device state
            metric.update(d_preds[lo:lo + 20], d_target[lo:lo + 20])
        assert metric.speech_total.dtype == torch.int64 and metric.speech_total.is_cuda
        assert float(metric.compute()) == value, klass.__name__
        metric.reset()
        assert int(metric.speech_total) == 0
    thresholds = torch.linspace(0.0, 1.0, 51)
    counts, total = metrics_truth.chunk_components(preds, target, thresholds.numpy())
    sums = counts.sum(axis=0)
    der = sums.sum(axis=1) / (float(total.sum()) + 1e-8)
    best = int(np.argmin(der))
    for klass, value in {metrics.OptimalDiarizationErrorRate: der[best],
                         metrics.OptimalDiarizationErrorRateThreshold: float(thresholds[best]),
                         metrics.OptimalFalseAlarmRate: sums[best, 0] / (float(total.sum()) + 1e-8),
                         metrics.OptimalMissedDetectionRate: sums[best, 1] / (float(total.sum()) + 1e-8),
                         metrics.OptimalSpeakerConfusionRate: sums[best, 2] / (float(total.sum()) + 1e-8)}.items():
        metric = klass()
        for lo in range(0, 60, 30):
            metric.update(d_preds[lo:lo + 30], d_target[lo:lo + 30])
        assert float(metric.compute()) == value, klass.__name__
    # windows of 100 frames every 50: the same counts as the unfolded batch
    windowed = metrics.SegmentationErrorRate(window_size=100, step_size=50)
    windowed.update(d_preds, d_target)
    p = np.stack([preds[:, :, lo:lo + 100] for lo in range(0, 293 - 99, 50)], axis=1).reshape(-1, 3, 100)
    t = np.stack([target[:, :, lo:lo + 100] for lo in range(0, 293 - 99, 50)], axis=1).reshape(-1, 3, 100)
    counts, total = metrics_truth.chunk_components(p, t, np.array([0.5], np.float32))
    assert int(windowed.speech_total) == int(total.sum())
    assert [int(windowed.false_alarm), int(windowed.missed_detection), int(windowed.speaker_confusion)] \
        == counts.sum(axis=0)[0].tolist()


def test_pipeline_output_scored_on_the_device(pipeline_dir, gpu_device):
    """SpeakerDiarization on a synthetic conversation; its `discrete_diarization` artifact, as a device tensor, against
    the conversation's true turns: DiscreteDiarizationErrorRate equals the truth computed from the host copy"""
    import pyannote_audio_amd as pa
    from oracle.synthetic import synth_conversation
    from pyannote_audio_amd.core import Annotation, Segment, SlidingWindowFeature
    wav, activity = synth_conversation(33.0, seed=5)
    pipeline = pa.Pipeline.from_pretrained(pipeline_dir).to(gpu_device)
    seen = {}

    def hook(step, artifact, file=None, total=None, completed=None):
        if step == "discrete_diarization" and artifact is not None:
            seen[step] = artifact
    pipeline({"waveform": wav, "sample_rate": 16000, "uri": "synth"}, hook=hook)
    discrete = seen["discrete_diarization"]
    reference = Annotation(uri="synth")
    activity = np.asarray(activity)
    for s in range(activity.shape[0]):
        edges = np.flatnonzero(np.diff(np.concatenate([[0], activity[s].astype(np.int8), [0]])))
        for a, b in zip(edges[0::2], edges[1::2]):
            reference[Segment(a / 16000.0, b / 16000.0), f"{s}_{a}"] = f"speaker{s}"
    assert len(reference.labels()) == activity.shape[0]
    host = np.asarray(discrete.data)
    on_device = SlidingWindowFeature(torch.from_numpy(host).to(gpu_device), discrete.sliding_window)
    metric = pa.DiscreteDiarizationErrorRate()
    value = metric(reference, on_device, detailed=True)
    truth = reference.discretize(discrete.extent, resolution=discrete.sliding_window).data
    common = min(len(truth), len(host))
    want = metrics_truth.file_components(truth[:common], host[:common])
    assert {k: value[k] for k in KEYS} == want and want["total"] > 1000
    errors = want["false alarm"] + want["missed detection"] + want["confusion"]
    assert abs(metric) == errors / want["total"] and abs(metric) < 1.0
    # the host copy gives the same numbers, and a uem over the middle of the file fewer frames
    assert metric(reference, discrete, detailed=True)["total"] == want["total"]
    inner = metric(reference, on_device, uem=[Segment(5.0, 25.0)], detailed=True)
    assert 0 < inner["total"] < want["total"]
    print(f"metrics: synthetic pipeline DER components {want}")
