"""GPU: `pa_annot_counts` (csrc/annot_metrics.hip) and `annotation_counts(..., device=cuda)` against the exact truth
of tests/annotation_metrics_truth.py.

Dyadic cases (every boundary and every collar boundary a multiple of 2^-10 s below 4096 s; the generator asserts
it) make every partial sum exactly representable, so all fields are compared with `==`.  The non-dyadic cases carry
a bound derived from the number of elementary intervals."""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import annotation_metrics_truth as truth

pytestmark = pytest.mark.gpu

# the sizes at which the kernels change shape: all four kernels run 256 threads per workgroup, one element each, and
# sweep the other side in LDS tiles of 256 (k_annot_rank: cuts; k_annot_intervals: items = segments + uem regions
# + collars); the reduction strides 256 lanes over the cuts - 1 intervals.  The number of cuts is always even.
TILE = 256


def _raw(case, device, ws_bytes=None, out=None):
    """the raw entry point on a case of the truth module -> (rc, float64 device tensor)"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    ref, hyp, uem = case["ref"], case["hyp"], case["uem"]
    Kr, Kh = case["Kr"], case["Kh"]

    def f64(rows):
        return torch.tensor([[a, b] for a, b, *_ in rows], dtype=torch.float64).reshape(-1, 2).to(device)

    def i32(rows):
        return torch.tensor([l for _, _, l in rows], dtype=torch.int32).to(device)

    ref_seg, hyp_seg, uem_seg, ref_lab, hyp_lab = f64(ref), f64(hyp), f64(uem), i32(ref), i32(hyp)
    need = int(lib.pa_annot_counts_workspace_bytes(len(ref), len(hyp), len(uem)))
    ws = torch.empty(max(need if ws_bytes is None else ws_bytes, 1), dtype=torch.uint8, device=device)
    if out is None:
        out = torch.full((max(Kr, 0) * max(Kh, 0) + max(Kr, 0) + max(Kh, 0) + 7,), float("nan"), dtype=torch.float64,
                         device=device)
    ptr = lambda t: ffi.ptr(t) if t.numel() else None  # noqa: E731
    with torch.cuda.device(device):
        rc = lib.pa_annot_counts(ptr(ref_seg), ptr(ref_lab), len(ref), Kr, ptr(hyp_seg), ptr(hyp_lab), len(hyp), Kh,
                                 ptr(uem_seg), len(uem), float(case["collar"]), int(case["skip_overlap"]),
                                 ffi.ptr(out), ffi.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                 ffi.stream())
        torch.cuda.synchronize()
    return rc, out


def _exact(case, device):
    truth.assert_dyadic(case)
    rc, out = _raw(case, device)
    assert rc == 0
    got = [Fraction(v) for v in out.cpu().tolist()]
    want = truth.flat(truth.case_truth(case))
    assert got == want
    return out


def _case(ref, hyp, uem, Kr, Kh, collar=0.0, skip_overlap=False):
    return {"ref": ref, "hyp": hyp, "uem": uem, "Kr": Kr, "Kh": Kh, "collar": collar, "skip_overlap": skip_overlap}


@pytest.mark.parametrize("Nr,Nh,Nu", [(0, 9, 2), (9, 0, 2), (9, 9, 0), (0, 0, 0), (0, 0, 3), (1, 0, 1), (1, 1, 1)])
@pytest.mark.parametrize("collar", [0.0, 0.5])
def test_empty_sides_and_single_segments(gpu_device, Nr, Nh, Nu, collar):
    case = truth.random_dyadic_case(11, Nr, Nh, Nu, Kr=3 if Nr else 0, Kh=2 if Nh else 0, collar=collar, span=8.0)
    out = _exact(case, gpu_device)
    if Nu == 0 or (Nr == 0 and Nh == 0):
        assert not out.any()


def test_hand_built_edges(gpu_device):
    """segments that touch, boundaries shared between reference, hypothesis and uem (duplicate cuts), a uem of
    several regions that cuts segments in the middle, a segment wholly outside the uem, collars that overlap each
    other and reach outside the uem, same-label tracks that overlap, zero-length segments"""
    ref = [(2.0, 4.0, 0), (4.0, 6.0, 0), (4.0, 8.0, 1), (8.0, 8.25, 2), (8.25, 8.5, 2), (20.0, 22.0, 1),
           (3.0, 5.0, 0), (7.0, 7.0, 2)]
    hyp = [(2.0, 4.0, 1), (4.0, 9.0, 0), (6.0, 8.0, 1), (20.0, 22.0, 0), (30.0, 31.0, 1), (8.5, 8.5, 0)]
    uem = [(2.0, 5.0), (4.5, 7.0), (7.5, 8.5), (12.0, 12.0), (21.0, 40.0)]
    for collar in (0.0, 0.25, 0.5, 1.0, 4.0):                    # 1.0: collars around 8, 8.25, 8.5 overlap
        for skip in (False, True):
            _exact(_case(ref, hyp, uem, 3, 2, collar, skip), gpu_device)
    # a uem that starts inside a collar; the collar around 2.0 reaches out of it
    _exact(_case(ref, hyp, [(1.875, 30.5)], 3, 2, 0.5), gpu_device)
    # reference and hypothesis identical: nothing but `both`
    out = _exact(_case(ref, [r for r in ref], [(0.0, 64.0)], 3, 3), gpu_device)
    n0 = 9 + 3 + 3
    total, false_alarm, missed, both = out[n0:n0 + 4].tolist()
    assert false_alarm == 0.0 and missed == 0.0 and total == both > 0.0


def test_64_labels_on_both_sides(gpu_device):
    """bit 63 of both masks is used; with everybody on at once Nr = Nh = 64"""
    case = truth.random_dyadic_case(3, Nr=150, Nh=140, Nu=3, Kr=64, Kh=64, collar=0.125, span=16.0)
    case["ref"] += [(2.0, 3.0, l) for l in range(64)]
    case["hyp"] += [(2.5, 3.5, l) for l in range(64)]
    case["uem"] += [(1.0, 4.0)]
    out = _exact(case, gpu_device)
    assert out[63 * 64 + 63].item() > 0.0                       # cooc[63][63]
    _exact(dict(case, skip_overlap=True), gpu_device)


@pytest.mark.parametrize("name,Nr,Nh,Nu,collar", [
    ("254 cuts: one workgroup, one tile, two cuts short", 60, 60, 7, 0.0),
    ("256 cuts: exactly one workgroup and one tile; 255 intervals", 60, 60, 8, 0.0),
    ("258 cuts: a second workgroup and a second tile of two; 257 intervals", 60, 61, 8, 0.0),
    ("254 cuts with collars", 30, 30, 7, 0.25),
    ("256 cuts with collars", 30, 30, 8, 0.25),
    ("258 cuts with collars", 30, 30, 9, 0.25),
    ("255 items, 510 cuts", 120, 127, 8, 0.0),
    ("256 items: one full item tile; 512 cuts: two full cut tiles", 120, 128, 8, 0.0),
    ("257 items, 514 cuts", 120, 129, 8, 0.0),
    ("255 items with collars", 60, 70, 5, 0.5),
    ("256 items with collars", 60, 70, 6, 0.5),
    ("257 items with collars", 60, 70, 7, 0.5),
    ("four workgroups", 130, 120, 6, 0.125),
])
@pytest.mark.parametrize("skip", [False, True])
def test_sizes_where_the_kernels_change_shape(gpu_device, name, Nr, Nh, Nu, collar, skip):
    cuts = 2 * (Nr + Nh + Nu) + (4 * Nr if collar else 0)
    items = Nr + Nh + Nu + (2 * Nr if collar else 0)
    numbers = [int(w) for w in name.replace(":", " ").replace(",", " ").split() if w.isdigit()]
    if "cuts" in name:
        assert cuts in numbers
    if "items" in name:
        assert items in numbers
    assert abs(cuts - TILE) <= 2 or abs(items - TILE) <= 1 or abs(cuts - 2 * TILE) <= 2 or cuts > 3 * TILE
    case = truth.random_dyadic_case(len(name) + Nu, Nr, Nh, Nu, Kr=4, Kh=5, collar=collar, skip_overlap=skip,
                                    span=32.0)
    _exact(case, gpu_device)


@functools.lru_cache(maxsize=None)
def _non_dyadic(collar, skip):
    """uniform random float64 boundaries, 300 segments per side, 8 labels.  With a collar the boundaries lie in
    [16, 31.5): there t -/+ collar / 2 is exact in float64 (2^-7 is a multiple of every ulp involved), so the
    kernel's collar boundaries are the truth's; the segments are short there, so that collars and overlap leave
    something to evaluate."""
    rng = np.random.default_rng(7)
    lo, hi = (16.0, 31.5) if collar else (0.0, 3600.0)

    def side():
        a = rng.uniform(lo, hi, 300)
        b = np.minimum(a + rng.uniform(0.0, (hi - lo) / (400.0 if collar else 40.0), 300), np.nextafter(hi, 0.0))
        return [(float(x), float(y), int(l)) for x, y, l in zip(a, b, rng.integers(0, 8, 300))]

    case = _case(side(), side(), [(lo + (hi - lo) * 0.01, lo + (hi - lo) * 0.6), (lo + (hi - lo) * 0.7, hi)], 8, 8,
                 collar, skip)
    return case, truth.case_truth(case)


@pytest.mark.parametrize("collar,skip", [(0.0, False), (2.0 ** -6, True)])
def test_non_dyadic_within_the_derived_bound(gpu_device, collar, skip):
    """Here the sums round.  Every term is non-negative.  An interval's length is one rounded subtraction and its
    term one rounded product with a small integer: relative error < 2 * 2^-53.  A sum of n such terms, in whatever
    fixed order, adds at most n - 1 roundings of partial sums that never exceed the (rounded) total: altogether
    |got - truth| <= (n + 1) * 2^-53 * truth * (1 + tiny) <= n * 2^-52 * truth per field, n = elementary intervals."""
    case, want = _non_dyadic(collar, skip)
    rc, out = _raw(case, gpu_device)
    assert rc == 0
    n = want["intervals"]
    assert n > 600
    worst = Fraction(0)
    for got, t in zip(out.cpu().tolist(), truth.flat(want)):
        bound = n * Fraction(1, 2 ** 52) * t
        error = abs(Fraction(got) - t)
        assert error <= bound, (got, float(t), float(error), float(bound))
        if t:
            worst = max(worst, error / t)
    print(f"non-dyadic (collar {collar}, skip_overlap {skip}): n = {n}, worst relative error "
          f"{float(worst):.3e}, bound {n * 2.0 ** -52:.3e}")
    assert all(t > 0 for t in truth.flat(want)[8 * 8 + 16:])    # (the case is not empty: every scalar counts something)


def test_same_call_twice_gives_the_same_bits(gpu_device):
    case, _ = _non_dyadic(0.0, False)
    _, first = _raw(case, gpu_device)
    _, second = _raw(case, gpu_device)
    assert torch.equal(first, second)
    assert torch.equal(first.view(torch.int64), second.view(torch.int64))


def test_refusals_launch_nothing(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    good = truth.random_dyadic_case(1, 5, 5, 2, Kr=3, Kh=3)
    sentinel = torch.full((65 * 65 + 130 + 7,), -7.0, dtype=torch.float64, device=gpu_device)
    for bad, message in ((dict(good, Kr=65), "labels"), (dict(good, Kh=65), "labels"), (dict(good, Kr=-1), "labels"),
                         (dict(good, collar=-0.5), "collar"), (dict(good, collar=float("nan")), "collar")):
        rc, out = _raw(bad, gpu_device, out=sentinel)
        assert rc == 3 and message in lib.pa_last_error().decode()
        assert bool((out == -7.0).all())
    rc, out = _raw(good, gpu_device, ws_bytes=64, out=sentinel)
    assert rc == 3 and "workspace" in lib.pa_last_error().decode() and bool((out == -7.0).all())
    # negative counts (no array is touched)
    none = ctypes.c_void_p(None)
    ws = torch.empty(4096, dtype=torch.uint8, device=gpu_device)
    for Nr, Nh, Nu in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        assert lib.pa_annot_counts_workspace_bytes(Nr, Nh, Nu) == 0
        rc = lib.pa_annot_counts(none, none, Nr, 1, none, none, Nh, 1, none, Nu, 0.0, 0, ffi.ptr(sentinel),
                                 ffi.ptr(ws), 4096, ffi.stream())
        assert rc == 3 and "negative" in lib.pa_last_error().decode()
    torch.cuda.synchronize()
    assert bool((sentinel == -7.0).all())
    assert lib.pa_annot_counts_workspace_bytes(1 << 21, 0, 0) == 0          # more cuts than the sort accepts


def _annotation(rows, names):
    import pyannote_audio_amd as pa
    from pyannote_audio_amd.core import Segment
    a = pa.Annotation()
    for n, (start, end, label) in enumerate(rows):
        a[Segment(start, end), n] = names[label]
    return a


@pytest.mark.parametrize("collar,skip", [(0.0, False), (0.5, True)])
def test_annotation_counts_on_the_device(gpu_device, collar, skip):
    from pyannote_audio_amd import annotation_metrics as am
    from pyannote_audio_amd.core import Segment
    case = truth.random_dyadic_case(21, Nr=90, Nh=80, Nu=4, Kr=6, Kh=7, collar=collar, skip_overlap=skip, span=40.0,
                                    shortest_ticks=1)
    ref = _annotation(case["ref"], [f"r{l}" for l in range(6)])
    hyp = _annotation(case["hyp"], [f"h{l}" for l in range(7)])
    uem = [Segment(a, b) for a, b in case["uem"]]
    kw = dict(uem=uem, collar=collar, skip_overlap=skip)
    dev, host = am.annotation_counts(ref, hyp, device=gpu_device, **kw), am.annotation_counts(ref, hyp, **kw)
    want = truth.case_truth(case)
    for counts in (dev, host):
        got = list(counts["cooc"].ravel()) + list(counts["ref_dur"]) + list(counts["hyp_dur"]) + \
            [counts[name] for name in truth.SCALARS]
        assert [Fraction(float(v)) for v in got] == truth.flat(want)
    # a class built on it, on the device, equals the same class on the host, bit for bit
    a = am.GreedyDiarizationErrorRate(collar=collar, skip_overlap=skip, device=gpu_device)(ref, hyp, uem=uem,
                                                                                           detailed=True)
    b = am.GreedyDiarizationErrorRate(collar=collar, skip_overlap=skip)(ref, hyp, uem=uem, detailed=True)
    assert a == b and a["total"] > 0
    with pytest.raises(ValueError, match="NaN"):
        am.annotation_counts(ref, hyp, uem=[Segment(0.0, float("nan"))], device=gpu_device)


def _greedy(together):
    """the issue's rule, restated here: first maximum in row-major order, its row and column out, while > 0"""
    rows, cols = set(range(len(together))), set(range(len(together[0]) if together else 0))
    pairs = {}
    while rows and cols:
        best, at = max(((together[j][i], (-j, -i)) for j in sorted(rows) for i in sorted(cols)))
        if best <= 0:
            break
        j, i = -at[0], -at[1]
        pairs[j] = i
        rows.discard(j)
        cols.discard(i)
    return pairs


def test_speaker_diarization_end_to_end(pipeline_dir, gpu_device):
    """a `SpeakerDiarization` run on a small synthetic conversation whose file carries its reference: the labels the
    pipeline hands out (counted on the device) are the host path's mapping, and the pipeline's own metric on its
    output equals the truth"""
    import pyannote_audio_amd as pa
    from oracle.synthetic import synth_conversation
    from pyannote_audio_amd import annotation_metrics as am
    from pyannote_audio_amd import diarization
    from pyannote_audio_amd.core import Segment
    seconds = 33.0
    wav, activity = synth_conversation(seconds, seed=5)
    reference = pa.Annotation(uri="synth")
    for s, row in enumerate(np.asarray(activity)):
        edges = np.flatnonzero(np.diff(np.concatenate([[0], row.astype(np.int8), [0]])))
        for n, (a, b) in enumerate(zip(edges[0::2], edges[1::2])):
            reference[Segment(a / 16000.0, b / 16000.0), f"{s}-{n}"] = f"spk{s}"
    assert len(reference.labels()) >= 2
    pipeline = pa.Pipeline.from_pretrained(pipeline_dir).to(gpu_device)
    seen = {}
    label_names = pipeline._label_names

    def spy(file, diarization_, labels):
        names = label_names(file, diarization_, labels)
        seen.update(diarization=diarization_, labels=labels, names=names)
        return names

    pipeline._label_names = spy
    uem = [Segment(0.0, seconds)]
    out = pipeline({"waveform": wav, "sample_rate": 16000, "uri": "synth", "annotation": reference})
    hypothesis = out.speaker_diarization
    _, host_mapping = diarization.optimal_mapping(reference, seen["diarization"], return_mapping=True)
    assert host_mapping and set(host_mapping.values()) <= set(reference.labels())
    assert seen["names"] == {label: host_mapping.get(label, label) for label in seen["labels"]}
    assert set(host_mapping.values()) <= set(hypothesis.labels())

    metric = pipeline.get_metric()
    assert type(metric) is am.GreedyDiarizationErrorRate and metric.device == gpu_device
    detail = metric(reference, hypothesis, uem=uem, detailed=True)
    ref_labels, ref_rows = truth.rows_of(reference)
    hyp_labels, hyp_rows = truth.rows_of(hypothesis)
    want = truth.truth_counts(ref_rows, hyp_rows, [(0.0, seconds)], len(ref_labels), len(hyp_labels))
    pairs = _greedy([[want["cooc"][i][j] for i in range(len(ref_labels))] for j in range(len(hyp_labels))])
    correct = sum(want["cooc"][i][j] for j, i in pairs.items())
    assert metric.greedy_mapping(reference, hypothesis, uem=uem) == \
        {hyp_labels[j]: ref_labels[i] for j, i in pairs.items()}
    expected = {"total": want["total"], "correct": correct, "false alarm": want["false_alarm"],
                "missed detection": want["missed"], "confusion": want["both"] - correct}
    eps = want["intervals"] * Fraction(1, 2 ** 52)            # the bound of the non-dyadic test, per count
    for name, t in expected.items():
        slack = eps * (t if name != "confusion" else want["both"] + correct)
        assert abs(Fraction(detail[name]) - t) <= slack, (name, detail[name], float(t))
    errors = expected["false alarm"] + expected["missed detection"] + expected["confusion"]
    assert want["total"] > 0
    assert detail["diarization error rate"] == pytest.approx(float(errors / want["total"]), rel=1e-12, abs=1e-12)
