"""The frame-domain kernels (csrc/frames.hip) through their own entry points, against tests/frames_model.py on the
cases listed there: pa_seg_chunk_stats, pa_embedding_masks, pa_speaker_count, pa_cluster_activations, pa_topk_binarize,
pa_topk_binarize_f32, pa_binarize_hysteresis, pa_cluster_max and pa_aggregate.

These kernels are exact by construction, so every comparison is np.array_equal -- float outputs bit for bit, NaN
compared as positions -- and no tolerance appears anywhere.  Every output, the 2T scratch of pa_speaker_count included,
lies between guard blocks that must be untouched afterwards.  Where a correct output may hold the guards' usual filling
(an int32 count of 0xA5, the NaN of a cluster without speaker or of a frame nobody voted on) the buffer is filled with a
value no correct result takes: a negative number for counts and activations, -7777.25 for the float outputs.  The uint8
segmentations lie between blocks of 0xFF bytes -- an over-read shows up in a sum -- and the float inputs between blocks
of +-1e30 (kernel_parity.GuardedInput).

What the model itself is held to: tests/test_frames_model_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import frames_model as fm
from kernel_parity import GUARD, Guarded, GuardedInput, dptr
from refusals import check_refusal

pytestmark = pytest.mark.gpu

INT_FILL = -7           # no count and no activation is negative
FLOAT_FILL = -7777.25   # exact in float32; scores lie in [0, 1], so no maximum, sum or average comes near it


class GuardedBytes:
    """a uint8 kernel input between two blocks of 0xFF bytes"""

    def __init__(self, data, device):
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        host = np.full(data.size + 2 * GUARD, 0xFF, dtype=np.uint8)
        host[GUARD:GUARD + data.size] = data
        self.buf = torch.from_numpy(host).to(device)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD)


def _device(array, device):
    return torch.from_numpy(np.ascontiguousarray(array)).to(device)


def _lib():
    import pyannote_audio_amd.ffi as ffi
    return ffi.load(), ffi.stream()


def _report(failed, total):
    assert not failed, f"{len(failed)} of {total} cases differ from the model, the first: {failed[:5]}"


def test_chunk_stats(gpu_device):
    lib, stream = _lib()
    failed, cases = [], fm.chunk_stats_cases()
    for case in cases:
        Cn, F, S = case["seg"].shape
        seg = GuardedBytes(case["seg"], gpu_device)
        active = Guarded(Cn * S, gpu_device, torch.int32, fill=INT_FILL)
        clean = Guarded(Cn * S, gpu_device, torch.int32, fill=INT_FILL)
        assert lib.pa_seg_chunk_stats(seg.ptr, Cn, F, S, active.ptr, clean.ptr, stream) == 0, case["id"]
        want_active, want_clean = fm.chunk_stats(case["seg"])
        got_active = active.check(what=case["id"] + " active").numpy().reshape(Cn, S)
        got_clean = clean.check(what=case["id"] + " clean").numpy().reshape(Cn, S)
        if not (np.array_equal(got_active, want_active) and np.array_equal(got_clean, want_clean)):
            failed.append(case["id"])
    _report(failed, len(cases))


@pytest.mark.parametrize("S", [0, 9])
def test_chunk_stats_refuses_other_speaker_counts(gpu_device, S):
    """the kernel unrolls to 8 local speakers; pa_embedding_masks has no such bound and refuses nothing"""
    lib, stream = _lib()
    Cn, F = 3, 63
    seg = GuardedBytes(np.ones((Cn, F, S), dtype=np.uint8), gpu_device)
    check_refusal(lambda active, clean: lib.pa_seg_chunk_stats(seg.ptr, Cn, F, S, active, clean, stream),
                  [((Cn, S), torch.int32), ((Cn, S), torch.int32)],
                  f"pa_seg_chunk_stats: 1 <= S <= 8 required (got {S})", gpu_device)


def test_embedding_masks(gpu_device):
    lib, stream = _lib()
    failed, cases = [], fm.embedding_masks_cases()
    for case in cases:
        Cn, F, S = case["seg"].shape
        seg = GuardedBytes(case["seg"], gpu_device)
        clean = _device(case["clean"], gpu_device)
        masks = Guarded(Cn * S * F, gpu_device, fill=FLOAT_FILL)
        assert lib.pa_embedding_masks(seg.ptr, Cn, F, S, dptr(clean), case["exclude_overlap"], case["min_num_frames"],
                                      masks.ptr, stream) == 0, case["id"]
        want = fm.embedding_masks(case["seg"], case["clean"], case["exclude_overlap"], case["min_num_frames"])
        got = masks.check(what=case["id"]).numpy().reshape(Cn, S, F)
        if not fm.same_bits(got, want):
            failed.append(case["id"])
    _report(failed, len(cases))


def test_speaker_count(gpu_device):
    lib, stream = _lib()
    failed, cases = [], fm.speaker_count_cases()
    for case in cases:
        Cn, F, S = case["seg"].shape
        T = case["T"]
        seg = GuardedBytes(case["seg"], gpu_device)
        start = _device(case["start"], gpu_device)
        count = Guarded(T, gpu_device, torch.uint8)
        scratch = Guarded(2 * T, gpu_device, torch.int32, fill=INT_FILL)
        assert lib.pa_speaker_count(seg.ptr, Cn, F, S, dptr(start) if Cn else None, T, count.ptr, scratch.ptr,
                                    stream) == 0, case["id"]
        scratch.check(what=case["id"] + " scratch")
        got = count.check(what=case["id"]).numpy()
        if not np.array_equal(got, fm.speaker_count(case["seg"], case["start"], T)):
            failed.append(case["id"])
        if Cn == 0:
            assert not got.any(), "no chunk: every count is 0"
    _report(failed, len(cases))


def test_cluster_activations(gpu_device):
    lib, stream = _lib()
    failed, cases = [], fm.cluster_activations_cases()
    for case in cases:
        Cn, F, S = case["seg"].shape
        T, K = case["T"], case["K"]
        seg = GuardedBytes(case["seg"], gpu_device)
        start, hard = _device(case["start"], gpu_device), _device(case["hard"], gpu_device)
        act = Guarded(T * K, gpu_device, torch.int32, fill=INT_FILL)
        assert lib.pa_cluster_activations(seg.ptr, Cn, F, S, dptr(start), dptr(hard), K, T, act.ptr, stream) == 0
        got = act.check(what=case["id"]).numpy().reshape(T, K)
        if not np.array_equal(got, fm.cluster_activations(case["seg"], case["start"], case["hard"], K, T)):
            failed.append(case["id"])
    _report(failed, len(cases))


@pytest.mark.parametrize("form", ["i32", "f32"])
def test_topk_binarize(gpu_device, form):
    """`out` and `tie` themselves: Reconstructor.discretize re-decides flagged frames on the host, so a missing flag
    shows there only where the host's np.argsort departs from lowest-index order"""
    lib, stream = _lib()
    entry = lib.pa_topk_binarize if form == "i32" else lib.pa_topk_binarize_f32
    failed, cases = [], fm.topk_i32_cases() if form == "i32" else fm.topk_f32_cases()
    for case in cases:
        T, K = case["act"].shape
        act = _device(case["act"], gpu_device) if form == "i32" else GuardedInput(torch.from_numpy(case["act"]),
                                                                                  gpu_device)
        count = _device(case["count"], gpu_device)
        out = Guarded(T * K, gpu_device, torch.uint8)
        tie = Guarded(T, gpu_device, torch.uint8)
        assert entry(dptr(act) if form == "i32" else act.ptr, dptr(count), T, K, case["cap"], out.ptr, tie.ptr,
                     stream) == 0, case["id"]
        want_out, want_tie = fm.topk(case["act"], case["count"], case["cap"])
        got_out = out.check(what=case["id"] + " out").numpy().reshape(T, K)
        got_tie = tie.check(what=case["id"] + " tie").numpy()
        if not (np.array_equal(got_out, want_out) and np.array_equal(got_tie, want_tie)):
            failed.append(case["id"])
        if case["distinct"]:
            assert not got_tie.any(), case["id"]
    _report(failed, len(cases))


def test_binarize_hysteresis(gpu_device):
    """the knife-edge cases -- a first score on the reference's float32 midpoint or next to it, then scores between
    the thresholds -- fail on a kernel that forms the midpoint from the float32 thresholds"""
    lib, stream = _lib()
    failed, cases = [], fm.hysteresis_cases()
    for case in cases:
        Cn, F, K = case["scores"].shape
        scores = GuardedInput(torch.from_numpy(case["scores"]), gpu_device)
        out = Guarded(Cn * F * K, gpu_device, torch.uint8)
        midpoint = float(fm.hysteresis_midpoint(case["onset"], case["offset"]))
        assert lib.pa_binarize_hysteresis(scores.ptr, Cn, F, K, case["onset"], case["offset"], midpoint,
                                          case["initial_state"], out.ptr, stream) == 0, case["id"]
        want = fm.hysteresis(case["scores"], case["onset"], case["offset"], case["initial_state"])
        if not np.array_equal(out.check(what=case["id"]).numpy().reshape(Cn, F, K), want):
            failed.append(case["id"])
    _report(failed, len(cases))


def test_binarize_wrapper_hands_over_the_reference_midpoint(gpu_device):
    """frames.binarize, the entry point's one caller, on the knife-edge cases"""
    from pyannote_audio_amd import frames as frame_ops
    cases = [c for c in fm.hysteresis_cases()
             if (c["onset"], c["offset"]) in fm.KNIFE_EDGE_PAIRS and c["scores"].shape[0] in (85, 86)]
    assert len(cases) == 18
    for case in cases:
        got = frame_ops.binarize(torch.from_numpy(case["scores"]).to(gpu_device), onset=case["onset"],
                                 offset=case["offset"], initial_state=None).cpu().numpy()
        want = fm.hysteresis(case["scores"], case["onset"], case["offset"], -1)
        assert np.array_equal(got, want), case["id"]


def test_cluster_max(gpu_device):
    lib, stream = _lib()
    failed, cases = [], fm.cluster_max_cases()
    for case in cases:
        Cn, F, S = case["scores"].shape
        K = case["K"]
        scores = GuardedInput(torch.from_numpy(case["scores"]), gpu_device)
        hard = _device(case["hard"], gpu_device)
        out = Guarded(Cn * F * K, gpu_device, fill=FLOAT_FILL)
        assert lib.pa_cluster_max(scores.ptr, Cn, F, S, dptr(hard), K, out.ptr, stream) == 0, case["id"]
        want = fm.cluster_max(case["scores"], case["hard"], K)
        assert np.isnan(want).any() and not np.isnan(want).all()
        if not fm.same_bits(out.check(what=case["id"]).numpy().reshape(Cn, F, K), want):
            failed.append(case["id"])
    _report(failed, len(cases))


def test_aggregate(gpu_device):
    lib, stream = _lib()
    failed, cases = [], fm.aggregate_cases()
    for case in cases:
        Cn, F, K = case["scores"].shape
        T = case["T"]
        scores = GuardedInput(torch.from_numpy(case["scores"]), gpu_device)
        start = _device(case["start"], gpu_device)
        window, warm = _device(case["window"], gpu_device), _device(case["warm"], gpu_device)
        assert window.dtype == warm.dtype == torch.float64
        out = Guarded(T * K, gpu_device, fill=FLOAT_FILL)
        assert lib.pa_aggregate(scores.ptr, Cn, F, K, dptr(start), T, dptr(window), dptr(warm), case["epsilon"],
                                case["missing"], case["skip_average"], out.ptr, stream) == 0, case["id"]
        want = fm.aggregate(case["scores"], case["start"], T, case["window"], case["warm"], case["epsilon"],
                            case["missing"], case["skip_average"])
        if not fm.same_bits(out.check(what=case["id"]).numpy().reshape(T, K), want):
            failed.append(case["id"])
    _report(failed, len(cases))
