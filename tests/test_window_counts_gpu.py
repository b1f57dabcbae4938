"""GPU: `pa_annot_window_counts` (csrc/annot_metrics.hip) against the exact truth of tests/annotation_metrics_truth.py:
the truth of window w is `truth_counts(ref, hyp, uem clipped to the window, Kr, Kh, collar, skip_overlap)`
(tests/window_counts_cases.py).

Dyadic cases (every boundary, collar boundary and window boundary a multiple of 2^-10 s below 4096 s; asserted) make
every partial sum exactly representable: all fields of all windows are compared with `==` as Fractions.  The
non-dyadic case carries the bound derived from the number of elementary intervals."""
from fractions import Fraction

import pytest
import torch

import annotation_metrics_truth as truth
import window_counts_cases as cases
from refusals import check_refusal

pytestmark = pytest.mark.gpu


def _nout(case):
    Kr, Kh = max(case["Kr"], 0), max(case["Kh"], 0)
    return Kr * Kh + Kr + Kh + 7


def _arrays(case, device):
    def f64(rows):
        return torch.tensor([[r[0], r[1]] for r in rows], dtype=torch.float64).reshape(-1, 2).to(device)

    def i32(rows):
        return torch.tensor([r[2] for r in rows], dtype=torch.int32).to(device)

    return f64(case["ref"]), i32(case["ref"]), f64(case["hyp"]), i32(case["hyp"]), f64(case["uem"])


def _ptr(t):
    import pyannote_audio_amd.ffi as ffi
    return ffi.ptr(t) if t.numel() else None


def _raw(case, device, ws_bytes=None, out=None):
    """the raw entry point on a case -> (rc, (W, nout) float64 device tensor)"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    ref_seg, ref_lab, hyp_seg, hyp_lab, uem_seg = _arrays(case, device)
    win = torch.tensor(case["windows"], dtype=torch.float64).reshape(-1, 2).to(device)
    W = len(case["windows"])
    need = int(lib.pa_annot_window_counts_workspace_bytes(len(case["ref"]), len(case["hyp"]), len(case["uem"]), W))
    ws = torch.empty(max(need if ws_bytes is None else ws_bytes, 1), dtype=torch.uint8, device=device)
    if out is None:
        out = torch.full((W, _nout(case)), float("nan"), dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        rc = lib.pa_annot_window_counts(_ptr(ref_seg), _ptr(ref_lab), len(case["ref"]), case["Kr"], _ptr(hyp_seg),
                                        _ptr(hyp_lab), len(case["hyp"]), case["Kh"], _ptr(uem_seg), len(case["uem"]),
                                        _ptr(win), W, float(case["collar"]), int(case["skip_overlap"]),
                                        ffi.ptr(out) if out.numel() else None, ffi.ptr(ws),
                                        ws.numel() if ws_bytes is None else ws_bytes, ffi.stream())
        torch.cuda.synchronize()
    return rc, out


def _whole_file(case, device):
    """`pa_annot_counts` of the same file -> float64 device tensor"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    ref_seg, ref_lab, hyp_seg, hyp_lab, uem_seg = _arrays(case, device)
    ws = torch.empty(int(lib.pa_annot_counts_workspace_bytes(len(case["ref"]), len(case["hyp"]), len(case["uem"]))),
                     dtype=torch.uint8, device=device)
    out = torch.full((_nout(case),), float("nan"), dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        rc = lib.pa_annot_counts(_ptr(ref_seg), _ptr(ref_lab), len(case["ref"]), case["Kr"], _ptr(hyp_seg),
                                 _ptr(hyp_lab), len(case["hyp"]), case["Kh"], _ptr(uem_seg), len(case["uem"]),
                                 float(case["collar"]), int(case["skip_overlap"]), ffi.ptr(out), ffi.ptr(ws),
                                 ws.numel(), ffi.stream())
        torch.cuda.synchronize()
    assert rc == 0
    return out


def _exact(case, device):
    cases.assert_dyadic(case)
    rc, out = _raw(case, device)
    assert rc == 0
    got = out.cpu().tolist()
    assert len(got) == len(case["windows"])
    for w, (row, want) in enumerate(zip(got, cases.window_truths(case))):
        assert [Fraction(v) for v in row] == truth.flat(want), (w, case["windows"][w])
    return out


@pytest.mark.parametrize("collar", [0.0, 0.25, 0.5, 1.0])
@pytest.mark.parametrize("skip", [False, True])
def test_hand_built_edges(gpu_device, collar, skip):
    """window edges on segment, uem and collar boundaries; the end of window w on the start of w + 2; a window outside
    the uem; windows across two and across all uem regions; zero-length windows; the whole file"""
    case = cases.hand_case(collar, skip)
    out = _exact(case, gpu_device)
    for w in cases.HAND_ZERO_ROWS:
        assert not out[w].any()
    if collar <= 0.25:                                         # (wider collars leave little to evaluate)
        assert out[:, -7].count_nonzero().item() >= 8          # `total`: most windows count something
    # the window that covers the whole file is pa_annot_counts of the file
    assert case["windows"][-1] == (0.0, 64.0)
    assert torch.equal(out[-1], _whole_file(case, gpu_device))
    # the same windows in descending order: the same rows
    down = sorted(case["windows"], reverse=True)
    assert down != case["windows"] and all(a >= b for a, b in zip(down, down[1:]))
    flipped = _exact(cases.hand_case(collar, skip, down), gpu_device)
    for w, window in enumerate(down):
        assert torch.equal(flipped[w], out[case["windows"].index(window)])


@pytest.mark.parametrize("windows", [[(3.0, 7.5)], [(5.0, 5.0)], [(50.0, 60.0)]])
def test_one_window(gpu_device, windows):
    _exact(cases.hand_case(0.25, False, windows), gpu_device)


def test_no_window_launches_nothing(gpu_device):
    case = cases.hand_case(0.25, False, [])
    sentinel = torch.full((64,), -7.0, dtype=torch.float64, device=gpu_device)
    rc, out = _raw(case, gpu_device, out=sentinel)
    assert rc == 0 and bool((out == -7.0).all())


def test_empty_sides(gpu_device):
    """no reference, no hypothesis, no uem, nothing at all but windows: the window cuts alone are sorted and swept"""
    for Nr, Nh, Nu in ((0, 9, 2), (9, 0, 2), (9, 9, 0), (0, 0, 0), (0, 0, 3)):
        case = truth.random_dyadic_case(11, Nr, Nh, Nu, Kr=3 if Nr else 0, Kh=2 if Nh else 0, collar=0.5, span=8.0)
        out = _exact(cases.with_windows(case, cases.random_windows(Nr + Nh, 5, span=8.0, longest=4.0)), gpu_device)
        if Nu == 0 or (Nr == 0 and Nh == 0):
            assert not out.any()


@pytest.mark.parametrize("name,Nr,Nh,Nu,W,collar", cases.SHAPES)
@pytest.mark.parametrize("skip", [False, True])
def test_sizes_where_the_kernels_change_shape(gpu_device, name, Nr, Nh, Nu, W, collar, skip):
    """the sizes of test_annotation_metrics_gpu.test_sizes_where_the_kernels_change_shape, counted WITH the two cuts of
    every window (the items of the sweep do not grow with the windows)"""
    case = cases.shape_case(name, Nr, Nh, Nu, W, collar, skip)
    _exact(case, gpu_device)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_intervals_in_a_window(gpu_device, n):
    """the reduction strides 256 lanes over the window's rank range: ranges of 1, 255, 256 and 257 intervals"""
    case = cases.range_case(n)
    (a, b), = cases.rank_ranges(case)
    assert b - a == n
    assert _exact(case, gpu_device)[0, -7].item() > 0.0


def test_window_without_an_interval_of_length(gpu_device):
    """A window with start <= end always has its own start cut in its range, so "no interval" is a zero-length window:
    its range holds the one interval between its own two cuts, of length 0 (more when other cuts tie with it) -- here
    inside a turn, on a segment boundary, and twice the same window."""
    case = cases.hand_case(0.0, False, [(3.5, 3.5), (4.0, 4.0), (3.5, 3.5)])
    ranges = cases.rank_ranges(case)
    assert ranges[0][1] - ranges[0][0] == 2 and ranges[2][1] - ranges[2][0] == 2 and ranges[1][1] > ranges[1][0]
    assert not _exact(case, gpu_device).any()
    alone = cases.hand_case(0.0, False, [(3.5, 3.5)])
    (a, b), = cases.rank_ranges(alone)
    assert b - a == 1
    assert not _exact(alone, gpu_device).any()


def test_64_labels_with_bit_63_inside_one_window_only(gpu_device):
    case = cases.labels64_case()
    _exact(dict(case, skip_overlap=True), gpu_device)
    out = _exact(case, gpu_device)
    last = 63 * 64 + 63                                                   # cooc[63][63]
    assert out[1, last].item() > 0.0
    assert [out[w, last].item() for w in (0, 2, 3, 4)] == [0.0] * 4
    assert out[4, 64 * 64 + 63].item() > 0.0                              # (ref_dur[63]: on in (2, 2.5), alone)


@pytest.mark.parametrize("collar,skip", [(0.0, False), (2.0 ** -6, True)])
def test_non_dyadic_within_the_derived_bound(gpu_device, collar, skip):
    """300 segments a side, 8 labels, 40 windows of irregular length, uniform float64 boundaries: the bound of
    `window_counts_cases.check_within_bound`"""
    case, truths, n = cases.non_dyadic(collar, skip)
    assert n > 600 and len(case["windows"]) == 40
    rc, out = _raw(case, gpu_device)
    assert rc == 0
    worst = cases.check_within_bound(out.cpu().tolist(), case, truths, n)
    print(f"non-dyadic windows (collar {collar}, skip_overlap {skip}): n = {n}, worst relative error {worst:.3e}, "
          f"bound {n * 2.0 ** -52:.3e}")
    assert sum(1 for t in truths if t["total"] > 0) >= 20                 # (the windows are not empty)


def test_same_call_twice_gives_the_same_bits(gpu_device):
    case, _, _ = cases.non_dyadic(0.0, False)
    _, first = _raw(case, gpu_device)
    _, second = _raw(case, gpu_device)
    assert torch.equal(first.view(torch.int64), second.view(torch.int64))


def test_refusals_launch_nothing(gpu_device):
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    good = cases.with_windows(truth.random_dyadic_case(1, 5, 5, 2, Kr=3, Kh=3), [(1.0, 9.0), (5.0, 30.0), (2.0, 2.0)])
    ref_seg, ref_lab, hyp_seg, hyp_lab, uem_seg = _arrays(good, gpu_device)
    win = torch.tensor(good["windows"], dtype=torch.float64, device=gpu_device)
    need = int(lib.pa_annot_window_counts_workspace_bytes(5, 5, 2, 3))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    # the fp64 output as its float32 words: room for 64 labels a side, whatever the refused call asks for
    outputs = [((3, 2 * (65 * 65 + 130 + 7)), torch.float32)]

    def call(Nr=5, Kr=3, Nh=5, Kh=3, Nu=2, W=3, collar=0.0, ws_bytes=need):
        def launch(out):
            with torch.cuda.device(gpu_device):
                return lib.pa_annot_window_counts(ffi.ptr(ref_seg), ffi.ptr(ref_lab), Nr, Kr, ffi.ptr(hyp_seg),
                                                  ffi.ptr(hyp_lab), Nh, Kh, ffi.ptr(uem_seg), Nu, ffi.ptr(win), W,
                                                  collar, 0, out, ffi.ptr(ws), ws_bytes, ffi.stream())
        return launch

    name = "pa_annot_window_counts: "
    for launch, message in (
            (call(Kr=65), "65 reference and 3 hypothesis labels, 0..64 each supported"),
            (call(Kh=65), "3 reference and 65 hypothesis labels, 0..64 each supported"),
            (call(Kr=-1), "-1 reference and 3 hypothesis labels, 0..64 each supported"),
            (call(Nr=-1), "negative segment or window count (-1, 5, 2, 3)"),
            (call(Nh=-1), "negative segment or window count (5, -1, 2, 3)"),
            (call(Nu=-1), "negative segment or window count (5, 5, -1, 3)"),
            (call(W=-1), "negative segment or window count (5, 5, 2, -1)"),
            (call(collar=-0.5), "collar -0.5 is negative or NaN"),
            (call(collar=float("nan")), "collar nan is negative or NaN"),
            (call(collar=0.25, ws_bytes=64), f"workspace of 64 bytes, {need} needed"),
            (call(collar=0.25, ws_bytes=need - 1), f"workspace of {need - 1} bytes, {need} needed")):
        check_refusal(launch, outputs, name + message, gpu_device)
    # more cuts than the quadratic sort accepts, with the arrays and the workspace such a call would need
    cap = 1 << 22
    Nr = cap // 2
    big_seg = torch.zeros((Nr, 2), dtype=torch.float64, device=gpu_device)
    big_lab = torch.zeros((Nr,), dtype=torch.int32, device=gpu_device)
    big_ws = torch.empty(48 * (cap + 8) + 4096, dtype=torch.uint8, device=gpu_device)

    def over_the_cap(out):
        with torch.cuda.device(gpu_device):
            return lib.pa_annot_window_counts(ffi.ptr(big_seg), ffi.ptr(big_lab), Nr, 3, None, None, 0, 3, None, 0,
                                              ffi.ptr(win), 1, 0.0, 0, out, ffi.ptr(big_ws), big_ws.numel(),
                                              ffi.stream())

    check_refusal(over_the_cap, outputs, name + f"more than {cap} cuts", gpu_device)
    # the size function answers 0 for what the call refuses
    for Nr_, Nh_, Nu_, W_ in ((-1, 0, 0, 1), (0, -1, 0, 1), (0, 0, -1, 1), (0, 0, 0, -1), (1 << 21, 0, 0, 1),
                              (0, 0, 0, (1 << 21) + 1)):
        assert lib.pa_annot_window_counts_workspace_bytes(Nr_, Nh_, Nu_, W_) == 0
    assert lib.pa_annot_window_counts_workspace_bytes(0, 0, 0, 1 << 21) > 0
