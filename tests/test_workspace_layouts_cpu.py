"""The `pa_*_workspace_bytes` functions of the float64 kernels return what they returned before their layouts moved
onto pa::Carver (csrc/workspace.h): tests/golden/workspace_bytes_v1.json holds `table()` below as the library at the
commit before that change computed it (tests/golden/make_workspace_bytes_golden.py).  The cases are the shapes where a
layout can go wrong -- counts on both sides of an alignment block, of a 64-tile and of a row block, empty arrays, the
arguments every function answers with 0, the environment switches of the linkage functions -- plus one hour-sized
shape per function.  The size functions are host code: no GPU is needed."""
import ctypes as C
import itertools
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes_v1.json")

SMALL = (2, 3, 63, 64, 65, 129)
HOUR = 7176                        # embeddings of one audio-hour
HOUR_FRAMES = 213_333              # 16.875 ms frames of one audio-hour
# environments of the linkage functions: default, fast path off, a cap that refuses the square matrix of HOUR points
# (8 * 7176 * 7176 B = 0.41 GB) and one that still holds it
LINKAGE_ENVS = ({}, {"PA_LINKAGE_FAST": "0"}, {"PA_LINKAGE_FAST_MAX_GB": "0.4"}, {"PA_LINKAGE_FAST_MAX_GB": "0.5"},
                {"PA_LINKAGE_FAST": "1", "PA_LINKAGE_FAST_MAX_GB": "0.001"})
ENV_NAMES = ("PA_LINKAGE_FAST", "PA_LINKAGE_FAST_MAX_GB")

# files of a corpus as (reference, hypothesis, uem rows, reference labels, hypothesis labels)
CORPORA = {
    "no_files": [],
    "one_empty_file": [(0, 0, 0, 0, 0)],
    "no_uem": [(5, 7, 0, 2, 3)],
    "three_files": [(5, 7, 2, 2, 3), (0, 0, 0, 0, 0), (63, 65, 1, 4, 4)],
    "hour_files": [(900, 1100, 3, 6, 7)] * 4,
    "too_many_labels": [(5, 7, 2, 65, 3)],
    "too_many_cuts": [(1 << 20, 5, 0, 2, 2)],
}


def cases():
    """[(function, arguments, environment)]; a corpus argument appears as its name in CORPORA"""
    out = []

    def add(function, args, env=None):
        out.append((function, list(args), dict(env or {})))

    # kmeans: N on both sides of a multiple of the 64-row blocks, K at every step of the trial count
    for N, K in itertools.product((64, 65, 127, 128, 129, HOUR), (2, 3, 8, 21, 55, 64)):
        add("pa_kmeans_workspace_bytes", (N, 256, K, 3))
    for N in SMALL:
        add("pa_kmeans_workspace_bytes", (N, 256, 2, 1))
        add("pa_kmeans_workspace_bytes", (N, 1, 2, 3))
    add("pa_kmeans_workspace_bytes", (HOUR, 512, 4, 10))
    add("pa_kmeans_workspace_bytes", (HOUR, 256, 4, 3))
    for bad in ((1, 256, 2, 3), (7, 256, 8, 3), (100, 256, 1, 3), (100, 256, 65, 3), (100, 0, 4, 3), (100, 513, 4, 3),
                (100, 256, 4, 0), (100, 256, 4, 65536), (1 << 24, 256, 4, 3)):
        add("pa_kmeans_workspace_bytes", bad)
    # vbx: one cluster, cluster counts that are no multiple of 32, one job and seven
    for n, s in itertools.product(SMALL + (HOUR,), (1, 7, 33, 45)):
        add("pa_vbx_workspace_bytes", (n, s, 128))
        for jobs in (1, 7):
            add("pa_vbx_batch_workspace_bytes", (jobs, n, s, 128))
    add("pa_vbx_workspace_bytes", (0, 0, 128))
    add("pa_vbx_workspace_bytes", (0, 7, 128))
    for bad in ((0, 5, 7, 128), (1, 0, 7, 128), (1, 5, 0, 128), (1, 5, 7, 0), (-1, 5, 7, 128)):
        add("pa_vbx_batch_workspace_bytes", bad)
    # the linkage family, under every environment
    for env in LINKAGE_ENVS:
        for n in (0, 1) + SMALL + (1024, 1025, HOUR, 11054, 11055, 150000, 150001):
            add("pa_linkage_workspace_bytes", (n,), env)
            add("pa_linkage_chain_workspace_bytes", (n,), env)
    # annotation counts: every count zero, no uem rows, sizes around a block, the refusals
    for Nr, Nh, Nu in ((0, 0, 0), (5, 7, 0), (5, 7, 2), (0, 3, 1), (3, 0, 1), (2, 2, 2), (63, 64, 65), (129, 3, 2),
                       (900, 1100, 3), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (1 << 20, 5, 0)):
        add("pa_annot_counts_workspace_bytes", (Nr, Nh, Nu))
    for name in CORPORA:
        add("pa_annot_corpus_workspace_bytes", (name,))
    # regions and the sweep over them
    for T, K, capacity in itertools.product(SMALL + (HOUR_FRAMES,), (1, 3, 16), (0, 1, 100)):
        add("pa_binarize_regions_workspace_bytes", (T, K, capacity))
    for bad in ((1, 3, 10), (100, 0, 10), (100, 17, 10), (100, 3, -1)):
        add("pa_binarize_regions_workspace_bytes", bad)
    for T in SMALL + (4096, 4097, HOUR_FRAMES):
        for groups, per, L, M, raw_rows, job_rows in ((1, 1, 1, 1, 1, 1), (3, 0, 40, 200, 1000, 5000),
                                                     (3, 2, 40, 0, 1000, 0), (3, 3, 40, 200, 0, 0),
                                                     (0, 0, 0, 0, 0, 0), (7, 7, 100, 1000, 12345, 123456)):
            add("pa_regions_sweep_workspace_bytes", (T, groups, per, L, M, raw_rows, job_rows))
    for bad in ((1, 1, 1, 1, 1, 1, 1), (100, -1, 1, 1, 1, 1, 1), (100, 1, -1, 1, 1, 1, 1), (100, 1, 1, -1, 1, 1, 1),
                (100, 1, 1, 1, -1, 1, 1), (100, 1, 1, 1, 1, -1, 1), (100, 1, 1, 1, 1, 1, -1)):
        add("pa_regions_sweep_workspace_bytes", bad)
    # DET curve: around a block of 1024 positions and a chunk of 1024 blocks
    for T in (1,) + SMALL + (1023, 1024, 1025, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 0x7fffffff, 0, -1, 1 << 31):
        add("pa_det_workspace_bytes", (T,))
    return out


def _corpus(ffi, files):
    """a pa_annot_corpus with the host tables the size function reads, and what keeps them alive"""
    def offsets(column):
        return (C.c_int32 * (len(files) + 1))(*itertools.accumulate([0] + [f[column] for f in files]))
    tables = [offsets(0), offsets(1), offsets(2), (C.c_int32 * max(1, len(files)))(*[f[3] for f in files]),
              (C.c_int32 * max(1, len(files)))(*[f[4] for f in files])]
    c = ffi.AnnotCorpus()
    c.F, c.R = len(files), sum(f[4] for f in files)
    for name, t in zip(("h_ref_off", "h_hyp_off", "h_uem_off", "h_Kr", "h_Kh"), tables):
        setattr(c, name, C.cast(t, C.c_void_p))
    return c, tables


def evaluate(lib, ffi, function, args):
    """the value of one case under the environment of the moment"""
    if function == "pa_annot_corpus_workspace_bytes":
        corpus, keep = _corpus(ffi, CORPORA[args[0]])
        return int(lib.pa_annot_corpus_workspace_bytes(C.byref(corpus)))
    return int(getattr(lib, function)(*args))


def table(lib, ffi):
    """[[function, arguments, environment, bytes], ...] in the order of cases()"""
    saved = {name: os.environ.get(name) for name in ENV_NAMES}
    rows = []
    try:
        for function, args, env in cases():
            for name in ENV_NAMES:
                os.environ.pop(name, None)
            os.environ.update(env)
            rows.append([function, args, env, evaluate(lib, ffi, function, args)])
        return rows
    finally:
        for name, value in saved.items():
            os.environ.pop(name, None)
            if value is not None:
                os.environ[name] = value


@pytest.fixture(scope="module")
def library():
    import __graft_entry__
    __graft_entry__.build()
    import pyannote_audio_amd.ffi as ffi
    return ffi.load(), ffi


with open(GOLDEN) as _fp:
    _GOLDEN = json.load(_fp)
_FUNCTIONS = sorted({row[0] for row in _GOLDEN})


def test_the_golden_file_holds_the_cases_of_this_module():
    assert [row[:3] for row in _GOLDEN] == [list(c) for c in json.loads(json.dumps(cases()))]
    assert len(_FUNCTIONS) == 10


@pytest.mark.parametrize("function", _FUNCTIONS)
def test_size_function_returns_the_recorded_bytes(library, monkeypatch, function):
    lib, ffi = library
    rows = [row for row in _GOLDEN if row[0] == function]
    # (pa_vbx_workspace_bytes has no refusal: it is a plain sum)
    assert any(row[3] > 0 for row in rows)
    assert function == "pa_vbx_workspace_bytes" or any(row[3] == 0 for row in rows)
    wrong = []
    for _, args, env, want in rows:
        for name in ENV_NAMES:
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        got = evaluate(lib, ffi, function, args)
        if got != want:
            wrong.append((args, env, got, want))
    assert not wrong, f"{len(wrong)} of {len(rows)} differ; first (arguments, environment, got, recorded): {wrong[:3]}"


def test_recorded_values_the_documents_quote(library, monkeypatch):
    for name in ENV_NAMES:
        monkeypatch.delenv(name, raising=False)
    lib, _ = library
    assert lib.pa_kmeans_workspace_bytes(7176, 256, 4, 3) == 18234112
    assert lib.pa_linkage_workspace_bytes(7176) == 412310912
    assert lib.pa_annot_counts_workspace_bytes(5, 7, 2) == 2368


def test_the_linkage_counters_are_the_last_128_bytes(library, monkeypatch):
    """distance.linkage_centroid reads ws[-128:]: with the fast path switched off the workspace is the heap kernel's
    five int blocks and one double block, each rounded up to 256 bytes, and the counters"""
    lib, _ = library
    monkeypatch.setenv("PA_LINKAGE_FAST", "0")
    up = lambda b: (b + 255) // 256 * 256
    for n in SMALL + (HOUR,):
        assert lib.pa_linkage_workspace_bytes(n) == 5 * up(4 * n) + up(8 * n) + 128
