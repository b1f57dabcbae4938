"""GPU: the front ends of several short files in shared launch groups (`apply_batch(pack=...)`).

* `pa_seg_forward_files` gives every file the rows `pa_seg_forward` gives it alone, with `torch.equal`: the sinc stage
  runs per file (its span is re-centred by the file's first chunk), everything behind it once over all chunks -- file
  boundaries inside 16-chunk tiles, a tile boundary inside a file, a one-chunk file (the per-chunk sinc path), an
  orphan chunk, silence and a DC offset; with and without the span path, in both file orders; guard rows around both
  outputs; the refusals of the C ABI;
* `pa_gather_chunks` against numpy, exactly: aligned and unaligned starts, rows and bases, chunks that end or start
  past their file's end, an empty file, 1 and 300 chunks, a guard band;
* `pipeline(files, pack=True)` == `[pipeline(f) for f in files]`: turns, centroids, URIs; the groups it formed;
  per-file `pipeline_kwargs`; the fallbacks; an abandoned iterator."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 32000            # samples per chunk of the kernel-level tests (2 s)
GUARD = 2            # guard rows before and behind the outputs


# ----------------------------------------------------------------------------------- pa_seg_forward_files
@pytest.fixture(scope="module")
def seg(gpu_device):
    from oracle import seeded_pyannet
    from pyannote_audio_amd.segmentation import SegmentationEngine
    from pyannote_audio_amd.weights import SegmentationPack
    model = seeded_pyannet(seed=1234, num_layers=4)
    pack = SegmentationPack(model.state_dict(), {"lstm": {"num_layers": 4}}, 7, 3, 2, gpu_device)
    return pack, SegmentationEngine(pack)


@pytest.fixture(scope="module")
def seg_files(gpu_device):
    """the six files of the kernel-level test, on the device"""
    g = torch.Generator().manual_seed(11)

    def speechlike(n):
        t = torch.arange(n)
        envelope = 0.5 + 0.5 * torch.sin(t * (2 * np.pi / 9000.0))
        return (0.1 * torch.randn(n, generator=g) * envelope + 0.05 * torch.sin(t * 0.01)).clamp(-1, 1)

    waves = [speechlike(N + 16 * 3200),            # 17 chunks at stride 3 200: a tile boundary inside the file
             speechlike(5000),                     # one zero-padded chunk (B = 1: the per-chunk sinc layer)
             speechlike(N),                        # exactly one chunk
             speechlike(N + 2 * 3200 + 777),       # three chunks + an orphan
             torch.zeros(N + 3 * 3200),            # silence
             speechlike(N + 5 * 3200) + 0.3]       # a DC offset of 0.3 (the span is re-centred by ITS chunk 0)
    return [w.to(gpu_device) for w in waves]


def _counts(waves, stride):
    from pyannote_audio_amd.inference import Inference
    return [sum(Inference.num_chunks(w.numel(), N, stride)) for w in waves]


def _forward_files_raw(pack, waves, counts, stride, num_samples=N, workspace_delta=0):
    """the C entry point itself, with guard rows around both outputs -> (rc, logp, multilabel) incl. the guards"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    w = pack.struct
    dev = pack.device
    n = len(waves)
    F = max(lib.pa_seg_num_frames(num_samples, 10), 1)
    total = sum(c for c in counts if c > 0)
    logp = torch.full((total + 2 * GUARD, F, w.num_classes), -777.0, dtype=torch.float32, device=dev)
    ml = torch.full((total + 2 * GUARD, F, w.num_speakers), 201, dtype=torch.uint8, device=dev)
    ptrs = (C.c_void_p * n)(*[x.data_ptr() for x in waves])
    lens = (C.c_int64 * n)(*[x.numel() for x in waves])
    cnts = (C.c_int * n)(*counts)
    need = lib.pa_seg_files_workspace_bytes(w, n, cnts, num_samples, stride)
    ws = torch.empty(max(need + workspace_delta, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.pa_seg_forward_files(w, ptrs, lens, cnts, n, stride, num_samples, ffi.ptr(logp[GUARD:]),
                                      ffi.ptr(ml[GUARD:]), ffi.ptr(ws), max(need + workspace_delta, 0), ffi.stream())
        torch.cuda.synchronize()
    return rc, need, logp, ml


def _guards_untouched(logp, ml):
    return bool((logp[:GUARD] == -777.0).all() and (logp[-GUARD:] == -777.0).all()
                and (ml[:GUARD] == 201).all() and (ml[-GUARD:] == 201).all())


@pytest.fixture(scope="module")
def per_file_reference(seg, seg_files):
    """`pa_seg_forward` on every file alone, per stride: computed once, shared"""
    _, engine = seg
    out = {}
    for stride in (3200, N):
        out[stride] = [engine.forward_strided(w, stride, c, N) for w, c in zip(seg_files, _counts(seg_files, stride))]
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("stride", [3200, N])
@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_packed_forward_equals_per_file_forward(seg, seg_files, per_file_reference, stride, order):
    pack, engine = seg
    idx = list(range(len(seg_files)))
    if order == "reversed":
        idx.reverse()
    waves = [seg_files[i] for i in idx]
    counts = _counts(waves, stride)
    if stride == 3200:
        assert sorted(counts) == sorted([17, 1, 1, 4, 4, 6])
    want_logp = torch.cat([per_file_reference[stride][i][0] for i in idx])
    want_ml = torch.cat([per_file_reference[stride][i][1] for i in idx])
    rc, _, logp, ml = _forward_files_raw(pack, waves, counts, stride)
    assert rc == 0
    assert _guards_untouched(logp, ml)
    assert torch.equal(logp[GUARD:-GUARD], want_logp)
    assert torch.equal(ml[GUARD:-GUARD], want_ml)
    assert not torch.isnan(want_logp).any() and want_ml.max() <= 1
    # ... and through the engine (launch groups of at most `max_chunks` chunks: 20 cuts the 17-chunk file off its
    # neighbours, 5 cuts it in four where `forward_strided` cuts it)
    for max_chunks in (4096, 20, 5):
        from pyannote_audio_amd.segmentation import SegmentationEngine
        small = SegmentationEngine(pack, max_chunks=max_chunks)
        got_logp, got_ml = small.forward_files(waves, stride, counts, N)
        if max_chunks == 5:
            ref = [small.forward_strided(w, stride, c, N) for w, c in zip(waves, counts)]
            assert torch.equal(got_logp, torch.cat([r[0] for r in ref]))
            assert torch.equal(got_ml, torch.cat([r[1] for r in ref]))
        else:
            assert torch.equal(got_logp, want_logp) and torch.equal(got_ml, want_ml)


def test_packed_forward_refusals_and_empty_files(seg, seg_files, per_file_reference):
    import pyannote_audio_amd.ffi as ffi
    pack, engine = seg
    lib = ffi.load()
    stride = 3200
    counts = _counts(seg_files, stride)
    # the size function is tight: one byte less is refused, nothing is launched
    rc, need, logp, ml = _forward_files_raw(pack, seg_files, counts, stride, workspace_delta=-1)
    assert need > 0 and rc == 3 and b"workspace too small" in lib.pa_last_error()
    assert (logp == -777.0).all() and (ml == 201).all()
    with pytest.raises(ValueError, match="workspace too small"):
        ffi.check(rc, "packed forward")
    # a negative chunk count
    bad = list(counts)
    bad[2] = -1
    rc, need, logp, ml = _forward_files_raw(pack, seg_files, bad, stride)
    assert need == 0 and rc == 3 and b"negative chunk count" in lib.pa_last_error()
    assert (logp == -777.0).all() and (ml == 201).all()
    with pytest.raises(ValueError):
        ffi.check(rc, "packed forward")
    with pytest.raises(ValueError):
        engine.forward_files(seg_files, stride, bad, N)
    # chunks too short for a frame
    rc, need, logp, ml = _forward_files_raw(pack, seg_files, [1] * len(seg_files), stride, num_samples=900)
    assert need == 0 and rc == 3 and b"too short" in lib.pa_last_error()
    assert (logp == -777.0).all() and (ml == 201).all()
    with pytest.raises(ValueError):
        ffi.check(rc, "packed forward")
    with pytest.raises(ValueError):
        engine.forward_files(seg_files, stride, [1] * len(seg_files), 900)
    # no chunk at all: 0, nothing written
    rc, _, logp, ml = _forward_files_raw(pack, seg_files[:2], [0, 0], stride)
    assert rc == 0 and (logp == -777.0).all() and (ml == 201).all()
    rc, _, logp, ml = _forward_files_raw(pack, [], [], stride)
    assert rc == 0 and (logp == -777.0).all() and (ml == 201).all()
    # a file of 0 chunks contributes nothing
    some = [counts[0], 0, counts[3]]
    rc, _, logp, ml = _forward_files_raw(pack, [seg_files[0], seg_files[1], seg_files[3]], some, stride)
    assert rc == 0 and _guards_untouched(logp, ml)
    ref = per_file_reference[stride]
    assert torch.equal(logp[GUARD:-GUARD], torch.cat([ref[0][0], ref[3][0]]))
    assert torch.equal(ml[GUARD:-GUARD], torch.cat([ref[0][1], ref[3][1]]))


# --------------------------------------------------------------------------------------- pa_gather_chunks
def _gather_case(num_chunks, num_samples, seed):
    """files (one empty, one whose base is not 16-byte aligned), starts of every residue modulo 4, chunks that end
    past and start past their file's end"""
    rng = np.random.default_rng(seed)
    lengths = [5000, 0, 16001, 40000, 401]
    host = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    chunk_file = rng.integers(0, len(lengths), num_chunks).astype(np.int32)
    chunk_start = np.zeros(num_chunks, dtype=np.int64)
    for c, f in enumerate(chunk_file):
        kind = c % 5
        n = lengths[f]
        if kind == 0:                                    # aligned start, inside the file where it is long enough
            chunk_start[c] = 4 * rng.integers(0, max(1, (n - num_samples) // 4 + 1)) if n > num_samples else 0
        elif kind == 1:                                  # any residue
            chunk_start[c] = rng.integers(0, max(1, n))
        elif kind == 2:                                  # ends past the file's end
            chunk_start[c] = max(0, n - rng.integers(1, num_samples + 1))
        elif kind == 3:                                  # starts at or past the file's end
            chunk_start[c] = n + rng.integers(0, 9)
        else:                                            # aligned start, ends past the end by a few samples
            chunk_start[c] = max(0, (n - num_samples + rng.integers(1, 8)) // 4 * 4)
    want = np.zeros((num_chunks, num_samples), dtype=np.float32)
    for c, (f, s) in enumerate(zip(chunk_file, chunk_start)):
        piece = host[f][s:s + num_samples]
        want[c, :len(piece)] = piece
    return host, chunk_file, chunk_start, want


@pytest.mark.parametrize("num_samples", [400, 401, 16000])
@pytest.mark.parametrize("num_chunks", [1, 300])
def test_gather_chunks_equals_numpy(gpu_device, num_chunks, num_samples):
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd import frames as frame_ops
    host, chunk_file, chunk_start, want = _gather_case(num_chunks, num_samples, seed=num_chunks + num_samples)
    if num_chunks == 1:
        chunk_file[0], chunk_start[0] = 2, 16001 - num_samples // 2 - 1          # one chunk: ends past its file
        want[:] = 0
        piece = host[2][chunk_start[0]:]
        want[0, :len(piece)] = piece
    # file 3 sits one sample behind an allocation's start: its base is not 16-byte aligned
    shifted = torch.from_numpy(np.concatenate([[9.0], host[3]]).astype(np.float32)).to(gpu_device)
    waves = [torch.from_numpy(h).to(gpu_device) for h in host]
    waves[3] = shifted[1:]
    assert waves[3].data_ptr() % 16 == 4 and waves[0].data_ptr() % 16 == 0
    assert (chunk_start % 4 != 0).any() or num_chunks == 1
    got = frame_ops.gather_chunks(waves, chunk_file, chunk_start, num_samples)
    torch.cuda.synchronize()
    assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)

    # the entry point itself, writing into the middle of a guarded buffer (rows of 401 samples: the output rows take
    # every alignment)
    band = 3 * num_samples
    buf = torch.full((band + num_chunks * num_samples + band,), -5.0, dtype=torch.float32, device=gpu_device)
    ptrs = torch.tensor([w.data_ptr() for w in waves], dtype=torch.int64, device=gpu_device)
    lens = torch.tensor([w.numel() for w in waves], dtype=torch.int64, device=gpu_device)
    cf = torch.from_numpy(chunk_file).to(gpu_device)
    cs = torch.from_numpy(chunk_start).to(gpu_device)
    with torch.cuda.device(gpu_device):
        ffi.check(ffi.load().pa_gather_chunks(ffi.ptr(ptrs), ffi.ptr(lens), ffi.ptr(cf), ffi.ptr(cs), num_chunks,
                                              num_samples, ffi.ptr(buf[band:]), ffi.stream()), "pa_gather_chunks")
        torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:band] == -5.0).all() and (out[-band:] == -5.0).all()
    assert np.array_equal(out[band:-band].reshape(num_chunks, num_samples), want)


def test_gather_chunks_refuses_bad_tables(gpu_device):
    from pyannote_audio_amd import frames as frame_ops
    wav = torch.zeros(1000, device=gpu_device)
    assert frame_ops.gather_chunks([wav], [], [], 400).shape == (0, 400)
    with pytest.raises(ValueError):
        frame_ops.gather_chunks([wav], [1], [0], 400)            # no such waveform
    with pytest.raises(ValueError):
        frame_ops.gather_chunks([wav], [0], [-4], 400)           # starts before the first sample
    with pytest.raises(ValueError):
        frame_ops.gather_chunks([wav], [0, 0], [0], 400)
    with pytest.raises(ValueError):
        frame_ops.gather_chunks([wav.double()], [0], [0], 400)


# ------------------------------------------------------------------------------------------------ pipeline
def _turns(ann):
    return [(s.start, s.end, l) for s, _, l in ann.itertracks(yield_label=True)]


def _files():
    from oracle.synthetic import synth_conversation
    files = [{"waveform": synth_conversation(sec, seed=seed)[0], "sample_rate": 16000, "uri": f"f{seed}"}
             for sec, seed in [(33.0, 5), (12.0, 3), (27.3, 8), (3.0, 21)]]       # (3 s: shorter than a window)
    files.append({"waveform": torch.zeros(1, 15 * 16000), "sample_rate": 16000, "uri": "silence"})
    files.append({"waveform": synth_conversation(10.0, seed=2)[0], "sample_rate": 16000, "uri": "f2"})
    return files


@pytest.fixture(scope="module")
def packed_case(pipeline_dir, gpu_device):
    """the pipeline, the six files and what `pipeline(file)` gives for each: computed once, shared"""
    import pyannote_audio_amd as pa
    pipeline = pa.Pipeline.from_pretrained(pipeline_dir).to(gpu_device)
    files = _files()
    want = [pipeline(copy.copy(f)) for f in files]
    assert _turns(want[0].speaker_diarization) != []
    return pipeline, files, want


def _same(got, files, want):
    assert [f["uri"] for f, _ in got] == [f["uri"] for f in files]
    for (f, out), ref in zip(got, want):
        assert _turns(out.speaker_diarization) == _turns(ref.speaker_diarization), f["uri"]
        assert _turns(out.exclusive_speaker_diarization) == _turns(ref.exclusive_speaker_diarization), f["uri"]
        assert np.array_equal(out.speaker_embeddings, ref.speaker_embeddings), f["uri"]


def test_packed_batch_equals_single_files(packed_case):
    pipeline, files, want = packed_case
    got = list(pipeline([copy.copy(f) for f in files], pack=True))
    _same(got, files, want)
    assert pipeline.last_pack_groups == [[f["uri"] for f in files]]
    # 54 chunks went through the segmentation network together; the embedding network saw those somebody speaks in
    # and at most one representative of the others
    total, embedded = pipeline.last_embedded_chunks
    assert total == 24 + 3 + 19 + 1 + 6 + 1 and 1 <= embedded <= total


def test_packed_batch_with_a_chunk_budget(packed_case):
    pipeline, files, want = packed_case
    got = list(pipeline([copy.copy(f) for f in files], pack=16))
    _same(got, files, want)
    # 24 | 3 | 19 | 1 + 6 + 1 chunks: the 33-second file alone exceeds the budget and is a group of its own
    assert pipeline.last_pack_groups == [["f5"], ["f3"], ["f8"], ["f21", "silence", "f2"]]
    with pytest.raises(ValueError):
        list(pipeline([copy.copy(f) for f in files], pack=0))


def test_packed_batch_honours_per_file_pipeline_kwargs(packed_case):
    pipeline, files, want = packed_case
    mine = [copy.copy(f) for f in files]
    mine[0]["pipeline_kwargs"] = {"num_speakers": 1}
    alone = pipeline(copy.copy(mine[0]))
    got = list(pipeline(mine, pack=True))
    assert len(got[0][1].speaker_diarization.labels()) == 1
    assert _turns(got[0][1].speaker_diarization) == _turns(alone.speaker_diarization)
    assert np.array_equal(got[0][1].speaker_embeddings, alone.speaker_embeddings)
    _same(got[1:], files[1:], want[1:])
    assert pipeline.last_pack_groups == [[f["uri"] for f in files]]


def test_packed_batch_with_files_in_which_nobody_speaks(packed_case, monkeypatch):
    """The synthetic model hears a speaker in digital silence, so the segmentation engine is wrapped here: the hard
    decisions of an all-zero waveform are cleared, in the per-file and in the packed entry point alike.  The silent
    file of a group gets the empty output `apply` gives it, its chunks stay out of the embedding launch (one
    representative apart), and its neighbours are untouched."""
    pipeline, files, want = packed_case
    engine = pipeline._segmentation.model.engine
    strided, packed = engine.forward_strided, engine.forward_files

    def hush_strided(wav, *args, **kwargs):
        logp, ml = strided(wav, *args, **kwargs)
        if not bool(wav.any()):
            ml.zero_()
        return logp, ml

    def hush_packed(wavs, chunk_stride, chunks_per_file, *args, **kwargs):
        logp, ml = packed(wavs, chunk_stride, chunks_per_file, *args, **kwargs)
        bounds = np.concatenate([[0], np.cumsum(chunks_per_file)])
        for wav, a, b in zip(wavs, bounds[:-1], bounds[1:]):
            if not bool(wav.any()):
                ml[a:b] = 0
        return logp, ml

    monkeypatch.setattr(engine, "forward_strided", hush_strided)
    monkeypatch.setattr(engine, "forward_files", hush_packed)
    alone = pipeline(copy.copy(files[4]))
    assert _turns(alone.speaker_diarization) == [] and alone.speaker_embeddings.shape[0] == 0
    hushed = want[:4] + [alone] + want[5:]
    got = list(pipeline([copy.copy(f) for f in files], pack=True))
    _same(got, files, hushed)
    assert pipeline.last_pack_groups == [[f["uri"] for f in files]]
    total, embedded = pipeline.last_embedded_chunks
    assert total == 54 and embedded <= total - 5              # six silent chunks, one representative
    # a group in which nobody speaks at all: no embedding stage
    quiet = [dict(files[4], uri=uri) for uri in ("q0", "q1", "q2")]
    got = list(pipeline(quiet, pack=True))
    assert [f["uri"] for f, _ in got] == ["q0", "q1", "q2"] and pipeline.last_pack_groups == [["q0", "q1", "q2"]]
    for _, out in got:
        assert _turns(out.speaker_diarization) == [] and out.speaker_embeddings.shape == alone.speaker_embeddings.shape


def test_pack_falls_back_with_a_hook(packed_case):
    pipeline, files, want = packed_case
    seen = []

    def hook(step, artefact, file=None, total=None, completed=None):
        seen.append(step)

    list(pipeline([copy.copy(f) for f in files[:2]], pack=True))
    assert pipeline.last_pack_groups != []
    got = list(pipeline([copy.copy(f) for f in files], pack=True, hook=hook))
    _same(got, files, want)
    assert pipeline.last_pack_groups == [] and "embeddings" in seen
    got = list(pipeline.apply_batch([copy.copy(f) for f in files[:3]], joint_clustering=True, pack=True))
    assert pipeline.last_pack_groups == [] and len(got) == 3


def test_abandoned_packed_iterator_leaves_the_next_call_working(packed_case):
    pipeline, files, want = packed_case
    it = iter(pipeline([copy.copy(f) for f in files], pack=16))
    first = next(it)
    it.close()
    assert first[0]["uri"] == "f5"
    assert _turns(first[1].speaker_diarization) == _turns(want[0].speaker_diarization)
    _same(list(pipeline([copy.copy(f) for f in files], pack=16)), files, want)
