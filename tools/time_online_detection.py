"""Time one `DetectionBank.push` (pyannote_audio_amd.online_detection, csrc/online_detect.hip) with every slot ready
(GPU).

Seeded synthetic models (those of the test suite), 5-s chunks, 0.5-s steps, latency = the chunk; N in {1, 16, 64, 256}
streams, each fed its own stretch of a synthetic conversation until its window is full.  Then, per N:

  * one push of N blocks, host clock from the host blocks to the values, states and regions on the host: median of
    `--runs` runs [min, max], after `--warmup` rounds; the bank sizes and the two kinds of bank alternate round by round;
  * the same step through `online.StreamBank` (segmentation, embeddings, clustering, emission), in the same rounds:
    what dropping the embedding stage saves;
  * the same streams as N banks of one, pushed one after another (measured for every N);
  * `pao_detect_step` alone through the C ABI by device events, on the scores of a real step, next to the numpy model
    of the test suite (tests/online_detect_model.py) on the same inputs (host clock), results compared with ==.

Nothing is concluded here: the numbers are written to profiles/online_detection_timing.txt (or --out) as they come."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from time_online import Feed, line  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_detection_timing.txt"))
    args = ap.parse_args()
    import online_detect_model as dm
    import pyannote_audio_amd.ffi as ffi
    import pyannote_audio_amd.model as pm
    from conftest import PYANNET_HPARAMS, WESPEAKER_HPARAMS
    from oracle.synthetic import calibrated_pyannet, calibrated_wespeaker, synth_conversation
    from pyannote_audio_amd import online
    from pyannote_audio_amd.online_detection import DetectionBank, DetectionState
    ffi.require_gpu()
    lib = ffi.load()
    device = torch.device("cuda:0")
    seg_o, emb_o = calibrated_pyannet(calib_seconds=60.0), calibrated_wespeaker(calib_seconds=24.0)
    seg = pm.PyanNet(seg_o.state_dict(), PYANNET_HPARAMS, pm.segmentation_specifications(5.0, True)).to(device)
    emb = pm.WeSpeakerResNet34(emb_o.state_dict(), WESPEAKER_HPARAMS, pm.embedding_specifications()).to(device)
    wav = synth_conversation(120.0, seed=5)[0].view(-1)
    detect = dict(min_duration_on=0.1, min_duration_off=0.1, device=device)
    diarize = dict(max_speakers=20, delta_new=0.7, device=device)
    lines = [f"tools/time_online_detection.py --runs {args.runs} --warmup {args.warmup}",
             f"device: {torch.cuda.get_device_name(0)}; torch threads {torch.get_num_threads()}",
             "seeded synthetic powerset PyanNet (+ WeSpeaker ResNet34 for StreamBank), 5-s chunks, 0.5-s steps, latency "
             "5 s; detection: any speaker, onset = offset = 0.5, min_duration_on = min_duration_off = 0.1 s",
             f"median [min, max] of {args.runs} runs; the bank sizes and the two kinds of bank alternate round by round",
             ""]

    feeds = {n: Feed(DetectionBank(seg, n, **detect), wav) for n in args.streams}
    diar = {n: Feed(online.StreamBank(seg, emb, n, **diarize), wav) for n in args.streams}
    print("banks filled", flush=True)

    # ------------------------------------------------------------------------------------------------ whole pushes
    whole, whole_diar = {n: [] for n in feeds}, {n: [] for n in feeds}
    for r in range(args.warmup + args.runs):
        for n in feeds:
            for feed, times in ((feeds[n], whole), (diar[n], whole_diar)):
                blocks = feed.blocks()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = feed.bank.push(blocks, feed.slots)
                elapsed = time.perf_counter() - t0     # (the results are on the host: push ends with its download)
                feed.at += feed.bank.step_samples
                assert len(out) == n
                if r >= args.warmup:
                    times[n].append(elapsed)
        print(f"round {r + 1} of {args.warmup + args.runs} done", flush=True)
    lines += ["one DetectionBank.push, every slot ready: host blocks -> values, states and final regions on the host "
              "(host clock)"]
    lines += [line(f"  N = {n}", whole[n]) for n in feeds]
    lines += ["", "the same step through StreamBank.push (segmentation, embeddings, cluster_step, emit), in the same rounds"]
    lines += [line(f"  N = {n}", whole_diar[n]) for n in feeds]
    lines += [f"  N = {n}: detection {statistics.median(whole[n]) * 1e3:.3f} ms, diarization "
              f"{statistics.median(whole_diar[n]) * 1e3:.3f} ms: {statistics.median(whole_diar[n]) / statistics.median(whole[n]):.2f}x"
              for n in feeds]

    # ------------------------------------------------------------------------------------------- N banks of one
    lines += ["", "N detection banks of one stream, pushed one after another (host clock for all N pushes)"]
    singles = [Feed(DetectionBank(seg, 1, **detect), wav) for _ in range(max(args.streams))]
    one_by_one = {}
    for n in args.streams:
        times = []
        for r in range(args.warmup + args.runs):
            blocks = [f.blocks() for f in singles[:n]]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for f, b in zip(singles[:n], blocks):
                f.bank.push(b, f.slots)
            elapsed = time.perf_counter() - t0
            for f in singles[:n]:
                f.at += f.bank.step_samples
            if r >= args.warmup:
                times.append(elapsed)
        one_by_one[n] = statistics.median(times)
        lines += [line(f"  N = {n}, measured", times)]
    for n in args.streams:
        batched = statistics.median(whole[n])
        lines += [f"  N = {n}: one bank {batched * 1e3:.3f} ms, {n} banks of one {one_by_one[n] * 1e3:.3f} ms: "
                  f"batching is {one_by_one[n] / batched:.2f}x"]

    # ---------------------------------------------------------------------------------- the kernel and its model
    lines += ["", "pao_detect_step alone (device events around the C call; scores of a real step and the step tables on "
                  "the device) and the numpy model of the test suite on the same inputs (host clock)"]
    for n, feed in feeds.items():
        b = feed.bank
        M = n
        slots = np.asarray(feed.slots, dtype=np.int32)
        flat = b.buffer.index_select(0, torch.as_tensor(slots, dtype=torch.long, device=device)).view(-1)
        _, scores = b.model.engine.forward_strided(flat, b.window, M, b.window, want_logp=False, want_multilabel=True)
        c = b._streams[0].chunks
        start = online.start_frame(c, b.step, b.frames)
        rows = np.stack([np.full(M, start), np.full(M, b._streams[0].emitted),
                         np.full(M, online.start_frame(c + 1, b.step, b.frames)), np.zeros(M)]).astype(np.int64)
        E = int((rows[2] - rows[1]).max())
        cap = E // 2 + 2
        d_rows, d_slots = torch.from_numpy(rows).to(device), torch.from_numpy(slots).to(device)
        on, off = b.onset.astype(np.float32), b.offset.astype(np.float32)
        names = [name for name, _, _ in DetectionState.FIELDS]
        entry = {name: getattr(b.state, name).clone() for name in names}
        host_scores = scores.cpu().numpy()
        window, warm = b._window.cpu().numpy(), b._warm.cpu().numpy()
        grid = (b.grid.start, b.grid.duration, b.grid.step)
        outs = [torch.empty(shape, dtype=dtype, device=device) for shape, dtype in (
            ((M, E, b.K), torch.float32), ((M, E, b.K), torch.uint8), ((M, b.K), torch.int32),
            ((M, b.K, cap, 2), torch.float64), ((M, b.K, cap), torch.int32))]
        t_kernel, t_model = [], []
        for r in range(args.warmup + args.runs):
            state = {name: t.clone() for name, t in entry.items()}
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            rc = lib.pao_detect_step(
                ffi.ptr(d_slots), slots.ctypes.data, M, b.num_slots, ffi.ptr(scores), 1, b.F, b.S, 1,
                ffi.ptr(b._window), ffi.ptr(b._warm), b.epsilon, b.missing, ffi.ptr(d_rows[0]), ffi.ptr(d_rows[1]),
                ffi.ptr(d_rows[2]), ffi.ptr(d_rows[3]), rows.ctypes.data, *grid, on.ctypes.data, off.ctypes.data,
                b.min_duration_on.ctypes.data, b.min_duration_off.ctypes.data, b.R, E, cap,
                *(ffi.ptr(state[name]) for name in names), *(ffi.ptr(t) for t in outs), ffi.stream())
            e[1].record()
            e[1].synchronize()
            assert rc == 0, lib.pa_last_error().decode()
            host = {name: t.cpu().numpy() for name, t in entry.items()}
            t0 = time.perf_counter()
            want = dm.detect_step(host, slots, host_scores, True, window, warm, b.epsilon, b.missing, *rows, grid,
                                  b.onset, b.offset, b.min_duration_on, b.min_duration_off, E, cap)
            t1 = time.perf_counter()
            for got, w in zip(outs, want):
                assert np.array_equal(got.cpu().numpy(), w, equal_nan=True)
            assert dm.same_state({name: t.cpu().numpy() for name, t in state.items()}, host)
            if r >= args.warmup:
                t_kernel.append(e[0].elapsed_time(e[1]) * 1e-3)
                t_model.append(t1 - t0)
        lines += [f"  N = {n}, E = {E} frames (results and state equal with ==)", line("    pao_detect_step", t_kernel),
                  line("    numpy model of detect_step", t_model)]

    step = feeds[min(feeds)].bank.step
    lines += ["", f"real-time budget: a push of N must take less than one step ({step * 1e3:.0f} ms)"]
    lines += [f"  N = {n}: {statistics.median(whole[n]) * 1e3:.3f} ms per push, {step / statistics.median(whole[n]):.1f}x "
              "faster than real time" for n in feeds]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(text)


if __name__ == "__main__":
    main()
