"""Time one `StreamBank.push` (pyannote_audio_amd.online, csrc/online.hip) with every slot ready (GPU).

Seeded synthetic models (those of the test suite), 5-s chunks, 0.5-s steps, latency = the chunk; N in {1, 16, 64, 256}
streams, each fed its own stretch of a synthetic conversation until its window is full.  Then, per N:

  * one push of N blocks, host clock from the host blocks to the decisions on the host: median of `--runs` runs
    [min, max], the N alternating round by round, after `--warmup` rounds;
  * the same push split by device events: upload and windows / segmentation / statistics + masks + embeddings /
    cluster_step / emit, and the host clock of the download;
  * the two new kernels alone, by device events on the inputs of a real step, next to the numpy model of the test
    suite (tests/online_model.py) on the same inputs: the yardstick of what the step would cost per stream on the host;
  * N banks of one stream pushed one after another (measured for N <= 16, N x the bank of one above that).

The real-time budget: N streams are sustained iff a push of N takes less than one step.  Writes
profiles/online_timing.txt (or --out)."""
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


def line(name, values, scale=1e3):
    return f"{name:64s} {statistics.median(values) * scale:10.3f} ms   [{min(values) * scale:.3f}, " \
           f"{max(values) * scale:.3f}]"


class Feed:
    """N streams of one bank, every slot open, and the audio they are fed"""

    def __init__(self, bank, wav):
        self.bank, self.wav = bank, wav
        self.slots = [bank.open() for _ in range(bank.num_slots)]
        self.at = 0
        for _ in range(bank.steps_per_window - 1):
            self.push()

    def blocks(self):
        step, n = self.bank.step_samples, self.wav.numel()
        rows = [self.wav[(self.at + 7919 * s) % (n - step):][:step] for s in self.slots]
        return torch.stack(rows)

    def push(self):
        out = self.bank.push(self.blocks(), self.slots)
        self.at += self.bank.step_samples
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import online_model as om
    import pyannote_audio_amd.ffi as ffi
    import pyannote_audio_amd.model as pm
    from conftest import PYANNET_HPARAMS, WESPEAKER_HPARAMS
    from oracle.synthetic import calibrated_pyannet, calibrated_wespeaker, synth_conversation
    from pyannote_audio_amd import frames as frame_ops
    from pyannote_audio_amd import online
    ffi.require_gpu()
    device = torch.device("cuda:0")
    seg_o, emb_o = calibrated_pyannet(calib_seconds=60.0), calibrated_wespeaker(calib_seconds=24.0)
    seg = pm.PyanNet(seg_o.state_dict(), PYANNET_HPARAMS, pm.segmentation_specifications(5.0, True)).to(device)
    emb = pm.WeSpeakerResNet34(emb_o.state_dict(), WESPEAKER_HPARAMS, pm.embedding_specifications()).to(device)
    wav = synth_conversation(120.0, seed=5)[0].view(-1)
    options = dict(max_speakers=20, delta_new=0.7, device=device)
    lines = [f"tools/time_online.py --runs {args.runs} --warmup {args.warmup}",
             f"device: {torch.cuda.get_device_name(0)}; torch threads {torch.get_num_threads()}",
             "seeded synthetic PyanNet + WeSpeaker ResNet34, 5-s chunks, 0.5-s steps, latency 5 s, 20 speakers per stream, "
             "delta_new 0.7 (untuned)",
             f"median [min, max] of {args.runs} runs, the bank sizes alternating round by round", ""]

    feeds = {n: Feed(online.StreamBank(seg, emb, n, **options), wav) for n in args.streams}
    print("banks filled", flush=True)

    # ------------------------------------------------------------------------------------------------ whole pushes
    whole = {n: [] for n in feeds}
    for r in range(args.warmup + args.runs):
        for n, feed in feeds.items():
            blocks = feed.blocks()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = feed.bank.push(blocks, feed.slots)
            elapsed = time.perf_counter() - t0       # (the decisions are on the host: push ends with its download)
            feed.at += feed.bank.step_samples
            assert len(out) == n
            if r >= args.warmup:
                whole[n].append(elapsed)
        print(f"round {r + 1} of {args.warmup + args.runs} done", flush=True)
    lines += ["one push, every slot ready: host blocks -> decisions on the host (host clock)"]
    lines += [line(f"  N = {n}", whole[n]) for n in feeds]

    # ---------------------------------------------------------------------------------------------- split by events
    stages = ("windows", "segmentation", "embeddings", "cluster_step", "emit", "download")
    split = {n: {s: [] for s in stages} for n in feeds}
    for r in range(args.runs):
        for n, feed in feeds.items():
            marks = []

            def hook(name, marks=marks):
                if name == "download":
                    marks.append((name, time.perf_counter()))
                    return
                event = torch.cuda.Event(enable_timing=True)
                event.record()
                if name == "emit":                   # host clock of the download starts when emit is queued
                    marks.append((name, event, time.perf_counter()))
                else:
                    marks.append((name, event))

            torch.cuda.synchronize()
            first = torch.cuda.Event(enable_timing=True)
            first.record()
            feed.bank.stage_hook = hook
            feed.push()
            feed.bank.stage_hook = None
            before = first
            for mark in marks:
                if mark[0] == "download":
                    continue
                split[n][mark[0]].append(before.elapsed_time(mark[1]) * 1e-3)
                before = mark[1]
            emit_mark, download_mark = marks[-2], marks[-1]
            # queue -> host copy done, minus the device time still ahead of the copy when emit was queued is not
            # separable on the host: reported as the host clock from "emit queued" to "rows on the host"
            split[n]["download"].append(download_mark[1] - emit_mark[2])
    lines += ["", "the same push by device events: `windows` = upload of the blocks, buffer update, upload of the step "
                  "table and the gather of the ready windows; `embeddings` includes the chunk statistics and the masks; "
                  "`download` is the host clock from the moment emit is queued to the rows on the host, so it contains the "
                  "device work still in flight at that moment"]
    for n in feeds:
        lines += [f"  N = {n}"] + [line(f"    {s}" + (" (host clock, see above)" if s == "download" else ""),
                                        split[n][s]) for s in stages]

    # ------------------------------------------------------------------------------- the two kernels and their model
    lines += ["", "the two new kernels alone (device events around the Python wrappers, which upload the slot and frame tables; "
                  "inputs of a real step on the device) and the numpy model of the test suite on the same inputs (host clock)"]
    for n, feed in feeds.items():
        b = feed.bank
        M = n
        slots = np.asarray(feed.slots, dtype=np.int32)
        flat = b.buffer.index_select(0, torch.as_tensor(slots, dtype=torch.long, device=device)).view(-1)
        _, dseg = b.seg_model.engine.forward_strided(flat, b.window, M, b.window, want_logp=False, want_multilabel=True)
        active, clean = frame_ops.chunk_stats(dseg)
        masks = frame_ops.embedding_masks(dseg, clean, b.exclude_overlap, b._min_num_frames())
        demb = b.emb_model.engine.forward_strided(flat, b.window, M, b.window, masks)
        c = b._streams[0].chunks
        start = np.full(M, online.start_frame(c, b.step, b.frames), dtype=np.int64)
        frm = np.full(M, b._streams[0].emitted, dtype=np.int64)
        to = np.full(M, online.start_frame(c + 1, b.step, b.frames), dtype=np.int64)
        E = int((to - frm).max())
        state = [t.clone() for t in (b.centroid_sum, b.centroid_n, b.acc_sum, b.acc_cnt)]
        host_in = [t.cpu().numpy() for t in (demb, active, clean, dseg)]
        t_step, t_emit, t_model_step, t_model_emit = [], [], [], []
        for r in range(args.warmup + args.runs):
            csum, cn, asum, acnt = (t.clone() for t in state)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            mp = online.cluster_step(slots, demb, active, clean, csum, cn, b.min_active_frames, b.min_update_frames,
                                     b.delta_new)
            e[1].record()
            out = online.emit(slots, dseg, mp, start, frm, to, asum, acnt, E)
            e[2].record()
            e[2].synchronize()
            h = [t.cpu().numpy() for t in state]
            t0 = time.perf_counter()
            want_mp = om.cluster_step(slots, host_in[0], host_in[1], host_in[2], h[0], h[1], b.min_active_frames,
                                      b.min_update_frames, b.delta_new)
            t1 = time.perf_counter()
            want = om.emit(slots, host_in[3], want_mp, start, frm, to, h[2], h[3], E)
            t2 = time.perf_counter()
            assert (mp.cpu().numpy() == want_mp).all() and (out.cpu().numpy() == want).all()
            assert (cn.cpu().numpy() == h[1]).all() and csum.cpu().numpy().tobytes() == h[0].tobytes()
            if r >= args.warmup:
                t_step.append(e[0].elapsed_time(e[1]) * 1e-3)
                t_emit.append(e[1].elapsed_time(e[2]) * 1e-3)
                t_model_step.append(t1 - t0)
                t_model_emit.append(t2 - t1)
        lines += [f"  N = {n} (results equal with ==)", line("    pao_cluster_step", t_step),
                  line("    numpy model of cluster_step", t_model_step), line("    pao_emit", t_emit),
                  line("    numpy model of emit", t_model_emit)]

    # ------------------------------------------------------------------------------------------- N banks of one
    lines += ["", "N banks of one stream, pushed one after another (host clock for all N pushes)"]
    singles = [Feed(online.StreamBank(seg, emb, 1, **options), wav) for _ in range(min(16, max(args.streams)))]
    one_by_one = {}
    for n in args.streams:
        if n > len(singles):
            continue
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
    base = statistics.median(whole[min(feeds)]) / min(feeds)
    for n in args.streams:
        batched = statistics.median(whole[n])
        alone = one_by_one.get(n, n * base)
        how = "measured" if n in one_by_one else f"{n} x the bank of one"
        lines += [f"  N = {n}: one bank {batched * 1e3:.3f} ms, {n} banks of one {alone * 1e3:.3f} ms ({how}): "
                  f"batching is {alone / batched:.2f}x"]

    # ------------------------------------------------------------------------------------------------------ budget
    step = feeds[min(feeds)].bank.step
    within = [n for n in feeds if statistics.median(whole[n]) < step]
    lines += ["", f"real-time budget: a push of N must take less than one step ({step * 1e3:.0f} ms)"]
    if within:
        n = max(within)
        t = statistics.median(whole[n])
        lines += [f"  largest measured N within the budget: {n} streams, {t * 1e3:.3f} ms per push: {step / t:.1f}x faster than "
                  f"real time, {(step - t) * 1e3:.1f} ms of margin per step"]
    else:
        lines += ["  no measured N is within the budget"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(text)


if __name__ == "__main__":
    main()
