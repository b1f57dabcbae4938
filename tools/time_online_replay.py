"""Time the replay route of the online diarization (pyannote_audio_amd.online, csrc/online_replay.hip) against the
streaming route it replaces for recorded files (GPU).

Seeded synthetic models (those of the test suite), 5-s chunks, 0.5-s steps, latency = the chunk, 20 speakers per
stream.  Recordings are a 120-s synthetic conversation repeated, every repetition rolled by another offset.  Median of
`--runs` runs [min, max] after `--warmup` rounds, the routes alternating round by round.  Parts (`--parts`):

  a  `OnlineSpeakerDiarization.apply` of one recorded file of 10 and of 60 minutes: `replay=False` (one push per step,
     the route the pipeline had) and `replay=True`, host clock from the waveform to the Annotation; the new route once
     more split by device events into the front end (every chunk through both networks) and the replay kernel;
  b  `tuning.OnlineTuner` on a 4 x 4 x 4 grid over three files (10 + 20 + 30 minutes): `prepare` and `sweep` by host
     clock, against (1) the literal loop -- a fresh pipeline per candidate, streaming `apply` per file, the metric --
     measured on `--literal` candidates and scaled to 64, and (2) the cached front end driven through `cluster_step` +
     `emit` once per chunk, measured on `--literal` candidates and scaled;
  c  the kernel alone (device events around `online.replay_jobs`, tables uploaded inside) at J = 1, 64 and 256 jobs of
     an hour-sized file, the jobs differing in delta_new.

Writes profiles/online_replay_timing.txt (or --out)."""
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


def line(name, values, scale=1e3, unit="ms"):
    return f"{name:72s} {statistics.median(values) * scale:12.3f} {unit}   [{min(values) * scale:.3f}, " \
           f"{max(values) * scale:.3f}]"


def recording(base, activity, minutes):
    """`minutes` of audio from the 120-s conversation, every repetition rolled by another offset -> (wave, activity)"""
    n = int(minutes * 60 * 16000)
    waves, acts, at, k = [], [], 0, 0
    while at < n:
        shift = 7919 * 16 * k
        waves.append(torch.roll(base, shift))
        acts.append(np.roll(activity, shift, axis=1))
        at += base.numel()
        k += 1
    return torch.cat(waves)[:n].contiguous(), np.concatenate(acts, axis=1)[:, :n]


def reference(activity, uri):
    from pyannote_audio_amd.core import Annotation, Segment
    out = Annotation(uri=uri)
    for s, row in enumerate(activity):
        edges = np.flatnonzero(np.diff(np.concatenate([[0], row.astype(np.int8), [0]])))
        for a, b in zip(edges[::2], edges[1::2]):
            out[Segment(a / 16000, b / 16000), s] = f"ref{s}"
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parts", nargs="+", default=["a", "b", "c"])
    ap.add_argument("--minutes", type=float, nargs="+", default=[10.0, 60.0])
    ap.add_argument("--literal", type=int, default=2, help="candidates the two baselines of part b are measured on")
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks every recording (a quick check of the tool)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_replay_timing.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import pyannote_audio_amd.ffi as ffi
    import pyannote_audio_amd.model as pm
    from conftest import PYANNET_HPARAMS, WESPEAKER_HPARAMS
    from oracle.synthetic import calibrated_pyannet, calibrated_wespeaker, synth_conversation
    from pyannote_audio_amd import online
    from pyannote_audio_amd.tuning import OnlineTuner
    ffi.require_gpu()
    device = torch.device("cuda:0")
    seg_o, emb_o = calibrated_pyannet(calib_seconds=60.0), calibrated_wespeaker(calib_seconds=24.0)
    seg = pm.PyanNet(seg_o.state_dict(), PYANNET_HPARAMS, pm.segmentation_specifications(5.0, True)).to(device)
    emb = pm.WeSpeakerResNet34(emb_o.state_dict(), WESPEAKER_HPARAMS, pm.embedding_specifications()).to(device)
    base, activity = synth_conversation(120.0, seed=5)
    base, activity = base.view(-1), np.asarray(activity)
    options = dict(max_speakers=20, delta_new=0.7)

    def pipeline(**more):
        return online.OnlineSpeakerDiarization(segmentation=seg, embedding=emb, **{**options, **more}).to(device)

    def as_file(wave, uri, act=None):
        file = {"waveform": wave.view(1, -1), "sample_rate": 16000, "uri": uri}
        if act is not None:
            file["annotation"] = reference(act, uri)
        return file

    lines = [f"tools/time_online_replay.py --runs {args.runs} --warmup {args.warmup} --parts {' '.join(args.parts)}"
             + (f" --scale {args.scale:g} (every duration below is multiplied by it)" if args.scale != 1.0 else ""),
             f"device: {torch.cuda.get_device_name(0)}; torch threads {torch.get_num_threads()}",
             "seeded synthetic PyanNet + WeSpeaker ResNet34, 5-s chunks, 0.5-s steps, latency 5 s, 20 speakers per stream, "
             "delta_new 0.7 (untuned); recordings: a 120-s synthetic conversation repeated",
             f"median [min, max] of {args.runs} runs after {args.warmup} warm-up round(s), the routes alternating round by "
             "round", ""]

    def write():                                 # after every part: a run cut short keeps what it measured
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")

    # ------------------------------------------------------------------------------------------- a: one recorded file
    if "a" in args.parts:
        pipe = pipeline()
        lines += ["(a) OnlineSpeakerDiarization.apply of one recorded file, waveform -> Annotation (host clock)"]
        for minutes in args.minutes:
            wave, _ = recording(base, activity, minutes * args.scale)
            file = as_file(wave, f"{minutes:g}min")
            streamed, replayed, front, kernel, rest = [], [], [], [], []
            for r in range(args.warmup + args.runs):
                t_stream, a = timed(lambda: pipe.apply(file))
                t_replay, b = timed(lambda: pipe.apply(file, replay=True))
                assert list(a.itertracks(yield_label=True)) == list(b.itertracks(yield_label=True)), \
                    "the two routes give different turns"
                # the new route once more, split by device events
                bank = pipe.bank(1)
                marks = {}

                def hook(name, marks=marks):
                    event = torch.cuda.Event(enable_timing=True)
                    event.record()
                    marks[name] = event

                bank.stage_hook = hook
                hook("start")
                t_split, _ = timed(lambda: bank.annotation_of(bank.replay(bank.front_ends([wave]))[0].decisions))
                if r >= args.warmup:
                    streamed.append(t_stream)
                    replayed.append(t_replay)
                    front.append(marks["start"].elapsed_time(marks["front_end"]) * 1e-3)
                    kernel.append(marks["replay_state"].elapsed_time(marks["replay"]) * 1e-3)
                    rest.append(t_split - front[-1] - kernel[-1])
                print(f"(a) {minutes:g} min: round {r + 1} done", flush=True)
            C = bank.schedule(wave.numel())[0]
            lines += [f"  {minutes:g} minutes of audio, {C} chunks",
                      line("    replay=False: one push per step (the route before this change)", streamed),
                      line("    replay=True: front ends of all chunks, one replay launch", replayed),
                      line("      of which, by device events: the front end (both networks)", front),
                      line("      of which, by device events: pao_replay, one job", kernel),
                      line("      the rest of that run (tables, concatenation, download, Annotation)", rest),
                      f"    replay=True is {statistics.median(streamed) / statistics.median(replayed):.1f}x the streaming "
                      f"route; the same turns (checked every round)"]
            write()
        lines += [""]

    # ------------------------------------------------------------------------------------------------- b: the tuner
    if "b" in args.parts:
        files = []
        for minutes in (10.0, 20.0, 30.0):
            wave, act = recording(base, activity, minutes * args.scale)
            files.append(as_file(wave, f"{minutes:g}min", act))
        grid = ([0.4, 0.6, 0.8, 1.0], [0.1, 0.25, 0.5, 1.0], [0.5, 1.0, 1.5, 2.0])
        pipe = pipeline()
        t_prepare, t_sweep = [], []
        for r in range(args.warmup + args.runs):
            tp, tuner = timed(lambda: OnlineTuner(pipe).prepare(files))
            ts, result = timed(lambda: tuner.sweep(*grid))
            if r >= args.warmup:
                t_prepare.append(tp)
                t_sweep.append(ts)
            print(f"(b) tuner round {r + 1} done", flush=True)
        candidates = tuner.candidates(*grid)
        picked = [candidates[i] for i in np.linspace(0, len(candidates) - 1, args.literal).astype(int)]
        # (1) the literal loop
        t_literal = []
        for params in picked:
            def literal(params=params):
                p = pipeline(**params)
                metric = p.get_metric()
                for file in files:
                    metric(file["annotation"], p.apply(file), uem=file.get("annotated"))
                return abs(metric)
            t, loss = timed(literal)
            entry = next(e for e in result["entries"] if e["params"] == params)
            assert loss == entry["loss"], f"{params}: literal loop {loss!r}, tuner {entry['loss']!r}"
            t_literal.append(t)
            print(f"(b) literal candidate done in {t:.1f} s", flush=True)
        # (2) the cached front end through cluster_step + emit, once per chunk
        bank = tuner.bank
        t_chunks = []
        for params in picked:
            def per_chunk(params=params):
                active_f, update_f = bank.threshold_frames(params["min_active"], params["min_update"])
                metric = pipe.get_metric()
                for file, fe in zip(files, tuner.front_ends):
                    csum = torch.zeros((1, bank.K, bank.D), dtype=torch.float64, device=device)
                    cn = torch.zeros((1, bank.K), dtype=torch.int32, device=device)
                    acc_sum = torch.zeros((1, bank.R, bank.K), dtype=torch.int32, device=device)
                    acc_cnt = torch.zeros((1, bank.R), dtype=torch.int32, device=device)
                    rows = []
                    for c in range(fe.num_chunks + 1):
                        g0, ga, gb = fe.schedule[c].tolist()
                        if c < fe.num_chunks:
                            mp = online.cluster_step([0], fe.emb[c:c + 1], fe.active[c:c + 1], fe.clean[c:c + 1], csum,
                                                     cn, active_f, update_f, params["delta_new"])
                            chunk = fe.seg[c:c + 1]
                        else:
                            mp = torch.full((1, bank.S), -1, dtype=torch.int32, device=device)
                            chunk = torch.zeros((1, bank.F, bank.S), dtype=torch.uint8, device=device)
                        rows.append(online.emit([0], chunk, mp, [g0], [ga], [gb], acc_sum, acc_cnt,
                                                max(1, gb - ga))[0, :gb - ga])
                    decisions = torch.cat(rows).cpu().numpy()               # one download per file
                    metric(file["annotation"], bank.annotation_of(decisions, uri=file["uri"]), uem=file.get("annotated"))
                return abs(metric)
            t, loss = timed(per_chunk)
            entry = next(e for e in result["entries"] if e["params"] == params)
            assert loss == entry["loss"], f"{params}: per-chunk loop {loss!r}, tuner {entry['loss']!r}"
            t_chunks.append(t)
            print(f"(b) per-chunk candidate done in {t:.1f} s", flush=True)
        n = len(candidates)
        tuned = statistics.median(t_prepare) + statistics.median(t_sweep)
        lit, chk = statistics.mean(t_literal) * n, statistics.median(t_prepare) + statistics.mean(t_chunks) * n
        lines += [f"(b) OnlineTuner, {n} candidates (4 x 4 x 4) on three files of 10 + 20 + 30 minutes "
                  f"({sum(fe.num_chunks for fe in tuner.front_ends)} chunks), host clock",
                  line("  prepare: the front ends of the three files, once", t_prepare, 1.0, "s "),
                  line(f"  sweep: {tuner.jobs} jobs through pao_replay, Annotations, metric", t_sweep, 1.0, "s "),
                  f"    {result['evaluations']} (candidate, file) evaluations, {result['shared_evaluations']} of them shared; best "
                  f"{result['best']['params']} at loss {result['best']['loss']:.4f}",
                  line(f"  literal loop, one candidate (measured on {len(picked)}; the same loss, checked)", t_literal, 1.0,
                       "s "),
                  line(f"  cached front end through cluster_step + emit per chunk, one candidate (measured on {len(picked)};"
                       " the same loss)", t_chunks, 1.0, "s "),
                  f"  all {n} candidates: tuner {tuned:.1f} s (prepare + sweep); literal loop {lit:.1f} s (scaled): "
                  f"{lit / tuned:.0f}x; per-chunk calls on the cached front end {chk:.1f} s (prepare + scaled): "
                  f"{chk / tuned:.1f}x", ""]
        write()

    # ------------------------------------------------------------------------------------------ c: the kernel alone
    if "c" in args.parts:
        bank = pipeline().bank(1)
        wave, _ = recording(base, activity, 60.0 * args.scale)
        fe = bank.front_end(wave)
        C = fe.num_chunks
        lines += [f"(c) pao_replay alone: J jobs of one hour-sized file ({C} chunks, {fe.total} frames), the jobs differing "
                  "in delta_new (device events around online.replay_jobs, which uploads the tables and zeroes map and out)"]
        active_f, update_f = bank.min_active_frames, bank.min_update_frames
        times = {J: [] for J in (1, 64, 256)}
        for r in range(args.warmup + args.runs):
            for J in times:
                jobs = [[0, active_f, update_f]] * J
                delta = np.linspace(0.3, 1.1, J) if J > 1 else np.array([0.7])
                offsets = np.stack([np.arange(J) * C, np.arange(J) * fe.total], axis=1)
                state = (torch.zeros((J, bank.K, bank.D), dtype=torch.float64, device=device),
                         torch.zeros((J, bank.K), dtype=torch.int32, device=device),
                         torch.zeros((J, bank.R, bank.K), dtype=torch.int32, device=device),
                         torch.zeros((J, bank.R), dtype=torch.int32, device=device))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                online.replay_jobs(fe.emb, fe.active, fe.clean, fe.seg, [[0, C, 0, fe.total]], fe.schedule, jobs, delta,
                                   offsets, *state)
                e1.record()
                e1.synchronize()
                if r >= args.warmup:
                    times[J].append(e0.elapsed_time(e1) * 1e-3)
        for J, t in times.items():
            lines += [line(f"  J = {J}", t),
                      f"    {statistics.median(t) / C * 1e6:.2f} us per step of one job; "
                      f"{statistics.median(t) / J * 1e3:.3f} ms per job"]
    write()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
