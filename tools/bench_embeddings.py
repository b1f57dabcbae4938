"""Speaker-verification throughput of the embedding path: SpeakerEmbedding.apply one file at a time against
apply_batch (ragged batches, EmbeddingEngine.forward_ragged), the equal-length rate of the same kernels, and the
sliding-window Inference of an embedding model.  Prints one JSON line.

Workload: a seeded list of 4 874 utterances (the size of VoxCeleb1-O), lengths log-normal around a 7 s median,
clipped to [4, 20] s, random audio, a seeded WeSpeaker ResNet34.  Every figure is the median of 3 timed passes after
one warm-up pass, with device synchronisation.

    python tools/bench_embeddings.py [--utterances 4874] [--single 256] [--out profiles/emb_verification.json]
    python tools/bench_embeddings.py --only batch      # one apply_batch pass (for a kernel trace)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 16000


def utterance_lengths(count: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    seconds = np.clip(np.exp(rng.normal(np.log(7.0), 0.4, count)), 4.0, 20.0)
    return np.round(seconds * SR).astype(np.int64)


def timed(fn, repeats: int = 3) -> float:
    """median wall time of `repeats` passes after one warm-up pass (device synchronised)"""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=4874)
    ap.add_argument("--single", type=int, default=256, help="files timed one at a time (a prefix of the list)")
    ap.add_argument("--hour", type=float, default=3600.0, help="seconds of the sliding-window file")
    ap.add_argument("--only", choices=["batch"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import __graft_entry__
    __graft_entry__.build()
    import pyannote_audio_amd.model as pm
    from oracle import seeded_wespeaker
    from pyannote_audio_amd import Inference, SpeakerEmbedding
    from pyannote_audio_amd.embedding import length_buckets

    dev = torch.device("cuda:0")
    hp = {"sample_rate": 16000, "num_channels": 1, "num_mel_bins": 80, "frame_length": 25, "frame_shift": 10,
          "dither": 0.0, "window_type": "hamming", "use_energy": False}
    model = pm.WeSpeakerResNet34(seeded_wespeaker(seed=4321).state_dict(), hp, pm.embedding_specifications()).to(dev)
    pipeline = SpeakerEmbedding(embedding=model)

    lengths = utterance_lengths(args.utterances)
    g = torch.Generator().manual_seed(1)
    audio = (0.1 * torch.randn(int(lengths.sum()), generator=g)).clamp(-1, 1)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    files = [{"waveform": audio[o:o + n].view(1, -1), "sample_rate": SR, "uri": f"utt{i:05d}"}
             for i, (o, n) in enumerate(zip(offsets, lengths))]
    total_s = float(lengths.sum()) / SR

    if args.only == "batch":
        pipeline.apply_batch(files)
        torch.cuda.synchronize()
        print(json.dumps({"apply_batch_pass": True, "utterances": len(files)}))
        return

    t_batch = timed(lambda: pipeline.apply_batch(files))
    single = files[:args.single]
    t_single = timed(lambda: [pipeline.apply(f) for f in single])
    single_s = float(lengths[:args.single].sum()) / SR

    # padding of the ragged launches: samples of the bucket's longest utterance / samples of the utterance
    srt = np.sort(lengths)
    padded = sum(int(srt[b1 - 1]) * (b1 - b0) for b0, b1 in length_buckets(srt))
    padding = 1.0 - float(lengths.sum()) / padded

    # the same total audio as equal-length chunks of the median length, already on the device
    eng = model.engine
    med = int(np.median(lengths))
    count = int(lengths.sum()) // med
    wav_d = audio[:count * med].to(dev)
    t_equal = timed(lambda: eng.forward_strided(wav_d, med, count, med))
    # the ragged engine pass alone (the utterances already on the device): what the 0.85 x target is about
    all_d = audio.to(dev)
    t_ragged = timed(lambda: eng.forward_ragged(all_d, offsets, lengths))
    del all_d

    hour = (0.1 * torch.randn(int(args.hour * SR), generator=g)).clamp(-1, 1).view(1, -1)
    sliding = Inference(model, window="sliding", duration=3.0, step=1.0)
    num_chunks = sum(Inference.num_chunks(hour.shape[1], 3 * SR, SR))
    t_slide = timed(lambda: sliding({"waveform": hour, "sample_rate": SR}))

    result = {
        "metric": "speaker_verification_embeddings", "device": torch.cuda.get_device_name(0),
        "utterances": len(files), "audio_s": round(total_s, 1), "median_s": round(med / SR, 3),
        "apply_batch_utt_per_s": round(len(files) / t_batch, 1),
        "apply_batch_audio_s_per_s": round(total_s / t_batch, 1),
        "apply_single_utt_per_s": round(len(single) / t_single, 1),
        "apply_single_audio_s_per_s": round(single_s / t_single, 1),
        "apply_single_files_timed": len(single),
        "batch_over_single": round(t_single / len(single) * len(files) / t_batch, 2),
        "padding_fraction": round(padding, 4),
        "equal_length_audio_s_per_s": round(count * med / SR / t_equal, 1),
        "ragged_engine_audio_s_per_s": round(total_s / t_ragged, 1),
        "ragged_over_equal_length": round((total_s / t_ragged) / (count * med / SR / t_equal), 3),
        "apply_batch_over_equal_length": round((total_s / t_batch) / (count * med / SR / t_equal), 3),
        "sliding_3s_1s_chunks_per_s": round(num_chunks / t_slide, 1), "sliding_file_s": args.hour,
        "seconds": {"apply_batch": round(t_batch, 4), "apply_single": round(t_single, 4),
                    "equal_length": round(t_equal, 4), "ragged_engine": round(t_ragged, 4), "sliding": round(t_slide, 4)},
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
