"""Regenerates tests/golden/metrics_v1.npz: what the REFERENCE'S OWN frame-level metrics make of seeded inputs.

  file mode    utils/metric.py `discrete_diarization_error_rate` (equal speaker counts) and
               `DiscreteDiarizationErrorRate.compute_components` on array pairs (its speaker padding)
  chunk mode   torchmetrics/functional/audio/diarization_error_rate.py `diarization_error_rate` with
               `return_components`, for reduce = "batch" and "chunk"

The reference is loaded where it lies by tests/refharness.py.  It is a valid yardstick only while its own number
formats hold the sums, and this file ASSERTS that they do:
  * file mode sums in np.half: every sum (total, per-frame, per-speaker) stays <= 2048, below which every integer
    is representable, and the components it returns are compared with tests/metrics_truth.py here;
  * chunk mode sums in float32: B * S * F < 2^24 in every case;
  * chunk mode picks its permutation from a float32 cost: chunks whose float64 gap between the two cheapest
    permutations is below `metrics_truth.permutation_margin` are listed as `near_tie` and left out of component
    comparisons; at most 1 % of all chunks may be (checked here).  Chunks with EXACT ties (duplicated score rows: every
    optimum gives the same counts) are never left out.
Scores are stored as float16 where their float32 values are exactly those, targets as uint8.

Run from the repository root:  python tests/golden/make_metrics_golden.py"""
import os
import sys

os.environ.setdefault("PYANNOTE_SKIP_DEPENDENCY_CHECK", "1")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import metrics_truth  # noqa: E402
import refharness  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "metrics_v1.npz")
KEYS = ("false alarm", "missed detection", "confusion", "total")


def file_cases():
    """name -> (reference (T, Sr) uint8, hypothesis (T, Sh) uint8)"""
    rng = np.random.default_rng(20241017)

    def pair(T, Sr, Sh, density=0.3, agree=0.8):
        S = max(Sr, Sh)
        base = (rng.random((T, S)) < density)
        ref = base[:, :Sr]
        hyp = np.where(rng.random((T, S)) < agree, base, rng.random((T, S)) < density)[:, rng.permutation(S)][:, :Sh]
        return ref.astype(np.uint8), hyp.astype(np.uint8)

    out = {}
    for T in (1, 63, 64, 65, 589):
        out[f"square_T{T}_S3"] = pair(T, 3, 3)
    out["square_T600_S7"] = pair(600, 7, 7, density=0.25)
    out["square_T63_S32"] = pair(63, 32, 32, density=0.5)
    out["square_T589_S1"] = pair(589, 1, 1, density=0.5)
    out["all_one_T64_S3"] = (np.ones((64, 3), np.uint8), np.ones((64, 3), np.uint8))
    out["all_one_T63_S32"] = (np.ones((63, 32), np.uint8), np.ones((63, 32), np.uint8))
    out["all_zero_T65_S3"] = (np.zeros((65, 3), np.uint8), np.zeros((65, 3), np.uint8))
    out["silent_reference_T65_S3"] = (np.zeros((65, 3), np.uint8), pair(65, 3, 3)[1])
    out["silent_hypothesis_T65_S3"] = (pair(65, 3, 3)[0], np.zeros((65, 3), np.uint8))
    # the class pads the narrower side
    out["padded_T589_S3_S7"] = pair(589, 3, 7, density=0.2)
    out["padded_T589_S7_S3"] = pair(589, 7, 3, density=0.2)
    out["padded_T64_S1_S32"] = pair(64, 1, 32, density=0.4)
    out["padded_T65_S32_S1"] = pair(65, 32, 1, density=0.4)
    return out


def chunk_cases():
    """name -> (preds (B, Sp, F) float32 with float16 values, target (B, St, F) uint8, thresholds (Q,) float32 or a
    Python float)"""
    import torch
    rng = np.random.default_rng(20241018)
    default = torch.linspace(0.0, 1.0, 51).numpy()
    grid64 = np.linspace(0.0, 1.0, 64).astype(np.float32)

    def target(B, S, F):
        t = np.zeros((B, S, F), dtype=np.uint8)
        for b in range(B):
            for s in range(S):
                pos = int(rng.integers(0, 120))
                while pos < F:
                    n = int(rng.integers(20, 200))
                    t[b, s, pos:pos + n] = 1
                    pos += n + int(rng.integers(20, 250))
        return t

    def scores(t, flip=0.15):
        B, S, F = t.shape
        on = np.where(rng.random(t.shape) < flip, 1 - t, t)
        p = np.where(on == 1, rng.uniform(0.4, 1.0, t.shape), rng.uniform(0.0, 0.6, t.shape))
        p = np.stack([p[b, rng.permutation(S)] for b in range(B)])
        return p.astype(np.float16).astype(np.float32)

    out = {}
    for S in (1, 2, 3, 4):
        t = target(12, S, 589)
        out[f"S{S}_F589_Q51"] = (scores(t), t, default)
    t = target(12, 3, 293)
    out["S3_F293_Q64"] = (scores(t), t, grid64)
    t = target(12, 4, 293)
    out["S4_F293_scalar"] = (scores(t), t, 0.5)
    t = target(12, 2, 589)
    out["S2_F589_scalar"] = (scores(t), t, 0.5)
    t = target(12, 5, 589)
    out["S5_F589_Q51"] = (scores(t), t, default)
    # scores that sit exactly on thresholds: `>` must stay a strict float32 comparison
    t = target(8, 3, 293)
    on_grid = default[rng.integers(0, 51, t.shape)]
    out["on_threshold_S3_F293_Q51"] = (on_grid.astype(np.float32), t, default)
    # exact ties: two identical score rows (either assignment gives the same counts), and all-equal rows
    t = target(8, 3, 293)
    p = scores(t)
    p[:, 1] = p[:, 0]
    p[4:, 2] = p[4:, 0]
    out["duplicate_rows_S3_F293_Q51"] = (p, t, default)
    # fewer score rows than target speakers, and the other way round: the narrower side is padded with zeros
    t = target(8, 3, 293)
    out["padded_preds_S2_S3"] = (scores(t)[:, :2], t, default)
    out["padded_target_S4_S2"] = (scores(target(8, 4, 293)), t[:, :2], default)
    return out


def generate() -> dict:
    import torch
    out = {}
    with refharness.reference_modules(third_party=True) as ref:
        metric = ref.load("pyannote.audio.utils.metric")
        functional = ref.load("pyannote.audio.torchmetrics.functional.audio.diarization_error_rate")

        names = []
        for name, (reference, hypothesis) in file_cases().items():
            names.append(name)
            # every half-precision sum of the reference's function is an integer <= 2048
            for a in (reference, hypothesis):
                assert a.sum() <= 2048 and a.shape[0] <= 2048, name
            padded = reference.shape[1] != hypothesis.shape[1]
            if padded:
                klass = metric.DiscreteDiarizationErrorRate
                components = klass.__new__(klass).compute_components(reference, hypothesis)
            else:
                der, components = metric.discrete_diarization_error_rate(reference, hypothesis)
                out[f"file/{name}/der"] = np.array(der, dtype=np.float64)
            values = [float(components[k]) for k in KEYS]
            assert all(v == int(v) for v in values), (name, values)
            got = dict(zip(KEYS, (int(v) for v in values)))
            assert got == metrics_truth.file_components(reference, hypothesis), \
                (name, got, metrics_truth.file_components(reference, hypothesis))
            out[f"file/{name}/reference"] = reference
            out[f"file/{name}/hypothesis"] = hypothesis
            out[f"file/{name}/components"] = np.array([got[k] for k in KEYS], dtype=np.int64)
            print(f"file/{name}: {got}")
        out["file_cases"] = np.array(names)

        names = []
        num_chunks = num_near = 0
        for name, (preds, target, thresholds) in chunk_cases().items():
            names.append(name)
            B, Sp, F = preds.shape
            S = max(Sp, target.shape[1])
            assert B * S * F < 2 ** 24, name
            half = np.array_equal(preds.astype(np.float16).astype(np.float32), preds)
            scalar = isinstance(thresholds, float)
            thr = thresholds if scalar else torch.from_numpy(np.asarray(thresholds, dtype=np.float32))
            p, t = torch.from_numpy(preds), torch.from_numpy(target.astype(np.float32))
            for reduce in ("batch", "chunk"):
                if reduce == "chunk" and not scalar:
                    # (the reference's own division (B, Q) / (B,) does not broadcast: components only)
                    components = functional._der_update(p, t, threshold=thr, reduce=reduce)
                else:
                    der, components = functional.diarization_error_rate(p, t, threshold=thr, reduce=reduce,
                                                                        return_components=True)
                    out[f"chunk/{name}/{reduce}_der"] = der.numpy()
                for key, value in zip(("false_alarm", "missed_detection", "confusion", "total"), components):
                    value = value.numpy().astype(np.float64)
                    assert np.array_equal(value, np.rint(value)), (name, key)
                    out[f"chunk/{name}/{reduce}_{key}"] = value.astype(np.int64)
            # near-ties of the permutation, on the padded arrays the reference permutes
            pp = np.pad(preds, ((0, 0), (0, S - Sp), (0, 0)))
            tt = np.pad(target, ((0, 0), (0, S - target.shape[1]), (0, 0)))
            _, gap, tied = metrics_truth.chunk_permutations(pp, tt)
            near = gap < metrics_truth.permutation_margin(S, F)
            # (zero-padded target rows are interchangeable too: the same counts whichever score row plays which)
            if not name.startswith(("duplicate_rows", "padded_target")):
                assert (tied == 0).all(), f"{name}: an exact tie outside the constructed cases"
            num_chunks += B
            num_near += int(near.sum())
            out[f"chunk/{name}/preds"] = preds.astype(np.float16) if half else preds
            out[f"chunk/{name}/target"] = target
            out[f"chunk/{name}/thresholds"] = np.asarray(thresholds, dtype=np.float64 if scalar else np.float32)
            out[f"chunk/{name}/near_tie"] = near
            print(f"chunk/{name}: B = {B}, S = {S}, F = {F}, near ties = {int(near.sum())}, "
                  f"smallest gap = {gap.min():.3e} (margin {metrics_truth.permutation_margin(S, F):.3e})")
        assert num_near <= 0.01 * num_chunks, f"{num_near} of {num_chunks} chunks are near ties"
        out["chunk_cases"] = np.array(names)
    return out


def main():
    out = generate()
    np.savez_compressed(PATH, **out)
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
