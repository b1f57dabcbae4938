"""Writes tests/golden/verification_v1.npz: the inputs of tests/verification_truth.small_cases() and, for
`distances` False and True, what sklearn.metrics.roc_curve followed by det_curve's lines gives for them
(pyannote.metrics.binary_classification.det_curve's published behaviour; pinned with scikit-learn 1.7.2).

    python tests/golden/make_verification_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from verification_truth import small_cases  # noqa: E402


def sklearn_det_curve(y_true, scores, distances):
    """det_curve as published, on top of sklearn's roc_curve -> (fpr, fnr, thresholds, eer, k)"""
    from sklearn.metrics import roc_curve
    scores = np.asarray(scores)
    if distances:
        scores = -scores
    fpr, tpr, thresholds = roc_curve(np.asarray(y_true) != 0, scores, pos_label=True)
    fnr = 1 - tpr
    if distances:
        thresholds = -thresholds
    k = np.where(fpr > fnr)[0][0]
    eer = 0.25 * (fpr[k - 1] + fpr[k] + fnr[k - 1] + fnr[k])
    return fpr, fnr, thresholds, float(eer), int(k)


def main():
    import sklearn
    arrays = {"sklearn_version": np.array(sklearn.__version__)}
    for name, (y_true, scores) in small_cases().items():
        arrays[f"{name}/y_true"] = y_true
        arrays[f"{name}/scores"] = scores
        for distances in (False, True):
            fpr, fnr, thresholds, eer, k = sklearn_det_curve(y_true, scores, distances)
            tag = f"{name}/{'distances' if distances else 'scores'}"
            arrays[f"{tag}/fpr"] = fpr
            arrays[f"{tag}/fnr"] = fnr
            arrays[f"{tag}/thresholds"] = thresholds.astype(np.float64)
            arrays[f"{tag}/eer"] = np.float64(eer)
            arrays[f"{tag}/k"] = np.int64(k)
    path = os.path.join(HERE, "verification_v1.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
