"""Writes tests/golden/g17_metrics.npz: the per-step training metrics of the reference's `log_losses` on the cases of
tests/metrics_ref.py, computed with the formulas of utils/pipelines/trainer_lighting.py:118-137 and
trainer_lighting_2d.py:203-262.

    python tests/golden/make_golden_metrics.py

Per case it records the inputs (logits, labels) and
  iou_all      sklearn.metrics.jaccard_score(preds, labels, average=None, labels=arange(C), zero_division=0.) over ALL
               rows, preds = logits.max(1)[1]: the source / mix / SN / RobustNet trainers
  iou_valid    the confusion-matrix Jaccard (intersection / union per class, 0 for an empty union) on the rows with
               label != -1, preds = softmax(logits).argmax(-1), a BEV tensor through .view(b, h, w, -1): the LiDOG
               trainers' JaccardIndex(num_classes, average=None) after their valid_idx filter
  present, occurs   torch.unique(labels, return_counts=True) without the ignore label
  mean_all, mean_valid   the mean over the present classes (source_iou), 0 if there are none
The trainers themselves cannot be run: pytorch-lightning and torchmetrics are not installed, so JaccardIndex is
restated from its definition, in float64.  The LiDOG trainer's softmax(...).argmax differs from the arg-max of the logits
only where rounding makes two probabilities equal; the generator asserts that NO row of a case differs (no row is left
out) and moves to the next seed otherwise.  CPU only; needs scikit-learn (1.7.2 when the fixture was written)."""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F
from sklearn.metrics import jaccard_score

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import metrics_ref as M  # noqa: E402


def confusion_jaccard(preds, labels, c):
    confmat = np.zeros((c, c), np.int64)
    np.add.at(confmat, (labels, preds), 1)
    inter = np.diag(confmat).astype(np.float64)
    union = (confmat.sum(0) + confmat.sum(1)).astype(np.float64) - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)


def case_results(logits, labels):
    c = M.C
    if logits.dim() == 4:
        b, _, h, w = logits.shape
        shaped = logits.view(b, h, w, -1)
    else:
        shaped = logits
    preds_max = shaped.reshape(-1, c).max(1)[1]
    preds_soft = F.softmax(shaped, dim=-1).argmax(dim=-1).view(-1)
    same = bool((preds_max == preds_soft).all())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        iou_all = jaccard_score(preds_max.numpy(), labels.numpy(), average=None, labels=np.arange(0, c),
                                zero_division=0.)
    valid = torch.logical_not(labels == M.IGNORE)
    iou_valid = confusion_jaccard(preds_soft[valid].numpy(), labels[valid].numpy(), c)
    present, occurs = torch.unique(labels, return_counts=True)
    occurs = occurs[present != M.IGNORE]
    present = present[present != M.IGNORE]
    p = present.numpy()
    return same, dict(iou_all=iou_all, iou_valid=iou_valid, present=p, occurs=occurs.numpy(),
                      mean_all=np.float64(np.mean(iou_all[p]) if p.size else 0.0),
                      mean_valid=np.float64(np.mean(iou_valid[p]) if p.size else 0.0))


def main():
    out = {}
    for name in M.CASES:
        seed = 0
        while True:
            logits, labels = M.make_case(name, seed)
            same, res = case_results(logits, labels)
            if same:
                break
            seed += 1
        out[f"{name}/seed"] = np.int64(seed)
        out[f"{name}/logits"] = logits.numpy()
        out[f"{name}/labels"] = labels.numpy()
        for k, v in res.items():
            out[f"{name}/{k}"] = v
        print(name, "seed", seed, "present", res["present"].tolist(), "mean_all", float(res["mean_all"]),
              "mean_valid", float(res["mean_valid"]))
    np.savez_compressed(M.G17, **out)
    print(M.G17, os.path.getsize(M.G17), "bytes")


if __name__ == "__main__":
    main()
