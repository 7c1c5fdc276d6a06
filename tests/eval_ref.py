"""Fixture G14 and the numpy restatement of the evaluation metric of test_step / test_epoch_end
(utils/pipelines/trainer_lighting.py:186-313, trainer_lighting_bev.py:265-383).

tests/golden/g14_eval.npz is written by tests/golden/make_golden_eval.py, which calls sklearn.metrics.jaccard_score
literally as test_step does.  Every case holds integer arrays: `preds`, `labels` (-1 = ignore), `scan` (the scan of
every row, numbered over the whole target) and `batch_of_scan` (the loader batch of every scan); the recorded results
are the IoU rows with one row per loader batch (the reference) and with one row per scan, the per-class means, the
mean IoU and the CSV text."""
import json
import os

import numpy as np

from helpers import GOLDEN

G14 = os.path.join(GOLDEN, "g14_eval.npz")
C = 7
IGNORE = -1
CLASS_NAMES = ("vehicle", "person", "road", "sidewalk", "terrain", "manmade", "vegetation")
SOURCES = "kitti120k"

# name -> (seed, rows of every scan grouped by loader batch, classes that may be labelled, classes that may be
# predicted, share of rows predicted as labelled, batches whose labels are all -1)
CASES = {
    "all_present": dict(seed=1, scans=[[700, 650, 720], [400, 900], [610]], label_classes=range(7),
                        pred_classes=range(7), hit=0.6, ignored_batches=()),
    "absent_but_predicted": dict(seed=2, scans=[[800, 500], [650, 700]], label_classes=range(5),
                                 pred_classes=range(7), hit=0.5, ignored_batches=()),
    "labelled_never_predicted": dict(seed=3, scans=[[900, 300], [450, 800]], label_classes=range(7),
                                     pred_classes=range(4), hit=0.7, ignored_batches=()),
    "all_ignored_batch": dict(seed=4, scans=[[600, 640], [500, 520]], label_classes=range(7), pred_classes=range(7),
                              hit=0.6, ignored_batches=(1,)),
    "empty_scan": dict(seed=5, scans=[[700, 0, 650], [480, 530]], label_classes=range(7), pred_classes=range(7),
                       hit=0.55, ignored_batches=()),
    # scans of very different sizes and accuracies in one batch: the mean of per-scan rows is not the row of the sum
    "batch_vs_scan": dict(seed=6, scans=[[1500, 60, 200], [90, 1300]], label_classes=range(7), pred_classes=range(7),
                          hit=(0.9, 0.1, 0.5, 0.2, 0.8), ignored_batches=()),
}
TWO_TARGETS = (("kitti120k", "all_present"), ("nusc35k", "batch_vs_scan"))
MODES = ("batch", "scan")


def make_case(name):
    """the integer arrays of a case, from its seed"""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    lab_cls, pred_cls = np.asarray(list(c["label_classes"])), np.asarray(list(c["pred_classes"]))
    preds, labels, scan, batch_of_scan = [], [], [], []
    s = 0
    for b, sizes in enumerate(c["scans"]):
        for n in sizes:
            hit = c["hit"][s] if isinstance(c["hit"], tuple) else c["hit"]
            l = rng.choice(np.concatenate([[IGNORE], lab_cls]), n)
            if b in c["ignored_batches"]:
                l[:] = IGNORE
            p = rng.choice(pred_cls, n)
            same = (rng.random(n) < hit) & np.isin(l, pred_cls)
            p[same] = l[same]
            preds.append(p)
            labels.append(l)
            scan.append(np.full(n, s))
            batch_of_scan.append(b)
            s += 1
    return {"preds": np.concatenate(preds).astype(np.int64), "labels": np.concatenate(labels).astype(np.int64),
            "scan": np.concatenate(scan).astype(np.int64), "batch_of_scan": np.asarray(batch_of_scan, np.int64)}


def load_g14():
    z = np.load(G14)
    meta = json.loads(str(z["meta"]))
    return meta, z


def case_arrays(z, name):
    return {k: z[f"{name}/{k}"].astype(np.int64) for k in ("preds", "labels", "scan", "batch_of_scan")}


# ------------------------------------------------------------------ the numpy restatement
def confusion_np(preds, labels, scan, n_scans, num_classes=C, ignore_label=IGNORE):
    """counts [n_scans, C + 1, C]: counts[scan, label + 1, pred]; row 0 takes every label outside 0..C-1 and the ignore
    label"""
    preds, labels, scan = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (preds, labels, scan))
    row = np.where((labels == ignore_label) | (labels < 0) | (labels >= num_classes), 0, labels + 1)
    counts = np.zeros((n_scans, num_classes + 1, num_classes), np.int64)
    ok = (scan >= 0) & (scan < n_scans)
    np.add.at(counts, (scan[ok], row[ok], preds[ok]), 1)
    return counts


def iou_rows_np(counts, rows="batch", batch_of_scan=None):
    """IoU rows from counts, class by class: tp / (true + pred - tp), 0 for an empty union, -1 for a class that no
    label of the row carries"""
    counts = np.asarray(counts, dtype=np.int64)
    if rows == "batch":
        b = np.zeros(counts.shape[0], np.int64) if batch_of_scan is None else np.asarray(batch_of_scan)
        groups = [counts[b == i].sum(axis=0) for i in np.unique(b)]
    else:
        groups = list(counts)
    out = []
    for m in groups:
        r = []
        for c in range(m.shape[1]):
            tp, true, pred = int(m[c + 1, c]), int(m[c + 1].sum()), int(m[:, c].sum())
            union = true + pred - tp
            r.append(-1.0 if true == 0 else (float(tp) / float(union) if union > 0 else 0.0))
        out.append(r)
    return np.asarray(out, dtype=np.float64).reshape(len(groups), counts.shape[2])


def epoch_end_np(rows):
    """(per-class IoU in percent, mean IoU) of test_epoch_end: -1 -> NaN, nan-mean over rows x 100, nan-mean"""
    import warnings
    x = np.array(rows, dtype=np.float64)
    x[x == -1] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        per_class = np.nanmean(x, axis=0) * 100
        return per_class, np.nanmean(per_class, axis=0)
