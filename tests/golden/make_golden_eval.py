"""Writes tests/golden/g14_eval.npz: the evaluation metric of the reference's test_step / test_epoch_end on the cases of
tests/eval_ref.py, computed with sklearn exactly as test_step calls it.

    python tests/golden/make_golden_eval.py

Per case and row grouping ("batch": one row per loader batch, what the reference computes; "scan": one row per scan)
it records the IoU rows, the per-class means in percent, the mean IoU and the CSV text; and the CSV text of a run over
two targets.  CPU only; needs scikit-learn (1.7.2 when the fixture was written)."""
import csv
import io
import json
import os
import sys
import warnings

import numpy as np
from sklearn.metrics import jaccard_score

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import eval_ref as E  # noqa: E402


def step_row(preds, labels):
    """one row of test_step: jaccard_score over the rows it is given, -1 for the classes absent from their labels"""
    if preds.shape[0] == 0:
        return -np.ones(E.C)          # sklearn refuses empty input; no label is present, so every class is masked
    iou_tmp = jaccard_score(preds, labels, average=None, labels=np.arange(0, E.C), zero_division=0.)
    present_labels = np.unique(labels)
    present_labels = present_labels[present_labels != E.IGNORE]
    iou = -np.ones_like(iou_tmp)
    iou[present_labels] = iou_tmp[present_labels]
    return iou


def rows_of(case, mode):
    group = case["batch_of_scan"][case["scan"]] if mode == "batch" else case["scan"]
    n = (case["batch_of_scan"].max() + 1) if mode == "batch" else case["batch_of_scan"].shape[0]
    return np.stack([step_row(case["preds"][group == g], case["labels"][group == g]) for g in range(n)])


def epoch_end(rows):
    x = rows.copy()
    x[x == -1] = float("nan")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # a class absent from every row stays NaN
        per_class = np.nanmean(x, axis=0) * 100
        return per_class, np.nanmean(per_class, axis=0)


def csv_text(entries, sources=E.SOURCES):
    """entries: [(target name, rows)]; the text test_epoch_end appends to a fresh file"""
    f = io.StringIO(newline="")
    w = csv.writer(f)
    for o, (target, rows) in enumerate(entries):
        per_class, average = epoch_end(rows)
        if o == 0:
            w.writerow(["source", "target"] + list(E.CLASS_NAMES) + ["mean"])
        w.writerow([sources, target] + [str(round(p, 2)).replace(".", ",") for p in per_class] +
                   [str(round(float(average), 2)).replace(".", ",")])
    return f.getvalue()


def main():
    arrays, meta = {}, {"cases": {}, "sklearn": __import__("sklearn").__version__}
    rows = {}
    for name in E.CASES:
        case = E.make_case(name)
        for k, v in case.items():
            arrays[f"{name}/{k}"] = v.astype(np.int16 if k == "scan" else np.int8)
        rec = {"rows": int(case["preds"].shape[0]), "scans": int(case["batch_of_scan"].shape[0])}
        for mode in E.MODES:
            r = rows[name, mode] = rows_of(case, mode)
            per_class, mean = epoch_end(r)
            arrays[f"{name}/{mode}/rows"], arrays[f"{name}/{mode}/per_class"] = r, per_class
            arrays[f"{name}/{mode}/mean"] = np.float64(mean)
            rec[f"csv_{mode}"] = csv_text([("nusc35k", r)])
        meta["cases"][name] = rec
    # what the cases have to show
    c = E.make_case("absent_but_predicted")
    assert not np.isin(c["labels"], [5, 6]).any() and np.isin(c["preds"], [5, 6]).any()
    assert (rows["absent_but_predicted", "batch"][:, 5:] == -1).all()
    c = E.make_case("labelled_never_predicted")
    assert np.isin(c["labels"], [4, 5, 6]).any() and not np.isin(c["preds"], [4, 5, 6]).any()
    assert (rows["labelled_never_predicted", "batch"][:, 4:] == 0).all()
    assert (rows["all_ignored_batch", "batch"][1] == -1).all() and (rows["all_ignored_batch", "batch"][0] >= 0).all()
    assert (rows["empty_scan", "scan"][1] == -1).all() and (rows["all_present", "batch"] > 0).all()
    pb, ps = (epoch_end(rows["batch_vs_scan", m])[0] for m in E.MODES)
    assert (np.abs(pb - ps) > 0.5).all(), (pb, ps)           # the two groupings give different tables
    meta["batch_vs_scan_gap"] = float(np.abs(pb - ps).min())
    for mode in E.MODES:
        meta[f"two_targets_csv_{mode}"] = csv_text([(t, rows[name, mode]) for t, name in E.TWO_TARGETS])
    meta["two_targets"] = [list(t) for t in E.TWO_TARGETS]
    arrays["meta"] = np.asarray(json.dumps(meta))
    np.savez_compressed(E.G14, **arrays)
    print(E.G14, os.path.getsize(E.G14), "bytes")


if __name__ == "__main__":
    main()
