"""eval_target --point-level --save-labels end to end on three tiny SemanticKITTI files: every label file holds one
uint32 per record of its scan, in file order, equal to what plain torch makes of the same logits; the -points.csv holds
the IoU rows of the numpy confusion of those labels; the voxel-level CSV and point clouds of the same invocation are the
bytes of a run without the new flags; the bf16 path writes files of the same sizes."""
import csv
import json
import os
import shutil

import numpy as np
import pytest
import torch

import pointlabels_ref as P
from lidog_amd import eval_target, evaluate, scans
from lidog_amd.checkpoint import load_lightning_checkpoint, save_lightning_checkpoint
from lidog_amd.train import build_model

pytestmark = pytest.mark.gpu

OUT_IDS = [10, 30, 40, 48, 72, 50, 70]          # the id written for every common class: not the identity, injective
FILL = 250
BATCHES = [[0, 1], [2]]                         # --batch 2 over three scans


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("points"))
    tree, label_map, lut = P.write_tiny_kitti_tree(os.path.join(root, "kitti"))
    inv = os.path.join(root, "common2kitti.json")
    with open(inv, "w") as f:
        json.dump({"learning_map_inv": dict({str(c): i for c, i in enumerate(OUT_IDS)}, **{"-1": FILL})}, f)
    torch.manual_seed(5)
    model = build_model("MinkUNet34")
    ckpts = {}
    for name in ("points", "plain", "bf16"):
        os.makedirs(os.path.join(root, name, "checkpoints"))
        ckpts[name] = os.path.join(root, name, "checkpoints", "fresh.ckpt")
    save_lightning_checkpoint(model, ckpts["points"])
    for name in ("plain", "bf16"):
        shutil.copyfile(ckpts["points"], ckpts[name])

    def argv(name):
        return ["--checkpoint", ckpts[name], "--model", "MinkUNet34", "--sources", "SemanticKITTI", "--target-files",
                f"SemanticKITTI={tree}", "--label-maps", label_map, "--batch", "2", "--rows", "scan", "--save-predictions"]

    flags = ["--point-level", "--save-labels", "--inverse-label-map", inv]
    res = {"points": eval_target.main(argv("points") + flags), "plain": eval_target.main(argv("plain")),
           "bf16": eval_target.main(argv("bf16") + flags + ["--precision", "bf16"])}
    return {"root": root, "tree": tree, "lut": lut, "ckpts": ckpts, "res": res}


def _label_file(runs, name, f):
    return os.path.join(runs["root"], name, "predictions", "SemanticKITTI", "sequences", "08", "predictions", f"{f:06d}.label")


def _records(runs, f):
    return np.fromfile(os.path.join(runs["tree"], "sequences", "08", "velodyne", f"{f:06d}.bin"), np.float32).reshape(-1, 4)


def test_label_files_equal_plain_torch(runs):
    model = build_model("MinkUNet34")
    load_lightning_checkpoint(model, runs["ckpts"]["points"])
    model.eval()
    data = scans.FileScans(scans.listing("SemanticKITTI", runs["tree"], "validation"), runs["lut"])
    batches = [(data.batch(ids, "cuda"), [data.item(i)[0] for i in ids]) for ids in BATCHES]
    run = evaluate.Predictor(model)                                  # evaluate.predict over the same stream of batches
    out_ids = np.asarray(OUT_IDS, dtype=np.uint32)
    for k, (ids, (b, items)) in enumerate(zip(BATCHES, batches)):
        nxt = batches[k + 1][0]["coords_int"] if k + 1 < len(batches) else None
        _, logits = run(b["coords_int"], b["source_features0"], nxt)
        pred = logits.cpu().max(dim=1)[1].numpy()
        start = 0
        for i, item in zip(ids, items):
            rec = _records(runs, i)
            keep = P.radius_mask_np(rec[:, :3], 50.0)
            inverse = item["inverse_map"].cpu().numpy()
            nv = item["coordinates"].shape[0]
            assert 0 < keep.sum() < rec.shape[0] and inverse.shape[0] == keep.sum() and nv < keep.sum()
            path = _label_file(runs, "points", i)
            assert os.path.getsize(path) == 4 * rec.shape[0]         # exactly one uint32 per record
            got = np.fromfile(path, dtype="<u4")
            assert not (got >> 16).any()                             # no instance half
            want = np.full(rec.shape[0], FILL, dtype=np.uint32)
            want[keep] = out_ids[pred[start + inverse]]
            assert np.array_equal(got, want), i
            assert (got[~keep] == FILL).all() and np.isin(got[keep], out_ids).all()
            start += nv
        assert start == logits.shape[0]
    assert sorted(os.listdir(os.path.dirname(_label_file(runs, "points", 0)))) == [f"{f:06d}.label" for f in range(3)]
    assert runs["res"]["points"][0]["label_files"] == 3
    assert runs["res"]["points"][0]["label_paths"] == [_label_file(runs, "points", f) for f in range(3)]


def test_points_csv_is_the_confusion_of_the_label_files(runs, tmp_path):
    res = runs["res"]["points"][0]
    class_of = {i: c for c, i in enumerate(OUT_IDS)}
    counts = np.zeros((3, 7, 7), dtype=np.int64)
    kept = 0
    for f in range(3):
        rec = _records(runs, f)
        keep = P.radius_mask_np(rec[:, :3], 50.0)
        raw = np.fromfile(os.path.join(runs["tree"], "sequences", "08", "labels", f"{f:06d}.label"), dtype=np.int32)
        true = runs["lut"][raw & 0xFFFF].astype(np.int64)[keep]
        pred = np.array([class_of[int(i)] for i in np.fromfile(_label_file(runs, "points", f), dtype="<u4")[keep]])
        sel = true != -1
        counts[f] = np.bincount(true[sel] * 7 + pred[sel], minlength=49).reshape(7, 7)
        kept += int(sel.sum())
    assert np.array_equal(res["point_counts"], counts) and counts.sum() == kept > 0
    rows = evaluate.iou_rows(evaluate.point_iou_counts(counts), "scan")
    assert rows.shape == (3, 7) and np.array_equal(res["point_iou_rows"], rows)
    per_class, mean = evaluate.mean_iou_rows(rows)
    assert res["point_mean_iou"] == mean and np.array_equal(res["point_per_class_iou"], per_class, equal_nan=True)
    path = os.path.join(runs["root"], "points", "results", "SemanticKITTI-TO-SemanticKITTI-points.csv")
    assert res["points_csv"] == path
    want = evaluate.write_results_csv(str(tmp_path), "SemanticKITTI", "SemanticKITTI", rows, evaluate.CLASS_NAMES,
                                      file_targets="SemanticKITTI-points")
    assert open(path).read() == open(want).read()
    with open(path, newline="") as f:
        table = list(csv.reader(f))
    assert table[0] == ["source", "target"] + list(evaluate.CLASS_NAMES) + ["mean"] and len(table) == 2
    assert all("." not in v for v in table[1][2:])                   # decimal commas, as the voxel CSV
    # the point level is another metric than the voxel level: several points per voxel, unlabelled points left out
    assert res["point_counts"].sum() > res["counts"][:, 1:].sum()


def _tree_bytes(folder):
    out = {}
    for d, _, files in os.walk(folder):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, folder)] = open(p, "rb").read()
    return out


def test_voxel_outputs_are_untouched(runs):
    with_points = {n: _tree_bytes(os.path.join(runs["root"], "points", n)) for n in ("results", "predictions")}
    plain = {n: _tree_bytes(os.path.join(runs["root"], "plain", n)) for n in ("results", "predictions")}
    assert sorted(plain["results"]) == ["SemanticKITTI-TO-SemanticKITTI.csv"]
    assert sorted(with_points["results"]) == ["SemanticKITTI-TO-SemanticKITTI-points.csv", "SemanticKITTI-TO-SemanticKITTI.csv"]
    assert sorted(plain["predictions"]) == sorted(f"SemanticKITTI/{k}/{i}.ply" for k in ("labels", "preds") for i in range(3))
    for kind in ("results", "predictions"):
        for rel, raw in plain[kind].items():
            assert with_points[kind][rel] == raw, rel               # byte for byte
    extra = sorted(set(with_points["predictions"]) - set(plain["predictions"]))
    assert extra == [f"SemanticKITTI/sequences/08/predictions/{f:06d}.label" for f in range(3)]
    a, b = runs["res"]["points"][0], runs["res"]["plain"][0]
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["iou_rows"], b["iou_rows"])
    assert set(b) == {"target", "checkpoint_epoch", "per_class_iou", "mean_iou", "rows", "rows_per", "scans", "scans_per_s",
                      "csv", "iou_rows", "counts"}                   # a run without the flags reports what it did


def test_bf16_writes_the_same_files(runs):
    res = runs["res"]["bf16"][0]
    for f in range(3):
        assert os.path.getsize(_label_file(runs, "bf16", f)) == 4 * _records(runs, f).shape[0]
        got = np.fromfile(_label_file(runs, "bf16", f), dtype="<u4")
        assert np.isin(got, OUT_IDS + [FILL]).all()
    with open(res["points_csv"], newline="") as f:
        table = list(csv.reader(f))
    vals = [float(v.replace(",", ".")) for v in table[1][2:]]
    assert len(vals) == 8 and all(np.isfinite(v) and 0.0 <= v <= 100.0 for v in vals)    # every class occurs in the files
    assert np.isfinite(res["point_mean_iou"]) and res["point_counts"].sum() == runs["res"]["points"][0]["point_counts"].sum()
