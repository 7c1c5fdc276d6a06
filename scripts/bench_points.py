"""The point-level path on the same box, the same batch:

  (a) device time of the keep index of 8 files plus the point labels and point confusion of their batch
      (lidog_scan_keep_rows x 8, lidog_point_labels) against a torch composition of the same result (the float32 radius
      mask and a cumsum per file, one argmax, two index_selects and a bincount), between HIP events, alternating rep by
      rep, median over --reps; the two results are compared before anything is timed.  The scans are synthetic
      kitti120k scans written out as SemanticKITTI records (a twentieth of the points moved beyond 50 m), voxelised by
      the library; the logits are random.
  (b) scans/s of `evaluate.TargetEvaluator` over a SemanticKITTI tree of such files (MinkUNet34BEV forward-only, file
      reads included) with and without `points`, alternating round by round, host clock from a synchronised device to
      the result on the host; one untimed pass of each first.  Every round's reading is printed.

One JSON line per measurement.

    python scripts/bench_points.py --batch 8 --batches 16 --rounds 7 --reps 50
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RADIUS, CLASSES = 50.0, 7


def scan_file(seed):
    """(records float32 [n, 4], raw labels int32 [n]) of synthetic scan `seed`: raw id = class + 1 in the lower half, an
    instance id in the upper"""
    from lidog_amd import synth
    pts, labels = synth.scan_points_labels(int(seed), "kitti120k")
    rng = np.random.default_rng(seed)
    pts = np.asarray(pts, dtype=np.float32).copy()
    far = rng.random(pts.shape[0]) < 0.05
    pts[far] *= (60.0 / np.maximum(np.linalg.norm(pts[far], axis=1, keepdims=True), 1e-3)).astype(np.float32)
    rec = np.concatenate([pts, rng.random((pts.shape[0], 1), dtype=np.float32)], axis=1)
    raw = (np.asarray(labels) + 1).astype(np.uint32) | (rng.integers(0, 1 << 16, pts.shape[0]).astype(np.uint32) << 16)
    return np.ascontiguousarray(rec, dtype=np.float32), raw.view(np.int32)


def label_map():
    return {k: k - 1 for k in range(CLASSES + 1)}


def write_tree(root, n):
    for d in ("velodyne", "labels"):
        os.makedirs(os.path.join(root, "sequences", "08", d), exist_ok=True)
    for f in range(n):
        rec, raw = scan_file(10 ** 6 + f)
        rec.tofile(os.path.join(root, "sequences", "08", "velodyne", f"{f:06d}.bin"))
        raw.tofile(os.path.join(root, "sequences", "08", "labels", f"{f:06d}.label"))
    return root


def bench_kernels(data, batch, reps):
    import torch
    from lidog_amd import evaluate
    ids = list(range(batch))
    b = data.batch(ids, "cuda")
    items = [data.point_item(i) for i in ids]
    v = b["coords_int"].shape[0]
    logits = torch.randn((v, CLASSES), device="cuda")
    counts = torch.zeros((batch, CLASSES, CLASSES), dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    lut = items[0]["lut"].long()
    r2 = torch.tensor(np.float32(RADIUS) ** 2, device="cuda")

    def kernels(out=None):
        pin = evaluate.point_inputs(items)
        return evaluate.point_labels(logits, pin["row_off"], pin["kept_off"], pin["vox_off"], pin["keep_row"],
                                     pin["inverse_map"], labels_raw=pin["labels_raw"], lut=pin["lut"],
                                     label_mask=pin["label_mask"], counts=out, err=err)

    def composition():
        pred = logits.argmax(dim=1)
        outs, cnts, vox = [], [], 0
        for it in items:
            p = it["points_raw"].view(-1, it["stride"])[:, :3]
            keep = (p * p).sum(dim=1) < r2
            keep_row = torch.cumsum(keep, 0) - 1
            voxel = torch.index_select(it["inverse_map"], 0, keep_row[keep]) + vox
            pk = torch.index_select(pred, 0, voxel)
            out = torch.zeros(p.shape[0], dtype=torch.int64, device="cuda")
            out[keep] = pk
            true = torch.index_select(lut, 0, (it["labels_raw"] & 0xFFFF).long()[keep])
            sel = true >= 0
            cnts.append(torch.bincount(true[sel] * CLASSES + pk[sel], minlength=CLASSES * CLASSES).view(CLASSES, CLASSES))
            outs.append(out)
            vox += it["voxels"]
        return torch.cat(outs), torch.stack(cnts)

    got, got_counts = kernels()
    want, want_counts = composition()
    evaluate.check_point_error(err)
    same = bool(torch.equal(got.view(torch.int32).long(), want)) and bool(torch.equal(got_counts, want_counts))
    ms = {"kernels": [], "torch": []}
    for r in range(reps + 3):
        for name, f in (("kernels", lambda: kernels(counts)), ("torch", composition)):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            e.record()
            e.synchronize()
            if r >= 3:
                ms[name].append(a.elapsed_time(e))
    res = {"bench": "point_labels", "batch": batch, "file_rows": int(sum(it["rows"] for it in items)),
           "kept_rows": int(sum(it["kept"] for it in items)), "voxels": int(v), "reps": reps, "same_result": same,
           "note": "HIP events around the calls: allocations, the concatenations and the launches included"}
    for name, x in ms.items():
        res[f"{name}_us_median"] = statistics.median(x) * 1e3
        res[f"{name}_us_min"] = min(x) * 1e3
    res["torch_over_kernels"] = res["torch_us_median"] / res["kernels_us_median"]
    return res


def bench_evaluator(model, data, batch, rounds):
    import torch
    from lidog_amd import evaluate
    n = len(data)
    ev = evaluate.TargetEvaluator(model)
    points = evaluate.PointPath.of(data)

    def plain():
        data.keep_raw = False
        return ev.run(evaluate.dataset_batches(data, batch), n, rows="scan")["mean"]

    def with_points():
        data.keep_raw = True
        return ev.run(evaluate.dataset_batches(data, batch), n, rows="scan", points=points)["point_mean"]

    paths = {"voxel_only": plain, "with_points": with_points}
    means = {k: f() for k, f in paths.items()}                    # untimed: first use of every kernel and buffer
    rates = {k: [] for k in paths}
    for _ in range(rounds):
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            rates[k].append(n / (time.perf_counter() - t0))
    res = {"bench": "target_evaluator_points", "model": "MinkUNet34BEV", "batch": batch, "scans": n, "rounds": rounds,
           "voxel_mean_iou": means["voxel_only"], "point_mean_iou": means["with_points"]}
    for k, r in rates.items():
        res[f"{k}_scans_per_s_median"] = statistics.median(r)
        res[f"{k}_scans_per_s"] = [round(x, 2) for x in r]
    res["with_over_without"] = res["with_points_scans_per_s_median"] / res["voxel_only_scans_per_s_median"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    import torch
    from lidog_amd import scans
    from lidog_amd.train import build_model
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, a.batch * a.batches)
        data = scans.FileScans(scans.listing("SemanticKITTI", root, "validation"), scans.label_lut(label_map()),
                               keep_raw=True)
        print(json.dumps(bench_kernels(data, a.batch, a.reps)), flush=True)
        model = build_model("MinkUNet34BEV").eval()
        print(json.dumps(bench_evaluator(model, data, a.batch, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
