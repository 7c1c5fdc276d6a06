"""The point <-> voxel kernels (csrc/field.hip) against the torch formulation of the same operators, on the same box,
alternating: device time (HIP events around --reps launches, median over --rounds, both sides taking turns) at the size
of --kernel-batch kitti120k scans, --points-per-voxel points in every voxel:

  floor    lidog_field_floor                 vs  floor(q / s) * s, a range select and .int()
  lists    lidog_field_lists                 vs  a stable argsort of the inverse map + bincount + cumsum
  reduce   lidog_field_reduce (average)      vs  zeros.index_add_(inverse, x) / counts          (atomics: order not fixed)
  gather   lidog_field_gather                vs  x.index_select(0, inverse)
  interp   lidog_interp_fwd / lidog_interp_bwd  vs  eight index_select / index_add_ passes with the weights as tensors

Every index tensor and weight the torch side needs is built before the clock.  One JSON line per case.

Then TargetEvaluator over --eval-scans scan files (written to a temporary SemanticKITTI tree from synthetic scans: every
voxel's points at random positions inside it, the voxel's label) with PointPath(interp="nearest") and
interp="trilinear", alternating: seconds per run and the point-level mIoU both ways.  The model is freshly
initialised unless --checkpoint names one, so the mIoU column only says how often the two rules disagree, not which is
better.

    python scripts/bench_field.py --rounds 7 --reps 50
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C_FEATURES, C_LOGITS = 32, 7


def _alternate(fns, rounds, reps):
    """{name: median ms per call}: every round times `reps` launches of each function in turn between HIP events"""
    import torch
    for f in fns.values():           # first use of every kernel
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            e.record()
            e.synchronize()
            ms[k].append(a.elapsed_time(e) / reps)
    return {k: statistics.median(v) for k, v in ms.items()}


def _record(case, C, rows, t, rounds, reps, diff):
    print(json.dumps({"bench": "field", "case": case, "C": C, "rows": int(rows), "hip_us": round(1e3 * t["hip"], 2),
                      "torch_us": round(1e3 * t["torch"], 2), "torch_over_hip": round(t["torch"] / t["hip"], 2),
                      "max_abs_diff": diff, "rounds": rounds, "reps": reps}), flush=True)


def bench_kernels(kernel_batch, per_voxel, rounds, reps):
    import torch
    import lidog_amd.me as ME
    from lidog_amd import _lib, synth
    from lidog_amd._lib import call, ptr
    b = synth.make_batch(range(kernel_batch), "kitti120k", "cuda")
    vox = b["coords_int"]
    g = torch.Generator(device="cuda").manual_seed(0)
    pts = vox.repeat_interleave(per_voxel, dim=0).float()
    pts[:, 1:] += torch.rand(pts.shape[0], 3, device="cuda", generator=g)
    pts = pts[torch.randperm(pts.shape[0], device="cuda", generator=g)].contiguous()
    n = pts.shape[0]
    field = ME.TensorField(torch.randn(n, C_FEATURES, device="cuda", generator=g), pts)
    fm = field._field_map()
    m, inv = fm.m, fm.inverse
    inv64 = inv.long()
    cnt = torch.bincount(inv64, minlength=m).float().unsqueeze(1)
    x, xv = field.F, torch.randn(m, C_FEATURES, device="cuda", generator=g)
    rows = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    y_m, y_n = torch.empty(m, C_FEATURES, device="cuda"), torch.empty(n, C_FEATURES, device="cuda")
    row_ptr = torch.empty(m + 1, dtype=torch.int32, device="cuda")
    row_list = torch.empty(n, dtype=torch.int32, device="cuda")
    nbytes = _lib.load().lidog_field_lists_ws(n, m)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def hip_floor():
        call("lidog_field_floor", ptr(pts), n, 1, ptr(rows), ptr(err))
        return rows

    def torch_floor():
        f = torch.floor(pts / 1.0) * 1.0
        return torch.where((f >= -2147483648.0) & (f < 2147483648.0), f, torch.full_like(f, -2147483648.0)).int()

    def hip_lists():
        call("lidog_field_lists", ptr(inv), n, m, ptr(row_ptr), ptr(row_list), ptr(ws), nbytes)
        return row_list

    def torch_lists():
        order = torch.sort(inv64, stable=True)[1]
        torch.cumsum(torch.bincount(inv64, minlength=m), 0)
        return order.int()

    def hip_reduce():
        call("lidog_field_reduce", ptr(x), n, ptr(fm.row_ptr), ptr(fm.row_list), m, C_FEATURES, 1, ptr(y_m))
        return y_m

    def torch_reduce():
        return torch.zeros(m, C_FEATURES, device="cuda").index_add_(0, inv64, x) / cnt

    def hip_gather():
        call("lidog_field_gather", ptr(xv), ptr(inv), n, m, C_FEATURES, None, ptr(y_n))
        return y_n

    def torch_gather():
        return xv.index_select(0, inv64)

    for case, hip, ref, C, nrows in (("floor", hip_floor, torch_floor, 4, n), ("lists", hip_lists, torch_lists, 1, n),
                                     ("reduce_avg", hip_reduce, torch_reduce, C_FEATURES, m),
                                     ("gather", hip_gather, torch_gather, C_FEATURES, n)):
        diff = float((hip().clone().float() - ref().float()).abs().max())
        _record(case, C, nrows, _alternate({"hip": hip, "torch": ref}, rounds, reps), rounds, reps, diff)

    # interpolation of C_LOGITS logits on the stride-1 map at every point
    cm = fm.cm
    nbr = ME.interpolation_neighbours(cm, 1, pts)
    lists = ME._field_lists(nbr, m)
    logits = torch.randn(m, C_LOGITS, device="cuda", generator=g)
    gy = torch.randn(n, C_LOGITS, device="cuda", generator=g)
    y_q, g_f = torch.empty(n, C_LOGITS, device="cuda"), torch.empty(m, C_LOGITS, device="cuda")
    t = pts[:, 1:] - torch.floor(pts[:, 1:])
    w = [torch.where(torch.tensor([(k >> a) & 1 for a in range(3)], device="cuda").bool(), t, 1 - t).prod(1, keepdim=True)
         for k in range(8)]
    have = [(nbr[k] >= 0).unsqueeze(1) for k in range(8)]
    rows64 = [nbr[k].clamp(min=0).long() for k in range(8)]
    # the gradient's torch side adds the pairs that exist only (an absent neighbour clamped to row 0 would make every
    # such entry an atomic on one row)
    sel = [torch.nonzero(nbr[k] >= 0).flatten() for k in range(8)]
    rows_sel = [nbr[k][sel[k]].long() for k in range(8)]
    w_sel = [w[k][sel[k]] for k in range(8)]

    def hip_interp():
        call("lidog_interp_fwd", ptr(logits), m, C_LOGITS, ptr(pts), ptr(nbr), n, 1, ptr(y_q))
        return y_q

    def torch_interp():
        out = torch.zeros(n, C_LOGITS, device="cuda")
        for k in range(8):
            out += torch.where(have[k], w[k] * logits.index_select(0, rows64[k]), torch.zeros((), device="cuda"))
        return out

    def hip_interp_bwd():
        call("lidog_interp_bwd", ptr(gy), ptr(pts), n, ptr(lists[0]), ptr(lists[1]), m, C_LOGITS, 1, ptr(g_f))
        return g_f

    def torch_interp_bwd():
        out = torch.zeros(m, C_LOGITS, device="cuda")
        for k in range(8):
            out.index_add_(0, rows_sel[k], w_sel[k] * gy.index_select(0, sel[k]))
        return out

    def hip_interp_lists():
        return ME._field_lists(nbr, m)[1]

    for case, hip, ref, nrows in (("interp_fwd", hip_interp, torch_interp, n),
                                  ("interp_bwd", hip_interp_bwd, torch_interp_bwd, m)):
        diff = float((hip().clone() - ref()).abs().max())
        _record(case, C_LOGITS, nrows, _alternate({"hip": hip, "torch": ref}, rounds, reps), rounds, reps, diff)
    t_l = _alternate({"hip": hip_interp_lists}, rounds, max(reps // 5, 1))
    print(json.dumps({"bench": "field", "case": "interp_bwd_lists", "rows": int(8 * n),
                      "hip_us": round(1e3 * t_l["hip"], 2), "note": "built once per backward pass"}), flush=True)


def write_tree(root, n_scans, per_voxel, seed=0):
    """a SemanticKITTI tree (sequence 08) of synthetic scans: `per_voxel` records inside every voxel of a kitti120k
    scan, raw label = class + 1 (0: unlabelled); returns the look-up table of that map"""
    import numpy as np
    from lidog_amd import scans, synth
    rng = np.random.default_rng(seed)
    for d in ("velodyne", "labels"):
        os.makedirs(os.path.join(root, "sequences", "08", d), exist_ok=True)
    for f in range(n_scans):
        b = synth.make_batch([f], "kitti120k", "cuda")
        vox = np.repeat(b["coords_int"][:, 1:].cpu().numpy().astype(np.float64), per_voxel, axis=0)
        lab = np.repeat(b["source_sem_labels0"].cpu().numpy().astype(np.int64), per_voxel)
        order = rng.permutation(vox.shape[0])
        xyz = ((vox + rng.random(vox.shape)) * 0.05)[order]
        rec = np.concatenate([xyz, rng.random((xyz.shape[0], 1))], axis=1).astype(np.float32)
        rec.tofile(os.path.join(root, "sequences", "08", "velodyne", f"{f:06d}.bin"))
        (lab[order] + 1).astype(np.int32).tofile(os.path.join(root, "sequences", "08", "labels", f"{f:06d}.label"))
    return scans.label_lut({0: -1, **{c + 1: c for c in range(7)}})


def bench_evaluator(n_scans, per_voxel, batch, rounds, checkpoint):
    import torch
    from lidog_amd import evaluate, scans
    from lidog_amd.train import build_model
    torch.manual_seed(0)
    model = build_model("MinkUNet34")
    if checkpoint:
        from lidog_amd.checkpoint import load_lightning_checkpoint
        load_lightning_checkpoint(model, checkpoint)
    model.eval()
    with tempfile.TemporaryDirectory() as root:
        lut = write_tree(root, n_scans, per_voxel)
        ev = evaluate.TargetEvaluator(model)
        sec = {"nearest": [], "trilinear": []}
        res = {}
        for r in range(rounds + 1):                      # round 0: first use of every kernel, not timed
            for interp in sec:
                data = scans.FileScans(scans.listing("SemanticKITTI", root, "validation"), lut)
                points = evaluate.PointPath.of(data, "cuda", interp=interp)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[interp] = ev.run(evaluate.dataset_batches(data, batch, "cuda"), len(data), points=points)
                if r:
                    sec[interp].append(time.perf_counter() - t0)
    near, tri = res["nearest"], res["trilinear"]
    moved = int(abs(near["point_counts"] - tri["point_counts"]).sum() // 2)
    print(json.dumps({"bench": "field", "case": "target_evaluator", "scans": n_scans, "batch": batch,
                      "labelled_points": int(near["point_counts"].sum()), "trained": bool(checkpoint),
                      "nearest_s": round(statistics.median(sec["nearest"]), 4),
                      "trilinear_s": round(statistics.median(sec["trilinear"]), 4),
                      "voxel_miou": round(near["mean"], 3), "nearest_point_miou": round(near["point_mean"], 3),
                      "trilinear_point_miou": round(tri["point_mean"], 3),
                      "confusion_entries_moved": moved, "rounds": rounds}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kernel-batch", type=int, default=4)
    ap.add_argument("--points-per-voxel", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--eval-scans", type=int, default=8, help="0: skip the TargetEvaluator part")
    ap.add_argument("--eval-batch", type=int, default=4)
    ap.add_argument("--eval-rounds", type=int, default=3)
    ap.add_argument("--checkpoint", default=None, help="a MinkUNet34 checkpoint for the TargetEvaluator part")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_field: no GPU (nothing here can be measured without one)")
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    bench_kernels(a.kernel_batch, a.points_per_voxel, a.rounds, a.reps)
    if a.eval_scans:
        bench_evaluator(a.eval_scans, a.points_per_voxel, a.eval_batch, a.eval_rounds, a.checkpoint)


if __name__ == "__main__":
    main()
