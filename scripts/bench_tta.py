"""Test-time augmentation (csrc/tta.hip, lidog_amd/tta.py) measured, on the same box, alternating:

  vote      lidog_tta_vote per mode (an accumulating view, first = 0)  vs  the torch composition of the same result:
            index_select -> softmax (prob) / nothing (logit) / argmax + one_hot (vote) -> add_
            at the size of --kernel-batch kitti120k scans with --points-per-voxel points in every voxel; device time
            (HIP events around --reps launches, median over --rounds, both sides taking turns)
  evaluator TargetEvaluator over --eval-scans scan files (a temporary SemanticKITTI tree of synthetic scans, as
            scripts/bench_field.py writes it) with 1, 4 and 8 views, alternating: scans per second
  miou      the point-level mIoU of one short training run's weights (--train-epochs epochs of MinkUNet34 on synthetic
            kitti120k scans, or --checkpoint) with and without `rot4`; a briefly trained model may gain nothing

One JSON line per case.

    python scripts/bench_tta.py --rounds 7 --reps 50
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_field import _alternate, write_tree  # noqa: E402

C_LOGITS = 7
VIEWS = {1: None, 4: ["rot4"], 8: ["rot4", "flipx", "flipy", "flipx+rotz90", "flipy+rotz90"]}


def bench_vote(kernel_batch, per_voxel, rounds, reps):
    import torch
    from lidog_amd import synth, tta
    m = synth.make_batch(range(kernel_batch), "kitti120k", "cuda")["coords_int"].shape[0]
    g = torch.Generator(device="cuda").manual_seed(0)
    k = m * per_voxel
    inverse = torch.arange(m, device="cuda").repeat_interleave(per_voxel)[torch.randperm(k, device="cuda", generator=g)]
    inverse = inverse.contiguous()
    logits = 4 * torch.randn(m, C_LOGITS, device="cuda", generator=g)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    for mode in tta.MODES:
        acc_h = torch.zeros(k, C_LOGITS, device="cuda")
        acc_t = torch.zeros(k, C_LOGITS, device="cuda")

        def hip():
            return tta.vote(logits, inverse, acc_h, mode, first=False, err=err)

        def composition():
            s = logits.index_select(0, inverse)
            if mode == "prob":
                s = torch.softmax(s, dim=1)
            elif mode == "vote":
                s = torch.nn.functional.one_hot(s.argmax(dim=1), C_LOGITS).float()
            return acc_t.add_(s)

        hip()
        composition()
        diff = float((acc_h - acc_t).abs().max())
        t = _alternate({"hip": hip, "torch": composition}, rounds, reps)
        # the kernel's own traffic: the index, the gathered rows, acc read and written
        nbytes = k * (8 + 3 * 4 * C_LOGITS)
        print(json.dumps({"bench": "tta", "case": f"vote_{mode}", "C": C_LOGITS, "points": int(k), "voxels": int(m),
                          "hip_us": round(1e3 * t["hip"], 2), "torch_us": round(1e3 * t["torch"], 2),
                          "torch_over_hip": round(t["torch"] / t["hip"], 2),
                          "hip_gb_per_s": round(nbytes / (1e6 * t["hip"]), 1), "max_abs_diff_one_view": diff,
                          "error_word": int(err.item()), "rounds": rounds, "reps": reps}), flush=True)


def _evaluate(model, root, lut, batch, views, mode="prob"):
    import torch
    from lidog_amd import evaluate, scans
    data = scans.FileScans(scans.listing("SemanticKITTI", root, "validation"), lut)
    points = evaluate.PointPath.of(data, "cuda", tta=views, tta_mode=mode)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = evaluate.TargetEvaluator(model).run(evaluate.dataset_batches(data, batch, "cuda"), len(data), points=points)
    return res, time.perf_counter() - t0


def bench_evaluator(model, root, lut, n_scans, batch, rounds):
    sec = {n: [] for n in VIEWS}
    res = {}
    for r in range(rounds + 1):                          # round 0: first use of every kernel, not timed
        for n, views in VIEWS.items():
            res[n], dt = _evaluate(model, root, lut, batch, views)
            if r:
                sec[n].append(dt)
    med = {n: statistics.median(v) for n, v in sec.items()}
    print(json.dumps({"bench": "tta", "case": "target_evaluator", "scans": n_scans, "batch": batch,
                      "labelled_points": int(res[1]["point_counts"].sum()),
                      **{f"views{n}_scans_per_s": round(n_scans / med[n], 2) for n in VIEWS},
                      **{f"views{n}_s": round(med[n], 4) for n in VIEWS},
                      "views4_over_views1": round(med[4] / med[1], 2), "views8_over_views1": round(med[8] / med[1], 2),
                      "rounds": rounds}), flush=True)


def short_run(epochs, scans_per_epoch, save_dir):
    """the last checkpoint of a short MinkUNet34 run on synthetic kitti120k scans"""
    from lidog_amd import train
    fit = train._fit_from_args(train.parse_args(
        ["--model", "MinkUNet34", "--config", "kitti120k", "--epochs", str(epochs), "--scans", str(scans_per_epoch),
         "--batch", "4", "--save-dir", save_dir]))
    return fit.run()[-1]["checkpoint"]


def bench_miou(model, root, lut, n_scans, batch, trained):
    from lidog_amd import tta
    plain, _ = _evaluate(model, root, lut, batch, None)
    out = {"bench": "tta", "case": "point_miou", "scans": n_scans, "weights": trained,
           "voxel_miou": round(plain["mean"], 3), "plain_point_miou": round(plain["point_mean"], 3)}
    for mode in tta.MODES:
        voted, _ = _evaluate(model, root, lut, batch, ["rot4"], mode)
        out[f"rot4_{mode}_point_miou"] = round(voted["point_mean"], 3)
        out[f"rot4_{mode}_confusion_entries_moved"] = int(abs(plain["point_counts"] - voted["point_counts"]).sum() // 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kernel-batch", type=int, default=8, help="scans of the vote kernel's batch (eval_target's batch)")
    ap.add_argument("--points-per-voxel", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--eval-scans", type=int, default=8, help="0: skip the TargetEvaluator and mIoU parts")
    ap.add_argument("--eval-batch", type=int, default=4)
    ap.add_argument("--eval-rounds", type=int, default=3)
    ap.add_argument("--train-epochs", type=int, default=3, help="epochs of the short run (0: fresh weights)")
    ap.add_argument("--train-scans", type=int, default=32)
    ap.add_argument("--checkpoint", default=None, help="a MinkUNet34 checkpoint instead of the short run")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta: no GPU (nothing here can be measured without one)")
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    bench_vote(a.kernel_batch, a.points_per_voxel, a.rounds, a.reps)
    if not a.eval_scans:
        return
    from lidog_amd.checkpoint import load_lightning_checkpoint
    from lidog_amd.train import build_model
    with tempfile.TemporaryDirectory() as root:
        lut = write_tree(os.path.join(root, "tree"), a.eval_scans, a.points_per_voxel)
        ckpt, trained = a.checkpoint, "checkpoint" if a.checkpoint else "fresh"
        if ckpt is None and a.train_epochs > 0:
            ckpt, trained = short_run(a.train_epochs, a.train_scans, os.path.join(root, "run")), \
                f"{a.train_epochs} epochs of {a.train_scans} scans"
        torch.manual_seed(0)
        model = build_model("MinkUNet34")
        if ckpt:
            load_lightning_checkpoint(model, ckpt)
        model.eval()
        bench_evaluator(model, os.path.join(root, "tree"), lut, a.eval_scans, a.eval_batch, a.eval_rounds)
        bench_miou(model, os.path.join(root, "tree"), lut, a.eval_scans, a.eval_batch, trained)


if __name__ == "__main__":
    main()
