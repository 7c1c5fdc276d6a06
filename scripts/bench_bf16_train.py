"""bf16 training (lidog_amd/precision.py:Bf16Training, csrc/sconv_bf16.hip:k_sconv_wgrad_bf16) against the fp32 path, on
the same box, the sides alternating round by round, medians over --rounds:

  (a) wgrad: device time (HIP events around --reps launches) of lidog_sconv_wgrad vs lidog_sconv_wgrad_bf16 on the kernel
      maps of the bench batch (kitti120k, --kernel-batch scans) at the layer shapes of MinkUNet34, random operands, each
      kernel with the work items me._wgrad_chunk cuts for it
  (b) step: the MinkUNet34BEV training step at --batch (the bench's model, optimiser, batches and prefetch), timed three
      ways on ONE model: (i) fp32 with the trunk executor, (ii) fp32 on the operator path (executor off), (iii) bf16
      (operator path).  Every round runs --steps steps of each between two device synchronisations, after one untimed
      step of that variant.
  (c) quality: one short run both ways (MinkUNet34, source8k, the same seed): loss per epoch and the validation mIoU of
      the weights each run ends with (evaluated in fp32)

One JSON line per measurement.

    python scripts/bench_bf16_train.py --rounds 5 --reps 10 --steps 10
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_bf16 import K2, K3, _alternate  # noqa: E402  (the layer table of DESIGN.md section 3r)


def bench_wgrad(kernel_batch, rounds, reps):
    import numpy as np
    import torch
    import lidog_amd.me as ME
    from lidog_amd import _lib, synth
    from lidog_amd._lib import call, ptr
    L = _lib.load()
    b = synth.make_batch(range(kernel_batch), "kitti120k", "cuda")
    cm = ME.SparseTensor(coordinates=b["coords_int"], features=b["source_features0"]).coordinate_manager
    prev = 1
    for s in (2, 4, 8, 16):
        cm.stride(prev, s)
        prev = s
    for kind, cases in (("k3s1", K3), ("k2s2", K2)):
        for s, Cin, Cout in cases:
            m = cm.kernel_map(s, s if kind == "k3s1" else 2 * s, 3 if kind == "k3s1" else 2)
            x = torch.randn(m.n_in, Cin, device="cuda")
            gy = torch.randn(m.n_out, Cout, device="cuda")
            gW = torch.empty(m.K, Cin, Cout, device="cuda")
            fns, info = {}, {}
            for name, bf in (("wgrad_fp32", False), ("wgrad_bf16", True)):
                chunk = ME._wgrad_chunk(m.k_off_host, Cin, Cout, bf)
                items, n_items, item_off = ME._wgrad_items_host(m.k_off_host, chunk)
                items = torch.from_numpy(np.ascontiguousarray(items)).cuda()
                item_off = torch.from_numpy(item_off).cuda()
                slabs = (L.lidog_sconv_wgrad_bf16_slabs if bf else L.lidog_sconv_wgrad_slabs)(Cin, Cout, n_items)
                partial = torch.empty(max(slabs, 1), Cin, Cout, device="cuda")
                entry = "lidog_sconv_wgrad_bf16" if bf else "lidog_sconv_wgrad"
                fns[name] = (lambda entry=entry, items=items, n_items=n_items, item_off=item_off, partial=partial:
                             call(entry, ptr(x), ptr(m.pair_in), ptr(gy), ptr(m.pair_out), ptr(items), n_items,
                                  ptr(item_off), m.K, Cin, Cout, ptr(partial), ptr(gW)))
                info[name] = {"chunk": int(chunk), "items": int(n_items), "slabs": int(slabs)}
            t = _alternate(fns, rounds, reps)
            rec = {"bench": "bf16_wgrad", "map": kind, "stride": s, "Cin": Cin, "Cout": Cout, "pairs": int(m.P),
                   "gflop": 2e-9 * m.P * Cin * Cout, "rounds": rounds, "reps": reps, "layout": info,
                   "slots_fp32": int(L.lidog_sconv_wgrad_slots(Cin, Cout, 0)),
                   "slots_bf16": int(L.lidog_sconv_wgrad_bf16_slots(Cin, Cout))}
            for k, v in t.items():
                rec[k + "_ms"] = round(v, 4)
            rec["fp32_over_bf16"] = round(t["wgrad_fp32"] / t["wgrad_bf16"], 3)
            rec["bf16_tflops"] = round(rec["gflop"] / t["wgrad_bf16"], 1)
            # least traffic: both gathered rows of every pair in (from L2 or HBM); the slots are small next to that
            rec["bf16_least_gb_per_s"] = round(4.0 * m.P * (Cin + Cout) / t["wgrad_bf16"] / 1e6, 0)
            print(json.dumps(rec), flush=True)


def bench_step(config, batch, rounds, steps):
    import torch
    from lidog_amd import synth, trunk
    from lidog_amd.train import build_model, build_step
    from lidog_amd.trainer import LiDOGStep
    torch.manual_seed(1234)
    model, step, _ = build_step(build_model("MinkUNet34BEV", bound_2d=50.0), "MinkUNet34BEV", optimizer="Adam", lr=1e-3,
                                weight_decay=1e-4, source_weights=(0.5, 0.5))
    bstep = LiDOGStep(model, step.opt, source_weights=(0.5, 0.5), precision="bf16")
    batches = [synth.make_batch(range(i * batch, (i + 1) * batch), config, "cuda") for i in range(2)]
    ready = torch.cuda.Event()
    ready.record()
    torch.cuda.synchronize()
    variants = {"fp32_executor": (step, True), "fp32_operators": (step, False), "bf16_operators": (bstep, False)}
    was = trunk.ENABLED
    count = [0]

    def run(st, n):
        for _ in range(n):
            i = count[0]
            count[0] += 1
            out = st.training_step(batches[i % 2], prefetch=batches[(i + 1) % 2], prefetch_ready=ready)
        return out

    ms, paths, losses = {k: [] for k in variants}, {}, {}
    try:
        for r in range(rounds + 1):                 # round 0 is untimed: first use of every path
            for name, (st, executor) in variants.items():
                trunk.set_enabled(executor and was)
                run(st, 1)                          # untimed: this variant's maps, work items and tables
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = run(st, steps)
                torch.cuda.synchronize()
                if r:
                    ms[name].append((time.perf_counter() - t0) / steps * 1e3)
                paths[name], losses[name] = st.last_path, float(out["loss"])
    finally:
        trunk.set_enabled(was)
    rec = {"bench": "bf16_step", "model": "MinkUNet34BEV", "config": config, "batch": batch, "rounds": rounds,
           "steps_per_round": steps, "voxels_per_batch": int(batches[0]["coords_int"].shape[0]), "paths": paths,
           "last_loss": losses, "packs": bstep.bf16.packs, "routes": dict(bstep.precision_ctx.launches)}
    for k, v in ms.items():
        rec[k + "_ms_median"] = round(statistics.median(v), 3)
        rec[k + "_ms"] = [round(x, 3) for x in v]
        rec[k + "_scans_per_s"] = round(batch / statistics.median(v) * 1e3, 2)
    rec["bf16_over_fp32_executor"] = round(rec["fp32_executor_ms_median"] / rec["bf16_operators_ms_median"], 3)
    rec["bf16_over_fp32_operators"] = round(rec["fp32_operators_ms_median"] / rec["bf16_operators_ms_median"], 3)
    return rec


def bench_quality(epochs, scans, val_scans):
    from lidog_amd import evaluate
    from lidog_amd.train import Fit, SynthScans
    rec = {"bench": "bf16_train_quality", "model": "MinkUNet34", "config": "source8k", "epochs": epochs,
           "train_scans": scans, "val_scans": val_scans, "seed": 1234}
    data = SynthScans(val_scans, "source8k", first=10 ** 6)
    for p in ("fp32", "bf16"):
        fit = Fit(model_kind="MinkUNet34", batch_size=4, optimizer="Adam", lr=1e-3, epochs=epochs, seed=1234,
                  train_data=SynthScans(scans, "source8k"), num_sanity_val_steps=0, log=lambda *_: None, precision=p)
        hist = fit.run()
        res = evaluate.TargetEvaluator(fit.model.eval()).run(evaluate.dataset_batches(data, 8), val_scans, rows="scan")
        rec[f"{p}_loss_per_epoch"] = [round(float(h["loss"]), 5) for h in hist]
        rec[f"{p}_loss_per_step"] = [round(float(l), 5) for h in hist for l in h["losses"]]
        rec[f"{p}_val_mean_iou"] = res["mean"]
        rec[f"{p}_val_per_class_iou"] = [round(float(v), 4) for v in res["per_class"]]
        rec[f"{p}_path"] = fit.step.last_path
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parts", nargs="+", default=["wgrad", "step", "quality"], choices=["wgrad", "step", "quality"])
    ap.add_argument("--kernel-batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--config", default="kitti120k")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--train-scans", type=int, default=16)
    ap.add_argument("--val-scans", type=int, default=16)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bf16_train: no GPU (nothing here can be measured without one)")
    if a.rounds < 5:
        raise SystemExit("bench_bf16_train: medians need at least 5 rounds")
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    if "wgrad" in a.parts:
        bench_wgrad(a.kernel_batch, a.rounds, a.reps)
    if "step" in a.parts:
        print(json.dumps(bench_step(a.config, a.batch, a.rounds, a.steps)), flush=True)
    if "quality" in a.parts:
        print(json.dumps(bench_quality(a.epochs, a.train_scans, a.val_scans)), flush=True)


if __name__ == "__main__":
    main()
