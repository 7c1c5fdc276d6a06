"""Evaluation throughput on the same box, the same model and the same batches:

  (a) scans/s of `evaluate.evaluate` (per batch one `.item()`, per scan a boolean selection and two [C, N] boolean
      matrices in torch) against `evaluate.TargetEvaluator` (lidog_eval_confusion into one preallocated tensor, one read
      per target), MinkUNet34BEV forward-only, kitti120k and nusc35k at --batch, alternating round by round; each round
      times one pass over --batches batches made ahead on the device, with the host clock, from a synchronised device to
      the result on the host; one untimed pass of each path first.  Every round's reading is printed.
  (b) device time of lidog_eval_confusion alone on one batch, between HIP events, median over --reps.

One JSON line per measurement.

    python scripts/bench_eval.py --batch 8 --batches 4 --rounds 5 --reps 30
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench_paths(model, config, batch, n_batches, rounds):
    import torch
    from lidog_amd import evaluate
    from lidog_amd.train import SynthScans
    n = batch * n_batches
    batches = list(evaluate.dataset_batches(SynthScans(n, config, first=10 ** 6), batch))
    ev = evaluate.TargetEvaluator(model)

    def old():
        per_class, mean = evaluate.evaluate(model, [b for b, _ in batches])
        return [float(x) for x in per_class.tolist()], float(mean)

    def new():
        res = ev.run(batches, n, rows="scan")
        return [float(x) for x in res["per_class"]], res["mean"]

    paths = {"evaluate": old, "target_evaluator": new}
    out = {k: f() for k, f in paths.items()}                      # untimed: first use of every kernel and buffer
    same = max(abs(a - b) for a, b in zip(out["evaluate"][0], out["target_evaluator"][0])) <= 1e-9
    rates = {k: [] for k in paths}
    for _ in range(rounds):
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            rates[k].append(n / (time.perf_counter() - t0))
    res = {"bench": "eval_paths", "model": "MinkUNet34BEV", "config": config, "batch": batch, "scans": n,
           "rounds": rounds, "voxels_per_batch": int(batches[0][0]["coords_int"].shape[0]), "same_table": same}
    for k, r in rates.items():
        res[f"{k}_scans_per_s_median"] = statistics.median(r)
        res[f"{k}_scans_per_s"] = [round(x, 2) for x in r]
    res["new_over_old"] = res["target_evaluator_scans_per_s_median"] / res["evaluate_scans_per_s_median"]
    return res


def bench_kernel(config, batch, reps):
    import torch
    from lidog_amd import evaluate, synth
    b = synth.make_batch([10 ** 6 + i for i in range(batch)], config, "cuda")
    coords, labels = b["coords_int"], b["source_sem_labels0"]
    logits = torch.randn((coords.shape[0], 7), device="cuda")
    counts = torch.zeros((batch, 8, 7), dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    ms = []
    for r in range(reps + 3):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        evaluate.confusion(logits, labels, coords, batch, out=counts, err=err)
        e.record()
        e.synchronize()
        if r >= 3:
            ms.append(a.elapsed_time(e))
    evaluate.check_scan_error(err)
    return {"bench": "lidog_eval_confusion", "config": config, "batch": batch, "rows": int(coords.shape[0]),
            "reps": reps, "device_us_median": statistics.median(ms) * 1e3, "device_us_min": min(ms) * 1e3,
            "note": "HIP events around the call: the preds allocation and the launch included"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    from lidog_amd.train import build_model
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    model = build_model("MinkUNet34BEV").eval()
    for config in ("kitti120k", "nusc35k"):
        print(json.dumps(bench_paths(model, config, a.batch, a.batches, a.rounds)), flush=True)
    for config in ("kitti120k", "nusc35k"):
        print(json.dumps(bench_kernel(config, a.batch, a.reps)), flush=True)


if __name__ == "__main__":
    main()
