"""MinkUNet34 vs MinkUNet34IBN training steps on the same box and the same kitti120k scans (synth "kitti120k", 0.05 m),
configs/ibn settings: SoftDICE, Adam (lr 0.01), batch 4.  The two models alternate round by round; each round times
--steps steps with the host clock after one synchronisation, behind --warmup untimed steps.  One JSON line per model:
median / min step time over the rounds.

    python scripts/bench_ibn.py --steps 10 --warmup 3 --rounds 3
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--models", default="MinkUNet34,MinkUNet34IBN")
    a = ap.parse_args()
    import torch
    import lidog_amd  # noqa: F401
    from lidog_amd import synth
    from lidog_amd.train import build_model, build_step
    torch.manual_seed(0)
    batch = synth.make_batch(list(range(a.batch)), "kitti120k", device="cuda")
    kinds = a.models.split(",")
    steps = {}
    for k in kinds:
        model = build_model(k, device="cuda")
        _, step, _ = build_step(model, k, optimizer="Adam", lr=1e-2)
        for _ in range(a.warmup):
            step.training_step(batch)
        steps[k] = step
    times = {k: [] for k in kinds}
    for _ in range(a.rounds):
        for k in kinds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                out = steps[k].training_step(batch)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    rows = int(batch["coords_int"].shape[0])
    for k in kinds:
        print(json.dumps({"model": k, "batch": a.batch, "scans": "kitti120k", "rows": rows, "steps": a.steps,
                          "rounds": a.rounds, "step_ms_median": round(statistics.median(times[k]), 3),
                          "step_ms_min": round(min(times[k]), 3), "step_ms_rounds": [round(t, 3) for t in times[k]],
                          "loss": float(out["loss"]) if k == kinds[-1] else None}), flush=True)
    if len(kinds) == 2:
        r = statistics.median(times[kinds[1]]) / statistics.median(times[kinds[0]])
        print(json.dumps({"ratio": f"{kinds[1]}/{kinds[0]}", "step_time_ratio": round(r, 3)}), flush=True)


if __name__ == "__main__":
    main()
