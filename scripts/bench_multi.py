"""Two-source LiDOG step (configs/lidog/multi) against its one-source parts on the same box: the kitti120k step and the
nusc35k step (MinkUNet34BEV, batch --batch each), the two-source step on both (--batch + --batch), and the same two-source
step with the trunk executor's accumulate mode off (the second backward pass hands fresh gradients to autograd, which
adds them).  The variants alternate round by round; each round times --steps steps with the host clock after one
synchronisation, behind --warmup untimed steps.  One JSON line per variant: median / min step time over the rounds.

    python scripts/bench_multi.py --steps 10 --warmup 3 --rounds 3
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
    ap.add_argument("--variants", default="kitti120k,nusc35k,multi,multi_autograd")
    a = ap.parse_args()
    import torch
    import lidog_amd  # noqa: F401
    from lidog_amd import synth, trunk
    from lidog_amd.train import build_model, build_step
    torch.manual_seed(0)
    seeds = list(range(a.batch))
    batches = {"kitti120k": synth.make_batch(seeds, "kitti120k", device="cuda"),
               "nusc35k": synth.make_batch(seeds, "nusc35k", device="cuda"),
               "multi": synth.make_batch(seeds, "kitti120k", device="cuda", seeds1=seeds, config1="nusc35k")}
    batches["multi_autograd"] = batches["multi"]
    names = a.variants.split(",")
    steps = {}

    def run(name, n):
        prev = trunk.set_accumulate(name != "multi_autograd")
        try:
            for _ in range(n):
                out = steps[name].training_step(batches[name])
        finally:
            trunk.set_accumulate(prev)
        return out

    for name in names:
        model = build_model("MinkUNet34BEV", device="cuda")
        _, steps[name], _ = build_step(model, "MinkUNet34BEV", num_sources=2 if name.startswith("multi") else 1)
        run(name, a.warmup)
    times = {k: [] for k in names}
    losses = {}
    for _ in range(a.rounds):
        for name in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run(name, a.steps)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
            losses[name] = float(out["loss"])
    for name in names:
        b = batches[name]
        rows = int(b["coords_int"].shape[0]) + (int(b["coords_int1"].shape[0]) if "coords_int1" in b else 0)
        print(json.dumps({"variant": name, "batch": a.batch, "rows": rows, "steps": a.steps, "rounds": a.rounds,
                          "paths": list(steps[name].last_paths),
                          "step_ms_median": round(statistics.median(times[name]), 3),
                          "step_ms_min": round(min(times[name]), 3), "step_ms_rounds": [round(t, 3) for t in times[name]],
                          "loss": losses[name]}), flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    if {"kitti120k", "nusc35k", "multi"} <= set(med):
        print(json.dumps({"ratio": "multi/(kitti120k+nusc35k)",
                          "step_time_ratio": round(med["multi"] / (med["kitti120k"] + med["nusc35k"]), 3)}), flush=True)
    if {"multi", "multi_autograd"} <= set(med):
        print(json.dumps({"ratio": "multi/multi_autograd", "step_time_ratio": round(med["multi"] / med["multi_autograd"], 3)}),
              flush=True)


if __name__ == "__main__":
    main()
