"""The training augmentation (sub_p 0.8, RandomRotation + RandomScale) on the same box and the same synthetic scans:

  (a) one item (lidog_amd.data.augment_item) of each scan of a batch of --batch kitti120k and nusc35k scans, in the BEV
      datasets' form (bounds filter, BEV label image) and in the plain form: device time between HIP events recorded
      on the merge stream around the item (the upload of the drawn rows and the read-backs included, since the stream
      waits for them), the host wall time of the call and of the draws, median over --reps
  (b) MinkUNet34BEV training steps (batch --batch, kitti120k) on --augment batches (lidog_amd.train.AugmentedSynthScans)
      against plain batches, alternating round by round as Fit.run drives them (the next batch is built before this
      step is queued); each round times --steps steps with the host clock after one synchronisation, behind --warmup
      untimed steps.  Both datasets read scans from an in-process cache, so neither pays for the synthetic scan
      generator.

One JSON line per measurement.

    python scripts/bench_augment.py --batch 4 --reps 20 --steps 10 --warmup 3 --rounds 3
"""
import argparse
import functools
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AUGS = ["RandomRotation", "RandomScale"]


def bench_item(config, form, batch, reps, sub_p=0.8):
    import numpy as np
    import torch
    from lidog_amd import data, synth
    from lidog_amd.train import bev_image_size
    dev = torch.device("cuda")
    side = data.merge_stream(dev)
    bev = (50.0, bev_image_size(50.0)) if form == "bev" else None
    voxel = synth.CONFIGS[config]["voxel"]
    with torch.cuda.stream(side):
        scans = []
        for j in range(batch):
            pts, labels = synth.scan_points_labels(j, config)
            scans.append({"points": torch.from_numpy(pts).to(dev), "sem_labels": torch.from_numpy(labels).to(dev),
                          "features": torch.ones((pts.shape[0], 1), dtype=torch.float32, device=dev)})
    dev_ms, host_ms, draw_ms, rows = [], [], [], []
    for r in range(reps + 2):
        for i, scan in enumerate(scans):
            t0 = time.perf_counter()
            draws = data.draw_augmentation(np.random.RandomState([r, i]), scan["points"].shape[0], sub_p, AUGS)
            t1 = time.perf_counter()
            with torch.cuda.stream(side):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(side)
                out = data.augment_item(scan, draws, voxel, bounds=bev is not None, bev=bev)
                b.record(side)
                t2 = time.perf_counter()
                b.synchronize()
            if r >= 2:                                   # two untimed passes: first use of every kernel and buffer
                dev_ms.append(a.elapsed_time(b))
                host_ms.append((t2 - t1) * 1e3)
                draw_ms.append((t1 - t0) * 1e3)
                rows.append(int(out["coordinates"].shape[0]))
    return {"bench": "augment_item", "config": config, "form": form, "batch": batch, "items": len(dev_ms),
            "points": int(scans[0]["points"].shape[0]), "device_ms_median": statistics.median(dev_ms),
            "device_ms_min": min(dev_ms), "host_ms_median": statistics.median(host_ms),
            "draws_host_ms_median": statistics.median(draw_ms), "voxels_median": statistics.median(rows),
            "device_ms_per_batch": statistics.median(dev_ms) * batch}


def _steps(step, data, batches, epoch=0):
    cur = data.batch(batches[0], "cuda")
    for i in range(len(batches)):
        nxt = data.batch(batches[i + 1], "cuda") if i + 1 < len(batches) else None
        step.training_step(cur, epoch=epoch, prefetch=nxt)
        cur = nxt


def bench_steps(batch, steps, warmup, rounds):
    import torch
    from lidog_amd import synth
    from lidog_amd.train import AugmentedSynthScans, SynthScans, bev_image_size, build_model, build_step
    synth.scan_voxels = functools.lru_cache(maxsize=None)(synth.scan_voxels)
    n = batch * 2
    size = bev_image_size(50.0)
    sets = {"plain": SynthScans(n, "kitti120k", bev_size=size),
            "augment": AugmentedSynthScans(n, "kitti120k", AUGS, sub_p=0.8, seed=1, bev=(50.0, size))}
    torch.manual_seed(0)
    model = build_model("MinkUNet34BEV")
    model, step, _ = build_step(model, "MinkUNet34BEV", lr=1e-3)
    order = [[(k * batch + j) % n for j in range(batch)] for k in range(steps)]
    for name, d in sets.items():                       # every scan in the cache, every kernel used once
        for k in range(2):
            d.batch([(k * batch + j) % n for j in range(batch)], "cpu" if name == "plain" else "cuda")
        _steps(step, d, order[:warmup])
    times = {k: [] for k in sets}
    for r in range(rounds):
        for name, d in sets.items():
            if hasattr(d, "set_epoch"):
                d.set_epoch(r)
            _steps(step, d, order[:warmup])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _steps(step, d, order)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / steps)
    res = {"bench": "augment_step", "model": "MinkUNet34BEV", "config": "kitti120k", "batch": batch, "steps": steps,
           "rounds": rounds}
    for name, t in times.items():
        res[f"{name}_ms_per_step_median"] = statistics.median(t)
        res[f"{name}_ms_per_step"] = t
    res["augment_over_plain"] = res["augment_ms_per_step_median"] / res["plain_ms_per_step_median"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    for config in ("kitti120k", "nusc35k"):
        for form in ("bev", "plain"):
            print(json.dumps(bench_item(config, form, a.batch, a.reps)), flush=True)
    if not a.skip_steps:
        print(json.dumps(bench_steps(a.batch, a.steps, a.warmup, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
