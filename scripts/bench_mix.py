"""PointCutMix / CoSMix scan mixing on the same box and the same kitti120k scans (synth "kitti120k", 0.05 m):

  (a) one merge (lidog_amd.data.pointcutmix_merge / cosmix_merge, sub_p 0.8) of each pair of a batch of --batch
      kitti120k pairs: device time between HIP events recorded on the merge stream around the merge (its host draws
      and read-backs included, since the stream waits for them), and the host wall time of the call, median over --reps;
      the CoSMix merge also with its in-merge augmentation (augmentations = RandomRotation, RandomScale: every pasted
      class transformed, voxel rows written by the gather itself) on the same scans, next to the plain merge
  (b) MinkUNet34 training steps (SoftDICE, Adam, batch --batch) on --mix cosmix batches (lidog_amd.train.MixedSynthScans)
      and on --mix cosmix --source-augment RandomRotation RandomScale batches (augmented items, then the augmented merge)
      against plain one-source batches, alternating round by round as Fit.run drives them (the next batch is built
      before this step is queued); each round times --steps steps with the host clock after one synchronisation,
      behind --warmup untimed steps.  Both datasets read scans from an in-process cache, so neither pays for the
      synthetic scan generator.

One JSON line per measurement.

    python scripts/bench_mix.py --batch 4 --reps 20 --steps 10 --warmup 3 --rounds 3
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


def bench_merge(method, batch, reps, augmentations=None):
    import numpy as np
    import torch
    from lidog_amd import data
    from lidog_amd.train import MixedSynthScans
    ds = MixedSynthScans(batch, batch, ("kitti120k", "kitti120k"), method=method, seed=1)
    merge = ds.merge if augmentations is None else functools.partial(ds.merge, augmentations=augmentations)
    dev = torch.device("cuda")
    side = data.merge_stream(dev)
    with torch.cuda.stream(side):
        pairs = [(ds._scan(0, j, dev), ds._scan(1, int(ds.pairs.perm1[j]), dev)) for j in range(batch)]
    dev_ms, host_ms, rows = [], [], []
    for r in range(reps + 2):
        for i, (s0, s1) in enumerate(pairs):
            with torch.cuda.stream(side):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record(side)
                out = merge(s0, s1, rng=np.random.RandomState([r, i]))
                b.record(side)
                t1 = time.perf_counter()
                b.synchronize()
            if r >= 2:                                   # two untimed passes: first use of every kernel and buffer
                dev_ms.append(a.elapsed_time(b))
                host_ms.append((t1 - t0) * 1e3)
                rows.append(int(out["coordinates"].shape[0]))
    return {"bench": "mix_merge", "method": method, "augmentations": augmentations, "config": "kitti120k", "batch": batch,
            "merges": len(dev_ms),
            "device_ms_median": statistics.median(dev_ms), "device_ms_min": min(dev_ms),
            "host_ms_median": statistics.median(host_ms), "merged_rows_median": statistics.median(rows),
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
    from lidog_amd.train import AugmentedSynthScans, MixedSynthScans, SynthScans, build_model, build_step
    synth.scan_voxels = functools.lru_cache(maxsize=None)(synth.scan_voxels)
    n = batch * 2
    pair = ("kitti120k", "kitti120k")
    sets = {"plain": SynthScans(n, "kitti120k"),
            "cosmix": MixedSynthScans(n, n, pair, method="cosmix", seed=1),
            # its items keep their scans' points on the host (AugmentedSynthScans.points), as the others their voxels
            "cosmix_aug": MixedSynthScans(n, n, pair, method="cosmix", seed=1,
                                          items=AugmentedSynthScans(n, pair, AUGS, sub_p=0.8, seed=1))}
    torch.manual_seed(0)
    model = build_model("MinkUNet34")
    model, step, _ = build_step(model, "MinkUNet34", lr=1e-3)
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
    res = {"bench": "mix_step", "model": "MinkUNet34", "config": "kitti120k", "batch": batch, "steps": steps,
           "rounds": rounds}
    for name, t in times.items():
        res[f"{name}_ms_per_step_median"] = statistics.median(t)
        res[f"{name}_ms_per_step"] = t
    res["cosmix_over_plain"] = res["cosmix_ms_per_step_median"] / res["plain_ms_per_step_median"]
    res["cosmix_aug_over_cosmix"] = res["cosmix_aug_ms_per_step_median"] / res["cosmix_ms_per_step_median"]
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
    for method in ("pointcutmix", "cosmix"):
        print(json.dumps(bench_merge(method, a.batch, a.reps)), flush=True)
    print(json.dumps(bench_merge("cosmix", a.batch, a.reps, AUGS)), flush=True)
    if not a.skip_steps:
        print(json.dumps(bench_steps(a.batch, a.steps, a.warmup, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
