"""The Raycast resampler (lidog_amd.raycast, csrc/raycast.hip) on the same box and the same synthetic scans:

  (a) kitti120k scans resampled to the nusc35k sensor (origin_between, snapped): the HIP path against a torch
      composition of the same result (packed int64 keys, scatter_reduce_('amin'), nonzero), alternating call by call.
      Per scan: device time between HIP events around the whole call, the one read-back of either side included (m for
      the HIP path, nonzero's size for torch), the host wall time of the call, and for the HIP path the device time of the
      launches alone (lidog_raycast without the read-back); median over --reps behind two untimed passes.  The two
      results are compared before anything is timed.
  (b) MinkUNet34 training steps (batch --batch, kitti120k) with --raycast-to nusc35k
      (lidog_amd.train.AugmentedSynthScans(augmentations=None, raycast=...)) against plain batches, alternating round by
      round as Fit.run drives them (the next batch is built before this step is queued); each round times --steps steps
      with the host clock after one synchronisation, behind --warmup untimed steps.  A resampled batch is smaller than a
      plain one (the target sensor has fewer cells than the source has points), so the two step times are two
      workloads, not one workload with and without an overhead; the batch sizes are printed with them.

One JSON line per measurement.

    python scripts/bench_raycast.py --batch 4 --reps 20 --steps 10 --warmup 3 --rounds 3
"""
import argparse
import functools
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SOURCE, TARGET = "kitti120k", "nusc35k"


def torch_raycast(points, spec, origin, tables):
    """the definition of lidog_raycast composed of torch operators (snap=True) -> (points_out, rows)"""
    import math
    import torch
    edges, cos_el, sin_el, cos_az, sin_az = tables
    n, n_az, n_cells = points.shape[0], spec.n_az, spec.n_cells
    q = points - origin
    qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
    r2 = (qx * qx + qy * qy) + qz * qz
    d = q.double()
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    az = torch.atan2(dy, dx)
    el = torch.atan2(dz, torch.sqrt(dx * dx + dy * dy))
    c = torch.remainder(torch.floor((az - spec.az0) / (2 * math.pi / n_az) + 0.5).long(), n_az)
    b = (torch.bucketize(el, edges, right=True) - 1).clamp_(0, spec.n_beams - 1)
    keep = (r2 > 0) & ~(r2 < float(spec.min_range) ** 2) & (el >= edges[0]) & (el < edges[-1])
    if spec.max_range is not None:
        keep &= ~(r2 >= float(spec.max_range) ** 2)
    cell = torch.where(keep, b * n_az + c, n_cells)                # dropped rows fall into a slot past the grid
    key = (r2.view(torch.int32).long() << 32) | torch.arange(n, device=points.device)
    empty = torch.iinfo(torch.int64).max
    table = torch.full((n_cells + 1,), empty, dtype=torch.int64, device=points.device)
    table.scatter_reduce_(0, cell, key, "amin")
    occ = (table[:n_cells] != empty).nonzero().squeeze(1)
    rows = table[occ] & 0xFFFFFFFF
    ob, oc = occ // n_az, occ % n_az
    r = torch.sqrt(dx[rows] * dx[rows] + dy[rows] * dy[rows] + dz[rows] * dz[rows])
    rc = r * cos_el[ob]
    out = torch.stack([rc * cos_az[oc], rc * sin_az[oc], r * sin_el[ob]], dim=1).float()
    return out, rows.int()


def bench_resample(batch, reps):
    import torch
    from lidog_amd import raycast, synth
    dev = torch.device("cuda")
    spec = raycast.sensor(TARGET)
    origin = torch.from_numpy(raycast.origin_between(SOURCE, TARGET)).to(dev)
    tables = spec.device_tables(dev)
    scans = [torch.from_numpy(synth.scan_points_labels(j, SOURCE)[0]).to(dev) for j in range(batch)]
    sides = {"hip": lambda p: raycast.raycast_points(p, spec, origin),
             "torch": lambda p: torch_raycast(p, spec, origin, tables),
             "hip_launch": lambda p: raycast._launch(p, spec, origin, True, False)}
    same = []
    for p in scans:                                      # the two sides give the same result before they are timed
        a, b = sides["hip"](p), sides["torch"](p)
        same.append(bool(torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))))
    dev_ms, host_ms, rows = {k: [] for k in sides}, {k: [] for k in sides}, []
    for r in range(reps + 2):
        for p in scans:
            for name, fn in sides.items():               # alternating call by call
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record()
                out = fn(p)
                b.record()
                t1 = time.perf_counter()
                b.synchronize()
                if r >= 2:                               # two untimed passes: first use of every kernel and buffer
                    dev_ms[name].append(a.elapsed_time(b))
                    host_ms[name].append((t1 - t0) * 1e3)
                    if name == "hip":
                        rows.append(int(out[1].shape[0]))
    res = {"bench": "raycast_points", "source": SOURCE, "target": TARGET, "batch": batch, "calls": len(dev_ms["hip"]),
           "points": int(scans[0].shape[0]), "cells": spec.n_cells, "rows_out_median": statistics.median(rows),
           "torch_gives_the_same_bytes": all(same)}
    for name in sides:
        res[f"{name}_device_ms_median"] = statistics.median(dev_ms[name])
        res[f"{name}_device_ms_min"] = min(dev_ms[name])
        res[f"{name}_host_ms_median"] = statistics.median(host_ms[name])
    res["torch_over_hip_device"] = res["torch_device_ms_median"] / res["hip_device_ms_median"]
    return res


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
    sets = {"plain": SynthScans(n, SOURCE, bev_size=bev_image_size(50.0)),
            "raycast": AugmentedSynthScans(n, SOURCE, None, seed=1, raycast=TARGET)}
    torch.manual_seed(0)
    model = build_model("MinkUNet34")
    model, step, _ = build_step(model, "MinkUNet34", lr=0.01)
    order = [[(k * batch + j) % n for j in range(batch)] for k in range(steps)]
    voxels = {}
    for name, d in sets.items():                       # every scan in the cache, every kernel used once
        for k in range(2):
            b = d.batch([(k * batch + j) % n for j in range(batch)], "cpu" if name == "plain" else "cuda")
        voxels[name] = int(b["coords_int"].shape[0])
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
    res = {"bench": "raycast_step", "model": "MinkUNet34", "config": SOURCE, "raycast_to": TARGET, "batch": batch,
           "steps": steps, "rounds": rounds}
    for name, t in times.items():
        res[f"{name}_ms_per_step_median"] = statistics.median(t)
        res[f"{name}_ms_per_step"] = t
        res[f"{name}_batch_voxels"] = voxels[name]
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
    print(json.dumps(bench_resample(a.batch, a.reps)), flush=True)
    if not a.skip_steps:
        print(json.dumps(bench_steps(a.batch, a.steps, a.warmup, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
