"""PolarMix / LaserMix scan mixing on the same box and the same kitti120k scans (synth "kitti120k", 0.05 m):

  (a) one merge (lidog_amd.data.polarmix_merge / lasermix_merge) of each pair of a batch of --batch kitti120k pairs
      against a torch composition of the same result (torch.atan2 masks, boolean indexing, torch.cat, a float64
      rotation, then the same quantize_rows), alternating merge by merge on the merge stream with the same draws:
      device time between HIP events recorded around the call (host draws and read-backs included, since the stream
      waits for them) and the host wall time of the call, median over --reps.  The composition decides rows on a
      boundary by atan2, not by the exact predicates, so its row count may differ by a few rows; both are reported.
  (b) MinkUNet34 training steps (SoftDICE, Adam, batch --batch) on plain one-source batches, on --mix cosmix batches and
      on --mix polarmix / lasermix batches (lidog_amd.train.MixedSynthScans), alternating round by round as Fit.run
      drives them (the next batch is built before this step is queued); each round times --steps steps with the host
      clock after one synchronisation, behind --warmup untimed steps.  Every dataset reads its scans from an in-process
      cache, so none pays for the synthetic scan generator.

One JSON line per measurement.

    python scripts/bench_sensormix.py --batch 4 --reps 20 --steps 10 --warmup 3 --rounds 3
"""
import argparse
import functools
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _columns(base, donor, keep, parts):
    import torch
    out = {}
    for k in ("features", "sem_labels"):
        out[k] = torch.cat([base[k][keep]] + [donor[k][p] for p in parts])
    return out


def _finish(coords, cols):
    """the merges' own quantisation: voxel rows -> the first row of every voxel"""
    import torch
    from lidog_amd.data import quantize_rows
    rows = torch.cat([torch.zeros((coords.shape[0], 1), dtype=torch.int32, device=coords.device),
                      coords.to(torch.int32)], dim=1).contiguous()
    q, index = quantize_rows(rows, return_index=True)
    return {"coordinates": q, "index": index, **{k: v[index] for k, v in cols.items()}}


def torch_lasermix(scan0, scan1, draws, pitch=(-25.0, 3.0)):
    import numpy as np
    import torch
    donor, base = (scan0, scan1) if draws["source"] == 0 else (scan1, scan0)
    th = torch.from_numpy(np.linspace(np.radians(pitch[0]), np.radians(pitch[1]), draws["n_areas"] + 1)[1:-1]).to(
        base["coordinates"].device)

    def bands(c):
        p = c.double() * 2 + 1
        return torch.bucketize(torch.atan2(p[:, 2], torch.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1])), th, right=True)

    keep, take = bands(base["coordinates"]) % 2 == 0, bands(donor["coordinates"]) % 2 == 1
    coords = torch.cat([base["coordinates"][keep], donor["coordinates"][take]])
    return _finish(coords, _columns(base, donor, keep, [take]))


def torch_polarmix(scan0, scan1, draws, instance_classes=(0, 1)):
    import numpy as np
    import torch
    donor, base = (scan0, scan1) if draws["source"] == 0 else (scan1, scan0)

    def inside(c):
        p = c.double() * 2 + 1
        return torch.remainder(torch.atan2(p[:, 1], p[:, 0]) - draws["alpha"], 2 * np.pi) < np.pi

    nb = base["coordinates"].shape[0]
    keep = ~inside(base["coordinates"]) if draws["swap"] else torch.ones(nb, dtype=torch.bool,
                                                                         device=base["coordinates"].device)
    parts, coords = [], [base["coordinates"][keep]]
    if draws["swap"]:
        take = inside(donor["coordinates"])
        parts.append(take)
        coords.append(donor["coordinates"][take])
    if draws["paste"]:
        inst = torch.isin(donor["sem_labels"], torch.tensor(instance_classes, device=donor["sem_labels"].device))
        c = donor["coordinates"][inst]
        parts += [inst] * 3
        coords.append(c)
        for w in (draws["omega1"], draws["omega2"]):
            u, v = c[:, 0].double() + 0.5, c[:, 1].double() + 0.5
            cw, sw = float(np.cos(w)), float(np.sin(w))
            coords.append(torch.stack([torch.floor(cw * u - sw * v).to(c.dtype), torch.floor(sw * u + cw * v).to(c.dtype),
                                       c[:, 2]], dim=1))
    return _finish(torch.cat(coords), _columns(base, donor, keep, parts))


def bench_merge(method, batch, reps):
    import numpy as np
    import torch
    from lidog_amd import data
    from lidog_amd.train import MixedSynthScans
    ds = MixedSynthScans(batch, batch, ("kitti120k", "kitti120k"), method=method, seed=1)
    draw = data.draw_polarmix if method == "polarmix" else functools.partial(data.draw_lasermix, areas=ds.areas)
    composition = torch_polarmix if method == "polarmix" else torch_lasermix
    dev = torch.device("cuda")
    side = data.merge_stream(dev)
    with torch.cuda.stream(side):
        pairs = [(ds._scan(0, j, dev), ds._scan(1, int(ds.pairs.perm1[j]), dev)) for j in range(batch)]
    runs = {"hip": lambda s0, s1, d: ds.merge(s0, s1, draws=d), "torch": composition}
    dev_ms = {k: [] for k in runs}
    host_ms = {k: [] for k in runs}
    rows = {k: [] for k in runs}
    for r in range(reps + 2):
        for i, (s0, s1) in enumerate(pairs):
            d = draw(np.random.RandomState([r, i]))
            for name in (("hip", "torch") if (r + i) % 2 == 0 else ("torch", "hip")):      # alternating
                with torch.cuda.stream(side):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    a.record(side)
                    out = runs[name](s0, s1, d)
                    b.record(side)
                    t1 = time.perf_counter()
                    b.synchronize()
                if r >= 2:                               # two untimed passes: first use of every kernel and buffer
                    dev_ms[name].append(a.elapsed_time(b))
                    host_ms[name].append((t1 - t0) * 1e3)
                    rows[name].append(int(out["coordinates"].shape[0]))
    res = {"bench": "sensormix_merge", "method": method, "config": "kitti120k", "batch": batch,
           "merges": len(dev_ms["hip"])}
    for name in runs:
        res[f"{name}_device_ms_median"] = statistics.median(dev_ms[name])
        res[f"{name}_device_ms_min"] = min(dev_ms[name])
        res[f"{name}_host_ms_median"] = statistics.median(host_ms[name])
        res[f"{name}_merged_rows_median"] = statistics.median(rows[name])
    res["rows_differ_in_merges"] = sum(x != y for x, y in zip(rows["hip"], rows["torch"]))
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
    from lidog_amd.train import MixedSynthScans, SynthScans, build_model, build_step
    synth.scan_voxels = functools.lru_cache(maxsize=None)(synth.scan_voxels)
    n = batch * 2
    pair = ("kitti120k", "kitti120k")
    sets = {"plain": SynthScans(n, "kitti120k")}
    for method in ("cosmix", "polarmix", "lasermix"):
        sets[method] = MixedSynthScans(n, n, pair, method=method, seed=1)
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
    res = {"bench": "sensormix_step", "model": "MinkUNet34", "config": "kitti120k", "batch": batch, "steps": steps,
           "rounds": rounds}
    for name, t in times.items():
        res[f"{name}_ms_per_step_median"] = statistics.median(t)
        res[f"{name}_ms_per_step"] = t
    for name in ("cosmix", "polarmix", "lasermix"):
        res[f"{name}_over_plain"] = res[f"{name}_ms_per_step_median"] / res["plain_ms_per_step_median"]
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
    if not torch.cuda.is_available():
        raise SystemExit("bench_sensormix.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    for method in ("polarmix", "lasermix"):
        print(json.dumps(bench_merge(method, a.batch, a.reps)), flush=True)
    if not a.skip_steps:
        print(json.dumps(bench_steps(a.batch, a.steps, a.warmup, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
