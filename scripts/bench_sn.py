"""The SN car-size scaling baseline (train_scaling_based.py) on one box, on the synthetic car scans (synth
"kitti120k_cars" / "nusc35k_cars", 0.05 m):

  (a) one scan's clustering: lidog_amd.cluster.dbscan_count + cluster_boxes on the car voxels of each of --scans scans
      that pass get_average_dims' min_pts, the boxes copied to the host: device time between HIP events on the stream
      it runs on (read-backs included, since the stream waits for them) and host wall time, median per scan after two
      untimed passes; next to sklearn.cluster.DBSCAN(eps=0.5, min_samples=10).fit_predict on the same float32 arrays
      on this box's host (n_jobs=None, as the reference calls it) when sklearn imports here, with the labels compared
  (b) the whole start-up statistic: lidog_amd.data.average_dims over a dataset of --dataset-scans scans (20 % drawn),
      scans read from an in-process cache so that the synthetic generator is not timed; wall time
  (c) MinkUNet34 training steps (SoftDICE, Adam, batch --batch) on kitti120k_cars with --sn-targets nusc35k_cars
      (lidog_amd.train.ScaledSynthScans: one re-quantisation per item), and with --source-augment RandomRotation
      RandomScale on top (every item augmented before it is scaled), against plain batches of the same scans,
      alternating round by round as scripts/bench_mix.py does

One JSON line per measurement.

    python scripts/bench_sn.py --scans 20 --dataset-scans 100 --batch 4 --steps 10 --warmup 3 --rounds 3
"""
import argparse
import functools
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = ("kitti120k_cars", "nusc35k_cars")


def _car_scans(config, n_scans):
    """the car voxels of the first n_scans scans with more than min_pts of them"""
    import numpy as np
    from lidog_amd import data, synth
    from lidog_amd.train import SynthDataset
    min_pts, _ = data.sn_thresholds(SynthDataset(1, config).name)
    out, seed = [], 0
    while len(out) < n_scans and seed < 20 * n_scans:
        vox, labels = synth.scan_voxels(seed, config)
        car = np.ascontiguousarray(vox[labels == 0], dtype=np.int32)
        if car.shape[0] > min_pts:
            out.append(car)
        seed += 1
    return out


def bench_cluster(config, n_scans):
    import numpy as np
    import torch
    from lidog_amd import cluster, synth
    voxel = synth.CONFIGS[config]["voxel"]
    cars = _car_scans(config, n_scans)
    dev = [torch.from_numpy(c).cuda() for c in cars]
    st = torch.cuda.current_stream()
    dev_ms, host_ms, labels = [], [], []
    for r in range(3):
        for c in dev:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record(st)
            lab, k = cluster.dbscan_count(c, voxel, eps=0.5, min_samples=10)
            boxes = [t.cpu() for t in cluster.cluster_boxes(c, lab, k)]
            b.record(st)
            t1 = time.perf_counter()
            b.synchronize()
            if r == 2:                                   # two untimed passes: first use of every kernel and buffer
                dev_ms.append(a.elapsed_time(b))
                host_ms.append((t1 - t0) * 1e3)
                labels.append(lab.cpu().numpy())
    res = {"bench": "sn_cluster", "config": config, "scans": len(cars),
           "car_voxels_median": statistics.median(c.shape[0] for c in cars),
           "car_voxels_min_max": [min(c.shape[0] for c in cars), max(c.shape[0] for c in cars)],
           "clusters_median": statistics.median(int(l.max()) + 1 for l in labels),
           "device_ms_median": statistics.median(dev_ms), "device_ms_min_max": [min(dev_ms), max(dev_ms)],
           "host_ms_median": statistics.median(host_ms)}
    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        res["sklearn"] = "not importable on this box"
        return res
    sk_ms, equal = [], True
    for c, lab in zip(cars, labels):
        x = (torch.from_numpy(c) * voxel).numpy()       # the float32 array the reference clusters
        t0 = time.perf_counter()
        want = DBSCAN(eps=0.5, min_samples=10).fit_predict(x)
        sk_ms.append((time.perf_counter() - t0) * 1e3)
        equal = equal and np.array_equal(want, lab)
    res.update({"sklearn_ms_median": statistics.median(sk_ms), "sklearn_ms_min_max": [min(sk_ms), max(sk_ms)],
                "labels_equal_sklearn": bool(equal),
                "sklearn_over_device": statistics.median(sk_ms) / statistics.median(host_ms)})
    return res


def bench_average_dims(config, n):
    import numpy as np
    import torch
    from lidog_amd import data
    from lidog_amd.train import SynthDataset
    ds = SynthDataset(n, config)
    record = []
    for timed in (False, True):                         # the first pass fills the scan cache and uses every kernel once
        record.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dims = data.average_dims(ds, rng=np.random.RandomState(0), record=record)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
    return {"bench": "sn_average_dims", "config": config, "dataset_scans": n, "drawn": int(0.2 * n),
            "clustered": len(record), "dims": [float(d) for d in dims], "wall_ms": ms,
            "wall_ms_per_drawn_scan": ms / max(int(0.2 * n), 1)}


def _steps(step, data, batches, epoch=0):
    cur = data.batch(batches[0], "cuda")
    for i in range(len(batches)):
        nxt = data.batch(batches[i + 1], "cuda") if i + 1 < len(batches) else None
        step.training_step(cur, epoch=epoch, prefetch=nxt)
        cur = nxt


def bench_steps(batch, steps, warmup, rounds, scaling):
    import torch
    from lidog_amd.train import AugmentedSynthScans, ScaledSynthScans, SynthScans, build_model, build_step
    n = batch * 2
    augs = ["RandomRotation", "RandomScale"]
    sets = {"plain": SynthScans(n, "kitti120k_cars"),
            "sn": ScaledSynthScans(n, ("kitti120k_cars",), ("nusc35k_cars",), seed=1, scaling=scaling),
            # --sn-targets with --source-augment: every item augmented (sub_p 0.8) before it is scaled
            "sn_aug": ScaledSynthScans(n, ("kitti120k_cars",), ("nusc35k_cars",), seed=1, scaling=scaling,
                                       items=AugmentedSynthScans(n, ("kitti120k_cars",), augs, sub_p=0.8, seed=1))}
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
    res = {"bench": "sn_step", "model": "MinkUNet34", "config": "kitti120k_cars", "batch": batch, "steps": steps,
           "rounds": rounds, "scaling": [float(x) for x in scaling[0][0]]}
    for name, t in times.items():
        res[f"{name}_ms_per_step_median"] = statistics.median(t)
        res[f"{name}_ms_per_step"] = t
    res["sn_over_plain"] = res["sn_ms_per_step_median"] / res["plain_ms_per_step_median"]
    res["sn_aug_over_sn"] = res["sn_aug_ms_per_step_median"] / res["sn_ms_per_step_median"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scans", type=int, default=20)
    ap.add_argument("--dataset-scans", type=int, default=100)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    import torch
    from lidog_amd import data, synth
    torch.cuda.set_device(0)
    synth.scan_voxels = functools.lru_cache(maxsize=None)(synth.scan_voxels)
    for config in CONFIGS:
        print(json.dumps(bench_cluster(config, a.scans)), flush=True)
    dims = {}
    for config in CONFIGS:
        res = bench_average_dims(config, a.dataset_scans)
        dims[config] = res["dims"]
        print(json.dumps(res), flush=True)
    if not a.skip_steps:
        import numpy as np
        scaling = data.scaling_params([np.asarray(dims[CONFIGS[0]], dtype=np.float32)],
                                      [np.asarray(dims[CONFIGS[1]], dtype=np.float32)])
        print(json.dumps(bench_steps(a.batch, a.steps, a.warmup, a.rounds, scaling)), flush=True)


if __name__ == "__main__":
    main()
