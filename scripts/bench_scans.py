"""Scans read from files (lidog_amd.scans) on the same box, over files written from the synthetic generator into a
temporary directory: KITTI-like (kitti120k points, 4 floats per record, int32 labels with instance ids in the upper half)
and nuScenes-like (nusc35k points, 5 floats per record, uint8 labels).

  (a) one load_scan per file: device time between HIP events recorded on the merge stream around the call (the upload of
      the file's bytes and the read of `info` included, since the stream waits for them) and the host wall time of the
      call, next to the host time of the numpy restatement on the same files (np.fromfile, mask, look-up, radius mask),
      median over --reps after two untimed passes
  (b) what crosses to the host: torch's profiler around --reps load_scan calls, counting device -> host copies and
      stream / device synchronisations per scan (the claim is ONE copy, `info`, and no other wait)
  (c) MinkUNet34BEV training steps (batch --batch) on FileScans batches of the KITTI-like files (BEV form, no
      augmentation list, use_cache off: every file is read and uploaded again) against SynthScans batches of the same
      scans served from a host cache, so the same voxel counts but not like for like, alternating round by
      round as Fit.run drives them; each round times --steps steps with the host clock after one synchronisation, behind
      --warmup untimed steps

One JSON line per measurement.

    python scripts/bench_scans.py --batch 4 --reps 20 --steps 10 --warmup 3 --rounds 3
"""
import argparse
import functools
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEARNING_MAP = {0: -1, 1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 6: 5, 7: 6}      # raw id = class + 1


def write_files(root, n):
    """n KITTI-like frames (sequences 00 and 08 hold the same frames) and n nuScenes-like files with their pair lists"""
    import numpy as np
    from lidog_amd import synth
    for j in range(n):
        pts, labels = synth.scan_points_labels(j, "kitti120k")
        rng = np.random.default_rng([j, 77])
        rec = np.concatenate([pts, rng.random((pts.shape[0], 1), dtype=np.float32)], axis=1)
        raw = (labels + 1).astype(np.uint32) | (rng.integers(0, 1 << 16, pts.shape[0]).astype(np.uint32) << 16)
        for seq in ("00", "01", "08"):
            for d in ("velodyne", "labels"):
                os.makedirs(os.path.join(root, "kitti", "sequences", seq, d), exist_ok=True)
            if seq != "01":
                rec.tofile(os.path.join(root, "kitti", "sequences", seq, "velodyne", f"{j:06d}.bin"))
                raw.view(np.int32).tofile(os.path.join(root, "kitti", "sequences", seq, "labels", f"{j:06d}.label"))
        pts, labels = synth.scan_points_labels(j, "nusc35k")
        rec = np.concatenate([pts, rng.random((pts.shape[0], 2), dtype=np.float32)], axis=1)
        os.makedirs(os.path.join(root, "nusc", "samples"), exist_ok=True)
        rec.tofile(os.path.join(root, "nusc", "samples", f"{j}.bin"))
        (labels + 1).astype(np.uint8).tofile(os.path.join(root, "nusc", "samples", f"{j}_lidarseg.bin"))
    for name in ("train.txt", "val.txt"):
        with open(os.path.join(root, "nusc", name), "w") as f:
            f.writelines(f"samples/{j}.bin samples/{j}_lidarseg.bin\n" for j in range(n))


def numpy_load(fmt, points_path, labels_path, lut, in_radius=50.0):
    """the reference's first mile on the host (semantickitti.py:106-112,190-197, nuscenes.py:150-160,245-246)"""
    import numpy as np
    pcd = np.fromfile(points_path, dtype=np.float32).reshape((-1, fmt["stride"]))
    raw = np.fromfile(labels_path, dtype=fmt["labels"])
    sem = lut[raw & fmt["mask"] if fmt["mask"] is not None else raw].astype(np.int32)
    points = pcd[:, :3]
    mask = np.sum(np.square(points), axis=1) < in_radius ** 2
    return points[mask], sem[mask]


def _listing(root, name):
    from lidog_amd import scans
    return scans.listing(name, os.path.join(root, "kitti" if name == "SemanticKITTI" else "nusc"), "train", version="mini")


def bench_load(root, name, reps, lut):
    import torch
    from lidog_amd import data, scans
    dev = torch.device("cuda")
    side = data.merge_stream(dev)
    lst = _listing(root, name)
    fmt = lst.format
    dev_ms, host_ms, numpy_ms, read_ms, kept = [], [], [], [], []
    with torch.cuda.stream(side):
        dlut = torch.from_numpy(lut).to(dev)
    for r in range(reps + 2):
        for p, l in lst.files:
            t0 = time.perf_counter()
            want = numpy_load(fmt, p, l, lut)
            t1 = time.perf_counter()
            pts, labels, stride = scans.read_files(fmt, p, l)
            t2 = time.perf_counter()
            with torch.cuda.stream(side):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(side)
                out = scans.load_scan(torch.from_numpy(pts).to(dev), torch.from_numpy(labels).to(dev), dlut, stride,
                                      fmt["mask"], 50.0, name=p)
                b.record(side)
                t3 = time.perf_counter()
                b.synchronize()
            assert out["points"].shape[0] == want[0].shape[0]
            if r >= 2:                                   # two untimed passes: first use of every kernel and buffer
                dev_ms.append(a.elapsed_time(b))
                host_ms.append((t3 - t2) * 1e3)
                read_ms.append((t2 - t1) * 1e3)
                numpy_ms.append((t1 - t0) * 1e3)
                kept.append(int(out["points"].shape[0]))
    return {"bench": "load_scan", "dataset": name, "files": len(lst), "scans": len(dev_ms),
            "points": int(pts.shape[0] // (4 * stride)), "kept_median": statistics.median(kept),
            "device_ms_median": statistics.median(dev_ms), "device_ms_min": min(dev_ms),
            "host_ms_median": statistics.median(host_ms), "file_read_host_ms_median": statistics.median(read_ms),
            "numpy_host_ms_median": statistics.median(numpy_ms)}


def trace_load(root, name, reps, lut):
    """device -> host copies and synchronisations per load_scan, from torch's profiler"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    from lidog_amd import data, scans
    dev = torch.device("cuda")
    side = data.merge_stream(dev)
    lst = _listing(root, name)
    fmt = lst.format
    p, l = lst.files[0]
    pts, labels, stride = scans.read_files(fmt, p, l)
    res = {"bench": "load_scan_trace", "dataset": name, "scans": reps}
    try:
        with torch.cuda.stream(side):
            dlut = torch.from_numpy(lut).to(dev)
            dp, dl = torch.from_numpy(pts).to(dev), torch.from_numpy(labels).to(dev)
            scans.load_scan(dp, dl, dlut, stride, fmt["mask"], 50.0)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(reps):
                    scans.load_scan(dp, dl, dlut, stride, fmt["mask"], 50.0)
                torch.cuda.synchronize()
        names = {}
        for e in prof.events():
            names[e.name] = names.get(e.name, 0) + 1
        pick = lambda *keys: {k: v for k, v in names.items() if any(s in k.lower() for s in keys)}
        res["copies"] = pick("memcpy", "dtoh", "htod")
        res["synchronisations"] = pick("synchronize")
        res["kernels"] = {k: v for k, v in names.items() if k.startswith("k_scan") or k.startswith("k_mix")}
    except Exception as e:                               # the profiler is optional equipment
        res["error"] = f"{type(e).__name__}: {e}"
    return res


def _steps(step, data, batches, epoch=0):
    cur = data.batch(batches[0], "cuda")
    for i in range(len(batches)):
        nxt = data.batch(batches[i + 1], "cuda") if i + 1 < len(batches) else None
        step.training_step(cur, epoch=epoch, prefetch=nxt)
        cur = nxt


def bench_steps(root, batch, steps, warmup, rounds, lut):
    import torch
    from lidog_amd import scans, synth
    from lidog_amd.train import SynthScans, bev_image_size, build_model, build_step
    synth.scan_voxels = functools.lru_cache(maxsize=None)(synth.scan_voxels)
    n = batch * 2
    size = bev_image_size(50.0)
    sets = {"synthetic": SynthScans(n, "kitti120k", bev_size=size),
            "files": scans.FileScans(_listing(root, "SemanticKITTI"), lut, bev=(50.0, size))}
    torch.manual_seed(0)
    model = build_model("MinkUNet34BEV")
    model, step, _ = build_step(model, "MinkUNet34BEV", lr=1e-3)
    order = [[(k * batch + j) % n for j in range(batch)] for k in range(steps)]
    voxels = {}
    for name, d in sets.items():                       # every scan in the cache, every kernel used once
        for k in range(2):
            b = d.batch([(k * batch + j) % n for j in range(batch)], "cuda")
            voxels[name] = int(b["coords_int"].shape[0])
        _steps(step, d, order[:warmup])
    times = {k: [] for k in sets}
    for r in range(rounds):
        for name, d in sets.items():
            _steps(step, d, order[:warmup])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _steps(step, d, order)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / steps)
    res = {"bench": "files_step", "model": "MinkUNet34BEV", "batch": batch, "steps": steps, "rounds": rounds,
           "voxels_of_a_batch": voxels,
           # not like for like: the synthetic scans come from a host cache, every file is read and uploaded again
           "synthetic_cached": True, "files_cached": False}
    for name, t in times.items():
        res[f"{name}_ms_per_step_median"] = statistics.median(t)
        res[f"{name}_ms_per_step"] = t
    res["files_over_synthetic"] = res["files_ms_per_step_median"] / res["synthetic_ms_per_step_median"]
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
    from lidog_amd import scans
    torch.cuda.set_device(0)
    lut = scans.label_lut(LEARNING_MAP)
    with tempfile.TemporaryDirectory() as root:
        write_files(root, a.batch * 2)
        for name in ("SemanticKITTI", "nuScenes"):
            print(json.dumps(bench_load(root, name, a.reps, lut)), flush=True)
            print(json.dumps(trace_load(root, name, a.reps, lut)), flush=True)
        if not a.skip_steps:
            print(json.dumps(bench_steps(root, a.batch, a.steps, a.warmup, a.rounds, lut)), flush=True)


if __name__ == "__main__":
    main()
