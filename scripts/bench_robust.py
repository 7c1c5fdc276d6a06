"""RobustNet on the same box and the same kitti120k scans (synth "kitti120k", 0.05 m), configs/robustnet settings:
SoftDICE, Adam (lr 0.01), batch 4, the instance-whitening loss on (epoch 5 on).

  (a) the instance-whitening loss, forward + backward, on the five aux maps of one MinkUNet34Robust forward pass: the
      fused path (lidog_amd.losses.iw_loss, one launch each way) against the literal bmm restatement of the reference
      (IWLoss per map, [n, C, C] intermediates), device time from HIP events, median over --reps
  (b) MinkUNet34 against MinkUNet34Robust training steps at epoch 5, alternating round by round; each round times
      --steps steps with the host clock after one synchronisation, behind --warmup untimed steps

One JSON line per measurement.

    python scripts/bench_robust.py --steps 10 --warmup 3 --rounds 3 --reps 20
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _literal(f_map):
    import torch
    n, C = f_map.shape
    eye = torch.eye(C, device=f_map.device)
    mask = torch.ones((C, C), device=f_map.device).triu(1)
    x = f_map.view(n, C, -1)
    f_cor = torch.bmm(x, x.transpose(1, 2)).div(n - 1) + 1e-5 * eye
    return torch.sum(torch.sum(torch.abs(f_cor * mask), dim=(1, 2), keepdim=True)) / n


def _device_ms(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def bench_iw(batch, reps):
    import torch
    import lidog_amd
    import lidog_amd.me as ME
    from lidog_amd.losses import iw_loss
    model = lidog_amd.MinkUNet34Robust(1, 7, 3).cuda().train()
    with torch.no_grad():
        _, maps = model(ME.SparseTensor(batch["source_features0"], coordinates=batch["coords_int"]), is_seg=False)
    feats = [m.F.detach().clone() for m in maps]
    shapes = [list(f.shape) for f in feats]
    mb = sum(f.numel() * 4 for f in feats) / 1e6

    def fused():
        xs = [f.requires_grad_(True) for f in feats]
        t, _ = iw_loss(xs)
        t.backward()
        for f in xs:
            f.grad = None

    def literal():
        xs = [f.requires_grad_(True) for f in feats]
        t = sum(_literal(f) / len(xs) for f in xs)
        t.backward()
        for f in xs:
            f.grad = None

    for fn in (fused, literal):
        fn()
    torch.cuda.synchronize()
    res = {}
    for name, fn in (("fused", fused), ("literal", literal)):
        ts = _device_ms(fn, reps)
        res[name] = statistics.median(ts)
        print(json.dumps({"iw_path": name, "maps": shapes, "map_mb": round(mb, 1), "reps": reps,
                          "fwd_bwd_ms_median": round(res[name], 4), "fwd_bwd_ms_min": round(min(ts), 4)}), flush=True)
    print(json.dumps({"iw_ratio": "literal/fused", "ratio": round(res["literal"] / res["fused"], 1)}), flush=True)
    del model, maps, feats
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--epoch", type=int, default=5)
    ap.add_argument("--models", default="MinkUNet34,MinkUNet34Robust")
    a = ap.parse_args()
    import torch
    import lidog_amd  # noqa: F401
    from lidog_amd import synth
    from lidog_amd.train import build_model, build_step
    torch.manual_seed(0)
    batch = synth.make_batch(list(range(a.batch)), "kitti120k", device="cuda")
    bench_iw(batch, a.reps)
    kinds = a.models.split(",")
    steps = {}
    for k in kinds:
        model = build_model(k, device="cuda")
        _, step, _ = build_step(model, k, optimizer="Adam", lr=1e-2)
        for _ in range(a.warmup):
            step.training_step(batch, epoch=a.epoch)
        steps[k] = step
    times = {k: [] for k in kinds}
    last = {}
    for _ in range(a.rounds):
        for k in kinds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                out = steps[k].training_step(batch, epoch=a.epoch)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
            last[k] = {n: float(v) for n, v in out.items()}
    rows = int(batch["coords_int"].shape[0])
    for k in kinds:
        print(json.dumps({"model": k, "batch": a.batch, "scans": "kitti120k", "rows": rows, "epoch": a.epoch,
                          "steps": a.steps, "rounds": a.rounds, "step_ms_median": round(statistics.median(times[k]), 3),
                          "step_ms_min": round(min(times[k]), 3), "step_ms_rounds": [round(t, 3) for t in times[k]],
                          "losses": last[k]}), flush=True)
    if len(kinds) == 2:
        r = statistics.median(times[kinds[1]]) / statistics.median(times[kinds[0]])
        print(json.dumps({"ratio": f"{kinds[1]}/{kinds[0]}", "step_time_ratio": round(r, 3)}), flush=True)


if __name__ == "__main__":
    main()
