"""MixStyle (csrc/mixstyle.hip) on one box: what the three launches cost against a torch composition of the same result,
and what the flag costs a MinkUNet34 training step.

  kernels  lidog_mixstyle_stats + _apply + _bwd against index_add_ sums in float64, the mix on [B, C] tables, a gather
           and the elementwise passes in torch, on block1's and block2's output of a kitti120k batch (the rows the
           modules see); the two alternate round by round, timed with device events
  step     the MinkUNet34 step (SoftDICE, Adam, configs/ibn settings) without MixStyle on the trunk executor, without it
           on the operator path (lidog_amd.trunk.set_enabled(False)), and with MixStyle behind block1 / block2 (which
           takes the operator path); the three alternate round by round, host clock after one synchronisation

One JSON line per part.  No ratio is promised.

    python scripts/bench_mixstyle.py --rounds 3 --reps 20 --torch-reps 2 --steps 10
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EPS = 1e-6


def _stage_outputs(batch):
    """{stage: SparseTensor}: block1's and block2's output of a MinkUNet34 forward pass in eval mode"""
    import torch
    import lidog_amd.me as ME
    from lidog_amd.train import build_model
    model = build_model("MinkUNet34", device="cuda").eval()
    seen = {}
    hooks = [getattr(model, s).register_forward_hook(lambda mod, inp, out, s=s: seen.setdefault(s, out))
             for s in ("block1", "block2")]
    with torch.no_grad():
        model(ME.SparseTensor(batch["source_features0"], coordinates=batch["coords_int"]))
    for h in hooks:
        h.remove()
    return seen


def _torch_mixstyle(x, dy, bidl, cnt, lam, partner):
    import torch
    B, C = cnt.shape[0], x.shape[1]
    xd = x.double()
    s1 = torch.zeros((B, C), dtype=torch.float64, device=x.device).index_add_(0, bidl, xd)
    s2 = torch.zeros((B, C), dtype=torch.float64, device=x.device).index_add_(0, bidl, xd * xd)
    mu = s1 / cnt
    sig = torch.sqrt(torch.clamp_min((s2 - s1 * s1 / cnt) / (cnt - 1), 0.0) + EPS)
    mu_mix = lam * mu + (1 - lam) * mu[partner]
    sig_mix = lam * sig + (1 - lam) * sig[partner]
    sub, scale, add = mu.float(), (sig_mix / sig).float(), mu_mix.float()
    y = torch.addcmul(add[bidl], x - sub[bidl], scale[bidl])
    return y, dy * scale[bidl]


def note(msg):
    sys.stderr.write(f"bench_mixstyle: {msg}\n")
    sys.stderr.flush()


def bench_kernels(batch_size, rounds, reps, torch_reps):
    import numpy as np
    import torch
    from lidog_amd import _lib, synth
    from lidog_amd._lib import call, ptr
    L = _lib.load()
    batch = synth.make_batch(list(range(batch_size)), "kitti120k", device="cuda")
    rec = {"bench": "mixstyle_kernels", "config": "kitti120k", "batch": batch_size, "rounds": rounds, "reps": reps,
           "torch_reps": torch_reps}
    rs = np.random.RandomState(0)
    for stage, st in _stage_outputs(batch).items():
        x = st.F.contiguous()
        n, C = x.shape
        perm, seg_off, bid, B = st.coordinate_manager.segments(st.coordinate_map_key)
        dy = torch.randn_like(x)
        lam = torch.from_numpy(rs.beta(0.1, 0.1, B).astype(np.float32)).pin_memory()
        partner = torch.from_numpy(((np.arange(B) + 1) % B).astype(np.int32)).pin_memory()
        tabs = torch.empty((5, B * C), dtype=torch.float32, device="cuda")
        ws = torch.empty(L.lidog_mixstyle_ws(B, C), dtype=torch.float64, device="cuda")
        y, dx = torch.empty_like(x), torch.empty_like(x)

        def hip():
            call("lidog_mixstyle_stats", ptr(x), n, C, B, ptr(perm), ptr(seg_off), ptr(lam), ptr(partner), EPS,
                 ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), ptr(tabs[3]), ptr(tabs[4]), ptr(ws))
            call("lidog_mixstyle_apply", ptr(x), n, C, B, ptr(bid), ptr(tabs[2]), ptr(tabs[3]), ptr(tabs[4]), ptr(y))
            call("lidog_mixstyle_bwd", ptr(dy), n, C, B, ptr(bid), ptr(tabs[3]), ptr(dx))

        bidl = bid.long()
        cnt = torch.bincount(bidl, minlength=B).double()[:, None]
        lam_d, partner_d = lam.cuda().double()[:, None], partner.cuda().long()

        def composed():
            return _torch_mixstyle(x, dy, bidl, cnt, lam_d, partner_d)

        ms = {"hip": [], "torch": []}
        for r in range(rounds + 1):                     # round 0 is untimed
            # the composition's float64 index_add_ onto B rows is seconds-slow at these sizes: it gets fewer repetitions
            for name, fn, k in (("hip", hip, reps), ("torch", composed, torch_reps)):
                fn()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(k):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                if r:
                    ms[name].append(t0.elapsed_time(t1) / k * 1e3)
                note(f"{stage} round {r} {name}: {t0.elapsed_time(t1) / k * 1e3:.1f} us per call")
        yt, dxt = composed()
        rec[stage] = {"rows": n, "C": C, "B": B, "hip_us_median": round(statistics.median(ms["hip"]), 2),
                      "torch_us_median": round(statistics.median(ms["torch"]), 2),
                      "hip_us": [round(v, 2) for v in ms["hip"]], "torch_us": [round(v, 2) for v in ms["torch"]],
                      "torch_over_hip": round(statistics.median(ms["torch"]) / statistics.median(ms["hip"]), 2),
                      "max_abs_y_diff": float((y - yt).abs().max()), "max_abs_dx_diff": float((dx - dxt).abs().max())}
    return rec


def bench_step(batch_size, rounds, steps, warmup):
    import torch
    from lidog_amd import synth, trunk
    from lidog_amd.train import build_model, build_step
    torch.manual_seed(0)
    batch = synth.make_batch(list(range(batch_size)), "kitti120k", device="cuda")

    def make(**ms):
        model = build_model("MinkUNet34", device="cuda", **ms)
        return build_step(model, "MinkUNet34", optimizer="Adam", lr=1e-2)[1]

    plain = make()
    variants = {"executor": (plain, True), "operators": (plain, False),
                "mixstyle": (make(mixstyle_layers=("block1", "block2"), mixstyle_p=0.5, mixstyle_alpha=0.1), True)}
    was = trunk.ENABLED
    ms, paths = {k: [] for k in variants}, {}
    try:
        for r in range(rounds + 1):                     # round 0 is untimed: warm-up of every variant
            for name, (step, executor) in variants.items():
                trunk.set_enabled(executor and was)
                for _ in range(warmup if r == 0 else 1):
                    step.training_step(batch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    out = step.training_step(batch)
                torch.cuda.synchronize()
                if r:
                    ms[name].append((time.perf_counter() - t0) / steps * 1e3)
                note(f"step round {r} {name}: {(time.perf_counter() - t0) / steps * 1e3:.2f} ms per step")
                paths[name] = getattr(step, "last_path", None)
                assert torch.isfinite(out["loss"]).all()
    finally:
        trunk.set_enabled(was)
    rec = {"bench": "mixstyle_step", "model": "MinkUNet34", "config": "kitti120k", "batch": batch_size,
           "voxels": int(batch["coords_int"].shape[0]), "rounds": rounds, "steps_per_round": steps, "paths": paths}
    for k, v in ms.items():
        rec[k + "_ms_median"] = round(statistics.median(v), 3)
        rec[k + "_ms"] = [round(x, 3) for x in v]
    rec["mixstyle_over_operators"] = round(rec["mixstyle_ms_median"] / rec["operators_ms_median"], 4)
    rec["mixstyle_over_executor"] = round(rec["mixstyle_ms_median"] / rec["executor_ms_median"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parts", nargs="+", default=["kernels", "step"], choices=["kernels", "step"])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import lidog_amd  # noqa: F401
    if "kernels" in a.parts:
        print(json.dumps(bench_kernels(a.batch, a.rounds, a.reps, a.torch_reps)), flush=True)
    if "step" in a.parts:
        print(json.dumps(bench_step(a.batch, a.rounds, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
