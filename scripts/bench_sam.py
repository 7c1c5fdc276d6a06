"""The gradient-norm, SAM-perturbation and clipping launches (csrc/sam.hip) against the torch composition of the same
results, on the same box, alternating: device time between HIP events around --reps calls, median over --rounds, both
sides taking turns, on the flat buffers of MinkUNet34BEV (38.7 M elements).

  norm      lidog_flat_sqnorm (two launches, a device double)      against torch.linalg.vector_norm over the flat gradient
  perturb   lidog_sam_perturb (one launch: backup, w += e)         against backup = w.clone(); w.add_(g * (rho / (norm + 1e-12)))
  restore   the device copy of SAM.second_step
  clip      lidog_flat_clip (one launch)                           against g.mul_(clamp(max_norm / (norm + 1e-6), max=1))
            with a max_norm nothing reaches on both sides: the same bytes move and the values stay where they are

Neither side reads anything back.  `*_gb_per_s` counts 4 n bytes for the norm, 16 n for the perturbation (w and g read,
backup and w written), 8 n for the restore and the clip.  Then the step: the MinkUNet34 and MinkUNet34BEV training steps
of bench.py at --step-batch kitti120k scans plain, with grad_clip_norm and with sam_rho, alternating on models with the
same weights.  One JSON line per case.

    python scripts/bench_sam.py --rounds 7 --reps 20
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_losses import _alternate  # noqa: E402


def bench_kernels(rounds, reps, rho=0.05):
    import torch
    from lidog_amd._lib import call, ptr
    from lidog_amd.optim import SAM, FlatAdam
    from lidog_amd.train import build_model
    model = build_model("MinkUNet34BEV", 50.0, device="cuda").train()
    opt = FlatAdam(model, lr=1e-3)
    sam = SAM(opt, rho)
    f = opt.flat
    n = f.total
    g = torch.Generator(device="cuda").manual_seed(0)
    f.grad.copy_(torch.randn(n, generator=g, device="cuda") * 1e-3)
    w0 = f.flat.clone()
    word = opt._own_sqnorm()
    t_w, t_g = w0.clone(), f.grad.clone()
    state = {}

    def hip_norm():
        opt._launch_sqnorm(word)

    def torch_norm():
        state["norm"] = torch.linalg.vector_norm(t_g)

    def hip_perturb():
        call("lidog_sam_perturb", ptr(f.flat), ptr(f.grad), ptr(sam.backup), n, ptr(word), rho, 0)

    def torch_perturb():
        state["backup"] = t_w.clone()
        t_w.add_(t_g.mul(rho / (state["norm"] + 1e-12)))

    def restore():
        f.flat.copy_(sam.backup)

    def hip_clip():
        call("lidog_flat_clip", ptr(f.grad), n, ptr(word), 1e30, 1.0)

    def torch_clip():
        t_g.mul_(torch.clamp(1e30 / (state["norm"] + 1e-6), max=1.0))

    # one of each, compared, before the clock
    hip_norm(), torch_norm(), hip_perturb(), torch_perturb()
    norm_diff = abs(float(word.sqrt()) - float(state["norm"])) / float(state["norm"])
    w_diff = float((f.flat - t_w).abs().max())
    f.flat.copy_(w0), t_w.copy_(w0)
    t = _alternate({"hip_norm": hip_norm, "torch_norm": torch_norm, "hip_perturb": hip_perturb,
                    "torch_perturb": torch_perturb, "restore": restore, "hip_clip": hip_clip, "torch_clip": torch_clip},
                   rounds, reps)
    us = {k: round(1e3 * v, 2) for k, v in t.items()}
    gbs = lambda nbytes, ms: round(nbytes * n / (1e6 * ms), 1)
    print(json.dumps({
        "bench": "sam", "case": "kernels_MinkUNet34BEV", "elements": n, **{f"{k}_us": v for k, v in us.items()},
        "norm_torch_over_hip": round(t["torch_norm"] / t["hip_norm"], 2),
        "perturb_torch_over_hip": round(t["torch_perturb"] / t["hip_perturb"], 2),
        "clip_torch_over_hip": round(t["torch_clip"] / t["hip_clip"], 2),
        "norm_gb_per_s": gbs(4, t["hip_norm"]), "perturb_gb_per_s": gbs(16, t["hip_perturb"]),
        "restore_gb_per_s": gbs(8, t["restore"]), "clip_gb_per_s": gbs(8, t["hip_clip"]),
        "norm_rel_diff_to_torch": norm_diff, "perturbed_max_abs_diff_to_torch": w_diff, "rounds": rounds, "reps": reps}),
        flush=True)


def bench_step(kind, step_batch, rounds, reps, rho=0.05, max_norm=1.0):
    import torch
    from lidog_amd import synth
    from lidog_amd.train import build_model, build_step
    batch = synth.make_batch(range(step_batch), "kitti120k", "cuda")
    torch.manual_seed(0)
    first = build_model(kind, 50.0, device="cuda")
    state = {k: v.clone() for k, v in first.state_dict().items()}
    steps, fns = {}, {}
    for name, kw in (("plain", {}), ("clip", dict(grad_clip_norm=max_norm)), ("sam", dict(sam_rho=rho))):
        model = first if name == "plain" else build_model(kind, 50.0, device="cuda")
        model.load_state_dict(state)
        model, step, _ = build_step(model, kind, optimizer="Adam", lr=1e-3, **kw)
        steps[name] = step
        fns[name] = lambda s=step: s.training_step(batch)
    for f in fns.values():           # the first steps record the trace of map uses and fill the allocator
        for _ in range(3):
            f()
    t = _alternate(fns, rounds, reps)
    print(json.dumps({"bench": "sam", "case": f"step_{kind}", "batch": step_batch,
                      "rows": int(batch["coords_int"].shape[0]), **{f"{k}_ms": round(v, 3) for k, v in t.items()},
                      "clip_over_plain": round(t["clip"] / t["plain"], 4), "sam_over_plain": round(t["sam"] / t["plain"], 4),
                      "grad_norm": float(steps["clip"].opt.sqnorm.sqrt()), "sam_rho": rho, "grad_clip_norm": max_norm,
                      "paths": {k: s.last_path for k, s in steps.items()}, "rounds": rounds, "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--step-batch", type=int, default=4, help="0: skip the step comparison")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sam: no GPU (nothing here can be measured without one)")
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    bench_kernels(a.rounds, a.reps)
    if a.step_batch:
        for kind in ("MinkUNet34", "MinkUNet34BEV"):
            bench_step(kind, a.step_batch, a.rounds, a.step_reps)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
