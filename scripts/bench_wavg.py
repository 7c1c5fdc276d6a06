"""WeightAverage (csrc/wavg.hip) against the torch composition of the same average, on the same box, alternating: device
time between HIP events around --reps calls, median over --rounds, both sides taking turns, on the parameter set of
MinkUNet34BEV (every parameter through the optimiser's flat buffer, every BatchNorm running statistic as a segment).

  update   WeightAverage.update() in ema mode: one launch
           against the reference's MomentumUpdater form over tensor lists, mp = tau * mp + (1 - tau) * op as
           torch._foreach_mul_(avg, tau); torch._foreach_add_(avg, live, alpha=1 - tau) over the parameters and over the
           floating-point buffers (the lists are built before the clock; a per-tensor python loop would cost more)
  swap     applied() entered and left: two SWAP launches and two refreshes of the transposed kernels; `swap_kernels_us`
           is the two SWAP launches alone

Then the step: the MinkUNet34BEV training step of bench.py at --step-batch kitti120k scans without and with
avg.update() behind it (what Fit(weight_average="ema") adds), alternating on two models with the same weights.
One JSON line per case.

    python scripts/bench_wavg.py --rounds 7 --reps 20
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_losses import _alternate  # noqa: E402


def bench_update(rounds, reps, tau=0.996):
    import torch
    from lidog_amd.optim import WAVG_SWAP, FlatAdam, WeightAverage
    from lidog_amd.train import build_model
    model = build_model("MinkUNet34BEV", 50.0, device="cuda").train()
    opt = FlatAdam(model, lr=1e-3)
    avg = WeightAverage(opt, model, "ema", decay=tau)
    avg.update()                                    # the copy
    with torch.no_grad():                           # live weights away from the average, as after some steps
        opt.flat.flat.mul_(1.01)
    live = [p.data for p in opt.flat.params] + [b for _, b in avg._live]
    mine = [t.clone() for t in live]
    views = [avg.params[o:o + p.numel()].view(p.shape) for p, o in zip(opt.flat.params, opt.flat.offsets)]
    torch._foreach_copy_(mine, views + list(avg._buffer_views))

    def composition():
        torch._foreach_mul_(mine, tau)
        torch._foreach_add_(mine, live, alpha=1.0 - tau)

    avg.update()
    composition()
    got = torch.cat([avg.params] + [v.reshape(-1) for v in avg._buffer_views])
    want = torch.cat([t.reshape(-1) for t in mine])
    diff = float((got - want).abs().max())
    scale = float(want.abs().max())

    def swap_pair():
        with avg.applied():
            pass

    def swap_kernels():
        avg._launch(WAVG_SWAP)
        avg._launch(WAVG_SWAP)

    t = _alternate({"hip": avg.update, "torch": composition, "swap": swap_pair, "swap_kernels": swap_kernels}, rounds, reps)
    elems = opt.flat.total + sum(b.numel() for _, b in avg._live)
    print(json.dumps({
        "bench": "wavg", "case": "update_MinkUNet34BEV", "elements": elems, "segments": avg.n_segs,
        "workgroups": avg.n_blocks, "tensors": len(live), "hip_us": round(1e3 * t["hip"], 2),
        "torch_us": round(1e3 * t["torch"], 2), "torch_over_hip": round(t["torch"] / t["hip"], 2),
        "hip_gb_per_s": round(12 * elems / (1e6 * t["hip"]), 1), "swap_pair_us": round(1e3 * t["swap"], 2),
        "swap_kernels_us": round(1e3 * t["swap_kernels"], 2),
        "swap_gb_per_s": round(2 * 16 * elems / (1e6 * t["swap_kernels"]), 1), "max_abs_diff_to_torch": diff,
        "max_abs_value": scale, "rounds": rounds, "reps": reps}), flush=True)


def bench_step(step_batch, rounds, reps):
    import torch
    from lidog_amd import synth
    from lidog_amd.optim import WeightAverage
    from lidog_amd.train import build_model, build_step
    batch = synth.make_batch(range(step_batch), "kitti120k", "cuda")
    torch.manual_seed(0)
    first = build_model("MinkUNet34BEV", 50.0, device="cuda")
    state = {k: v.clone() for k, v in first.state_dict().items()}
    steps, fns = {}, {}
    for name in ("plain", "ema"):
        model = first if name == "plain" else build_model("MinkUNet34BEV", 50.0, device="cuda")
        model.load_state_dict(state)
        model, step, _ = build_step(model, "MinkUNet34BEV", optimizer="Adam", lr=1e-3)
        steps[name] = step
        if name == "plain":
            fns[name] = lambda s=step: s.training_step(batch)
        else:
            avg = WeightAverage(step.opt, model, "ema")
            fns[name] = lambda s=step, a=avg: (s.training_step(batch), a.update())
    for f in fns.values():           # the first steps record the trace of map uses and fill the allocator
        for _ in range(3):
            f()
    t = _alternate(fns, rounds, reps)
    print(json.dumps({"bench": "wavg", "case": "step_MinkUNet34BEV", "batch": step_batch,
                      "rows": int(batch["coords_int"].shape[0]), "plain_ms": round(t["plain"], 3),
                      "ema_ms": round(t["ema"], 3), "ema_over_plain": round(t["ema"] / t["plain"], 4),
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
        raise SystemExit("bench_wavg: no GPU (nothing here can be measured without one)")
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    bench_update(a.rounds, a.reps)
    if a.step_batch:
        bench_step(a.step_batch, a.rounds, a.step_reps)


if __name__ == "__main__":
    main()
