"""LovaszSoftmaxLoss (csrc/lovasz.hip) against the torch composition of the same loss, on the same box, alternating:
device time (HIP events around --reps forward + backward passes, median over --rounds, both sides taking turns) at two
row shapes of the step at --kernel-batch kitti120k scans:

  sem   the semantic logits [n, 7] with the scans' own labels (the shape the training steps give the auxiliary criterion)
  bev   the BEV logits [B, 7, 167, 167] read through .view(-1, 7) with rasterised labels (mostly ignored)

The torch side is the published lovasz_softmax_flat(classes='present') on the device: the valid rows selected by a
boolean mask, softmax, and per present class torch.sort(descending=True, stable=True), cumsum and dot, under autograd.
Its mask and its present-class test read the device back, as the published code does; that is part of what it costs.
Both sides go through autograd: forward, then backward into a fresh gradient.

`hip_kernels_us` is the launches alone (lidog_lovasz_fwd and lidog_lovasz_bwd through the C entries, buffers allocated
before the clock): what is left of `hip_us` beyond it is autograd and the allocations of a call.

Then the step: the MinkUNet34 training step at --step-batch scans without and with sem_aux_criterion="LovaszSoftmaxLoss",
alternating on two models with the same weights.  One JSON line per case.

    python scripts/bench_lovasz.py --rounds 7 --reps 20
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_losses import _alternate  # noqa: E402


def torch_lovasz(x, y, ignore=-1):
    """lovasz_softmax_flat(classes='present') of Berman et al. in torch ops, stable sort"""
    import torch
    C = x.shape[1]
    keep = (y != ignore) & (y >= 0) & (y < C)
    probas, labels = torch.softmax(x, 1)[keep], y[keep]
    losses = []
    for c in range(C):
        fg = (labels == c).float()
        if fg.sum() == 0:
            continue
        errors = (fg - probas[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
        fg_sorted = fg[perm]
        gts = fg_sorted.sum()
        jaccard = 1.0 - (gts - fg_sorted.cumsum(0)) / (gts + (1 - fg_sorted).cumsum(0))
        jaccard = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
        losses.append(torch.dot(errors_sorted, jaccard))
    return torch.stack(losses).mean() if losses else x.sum() * 0.0


def bench_kernels(kernel_batch, rounds, reps):
    import torch
    from lidog_amd import data, synth
    from lidog_amd._lib import call, load, ptr
    from lidog_amd.losses import LovaszSoftmaxLoss
    b = synth.make_batch(range(kernel_batch), "kitti120k", "cuda")
    labels = b["source_sem_labels0"].long()
    bev, _ = data.bev_labels(b["coords_int"], labels, bound=50.0, img_size=167, batch_size=kernel_batch)
    shapes = {"sem": (torch.randn(labels.shape[0], 7, device="cuda") * 3, labels),
              "bev": ((torch.randn(kernel_batch, 7, 167, 167, device="cuda") * 3).view(-1, 7), bev.view(-1))}
    crit = LovaszSoftmaxLoss(ignore_label=-1)
    for shape, (x, y) in shapes.items():
        n, C = x.shape
        valid = int(((y != -1) & (y >= 0) & (y < C)).sum())
        x = x.clone().requires_grad_(True)

        def run(loss_of):
            def f():
                x.grad = None
                loss = loss_of()
                loss.backward()
                return loss
            return f

        ws = torch.empty(load().lidog_lovasz_ws(n, C), dtype=torch.uint8, device="cuda")
        out, coef, go = torch.empty((), device="cuda"), torch.empty(n * C + 1, device="cuda"), torch.ones((), device="cuda")
        g, xd = torch.empty(n, C, device="cuda"), x.detach()

        def kernels():
            call("lidog_lovasz_fwd", ptr(xd), ptr(y), n, C, -1, 1, ptr(ws), ptr(out), ptr(coef), None)
            call("lidog_lovasz_bwd", ptr(xd), ptr(y), n, C, -1, 1, ptr(coef), ptr(coef[n * C:]), ptr(go), ptr(g))

        hip, ref = run(lambda: crit(x, y)), run(lambda: torch_lovasz(x, y))
        lh = float(hip().detach())
        gh = x.grad.clone()
        lt = float(ref().detach())
        diff = float((gh - x.grad).abs().max())
        t = _alternate({"hip": hip, "torch": ref, "kernels": kernels}, rounds, reps)
        print(json.dumps({
            "bench": "lovasz", "case": shape, "n": n, "C": C, "valid_rows": valid, "ws_mb": round(ws.numel() / 1e6, 1),
            "hip_us": round(1e3 * t["hip"], 2), "torch_us": round(1e3 * t["torch"], 2),
            "torch_over_hip": round(t["torch"] / t["hip"], 2), "hip_kernels_us": round(1e3 * t["kernels"], 2),
            "loss_hip": lh, "loss_torch": lt, "max_abs_grad_diff": diff, "rounds": rounds, "reps": reps}), flush=True)


def bench_step(step_batch, rounds, reps):
    import torch
    from lidog_amd import synth
    from lidog_amd.train import build_model, build_step
    batch = synth.make_batch(range(step_batch), "kitti120k", "cuda")
    torch.manual_seed(0)
    first = build_model("MinkUNet34", 50.0, device="cuda")
    state = {k: v.clone() for k, v in first.state_dict().items()}
    steps = {}
    for name, kw in (("plain", {}), ("lovasz", dict(sem_aux_criterion="LovaszSoftmaxLoss"))):
        model = first if name == "plain" else build_model("MinkUNet34", 50.0, device="cuda")
        model.load_state_dict(state)
        steps[name] = build_step(model, "MinkUNet34", **kw)[1]
    fns = {k: (lambda s=s: s.training_step(batch)) for k, s in steps.items()}
    for f in fns.values():           # the first steps record the trace of map uses and fill the allocator
        for _ in range(3):
            f()
    t = _alternate(fns, rounds, reps)
    print(json.dumps({"bench": "lovasz", "case": "step_MinkUNet34", "batch": step_batch,
                      "rows": int(batch["coords_int"].shape[0]), "plain_ms": round(t["plain"], 3),
                      "lovasz_ms": round(t["lovasz"], 3), "lovasz_over_plain": round(t["lovasz"] / t["plain"], 4),
                      "paths": {k: s.last_path for k, s in steps.items()}, "rounds": rounds, "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kernel-batch", type=int, default=4)
    ap.add_argument("--step-batch", type=int, default=4, help="0: skip the step comparison")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lovasz: no GPU (nothing here can be measured without one)")
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    bench_kernels(a.kernel_batch, a.rounds, a.reps)
    if a.step_batch:
        bench_step(a.step_batch, a.rounds, a.step_reps)


if __name__ == "__main__":
    main()
