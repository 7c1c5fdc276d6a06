"""CELoss / FocalLoss (csrc/losses.hip) against torch's cross-entropy, on the same box, alternating: device time (HIP
events around --reps forward + backward passes, median over --rounds, both sides taking turns) at the two shapes of the
LiDOG step at --kernel-batch kitti120k scans:

  sem   the semantic logits [n, 7] with the scans' own labels
  bev   the BEV logits [B, 7, 167, 167] read through .view(-1, 7) with rasterised labels (mostly ignored)

The torch side is torch.nn.functional.cross_entropy(ignore_index=-1) on the device (log_softmax, nll_loss and their
backward kernels) and, for the focal loss, the reference's formula on top of it (utils/losses/losses.py:432-436); the
reference's own `.cpu()` round trip is not included.  Both sides go through autograd: forward, then backward into a fresh
gradient.

`hip_kernels_us` is the three launches alone (lidog_ce_fwd's two and lidog_ce_bwd's one through the C entries, buffers
allocated before the clock): what is left of `hip_us` beyond it is autograd and the four allocations of a call.

Reported per case: microseconds per forward + backward on both sides, the kernels' LEAST traffic (forward: the logits and
the labels read once, n C 4 + n 8 bytes; backward: the same plus the gradient written, n C 4) and the TB/s that time
gives it.  Then the step: the MinkUNet34BEV training step at --step-batch scans with the default criteria (SoftDICELoss /
DICELoss) and with CELoss on both, alternating on two models with the same weights.  One JSON line per case.

    python scripts/bench_losses.py --rounds 7 --reps 50
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _alternate(fns, rounds, reps):
    """{name: median ms per call}: every round times `reps` calls of each function in turn between HIP events"""
    import torch
    for f in fns.values():           # first use of every kernel
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            e.record()
            e.synchronize()
            ms[k].append(a.elapsed_time(e) / reps)
    return {k: statistics.median(v) for k, v in ms.items()}


def bench_kernels(kernel_batch, rounds, reps):
    import torch
    import torch.nn.functional as F
    from lidog_amd import data, synth
    from lidog_amd._lib import call, load, ptr
    from lidog_amd.losses import CELoss, FocalLoss
    b = synth.make_batch(range(kernel_batch), "kitti120k", "cuda")
    labels = b["source_sem_labels0"].long()
    bev, _ = data.bev_labels(b["coords_int"], labels, bound=50.0, img_size=167, batch_size=kernel_batch)
    shapes = {"sem": (torch.randn(labels.shape[0], 7, device="cuda") * 3, labels),
              "bev": ((torch.randn(kernel_batch, 7, 167, 167, device="cuda") * 3).view(-1, 7), bev.view(-1))}
    for shape, (x, y) in shapes.items():
        n, C = x.shape
        scored = int((y != -1).sum())
        x = x.clone().requires_grad_(True)

        def run(loss_of):
            def f():
                x.grad = None
                loss = loss_of()
                loss.backward()
                return loss
            return f

        def torch_focal():
            ce_t = F.cross_entropy(x, y, ignore_index=-1)
            return (1 - torch.exp(-ce_t)) ** 2 * 0.25 * ce_t

        ws = torch.empty(load().lidog_ce_ws(C), dtype=torch.float64, device="cuda")
        out, coef, go = torch.empty((), device="cuda"), torch.empty(1, device="cuda"), torch.ones((), device="cuda")
        g, xd = torch.empty(n, C, device="cuda"), x.detach()

        def kernels(is_focal):
            def f():
                call("lidog_ce_fwd", ptr(xd), ptr(y), n, C, -1, 1, None, is_focal, 0.25, 2.0, ptr(ws), ptr(out), ptr(coef))
                call("lidog_ce_bwd", ptr(xd), ptr(y), n, C, -1, 1, None, ptr(coef), ptr(go), ptr(g))
            return f

        ce, focal = CELoss(ignore_label=-1), FocalLoss(alpha=0.25, gamma=2)
        cases = {"ce": (run(lambda: ce(x, y)), run(lambda: F.cross_entropy(x, y, ignore_index=-1))),
                 "focal": (run(lambda: focal(x, y)), run(torch_focal))}
        for what, (hip, ref) in cases.items():
            lh = float(hip().detach())
            gh = x.grad.clone()
            lt = float(ref().detach())
            diff = float((gh - x.grad).abs().max())
            t = _alternate({"hip": hip, "torch": ref, "kernels": kernels(int(what == "focal"))}, rounds, reps)
            least = n * C * 4 + n * 8 + (n * C * 4 + n * 8 + n * C * 4)
            print(json.dumps({
                "bench": "losses", "case": f"{shape}_{what}", "n": n, "C": C, "scored_rows": scored,
                "least_mb": round(least / 1e6, 2), "hip_us": round(1e3 * t["hip"], 2),
                "torch_us": round(1e3 * t["torch"], 2), "torch_over_hip": round(t["torch"] / t["hip"], 2),
                "hip_kernels_us": round(1e3 * t["kernels"], 2),
                "hip_kernels_least_tb_per_s": round(least / t["kernels"] / 1e9, 3),
                "hip_least_tb_per_s": round(least / t["hip"] / 1e9, 3),
                "torch_least_tb_per_s": round(least / t["torch"] / 1e9, 3), "loss_hip": lh, "loss_torch": lt,
                "max_abs_grad_diff": diff, "rounds": rounds, "reps": reps}), flush=True)


def bench_step(step_batch, rounds, reps):
    import torch
    from lidog_amd import synth
    from lidog_amd.train import build_model, build_step
    batch = synth.make_batch(range(step_batch), "kitti120k", "cuda")
    torch.manual_seed(0)
    first = build_model("MinkUNet34BEV", 50.0, device="cuda")
    state = {k: v.clone() for k, v in first.state_dict().items()}
    steps = {}
    for name, kw in (("default", {}), ("celoss", dict(sem_criterion="CELoss", sem_bev_criterion="CELoss"))):
        model = first if name == "default" else build_model("MinkUNet34BEV", 50.0, device="cuda")
        model.load_state_dict(state)
        steps[name] = build_step(model, "MinkUNet34BEV", **kw)[1]
    fns = {k: (lambda s=s: s.training_step(batch)) for k, s in steps.items()}
    for f in fns.values():           # the first steps record the trace of map uses and fill the allocator
        for _ in range(3):
            f()
    t = _alternate(fns, rounds, reps)
    print(json.dumps({"bench": "losses", "case": "step_MinkUNet34BEV", "batch": step_batch,
                      "rows": int(batch["coords_int"].shape[0]), "default_ms": round(t["default"], 3),
                      "celoss_ms": round(t["celoss"], 3), "celoss_over_default": round(t["celoss"] / t["default"], 4),
                      "paths": {k: s.last_path for k, s in steps.items()}, "rounds": rounds, "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kernel-batch", type=int, default=4)
    ap.add_argument("--step-batch", type=int, default=4, help="0: skip the step comparison")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step-reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_losses: no GPU (nothing here can be measured without one)")
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    bench_kernels(a.kernel_batch, a.rounds, a.reps)
    if a.step_batch:
        bench_step(a.step_batch, a.rounds, a.step_reps)


if __name__ == "__main__":
    main()
