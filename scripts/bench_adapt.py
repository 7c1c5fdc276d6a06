"""Test-time adaptation (lidog_amd.adapt, csrc/entropy.hip), measured on one box with both sides alternating in one
process and HIP events around every timed window:

  entropy   lidog_entropy_fwd + lidog_entropy_bwd (through EntropyLoss and autograd, and the three launches alone)
            against the torch composition log_softmax -> exp -> mul -> sum -> mean with autograd, at 355 902 x 7 and
            111 556 x 7 random N(0, 3^2) logits; --reps forward + backward passes per window, median over --rounds
  eval      TargetEvaluator scans/s on --scans kitti120k scans at --batch per batch with no adapter and with the bn, adabn
            (estimate over the same batches included) and tent adapters, every mode on a model of its own with the same
            weights, the modes taking turns, median over --eval-rounds

Least traffic of the entropy kernels: forward reads the logits and writes row_h (n C 4 + n 4 bytes), backward reads the
logits and row_h and writes the gradient (2 n C 4 + n 4).  One JSON line per case.

    python scripts/bench_adapt.py --rounds 7 --reps 50
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((355902, 7), (111556, 7))


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


def bench_entropy(rounds, reps):
    import torch
    from lidog_amd._lib import call, load, ptr
    from lidog_amd.losses import EntropyLoss
    for n, C in SHAPES:
        x = (torch.randn(n, C, device="cuda") * 3).requires_grad_(True)
        crit = EntropyLoss()

        def run(loss_of):
            def f():
                x.grad = None
                loss = loss_of()
                loss.backward()
                return loss
            return f

        def torch_entropy():
            logp = torch.log_softmax(x, dim=1)
            return -(logp.exp() * logp).sum(dim=1).mean()

        xd = x.detach()
        ws = torch.empty(load().lidog_entropy_ws(C), dtype=torch.float64, device="cuda")
        out, coef, go = torch.empty((), device="cuda"), torch.empty(2, device="cuda"), torch.ones((), device="cuda")
        row_h, g = torch.empty(n, device="cuda"), torch.empty(n, C, device="cuda")

        def kernels():
            call("lidog_entropy_fwd", ptr(xd), None, n, C, 0.0, ptr(ws), ptr(out), ptr(coef), ptr(row_h))
            call("lidog_entropy_bwd", ptr(xd), None, ptr(row_h), n, C, 0.0, ptr(coef), ptr(go), ptr(g))

        hip, ref = run(lambda: crit(x)), run(torch_entropy)
        lh = float(hip().detach())
        gh = x.grad.clone()
        lt = float(ref().detach())
        diff = float((gh - x.grad).abs().max())
        t = _alternate({"hip": hip, "torch": ref, "kernels": kernels}, rounds, reps)
        least = (n * C * 4 + n * 4) + (2 * n * C * 4 + n * 4)
        print(json.dumps({
            "bench": "adapt", "case": "entropy", "n": n, "C": C, "least_mb": round(least / 1e6, 2),
            "hip_us": round(1e3 * t["hip"], 2), "torch_us": round(1e3 * t["torch"], 2),
            "torch_over_hip": round(t["torch"] / t["hip"], 2), "hip_kernels_us": round(1e3 * t["kernels"], 2),
            "hip_kernels_least_tb_per_s": round(least / t["kernels"] / 1e9, 3), "loss_hip": lh, "loss_torch": lt,
            "max_abs_grad_diff": diff, "rounds": rounds, "reps": reps}), flush=True)


def bench_eval(kind, scans, batch, rounds):
    import torch
    from lidog_amd import adapt, evaluate
    from lidog_amd.train import SynthScans, build_model
    data = SynthScans(scans, "kitti120k", first=10 ** 6)
    batches = list(evaluate.dataset_batches(data, batch))       # on the device before the clock, for every mode alike
    torch.manual_seed(0)
    first = build_model(kind, 50.0, device="cuda").eval()
    state = {k: v.clone() for k, v in first.state_dict().items()}
    runs = {}
    for mode in ("none",) + adapt.MODES:
        model = first if mode == "none" else build_model(kind, 50.0, device="cuda").eval()
        model.load_state_dict(state)
        adapter = None if mode == "none" else adapt.TestTimeAdapter(model, mode)
        ev = evaluate.TargetEvaluator(model, adapter=adapter)

        def f(ev=ev, adapter=adapter, mode=mode):
            if adapter is not None:
                adapter.reset()
            if mode == "adabn":
                adapter.estimate(batches)
            return ev.run(batches, scans)                        # ends with the host copy of the counts
        runs[mode] = f
    means = {k: f()["mean"] for k, f in runs.items()}            # first use: traces, allocator, every kernel
    sec = {k: [] for k in runs}
    for _ in range(rounds):
        for k, f in runs.items():
            torch.cuda.synchronize()
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            e.record()
            e.synchronize()
            sec[k].append(a.elapsed_time(e) / 1e3)
    med = {k: statistics.median(v) for k, v in sec.items()}
    print(json.dumps({
        "bench": "adapt", "case": "eval", "model": kind, "config": "kitti120k", "scans": scans, "batch": batch,
        "rows": int(sum(b["coords_int"].shape[0] for b, _ in batches)),
        "scans_per_s": {k: round(scans / v, 2) for k, v in med.items()},
        "over_none": {k: round(v / med["none"], 3) for k, v in med.items()},
        "mean_iou_random_weights": {k: round(v, 3) for k, v in means.items()}, "rounds": rounds}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--model", default="MinkUNet34")
    ap.add_argument("--scans", type=int, default=16, help="0: skip the evaluation comparison")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--eval-rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_adapt: no GPU (nothing here can be measured without one)")
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    bench_entropy(a.rounds, a.reps)
    if a.scans:
        bench_eval(a.model, a.scans, a.batch, a.eval_rounds)


if __name__ == "__main__":
    main()
