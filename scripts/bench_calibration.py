"""Calibration (lidog_amd.calibration, csrc/calib.hip), measured on one box with both sides alternating in one process and
HIP events around every timed window:

  table   CalibrationTable.add (one launch of lidog_calib_stats) against a torch composition of the same table
          (softmax -> max -> bucketize -> bincount / index_add_, NLL by log_softmax + gather, Brier by one_hot) at
          355 902 x 7 and 111 556 x 7 random N(0, 3^2) logits, 15 bins; also the same launch over 256 rows, which is
          what a launch costs when it has next to nothing to do; --reps calls per window, median over --rounds
  fit     fit_temperature (24 launches of lidog_calib_fit_step, the temperature read at the end) against torch's usual
          fit: LBFGS on log T over cross_entropy(logits / T) (lr 0.1, max_iter 50), on the same logits with labels drawn
          from softmax(logits / 3); both temperatures are printed
  eval    TargetEvaluator scans/s on --scans kitti120k scans at --batch per batch without and with
          calibration=[raw, scaled], taking turns, median over --eval-rounds

Least traffic of lidog_calib_stats: the logits and the labels once (n C 4 + n 8 bytes).  One JSON line per case.

    python scripts/bench_calibration.py --rounds 7 --reps 50
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((355902, 7), (111556, 7))
BINS = 15


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


def _labels(x, scale, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.multinomial(torch.softmax(x / scale, dim=1), 1, generator=g).view(-1)


def torch_table(x, labels, bins=BINS):
    """(table [B, 3] float64: count, correct, confidence sum; rows, brier sum, nll sum) by torch operators"""
    import torch
    logp = torch.log_softmax(x.double(), dim=1)
    p = logp.exp()
    conf, pred = p.max(dim=1)
    edges = torch.arange(1, bins, device=x.device, dtype=torch.float64) / bins
    b = torch.bucketize(conf, edges, right=True)
    table = torch.zeros((bins, 3), dtype=torch.float64, device=x.device)
    table[:, 0] = torch.bincount(b, minlength=bins).double()
    table[:, 1].index_add_(0, b, (pred == labels).double())
    table[:, 2].index_add_(0, b, conf)
    nll = -logp.gather(1, labels.view(-1, 1)).sum()
    brier = ((p - torch.nn.functional.one_hot(labels, x.shape[1]).double()) ** 2).sum()
    return table, x.shape[0], brier, nll


def bench_table(rounds, reps):
    import torch
    from lidog_amd.calibration import CalibrationTable
    small = torch.randn(256, 7, device="cuda") * 3
    small_l = _labels(small, 1.0, 1)
    for n, C in SHAPES:
        x = torch.randn(n, C, device="cuda") * 3
        labels = _labels(x, 1.0, 2)
        table, tiny = CalibrationTable(BINS), CalibrationTable(BINS)
        t = _alternate({"hip": lambda: table.add(x, labels), "torch": lambda: torch_table(x, labels),
                        "hip_256_rows": lambda: tiny.add(small, small_l)}, rounds, reps)
        once = CalibrationTable(BINS).add(x, labels).result()
        tt, rows, brier, nll = torch_table(x, labels)
        least = n * C * 4 + n * 8
        print(json.dumps({
            "bench": "calibration", "case": "table", "n": n, "C": C, "bins": BINS, "least_mb": round(least / 1e6, 2),
            "hip_us": round(1e3 * t["hip"], 2), "torch_us": round(1e3 * t["torch"], 2),
            "torch_over_hip": round(t["torch"] / t["hip"], 2), "hip_256_rows_us": round(1e3 * t["hip_256_rows"], 2),
            "hip_least_tb_per_s": round(least / t["hip"] / 1e9, 3),
            "counts_equal": bool((tt[:, 0].cpu().numpy() == once["reliability"][:, 1]).all()),
            "ece_hip": once["ece"], "nll_hip": once["nll"], "nll_torch": float(nll) / rows,
            "brier_hip": once["brier"], "brier_torch": float(brier) / rows, "rounds": rounds, "reps": reps}), flush=True)


def torch_fit(x, labels):
    """the usual temperature fit: LBFGS on log T"""
    import torch
    log_t = torch.zeros(1, device=x.device, requires_grad=True)
    opt = torch.optim.LBFGS([log_t], lr=0.1, max_iter=50)

    def closure():
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(x / log_t.exp(), labels)
        loss.backward()
        return loss
    opt.step(closure)
    return float(log_t.detach().exp())


def bench_fit(rounds, reps):
    import torch
    from lidog_amd.calibration import fit_temperature
    for n, C in SHAPES:
        x = torch.randn(n, C, device="cuda") * 3
        labels = _labels(x, 3.0, 3)                              # the logits are three times too sharp: T near 3
        res = {}

        def hip():
            res["hip"] = fit_temperature(x, labels).temperature()          # the read is part of it, as torch's float()

        def ref():
            res["torch"] = torch_fit(x, labels)
        t = _alternate({"hip": hip, "torch": ref}, rounds, max(1, reps // 10))
        print(json.dumps({
            "bench": "calibration", "case": "fit", "n": n, "C": C, "iters": 24, "hip_ms": round(t["hip"], 3),
            "torch_lbfgs_ms": round(t["torch"], 3), "torch_over_hip": round(t["torch"] / t["hip"], 2),
            "hip_us_per_launch": round(1e3 * t["hip"] / 24, 2), "T_hip": res["hip"], "T_torch": res["torch"],
            "rounds": rounds, "reps": max(1, reps // 10)}), flush=True)


def bench_eval(kind, scans, batch, rounds):
    import torch
    from lidog_amd import evaluate
    from lidog_amd.train import SynthScans, build_model
    data = SynthScans(scans, "kitti120k", first=10 ** 6)
    batches = list(evaluate.dataset_batches(data, batch))       # on the device before the clock, for both sides alike
    torch.manual_seed(0)
    model = build_model(kind, 50.0, device="cuda").eval()
    ev = evaluate.TargetEvaluator(model)
    beta = torch.tensor([0.5], dtype=torch.float64, device="cuda")
    runs = {"plain": lambda: ev.run(batches, scans),
            "calibration": lambda: ev.run(batches, scans, calibration=[("raw", None), ("scaled", beta)])}
    out = {k: f() for k, f in runs.items()}                      # first use: traces, allocator, every kernel
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
        "bench": "calibration", "case": "eval", "model": kind, "config": "kitti120k", "scans": scans, "batch": batch,
        "rows": int(sum(b["coords_int"].shape[0] for b, _ in batches)),
        "scans_per_s": {k: round(scans / v, 2) for k, v in med.items()},
        "calibration_over_plain": round(med["calibration"] / med["plain"], 4),
        "counts_equal": bool((out["plain"]["counts"] == out["calibration"]["counts"]).all()),
        "ece_random_weights": out["calibration"]["calibration"]["raw"]["ece"], "rounds": rounds}), flush=True)


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
        raise SystemExit("bench_calibration: no GPU (nothing here can be measured without one)")
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    bench_table(a.rounds, a.reps)
    bench_fit(a.rounds, a.reps)
    if a.scans:
        bench_eval(a.model, a.scans, a.batch, a.eval_rounds)


if __name__ == "__main__":
    main()
