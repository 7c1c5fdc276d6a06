"""bf16 inference (lidog_amd/precision.py, csrc/sconv_bf16.hip) against the fp32 path, on the same box, alternating:

  (a) kernels: device time (HIP events around --reps launches, median over --rounds, fp32 and bf16 taking turns) of
      lidog_sconv_gemm vs lidog_sconv_gemm_bf16 and of lidog_sconv_os_bn vs lidog_sconv_os_bn_bf16 on the kernel maps of
      the bench batch (kitti120k, --kernel-batch scans) at the layer shapes of MinkUNet34, random operands; with the
      bytes each launch has to move (gathered rows in, weights in, rows out) and the rate that makes
  (b) evaluation: scans/s of evaluate.TargetEvaluator at --batch over --batches batches made ahead on the device, both
      precisions alternating round by round, host clock from a synchronised device to the result on the host
  (c) quality: one short synthetic training run (MinkUNet34, source8k), its weights evaluated both ways: mIoU, per-class
      IoU and the share of voxels whose prediction differs

One JSON line per measurement.

    python scripts/bench_bf16.py --rounds 5 --reps 10 --batch 8 --batches 2
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (tensor stride, Cin, Cout) of the 3^3 stride-1 convolutions and (stride in, Cin, Cout) of the k2 s2 ones of MinkUNet34
K3 = [(1, 96, 96), (1, 128, 96), (2, 32, 32), (2, 96, 96), (2, 128, 96), (4, 64, 64), (4, 128, 128), (4, 192, 128),
      (8, 128, 128), (8, 256, 256), (8, 384, 256), (16, 256, 256)]
K2 = [(1, 32, 32), (2, 32, 32), (4, 64, 64), (8, 128, 128)]


def _alternate(fns, rounds, reps):
    """{name: median ms per call}: every round times `reps` launches of each function in turn between HIP events"""
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
    import lidog_amd.me as ME
    from lidog_amd import _lib, synth
    from lidog_amd._lib import call, ptr
    L = _lib.load()
    b = synth.make_batch(range(kernel_batch), "kitti120k", "cuda")
    cm = ME.SparseTensor(coordinates=b["coords_int"], features=b["source_features0"]).coordinate_manager
    prev = 1
    for s in (2, 4, 8, 16):
        cm.stride(prev, s)
        prev = s

    def pack(W):
        K, Cin, Cout = W.shape
        buf = torch.empty(W.numel(), dtype=torch.bfloat16, device="cuda")
        desc = torch.tensor([[0, 0, K, Cin, Cout, 0]], dtype=torch.int64, device="cuda")
        call("lidog_pack_kernels_bf16", ptr(W), ptr(buf), ptr(desc), 1, K * (Cin // 32) * (Cout // 32))
        return buf

    for kind, cases in (("k3s1", K3), ("k2s2", K2)):
        for s, Cin, Cout in cases:
            m = cm.kernel_map(s, s if kind == "k3s1" else 2 * s, 3 if kind == "k3s1" else 2)
            x = torch.randn(m.n_in, Cin, device="cuda")
            W = torch.randn(m.K, Cin, Cout, device="cuda") * 0.1
            Wp = pack(W)
            T = torch.empty(m.P, Cout, device="cuda")
            tiles = (ptr(m.tiles[0]), ptr(m.tiles[1]), ptr(m.tiles[2]), m.n_tiles)
            fns = {"gemm_fp32": lambda: call("lidog_sconv_gemm", ptr(x), ptr(m.pair_in), ptr(W), None, *tiles, Cin, Cout,
                                             ptr(T), None, x.shape[0]),
                   "gemm_bf16": lambda: call("lidog_sconv_gemm_bf16", ptr(x), ptr(m.pair_in), ptr(Wp), None, *tiles, Cin,
                                             Cout, ptr(T), None)}
            # least traffic of a gathered GEMM: every pair's input row in, every product row out (the weights are small)
            moved = 4.0 * m.P * (Cin + Cout)
            if kind == "k3s1":
                n = m.n_out
                pad = (n + 127) // 128 * 128
                perm = torch.empty(pad, dtype=torch.int32, device="cuda")
                wm = torch.empty(pad // 32, dtype=torch.int32, device="cuda")
                order = torch.empty(pad // 128, dtype=torch.int32, device="cuda")
                ws = torch.empty(L.lidog_kernel_map_sorted_ws(n), dtype=torch.uint8, device="cuda")
                call("lidog_kernel_map_sorted", ptr(m.nbr), n, m.K, ptr(m.k_off), ptr(perm), ptr(wm), ptr(order), ptr(ws),
                     ws.numel())
                bn = [torch.randn(Cout, device="cuda") * 0.3, torch.rand(Cout, device="cuda") + 0.5,
                      torch.rand(Cout, device="cuda") + 0.5, torch.randn(Cout, device="cuda") * 0.3]
                res = torch.randn(n, Cout, device="cuda")
                out = torch.empty(n, Cout, device="cuda")
                head = (ptr(x), ptr(m.nbr), n, m.K, ptr(perm), ptr(wm), ptr(order))
                tail = (None, Cin, Cout, *(ptr(v) for v in bn), ptr(res), 1, ptr(out))
                fns["os_bn_fp32"] = lambda: call("lidog_sconv_os_bn", *head, ptr(W), *tail)
                fns["os_bn_bf16"] = lambda: call("lidog_sconv_os_bn_bf16", *head, ptr(Wp), *tail)
            t = _alternate(fns, rounds, reps)
            rec = {"bench": "bf16_kernels", "map": kind, "stride": s, "Cin": Cin, "Cout": Cout, "rows": int(m.n_out),
                   "pairs": int(m.P), "gflop": 2e-9 * m.P * Cin * Cout, "rounds": rounds, "reps": reps}
            for k, v in t.items():
                rec[k + "_ms"] = round(v, 4)
            rec["gemm_fp32_over_bf16"] = round(t["gemm_fp32"] / t["gemm_bf16"], 3)
            rec["gemm_bf16_tflops"] = round(rec["gflop"] / t["gemm_bf16"], 1)
            rec["gemm_bf16_least_gb_per_s"] = round(moved / t["gemm_bf16"] / 1e6, 0)
            if "os_bn_bf16" in t:
                rec["os_bn_fp32_over_bf16"] = round(t["os_bn_fp32"] / t["os_bn_bf16"], 3)
                rec["os_bn_bf16_tflops"] = round(rec["gflop"] / t["os_bn_bf16"], 1)
                # least traffic of the output-stationary form: every pair's input row in (from L2 or HBM), every output
                # row and its residual once
                rec["os_bn_bf16_least_gb_per_s"] = round((4.0 * m.P * Cin + 8.0 * m.n_out * Cout) / t["os_bn_bf16"] / 1e6, 0)
            print(json.dumps(rec), flush=True)


def bench_eval(model, config, batch, n_batches, rounds):
    import torch
    from lidog_amd import evaluate
    from lidog_amd.train import SynthScans
    n = batch * n_batches
    batches = list(evaluate.dataset_batches(SynthScans(n, config, first=10 ** 6), batch))
    evs = {p: evaluate.TargetEvaluator(model, precision=p) for p in ("fp32", "bf16")}
    out = {p: ev.run(batches, n, rows="scan") for p, ev in evs.items()}          # untimed: first use of everything
    rates = {p: [] for p in evs}
    for _ in range(rounds):
        for p, ev in evs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.run(batches, n, rows="scan")
            rates[p].append(n / (time.perf_counter() - t0))
    rec = {"bench": "bf16_eval", "model": type(model).__name__, "config": config, "batch": batch, "scans": n,
           "rounds": rounds, "voxels_per_batch": int(batches[0][0]["coords_int"].shape[0]),
           "note": "a bf16 run includes its one weight pack"}
    for p, r in rates.items():
        rec[f"{p}_scans_per_s_median"] = round(statistics.median(r), 2)
        rec[f"{p}_scans_per_s"] = [round(v, 2) for v in r]
        rec[f"{p}_mean_iou"] = out[p]["mean"]
    rec["bf16_over_fp32"] = round(rec["bf16_scans_per_s_median"] / rec["fp32_scans_per_s_median"], 3)
    return rec


def bench_quality(epochs, scans, val_scans):
    import numpy as np
    import torch
    from lidog_amd import evaluate
    from lidog_amd.train import Fit, SynthScans
    fit = Fit(model_kind="MinkUNet34", batch_size=4, optimizer="Adam", lr=1e-3, epochs=epochs,
              train_data=SynthScans(scans, "source8k"), num_sanity_val_steps=0, log=lambda *_: None)
    hist = fit.run()
    model = fit.model.eval()
    data = SynthScans(val_scans, "source8k", first=10 ** 6)
    res, preds = {}, {}
    for p in ("fp32", "bf16"):
        res[p] = evaluate.TargetEvaluator(model, precision=p).run(evaluate.dataset_batches(data, 8), val_scans, rows="scan")
        run = evaluate.Predictor(model, precision=p)
        preds[p] = torch.cat([run(b["coords_int"], b["source_features0"])[0] for b, _ in evaluate.dataset_batches(data, 8)])
    return {"bench": "bf16_quality", "model": "MinkUNet34", "config": "source8k", "epochs": epochs, "train_scans": scans,
            "val_scans": val_scans, "loss_first": hist[0]["loss"], "loss_last": hist[-1]["loss"],
            "fp32_mean_iou": res["fp32"]["mean"], "bf16_mean_iou": res["bf16"]["mean"],
            "fp32_per_class_iou": [round(float(v), 4) for v in res["fp32"]["per_class"]],
            "bf16_per_class_iou": [round(float(v), 4) for v in res["bf16"]["per_class"]],
            "per_class_abs_diff_max": float(np.nanmax(np.abs(res["fp32"]["per_class"] - res["bf16"]["per_class"]))),
            "voxels": int(preds["fp32"].numel()),
            "predictions_that_differ": float((preds["fp32"] != preds["bf16"]).float().mean())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parts", nargs="+", default=["kernels", "eval", "quality"], choices=["kernels", "eval", "quality"])
    ap.add_argument("--kernel-batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--config", default="kitti120k")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--train-scans", type=int, default=16)
    ap.add_argument("--val-scans", type=int, default=16)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bf16: no GPU (nothing here can be measured without one)")
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    if "kernels" in a.parts:
        bench_kernels(a.kernel_batch, a.rounds, a.reps)
    if "eval" in a.parts:
        from lidog_amd.train import build_model
        model = build_model("MinkUNet34BEV").eval()
        print(json.dumps(bench_eval(model, a.config, a.batch, a.batches, a.rounds)), flush=True)
    if "quality" in a.parts:
        print(json.dumps(bench_quality(a.epochs, a.train_scans, a.val_scans)), flush=True)


if __name__ == "__main__":
    main()
