"""The three light kernels between the trunk and the BEV head, each alone, on a bench batch (4 kitti120k scans, C = 96,
pool (5, 3, 1), bound 50 m): device time between HIP events around ONE call, median of --reps calls after --warmup.

  bev_pool_fwd     lidog_bev_pool_fwd, with the row bitmasks the training step asks for (the two memsets included)
  bev_pool_bwd     lidog_bev_pool_bwd on a random gradient image
  gemm_addend      lidog_sconv_gemm_addend, 7 -> 96 in place (addend == T), the classifier's data gradient

Reported per kernel: microseconds, the bytes the kernel has to move at least (the floor's numerator) and the TB/s that
makes of the median.  One JSON line per kernel.

    python scripts/bench_bev_projection.py --reps 20 --warmup 3
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_us(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        e.record()
        e.synchronize()
        us.append(1e3 * a.elapsed_time(e))
    return statistics.median(us), min(us), max(us)


def bench(reps, warmup, batch):
    import torch
    import lidog_amd.me as ME
    from lidog_amd import bev, synth
    from lidog_amd._lib import call, ptr
    b = synth.make_batch(range(batch), "kitti120k", "cuda")
    coords = b["coords_int"]
    n, C, B = coords.shape[0], 96, batch
    pk, ps, pp = 5, 3, 1
    feats = torch.randn(n, C, device="cuda").relu_()
    lx, ly, lo, H = bev._device_luts(50.0, 0.05, feats.device)
    W = H
    Ho = Wo = (H + 2 * pp - pk) // ps + 1
    winner = torch.full((B, H, W), -1, dtype=torch.int32, device="cuda")
    pixel = torch.empty(n, dtype=torch.int32, device="cuda")
    call("lidog_bev_winner", ptr(coords), n, ptr(lx), ptr(ly), lo, lx.shape[0], H, W, ptr(winner), ptr(pixel))
    out = torch.empty((B, C, Ho, Wo), device="cuda")
    arg = torch.empty((B, C, Ho, Wo), dtype=torch.int32, device="cuda")
    act = torch.empty(ME._lib.load().lidog_conv2d_support_ws(B, C, Ho, Wo), dtype=torch.int32, device="cuda")
    gout = torch.randn(B, C, Ho, Wo, device="cuda")
    gfeats = torch.empty(n, C, device="cuda")
    occupied = int((winner >= 0).sum())

    def fwd():
        call("lidog_bev_pool_fwd", ptr(feats), C, ptr(winner), ptr(pixel), n, B, H, W, pk, ps, pp, Ho, Wo, ptr(out),
             ptr(arg), ptr(act))

    def bwd():
        call("lidog_bev_pool_bwd", ptr(gout), ptr(arg), ptr(winner), ptr(pixel), n, C, B, H, W, pk, ps, pp, Ho, Wo,
             ptr(gfeats))

    im = ME._IdentityMap(n, "cuda")
    glog = torch.randn(n, 7, device="cuda")
    Wt = torch.randn(1, 7, C, device="cuda")
    T = torch.randn(n, C, device="cuda")

    def addend():
        call("lidog_sconv_gemm_addend", ptr(glog), None, ptr(Wt), ptr(im.tiles[0]), ptr(im.tiles[1]), ptr(im.tiles[2]),
             im.n_tiles, 7, C, ptr(T), ptr(T), None)

    fwd()
    # windows the forward kernel computes: argsrc is filled with -1 only without row bitmasks, so count them in a run
    # without
    call("lidog_bev_pool_fwd", ptr(feats), C, ptr(winner), ptr(pixel), n, B, H, W, pk, ps, pp, Ho, Wo, ptr(out), ptr(arg),
         None)
    nonzero = int((out != 0).sum())
    fwd()
    cases = {
        # the image is cleared (4 B a cell) and the occupied pixels' cells are read once; the windows written are extra
        "bev_pool_fwd": (fwd, 4.0 * out.numel() + 4.0 * occupied * C),
        # every gradient cell written once; per cell one (argsrc, gout) pair at the least
        "bev_pool_bwd": (bwd, 4.0 * n * C + 8.0 * occupied * C),
        # T read and written, the 7 inputs of every row read
        "gemm_addend": (addend, 4.0 * n * (7 + 2 * C)),
    }
    for name, (fn, least) in cases.items():
        med, lo_us, hi_us = _median_us(fn, reps, warmup)
        print(json.dumps({"bench": "bev_projection", "kernel": name, "rows": n, "occupied_pixels": occupied,
                          "nonzero_cells": nonzero, "C": C, "median_us": round(med, 1), "min_us": round(lo_us, 1),
                          "max_us": round(hi_us, 1), "least_mb": round(least / 1e6, 1),
                          "least_tb_per_s": round(least / med / 1e6, 3), "reps": reps, "warmup": warmup}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bev_projection: no GPU (nothing here can be measured without one)")
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    bench(a.reps, a.warmup, a.batch)


if __name__ == "__main__":
    main()
