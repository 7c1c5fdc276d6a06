"""Sparse pooling (csrc/pool.hip) against the torch formulation of the same operator, on the same box, alternating:
device time (HIP events around --reps launches, median over --rounds, both sides taking turns) on the kernel maps of
--kernel-batch kitti120k scans:

  k2 s2 on the stride-1 map (C = 32) and k3 s1 on the stride-2 map (C = 96): max and avg pooling, forward and backward
  global max over the stride-16 map (C = 256)

The torch side is index_select over the rule book's pairs followed by index_add_ (sum / avg) or
scatter_reduce_(amax) (max): it gathers P x C floats into a temporary and scatters them with atomics (its max returns no
argmax; its max-backward is written here as a mask of the equal entries, which hands a tied window's gradient to every
tie).  Every index tensor it needs (int64 pairs, the expanded scatter index, the counts) is built before the clock.

Reported per case: microseconds per call on both sides and TB/s of LEAST traffic = every pair's row read once and every
result row written once, 4 (P + rows) C bytes (the lists, the argmax and any re-read are not counted).  One JSON line per
case.

    python scripts/bench_pool.py --rounds 7 --reps 50
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LOCAL = [("k2s2", 1, 2, 2, 32), ("k3s1", 2, 2, 3, 96)]       # name, stride in, stride out, kernel size, channels
GLOBAL = (16, 256)                                          # tensor stride, channels


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


def _record(case, C, rows, pairs, t, rounds, reps, diff):
    least = 4.0 * (pairs + rows) * C
    rec = {"bench": "pool", "case": case, "C": C, "result_rows": int(rows), "pairs": int(pairs),
           "least_mb": round(least / 1e6, 2), "hip_us": round(1e3 * t["hip"], 2), "torch_us": round(1e3 * t["torch"], 2),
           "torch_over_hip": round(t["torch"] / t["hip"], 2), "hip_least_tb_per_s": round(least / t["hip"] / 1e9, 3),
           "torch_least_tb_per_s": round(least / t["torch"] / 1e9, 3), "max_abs_diff": diff, "rounds": rounds,
           "reps": reps}
    print(json.dumps(rec), flush=True)


def bench(kernel_batch, rounds, reps):
    import torch
    import lidog_amd.me as ME
    from lidog_amd import _lib, synth
    from lidog_amd._lib import call, ptr
    b = synth.make_batch(range(kernel_batch), "kitti120k", "cuda")
    cm = ME.SparseTensor(coordinates=b["coords_int"], features=b["source_features0"]).coordinate_manager
    prev = 1
    for s in (2, 4, 8, 16):
        cm.stride(prev, s)
        prev = s
    ninf = float("-inf")
    for name, s_in, s_out, ks, C in LOCAL:
        m = cm.kernel_map(s_in, s_out, ks)
        out_lists, in_lists = ME._pool_side(m, "out"), ME._pool_side(m, "in")
        pin, pout = m.pair_in.long(), m.pair_out.long()
        pout_c = pout.unsqueeze(1).expand(-1, C).contiguous()
        cnt = (out_lists[0][1:] - out_lists[0][:-1]).float().clamp(min=1).unsqueeze(1)
        x = torch.randn(m.n_in, C, device="cuda")
        gy = torch.randn(m.n_out, C, device="cuda")
        y = torch.empty(m.n_out, C, device="cuda")
        arg = torch.empty(m.n_out, C, dtype=torch.int32, device="cuda")
        gx = torch.empty(m.n_in, C, device="cuda")

        def hip_rows(src, lists, dst, avg, counts=None):
            call("lidog_pool_rows", ptr(src), ptr(lists[0]), ptr(lists[1]), ptr(lists[2]), lists[3], C, avg, ptr(counts),
                 ptr(dst))
            return dst

        def hip_max():
            call("lidog_pool_rows_max", ptr(x), ptr(out_lists[0]), ptr(out_lists[1]), ptr(out_lists[2]), m.n_out, C,
                 ptr(y), ptr(arg))
            return y

        def hip_max_bwd():
            call("lidog_pool_rows_max_bwd", ptr(gy), ptr(arg), ptr(in_lists[0]), ptr(in_lists[1]), ptr(in_lists[2]),
                 m.n_in, C, ptr(gx))
            return gx

        def torch_avg():
            return torch.zeros(m.n_out, C, device="cuda").index_add_(0, pout, x.index_select(0, pin)) / cnt

        def torch_max():
            return torch.full((m.n_out, C), ninf, device="cuda").scatter_reduce_(0, pout_c, x.index_select(0, pin), "amax")

        def torch_avg_bwd():
            return torch.zeros(m.n_in, C, device="cuda").index_add_(0, pin, (gy / cnt).index_select(0, pout))

        ymax = torch_max()

        def torch_max_bwd():
            mask = x.index_select(0, pin) == ymax.index_select(0, pout)
            return torch.zeros(m.n_in, C, device="cuda").index_add_(0, pin, gy.index_select(0, pout) * mask)

        cases = {
            "avg_fwd": (lambda: hip_rows(x, out_lists, y, 1), torch_avg, m.n_out),
            "avg_bwd": (lambda: hip_rows(gy, in_lists, gx, 0, out_lists[0]), torch_avg_bwd, m.n_in),
            "max_fwd": (hip_max, torch_max, m.n_out),
            "max_bwd": (hip_max_bwd, torch_max_bwd, m.n_in),
        }
        for what, (hip, ref, rows) in cases.items():
            diff = float((hip().clone() - ref()).abs().max())       # randn operands: no ties, so max-backward agrees too
            t = _alternate({"hip": hip, "torch": ref}, rounds, reps)
            _record(f"{name}_{what}", C, rows, m.P, t, rounds, reps, diff)
    s, C = GLOBAL
    perm, seg_off, bid, B = cm.segments(s)
    n = cm.maps[s].n
    x = torch.randn(n, C, device="cuda")
    y = torch.empty(B, C, device="cuda")
    arg = torch.empty(B, C, dtype=torch.int32, device="cuda")
    nbytes = _lib.load().lidog_pool_global_ws(n, B, C)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    bid_c = bid.long().unsqueeze(1).expand(-1, C).contiguous()

    def hip_global():
        call("lidog_pool_global", ptr(x), n, C, B, ptr(perm), ptr(seg_off), 2, ptr(y), ptr(arg), ptr(ws), nbytes)
        return y

    def torch_global():
        return torch.full((B, C), ninf, device="cuda").scatter_reduce_(0, bid_c, x, "amax")

    diff = float((hip_global().clone() - torch_global()).abs().max())
    t = _alternate({"hip": hip_global, "torch": torch_global}, rounds, reps)
    _record(f"global_max_s{s}", C, B, n, t, rounds, reps, diff)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kernel-batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pool: no GPU (nothing here can be measured without one)")
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    bench(a.kernel_batch, a.rounds, a.reps)


if __name__ == "__main__":
    main()
