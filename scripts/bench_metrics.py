"""Cost of the per-step training metrics on the same box, in one process:

  (a) device time of lidog_train_confusion alone at the bench batch (kitti120k, --batch scans: one point segment + one
      167 x 167 BEV level), between HIP events, median over --reps; the bytes it reads (36 per row: 7 floats + an int64
      label) over that time.
  (b) the MinkUNet34BEV training step as bench.py runs it (two resident batches cycled, the next batch's maps prefetched),
      with metrics off, with log_every_n_steps = 1 (the worst case: every step records, flushes and reads the flush
      before) and with every step recorded into a ring of 50 slots (what a logged step of the reference's setting
      costs: a flush every 50th record), alternating blocks of --steps steps queued back to back, each block between two device synchronisations
      with the host clock; the step time of every block, the median over the blocks of a kind, and the off blocks' own
      spread (max - min), which is the margin an "on" figure has to be read against.

One JSON line per measurement.

    python scripts/bench_metrics.py --batch 4 --steps 20 --blocks 4 --reps 30
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench_kernel(config, batch, reps, bev=167, c=7):
    import torch
    from lidog_amd import metrics, synth
    b = synth.make_batch(range(batch), config, "cuda")
    labels = b["source_sem_labels0"].long()
    logits = torch.randn((labels.shape[0], c), device="cuda")
    bev_labels = b["source_bev_labels0"]["block8"].long()
    bev_logits = torch.randn((batch, c, bev, bev), device="cuda")
    pairs = [(logits, labels), (bev_logits, bev_labels)]
    counts = torch.zeros((2, c + 1, c), dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    ms = []
    for r in range(reps + 3):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        metrics.train_confusion(pairs, c, out=counts, err=err)
        e.record()
        e.synchronize()
        if r >= 3:
            ms.append(a.elapsed_time(e))
    metrics.check_label_error(err)
    rows = int(labels.numel() + bev_labels.numel())
    us = statistics.median(ms) * 1e3
    return {"bench": "lidog_train_confusion", "config": config, "batch": batch, "rows": rows,
            "point_rows": int(labels.numel()), "bev_rows": int(bev_labels.numel()), "bytes_read": rows * (4 * c + 8),
            "reps": reps, "device_us_median": us, "device_us_min": min(ms) * 1e3,
            "read_GB_per_s_at_median": rows * (4 * c + 8) / (us * 1e-6) / 1e9,
            "note": "HIP events around the call: the host side of the launch included"}


def bench_step(config, batch, steps, blocks, warmup):
    import torch
    from lidog_amd import synth
    from lidog_amd.metrics import MetricLayout, StepMetrics
    from lidog_amd.train import build_model, build_step
    torch.manual_seed(1234)
    model, step, _ = build_step(build_model("MinkUNet34BEV", bound_2d=50.0), "MinkUNet34BEV", optimizer="Adam", lr=1e-3,
                                weight_decay=1e-4, source_weights=(0.5, 0.5))
    batches = [synth.make_batch(range(i * batch, (i + 1) * batch), config, "cuda") for i in range(2)]
    sm = StepMetrics(MetricLayout.for_step(step, [config], levels=("block8",)), log_every_n_steps=1)
    # where the host's time goes in a logged step: inside record() as a whole, and of that inside the wait for the
    # previous flush's event
    host = {"record": [], "wait": []}
    record, harvest = sm.record, sm._harvest

    def timed_record(*a, **kw):
        t0 = time.perf_counter()
        record(*a, **kw)
        host["record"].append((time.perf_counter() - t0) * 1e3)

    def timed_harvest(pending):
        if pending is not None:
            t0 = time.perf_counter()
            pending[-1].synchronize()
            host["wait"].append((time.perf_counter() - t0) * 1e3)
        harvest(pending)

    sm.record, sm._harvest = timed_record, timed_harvest
    ready = torch.cuda.Event()
    ready.record()
    torch.cuda.synchronize()
    n = 0

    ring50 = StepMetrics(sm.layout, log_every_n_steps=50)
    kinds = {"off": None, "on": sm, "ring50": ring50}

    def block(kind, k):
        """k steps back to back, one synchronisation at the end: what a training run does"""
        nonlocal n
        step.metrics = kinds[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            step.training_step(batches[n % 2], prefetch=batches[(n + 1) % 2], prefetch_ready=ready)
            n += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k

    for kind in kinds:
        block(kind, warmup)
    host["record"].clear()
    host["wait"].clear()
    res = {kind: [] for kind in kinds}
    for _ in range(blocks):
        for kind in kinds:
            res[kind].append(block(kind, steps))
    records = len(sm.finish())
    ring50.finish()
    step.metrics = None
    out = {"bench": "step_with_metrics", "model": "MinkUNet34BEV", "config": config, "batch": batch, "steps": steps,
           "blocks": blocks, "log_every_n_steps": 1, "records": records,
           "voxels_per_batch": int(batches[0]["coords_int"].shape[0])}
    for kind, r in res.items():
        out[f"{kind}_ms_per_step_blocks"] = [round(x, 4) for x in r]
        out[f"{kind}_ms_per_step_median"] = statistics.median(r)
    out["host_ms_in_record_median"] = statistics.median(host["record"])
    out["host_ms_waiting_for_previous_flush_median"] = statistics.median(host["wait"])
    out["off_spread_ms"] = max(res["off"]) - min(res["off"])
    out["on_minus_off_ms"] = out["on_ms_per_step_median"] - out["off_ms_per_step_median"]
    out["ring50_minus_off_ms"] = out["ring50_ms_per_step_median"] - out["off_ms_per_step_median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="kitti120k")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    print(json.dumps(bench_kernel(a.config, a.batch, a.reps)), flush=True)
    print(json.dumps(bench_step(a.config, a.batch, a.steps, a.blocks, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
