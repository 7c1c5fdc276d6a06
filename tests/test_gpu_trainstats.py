"""Per-step training metrics on the GPU: lidog_train_confusion against numpy counts (exact integers), the step classes
with metrics on against a twin with metrics off (bit for bit) and against counts made on the host, and the driver's
metrics file."""
import os

import numpy as np
import pytest
import torch

import metrics_ref as M
from helpers import seeded_state_dict

pytestmark = pytest.mark.gpu

ROWS = M.kernel_rows_per_block()


def _segment(n, c, seed, special=True):
    """(logits [n, c] float32, labels [n] int64 with -1) on the host; with `special` a few rows get exact ties, a NaN,
    +inf, -inf, all -inf and all equal values"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, c), generator=g)
    lab = torch.randint(-1, c, (n,), generator=g)
    if special and n:
        r = torch.randint(0, n, (12,), generator=g).tolist()
        x[r[0], :] = 0.5                                        # every class ties: the first
        x[r[1], c - 1] = x[r[1]].max() if c > 1 else x[r[1], 0]                       # tie with the last: the earlier one
        x[r[2], c // 2] = float("nan")
        x[r[3], 0] = float("nan")
        x[r[3], c - 1] = float("nan")                           # two NaNs: the first
        x[r[4], c - 1] = float("inf")
        x[r[5], :] = float("-inf")                              # all -inf: the first
        x[r[6], 0] = float("-inf")
        x[r[7], c // 2] = float("inf")
        x[r[7], c - 1] = float("nan")                           # a NaN beats +inf
    return x, lab


@pytest.mark.parametrize("c", [7, 19, 32])
def test_eight_segments_in_one_launch_equal_numpy_counts(c):
    """sizes 0, 1, one below / at / one above the rows of a block, three blocks and a bit; an empty segment in the
    middle; one segment on a 4-byte boundary only (the copy to LDS without 16-byte loads)"""
    from lidog_amd.metrics import train_confusion
    sizes = [1, ROWS - 1, ROWS, 0, ROWS + 1, 2 * ROWS + 437, 300, 0]
    segs = [_segment(n, c, 100 * c + s) for s, n in enumerate(sizes)]
    pairs = []
    for s, (x, lab) in enumerate(segs):
        if s == 6:                                              # logits starting one float past an aligned buffer
            buf = torch.empty(x.numel() + 1, device="cuda")
            buf[1:] = x.reshape(-1).cuda()
            pairs.append((buf[1:].view(x.shape), lab.cuda()))
            assert pairs[-1][0].data_ptr() % 16 == 4
        else:
            pairs.append((x.cuda(), lab.cuda()))
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = train_confusion(pairs, num_classes=c, err=err)
    assert got.shape == (8, c + 1, c) and got.dtype == torch.int64
    want = np.stack([M.host_counts(x, lab.numpy(), c) for x, lab in segs])
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(err.item()) == 0
    assert got.sum(dim=(1, 2)).tolist() == sizes
    # one segment alone, and the same launch again into the same buffer: the sum
    alone = train_confusion([pairs[5]], num_classes=c)
    assert np.array_equal(alone.cpu().numpy()[0], want[5])
    train_confusion(pairs, num_classes=c, out=got, err=err)
    assert np.array_equal(got.cpu().numpy(), 2 * want)


def test_bev_level_is_read_as_the_view_reads_it():
    """[2, 7, 5, 5] NCHW logits as they are against torch's `view(2, 5, 5, -1).argmax(-1)` on the CPU"""
    from lidog_amd.metrics import train_confusion
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 7, 5, 5), generator=g)
    lab = torch.randint(-1, 7, (2, 5, 5), generator=g)
    pred = x.view(2, 5, 5, -1).argmax(dim=-1).view(-1)
    want = torch.zeros((8, 7), dtype=torch.int64)
    want.index_put_((lab.view(-1) + 1, pred), torch.ones(50, dtype=torch.int64), accumulate=True)
    pts, pl = _segment(40, 7, 6)
    got = train_confusion([(pts.cuda(), pl.cuda()), (x.cuda(), lab.cuda())])
    assert torch.equal(got[1].cpu(), want)
    assert np.array_equal(got[0].cpu().numpy(), M.host_counts(pts, pl.numpy()))


def test_out_of_range_labels_set_the_error_bit_and_stay_inside_counts():
    from lidog_amd.metrics import check_label_error, train_confusion
    c, guard = 7, 4096
    segs = [_segment(n, c, 900 + s, special=False) for s, n in enumerate((500, ROWS + 30, 700))]
    segs[1][1][[3, ROWS + 7]] = torch.tensor([c, -2])            # one past the classes, a negative other than -1
    segs[2][1][11] = 1 << 40
    size = 3 * (c + 1) * c
    buf = torch.full((guard + size + guard,), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
    counts = buf[guard:guard + size].view(3, c + 1, c)
    counts.zero_()
    errbuf = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    errbuf[1] = 0
    train_confusion([(x.cuda(), lab.cuda()) for x, lab in segs], num_classes=c, out=counts, err=errbuf[1:2])
    assert errbuf.tolist() == [0x5A5A5A5A, 0b110, 0x5A5A5A5A]
    host = buf.cpu()
    assert bool((host[:guard] == -0x0123456789ABCDEF).all()) and bool((host[guard + size:] == -0x0123456789ABCDEF).all())
    want = np.stack([M.host_counts(x, lab.numpy(), c) for x, lab in segs])           # such labels land in row 0
    assert np.array_equal(counts.cpu().numpy(), want)
    assert want[1, 0].sum() == int(((segs[1][1] < 0) | (segs[1][1] >= c)).sum())
    with pytest.raises(ValueError, match=r"segment\(s\) \[1, 2\]"):
        check_label_error(errbuf[1:2])
    with pytest.raises(ValueError):                              # without an error word the call itself checks
        train_confusion([(segs[2][0].cuda(), segs[2][1].cuda())], num_classes=c)


def test_wrapper_refuses_what_the_kernel_cannot_read():
    from lidog_amd.metrics import train_confusion
    x, lab = torch.randn(10, 7, device="cuda"), torch.zeros(10, dtype=torch.int64, device="cuda")
    for bad in ([(x.double(), lab)], [(x, lab.int())], [(x[:, :6], lab)], [(x.cpu(), lab.cpu())], [], [(x, lab)] * 9):
        with pytest.raises((ValueError, RuntimeError)):
            train_confusion(bad)
    with pytest.raises(ValueError):
        train_confusion([(x, lab)], out=torch.zeros((1, 8, 7), dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------ the step classes
def _twin_steps(kind):
    import lidog_amd
    from lidog_amd.trainer import FlatAdam, LiDOGStep, SourceStep
    if kind == "LiDOGStep":
        make = lambda: lidog_amd.MinkUNet34BEV(in_channels=1, out_channels=7, D=3, decoder_2d_level=["block8"],
                                               mapping_bound_2d=5.0)
        cls = LiDOGStep
    else:
        make = lambda: lidog_amd.MinkUNet34(in_channels=1, out_channels=7, D=3)
        cls = SourceStep
    sd = seeded_state_dict(make(), seed=5)
    steps = []
    for _ in range(3):
        m = make()
        m.load_state_dict(sd)
        m.cuda().train()
        steps.append(cls(m, FlatAdam(m, lr=1e-3, weight_decay=1e-4)))
    return steps


@pytest.mark.parametrize("kind", ["LiDOGStep", "SourceStep"])
def test_step_with_metrics_is_bit_identical_and_records_the_host_counts(kind):
    from lidog_amd.metrics import MetricLayout, StepMetrics, iou_from_counts, mean_present
    on, off, twin = _twin_steps(kind)
    layout = MetricLayout.for_step(on, ["scenes"], levels=("block8",))
    on.metrics = StepMetrics(layout, log_every_n_steps=1)
    batches = [M.scene_batch((40 + i, 50 + i), "cuda") for i in range(2)]
    # step 1 of a state-identical twin, on the host: the counts of forward_loss's outputs
    twin.metrics = object()                 # forward_loss records nothing; a LiDOGStep with metrics keeps its BEV logits
    out = twin.forward_loss(batches[0])
    sem = out[-1]
    want_counts = [M.host_counts(sem.F.detach().cpu(), batches[0]["source_sem_labels0"].cpu().numpy())]
    want_losses = {"loss": float(out[0].detach())}
    if kind == "LiDOGStep":
        bev = twin._bev_outs[0]["block8"].detach().cpu()
        assert tuple(bev.shape) == (2, 7, 17, 17)
        want_counts.append(M.host_counts(bev, batches[0]["source_bev_labels0"]["block8"].cpu().numpy()))
        want_losses.update(sem_loss=float(out[1].detach()), bev_loss=float(out[2].detach()))
    else:
        want_losses.update(sem_loss=float(out[0].detach()))
    got_on = [on.training_step(b) for b in batches]
    got_off = [off.training_step(b) for b in batches]
    for a, b in zip(got_on, got_off):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a), (a, b)
    for (k, a), (_, b) in zip(on.model.state_dict().items(), off.model.state_dict().items()):
        assert torch.equal(a, b), k
    recs = on.metrics.finish()
    assert [r["step"] for r in recs] == [1, 2] and on.metrics.finish() == []
    rec = recs[0]
    tails = ["", "_bev_block8"]
    means = ["source_iou0", "source_iou_bev0_block8"]
    expected = {"step", "training/epoch", "training/lr", "training/scenes/total_loss", "training/scenes/sem_loss0"}
    for counts, tail, mean in zip(want_counts, tails, means):
        iou, present, occ = iou_from_counts(torch.from_numpy(counts), layout.count_ignored)
        assert bool(present.all())                               # 2 x 1200 random labels: every class occurs
        for c, name in enumerate(layout.class_names):
            assert rec[f"training/scenes/{name}_iou{tail}"] == float(iou[c])
            assert rec[f"training/scenes/{name}_count{tail}"] == int(occ[c])
            expected |= {f"training/scenes/{name}_iou{tail}", f"training/scenes/{name}_count{tail}"}
        assert abs(rec[f"training/scenes/{mean}"] - float(mean_present(iou, present))) <= 1e-15
        expected.add(f"training/scenes/{mean}")
    assert rec["training/scenes/total_loss"] == want_losses["loss"] == float(got_on[0]["loss"])
    assert rec["training/scenes/sem_loss0"] == want_losses["sem_loss"]
    if kind == "LiDOGStep":
        assert rec["training/scenes/bev_loss0"] == want_losses["bev_loss"]
        expected.add("training/scenes/bev_loss0")
    assert rec["training/lr"] == 1e-3 and rec["training/epoch"] == 0
    assert set(rec) == expected


# ------------------------------------------------------------------ the driver
def _fit(tmp_path, name, n, kind="MinkUNet34BEV", val=None):
    from lidog_amd.train import Trainer
    return Trainer(model_kind=kind, bound_2d=5.0, batch_size=2, lr=1e-3, epochs=2, train_data=M.Scenes(6), val_data=val,
                   check_val_every_n_epoch=1, save_dir=str(tmp_path / name), log=lambda *_: None, log_every_n_steps=n)


@pytest.mark.parametrize("n,steps", [(1, [1, 2, 3, 4, 5, 6]), (2, [2, 4, 6])])
def test_trainer_writes_one_record_per_logged_step(tmp_path, n, steps):
    from lidog_amd.metrics import MetricsWriter
    fit = _fit(tmp_path, f"n{n}", n, val=M.Scenes(2, seed0=80) if n == 2 else None)
    hist = fit.run()
    recs = MetricsWriter.read(os.path.join(fit.save_dir, "metrics.jsonl"))
    val = [r for r in recs if "validation/epoch" in r]
    recs = [r for r in recs if "validation/epoch" not in r]
    if n == 2:      # the validation results of every epoch under the reference's keys, behind the epoch's steps
        assert [(r["step"], r["validation/epoch"]) for r in val] == [(3, 0), (6, 1)]
        for r, h in zip(val, hist):
            assert r["validation/scenes/sem_loss"] == h["validation"]["sem_loss"]
            assert r["validation/scenes/source_iou"] == h["validation"]["source_iou"]
            assert all(0.0 <= r[f"validation/scenes/{c}_source_iou"] <= 1.0 for c in fit.metrics.layout.class_names)
            assert len(r) == 4 + 7
    else:
        assert val == []
    assert [r["step"] for r in recs] == steps
    assert [r["step"] for h in hist for r in h["metrics"]] == steps
    assert [r["training/epoch"] for r in recs] == [(s - 1) // 3 for s in steps]
    keys = set(fit.metrics.layout.keys) | {"step", "training/epoch"}
    assert len(keys) == 36
    for r, h in zip(recs, [r for h in hist for r in h["metrics"]]):
        assert r == h and set(r) <= keys
        assert {"training/scenes/source_iou0", "training/scenes/source_iou_bev0_block8", "training/scenes/total_loss",
                "training/scenes/sem_loss0", "training/scenes/bev_loss0", "training/lr"} <= set(r)
        assert all(np.isfinite(v) for v in r.values())
        assert all(0.0 <= v <= 1.0 for k, v in r.items() if "_iou" in k)
        assert sum(v for k, v in r.items() if k.endswith("_count")) <= 2 * 1300      # labelled voxels of two scenes
        assert sum(v for k, v in r.items() if k.endswith("_count_bev_block8")) <= 2 * 17 * 17
    # the history's loss of a logged step is the recorded total
    flat = [l for h in hist for l in h["losses"]]
    assert [r["training/scenes/total_loss"] for r in recs] == [flat[s - 1] for s in steps]


def test_trainer_without_the_flag_writes_nothing(tmp_path):
    fit = _fit(tmp_path, "off", 0, kind="MinkUNet34")
    hist = fit.run()
    assert fit.metrics is None and fit.step.metrics is None
    assert all("metrics" not in h for h in hist)
    assert not os.path.exists(os.path.join(fit.save_dir, "metrics.jsonl"))
