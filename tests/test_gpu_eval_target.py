"""eval_target on the GPU: lidog_eval_confusion against torch's CPU arg-max and the numpy counts (full-size batch, ties,
NaN rows, shuffled rows, accumulation, a batch index out of range, two runs), every G14 case through the device against
the rows sklearn gave, TargetEvaluator against evaluate.evaluate and against eval_ref, the packed prediction records,
and train -> checkpoint -> eval_target end to end with two targets and saved predictions."""
import csv
import os

import numpy as np
import pytest
import torch

import eval_ref as E
from lidog_amd import evaluate, synth

pytestmark = pytest.mark.gpu

META, G14 = E.load_g14()
CASES = sorted(E.CASES)


def _logits(n, c, seed):
    """random float32 logits: a third of the rows on a grid of 0.5 (exact ties, often of the maximum), about 2 % of the
    rows with one or two NaN at any position"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, c), generator=g)
    grid = torch.randint(0, 3, (n, c), generator=g).float() * 0.5
    tied = torch.rand(n, generator=g) < 0.33
    x[tied] = grid[tied]
    nan_rows = torch.nonzero(torch.rand(n, generator=g) < 0.02).view(-1)
    x[nan_rows, torch.randint(0, c, (nan_rows.shape[0],), generator=g)] = float("nan")
    x[nan_rows[::2], torch.randint(0, c, (nan_rows[::2].shape[0],), generator=g)] = float("nan")
    return x


# ------------------------------------------------------------------ the confusion kernel
def test_confusion_full_size_batch():
    b = synth.make_batch(list(range(8)), "kitti120k", "cuda")
    coords, labels = b["coords_int"], b["source_sem_labels0"]
    n = coords.shape[0]
    assert n > 600000
    host = _logits(n, 7, 0)
    want_preds = host.max(1)[1]
    assert (host.max(1)[0].isnan()).sum() > 1000 and ((host == host.max(1, keepdim=True)[0]).sum(1) > 1).sum() > 10000
    logits = host.cuda()
    scan = coords[:, 0].cpu().numpy()
    want = E.confusion_np(want_preds.numpy(), labels.cpu().numpy(), scan, 8)
    preds, counts = evaluate.confusion(logits, labels, coords, 8)
    assert preds.dtype == counts.dtype == torch.int64 and counts.shape == (8, 8, 7)
    assert torch.equal(preds.cpu(), want_preds)
    assert np.array_equal(counts.cpu().numpy(), want) and int(counts.sum()) == n
    # two runs give the same bytes
    preds2, counts2 = evaluate.confusion(logits, labels, coords, 8)
    assert torch.equal(preds, preds2) and torch.equal(counts, counts2)
    # accumulation: counts are added to
    _, acc = evaluate.confusion(logits, labels, coords, 8, out=counts2)
    assert acc is counts2 and np.array_equal(acc.cpu().numpy(), 2 * want)
    # into a slice of a larger tensor, as TargetEvaluator does
    big = torch.zeros((20, 8, 7), dtype=torch.int64, device="cuda")
    evaluate.confusion(logits, labels, coords, 8, out=big[5:13])
    assert np.array_equal(big[5:13].cpu().numpy(), want) and int(big[:5].abs().sum() + big[13:].abs().sum()) == 0
    # shuffled rows: the scans are not contiguous
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).cuda()
    sp, sc = evaluate.confusion(logits[perm].contiguous(), labels[perm].contiguous(), coords[perm].contiguous(), 8)
    assert torch.equal(sp, preds[perm]) and np.array_equal(sc.cpu().numpy(), want)
    # a batch index out of range is reported, not counted, and nothing else changes
    bad = coords.clone()
    rows = torch.tensor([0, n // 2, n - 1], device="cuda")
    bad[rows, 0] = torch.tensor([8, -1, 2 ** 31 - 1], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="batch index"):
        evaluate.confusion(logits, labels, bad, 8)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    bp, bc = evaluate.confusion(logits, labels, bad, 8, err=err)
    assert int(err) == 1 and torch.equal(bp, preds)
    assert np.array_equal(bc.cpu().numpy(), E.confusion_np(want_preds.numpy(), labels.cpu().numpy(),
                                                           bad[:, 0].cpu().numpy(), 8))
    err.zero_()
    evaluate.confusion(logits, labels, coords, 8, err=err)
    assert int(err) == 0
    with pytest.raises(ValueError, match="batch index"):
        evaluate.check_scan_error(torch.ones(1, dtype=torch.int32, device="cuda"))


def test_confusion_many_scans_and_classes():
    """32 classes leave LDS room for 7 scans per pass: 40 interleaved scans take several passes per block"""
    n, c, s = 20000, 32, 40
    g = torch.Generator().manual_seed(2)
    host = _logits(n, c, 3)
    labels = torch.randint(-1, c + 2, (n,), generator=g)                 # labels past the classes go to row 0
    coords = torch.randint(-50, 50, (n, 4), generator=g).int()
    coords[:, 0] = torch.randint(0, s, (n,), generator=g).int()
    preds, counts = evaluate.confusion(host.cuda(), labels.cuda(), coords.cuda(), s)
    assert torch.equal(preds.cpu(), host.max(1)[1])
    want = E.confusion_np(host.max(1)[1].numpy(), labels.numpy(), coords[:, 0].numpy(), s, c)
    assert np.array_equal(counts.cpu().numpy(), want)
    assert int(want[:, 0].sum()) == int(((labels < 0) | (labels >= c)).sum()) > n // 20      # 3 of 35 label values
    # an in-range ignore label goes to row 0 as well
    _, c3 = evaluate.confusion(host.cuda(), labels.cuda(), coords.cuda(), s, ignore_label=3)
    assert np.array_equal(c3.cpu().numpy(), E.confusion_np(host.max(1)[1].numpy(), labels.numpy(),
                                                           coords[:, 0].numpy(), s, c, ignore_label=3))
    with pytest.raises(ValueError, match="classes"):
        evaluate.confusion(torch.zeros((4, 33), device="cuda"), labels[:4].cuda(), coords[:4].cuda(), s)
    # no rows: nothing is launched, the counts stay
    p0, c0 = evaluate.confusion(torch.zeros((0, 7), device="cuda"), labels[:0].cuda(), coords[:0].cuda(), 2)
    assert p0.shape == (0,) and int(c0.sum()) == 0


# ------------------------------------------------------------------ G14 through the device
def _device_counts(case):
    """counts of a case, batch by batch, into one tensor (the scans of a batch numbered from 0, as collated)"""
    n_scans = case["batch_of_scan"].shape[0]
    counts = torch.zeros((n_scans, E.C + 1, E.C), dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    for b in np.unique(case["batch_of_scan"]):
        scans = np.nonzero(case["batch_of_scan"] == b)[0]
        sel = np.isin(case["scan"], scans)
        preds = torch.from_numpy(case["preds"][sel])
        coords = torch.zeros((int(sel.sum()), 4), dtype=torch.int32)
        coords[:, 0] = torch.from_numpy(case["scan"][sel] - scans[0]).int()
        logits = torch.nn.functional.one_hot(preds, E.C).float()
        got, _ = evaluate.confusion(logits.cuda(), torch.from_numpy(case["labels"][sel]).cuda(), coords.cuda(),
                                    len(scans), out=counts[scans[0]:scans[-1] + 1], err=err)
        assert torch.equal(got.cpu(), preds)
    evaluate.check_scan_error(err)
    return counts


@pytest.mark.parametrize("name", CASES)
def test_g14_through_the_device(name):
    case = E.case_arrays(G14, name)
    counts = _device_counts(case)
    assert np.array_equal(counts.cpu().numpy(), E.confusion_np(case["preds"], case["labels"], case["scan"],
                                                               case["batch_of_scan"].shape[0]))
    for mode in E.MODES:
        rows = evaluate.iou_rows(counts, mode, case["batch_of_scan"])
        assert np.array_equal(rows, G14[f"{name}/{mode}/rows"]), mode
        per_class, mean = evaluate.mean_iou_rows(rows)
        assert np.array_equal(per_class, G14[f"{name}/{mode}/per_class"], equal_nan=True)
        assert mean == float(G14[f"{name}/{mode}/mean"])
    # per scan: the existing per_class_iou, exactly
    rows = evaluate.iou_rows(counts, "scan")
    for s in range(rows.shape[0]):
        sel = case["scan"] == s
        old = evaluate.per_class_iou(torch.from_numpy(case["preds"][sel]).cuda(),
                                     torch.from_numpy(case["labels"][sel]).cuda())
        assert np.array_equal(old.cpu().numpy(), rows[s]), s


# ------------------------------------------------------------------ TargetEvaluator
@pytest.mark.parametrize("kind", ["MinkUNet34", "MinkUNet34BEV"])
def test_target_evaluator_equals_evaluate(kind):
    from lidog_amd.train import SynthScans, build_model
    torch.manual_seed(11)
    model = build_model(kind).eval()
    data = SynthScans(6, "nusc35k", first=10 ** 6)
    batches = list(evaluate.dataset_batches(data, 4))
    assert [len(ids) for _, ids in batches] == [4, 2]                    # one ragged last batch
    old_per_class, old_mean = evaluate.evaluate(model, [b for b, _ in batches])
    ev = evaluate.TargetEvaluator(model)
    res = ev.run(batches, 6, rows="scan")
    assert res["scans"] == 6 and res["rows"].shape == (6, 7) and res["counts"].shape == (6, 8, 7)
    assert list(res["batch_of_scan"]) == [0, 0, 0, 0, 1, 1]
    assert int(res["counts"].sum()) == sum(b["coords_int"].shape[0] for b, _ in batches)
    # the same rows through the same nan-mean where evaluate() takes it, on the device: exactly evaluate()'s numbers
    # (torch's CPU nan-mean adds the six rows in another order than its device reduction and may end an ulp away)
    per_class, mean = evaluate.mean_iou(torch.from_numpy(res["rows"]).cuda())
    assert torch.equal(per_class, old_per_class) and torch.equal(mean, old_mean)
    # run()'s own numpy nan-mean adds the same <= 6 float64 terms per class, possibly in another order: a few ulp of
    # values <= 100
    assert np.allclose(res["per_class"], old_per_class.cpu().numpy(), rtol=0, atol=1e-12, equal_nan=True)
    assert abs(res["mean"] - float(old_mean)) <= 1e-12
    # per batch, as the reference: eval_ref on the per-scan counts
    resb = ev.run(batches, 6, rows="batch")
    assert np.array_equal(resb["counts"], res["counts"])                 # two runs: the same bytes
    want = E.iou_rows_np(res["counts"], "batch", res["batch_of_scan"])
    assert resb["rows"].shape == (2, 7) and np.array_equal(resb["rows"], want)
    per_class, mean = E.epoch_end_np(want)
    assert np.array_equal(resb["per_class"], per_class, equal_nan=True) and resb["mean"] == mean
    # a generator of batches (what eval_target passes) gives the same
    resg = ev.run(evaluate.dataset_batches(data, 4), 6, rows="batch")
    assert np.array_equal(resg["counts"], res["counts"])
    with pytest.raises(ValueError, match="n_scans"):
        ev.run(batches, 5)


# ------------------------------------------------------------------ the prediction dump
def test_packed_prediction_records():
    b = synth.make_batch([3, 4, 5], "nusc35k", "cuda")
    coords, labels = b["coords_int"], b["source_sem_labels0"]
    n = coords.shape[0]
    preds = torch.randint(0, 7, (n,), generator=torch.Generator().manual_seed(5)).cuda()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(6)).cuda()     # scans interleaved
    for c, p, l in ((coords, preds, labels), (coords[perm].contiguous(), preds[perm], labels[perm])):
        buf = evaluate.pack_predictions(c, p, l, 3)
        assert buf.dtype == torch.int32 and buf.shape == (4 + 5 * n,)
        again = evaluate.pack_predictions(c, p, l, 3)
        recs = evaluate.unpack_predictions(buf, 3)
        start = buf[:4].cpu().numpy()
        assert torch.equal(buf[:4 + 5 * int(start[3])], again[:4 + 5 * int(start[3])])
        ch, ph, lh = c.cpu().numpy(), p.cpu().numpy(), l.cpu().numpy()
        for s in range(3):
            keep = np.nonzero((ch[:, 0] == s) & (lh != -1))[0]                      # ascending row order
            want = np.concatenate([ch[keep, 1:], ph[keep, None], lh[keep, None]], axis=1).astype(np.int32)
            assert recs[s].shape == want.shape and np.array_equal(recs[s], want), s
        assert int(start[3]) == int((lh != -1).sum()) and 0 < start[3] < n
    # an empty scan inside a batch, and every label ignored
    two = coords.clone()
    two[two[:, 0] == 1, 0] = 2
    recs = evaluate.unpack_predictions(evaluate.pack_predictions(two, preds, labels, 3), 3)
    assert recs[1].shape == (0, 5) and recs[0].shape[0] > 0 and recs[2].shape[0] > recs[0].shape[0]
    recs = evaluate.unpack_predictions(evaluate.pack_predictions(coords, preds, torch.full_like(labels, -1), 3), 3)
    assert all(r.shape == (0, 5) for r in recs)
    bad = coords.clone()
    bad[7, 0] = 3
    with pytest.raises(ValueError, match="batch index"):
        evaluate.pack_predictions(bad, preds, labels, 3)


# ------------------------------------------------------------------ end to end
def _check_clouds(folder, target, config, t, scans, with_labels):
    pal = evaluate.palette(7)
    assert sorted(os.listdir(os.path.join(folder, target))) == (["labels", "preds"] if with_labels else ["preds"])
    for kind in (("preds", "labels") if with_labels else ("preds",)):
        assert sorted(os.listdir(os.path.join(folder, target, kind))) == sorted(f"{i}.ply" for i in range(scans))
    for i in range(scans):
        vox, lab = synth.scan_voxels(10 ** 6 + t * synth.SOURCE1_SEED + i, config)
        keep = lab != -1
        pts, col = evaluate.read_ply(os.path.join(folder, target, "preds", f"{i}.ply"))
        assert np.array_equal(pts, vox[keep].astype(np.float64))                   # exactly the labelled voxels
        assert all(tuple(c) in {tuple(p) for p in pal[1:]} for c in np.unique(col, axis=0))
        if with_labels:
            pts, col = evaluate.read_ply(os.path.join(folder, target, "labels", f"{i}.ply"))
            assert np.array_equal(pts, vox[keep].astype(np.float64)) and np.array_equal(col, pal[lab[keep] + 1])


def _check_csv(path, sources, targets):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["source", "target"] + list(evaluate.CLASS_NAMES) + ["mean"] and len(rows) == 1 + len(targets)
    for row, target in zip(rows[1:], targets):
        assert row[:2] == [sources, target] and len(row) == 10
        vals = [float(v.replace(",", ".")) for v in row[2:]]
        assert all(0.0 <= v <= 100.0 for v in vals)
        assert all("." not in v and len(v.split(",")[1]) <= 2 for v in row[2:])
    return rows


def test_train_then_eval_target_end_to_end(tmp_path, capsys):
    import json
    from lidog_amd import eval_target, train
    run = str(tmp_path / "run")
    train.main(["--model", "MinkUNet34BEV", "--config", "source8k", "--scans", "2", "--batch", "2", "--epochs", "1",
                "--save-dir", run])
    ckpt = train.last_checkpoint(run)
    assert ckpt == os.path.join(run, "checkpoints", "epoch=0-step=1.ckpt")
    capsys.readouterr()
    res = eval_target.main(["--checkpoint", ckpt, "--sources", "source8k", "--targets", "source8k", "nusc35k",
                            "--scans", "3", "--batch", "2", "--save-predictions"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["target"] for l in lines] == ["source8k", "nusc35k"] == [r["target"] for r in res]
    for l, r in zip(lines, res):
        assert l["scans"] == 3 and l["rows"] == 2 and l["scans_per_s"] > 0 and len(l["per_class_iou"]) == 7
        assert l["checkpoint_epoch"] == 0 and r["iou_rows"].shape == (2, 7) and l["mean_iou"] == r["mean_iou"]
    path = os.path.join(run, "results", "source8k-TO-source8knusc35k.csv")
    assert os.listdir(os.path.join(run, "results")) == ["source8k-TO-source8knusc35k.csv"] and res[0]["csv"] == path
    rows = _check_csv(path, "source8k", ["source8k", "nusc35k"])
    for row, r in zip(rows[1:], res):
        assert row[-1] == str(round(r["mean_iou"], 2)).replace(".", ",")
    # the BEV model's test_step writes preds only
    for t, target in enumerate(("source8k", "nusc35k")):
        _check_clouds(os.path.join(run, "predictions"), target, target, t, 3, with_labels=False)
    # per scan rows on request; no predictions folder without the switch
    run2 = str(tmp_path / "run2")
    os.makedirs(os.path.join(run2, "checkpoints"))
    import lidog_amd
    torch.manual_seed(3)
    model = lidog_amd.MinkUNet34(1, 7, 3)
    plain = os.path.join(run2, "checkpoints", "weights.ckpt")
    torch.save({"model." + k: v for k, v in model.state_dict().items()}, plain)     # Lightning's key names, no wrapper
    res2 = eval_target.main(["--checkpoint", plain, "--model", "MinkUNet34", "--sources", "source8k", "--targets",
                             "nusc35k", "--scans", "3", "--batch", "2", "--rows", "scan"])
    assert res2[0]["iou_rows"].shape == (3, 7) and res2[0]["checkpoint_epoch"] is None
    assert not os.path.exists(os.path.join(run2, "predictions"))
    _check_csv(os.path.join(run2, "results", "source8k-TO-nusc35k.csv"), "source8k", ["nusc35k"])
    # the other models write labels as well; the weights that were loaded are the file's
    res3 = eval_target.main(["--checkpoint", plain, "--model", "MinkUNet34", "--sources", "source8k", "--targets",
                             "nusc35k", "--scans", "3", "--batch", "2", "--rows", "scan", "--save-predictions"])
    assert np.array_equal(res3[0]["counts"], res2[0]["counts"])
    _check_clouds(os.path.join(run2, "predictions"), "nusc35k", "nusc35k", 0, 3, with_labels=True)
    ev = evaluate.TargetEvaluator(model.cuda().eval())
    direct = ev.run(evaluate.dataset_batches(train.SynthScans(3, "nusc35k", first=10 ** 6), 2), 3, rows="scan")
    assert np.array_equal(direct["counts"], res2[0]["counts"])
