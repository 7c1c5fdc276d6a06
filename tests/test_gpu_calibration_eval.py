"""Calibration in the evaluation loop: TargetEvaluator.run(calibration=...) against a hand loop of Predictor ->
CalibrationTable.add, the batch cut, and eval_target --calibration end to end: every other output byte for byte what a run
without the flags writes, the two new files, the fit on the calibration set, the suffixes, --adapt bn and --precision bf16.
A randomly initialised MinkUNet34 with the BatchNorm running statistics moved away from (0, 1); 4 synthetic scans of
source8k in batches of 2; the checkpoint is written by the test."""
import csv
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KIND = "MinkUNet34"


def _model(seed=5):
    from lidog_amd import adapt
    from lidog_amd.train import build_model
    torch.manual_seed(seed)
    model = build_model(KIND)
    g = torch.Generator().manual_seed(seed + 1)
    for bn in adapt.batch_norms(model):
        bn.running_mean.copy_(torch.randn(bn.num_features, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(bn.num_features, generator=g) + 0.5)
    return model.eval()


def _batches(batch, n=4):
    from lidog_amd import evaluate
    from lidog_amd.train import SynthScans
    return list(evaluate.dataset_batches(SynthScans(n, "source8k", first=10 ** 6), batch))


def _same(a, b):
    for k in ("ece", "mce", "nll", "brier", "accuracy", "confidence", "rows"):
        assert a[k] == b[k], k
    assert np.array_equal(a["reliability"], b["reliability"])


def test_target_evaluator_equals_the_hand_loop():
    from lidog_amd import calibration, evaluate
    model = _model()
    batches = _batches(2)
    beta = torch.tensor([0.5], dtype=torch.float64, device="cuda")
    ev = evaluate.TargetEvaluator(model)
    res = ev.run(batches, 4, calibration=[("raw", None), ("half", beta)], calib_bins=10)
    plain = ev.run(batches, 4)
    assert "calibration" not in plain and set(res["calibration"]) == {"raw", "half"}
    assert np.array_equal(res["counts"], plain["counts"]) and np.array_equal(res["rows"], plain["rows"])
    run = evaluate.Predictor(model)
    raw, half = calibration.CalibrationTable(10), calibration.CalibrationTable(10)
    labelled = 0
    for i, (b, _) in enumerate(batches):
        nxt = batches[i + 1][0]["coords_int"] if i + 1 < len(batches) else None
        _, logits = run(b["coords_int"], b["source_features0"], nxt)
        raw.add(logits, b["source_sem_labels0"])
        half.add(logits, b["source_sem_labels0"], beta=beta)
        labelled += int(((b["source_sem_labels0"] >= 0) & (b["source_sem_labels0"] < 7)).sum())
    _same(res["calibration"]["raw"], raw.result())                # bit for bit: the same launches in the same order
    _same(res["calibration"]["half"], half.result())
    assert res["calibration"]["raw"]["rows"] == labelled > 0
    assert res["calibration"]["raw"]["accuracy"] == res["calibration"]["half"]["accuracy"]
    assert res["calibration"]["raw"]["reliability"].shape == (10, 4)
    # the accuracy is the confusion counts' (the same arg-max, the same labelled rows)
    c = plain["counts"][:, 1:, :].sum(axis=0)
    assert res["calibration"]["raw"]["accuracy"] == np.trace(c) / c.sum() and c.sum() == labelled
    # batch 2 and batch 4 give identical integer tables (the logits of a scan do not depend on its batch: eval mode)
    four = ev.run(_batches(4), 4, calibration=[("raw", None), ("half", beta)], calib_bins=10)
    for name in ("raw", "half"):
        a, b = res["calibration"][name], four["calibration"][name]
        assert np.array_equal(a["reliability"], b["reliability"]) and a["brier"] == b["brier"] and a["rows"] == b["rows"]
        assert abs(a["nll"] - b["nll"]) <= 1e-12 * abs(a["nll"])
    with pytest.raises(ValueError, match="share a name"):
        ev.run(batches, 4, calibration=[("raw", None), ("raw", beta)])


def _read(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def _num(s):
    return float(s.replace(",", "."))


def test_eval_target_calibration_end_to_end(tmp_path, capsys):
    from lidog_amd import calibration, eval_target, evaluate
    model = _model()
    runs = {}
    for name in ("plain", "calib"):
        run = str(tmp_path / name)
        os.makedirs(os.path.join(run, "checkpoints"))
        ckpt = os.path.join(run, "checkpoints", "weights.ckpt")
        sd = {"model." + k: v.cpu() for k, v in model.state_dict().items()}
        torch.save({"state_dict": sd, "averaged_state_dict": sd, "epoch": 0}, ckpt)
        runs[name] = (run, ckpt)
    common = ["--model", KIND, "--sources", "source8k", "--targets", "source8k", "nusc35k", "--scans", "4", "--batch", "2"]
    flags = ["--calibration", "--calib-bins", "10", "--temperature", "fit", "--calibrate-on", "source8k",
             "--calibrate-scans", "4"]
    capsys.readouterr()
    plain = eval_target.main(["--checkpoint", runs["plain"][1]] + common)
    plain_lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    calib = eval_target.main(["--checkpoint", runs["calib"][1]] + common + flags)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    # everything a run without the flags writes stays byte for byte
    results = {n: os.path.join(runs[n][0], "results") for n in runs}
    assert os.listdir(results["plain"]) == ["source8k-TO-source8knusc35k.csv"]
    assert sorted(os.listdir(results["calib"])) == ["source8k-TO-source8knusc35k-calibration.csv",
                                                    "source8k-TO-source8knusc35k-reliability.csv",
                                                    "source8k-TO-source8knusc35k.csv"]
    name = "source8k-TO-source8knusc35k.csv"
    assert open(os.path.join(results["plain"], name), "rb").read() == open(os.path.join(results["calib"], name), "rb").read()
    new_keys = {"calibration", "calibration_csv", "reliability_csv", "temperature", "temperature_fit"}
    for t in range(2):
        assert np.array_equal(plain[t]["counts"], calib[t]["counts"])
        assert np.array_equal(plain[t]["iou_rows"], calib[t]["iou_rows"])
        assert set(lines[t]) - set(plain_lines[t]) == new_keys and set(plain_lines[t]) <= set(lines[t])
        for k in set(plain_lines[t]) - {"scans_per_s", "csv"}:
            assert plain_lines[t][k] == lines[t][k], k
    # the fit: the scaled NLL is no larger than the raw one on the calibration set itself, which is target 0 here
    # (--calibrate-on source8k draws the validation scans target 0 is made of)
    T = lines[0]["temperature"]
    fit = lines[0]["temperature_fit"]
    assert 0.01 <= T <= 100 and lines[1]["temperature"] == T and fit["on"] == "source8k" and fit["scans"] == 4
    assert fit["nll_scaled"] <= fit["nll_raw"]
    # (one call over the set there, one per batch here: the integers agree, nll_sum up to its rounding)
    assert fit["rows"] == lines[0]["calibration"]["raw"]["rows"]
    for n in ("raw", "scaled"):
        assert abs(fit["nll_" + n] - lines[0]["calibration"][n]["nll"]) <= 1e-12 * fit["nll_" + n]
    assert lines[0]["calibration"]["scaled"]["nll"] <= lines[0]["calibration"]["raw"]["nll"]
    # the same fit by hand
    logits, labels = calibration.collect_logits(evaluate.Predictor(model), _batches(2))
    hand = calibration.fit_temperature(logits, labels)
    assert hand.temperature() == T
    # the two new files: one row per target and temperature, the bins add up to the labelled voxels
    rows = _read(os.path.join(results["calib"], "source8k-TO-source8knusc35k-calibration.csv"))
    assert rows[0] == ["source", "target", "T", "ECE", "MCE", "NLL", "Brier", "accuracy", "confidence"]
    assert [r[:2] for r in rows[1:]] == [["source8k", "source8k"]] * 2 + [["source8k", "nusc35k"]] * 2
    assert [r[2] for r in rows[1:]] == ["1,0000", f"{T:.4f}".replace(".", ",")] * 2
    rel = _read(os.path.join(results["calib"], "source8k-TO-source8knusc35k-reliability.csv"))
    assert rel[0] == ["source", "target", "T", "bin", "count", "accuracy", "confidence"] and len(rel) == 1 + 2 * 2 * 10
    for t, target in enumerate(("source8k", "nusc35k")):
        labelled = int(calib[t]["counts"][:, 1:, :].sum())
        for n, temp in (("raw", "1,0000"), ("scaled", rows[2][2])):
            m = calib[t]["calibration_tables"][n]
            assert m["rows"] == labelled == lines[t]["calibration"][n]["rows"]
            mine = [r for r in rel[1:] if r[1] == target and r[2] == temp]
            assert len(mine) == 10 and sum(int(r[4]) for r in mine) == labelled
            row = [r for r in rows[1:] if r[1] == target and r[2] == temp][0]
            for col, key in zip(row[3:], calibration.METRICS):
                assert abs(_num(col) - m[key]) <= 0.5e-4 + 1e-12, key
        acc = np.trace(calib[t]["counts"][:, 1:, :].sum(axis=0)) / labelled
        assert calib[t]["calibration_tables"]["raw"]["accuracy"] == acc == calib[t]["calibration_tables"]["scaled"]["accuracy"]


def test_suffixes_adapters_and_bf16(tmp_path, capsys):
    from lidog_amd import eval_target
    model = _model()
    run = str(tmp_path / "run")
    os.makedirs(os.path.join(run, "checkpoints"))
    ckpt = os.path.join(run, "checkpoints", "weights.ckpt")
    sd = {"model." + k: v.cpu() for k, v in model.state_dict().items()}
    torch.save({"state_dict": sd, "averaged_state_dict": sd, "epoch": 0}, ckpt)
    common = ["--checkpoint", ckpt, "--model", KIND, "--sources", "source8k", "--targets", "source8k", "--scans", "4",
              "--batch", "2", "--calibration"]
    fit = ["--temperature", "fit", "--calibrate-on", "source8k", "--calibrate-scans", "2"]
    avg = eval_target.main(common + ["--weights", "averaged", "--temperature", "2"])
    bn = eval_target.main(common + ["--adapt", "bn"] + fit)
    bf = eval_target.main(common + ["--precision", "bf16"] + fit)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    stem = "source8k-TO-source8k"
    assert sorted(os.listdir(os.path.join(run, "results"))) == sorted(
        [f"{stem}{s}.csv" for s in ("", "-avg", "-adapt-bn")] +
        [f"{stem}-{kind}{s}.csv" for s in ("", "-avg", "-adapt-bn") for kind in ("calibration", "reliability")])
    assert avg[0]["calibration_csv"].endswith(f"{stem}-calibration-avg.csv")
    assert bn[0]["reliability_csv"].endswith(f"{stem}-reliability-adapt-bn.csv")
    assert bf[0]["calibration_csv"].endswith(f"{stem}-calibration.csv")
    assert lines[0]["temperature"] == 2.0 and "temperature_fit" not in lines[0]
    for res, line in zip((avg, bn, bf), lines):
        labelled = int(res[0]["counts"][:, 1:, :].sum())
        for n in ("raw", "scaled"):
            m = res[0]["calibration_tables"][n]
            assert m["rows"] == labelled > 0 and m["reliability"][:, 1].sum() == labelled
            assert all(np.isfinite(m[k]) for k in ("ece", "mce", "nll", "brier"))
        assert 0.01 <= line["temperature"] <= 100
    # the averaged weights are the live ones here: T = 2 halves the logits of the same rows
    assert avg[0]["calibration_tables"]["raw"]["accuracy"] == avg[0]["calibration_tables"]["scaled"]["accuracy"]
    # under --adapt bn the adapter went over the calibration set and came back: the counts are those of a run without it
    alone = eval_target.main(common[:-1] + ["--adapt", "bn"])
    assert np.array_equal(alone[0]["counts"], bn[0]["counts"])


def test_file_targets_with_a_calibration_set_from_files(tmp_path, capsys):
    """--calibrate-files / --calibrate-label-maps next to --target-files, --point-level and --save-labels on three tiny
    SemanticKITTI files: the fit is fit_temperature over the validation listing, and the point-level outputs are those of
    a run without the calibration flags"""
    import pointlabels_ref as P
    from lidog_amd import calibration, eval_target, evaluate, scans
    from lidog_amd.checkpoint import save_lightning_checkpoint
    tree, label_map, lut = P.write_tiny_kitti_tree(str(tmp_path / "kitti"))
    model = _model()
    ckpts = {}
    for name in ("plain", "calib"):
        os.makedirs(str(tmp_path / name / "checkpoints"))
        ckpts[name] = str(tmp_path / name / "checkpoints" / "fresh.ckpt")
        save_lightning_checkpoint(model, ckpts[name])
    common = ["--model", KIND, "--sources", "SemanticKITTI", "--target-files", f"SemanticKITTI={tree}", "--label-maps",
              label_map, "--batch", "2", "--point-level", "--save-labels"]
    flags = ["--calibration", "--temperature", "fit", "--calibrate-files", f"SemanticKITTI={tree}",
             "--calibrate-label-maps", label_map, "--calibrate-scans", "2"]
    plain = eval_target.main(["--checkpoint", ckpts["plain"]] + common)
    calib = eval_target.main(["--checkpoint", ckpts["calib"]] + common + flags)
    line = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    assert np.array_equal(plain[0]["counts"], calib[0]["counts"])
    assert np.array_equal(plain[0]["point_counts"], calib[0]["point_counts"])
    for a, b in zip(plain[0]["label_paths"], calib[0]["label_paths"]):
        assert open(a, "rb").read() == open(b, "rb").read()
    data = scans.FileScans(scans.listing("SemanticKITTI", tree, "validation", limit=2), lut)
    logits, labels = calibration.collect_logits(evaluate.Predictor(model), evaluate.dataset_batches(data, 2))
    assert line["temperature"] == calibration.fit_temperature(logits, labels).temperature()
    assert line["temperature_fit"]["on"] == "SemanticKITTI" and line["temperature_fit"]["rows"] > 0
    labelled = int(calib[0]["counts"][:, 1:, :].sum())
    assert calib[0]["calibration_tables"]["scaled"]["rows"] == labelled > 0
    assert sorted(os.listdir(str(tmp_path / "calib" / "results"))) == [
        "SemanticKITTI-TO-SemanticKITTI-calibration.csv", "SemanticKITTI-TO-SemanticKITTI-points.csv",
        "SemanticKITTI-TO-SemanticKITTI-reliability.csv", "SemanticKITTI-TO-SemanticKITTI.csv"]

