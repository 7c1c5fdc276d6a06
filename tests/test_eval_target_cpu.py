"""eval_target without a GPU: the G14 fixture covers its cases, eval_ref's numpy restatement and evaluate.iou_rows equal
every recorded row exactly (one float64 division on each side: no tolerance), the CSV text for one and two targets, the
PLY round trip, the command line, the C ABI."""
import csv
import ctypes
import os

import numpy as np
import pytest
import torch

import eval_ref as E
from helpers import REPO
from lidog_amd import evaluate

META, G14 = E.load_g14()
CASES = sorted(E.CASES)
EVAL_SYMBOLS = ("lidog_eval_confusion", "lidog_eval_pack_ws", "lidog_eval_pack")


def _counts(case):
    return E.confusion_np(case["preds"], case["labels"], case["scan"], case["batch_of_scan"].shape[0])


# ------------------------------------------------------------------ the fixture
def test_g14_covers_the_cases():
    assert os.path.getsize(E.G14) <= 300 * 1024
    assert set(META["cases"]) == set(E.CASES)
    for name in CASES:
        made, stored = E.make_case(name), E.case_arrays(G14, name)
        assert all(np.array_equal(made[k], stored[k]) for k in made), name       # the arrays are the seeds' arrays
        assert 2000 <= META["cases"][name]["rows"] <= 6000
    c = E.case_arrays(G14, "absent_but_predicted")
    assert not np.isin(c["labels"], [5, 6]).any() and np.isin(c["preds"], [5, 6]).any()
    c = E.case_arrays(G14, "labelled_never_predicted")
    assert np.isin(c["labels"], [4, 5, 6]).any() and not np.isin(c["preds"], [4, 5, 6]).any()
    c = E.case_arrays(G14, "all_ignored_batch")
    assert (c["labels"][c["batch_of_scan"][c["scan"]] == 1] == -1).all()
    c = E.case_arrays(G14, "empty_scan")
    assert not (c["scan"] == 1).any() and c["batch_of_scan"][1] == 0
    assert (G14["all_present/batch/rows"] > 0).all()
    # per-batch rows (the reference) and per-scan rows give different tables
    gap = np.abs(G14["batch_vs_scan/batch/per_class"] - G14["batch_vs_scan/scan/per_class"])
    assert (gap > 0.5).all() and abs(gap.min() - META["batch_vs_scan_gap"]) < 1e-12
    assert G14["batch_vs_scan/batch/rows"].shape == (2, 7) and G14["batch_vs_scan/scan/rows"].shape == (5, 7)


# ------------------------------------------------------------------ rows, means
@pytest.mark.parametrize("mode", E.MODES)
@pytest.mark.parametrize("name", CASES)
def test_rows_equal_sklearn_exactly(name, mode):
    case = E.case_arrays(G14, name)
    counts = _counts(case)
    want = G14[f"{name}/{mode}/rows"]
    ref = E.iou_rows_np(counts, mode, case["batch_of_scan"])
    got = evaluate.iou_rows(counts, mode, case["batch_of_scan"])
    assert ref.dtype == got.dtype == want.dtype == np.float64
    assert np.array_equal(ref, want) and np.array_equal(got, want)
    assert np.array_equal(evaluate.iou_rows(torch.from_numpy(counts), mode, case["batch_of_scan"]), want)
    for per_class, mean in (E.epoch_end_np(got), evaluate.mean_iou_rows(got)):
        assert np.array_equal(per_class, G14[f"{name}/{mode}/per_class"], equal_nan=True)
        assert mean == float(G14[f"{name}/{mode}/mean"])


def test_iou_rows_arguments():
    counts = _counts(E.case_arrays(G14, "all_present"))
    one = evaluate.iou_rows(counts)                                     # no grouping given: all scans are one batch
    assert one.shape == (1, 7) and np.array_equal(one, evaluate.iou_rows(counts.sum(0, keepdims=True), "scan"))
    with pytest.raises(ValueError):
        evaluate.iou_rows(counts, "point")
    with pytest.raises(ValueError):
        evaluate.iou_rows(counts[:, :7], "scan")
    with pytest.raises(ValueError):
        evaluate.iou_rows(counts, "batch", [0, 1])
    # a point labelled -1 enlarges the union of the class it is predicted as
    m = np.zeros((1, 8, 7), np.int64)
    m[0, 1, 0], m[0, 0, 0] = 3, 1
    assert evaluate.iou_rows(m, "scan")[0, 0] == 3 / 4 and (evaluate.iou_rows(m, "scan")[0, 1:] == -1).all()


# ------------------------------------------------------------------ CSV
def _read(path):
    with open(path, newline="") as f:
        return f.read()


@pytest.mark.parametrize("mode", E.MODES)
def test_csv_text_one_target(tmp_path, mode):
    for name in CASES:
        d = str(tmp_path / name)
        p = evaluate.write_results_csv(d, E.SOURCES, "nusc35k", G14[f"{name}/{mode}/rows"], E.CLASS_NAMES)
        assert p == os.path.join(d, "results", f"{E.SOURCES}-TO-nusc35k.csv")
        assert _read(p) == META["cases"][name][f"csv_{mode}"], name
    assert "nan" in META["cases"]["absent_but_predicted"]["csv_batch"]          # a class no row carries


@pytest.mark.parametrize("mode", E.MODES)
def test_csv_text_two_targets(tmp_path, mode):
    names = "".join(t for t, _ in E.TWO_TARGETS)
    for o, (target, name) in enumerate(E.TWO_TARGETS):
        p = evaluate.write_results_csv(str(tmp_path), E.SOURCES, target, G14[f"{name}/{mode}/rows"], E.CLASS_NAMES,
                                       first_target=o == 0, file_targets=names)
    assert p.endswith(f"results/{E.SOURCES}-TO-kitti120knusc35k.csv") and os.listdir(tmp_path / "results") == [
        f"{E.SOURCES}-TO-kitti120knusc35k.csv"]
    text = _read(p)
    assert text == META[f"two_targets_csv_{mode}"]
    rows = list(csv.reader(text.splitlines()))
    assert rows[0] == ["source", "target"] + list(E.CLASS_NAMES) + ["mean"]
    assert [r[1] for r in rows[1:]] == ["kitti120k", "nusc35k"] and all(len(r) == 10 for r in rows)


def test_csv_default_output_unchanged(tmp_path):
    """the one-target call without the new argument writes the bytes it always wrote"""
    iou = torch.tensor([[0.5, -1.0, 0.25], [0.7, 0.1, -1.0]], dtype=torch.float64)
    p = evaluate.write_results_csv(str(tmp_path), "SemanticKITTI", "NuScenes", iou, ["vehicle", "person", "road"])
    assert p.endswith("results/SemanticKITTI-TO-NuScenes.csv")
    assert _read(p) == "source,target,vehicle,person,road,mean\r\nSemanticKITTI,NuScenes,\"60,0\",\"10,0\",\"25,0\",\"31,67\"\r\n"


def test_csv_takes_numpy_rows(tmp_path):
    iou = torch.tensor([[0.5, -1.0, 0.25], [0.7, 0.1, -1.0]], dtype=torch.float64)
    p = evaluate.write_results_csv(str(tmp_path / "t"), "SemanticKITTI", "NuScenes", iou, ["vehicle", "person", "road"])
    q = evaluate.write_results_csv(str(tmp_path / "np"), "SemanticKITTI", "NuScenes", iou.numpy(),
                                   ["vehicle", "person", "road"])
    assert _read(q) == _read(p)


# ------------------------------------------------------------------ PLY
def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    pts = rng.integers(-1200, 1200, (500, 3)).astype(np.int32)
    pal = evaluate.palette(7)
    assert pal.shape == (8, 3) and pal.dtype == np.uint8 and len({tuple(c) for c in pal}) == 8
    assert evaluate.palette(9).shape == (10, 3) and np.array_equal(evaluate.palette(9)[:8], pal)
    col = pal[rng.integers(-1, 7, 500) + 1]
    p = evaluate.write_ply(str(tmp_path / "a.ply"), pts, col)
    raw = open(p, "rb").read()
    head = raw[:raw.index(b"end_header\n")].decode().split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"] and "element vertex 500" in head
    assert [l for l in head if l.startswith("property")] == [
        "property double x", "property double y", "property double z",
        "property uchar red", "property uchar green", "property uchar blue"]
    assert len(raw) == raw.index(b"end_header\n") + len(b"end_header\n") + 500 * 27
    got_p, got_c = evaluate.read_ply(p)
    assert got_p.dtype == np.float64 and np.array_equal(got_p, pts) and np.array_equal(got_c, col)
    e = evaluate.write_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8))
    got_p, got_c = evaluate.read_ply(e)
    assert got_p.shape == (0, 3) and got_c.shape == (0, 3)
    with pytest.raises(ValueError):
        evaluate.write_ply(str(tmp_path / "bad.ply"), pts, col[:10])


# ------------------------------------------------------------------ command line
def test_cli_parsing(capsys):
    from lidog_amd import eval_target as T
    a = T.parse_args(["--checkpoint", "/runs/r1/checkpoints/epoch=4-step=100.ckpt"])
    assert (a.model, a.bound, a.sources, a.targets, a.scans, a.batch, a.rows, a.save_predictions, a.seed) == (
        "MinkUNet34BEV", 50.0, ["kitti120k"], ["nusc35k"], 16, 8, "batch", False, 1234)
    from lidog_amd.train import parse_args as train_args
    assert a.batch == 2 * train_args([]).batch                            # eval_target.py doubles the batch size
    assert T.save_dir_of(a.checkpoint) == "/runs/r1"
    assert T.save_dir_of("run/checkpoints/last.ckpt") == "run"
    a = T.parse_args(["--checkpoint", "c.ckpt", "--targets", "kitti120k", "nusc35k", "--rows", "scan",
                      "--model", "MinkUNet34IBN", "--sources", "source8k", "nusc35k", "--save-predictions"])
    assert a.targets == ["kitti120k", "nusc35k"] and a.rows == "scan" and a.save_predictions
    with pytest.raises(NotImplementedError):
        T.parse_args(["--checkpoint", "c.ckpt", "--targets", "kitti120k", "nusc35k", "source8k"])
    with pytest.raises(SystemExit):
        T.parse_args(["--targets", "nusc35k"])
    assert "You must provide a checkpoint for evaluation!" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        T.parse_args(["--checkpoint", "c.ckpt", "--model", "PointNet"])


# ------------------------------------------------------------------ C ABI
def test_eval_symbols_exported_and_bound():
    from lidog_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    for name in EVAL_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f"{name}(" in header
    assert _lib.ABI_VERSION == 9 and lib.lidog_abi_version() == 9          # additive entries: the version stays
    assert "evalstats.hip" in build.SOURCES
    lib.lidog_eval_pack_ws.restype = ctypes.c_int64
    lib.lidog_mix_split_ws.restype = ctypes.c_int64
    for n, s in ((0, 1), (5000, 8), (700000, 8)):
        ws = lib.lidog_eval_pack_ws(ctypes.c_int64(n), ctypes.c_int32(s))
        assert ws == 2 * n + 2 * s + 1 + lib.lidog_mix_split_ws(ctypes.c_int64(n), ctypes.c_int32(s))
    # arguments are refused on the host, before any launch: 33 classes, 257 scans of a dump
    lib.lidog_last_error.restype = ctypes.c_char_p
    i64, i32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    assert lib.lidog_eval_confusion(vp(), vp(), vp(), i64(10), i32(33), i32(1), i64(-1), vp(), vp(), vp(), vp()) == 2
    assert b"33 classes" in lib.lidog_last_error()
    assert lib.lidog_eval_pack(vp(), vp(), vp(), i64(10), i32(257), i64(-1), vp(), vp(), vp(), vp()) == 2
    assert b"257 scans" in lib.lidog_last_error()
