"""Calibration without a GPU: metrics_from_table on hand-made tables, the numpy restatement (tests/calibration_ref.py) on a
perfectly calibrated set and on the fit's edge cases, the bytes of the two CSV writers, every refusal of eval_target's new
flags, and the new entry points in the header, the derived binding and the built library."""
import ctypes
import math
import os

import numpy as np
import pytest

import calibration_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = ["--checkpoint", "run/checkpoints/c.ckpt"]
ENTRY_POINTS = ("lidog_calib_ws", "lidog_calib_stats", "lidog_calib_fit_init", "lidog_calib_fit_step")
Q = 2 ** 32


# ------------------------------------------------------------------ metrics_from_table
def test_metrics_single_bin():
    from lidog_amd.calibration import metrics_from_table
    m = metrics_from_table([[8, 6, int(0.5 * Q) * 8]], [8, 3 * Q], 4.0)
    assert m["rows"] == 8 and m["accuracy"] == 0.75 and m["confidence"] == 0.5
    assert m["ece"] == 0.25 and m["mce"] == 0.25 and m["nll"] == 0.5 and m["brier"] == 0.375
    assert m["reliability"].tolist() == [[0.0, 8.0, 0.75, 0.5]]


def test_metrics_with_an_empty_bin():
    from lidog_amd.calibration import metrics_from_table
    table = [[2, 0, 2 * int(0.125 * Q)], [0, 0, 0], [0, 0, 0], [6, 6, 6 * int(0.875 * Q)]]
    m = metrics_from_table(table, [8, Q], 2.0)
    assert m["ece"] == (2 / 8) * 0.125 + (6 / 8) * 0.125 and m["mce"] == 0.125
    assert m["accuracy"] == 0.75 and m["confidence"] == (2 * 0.125 + 6 * 0.875) / 8
    assert m["reliability"].tolist() == [[0.0, 2.0, 0.0, 0.125], [0.25, 0.0, 0.0, 0.0], [0.5, 0.0, 0.0, 0.0],
                                         [0.75, 6.0, 1.0, 0.875]]
    assert np.isfinite(m["reliability"]).all()


def test_metrics_all_rows_in_the_last_bin():
    from lidog_amd.calibration import metrics_from_table
    table = np.zeros((15, 3), dtype=np.int64)
    table[14] = (5, 4, 5 * Q)                                   # conf == 1 exactly: the last bin, conf_q = 2^32 a row
    m = metrics_from_table(table, np.array([5, 2 * Q]), 1e4)
    assert m["confidence"] == 1.0 and m["accuracy"] == 0.8 and abs(m["ece"] - 0.2) < 1e-15 and m["ece"] == m["mce"]
    assert m["nll"] == 2e3 and m["brier"] == 0.4


def test_metrics_of_no_rows_are_zeros():
    from lidog_amd.calibration import metrics_from_table, METRICS
    m = metrics_from_table(np.zeros((10, 3), dtype=np.int64), [0, 0], 0.0)
    assert m["rows"] == 0 and all(m[k] == 0.0 for k in METRICS)
    assert np.isfinite(m["reliability"]).all() and m["reliability"][:, 1:].sum() == 0
    with pytest.raises(ValueError, match="totals"):
        metrics_from_table([[3, 1, 0]], [4, 0], 0.0)             # the bins and the total disagree
    with pytest.raises(ValueError, match="table"):
        metrics_from_table(np.zeros((4, 2)), [0, 0], 0.0)


# ------------------------------------------------------------------ the restatement
def test_restatement_on_a_perfectly_calibrated_set():
    """labels drawn from the softmax itself: in every bin the accuracy is a mean of n_b Bernoulli(conf_i) draws, so
    E[acc_b] = conf_b and sd(acc_b) = sqrt(sum conf_i (1 - conf_i)) / n_b; |acc_b - conf_b| <= 4 sd in every bin (a
    4-sigma event has probability 6e-5 per bin), hence ECE <= sum_b (n_b / N) 4 sd_b"""
    from lidog_amd.calibration import metrics_from_table
    rng = np.random.default_rng(0)
    n, C, B = 40000, 7, 15
    x = (rng.standard_normal((n, C)) * 2.0).astype(np.float32)
    e = np.exp(x.astype(np.float64) - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    labels = (rng.random(n)[:, None] > np.cumsum(p, axis=1)).sum(axis=1).clip(0, C - 1)
    ref = R.stats(x, labels, 1.0, B)
    m = metrics_from_table(ref["table"], ref["totals"], ref["nll_sum"])
    assert m["rows"] == n and ref["err"] == 0
    bound = 0.0
    for b in range(B):
        c = ref["conf"][ref["bins"] == b]
        if c.size:
            sd = math.sqrt(float((c * (1 - c)).sum())) / c.size
            bound += c.size / n * 4 * sd
            row = m["reliability"][b]
            assert row[1] == c.size and abs(row[2] - row[3]) <= 4 * sd + 2.0 ** -32, b
            assert abs(row[3] - c.mean()) <= 2.0 ** -32           # fixed point: half a unit per row
    print(f"perfectly calibrated: ECE {m['ece']:.3g} <= {bound:.3g}")
    assert 0 < m["ece"] <= bound <= 2 * math.sqrt(B / n)      # sd_b <= 1 / (2 sqrt n_b), then Cauchy-Schwarz over the bins
    # the proper scores against their direct formulas
    assert abs(m["nll"] - (-np.log(p[np.arange(n), labels])).mean()) <= 1e-12
    onehot = np.eye(C)[labels]
    assert abs(m["brier"] - ((p - onehot) ** 2).sum(axis=1).mean()) <= 2.0 ** -32
    # a sharpened softmax of the same logits is over-confident: the ECE leaves the spread
    over = R.stats(x, labels, 3.0, B)
    assert metrics_from_table(over["table"], over["totals"], over["nll_sum"])["ece"] > bound
    # the cut into batches does not reach the integers
    parts = [R.stats(x[a:b], labels[a:b], 1.0, B) for a, b in ((0, 13), (13, 20001), (20001, n))]
    assert np.array_equal(sum(q["table"] for q in parts), ref["table"])
    assert np.array_equal(sum(q["totals"] for q in parts), ref["totals"])


def test_restatement_leaves_out_what_the_header_says():
    x = np.zeros((6, 3), dtype=np.float32)
    x[:, 1] = 1.0
    x[4, 0] = np.nan
    x[5, 2] = np.inf
    labels = np.array([1, -1, 3, 2, 1, 1])
    ref = R.stats(x, labels, 1.0, 4, ignore_label=2)
    assert ref["take"].tolist() == [True, False, False, False, False, False] and ref["err"] == 2
    assert ref["totals"][0] == 1 and ref["table"][:, 0].sum() == 1
    assert R.stats(x[:4], labels[:4], 1.0, 4)["err"] == 0
    # equal logits: conf = 1 / C, pred = class 0
    eq = R.stats(np.full((2, 4), 7.5, dtype=np.float32), np.array([0, 1]), 0.4, 10)
    assert eq["conf"].tolist() == [0.25, 0.25] and eq["table"][2].tolist() == [2, 1, 2 * (Q // 4)]
    assert R.edge_distance(np.array([0.25]), 4) == 0 and R.edge_distance(np.array([0.25]), 10) == pytest.approx(0.05)
    assert R.edge_distance(np.array([1.0, 0.0]), 5) == math.inf         # 0 and 1 are no interior edges


def test_fit_restatement_finds_the_scale():
    rng = np.random.default_rng(5)
    for k in (0.4, 1.0, 3.0):
        u = rng.standard_normal((20000, 7)) * 2.0
        e = np.exp(u - u.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
        labels = (rng.random(20000)[:, None] > np.cumsum(p, axis=1)).sum(axis=1).clip(0, 6)
        x = (k * u).astype(np.float32)
        state, trace = R.fit(x, labels)
        assert abs(state["beta"] * k - 1) < 0.05 and state["lo"] <= state["beta"] <= state["hi"]
        assert np.isfinite(trace).all() and trace[0, 0] == 1.0 and trace[-1, 1] <= trace[0, 1]
        assert abs(trace[-1, 2]) < 1e-12                          # the gradient at the last evaluated beta
        root = R.fit_root(x, labels, state["beta"])
        assert abs(float(root) - state["beta"]) <= 1e-12 * state["beta"]
        # the gradient is the derivative of the NLL: central differences
        b = 0.7
        num = (R.fit_sums(x, labels, b + 1e-5)[0] - R.fit_sums(x, labels, b - 1e-5)[0]) / 2e-5
        assert abs(num - R.fit_sums(x, labels, b)[1]) < 1e-7
        numh = (R.fit_sums(x, labels, b + 1e-5)[1] - R.fit_sums(x, labels, b - 1e-5)[1]) / 2e-5
        assert abs(numh - R.fit_sums(x, labels, b)[2]) < 1e-6


def test_fit_restatement_edge_cases():
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((300, 5)) * 2.0).astype(np.float32)
    right, wrong = x.argmax(axis=1), x.argmin(axis=1)
    state, trace = R.fit(x, right)                                # separable: the gradient stays negative
    assert state["beta"] == state["lo"] == state["hi"] == 100.0 and np.isfinite(trace).all()
    assert (trace[:, 2] < 0).all() and R.fit_root(x, right, 1.0) == 100.0
    state, trace = R.fit(x, wrong)                                # every label the least likely class
    assert state["beta"] == state["lo"] == state["hi"] == 0.01 and (trace[:, 2] > 0).all()
    state, trace = R.fit(x, np.full(300, -1))                     # nothing labelled
    assert state["beta"] == 1.0 and state["rows"] == 0 and state["iterations"] == 24 and not trace[:, 1:].any()
    assert R.fit_root(x, np.full(300, -1), 1.0) is None


# ------------------------------------------------------------------ the result files
def test_csv_writers_bytes(tmp_path):
    from lidog_amd.calibration import metrics_from_table, write_calibration_csv, write_reliability_csv
    raw = metrics_from_table([[2, 0, 2 * int(0.125 * Q)], [6, 6, 6 * int(0.875 * Q)]], [8, Q], 2.0)
    scaled = metrics_from_table([[0, 0, 0], [8, 6, 8 * int(0.75 * Q)]], [8, Q // 2], 1.0)
    entries = [(1.0, raw), (1.5, scaled)]
    path = write_calibration_csv(str(tmp_path), "kitti", "nusc", entries, file_targets="nuscpoly-calibration-avg")
    assert path == os.path.join(str(tmp_path), "results", "kitti-TO-nuscpoly-calibration-avg.csv")
    write_calibration_csv(str(tmp_path), "kitti", "poly", entries[:1], first_target=False,
                          file_targets="nuscpoly-calibration-avg")
    assert open(path, newline="").read() == (
        'source,target,T,ECE,MCE,NLL,Brier,accuracy,confidence\r\n'
        'kitti,nusc,"1,0000","0,1250","0,1250","0,2500","0,1250","0,7500","0,6875"\r\n'
        'kitti,nusc,"1,5000","0,0000","0,0000","0,1250","0,0625","0,7500","0,7500"\r\n'
        'kitti,poly,"1,0000","0,1250","0,1250","0,2500","0,1250","0,7500","0,6875"\r\n')
    rel = write_reliability_csv(str(tmp_path), "kitti", "nusc", entries, file_targets="nusc-reliability")
    assert rel.endswith("kitti-TO-nusc-reliability.csv")
    assert open(rel, newline="").read() == (
        'source,target,T,bin,count,accuracy,confidence\r\n'
        'kitti,nusc,"1,0000","0,0000",2,"0,0000","0,1250"\r\n'
        'kitti,nusc,"1,0000","0,5000",6,"1,0000","0,8750"\r\n'
        'kitti,nusc,"1,5000","0,0000",0,"0,0000","0,0000"\r\n'
        'kitti,nusc,"1,5000","0,5000",8,"0,7500","0,7500"\r\n')


# ------------------------------------------------------------------ eval_target's flags
def test_flag_defaults():
    from lidog_amd import eval_target as T
    a = T.parse_args(CKPT)
    assert not a.calibration and a.temperature is None and a.calib_bins is None and a.calibrate_on is None
    a = T.parse_args(CKPT + ["--calibration"])
    assert a.calibration and a.calib_bins == 15 and a.temperature is None
    a = T.parse_args(CKPT + ["--calibration", "--calib-bins", "10", "--temperature", "1.5"])
    assert a.calib_bins == 10 and a.temperature == 1.5
    a = T.parse_args(CKPT + ["--calibration", "--temperature", "fit", "--calibrate-on", "kitti120k"])
    assert a.temperature == "fit" and a.calibrate_on == "kitti120k" and a.calibrate_scans == 16
    a = T.parse_args(CKPT + ["--calibration", "--temperature", "fit", "--calibrate-files", "SemanticKITTI=/data/kitti",
                             "--calibrate-label-maps", "m.yaml", "--calibrate-scans", "4", "--adapt", "bn",
                             "--weights", "averaged"])
    assert a.calibrate_files == ("SemanticKITTI", "/data/kitti") and a.calibrate_scans == 4
    for extra in (["--precision", "bf16"], ["--adapt", "tent"], ["--adapt", "adabn"]):
        assert T.parse_args(CKPT + ["--calibration", "--temperature", "0.5"] + extra).temperature == 0.5


@pytest.mark.parametrize("extra,words", [
    (["--calib-bins", "10"], "go with --calibration"),
    (["--temperature", "2"], "go with --calibration"),
    (["--temperature", "fit", "--calibrate-on", "kitti120k"], "go with --calibration"),
    (["--calibrate-on", "kitti120k"], "go with --calibration"),
    (["--calibrate-scans", "4"], "go with --calibration"),
    (["--calibrate-files", "SemanticKITTI=/d"], "go with --calibration"),
    (["--calibrate-label-maps", "m.yaml"], "go with --calibration"),
    (["--calibration", "--temperature", "fit"], "exactly one calibration set"),
    (["--calibration", "--temperature", "fit", "--calibrate-on", "kitti120k", "--calibrate-files", "SemanticKITTI=/d",
      "--calibrate-label-maps", "m.yaml"], "exactly one calibration set"),
    (["--calibration", "--temperature", "0"], "positive"),
    (["--calibration", "--temperature", "-2"], "positive"),
    (["--calibration", "--temperature", "nan"], "positive"),
    (["--calibration", "--temperature", "0.001"], "0.01..100"),
    (["--calibration", "--temperature", "101"], "0.01..100"),
    (["--calibration", "--temperature", "warm"], "neither a number nor"),
    (["--calibration", "--calib-bins", "0"], "1..64"),
    (["--calibration", "--calib-bins", "65"], "1..64"),
    (["--calibration", "--calibrate-on", "kitti120k"], "go with --temperature fit"),
    (["--calibration", "--temperature", "2", "--calibrate-scans", "4"], "go with --temperature fit"),
    (["--calibration", "--temperature", "fit", "--calibrate-on", "kitti120k", "--calibrate-scans", "0"], "positive"),
    (["--calibration", "--temperature", "fit", "--calibrate-files", "SemanticKITTI=/d"], "go together"),
    (["--calibration", "--temperature", "fit", "--calibrate-files", "Nope=/d", "--calibrate-label-maps", "m.yaml"],
     "--calibrate-files"),
    (["--calibration", "--temperature", "fit", "--calibrate-files", "Synth4D-kitti=/d", "--calibrate-label-maps",
      "m.yaml"], "--synth4d-splits"),
    (["--calibration", "--temperature", "fit", "--calibrate-on", "nowhere"], "invalid choice"),
])
def test_refusals(extra, words, capsys):
    from lidog_amd import eval_target as T
    with pytest.raises(SystemExit):
        T.parse_args(CKPT + extra)
    assert words in capsys.readouterr().err


# ------------------------------------------------------------------ header, binding, library
def test_entry_points_in_header_binding_and_library():
    from lidog_amd import _lib, build
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    lib = ctypes.CDLL(build.build())
    for name in ENTRY_POINTS:
        assert f"{name}(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "calib.hip" in build.SOURCES
    vp, d, i32, i64 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int32, ctypes.c_int64
    S = _lib.SIGNATURES
    assert S["lidog_calib_ws"] == [i64] and _lib._RESTYPES["lidog_calib_ws"] is i64
    assert S["lidog_calib_stats"] == [vp, vp, i64, i32, i64, vp, i32, vp, vp, vp, vp, vp, vp]
    assert S["lidog_calib_fit_init"] == [vp, d, d, vp]
    assert S["lidog_calib_fit_step"] == [vp, vp, i64, i32, i64, d, d, vp, vp, vp, vp, vp]
    import re
    for k, name in enumerate(R.STATE):                          # the state layout is written down in the header
        tag = {"beta": "BETA", "nll": "NLL", "iterations": "ITER"}.get(name, name.upper())
        assert re.search(rf"#define LIDOG_CALIB_{tag} {k}\b", header), name
    assert re.search(r"#define LIDOG_CALIB_STATE 8\b", header)
    # refused on the host, before any launch (no device is needed to be told so)
    lib.lidog_calib_ws.restype = i64
    lib.lidog_calib_ws.argtypes = [i64]
    assert 2 <= lib.lidog_calib_ws(1) <= lib.lidog_calib_ws(10 ** 9) == 1 + 4 * 1024
    for fn, args in (("lidog_calib_stats", S["lidog_calib_stats"]), ("lidog_calib_fit_step", S["lidog_calib_fit_step"])):
        getattr(lib, fn).argtypes = args
    null = [None] * 6
    for C, B in ((1, 15), (33, 15), (7, 0), (7, 65)):
        assert lib.lidog_calib_stats(None, None, 10, C, -1, None, B, *null) == 2
    assert lib.lidog_calib_stats(None, None, 2 ** 31 // 7 + 1, 7, -1, None, 15, *null) == 2      # n C >= 2^31
    assert lib.lidog_calib_stats(None, None, 0, 7, -1, None, 15, *null) == 0                     # n == 0: nothing to do
    for C in (1, 33):
        assert lib.lidog_calib_fit_step(None, None, 10, C, -1, 0.01, 100.0, None, None, None, None, None) == 2
    assert lib.lidog_calib_fit_step(None, None, 10, 7, -1, 0.0, 100.0, None, None, None, None, None) == 2
    lib.lidog_calib_fit_init.argtypes = S["lidog_calib_fit_init"]
    assert lib.lidog_calib_fit_init(None, 0.01, 100.0, None) == 2


def test_public_names():
    import lidog_amd
    import torch
    from lidog_amd import calibration
    for name in ("CalibrationTable", "fit_temperature", "collect_logits", "metrics_from_table"):
        assert getattr(lidog_amd, name) is getattr(calibration, name)
    with pytest.raises(RuntimeError, match="GPU"):               # no CPU path behind the kernels
        calibration.CalibrationTable(device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        calibration.fit_temperature(torch.zeros(4, 7), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="n_bins"):
        calibration.CalibrationTable(n_bins=65)
