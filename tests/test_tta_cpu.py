"""Test-time augmentation without a GPU: the view names, the switches of eval_target and PointPath, the C ABI of
lidog_tta_vote and what its host side refuses before any launch."""
import ctypes
import os

import numpy as np
import pytest

import tta_ref as R
from helpers import REPO
from lidog_amd import evaluate, tta


# ------------------------------------------------------------------ views
def test_presets_expand_as_stated():
    assert [v.name for v in tta.parse_views(["rot4"])] == ["identity", "rotz90", "rotz180", "rotz270"]
    assert [v.name for v in tta.parse_views(["flip4"])] == ["identity", "flipx", "flipy", "flipx+flipy"]
    names = ["flipx", "rot4", "scale0.95", "rotz7.5+flipy"]
    views = tta.parse_views(names)
    assert [v.name for v in views] == R.expand(names)
    assert views[0].ops == [] and np.array_equal(views[0].matrix, np.eye(3))
    assert tta.parse_views([]) == [tta.View("identity")] and len(tta.parse_views([])) == 1
    assert tta.parse_views(views[1:]) == views                       # View objects pass through
    assert tta.MAX_VIEWS == 16 and tta.MODES == ("prob", "logit", "vote")


def test_ops_are_augment_points_operations():
    (v,) = tta.parse_views(["rotz30+flipx+scale0.5+flipy"])[1:]
    assert [a for a, _ in v.ops] == ["RandomRotation", "RandomScale", "RandomScale", "RandomScale"] and v.f64
    want = R.view_ops(v.name)
    for (_, got), (_, par) in zip(v.ops, want):
        assert got.dtype == np.float64 and np.array_equal(got, par)
    c, s = np.cos(np.radians(30.0)), np.sin(np.radians(30.0))
    assert np.array_equal(v.ops[0][1], np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]))
    assert np.array_equal(v.ops[1][1], [-1, 1, 1]) and np.array_equal(v.ops[2][1], [0.5, 0.5, 0.5])
    assert np.array_equal(v.ops[3][1], [1, -1, 1])
    assert not tta.View("flipx+scale0.95").f64 and not tta.View("identity").f64


@pytest.mark.parametrize("name,c,s", [("rotz90", 0, 1), ("rotz180", -1, 0), ("rotz270", 0, -1), ("rotz-90", 0, -1),
                                      ("rotz450", 0, 1), ("rotz-180.0", -1, 0)])
def test_right_angles_are_exact(name, c, s):
    m = tta.View(name).ops[0][1]
    want = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)
    assert m.tobytes() == (want + 0.0).tobytes()                     # no negative zero either
    assert set(np.abs(m).ravel().tolist()) == {0.0, 1.0}             # exactly 0 and +-1, not cos(pi / 2)
    assert np.array_equal(m, R.rotz(float(name[4:])))
    # rotz90 permutes coordinates exactly: (x, y, z) @ R = (y, -x, z)
    p = np.array([[0.1, -2.7, 3.3]], dtype=np.float32)
    if name == "rotz90":
        assert np.array_equal(R.transform(p, [("rot", m)]), np.array([[p[0, 1], -p[0, 0], p[0, 2]]], dtype=np.float64))


@pytest.mark.parametrize("names,word", [
    (["rotx90"], "rotx90"), (["flipz"], "flipz"), (["rotz"], "'rotz'"), (["rotz90+"], "''"), (["scale"], "'scale'"),
    (["rotz9o"], "rotz9o"), (["rotznan"], "rotznan"), (["rotzinf"], "rotzinf"),
    (["scale0"], "scale0"), (["scale-1.5"], "scale-1.5"), (["scalenan"], "scalenan"), (["scaleinf"], "scaleinf"),
    (["flipx+scale-2"], "scale-2"),
    (["identity"], "identity"), (["rotz0"], "rotz0"), (["rotz360"], "rotz360"), (["scale1"], "scale1"),
    (["flipx+flipx"], "flipx+flipx"), (["rotz90+rotz270"], "rotz90+rotz270"),
    (["flipx", "flipx"], "flipx"), (["rot4", "rotz180"], "rotz180"), (["rotz270", "rotz-90"], "rotz-90"),
    (["rot4", "flip4"], "flipx+flipy"),                              # = rotz180: the same matrix
    (["rotz1+rotz2+rotz3+rotz4+rotz5"], "atoms"),
    ([f"rotz{d}" for d in range(1, 17)], "rotz16"),
])
def test_refused_views_name_the_offender(names, word):
    with pytest.raises(ValueError, match="tta") as e:
        tta.parse_views(names)
    assert word in str(e.value)


def test_sixteen_views_are_taken():
    assert len(tta.parse_views([f"rotz{d}" for d in range(1, 16)])) == 16


# ------------------------------------------------------------------ switches
BASE = ["--checkpoint", "c.ckpt", "--target-files", "SemanticKITTI=/data/kitti", "--label-maps", "map.yaml"]


def test_eval_target_arguments(capsys):
    from lidog_amd import eval_target as T
    a = T.parse_args(BASE + ["--point-level"])
    assert a.tta is None and a.tta_mode == "prob"
    a = T.parse_args(BASE + ["--point-level", "--tta", "rot4"])
    assert a.tta == ["rot4"] and a.tta_mode == "prob"
    a = T.parse_args(BASE + ["--save-labels", "--tta", "flipx", "flipy", "scale0.95", "--tta-mode", "logit"])
    assert a.tta == ["flipx", "flipy", "scale0.95"] and a.tta_mode == "logit"
    assert T.parse_args(BASE + ["--point-level", "--tta", "rot4", "--tta-mode", "vote"]).tta_mode == "vote"
    for argv, word in ((BASE + ["--tta", "rot4"], "--tta goes with"),
                       (["--checkpoint", "c.ckpt", "--tta", "rot4"], "--tta goes with"),
                       (BASE + ["--point-level", "--tta", "rot4", "--point-interp", "trilinear"], "nearest"),
                       (BASE + ["--point-level", "--tta-mode", "vote"], "--tta-mode goes with --tta"),
                       (BASE + ["--point-level", "--tta-mode", "prob"], "--tta-mode goes with --tta"),
                       (BASE + ["--point-level", "--tta", "rot4", "--tta-mode", "mean"], "invalid choice"),
                       (BASE + ["--point-level", "--tta"], "expected at least one argument"),
                       (BASE + ["--point-level", "--tta", "rotx90"], "rotx90"),
                       (BASE + ["--point-level", "--tta", "rot4", "rotz-90"], "rotz-90")):
        with pytest.raises(SystemExit):
            T.parse_args(argv)
        assert word in capsys.readouterr().err, argv


def test_point_path_arguments():
    items = lambda ids: []                                           # noqa: E731
    p = evaluate.PointPath(items)
    assert p.tta is None and p.tta_mode == "prob"
    assert evaluate.PointPath(items, tta=[]).tta is None and evaluate.PointPath(items, tta=None).tta is None
    p = evaluate.PointPath(items, tta=["rot4"], tta_mode="vote")
    assert [v.name for v in p.tta] == ["identity", "rotz90", "rotz180", "rotz270"] and p.tta_mode == "vote"
    assert evaluate.PointPath(items, tta=[tta.View("flipy")]).tta[1].name == "flipy"
    with pytest.raises(ValueError, match="trilinear"):
        evaluate.PointPath(items, interp="trilinear", tta=["rot4"])
    assert evaluate.PointPath(items, interp="trilinear", tta=[]).interp == "trilinear"
    with pytest.raises(ValueError, match="tta_mode"):
        evaluate.PointPath(items, tta=["rot4"], tta_mode="mean")
    with pytest.raises(ValueError, match="tta_mode"):
        evaluate.PointPath(items, tta_mode="softmax")
    with pytest.raises(ValueError, match="flipz"):
        evaluate.PointPath(items, tta=["flipz"])


# ------------------------------------------------------------------ C ABI
def test_vote_symbol_exported_bound_and_refusing():
    from lidog_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    assert hasattr(lib, "lidog_tta_vote") and "lidog_tta_vote" in _lib.SIGNATURES and "lidog_tta_vote(" in header
    assert len(_lib.SIGNATURES["lidog_tta_vote"]) == 10
    assert _lib.ABI_VERSION == 9 and lib.lidog_abi_version() == 9          # additive entries: the version stays
    assert "tta.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "tta.hip"))
    # arguments are refused on the host, before any launch (every pointer is NULL here)
    lib.lidog_last_error.restype = ctypes.c_char_p
    i64, i32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p

    def vote(m, c, k, mode):
        return lib.lidog_tta_vote(vp(), i64(m), i32(c), vp(), i64(k), i32(mode), i32(1), vp(), vp(), vp())

    for args, word in (((10, 33, 10, 0), b"33 classes"), ((10, 0, 10, 0), b"0 classes"), ((10, -1, 10, 1), b"-1 classes"),
                       ((10, 7, 10, 3), b"mode = 3"), ((10, 7, 10, -1), b"mode = -1"),
                       ((10, 7, -1, 0), b"-1 points"), ((-2, 7, 10, 0), b"-2 rows"),
                       ((10, 33, 0, 0), b"33 classes"), ((10, 7, 0, 5), b"mode = 5")):       # k = 0 is no excuse
        assert vote(*args) == 2, args
        assert word in lib.lidog_last_error(), (args, lib.lidog_last_error())
    assert vote(10, 7, 0, 0) == 0 and vote(0, 32, 0, 2) == 0                # k = 0 launches nothing
    assert vote(10, 7, 10, 0) == 2 and b"null argument" in lib.lidog_last_error()


def test_vote_wrapper_refuses_on_the_host():
    import torch
    with pytest.raises(ValueError, match="mode"):
        tta.vote(torch.zeros(2, 7), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 7), mode="mean")
    with pytest.raises(RuntimeError, match="GPU"):
        tta.vote(torch.zeros(2, 7), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 7))


# ------------------------------------------------------------------ the restatement itself
def test_reference_modes_and_rows():
    x = np.array([[1.0, 3.0, 3.0], [np.nan, 5.0, np.nan], [0.0, -np.inf, 0.0]], dtype=np.float32)
    assert R.first_argmax(x).tolist() == [1, 0, 0]
    assert np.array_equal(R.scores(x, "vote"), np.eye(3)[[1, 0, 0]])
    p = R.scores(x, "prob")
    assert np.allclose(p[0], np.exp([-2.0, 0, 0]) / (2 + np.exp(-2.0))) and np.isnan(p[1]).all()
    assert np.array_equal(p[2], [0.5, 0.0, 0.5])
    acc = R.vote([(x[:1], [0, 0]), (x[2:], [0, 0])], "logit")
    assert np.array_equal(acc, np.array([[1.0, -np.inf, 3.0]] * 2))
    # points on faces, negative coordinates: the float32 floor of the float32 quotient, a flip in float32
    pts = np.array([[0.05, -0.05, 0.0], [-0.024, 0.1, -1.0]], dtype=np.float32)
    rows = R.view_rows(pts, R.view_ops("flipx"), 0.05, batch=3)
    want = np.floor((pts * np.float32([-1, 1, 1])) / np.float32(0.05)).astype(np.int32)
    assert rows.dtype == np.int32 and np.array_equal(rows[:, 0], [3, 3]) and np.array_equal(rows[:, 1:], want)
    assert R.transform(pts, R.view_ops("rotz90")).dtype == np.float64
    assert R.transform(pts, R.view_ops("scale0.95+flipy")).dtype == np.float32
    assert R.prob_bound(3, 7) == 3 * 14 * 2.0 ** -24
