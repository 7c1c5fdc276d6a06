"""The training augmentation (sub_p / augmentation_list) without a GPU: the G13 fixture covers what it has to, the host's
draws replay the reference's random sequence, augment_ref's numpy restatement reproduces every recorded output under the
fixture's rules (integers exactly, float64 xyz within the bound of the arithmetic, face / threshold margins on every
input), the command line, the dataset class's draws, the synthetic per-point labels, the C ABI."""
import ctypes
import os
import sys

import numpy as np
import pytest

import augment_ref as A
from helpers import REPO
from lidog_amd import data, synth
from lidog_amd.train import AugmentedSynthScans, parse_args

META, G13 = A.load_g13()
CASES = sorted(A.CASES)
AUG_SYMBOLS = ("lidog_augment_is_f64", "lidog_augment_ws", "lidog_augment_points")


def _bev(case):
    return A.BEV if case["form"] == "bev" else None


# ------------------------------------------------------------------ the fixture
def test_g13_covers_the_cases():
    assert os.path.getsize(A.G13) <= 300 * 1024
    assert set(META["cases"]) == set(A.CASES)
    cases = list(A.CASES.values())
    for cfg in ("kitti120k", "nusc35k"):
        assert {c["form"] for c in cases if c["config"] == cfg} == {"bev", "plain"}
    lists = {tuple(c["augs"]) for c in cases}
    assert lists == {(A.ROT, A.SCALE), (A.ROT,), (A.SCALE,), (A.SCALE, A.ROT), ()}
    assert any(c["sub_p"] is None for c in cases) and {c["bev_from"] for c in cases} == {"voted", "first"}
    assert len({c["seed"] for c in cases}) == len(cases)
    recs = META["cases"]
    assert all(r["outcome"] == "ok" for r in recs.values())      # the reference returns an empty item, it does not raise
    assert recs["kitti_bev_none_kept"]["kept"] == 0 and recs["kitti_bev_none_kept"]["voxels"] == 0
    assert recs["kitti_bev_ego_box"]["kept"] < 0.7 * recs["kitti_bev_ego_box"]["sampled"]
    assert recs["nusc_bev_ego_box"]["kept"] < 0.7 * recs["nusc_bev_ego_box"]["sampled"]
    for name, r in recs.items():
        assert r["xyz_dtype"] == ("float64" if A.ROT in r["augs"] else "float32"), name
        if r["kept"]:
            assert r["voxels"] < r["kept"] or "ego" in name, name        # several points per voxel: the order matters
    assert sum(r["voted_ignore"] for r in recs.values()) > 100       # the vote changes labels


@pytest.mark.parametrize("name", CASES)
def test_margins_hold(name):
    """no transformed coordinate within 1e-9 voxel of a voxel face or 1e-9 m of a bounds threshold"""
    case = A.CASES[name]
    pts, _, _ = A.case_input(case)
    draws = A.case_draws(name, G13)
    p, _ = A.transform_np(pts[draws["sampled_idx"]], draws["ops"])
    face, thr = A.margins(p, A.VOXEL, case["form"] == "bev")
    assert face > A.MARGIN and thr > A.MARGIN, (face, thr)


# ------------------------------------------------------------------ the draws
@pytest.mark.parametrize("name", CASES)
def test_draws_replay_the_reference_sequence(name):
    case, rec = A.CASES[name], META["cases"][name]
    want = A.case_draws(name, G13)
    np.random.seed(case["seed"])
    got = data.draw_augmentation(np.random, rec["rows_in"], case["sub_p"], case["augs"])
    assert float(np.random.rand()) == rec["next_rand"]              # as many draws as the reference makes
    assert got["sampled_idx"].dtype == np.int64 and np.array_equal(got["sampled_idx"], want["sampled_idx"])
    assert [a for a, _ in got["ops"]] == case["augs"]
    for (a, g), (_, w) in zip(got["ops"], want["ops"]):
        assert g.dtype == np.float64
        assert np.array_equal(g, w), (a, np.abs(g - w).max())       # scipy imports here: R is expm's, bit for bit
    rs = np.random.RandomState(case["seed"])                        # a RandomState of its own draws the same
    again = data.draw_augmentation(rs, rec["rows_in"], case["sub_p"], case["augs"])
    assert np.array_equal(again["sampled_idx"], want["sampled_idx"]) and float(rs.rand()) == rec["next_rand"]


def test_rotation_closed_form_without_scipy(monkeypatch):
    want = [(n, G13[f"{n}__R"]) for n in CASES if f"{n}__R" in G13]
    assert len(want) >= 10
    monkeypatch.setitem(sys.modules, "scipy.linalg", None)          # `from scipy.linalg import ...` raises ImportError
    for name, R in want:
        np.random.seed(A.CASES[name]["seed"])
        got = data.draw_augmentation(np.random, META["cases"][name]["rows_in"], A.CASES[name]["sub_p"],
                                     A.CASES[name]["augs"])
        mine = [p for a, p in got["ops"] if a == A.ROT][0]
        assert np.abs(mine - R.reshape(3, 3)).max() <= 1e-15
        assert float(np.random.rand()) == META["cases"][name]["next_rand"]


def test_sub_p_none_and_permutation_prefix():
    rs = np.random.RandomState(5)
    d = data.draw_augmentation(rs, 1000, None, [])
    assert np.array_equal(d["sampled_idx"], np.arange(1000)) and d["ops"] == []
    assert float(rs.rand()) == float(np.random.RandomState(5).rand())       # nothing was drawn
    d = data.draw_augmentation(np.random.RandomState(6), 1001, 0.8, [])
    assert np.array_equal(d["sampled_idx"], np.random.RandomState(6).permutation(1001)[:800])
    assert data.draw_augmentation(np.random.RandomState(6), 1, 0.8, [])["sampled_idx"].shape == (0,)
    with pytest.raises(NotImplementedError):
        data.draw_augmentation(np.random.RandomState(6), 10, 0.8, ["RandomShear"])


# ------------------------------------------------------------------ the restatement against the fixture
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_g13(name):
    case = A.CASES[name]
    pts, feats, labels = A.case_input(case)
    got = A.augment_np(pts, feats, labels, A.case_draws(name, G13), A.VOXEL, case["form"] == "bev", A.IGNORE, _bev(case),
                       case["bev_from"])
    want = A.case_outputs(name, G13)
    assert set(want) == set(A.INT_OUTPUTS if case["form"] == "bev" else A.INT_OUTPUTS[:-2]) | {"xyz", "features"}
    A.compare(got, want, got["_xyz_bound"], name)
    assert (got["_xyz_bound"] is None) == (A.ROT not in case["augs"])


def test_dtype_rules_decide_results():
    """the float32 round trip of a scale without a rotation, and float64 after one, are visible in the fixture's inputs"""
    pts, _, _ = A.case_input(A.CASES["kitti_plain_scale"])
    s = G13["kitti_plain_scale__scale"].reshape(3)
    p32, mag = A.transform_np(pts, [(A.SCALE, s)])
    assert p32.dtype == np.float32 and mag is None
    assert np.array_equal(p32, (pts.astype(np.float64) * s).astype(np.float32))
    assert not np.array_equal(p32, pts * s.astype(np.float32))              # a float32 product is another number
    R = G13["kitti_plain_rot_scale__R"].reshape(3, 3)
    p64, mag = A.transform_np(pts, [(A.SCALE, s), (A.ROT, R)])
    assert p64.dtype == np.float64 and mag.shape == p64.shape
    blas = p32 @ R
    assert np.abs(blas - p64).max() > 0 and (np.abs(blas - p64) <= A.xyz_bound(mag)).all()


# ------------------------------------------------------------------ the command line
def test_command_line():
    assert parse_args([]).augment is None
    assert parse_args(["--augment"]).augment == []
    a = parse_args(["--augment", "RandomScale", "RandomRotation", "--sub-p", "0.5", "--model", "MinkUNet34"])
    assert a.augment == ["RandomScale", "RandomRotation"] and a.sub_p == 0.5
    assert parse_args(["--augment", "RandomRotation", "--sources", "kitti120k", "nusc35k"]).sources == ["kitti120k", "nusc35k"]
    with pytest.raises(NotImplementedError):
        parse_args(["--augment", "RandomShear"])
    with pytest.raises(NotImplementedError):
        parse_args(["--augment", "RandomRotation", "RandomTranslation"])
    for extra in (["--mix", "cosmix", "--model", "MinkUNet34"], ["--mix3d"],
                  ["--sn-targets", "nusc35k_cars", "--model", "MinkUNet34"]):
        with pytest.raises(SystemExit):
            parse_args(["--augment", "RandomRotation"] + extra)


# ------------------------------------------------------------------ the dataset class
def _same(a, b):
    return (np.array_equal(a["sampled_idx"], b["sampled_idx"]) and [n for n, _ in a["ops"]] == [n for n, _ in b["ops"]]
            and all(np.array_equal(p, q) for (_, p), (_, q) in zip(a["ops"], b["ops"])))


def test_dataset_draws_do_not_depend_on_batching_or_replay():
    augs = ["RandomRotation", "RandomScale"]
    d0 = AugmentedSynthScans(6, "source8k", augs, seed=3)
    d1 = AugmentedSynthScans(6, "source8k", augs, seed=3)
    d0.set_epoch(1)
    d1.set_epoch(1)
    fwd = {i: d0.item(i) for i in range(6)}
    for i in (5, 2, 0, 3, 1, 4):                                    # another order, as another batch split visits them
        (s, j, draws), = d1.item(i)
        assert (s, j) == (0, i) and _same(draws, fwd[i][0][2])
    first = d0.item(2)[0][2]
    d0.set_epoch(0)
    other = d0.item(2)[0][2]
    assert not np.array_equal(other["sampled_idx"], first["sampled_idx"])       # another epoch, other draws
    d0.set_epoch(1)
    assert _same(d0.item(2)[0][2], first)                           # a resume replays the epoch
    assert not _same(AugmentedSynthScans(6, "source8k", augs, seed=4).item(2)[0][2], other)
    n = synth.scan_points_labels(2, "source8k")[0].shape[0]
    assert first["sampled_idx"].shape == (int(0.8 * n),) and len(set(first["sampled_idx"].tolist())) == int(0.8 * n)


def test_dataset_two_sources_and_refusals():
    d = AugmentedSynthScans(3, ("source8k", "source8k"), ["RandomScale"], seed=1, sub_p=None)
    assert d.num_sources == 2 and len(d) == 3
    (s0, j0, a), (s1, j1, b) = d.item(1)
    assert (s0, s1) == (0, 1) and (j0, j1) == d.pairs.pair(1)
    assert not np.array_equal(a["ops"][0][1], b["ops"][0][1])       # one generator, source 0 first
    rs = d.item_rng(1)
    assert np.array_equal(a["ops"][0][1], np.concatenate([0.2 * rs.rand(1) + 0.9 for _ in range(3)]))
    assert not np.array_equal(d.points(0, 0)[0], d.points(1, 0)[0])
    with pytest.raises(NotImplementedError):
        AugmentedSynthScans(3, "source8k", ["RandomShear"])
    with pytest.raises(NotImplementedError):
        AugmentedSynthScans(3, ("source8k",) * 3, [])


def test_hand_over_walks_nested_batches():
    """on_merge_stream's walk over what crosses streams: nested dicts, lists and tuples; host tensors and others skipped"""
    import torch
    a, b, c = torch.zeros(1), torch.zeros(2), torch.zeros(3)
    assert data._device_tensors({"x": a, "bev": {"block8": b}, "l": [c, (a, 5, "s")], "n": None}) == []    # no device here

    class Fake:
        is_cuda = True

    f, g = Fake(), Fake()
    real = torch.is_tensor
    try:
        torch.is_tensor = lambda o: isinstance(o, Fake) or real(o)
        got = data._device_tensors({"x": f, "bev": {"block8": g}, "l": [a, (f, 5, "s")], "n": None})
    finally:
        torch.is_tensor = real
    assert got == [f, g, f]


# ------------------------------------------------------------------ synthetic per-point labels
@pytest.mark.parametrize("config", ["kitti120k", "nusc35k", "kitti120k_cars"])
def test_scan_points_labels(config):
    before = synth.scan_voxels(0, config)
    pts, labels = synth.scan_points_labels(0, config)
    again = synth.scan_points_labels(0, config)
    after = synth.scan_voxels(0, config)
    assert np.array_equal(pts, again[0]) and np.array_equal(labels, again[1])
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert pts.dtype == np.float32 and labels.dtype == np.int64 and labels.shape == (pts.shape[0],)
    assert labels.min() == -1 and labels.max() <= 6
    if "cars" not in config:
        assert np.array_equal(pts, synth.scan_points(0, **synth.CONFIGS[config])[0])
    else:
        assert (labels == synth.CAR_CLASS).any()
    assert not np.array_equal(labels, synth.scan_points_labels(1, config)[1][:labels.shape[0]])
    cfg = synth.CONFIGS[config]
    feats = np.ones((pts.shape[0], 1), np.float32)
    item = A.augment_np(pts, feats, labels, {"sampled_idx": np.arange(pts.shape[0]), "ops": []}, cfg["voxel"],
                        cfg["lidog_bounds"])
    assert np.array_equal(item["coordinates"], before[0])           # the same voxels as scan_voxels
    share = float((item["voted_labels"] != -1).mean())
    assert 0.85 < share < 0.97, share                               # coherent: the vote leaves most voxels labelled
    if config == "kitti120k":
        assert abs(share - 0.9192) < 5e-4                           # the share DESIGN.md states for seed 0


# ------------------------------------------------------------------ C ABI
def test_augment_symbols_exported_and_bound():
    from lidog_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    for name in AUG_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f"{name}(" in header
    assert _lib.ABI_VERSION == 9 and lib.lidog_abi_version() == 9          # additive entries: the version stays
    kinds = (ctypes.c_int32 * 2)(1, 0)
    assert lib.lidog_augment_is_f64(kinds, 2) == 1 and lib.lidog_augment_is_f64(kinds, 1) == 0
    lib.lidog_augment_ws.restype = ctypes.c_int64
    assert lib.lidog_augment_ws(ctypes.c_int64(0)) >= 3 and lib.lidog_augment_ws(ctypes.c_int64(5000)) >= 10003
    assert "augment.hip" in build.SOURCES
