"""The Raycast baseline without a GPU: the numpy restatement of the definition (raycast_ref) against brute force and on
hand-made cases, the sensors, the command line, the C ABI, the Fake dataset writer and readers (the device part of the
writer stubbed by the restatement), and the conditions the GPU tests' realistic cases rest on."""
import json
import os
import re

import numpy as np
import pytest

import raycast_ref as RR
import scans_ref as R
from lidog_amd import raycast, scans, synth
from lidog_amd.train import parse_args

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lidog_raycast_ws", "lidog_raycast")


def _ray(az, el, r):
    az, el, r = np.broadcast_arrays(np.asarray(az, np.float64), np.asarray(el, np.float64), np.asarray(r, np.float64))
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=1).astype(np.float32)


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("config", ["nusc35k", "source8k"])
def test_identity_keeps_every_point(config):
    """a synthetic scan resampled to its own sensor from its own position: every point has a cell of its own"""
    pts, _ = synth.scan_points_labels(0, config)
    ref = RR.raycast_ref(pts, raycast.sensor(config), None, snap=False)
    assert ref.occupied == pts.shape[0] and not ref.ambiguous.any()
    assert np.array_equal(np.sort(ref.rows), np.arange(pts.shape[0]))
    assert np.array_equal(ref.points.view(np.uint32), pts[ref.rows].view(np.uint32))
    snapped = RR.raycast_ref(pts, raycast.sensor(config), None, snap=True)
    # on its cell's ray the point keeps its range: it moves by at most the range noise times the angle to the ray
    assert np.array_equal(snapped.rows, ref.rows) and np.abs(snapped.points - pts[ref.rows]).max() < 1e-4


def test_winners_equal_brute_force():
    rng = np.random.default_rng(3)
    spec = RR.spec_like(np.deg2rad([-20.0, -11.0, -4.0, 0.0, 9.0]), 12, az0=0.3, min_range=1.0, max_range=30.0)
    pts = _ray(rng.uniform(-np.pi, np.pi, 3000), np.deg2rad(rng.uniform(-30, 16, 3000)), rng.uniform(0.5, 35.0, 3000))
    origin = np.array([0.3, -0.2, 0.1], np.float32)
    ref = RR.raycast_ref(pts, spec, origin, snap=False)
    want = RR.brute_force_winners((pts - origin).astype(np.float32), ref.cells)
    assert 0 < ref.occupied <= 60 and (ref.cells == -1).any()
    assert np.all(np.diff(ref.out_cells) > 0) and ref.out_cells.tolist() == sorted(want)
    assert ref.rows.tolist() == [want[c] for c in sorted(want)]
    assert np.array_equal(ref.cells[ref.rows], ref.out_cells)


def test_tie_goes_to_the_smallest_row():
    spec = RR.spec_like(np.deg2rad([-10.0, 10.0]), 4)
    one = _ray([0.1], [0.05], [7.0])
    pts = np.concatenate([_ray([0.1], [0.05], [9.0]), one, one, one, _ray([0.1], [0.05], [8.0])])
    ref = RR.raycast_ref(pts, spec, snap=False)
    assert ref.rows.tolist() == [1] and ref.cells.tolist() == [4] * 5


def test_range_and_fov_drops():
    spec = RR.spec_like(np.deg2rad([-10.0, 0.0, 10.0]), 8, min_range=2.0, max_range=20.0)
    pts = np.concatenate([_ray(0.0, 0.0, [0.0, 1.0, 2.0, 19.99, 20.0, 25.0]),      # the origin, near, on min, far
                          _ray(1.0, np.deg2rad([-15.1, -14.9, 14.9, 15.1]), 5.0),    # around the outer edges
                          np.array([[0, 0, 5.0], [0, 0, -5.0]], np.float32)])         # on the z axis: outside
    ref = RR.raycast_ref(pts, spec)
    assert (ref.cells >= 0).tolist() == [False, False, True, True, False, False, False, True, True, False, False, False]
    assert ref.cells[7] // 8 == 0 and ref.cells[8] // 8 == 2 and ref.cells[2] == 8
    # float32(2.0)^2 == 4 exactly: r2 < min2 is false on the limit, r2 >= max2 is true on it
    assert np.float32(pts[2, 0]) ** 2 == np.float32(4.0)


def test_edges_of_a_non_uniform_table():
    el = np.deg2rad([-25.0, -10.0, -4.0, 0.0, 3.0])
    spec = raycast.SensorSpec(el, 10)
    want = np.deg2rad([-32.5, -17.5, -7.0, -2.0, 1.5, 4.5])
    np.testing.assert_allclose(spec.edges(), want, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(spec.edges(), RR.edges_of(el))
    edges, cos_el, sin_el, cos_az, sin_az = spec.host_tables()
    assert all(t.dtype == np.float64 for t in (edges, cos_el, sin_el, cos_az, sin_az))
    assert cos_el.shape == (5,) and cos_az.shape == (10,) and cos_az[0] == 1.0 and sin_az[0] == 0.0
    for bad in ([0.1], [0.2, 0.1], [0.1, 0.1], [0.0, np.nan], [-2.0, 0.0]):
        with pytest.raises(ValueError):
            raycast.SensorSpec(np.array(bad), 10)
    with pytest.raises(ValueError):
        raycast.SensorSpec(el, 0)
    with pytest.raises(ValueError):
        raycast.SensorSpec(el, 10, min_range=5.0, max_range=5.0)


def test_built_in_sensors_and_origin():
    assert set(raycast.SENSORS) == set(synth.CONFIGS) | {"hdl32e"}
    for name, cfg in synth.CONFIGS.items():
        s = raycast.sensor(name)
        assert (s.n_beams, s.n_az, s.az0, s.min_range, s.max_range) == (cfg["n_beams"], cfg["n_az"], 0.0, 0.0, None)
        np.testing.assert_array_equal(s.elevations, np.deg2rad(np.linspace(*cfg["elev"], cfg["n_beams"])))
    h = raycast.sensor("hdl32e")
    assert (h.n_beams, h.n_az) == (32, 1090)
    np.testing.assert_allclose(np.rad2deg(h.elevations[[0, -1]]), [-30.67, 10.67], rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.diff(h.elevations), np.deg2rad(41.34 / 31), rtol=0, atol=1e-12)
    o = raycast.origin_between("kitti120k", "nusc35k")
    assert o.dtype == np.float32 and o.tolist() == [0.0, 0.0, float(np.float32(1.84 - 1.73))]
    assert raycast.origin_between("nusc35k", "kitti120k")[2] == -o[2]
    with pytest.raises(ValueError, match="HDL-64E"):
        raycast.sensor("hdl64e")


def test_json_sensor_round_trip(tmp_path):
    spec = raycast.SensorSpec(np.deg2rad([-25.0, -10.0, -4.0, 0.1, 3.0]), 77, az0=0.01, min_range=1.5, max_range=80.0,
                              name="odd")
    path = str(tmp_path / "odd.json")
    with open(path, "w") as f:
        json.dump(spec.to_json(), f)
    back = raycast.sensor(path)
    np.testing.assert_array_equal(back.elevations, spec.elevations)
    assert (back.n_az, back.az0, back.min_range, back.max_range, back.name) == (77, 0.01, 1.5, 80.0, "odd")
    with open(path, "w") as f:
        json.dump({"elevations_deg": [-10, 0, 10], "n_az": 36}, f)
    plain = raycast.sensor(path)
    np.testing.assert_array_equal(plain.elevations, np.deg2rad(np.array([-10.0, 0.0, 10.0])))
    assert (plain.n_az, plain.az0, plain.min_range, plain.max_range, plain.name) == (36, 0.0, 0.0, None, "odd")
    with open(path, "w") as f:
        json.dump({"n_az": 36}, f)
    with pytest.raises(ValueError):
        raycast.sensor(path)


# ------------------------------------------------------------------ the command line
def test_cli_shape_of_the_raycast_configs(tmp_path):
    a = parse_args(["--model", "MinkUNet34", "--config", "kitti120k", "--raycast-to", "nusc35k", "--lr", "0.01",
                    "--scheduler", "ExponentialLR"])
    assert a.raycast_to == "nusc35k" and a.augment is None and a.mix is None and not hasattr(a, "raycast_origin")
    b = parse_args(["--model", "MinkUNet34", "--raycast-to", "hdl32e", "--raycast-origin", "0", "0", "0.5",
                    "--augment", "RandomRotation", "RandomScale"])
    assert b.raycast_origin == [0.0, 0.0, 0.5] and b.augment == ["RandomRotation", "RandomScale"]
    assert not hasattr(parse_args([]), "raycast_to")
    path = str(tmp_path / "s.json")
    with open(path, "w") as f:
        json.dump(RR.sensor_8x125().to_json(), f)
    assert parse_args(["--raycast-to", path]).raycast_to == path


@pytest.mark.parametrize("argv", [["--model", "MinkUNet34", "--raycast-to", "nusc35k", "--mix", "cosmix"],
                                  ["--model", "MinkUNet34", "--raycast-to", "nusc35k", "--mix3d"],
                                  ["--model", "MinkUNet34", "--config", "kitti120k_cars", "--raycast-to", "nusc35k",
                                   "--sn-targets", "nusc35k_cars"]])
def test_cli_raycast_with_another_method_is_refused(argv, capsys):
    with pytest.raises(SystemExit):
        parse_args(argv)
    assert "different methods" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--model", "MinkUNet34", "--mix", "raycast"], ["--raycast-to", "no-such-sensor"],
                                  ["--raycast-origin", "0", "0", "1"]])
def test_cli_refusals(argv, capsys):
    with pytest.raises(SystemExit):
        parse_args(argv)


def test_datasets_take_raycast_only_for_training():
    from lidog_amd.train import AugmentedSynthScans
    ds = AugmentedSynthScans(4, "kitti120k", None, raycast="nusc35k")
    assert ds.augmentations is None and ds.raycast is raycast.SENSORS["nusc35k"]
    assert ds.raycast_origins[0].tolist() == raycast.origin_between("kitti120k", "nusc35k").tolist()
    assert ds.draws(ds.item_rng(0), 5)["sampled_idx"].tolist() == [0, 1, 2, 3, 4] and ds.draws(None, 5)["ops"] == []
    assert AugmentedSynthScans(4, "kitti120k", None, raycast=RR.sensor_8x125()).raycast_origins == [None]
    with pytest.raises(TypeError):
        AugmentedSynthScans(4, "kitti120k", None)                  # without raycast a list is still required
    val = scans.Listing("SemanticKITTI", [], "validation")
    with pytest.raises(ValueError, match="raycast"):
        scans.FileScans(val, np.zeros(4, np.int32), raycast="nusc35k")
    assert scans.FileScans(scans.Listing("SemanticKITTI", [], "train"), np.zeros(4, np.int32),
                           raycast="nusc35k").raycast is raycast.SENSORS["nusc35k"]


# ------------------------------------------------------------------ C ABI
def test_raycast_symbols_are_declared_bound_and_exported():
    from lidog_amd import _lib, build
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    lib = __import__("ctypes").CDLL(build.build())
    for name in SYMBOLS:
        decl = re.search(rf"\b{name}\(([^;]*)\);", header)
        assert decl, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    assert "raycast.hip" in build.SOURCES and "lidog_raycast_ws" in _lib._RESTYPES
    assert _lib.ABI_VERSION == 9 and lib.lidog_abi_version() == 9          # additive entries: the version stays
    for name in ("SensorSpec", "SENSORS", "sensor", "origin_between", "raycast_points", "raycast_scan", "write_fake"):
        assert hasattr(raycast, name), name


# ------------------------------------------------------------------ writer -> reader
def _stub(monkeypatch):
    def resample_file(points, labels_raw, spec, origin=None, snap=True, device="cuda"):
        ref = RR.raycast_ref(points, spec, origin, snap)
        return ref.points, np.asarray(labels_raw)[ref.rows]
    monkeypatch.setattr(raycast, "resample_file", resample_file)


def test_writer_reader_round_trip(tmp_path, monkeypatch):
    """the device part of the writer replaced by the restatement: the layout, the dtypes and the listings"""
    _stub(monkeypatch)
    _, g15 = R.load_g15()
    trees = R.write_trees(str(tmp_path / "src"), R.fixture_maps(g15))
    spec = raycast.sensor("source8k")
    kw = dict(version="mini", synth4d_splits=trees["splits"])
    for name, fake in raycast.FAKE_OF.items():
        out = str(tmp_path / fake)
        for phase in scans.PHASES:
            src = scans.listing(name, R.tree_root(trees, name), phase, **kw)
            if name == "Synth4D-nuscenes" and phase == "train":        # this tree holds negative raw ids
                with pytest.raises(ValueError, match="int8"):
                    raycast.write_fake(src, spec, out)
                continue
            assert raycast.write_fake(src, spec, out) == len(src)
            back = scans.listing(fake, out, phase, **kw)
            assert len(back) == len(src) and back.format["stride"] == 4
            assert back.format["radius"] == (fake == "FakeKITTI")
            for (sp, sl), (bp, bl) in zip(src.files, back.files):
                raw_p, raw_l, stride = scans.read_files(src.format, sp, sl)
                xyz = raw_p.view(np.float32).reshape(-1, stride)[:, :3] if raw_p.dtype == np.uint8 else raw_p[:, :3]
                ref = RR.raycast_ref(xyz, spec)
                got_p, got_l, got_stride = scans.read_files(back.format, bp, bl)
                rec = got_p.view(np.float32).reshape(-1, 4)
                assert got_stride == 4 and 0 < ref.occupied < xyz.shape[0]
                assert np.array_equal(rec[:, :3].view(np.uint32), ref.points.view(np.uint32)) and not rec[:, 3].any()
                if raw_l is None:                                         # no label file in, none out
                    assert got_l is None and not os.path.exists(bl)
                    continue
                assert got_l.dtype == (np.uint8 if fake == "FakeSynth4D-nuscenes" else np.int32)
                assert np.array_equal(got_l.astype(np.int64), raw_l.astype(np.int64)[ref.rows])     # the RAW words
                assert os.path.getsize(bl) == ref.occupied * got_l.dtype.itemsize
    assert os.path.exists(os.path.join(str(tmp_path / "FakeKITTI"), "sequences", "00", "velodyne", "000001.bin"))
    assert os.path.exists(os.path.join(str(tmp_path / "FakeSynth4D-kitti"), "Town06", "labels", "000010.label"))
    with pytest.raises(ValueError):
        raycast.write_fake(scans.listing("nuScenes", trees["nuScenes"], "train"), spec, str(tmp_path / "no"))


def test_writer_command_line(tmp_path, monkeypatch, capsys):
    _stub(monkeypatch)
    _, g15 = R.load_g15()
    root = R.write_kitti_tree(str(tmp_path / "kitti"), R.fixture_maps(g15))
    out = str(tmp_path / "fake")
    raycast.main(["--files", f"SemanticKITTI={root}", "--raycast-to", "source8k", "--out", out, "--version", "mini",
                  "--phases", "train", "--limit-files", "2"])
    assert "FakeKITTI train: 2 scans" in capsys.readouterr().out
    assert sorted(os.listdir(os.path.join(out, "sequences", "00", "velodyne"))) == ["000000.bin", "000001.bin"]
    assert not os.path.exists(os.path.join(out, "sequences", "08"))
    for argv in (["--files", f"nuScenes={root}", "--raycast-to", "source8k", "--out", out],
                 ["--files", f"Synth4D-kitti={root}", "--raycast-to", "source8k", "--out", out],
                 ["--files", f"SemanticKITTI={root}", "--raycast-to", "hdl64e", "--out", out]):
        with pytest.raises(SystemExit):
            raycast.parse_args(argv)
    a = parse_args(["--files", f"FakeKITTI={out}", "--label-maps", "m.json", "--raycast-to", "nusc35k",
                    "--raycast-origin", "0", "0", "0.1"])
    assert a.files == [("FakeKITTI", out)] and a.raycast_to == "nusc35k"
    with pytest.raises(SystemExit):
        parse_args(["--files", f"FakeSynth4D-kitti={out}", "--label-maps", "m.json"])     # needs --synth4d-splits


# ------------------------------------------------------------------ what the GPU tests' realistic cases rest on
@pytest.mark.parametrize("source,target", RR.REALISTIC)
def test_realistic_cases_keep_the_cap(source, target):
    """asserted on the restatement alone: the output sizes, and that the cells an ambiguous point could enter (left out
    of the comparison of output rows on the GPU) are at most 1 % of the occupied cells"""
    pts, _, spec, origin, ref = RR.realistic(source, target)
    assert ref.occupied == RR.REALISTIC_COUNTS[(source, target)]
    assert int(ref.ambiguous.sum()) == {("nusc35k", "kitti120k"): 26}.get((source, target), 0)
    assert len(ref.tainted) <= RR.CAP * ref.occupied
    assert origin.tolist() == raycast.origin_between(source, target).tolist()
    if (source, target) == ("nusc35k", "kitti120k"):                 # sparse -> dense: cells stay empty, points leave
        assert ref.occupied < pts.shape[0] < spec.n_cells and (ref.cells == -1).sum() > 0


def test_the_8x125_sensor_keeps_the_cap():
    pts, _ = synth.scan_points_labels(0, "source8k")
    ref = RR.raycast_ref(pts, RR.sensor_8x125())
    assert ref.occupied == 1000 and len(ref.tainted) == 0
    zero = raycast.SensorSpec(RR.sensor_8x125().elevations, 125)      # why the sensor has an az0: see sensor_8x125
    assert len(RR.raycast_ref(pts, zero).tainted) > RR.CAP * 1000
