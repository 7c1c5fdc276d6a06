"""Scans from files, the parts that need no GPU: the label maps and their look-up tables, the numpy restatement of the
first mile against every recorded output of the reference (G15), the file listings, the command lines and the C ABI."""
import ctypes
import os
import pickle

import numpy as np
import pytest

import scans_ref as R
from lidog_amd import scans

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META, G15 = R.load_g15()
MAPS = R.fixture_maps(G15)


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    return R.write_trees(str(tmp_path_factory.mktemp("scans")), MAPS)


def _listing(trees, dataset, phase, **kw):
    return scans.listing(dataset, R.tree_root(trees, dataset), phase, version="mini", synth4d_splits=trees["splits"], **kw)


# ------------------------------------------------------------------ label maps
@pytest.mark.parametrize("name", sorted(R.MAPS))
def test_luts_from_yaml_equal_recorded(name):
    """the only test that needs PyYAML, which is part of this project's test environment: without it this fails"""
    import yaml  # noqa: F401
    lm = scans.load_label_map(os.path.join(R.GOLDEN, R.MAPS[name]))
    lut = scans.label_lut(lm)
    assert lut.dtype == np.int32 and np.array_equal(lut, G15[f"lut_{name}"])
    assert lut.shape[0] == max(lm) + 100
    assert np.array_equal(np.array(list(lm.keys())), MAPS[name][0]) and np.array_equal(np.array(list(lm.values())), MAPS[name][1])


def test_label_map_from_json(tmp_path):
    for name, (keys, vals) in MAPS.items():                  # all three maps, without PyYAML
        p = tmp_path / f"{name}.json"
        p.write_text('{"learning_map": {%s}}' % ", ".join(f'"{k}": {v}' for k, v in zip(keys, vals)))
        lm = scans.load_label_map(str(p))
        assert list(lm.items()) == list(zip(keys.tolist(), vals.tolist()))
        assert np.array_equal(scans.label_lut(lm), G15[f"lut_{name}"])
    (tmp_path / "bad.json").write_text('{"labels": {}}')
    with pytest.raises(ValueError, match="learning_map"):
        scans.load_label_map(str(tmp_path / "bad.json"))


# ------------------------------------------------------------------ the restatement against the reference
@pytest.mark.parametrize("name", sorted(META["cases"]))
def test_restatement_equals_reference(trees, name):
    case = META["cases"][name]
    dataset = case["dataset"]
    rel_p, rel_l = META["listings"][f"{dataset}_{case['phase']}"][case["index"]]
    base = R.tree_root(trees, dataset)
    raw_p, raw_l, stride, mask, radius = R.read_np(dataset, os.path.join(base, rel_p), os.path.join(base, rel_l))
    assert (raw_l is not None) == case["labels_file"]
    pts, lab, mapped = R.load_scan_np(raw_p, raw_l, G15[f"lut_{R.map_of(dataset)}"], stride, mask, radius)
    assert mapped.shape[0] == case["rows"] and pts.shape[0] == case["kept"]
    want = R.case_outputs(name, G15, "data")
    assert pts.dtype == np.float32 and np.array_equal(pts.view(np.uint32), want["points"].view(np.uint32))
    assert lab.dtype == np.int32 and np.array_equal(lab, want["labels"])
    item, want = R.item_np(pts, lab), R.case_outputs(name, G15, "item")
    assert sorted(want) == ["coordinates", "features", "index", "inverse_map", "sem_labels"]
    for k, w in want.items():
        assert np.array_equal(np.asarray(item[k]).astype(np.float64), w.astype(np.float64)), (name, k)


def test_fixture_exercises_the_rules():
    """the radius mask drops rows of every masked case and never of Synth4D; voxels hold several points; a negative id
    wraps; the file without labels has zeros"""
    for name, case in META["cases"].items():
        masked = case["dataset"] in ("SemanticKITTI", "nuScenes")
        assert (case["kept"] < case["rows"] - R.FAR) if masked else case["kept"] == case["rows"], name
        assert case["voxels"] < case["kept"], name
    assert not META["cases"]["Synth4D-kitti_validation_1"]["labels_file"]
    assert not G15["Synth4D-kitti_validation_1__data_labels"].any()
    assert META["stats"]["Synth4D-kitti_validation"].startswith("raises")


@pytest.mark.parametrize("key", sorted(k for k, v in META["stats"].items() if v == "ok"))
def test_restated_stats_equal_reference(trees, key):
    dataset, phase = key.rsplit("_", 1)
    lut = G15[f"lut_{R.map_of(dataset)}"]
    w = np.zeros(int(lut.max()) + 1)
    base = R.tree_root(trees, dataset)
    for rel_p, rel_l in META["listings"][key]:
        raw_p, raw_l, stride, mask, _ = R.read_np(dataset, os.path.join(base, rel_p), os.path.join(base, rel_l))
        w += R.counts_np(R.load_scan_np(raw_p, raw_l, lut, stride, mask)[2], w.shape[0])
    assert np.array_equal(w, G15[f"{key}__stats"]) and w.sum() > 0


# ------------------------------------------------------------------ listings
@pytest.mark.parametrize("dataset", R.DATASETS)
@pytest.mark.parametrize("phase", R.PHASES)
def test_listing_order(trees, dataset, phase):
    lst = _listing(trees, dataset, phase)
    base = R.tree_root(trees, dataset)
    got = [[os.path.relpath(os.path.normpath(p), base), os.path.relpath(os.path.normpath(l), base)] for p, l in lst.files]
    assert got == META["listings"][f"{dataset}_{phase}"] and len(lst) == len(got) and lst.phase == phase
    assert len(_listing(trees, dataset, phase, limit=1)) == 1
    assert [f for f in _listing(trees, dataset, phase, limit=1).files] == lst.files[:1]


def test_synth4d_ids_sort_as_numbers(trees):
    files = scans.synth4d_files(trees["Synth4D"], "Synth4D-kitti", trees["splits"], "train")
    assert [os.path.basename(p) for p, _ in files] == ["9.npy", "10.npy", "3.npy", "12.npy"]          # Town06, then Town03
    assert all(os.path.normpath(l) == os.path.normpath(p).replace("velodyne", "labels") for p, l in files)


def test_semantickitti_splits(tmp_path):
    root = str(tmp_path)
    frames = {"00": 2, "01": 0, "02": 1, "03": 1, "04": 1, "05": 1, "06": 1, "07": 1, "08": 3, "09": 1, "10": 2}
    for seq, n in frames.items():
        os.makedirs(os.path.join(root, "sequences", seq, "labels"))
        for f in range(n):
            open(os.path.join(root, "sequences", seq, "labels", f"{f:06d}.label"), "wb").close()
    rel = lambda files: [os.path.relpath(p, os.path.join(root, "sequences")) for p, _ in files]
    full = scans.semantickitti_files(root, "train", "full")
    assert rel(full) == [f"{s}/velodyne/{f:06d}.bin" for s in ("00", "01", "02", "03", "04", "05", "06", "07", "09", "10")
                         for f in range(frames[s])]
    assert full[0][1] == os.path.join(root, "sequences", "00", "labels", "000000.label")
    assert rel(scans.semantickitti_files(root, "train", "mini")) == ["00/velodyne/000000.bin", "00/velodyne/000001.bin"]
    for version in ("full", "mini"):
        assert rel(scans.semantickitti_files(root, "validation", version)) == [f"08/velodyne/{f:06d}.bin" for f in range(3)]
    with pytest.raises(NotImplementedError):
        scans.semantickitti_files(root, "train", "tiny")
    with pytest.raises(ValueError):
        scans.semantickitti_files(root, "test", "full")
    os.rmdir(os.path.join(root, "sequences", "01", "labels"))
    with pytest.raises(FileNotFoundError, match="01"):                   # a missing sequence is an error
        scans.semantickitti_files(root, "train", "mini")


def test_pair_list_and_listing_errors(tmp_path, trees):
    (tmp_path / "train.txt").write_text("a.bin a_seg.bin\n\nb.bin  b_seg.bin\n")
    assert scans.pair_list_files(str(tmp_path), "train") == [(str(tmp_path / "a.bin"), str(tmp_path / "a_seg.bin")),
                                                             (str(tmp_path / "b.bin"), str(tmp_path / "b_seg.bin"))]
    (tmp_path / "val.txt").write_text("a.bin\n")
    with pytest.raises(ValueError, match="val.txt:1"):
        scans.pair_list_files(str(tmp_path), "validation")
    with pytest.raises(ValueError, match="split"):
        scans.listing("Synth4D-kitti", trees["Synth4D"], "train")
    with pytest.raises(ValueError):
        scans.listing("SemanticPOSS", str(tmp_path), "train")


def test_split_pickles_read_as_the_reference_writes_them(tmp_path):
    """a list (training) and an ndarray (validation) of ids, towns in the pickle's order"""
    os.makedirs(tmp_path / "s" / "nuscenes_synth")
    with open(tmp_path / "s" / "nuscenes_synth" / "validation_split.pkl", "wb") as f:
        pickle.dump({"Town10HD": np.array([30, 4]), "Town03": np.array([7])}, f)
    files = scans.synth4d_files("/d", "Synth4D-nuscenes", str(tmp_path / "s"), "validation")
    assert [p for p, _ in files] == ["/d/nuscenes_synth/Town10HD/velodyne/4.npy", "/d/nuscenes_synth/Town10HD/velodyne/30.npy",
                                     "/d/nuscenes_synth/Town03/velodyne/7.npy"]


# ------------------------------------------------------------------ sizes are checked on the host, before any launch
def test_file_size_mismatch(tmp_path):
    p, l = str(tmp_path / "p.bin"), str(tmp_path / "l.label")
    np.zeros(4 * 10 + 1, np.float32).tofile(p)
    np.zeros(10, np.int32).tofile(l)
    with pytest.raises(ValueError, match="16-byte point record"):
        scans.read_files(scans.FORMATS["SemanticKITTI"], p, l)
    np.zeros(5 * 10, np.float32).tofile(p)
    with open(l, "wb") as f:
        f.write(b"\0" * 10)
    pts, labels, stride = scans.read_files(scans.FORMATS["nuScenes"], p, l)
    assert pts.dtype == np.uint8 and pts.shape[0] == 200 and labels.dtype == np.uint8 and stride == 5
    np.zeros(4 * 10, np.float32).tofile(p)
    with pytest.raises(ValueError, match="4-byte label record"):
        scans.read_files(scans.FORMATS["SemanticKITTI"], p, l)
    np.save(str(tmp_path / "a.npy"), np.zeros((10, 2)))
    with pytest.raises(ValueError, match="shape"):
        scans.read_files(scans.FORMATS["Synth4D-kitti"], str(tmp_path / "a.npy"), str(tmp_path / "none.npy"))


def test_file_scans_arguments(trees):
    lut = G15["lut_SemanticKITTI"]
    tr, va = _listing(trees, "SemanticKITTI", "train"), _listing(trees, "SemanticKITTI", "validation")
    d = scans.FileScans([tr, _listing(trees, "nuScenes", "train")], [lut, G15["lut_nuScenes"]], augmentations=[])
    assert len(d) == 3 and d.num_sources == 2 and d.augmentations == [] and d.train
    assert scans.FileScans(va, lut, augmentations=["RandomScale"], bev=(50.0, 167)).bev is None      # validation: plain
    with pytest.raises(ValueError):
        scans.FileScans([tr, va], [lut, lut])
    with pytest.raises(ValueError):
        scans.FileScans([va, va], [lut, lut])
    with pytest.raises(ValueError):
        scans.FileScans([tr, tr], [lut])
    with pytest.raises(NotImplementedError):
        scans.FileScans(tr, lut, use_intensity=True)
    with pytest.raises(NotImplementedError):
        scans.FileScans(tr, lut, augmentations=["RandomFlip"])


# ------------------------------------------------------------------ command lines
FILES = ["--files", "SemanticKITTI=/data/kitti", "--label-maps", "k.yaml"]


def test_train_cli_parses_files():
    from lidog_amd.train import parse_args
    a = parse_args(FILES + ["--version", "mini", "--limit-files", "8", "--augment", "RandomRotation", "--sub-p", "0.7"])
    assert a.files == [("SemanticKITTI", "/data/kitti")] and a.label_maps == ["k.yaml"] and a.version == "mini"
    assert a.limit_files == 8 and a.augment == ["RandomRotation"] and a.sub_p == 0.7 and a.config == "kitti120k"
    a = parse_args(["--files", "Synth4D-kitti=/d/s4d", "nuScenes=/d/nusc", "--label-maps", "s.yaml", "n.json",
                    "--synth4d-splits", "/d/_split", "--model", "MinkUNet34", "--source-weights", "0.3", "0.7"])
    assert a.files == [("Synth4D-kitti", "/d/s4d"), ("nuScenes", "/d/nusc")] and a.synth4d_splits == "/d/_split"
    assert a.version == "full" and a.limit_files is None


def test_train_cli_defaults_unchanged():
    from lidog_amd.train import parse_args
    a = vars(parse_args([]))
    new = {"files": None, "label_maps": None, "synth4d_splits": None, "version": "full", "limit_files": None}
    assert {k: a[k] for k in new} == new
    assert {k: v for k, v in a.items() if k not in new} == dict(
        model="MinkUNet34BEV", bound=50.0, batch=4, optimizer="Adam", lr=1e-3, scheduler=None, epochs=25, warmup_epochs=0,
        scans=16, val_scans=0, config="kitti120k", sources=None, source_weights=(0.5, 0.5), mix3d=False, mix=None,
        sub_p=0.8, augment=None, sn_targets=None, check_val_every_n_epoch=5, save_dir=None, resume=None,
        auto_resume=False, seed=1234)
    assert parse_args(["--config", "nusc35k"]).config == "nusc35k"


@pytest.mark.parametrize("argv", [
    FILES + ["--config", "kitti120k"],
    FILES + ["--sources", "kitti120k", "nusc35k"],
    FILES + ["--mix", "cosmix", "--model", "MinkUNet34"],
    FILES + ["--mix3d"],
    FILES + ["--sn-targets", "nusc35k_cars", "--model", "MinkUNet34"],
    ["--files", "SemanticKITTI=/data/kitti"],                                              # no label map
    ["--files", "SemanticKITTI=/a", "nuScenes=/b", "--label-maps", "k.yaml"],              # one map for two entries
    ["--files", "SemanticKITTI=/a", "nuScenes=/b", "nuScenes=/c", "--label-maps", "a", "b", "c"],
    ["--files", "SemanticPOSS=/a", "--label-maps", "k.yaml"],
    ["--files", "SemanticKITTI", "--label-maps", "k.yaml"],
    ["--files", "Synth4D-kitti=/a", "--label-maps", "k.yaml"],                             # no split folder
    FILES + ["--limit-files", "0"],
    FILES + ["--version", "tiny"],
    ["--label-maps", "k.yaml"],
    ["--limit-files", "3"],
])
def test_train_cli_errors(argv, capsys):
    from lidog_amd.train import parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_eval_target_cli():
    from lidog_amd.eval_target import parse_args
    a = parse_args(["--checkpoint", "c.ckpt"])
    assert a.targets == ["nusc35k"] and a.target_files is None and a.label_maps is None
    a = parse_args(["--checkpoint", "c.ckpt", "--target-files", "SemanticKITTI=/k", "nuScenes=/n", "--label-maps", "k.yaml",
                    "n.yaml", "--limit-files", "5"])
    assert a.target_files == [("SemanticKITTI", "/k"), ("nuScenes", "/n")] and a.targets == ["SemanticKITTI", "nuScenes"]
    assert a.limit_files == 5 and a.version == "full"
    for argv in (["--target-files", "SemanticKITTI=/k"], ["--target-files", "KITTI=/k", "--label-maps", "k.yaml"],
                 ["--label-maps", "k.yaml"], ["--target-files", "Synth4D-nuscenes=/s", "--label-maps", "s.yaml"]):
        with pytest.raises(SystemExit):
            parse_args(["--checkpoint", "c.ckpt"] + argv)


# ------------------------------------------------------------------ C ABI
def test_scan_symbols_exported_and_bound():
    from lidog_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    for name in ("lidog_scan_load_ws", "lidog_scan_load"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f"{name}(" in header
    assert _lib.ABI_VERSION == 9 and lib.lidog_abi_version() == 9          # additive entries: the version stays
    assert "scanload.hip" in build.SOURCES
    lib.lidog_scan_load_ws.restype = ctypes.c_int64
    lib.lidog_mix_split_ws.restype = ctypes.c_int64
    for n in (0, 1, 1025, 130000):
        assert lib.lidog_scan_load_ws(ctypes.c_int64(n)) == 3 * n + 3 + lib.lidog_mix_split_ws(ctypes.c_int64(n), ctypes.c_int32(1))
    # arguments are refused on the host, before any launch
    lib.lidog_last_error.restype = ctypes.c_char_p
    i64, i32, vp, f32 = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_float
    args = lambda stride, kind, classes: (vp(8), i32(stride), vp(), i32(kind), i32(-1), i64(10), vp(), i32(0), i32(0),
                                          f32(0), vp(), vp(), vp(8), i32(classes), vp(8), vp(), vp())
    assert lib.lidog_scan_load(*args(2, 0, 7)) == 2 and b"point_stride = 2" in lib.lidog_last_error()
    assert lib.lidog_scan_load(*args(4, 3, 7)) == 2 and b"label_kind = 3" in lib.lidog_last_error()
    assert lib.lidog_scan_load(*args(4, 0, 257)) == 2 and b"257 classes" in lib.lidog_last_error()
    assert lib.lidog_scan_load(*args(4, 1, 7)) == 2 and b"look-up table" in lib.lidog_last_error()
