"""The point-level path without a GPU: the numpy restatement (tests/pointlabels_ref.py) against cases written out by
hand, the command line of --point-level / --save-labels / --inverse-label-map, the label files' paths and bytes, the
inverse label map, the wrappers' argument checks that need no device, the C ABI."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import pointlabels_ref as P
from helpers import REPO
from lidog_amd import evaluate

POINT_SYMBOLS = ("lidog_scan_keep_rows_ws", "lidog_scan_keep_rows", "lidog_point_labels_ws", "lidog_point_labels")
NAN = float("nan")


# ------------------------------------------------------------------ the restatement, by hand
def test_keep_rows_by_hand():
    one_in = np.nextafter(np.float32(50.0), np.float32(0.0))
    pts = np.array([[1, 2, 3, 9], [50, 0, 0, 9], [one_in, 0, 0, 9], [0, 60, 0, 9], [NAN, 0, 0, 9], [np.inf, 0, 0, 9],
                    [0, 0, -49, 9], [30, 40, 0, 9], [30, 30, 30, 9]], dtype=np.float32)
    keep_row, m = P.keep_rows_np(pts, 4, 50.0)
    # (50, 0, 0) and (30, 40, 0) lie exactly on the sphere: the comparison is strict
    assert keep_row.dtype == np.int32 and keep_row.tolist() == [0, -1, 1, -1, -1, -1, 2, -1, -1] and m == 3
    keep_row, m = P.keep_rows_np(pts, 4, None)
    assert keep_row.tolist() == list(range(9)) and m == 9
    keep_row, m = P.keep_rows_np(np.zeros((0, 5), np.float32), 5, 50.0)
    assert keep_row.shape == (0,) and m == 0
    # raw bytes are taken as float32 words; stride 3 has no padding column
    keep_row, m = P.keep_rows_np(pts[:, :3].copy().view(np.uint8), 3, 50.0)
    assert keep_row.tolist() == [0, -1, 1, -1, -1, -1, 2, -1, -1]


def test_argmax_and_label_map_by_hand():
    x = np.array([[0, 1, 1, 0], [2, 2, 2, 2], [0, NAN, 5, NAN], [-np.inf, -np.inf, -np.inf, -np.inf], [1, 0, np.inf, 3]],
                 dtype=np.float32)
    assert P.argmax_np(x).tolist() == [1, 0, 1, 0, 2]
    assert P.argmax_np(x).tolist() == torch.from_numpy(x).max(1)[1].tolist()         # torch's CPU rule
    lut = np.array([-1, 0, 1, 2, -1], dtype=np.int32)
    mapped, bad = P.map_labels_np(np.array([1, 0x70003, 4, 5, -1, -5, -6], np.int32), lut, 0xFFFF)
    # 0xFFFF & -1 = 65535 and the like: outside the table; without the mask -1 wraps as numpy's indexing does
    assert mapped.tolist() == [0, 2, -1, -1, -1, -1, -1] and bad.tolist() == [False, False, False, True, True, True, True]
    mapped, bad = P.map_labels_np(np.array([1, -1, -5, -6], np.int32), lut, None)
    assert mapped.tolist() == [0, -1, -1, -1] and bad.tolist() == [False, False, False, True]
    mapped, bad = P.map_labels_np(np.array([3, 200], np.uint8), lut, None)
    assert mapped.tolist() == [2, -1] and bad.tolist() == [False, True]


def _hand_batch():
    """two scans and an empty one between them.  Scan 0: 5 records, record 1 dropped, 3 voxels (voxel 2 holds no point);
    scan 1: nothing; scan 2: 3 records, the last dropped, 2 voxels"""
    logits = np.array([[0, 1, 0], [2, 2, 1], [0, 0, 9],          # scan 0: predictions 1, 0 (tie), 2
                       [NAN, 5, 0], [0, 0, 0.5]], np.float32)    # scan 2: predictions 0 (NaN), 2
    return dict(logits=logits, row_off=[0, 5, 5, 8], kept_off=[0, 4, 4, 6], vox_off=[0, 3, 3, 5],
                keep_row=np.array([0, -1, 1, 2, 3, 0, 1, -1], np.int32),
                inverse_map=np.array([1, 0, 0, 1, 1, 0], np.int64))


def test_point_labels_by_hand():
    b = _hand_batch()
    out, counts, err = P.point_labels_np(**b)
    assert out.dtype == np.uint32 and out.tolist() == [0, 0, 1, 1, 0, 2, 0, 0] and counts is None and err == 0
    out, _, _ = P.point_labels_np(**b, out_lut=[40, 10, 70], fill=255)
    assert out.tolist() == [40, 255, 10, 10, 40, 70, 40, 255]
    # raw labels through a table: classes 0 1 ignored 1 2 | 2 0 1; record 1 and 7 are dropped, record 2 is ignored
    lut = np.array([-1, 0, 1, 2], np.int32)
    raw = np.array([1, 2, 0, 2, 3, 3, 1, 2], np.int32) | (7 << 16)
    out, counts, err = P.point_labels_np(**b, labels_raw=raw, lut=lut, mask=0xFFFF)
    want = np.zeros((3, 3, 3), np.int64)
    want[0, 0, 0] = 1        # record 0: label 0, prediction 0
    want[0, 1, 1] = 1        # record 3: label 1, prediction 1
    want[0, 2, 0] = 1        # record 4: label 2, prediction 0
    want[2, 2, 2] = 1        # record 5: label 2, prediction 2
    want[2, 0, 0] = 1        # record 6: label 0, prediction 0
    assert err == 0 and np.array_equal(counts, want) and counts.sum() == 5
    # an in-range ignore label leaves its records out
    _, counts, _ = P.point_labels_np(**b, labels_raw=raw, lut=lut, mask=0xFFFF, ignore_label=2)
    assert counts.sum() == 3 and counts[:, 2].sum() == 0


def test_point_labels_errors_by_hand():
    b = _hand_batch()
    lut = np.array([-1, 0, 1, 2], np.int32)
    raw = np.array([1, 2, 0, 2, 3, 3, 1, 2], np.int32)
    clean, clean_counts, _ = P.point_labels_np(**b, labels_raw=raw, lut=lut, fill=9)
    # record 3's label is outside the table: fill, not counted
    r = raw.copy()
    r[3] = 4
    out, counts, err = P.point_labels_np(**b, labels_raw=r, lut=lut, fill=9)
    assert err == P.ERR_LABEL and out[3] == 9 and np.array_equal(np.delete(out, 3), np.delete(clean, 3))
    assert counts.sum() == clean_counts.sum() - 1 and counts[0, 1, 1] == 0
    # kept row 3 of scan 0 (record 4) points at voxel 3 of 3
    k = dict(b, inverse_map=b["inverse_map"].copy())
    k["inverse_map"][3] = 3
    out, counts, err = P.point_labels_np(**k, labels_raw=raw, lut=lut, fill=9)
    assert err == P.ERR_INVERSE and out[4] == 9 and np.array_equal(np.delete(out, 4), np.delete(clean, 4))
    assert counts.sum() == clean_counts.sum() - 1
    # record 6 of scan 2 claims kept row 2 of 2; -2 is as wrong
    for value in (2, -2):
        k = dict(b, keep_row=b["keep_row"].copy())
        k["keep_row"][6] = value
        out, counts, err = P.point_labels_np(**k, labels_raw=raw, lut=lut, fill=9)
        assert err == P.ERR_KEEP and out[6] == 9 and np.array_equal(np.delete(out, 6), np.delete(clean, 6))
        assert counts.sum() == clean_counts.sum() - 1 and counts[2, 0, 0] == 0
    assert [b for b, _ in evaluate.POINT_ERRORS] == [P.ERR_SCAN, P.ERR_LABEL, P.ERR_INVERSE, P.ERR_KEEP]


def test_point_counts_feed_iou_rows():
    c = np.zeros((2, 3, 3), np.int64)
    c[0] = [[4, 1, 0], [0, 2, 0], [0, 0, 0]]
    c[1] = [[0, 0, 0], [0, 0, 3], [0, 0, 5]]
    wide = evaluate.point_iou_counts(c)
    assert wide.shape == (2, 4, 3) and wide[:, 0].sum() == 0 and np.array_equal(wide[:, 1:], c)
    rows = evaluate.iou_rows(wide, "scan")
    assert np.array_equal(rows, [[4 / 5, 2 / 3, -1.0], [-1.0, 0.0, 5 / 8]])
    rows = evaluate.iou_rows(wide, "batch")
    assert np.array_equal(rows, [[4 / 5, 2 / 6, 5 / 8]])


# ------------------------------------------------------------------ command line
FILES = ["--checkpoint", "c.ckpt", "--target-files", "SemanticKITTI=/k", "nuScenes=/n", "--label-maps", "k.json", "n.json"]


def test_cli_point_flags(capsys):
    from lidog_amd import eval_target as T
    a = T.parse_args(FILES)
    assert (a.point_level, a.save_labels, a.inverse_label_map) == (False, False, None)
    a = T.parse_args(FILES + ["--point-level", "--rows", "scan"])
    assert a.point_level and not a.save_labels and a.rows == "scan"
    a = T.parse_args(FILES + ["--save-labels", "--inverse-label-map", "ki.yaml", "ni.json"])
    assert a.save_labels and not a.point_level and a.inverse_label_map == ["ki.yaml", "ni.json"]
    for flags in (["--point-level"], ["--save-labels"], ["--inverse-label-map", "x.json"]):
        with pytest.raises(SystemExit):
            T.parse_args(["--checkpoint", "c.ckpt", "--targets", "nusc35k"] + flags)     # a synthetic target has no file
        assert "--target-files" in capsys.readouterr().err
    for maps in (["one.json"], ["a.json", "b.json", "c.json"]):                          # one map per target
        with pytest.raises(SystemExit):
            T.parse_args(FILES + ["--save-labels", "--inverse-label-map"] + maps)
        assert "one file per" in capsys.readouterr().err


# ------------------------------------------------------------------ label files
def test_label_file_paths_and_bytes(tmp_path):
    folder = str(tmp_path / "predictions")
    p = evaluate.label_file_path(folder, "SemanticKITTI", "SemanticKITTI", 7, "/data/kitti/sequences/08/velodyne/000123.bin")
    assert p == os.path.join(folder, "SemanticKITTI", "sequences", "08", "predictions", "000123.label")
    p = evaluate.label_file_path(folder, "SemanticKITTI", "SemanticKITTI", 0, "rel/sequences/11/velodyne/../velodyne/000000.bin")
    assert p.endswith(os.path.join("sequences", "11", "predictions", "000000.label"))
    with pytest.raises(ValueError, match="sequences/SS/velodyne"):
        evaluate.label_file_path(folder, "SemanticKITTI", "SemanticKITTI", 0, "/data/kitti/08/000123.bin")
    assert evaluate.label_file_path(folder, "nuScenes", "nuScenes", 7, "/n/samples/LIDAR_TOP/a.pcd.bin") == \
        os.path.join(folder, "nuScenes", "point_labels", "7.label")
    ids = np.array([0, 1, 40, 65535, 7], dtype=np.uint32)
    path = evaluate.write_label_file(str(tmp_path / "a" / "b" / "x.label"), ids)
    raw = open(path, "rb").read()
    assert len(raw) == 4 * 5 and raw[:12] == b"\x00\x00\x00\x00\x01\x00\x00\x00\x28\x00\x00\x00"      # little-endian
    back = np.fromfile(path, dtype=np.uint32)
    assert np.array_equal(back, ids) and not (back >> 16).any()
    assert os.path.getsize(evaluate.write_label_file(str(tmp_path / "empty.label"), ids[:0])) == 0
    # the writer: one file per scan of a batch, split at the row offsets, named after the listing's files
    files = [(f"/k/sequences/08/velodyne/{i:06d}.bin", f"/k/sequences/08/labels/{i:06d}.label") for i in range(5)]
    w = evaluate.PointLabelWriter(folder, "SemanticKITTI", "SemanticKITTI", files)
    w(3, np.arange(10, dtype=np.uint32), [0, 4, 4, 10][:3])
    assert [os.path.basename(p) for p in w.written] == ["000003.label", "000004.label"]
    assert np.fromfile(w.written[0], np.uint32).tolist() == [0, 1, 2, 3] and os.path.getsize(w.written[1]) == 0
    g = evaluate.PointLabelWriter(folder, "nuScenes", "nuScenes", files)
    g(1, np.arange(10, dtype=np.uint32), [0, 4, 10])
    assert [os.path.relpath(p, folder) for p in g.written] == ["nuScenes/point_labels/1.label", "nuScenes/point_labels/2.label"]
    assert np.fromfile(g.written[1], np.uint32).tolist() == [4, 5, 6, 7, 8, 9]


def test_inverse_label_map(tmp_path):
    lut, fill = evaluate.inverse_lut(None, 7)
    assert lut.dtype == np.int32 and lut.tolist() == list(range(7)) and fill == 0         # the identity, fill 0
    j = tmp_path / "inv.json"
    j.write_text(json.dumps({"learning_map_inv": {"-1": 0, "0": 10, "1": 30, "6": 70}, "learning_map": {"10": 0}}))
    m = evaluate.load_inverse_label_map(str(j))
    assert m == {-1: 0, 0: 10, 1: 30, 6: 70}
    lut, fill = evaluate.inverse_lut(m, 7)
    assert lut.tolist() == [10, 30, 2, 3, 4, 5, 70] and fill == 0
    lut, fill = evaluate.inverse_lut({-1: 255, 2: 40}, 7)
    assert lut.tolist() == [0, 1, 40, 3, 4, 5, 6] and fill == 255
    y = tmp_path / "inv.yaml"
    y.write_text("learning_map_inv:\n  -1: 1\n  0: 10\n  3: 48\n")
    pytest.importorskip("yaml")
    assert evaluate.load_inverse_label_map(str(y)) == {-1: 1, 0: 10, 3: 48}
    (tmp_path / "no.json").write_text(json.dumps({"learning_map": {"10": 0}}))
    with pytest.raises(ValueError, match="learning_map_inv"):
        evaluate.load_inverse_label_map(str(tmp_path / "no.json"))
    with pytest.raises(ValueError, match="class 7"):
        evaluate.inverse_lut({7: 1}, 7)
    with pytest.raises(ValueError, match="id 65536"):
        evaluate.inverse_lut({0: 65536}, 7, max_id=0xFFFF)                               # SemanticKITTI's upper half
    with pytest.raises(ValueError, match="id -3"):
        evaluate.inverse_lut({0: -3}, 7)


# ------------------------------------------------------------------ the library's surface
def test_wrappers_refuse_host_tensors():
    from lidog_amd import scans
    with pytest.raises(RuntimeError, match="GPU"):
        scans.keep_rows(torch.zeros(8), 4, 50.0)
    with pytest.raises(RuntimeError, match="GPU"):
        evaluate.point_labels(torch.zeros((2, 3)), [0, 1], [0, 1], [0, 2], torch.zeros(1, dtype=torch.int32),
                              torch.zeros(1, dtype=torch.int64))
    lst = scans.Listing("SemanticKITTI", [], "train")
    with pytest.raises(ValueError, match="validation"):
        scans.FileScans(lst, np.zeros(4, np.int32), keep_raw=True)
    data = scans.FileScans(scans.Listing("SemanticKITTI", [], "validation"), np.zeros(4, np.int32))
    assert data.keep_raw is False
    with pytest.raises(KeyError, match="keep_raw"):
        data.point_item(0)
    path = evaluate.PointPath(lambda ids: [], fill=3)
    assert path.fill == 3 and path.with_labels and path.out_lut is None and path.on_point_labels is None


def test_point_symbols_exported_and_bound():
    from lidog_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    for name in POINT_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f"{name}(" in header
    assert _lib.ABI_VERSION == 9 and lib.lidog_abi_version() == 9          # additive entries: the version stays
    assert "pointlabels.hip" in build.SOURCES
    # one definition of the radius test and the label look-up for the loader and the point path
    for f in ("scanload.hip", "pointlabels.hip"):
        assert '#include "scan_ops.h"' in open(os.path.join(REPO, "lidog_amd", "csrc", f)).read()
    ops = open(os.path.join(REPO, "lidog_amd", "csrc", "scan_ops.h")).read()
    assert "scan_in_radius" in ops and "fp contract(off)" in ops
    for name in ("lidog_scan_keep_rows_ws", "lidog_point_labels_ws", "lidog_mix_split_ws"):
        getattr(lib, name).restype = ctypes.c_int64
    for n in (0, 1, 5000, 130000):
        assert lib.lidog_scan_keep_rows_ws(ctypes.c_int64(n)) == \
            2 * n + 3 + lib.lidog_mix_split_ws(ctypes.c_int64(n), ctypes.c_int32(1))
        assert lib.lidog_point_labels_ws(ctypes.c_int64(n)) == n
    # arguments are refused on the host, before any launch
    lib.lidog_last_error.restype = ctypes.c_char_p
    i64, i32, u32, vp, f32 = ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_float
    assert lib.lidog_scan_keep_rows(vp(), i32(2), i64(10), i32(1), f32(2500.0), vp(), vp(), vp(), vp()) == 2
    assert b"point_stride = 2" in lib.lidog_last_error()

    def labels(c, b, kind):
        return lib.lidog_point_labels(vp(), i64(10), i32(c), i32(b), vp(), vp(), vp(), i64(10), i64(10), vp(), vp(), vp(),
                                      u32(0), vp(), i32(kind), i32(-1), vp(), i32(0), i64(-1), vp(), vp(), vp(), vp(), vp())
    assert labels(33, 1, 0) == 2 and b"33 classes" in lib.lidog_last_error()
    assert labels(7, 65, 0) == 2 and b"65 scans" in lib.lidog_last_error()         # the offsets ride in the launch
    assert labels(7, 0, 0) == 2 and b"0 scans" in lib.lidog_last_error()
    assert labels(7, 1, 3) == 2 and b"label_kind = 3" in lib.lidog_last_error()
    assert labels(7, 1, 1) == 2 and b"look-up table" in lib.lidog_last_error()
    assert labels(7, 1, 0) == 2 and b"null argument" in lib.lidog_last_error()
    # the offsets are host arrays, checked before any launch: every pointer here is a dummy that is never followed
    one = ctypes.c_int64(0)
    dummy = ctypes.cast(ctypes.pointer(one), vp)

    def offsets(row, kept, vox):
        arrs = [(ctypes.c_int64 * 3)(*o) for o in (row, kept, vox)]
        return lib.lidog_point_labels(dummy, i64(10), i32(7), i32(2), arrs[0], arrs[1], arrs[2], i64(10), i64(10), dummy,
                                      dummy, dummy, u32(0), vp(), i32(0), i32(-1), vp(), i32(0), i64(-1), dummy, vp(), dummy,
                                      dummy, vp())
    assert offsets([0, 6, 5], [0, 5, 10], [0, 5, 10]) == 2 and b"scan 2" in lib.lidog_last_error()
    assert offsets([1, 6, 10], [0, 5, 10], [0, 5, 10]) == 2 and b"scan 0" in lib.lidog_last_error()
    assert offsets([0, 6, 10], [0, 5, 10], [0, 5, 9]) == 2 and b"not at the sizes given" in lib.lidog_last_error()
