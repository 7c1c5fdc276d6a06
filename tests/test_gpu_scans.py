"""Scans from files on the GPU: lidog_amd.scans.load_scan equals the reference's cached `data` dict on every G15 case
(point bytes, labels, kept rows, label statistics) and scans_ref's numpy restatement over a sweep of sizes, layouts and
keep masks; the radius rule on points whose squared radius rounds onto the threshold; numpy's indexing rules for the
labels; FileScans' validation and training items, class_counts and batches; and a --files fit that validates, saves and
resumes, a two-source step and eval_target --target-files."""
import hashlib
import os

import numpy as np
import pytest
import torch

import augment_ref as A
import scans_ref as R
from lidog_amd import scans

pytestmark = pytest.mark.gpu

META, G15 = R.load_g15()
MAPS = R.fixture_maps(G15)
CASES = sorted(META["cases"])
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 100003)
KEEPS = (1.0, 0.0, 0.5, 0.03)
BOTH = [A.ROT, A.SCALE]


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    return R.write_trees(str(tmp_path_factory.mktemp("scans")), MAPS)


def _lut(dataset):
    return G15[f"lut_{R.map_of(dataset)}"]


def _listing(trees, dataset, phase):
    return scans.listing(dataset, R.tree_root(trees, dataset), phase, version="mini", synth4d_splits=trees["splits"])


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _load(raw_p, raw_l, lut, stride, mask, radius, counts=None, **kw):
    got = scans.load_scan(_cuda(raw_p), _cuda(raw_l), _cuda(lut), stride, mask, radius, counts=counts, **kw)
    assert got["points"].dtype == torch.float32 and got["sem_labels"].dtype == torch.int32
    assert got["features"].dtype == torch.float32 and got["features"].shape == (got["points"].shape[0], 1)
    assert bool((got["features"] == 1).all()) and got["points"].shape[1:] == (3,)
    return got["points"].cpu().numpy(), got["sem_labels"].cpu().numpy()


def _same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", CASES)
def test_load_scan_equals_the_reference(trees, name):
    case = META["cases"][name]
    dataset = case["dataset"]
    lst = _listing(trees, dataset, case["phase"])
    pts, labels, stride = scans.read_files(lst.format, *lst.files[case["index"]])
    lut = _lut(dataset)
    counts = torch.zeros(int(lut.max()) + 1, dtype=torch.int64, device="cuda")
    got_p, got_l = _load(pts, labels, lut, stride, lst.format["mask"], R.IN_RADIUS if lst.format["radius"] else None,
                         counts=counts)
    want = R.case_outputs(name, G15, "data")
    assert got_p.shape[0] == case["kept"]
    assert _same_bytes(got_p, want["points"]) and np.array_equal(got_l, want["labels"])
    raw_p, raw_l, st, mask, _ = R.read_np(dataset, *lst.files[case["index"]])
    mapped = R.load_scan_np(raw_p, raw_l, lut, st, mask)[2]
    assert np.array_equal(counts.cpu().numpy(), R.counts_np(mapped, counts.shape[0]).astype(np.int64))


@pytest.mark.parametrize("key", sorted(k for k, v in META["stats"].items() if v == "ok"))
def test_counts_of_a_listing_equal_the_reference_stats(trees, key):
    """the counts load_scan adds while it loads, over a listing: get_dataset_stats"""
    dataset, phase = key.rsplit("_", 1)
    lst = _listing(trees, dataset, phase)
    lut = _lut(dataset)
    counts = torch.zeros(int(lut.max()) + 1, dtype=torch.int64, device="cuda")
    for files in lst.files:
        pts, labels, stride = scans.read_files(lst.format, *files)
        _load(pts, labels, lut, stride, lst.format["mask"], R.IN_RADIUS if lst.format["radius"] else None, counts=counts)
    assert np.array_equal(counts.cpu().numpy().astype(np.float64), G15[f"{key}__stats"])


# ------------------------------------------------------------------ sizes, layouts, keep masks against the restatement
def _sweep_input(n, layout, keep, seed):
    """(points_raw [n, stride] float32, labels_raw, lut, stride, mask, radius): a share `keep` of the rows inside 50 m"""
    rng = np.random.default_rng([n, int(keep * 100), seed])
    stride = {"kitti": 4, "nusc": 5, "synth3": 3, "synth6": 6}[layout]
    d = rng.normal(size=(n, 3))
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
    inside = rng.random(n) < keep
    r = np.where(inside, rng.uniform(1.0, 49.0, n), rng.uniform(51.0, 80.0, n))
    rec = np.concatenate([d * r[:, None], rng.random((n, stride - 3))], axis=1).astype(np.float32)
    cls = rng.integers(-1, 7, n)
    if layout == "kitti":
        keys, vals = MAPS["SemanticKITTI"]
        raw = (R.raw_ids(rng, cls, keys, vals).astype(np.uint32) | (rng.integers(0, 1 << 16, n).astype(np.uint32) << 16)).view(np.int32)
        return rec, raw, G15["lut_SemanticKITTI"], stride, 0xFFFF, R.IN_RADIUS, inside
    if layout == "nusc":
        keys, vals = MAPS["nuScenes"]
        return rec, R.raw_ids(rng, cls, keys, vals).astype(np.uint8), G15["lut_nuScenes"], stride, None, R.IN_RADIUS, inside
    keys, vals = MAPS["Synth4D"]
    lut = G15["lut_Synth4D"]
    raw = R.raw_ids(rng, cls, keys, vals)
    raw = np.where(rng.random(n) < 0.25, raw - lut.shape[0], raw).astype(np.int32)       # a quarter wraps
    return rec, raw, lut, stride, None, None, np.ones(n, dtype=bool)


@pytest.mark.parametrize("layout", ["kitti", "nusc", "synth3", "synth6"])
def test_size_sweep_equals_the_restatement(layout):
    for n in SIZES:
        for keep in KEEPS:
            rec, raw, lut, stride, mask, radius, inside = _sweep_input(n, layout, keep, 3)
            counts = torch.zeros(int(lut.max()) + 1, dtype=torch.int64, device="cuda")
            got_p, got_l = _load(rec, raw, lut, stride, mask, radius, counts=counts)
            want_p, want_l, mapped = R.load_scan_np(rec, raw, lut, stride, mask, radius)
            what = (layout, n, keep)
            assert _same_bytes(got_p, want_p) and np.array_equal(got_l, want_l), what
            rows = np.flatnonzero(inside)                         # stable: ascending row order
            assert _same_bytes(got_p, rec[rows, :3]) and np.array_equal(got_l, mapped[rows]), what
            assert np.array_equal(counts.cpu().numpy(), R.counts_np(mapped, counts.shape[0]).astype(np.int64)), what
            if n >= 1023 and radius is not None:
                assert abs(rows.shape[0] - keep * n) <= 0.05 * n + 1, what     # the masks are what they are called


def test_raw_bytes_and_unaligned_buffers():
    """the points as raw bytes, and a stride-4 buffer that does not start on 16 bytes (the dword path)"""
    rec, raw, lut, stride, mask, radius, _ = _sweep_input(1025, "kitti", 0.5, 4)
    want_p, want_l, _ = R.load_scan_np(rec, raw, lut, stride, mask, radius)
    got = scans.load_scan(_cuda(rec.reshape(-1).view(np.uint8)), _cuda(raw), _cuda(lut), stride, mask, radius)
    assert _same_bytes(got["points"].cpu().numpy(), want_p)
    buf = torch.zeros(rec.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = _cuda(rec.reshape(-1))
    assert buf[1:].data_ptr() % 16 == 4
    got = scans.load_scan(buf[1:], _cuda(raw), _cuda(lut), stride, mask, radius)
    assert _same_bytes(got["points"].cpu().numpy(), want_p) and np.array_equal(got["sem_labels"].cpu().numpy(), want_l)


def test_load_scan_twice_same_bytes():
    rec, raw, lut, stride, mask, radius, _ = _sweep_input(100003, "nusc", 0.5, 5)
    a, b = _load(rec, raw, lut, stride, mask, radius), _load(rec, raw, lut, stride, mask, radius)
    assert _same_bytes(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------ the radius rule
@pytest.mark.parametrize("radius", [50.0, 35.5])
def test_radius_rule_on_the_threshold(radius):
    """4097 points on the shell r = radius (1 +- 3e-7).  Conditions on the input, checked on the CPU before the device is
    looked at: at least 16 rows that a fused multiply-add evaluation, fma(z, z, fma(y, y, x x)), classifies differently
    from numpy's float32 (x x + y y) + z z, and at least 16 rows whose sum is exactly the threshold (strictness)."""
    rng = np.random.default_rng([15, int(radius * 10)])
    d = rng.normal(size=(4097, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = (d * (radius * (1 + rng.uniform(-3e-7, 3e-7, 4097)))[:, None]).astype(np.float32)
    r2 = np.float32(radius ** 2)
    s = np.sum(np.square(p), axis=1)
    assert s.dtype == np.float32
    assert np.array_equal(s, (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    y, z = p[:, 1].astype(np.float64), p[:, 2].astype(np.float64)          # a 24 x 24 bit product is exact in float64
    inner = (y * y + (p[:, 0] * p[:, 0]).astype(np.float64)).astype(np.float32)
    fused = (z * z + inner.astype(np.float64)).astype(np.float32)
    assert int(((fused < r2) != (s < r2)).sum()) >= 16
    assert int((s == r2).sum()) >= 16
    rec = np.concatenate([p, np.zeros((4097, 1), np.float32)], axis=1)
    raw = np.zeros(4097, dtype=np.int32)
    lut = G15["lut_SemanticKITTI"]
    got_p, _ = _load(rec, raw, lut, 4, 0xFFFF, radius)
    assert _same_bytes(got_p, p[s < r2])
    want_p, _, _ = R.load_scan_np(rec, raw, lut, 4, 0xFFFF, radius)
    assert _same_bytes(got_p, want_p)


# ------------------------------------------------------------------ label edges
def test_label_edges():
    lut = G15["lut_Synth4D"]
    L = lut.shape[0]
    rng = np.random.default_rng(9)
    pts = rng.uniform(-20, 20, (64, 3)).astype(np.float32)
    raw = rng.integers(0, L, 64).astype(np.int32)
    raw[:4] = (-1, -L, L - 1, -L + 7)                                       # the edges of numpy's wrap
    _, got = _load(pts, raw, lut, 3, None, None)
    assert np.array_equal(got, lut[raw]) and got[3] == lut[7]
    for bad in (L, -L - 1, 1 << 20, -(1 << 31)):
        r = raw.copy()
        r[17] = bad
        with pytest.raises(IndexError, match="frame-17"):
            _load(pts, r, lut, 3, None, None, name="frame-17")
        with pytest.raises(IndexError):
            lut[r]                                                           # as numpy
    # SemanticKITTI: the mask comes first, so a negative int32 (instance id >= 2^15) is in range
    lk = G15["lut_SemanticKITTI"]
    r = np.array([(0xFFFF << 16) | 10, (0x8000 << 16) | 40, 0x7FFF0000 | 252], dtype=np.uint32).view(np.int32)
    _, got = _load(pts[:3], r, lk, 3, 0xFFFF, None)
    assert np.array_equal(got, lk[r & 0xFFFF])
    with pytest.raises(IndexError):                                          # 0xFFFF itself is past the table
        _load(pts[:3], np.array([-1, 0, 0], np.int32), lk, 3, 0xFFFF, None)
    # nuScenes: a byte past the table
    ln = G15["lut_nuScenes"]
    assert ln.shape[0] < 255
    with pytest.raises(IndexError):
        _load(pts[:3], np.array([0, 255, 1], np.uint8), ln, 3, None, None)
    # no label file: zeros, unmapped; nothing is looked up
    _, got = _load(pts, None, lut, 3, None, None)
    assert got.shape == (64,) and not got.any()


def test_non_finite_points():
    lut = G15["lut_nuScenes"]
    rng = np.random.default_rng(10)
    rec = rng.uniform(-20, 20, (300, 5)).astype(np.float32)
    raw = rng.integers(0, 32, 300).astype(np.uint8)
    rec[5, 0], rec[70, 1], rec[299, 2], rec[150, 1] = np.nan, np.nan, np.inf, -np.inf
    rec[8, 3] = np.nan                                                       # not a coordinate
    got_p, got_l = _load(rec, raw, lut, 5, None, 50.0)
    keep = np.ones(300, dtype=bool)
    keep[[5, 70, 299, 150]] = False
    assert _same_bytes(got_p, rec[keep, :3]) and np.array_equal(got_l, lut[raw][keep])
    with pytest.raises(ValueError, match="non-finite"):
        _load(rec, raw, lut, 5, None, None)


def test_size_errors_before_any_launch():
    lut = _cuda(G15["lut_SemanticKITTI"])
    pts = torch.zeros(41, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="16-byte record"):
        scans.load_scan(pts, None, lut, 4)
    with pytest.raises(ValueError, match="shape 10 and 9"):
        scans.load_scan(pts[:40], torch.zeros(9, dtype=torch.int32, device="cuda"), lut, 4)
    with pytest.raises(ValueError, match="float32"):
        scans.load_scan(torch.zeros(43, dtype=torch.uint8, device="cuda"), None, lut, 4)
    with pytest.raises(ValueError, match="int32 or uint8"):
        scans.load_scan(pts[:40], torch.zeros(10, dtype=torch.int64, device="cuda"), lut, 4)
    with pytest.raises(ValueError, match="point_stride"):
        scans.load_scan(pts[:40], None, lut, 2)
    with pytest.raises(NotImplementedError):
        scans.load_scan(pts[:40], None, lut, 4, use_intensity=True)
    with pytest.raises(RuntimeError, match="GPU"):
        scans.load_scan(pts[:40].cpu(), None, lut, 4)


# ------------------------------------------------------------------ the dataset
def _host(item):
    return {k: v.cpu().numpy() for k, v in item.items()}


@pytest.mark.parametrize("name", CASES)
def test_validation_item_equals_the_reference(trees, name):
    """the plain item (validation phase; a training listing without augmentations and BEV labels is the same)"""
    case = META["cases"][name]
    ds = scans.FileScans(_listing(trees, case["dataset"], case["phase"]), _lut(case["dataset"]), voxel_size=R.VOXEL)
    (item,) = ds.item(case["index"])
    got, want = _host(item), R.case_outputs(name, G15, "item")
    assert got["coordinates"].dtype == np.int32 and got["coordinates"].shape[0] == case["voxels"]
    for k, g in (("coordinates", "coordinates"), ("sem_labels", "sem_labels"), ("inverse_map", "inverse_map"),
                 ("index", "sampled_idx"), ("index", "index")):
        assert np.array_equal(got[g].astype(np.int64), want[k].astype(np.int64)), (name, k)
    assert got["features"].dtype == np.float32 and np.array_equal(got["features"], want["features"])
    assert _same_bytes(got["xyz"], R.case_outputs(name, G15, "data")["points"][want["index"].astype(np.int64)])


@pytest.mark.parametrize("dataset,augs", [("SemanticKITTI", None), ("SemanticKITTI", BOTH), ("nuScenes", None),
                                          ("nuScenes", BOTH), ("Synth4D-kitti", BOTH)])
def test_bev_training_item_equals_the_restatement(trees, dataset, augs):
    from lidog_amd.train import bev_image_size
    bev = (50.0, bev_image_size(50.0))
    lst = _listing(trees, dataset, "train")
    ds = scans.FileScans(lst, _lut(dataset), voxel_size=R.VOXEL, augmentations=augs, sub_p=0.8, seed=77, bev=bev)
    ds.set_epoch(2)
    bev_from = "first" if dataset == "nuScenes" else "voted"
    for i in range(len(lst)):
        raw_p, raw_l, stride, mask, radius = R.read_np(dataset, *lst.files[i])
        pts, lab, _ = R.load_scan_np(raw_p, raw_l, _lut(dataset), stride, mask, radius)
        draws = ds.draws(ds.item_rng(i), pts.shape[0])
        if augs is None:                                          # no sub-sample without an augmentation list
            assert np.array_equal(draws["sampled_idx"], np.arange(pts.shape[0])) and draws["ops"] == []
        else:
            assert draws["sampled_idx"].shape[0] == int(0.8 * pts.shape[0]) and [a for a, _ in draws["ops"]] == BOTH
        want = A.augment_np(pts, np.ones((pts.shape[0], 1), np.float32), lab.astype(np.int64), draws, R.VOXEL, True,
                            R.IGNORE, bev, bev_from)
        (item,) = ds.item(i)                                      # kernel and restatement use the same plain chain
        got = _host(item)
        assert got["coordinates"].shape[0] < pts.shape[0]         # the bounds filter and the voxels did something
        A.compare(got, want, want["_xyz_bound"], f"{dataset} {i}")


def test_class_counts(trees):
    for key, state in sorted(META["stats"].items()):
        dataset, phase = key.rsplit("_", 1)
        ds = scans.FileScans(_listing(trees, dataset, phase), _lut(dataset))
        if state == "ok":
            w = ds.class_counts()
            assert w.dtype == np.float64 and np.array_equal(w, G15[f"{key}__stats"]), key
        else:
            with pytest.raises(FileNotFoundError):
                ds.class_counts()
    two = scans.FileScans([_listing(trees, "SemanticKITTI", "train"), _listing(trees, "nuScenes", "train")],
                          [_lut("SemanticKITTI"), _lut("nuScenes")]).class_counts()
    assert np.array_equal(two[0], G15["SemanticKITTI_train__stats"]) and np.array_equal(two[1], G15["nuScenes_train__stats"])


def _digest(batch):
    h = hashlib.sha1()
    for k in sorted(batch):
        v = batch[k]["block8"] if isinstance(batch[k], dict) else batch[k]
        h.update(k.encode() + str(tuple(v.shape)).encode() + v.cpu().numpy().tobytes())
    return h.hexdigest()


def test_batches(trees):
    from lidog_amd.train import bev_image_size
    size = bev_image_size(50.0)
    lut = [_lut("SemanticKITTI"), _lut("nuScenes")]
    one = scans.FileScans(_listing(trees, "SemanticKITTI", "train"), lut[0], augmentations=BOTH, seed=5, bev=(50.0, size))
    b = one.batch([2, 0], "cuda")
    torch.cuda.synchronize()
    assert set(b) == {"coords_int", "source_coordinates0", "source_features0", "source_sem_labels0", "source_bev_labels0"}
    assert b["source_bev_labels0"]["block8"].shape == (2, size, size) and b["source_sem_labels0"].dtype == torch.int64
    assert b["coords_int"].dtype == torch.int32 and b["coords_int"][:, 0].unique().tolist() == [0, 1]
    assert torch.equal(b["source_coordinates0"], b["coords_int"].float())
    assert _digest(one.batch([2, 0], "cuda")) == _digest(b)                    # made twice: identical bytes
    one.set_epoch(1)
    assert _digest(one.batch([2, 0], "cuda")) != _digest(b)                    # another epoch draws again
    cached = scans.FileScans(_listing(trees, "SemanticKITTI", "train"), lut[0], augmentations=BOTH, seed=5,
                             bev=(50.0, size), use_cache=True)
    assert _digest(cached.batch([2, 0], "cuda")) == _digest(b) and len(cached._cache) == 2
    assert _digest(cached.batch([2, 0], "cuda")) == _digest(b)
    two = scans.FileScans([_listing(trees, "SemanticKITTI", "train"), _listing(trees, "nuScenes", "train")], lut,
                          augmentations=None, seed=5, bev=(50.0, size))
    assert len(two) == 3 and two.num_sources == 2
    b2 = two.batch([0, 1], "cuda")
    assert {"coords_int", "coords_int1", "source_bev_labels0", "source_bev_labels1", "source_features1"} <= set(b2)
    val = scans.FileScans(_listing(trees, "nuScenes", "validation"), lut[1])
    bv = val.batch([0], "cuda")
    assert set(bv) == {"coords_int", "source_coordinates0", "source_features0", "source_sem_labels0"}
    assert bv["coords_int"].shape[0] == META["cases"]["nuScenes_validation_0"]["voxels"]


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def mini_tree(tmp_path_factory):
    """a `mini` SemanticKITTI tree of source8k-sized frames and its label map as JSON"""
    root = str(tmp_path_factory.mktemp("mini"))
    R.write_kitti_tree(os.path.join(root, "kitti"), MAPS, {"00": 2, "01": 1, "08": 2}, whole=True)
    R.write_kitti_tree(os.path.join(root, "other"), MAPS, {"00": 1, "01": 1, "08": 1}, whole=True)
    return os.path.join(root, "kitti"), os.path.join(root, "other"), R.write_label_map_json(
        os.path.join(root, "kitti.json"), MAPS, "SemanticKITTI")


def _recording(fit, log):
    inner = fit.train_data.batch

    def batch(indices, device):
        b = inner(indices, device)
        log.append((fit.train_data.epoch, tuple(int(i) for i in indices), _digest(b)))
        return b

    fit.train_data.batch = batch


def _assert_same_state(fit, ckpt, when):
    """the model's weights and buffers and the optimiser's state (torch.optim's layout: moments and step per parameter,
    the group's lr) of `fit` equal those of a checkpoint dict bit for bit"""
    have = {k: v.detach().cpu() for k, v in fit.model.state_dict().items()}
    assert set(have) == {k[len("model."):] for k in ckpt["state_dict"]}
    for k, v in ckpt["state_dict"].items():
        assert torch.equal(have[k[len("model."):]], v), f"{when}: {k} differs"
    mine, want = fit.opt.torch_state_dict(), ckpt["optimizer_states"][0]
    assert set(mine["state"]) == set(want["state"]) and len(want["state"]) > 0
    for i, entry in want["state"].items():
        assert set(mine["state"][i]) == set(entry) and {"exp_avg", "exp_avg_sq", "step"} <= set(entry)
        for name, v in entry.items():
            assert torch.equal(mine["state"][i][name].detach().cpu(), v), f"{when}: optimiser {name} of parameter {i} differs"
    assert mine["param_groups"][0]["lr"] == want["param_groups"][0]["lr"]
    assert fit.global_step == ckpt["global_step"]


@pytest.mark.timeout(300)
def test_cli_files_fit_validate_resume_and_eval_target(mini_tree, tmp_path, capsys):
    """--files fits two epochs, validates and saves.  A run resumed from the first epoch's checkpoint starts from exactly
    its weights and its Adam state (moments and step counts, compared with the checkpoint entry by entry), is fed
    byte-identical batches, and ends with the SAME weights and Adam state as the uninterrupted run, bit for bit: the
    library has no float atomic and takes no position from an atomic, so a step on the same bytes gives the same bytes,
    and anything the restore got slightly wrong (a stale second moment, a step count off by one) shows here.  The
    largest difference is printed before it is asserted.  Then eval_target --target-files on the saved checkpoint
    writes the CSV under the target's name."""
    from lidog_amd import eval_target
    from lidog_amd.train import _fit_from_args, parse_args
    kitti, _, label_map = mini_tree
    argv = ["--files", f"SemanticKITTI={kitti}", "--label-maps", label_map, "--version", "mini", "--model", "MinkUNet34BEV",
            "--augment", "RandomRotation", "RandomScale", "--batch", "1", "--check-val-every-n-epoch", "1"]
    fit = _fit_from_args(parse_args(argv + ["--epochs", "2", "--save-dir", str(tmp_path / "a")]))
    fit.log = lambda *_: None
    assert isinstance(fit.train_data, scans.FileScans) and len(fit.train_data) == 3 and fit.train_data.bev is not None
    assert list(fit.val_data) == ["SemanticKITTI"] and len(fit.val_data["SemanticKITTI"]) == 2
    assert fit.val_data["SemanticKITTI"].phase == "validation" and fit.val_data["SemanticKITTI"].augmentations is None
    whole = []
    _recording(fit, whole)
    hist = fit.run()
    assert len(hist) == 2 and all(len(h["losses"]) == 3 and np.isfinite(h["losses"]).all() for h in hist)
    assert all(h["validation"]["SemanticKITTI"]["steps"] == 2 and np.isfinite(h["validation"]["SemanticKITTI"]["sem_loss"])
               for h in hist)
    assert [os.path.basename(h["checkpoint"]) for h in hist] == ["epoch=0-step=3.ckpt", "epoch=1-step=6.ckpt"]
    assert len({d for _, _, d in whole}) == 6                    # every item of every epoch is another point set
    # resumed from the first epoch's checkpoint: the same weights to start from, the same batches, the same epoch
    again = _fit_from_args(parse_args(argv + ["--epochs", "2", "--save-dir", str(tmp_path / "b"), "--resume",
                                              hist[0]["checkpoint"]]))
    again.log = lambda *_: None
    assert again.epoch == 1 and again.global_step == 3
    ck0 = torch.load(hist[0]["checkpoint"], map_location="cpu", weights_only=False)
    _assert_same_state(again, ck0, "after the restore")
    resumed = []
    _recording(again, resumed)
    h2 = again.run()
    assert len(h2) == 1 and h2[0]["epoch"] == 1 and h2[0]["global_step"] == 6
    assert sorted(resumed) == sorted(x for x in whole if x[0] == 1) and len(resumed) == 3
    # the bound of the sibling resume test (test_gpu_train.py) on the same quantities
    np.testing.assert_allclose(h2[0]["losses"], hist[1]["losses"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(h2[0]["validation"]["SemanticKITTI"]["sem_loss"],
                               hist[1]["validation"]["SemanticKITTI"]["sem_loss"], rtol=0, atol=1e-6)
    ck1 = torch.load(hist[1]["checkpoint"], map_location="cpu", weights_only=False)
    diff = max(float((again.model.state_dict()[k[len("model."):]].detach().cpu().double() - v.double()).abs().max())
               for k, v in ck1["state_dict"].items() if v.is_floating_point())
    with capsys.disabled():
        print(f"\nlargest weight difference, resumed against uninterrupted: {diff:.3e}")
    _assert_same_state(again, ck1, "at the end of the resumed run")
    # eval_target on the saved checkpoint: the CSV carries the target's name
    capsys.readouterr()
    res = eval_target.main(["--checkpoint", hist[1]["checkpoint"], "--sources", "SemanticKITTI", "--target-files",
                            f"SemanticKITTI={kitti}", "--label-maps", label_map, "--version", "mini", "--batch", "2"])
    assert len(res) == 1 and res[0]["target"] == "SemanticKITTI" and res[0]["scans"] == 2 and res[0]["rows"] == 1
    assert res[0]["csv"].endswith("results/SemanticKITTI-TO-SemanticKITTI.csv")
    rows = open(res[0]["csv"]).read().splitlines()
    assert len(rows) == 2 and rows[1].startswith("SemanticKITTI,SemanticKITTI,")
    assert int(res[0]["counts"].sum()) == sum(int(fit.val_data["SemanticKITTI"].batch([i], "cuda")["coords_int"].shape[0])
                                              for i in range(2))


@pytest.mark.timeout(300)
def test_cli_two_entries_take_a_two_source_step(mini_tree):
    from lidog_amd.train import _fit_from_args, parse_args
    kitti, other, label_map = mini_tree
    fit = _fit_from_args(parse_args(["--files", f"SemanticKITTI={kitti}", f"SemanticKITTI={other}", "--label-maps",
                                     label_map, label_map, "--version", "mini", "--model", "MinkUNet34BEV", "--batch", "2",
                                     "--epochs", "1", "--limit-files", "2", "--source-weights", "0.4", "0.6"]))
    fit.log = lambda *_: None
    assert fit.step.num_sources == 2 and fit.train_data.num_sources == 2 and len(fit.train_data) == 2
    assert list(fit.val_data) == ["SemanticKITTI:0", "SemanticKITTI:1"]
    hist = fit.run()
    assert len(hist) == 1 and len(hist[0]["losses"]) == 1 and np.isfinite(hist[0]["losses"]).all()
