"""The Raycast baseline in the training data path: scans.FileScans and train.AugmentedSynthScans with `raycast=` give the
items and batches that the restatement's resample (raycast_ref) followed by the existing augment_item path gives; the
Fake dataset writer's files hold the restatement's bytes and read back through the Fake* readers; two training steps of
the command line's shape; and a run without --raycast-to takes the step it took before."""
import json
import os

import numpy as np
import pytest
import torch

import augment_ref as A
import raycast_ref as RR
import scans_ref as R
from lidog_amd import raycast, scans, synth
from lidog_amd.data import augment_item, collate_items
from lidog_amd.train import AugmentedSynthScans, Fit, SynthScans, _fit_from_args, bev_image_size, parse_args

pytestmark = pytest.mark.gpu

META, G15 = R.load_g15()
MAPS = R.fixture_maps(G15)
BOTH = [A.ROT, A.SCALE]
ORIGIN = np.array([0.05, -0.1, 0.2], np.float32)
KEYS = ("coordinates", "sem_labels", "inverse_map", "sampled_idx", "features")


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    return R.write_trees(str(tmp_path_factory.mktemp("raycast")), MAPS)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ref_scan(pts, labels, spec, origin):
    """the restatement's resample of a host scan, as the scan dict augment_item takes; nothing may be ambiguous"""
    ref = RR.raycast_ref(pts, spec, origin)
    assert not ref.ambiguous.any() and 0 < ref.occupied < pts.shape[0]
    lab = np.asarray(labels)[ref.rows]
    return {"points": _cuda(ref.points), "sem_labels": _cuda(lab),
            "features": torch.ones((ref.occupied, 1), dtype=torch.float32, device="cuda")}


def _same_item(got, want, what):
    for k in KEYS:
        assert torch.equal(got[k], want[k]), (what, k)
    assert got["xyz"].dtype == want["xyz"].dtype and torch.equal(got["xyz"], want["xyz"]), what


def _same_batch(got, want):
    assert set(got) == set(want)
    for k in got:
        g, w = (got[k]["block8"], want[k]["block8"]) if isinstance(got[k], dict) else (got[k], want[k])
        assert g.dtype == w.dtype and torch.equal(g, w), k


@pytest.mark.parametrize("dataset,augs,bev", [("SemanticKITTI", None, False), ("SemanticKITTI", BOTH, True),
                                               ("Synth4D-kitti", BOTH, False)])
def test_file_scans_equal_reference_resample_then_augment(trees, dataset, augs, bev):
    spec = RR.sensor_8x125()
    bev = (50.0, bev_image_size(50.0)) if bev else None
    lut = G15[f"lut_{R.map_of(dataset)}"]
    lst = scans.listing(dataset, R.tree_root(trees, dataset), "train", version="mini", synth4d_splits=trees["splits"])
    ds = scans.FileScans(lst, lut, voxel_size=R.VOXEL, augmentations=augs, sub_p=0.8, seed=31, bev=bev, raycast=spec,
                         raycast_origin=ORIGIN)
    ds.set_epoch(1)
    want_items = []
    for i in range(len(lst)):
        raw_p, raw_l, stride, mask, radius = R.read_np(dataset, *lst.files[i])
        pts, lab, _ = R.load_scan_np(raw_p, raw_l, lut, stride, mask, radius)
        scan = _ref_scan(pts, lab, spec, ORIGIN)
        m = scan["points"].shape[0]
        draws = ds.draws(ds.item_rng(i), m)                          # the draws see the resampled point count
        assert draws["sampled_idx"].shape[0] == (m if augs is None else int(0.8 * m))
        want = augment_item(scan, draws, voxel_size=R.VOXEL, bounds=bev is not None, ignore_label=-1, bev=bev,
                            bev_from=lst.format["bev_from"])
        (got,) = ds.item(i)
        _same_item(got, want, (dataset, i))
        want_items.append([want])
    ids = list(range(len(lst)))[::-1]
    _same_batch(ds.batch(ids, "cuda"), collate_items([want_items[i] for i in ids], bev is not None))
    torch.cuda.synchronize()


@pytest.mark.parametrize("augs,bev", [(None, False), (BOTH, True)])
def test_synthetic_scans_equal_reference_resample_then_augment(augs, bev):
    spec = RR.sensor_8x125()
    bev = (50.0, bev_image_size(50.0)) if bev else None
    ds = AugmentedSynthScans(3, "source8k", augs, sub_p=0.8, seed=9, bev=bev, raycast=spec, raycast_origin=ORIGIN)
    ds.set_epoch(2)
    voxel = synth.CONFIGS["source8k"]["voxel"]
    want_items = []
    for i in range(3):
        pts, labels = synth.scan_points_labels(i, "source8k")
        scan = _ref_scan(pts, labels, spec, ORIGIN)
        draws = ds.draws(ds.item_rng(i), scan["points"].shape[0])
        want_items.append([augment_item(scan, draws, voxel_size=voxel, bounds=bev is not None, ignore_label=-1, bev=bev)])
    _same_batch(ds.batch([2, 0, 1], "cuda"), collate_items([want_items[i] for i in (2, 0, 1)], bev is not None))
    # as the item provider of the mixing / scaling datasets
    rng = ds.item_rng(1)
    draws = ds.draw_item(0, 1, rng, "cuda")
    item = ds.make_item(0, 1, draws, "cuda")
    torch.cuda.synchronize()
    for k in ("coordinates", "sem_labels", "features"):
        assert torch.equal(item[k], want_items[1][0][k]), k
    # the default origin of a configuration's sensor is the height difference
    auto = AugmentedSynthScans(1, "kitti120k", None, raycast="nusc35k")
    pts, labels, nusc, origin, ref = RR.realistic("kitti120k", "nusc35k")
    got = auto.scan(0, 0, torch.device("cuda"))
    assert got["points"].shape[0] == ref.occupied and torch.equal(got["rows"].cpu(), torch.from_numpy(ref.rows))


def test_validation_is_never_resampled(trees):
    lst = scans.listing("SemanticKITTI", trees["SemanticKITTI"], "validation", version="mini")
    with pytest.raises(ValueError, match="raycast"):
        scans.FileScans(lst, G15["lut_SemanticKITTI"], raycast="nusc35k")


@pytest.mark.parametrize("dataset", ["SemanticKITTI", "Synth4D-nuscenes"])
def test_writer_files_equal_the_reference_bytes(trees, tmp_path, dataset):
    spec = RR.sensor_8x125()
    fake = raycast.FAKE_OF[dataset]
    kw = dict(version="mini", synth4d_splits=trees["splits"])
    src = scans.listing(dataset, R.tree_root(trees, dataset), "validation", **kw)
    assert raycast.write_fake(src, spec, str(tmp_path), origin=ORIGIN) == len(src) > 0
    back = scans.listing(fake, str(tmp_path), "validation", **kw)
    for (sp, sl), (bp, bl) in zip(src.files, back.files):
        raw_p, raw_l, stride, _, _ = R.read_np(dataset, sp, sl)
        xyz = np.ascontiguousarray(raw_p.reshape(-1, stride)[:, :3])
        ref = RR.raycast_ref(xyz, spec, ORIGIN)
        assert not ref.ambiguous.any() and ref.occupied > 0
        rec = np.zeros((ref.occupied, 4), np.float32)
        rec[:, :3] = ref.points
        assert open(bp, "rb").read() == rec.tobytes()
        want_l = raw_l[ref.rows].astype(np.uint8 if dataset == "Synth4D-nuscenes" else np.int32)
        assert open(bl, "rb").read() == want_l.tobytes()             # the raw words, instance ids included
    # and the files train: the Fake reader's items are load_scan of those bytes
    lut = G15[f"lut_{R.map_of(dataset)}"]
    ds = scans.FileScans(back, lut, voxel_size=R.VOXEL)
    (item,) = ds.item(0)
    raw_p, raw_l, stride, mask, radius = R.read_np(dataset, *src.files[0])
    ref = RR.raycast_ref(np.ascontiguousarray(raw_p.reshape(-1, stride)[:, :3]), spec, ORIGIN)
    pts, lab, _ = R.load_scan_np(np.concatenate([ref.points, np.zeros((ref.occupied, 1), np.float32)], axis=1),
                                 raw_l[ref.rows], lut, 4, mask, radius)
    want = R.item_np(pts, lab)
    assert np.array_equal(item["coordinates"].cpu().numpy(), want["coordinates"])
    assert np.array_equal(item["sem_labels"].cpu().numpy().astype(np.int64), want["sem_labels"].astype(np.int64))


@pytest.mark.timeout(300)
def test_two_steps_of_the_command_line(tmp_path):
    path = str(tmp_path / "beams8x125.json")
    with open(path, "w") as f:
        json.dump(RR.sensor_8x125().to_json(), f)
    fit = _fit_from_args(parse_args(["--model", "MinkUNet34", "--config", "source8k", "--raycast-to", path, "--lr", "0.01",
                                     "--scheduler", "ExponentialLR", "--scans", "2", "--batch", "1", "--epochs", "1"]))
    fit.log = lambda *_: None
    ds = fit.train_data
    assert isinstance(ds, AugmentedSynthScans) and ds.augmentations is None and ds.raycast.n_az == 125 and fit.val_data is None
    assert ds.raycast.az0 == RR.sensor_8x125().az0 and ds.raycast_origins == [None]
    voxel = synth.CONFIGS["source8k"]["voxel"]
    for i in range(2):                                               # the batch's voxel count equals the reference's
        pts, labels = synth.scan_points_labels(i, "source8k")
        scan = _ref_scan(pts, labels, ds.raycast, None)
        want = augment_item(scan, {"sampled_idx": np.arange(scan["points"].shape[0]), "ops": []}, voxel_size=voxel)
        got = ds.batch([i], "cuda")
        assert got["coords_int"].shape[0] == want["coordinates"].shape[0] > 500
        assert torch.equal(got["coords_int"][:, 1:], want["coordinates"])
    hist = fit.run()
    assert len(hist) == 1 and len(hist[0]["losses"]) == 2 and np.isfinite(hist[0]["losses"]).all()
    assert fit.global_step == 2


@pytest.mark.timeout(300)
def test_a_run_without_raycast_takes_the_step_it_took(tmp_path):
    """the dataset built by the command line without --raycast-to and the dataset as it was always built give the same
    first-step loss, bit for bit"""
    argv = ["--model", "MinkUNet34", "--config", "source8k", "--scans", "1", "--batch", "1", "--epochs", "1"]
    a = parse_args(argv)
    assert not hasattr(a, "raycast_to")
    by_cli = _fit_from_args(a)
    assert type(by_cli.train_data) is SynthScans and by_cli.train_data.config == "source8k"
    by_cli.log = lambda *_: None
    direct = Fit("MinkUNet34", a.bound, 1, a.optimizer, a.lr, a.scheduler, 1, a.warmup_epochs, seed=a.seed,
                 check_val_every_n_epoch=a.check_val_every_n_epoch,
                 train_data=SynthScans(1, "source8k", mix3d=False, bev_size=bev_image_size(a.bound)), log=lambda *_: None)
    l0, l1 = by_cli.run()[0]["losses"][0], direct.run()[0]["losses"][0]
    assert np.isfinite(l0) and np.float32(l0).view(np.uint32) == np.float32(l1).view(np.uint32)
    # and --augment without --raycast-to still builds the dataset it built
    aug = _fit_from_args(parse_args(argv + ["--augment", "RandomRotation"])).train_data
    assert isinstance(aug, AugmentedSynthScans) and aug.raycast is None and aug.augmentations == ["RandomRotation"]
    old = AugmentedSynthScans(1, "source8k", ["RandomRotation"], sub_p=a.sub_p, seed=a.seed)
    _same_batch(aug.batch([0], "cuda"), old.batch([0], "cuda"))
