"""CoSMix's in-merge augmentation and the composed datasets on the GPU: cosmix_merge with every list form equals the
reference's merge_data (G16) with exact integers and bit-equal copied columns, mix3d_merge returns the reference's
remaining keys, MixedSynthScans / ScaledSynthScans over augmented items equal the numpy composition with the same
generator, the SN statistics over an augmented dataset face equal the restatement's boxes, the file forms of the command
line make reproducible batches, and two --mix cosmix --source-augment training steps repeat bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

import augment_ref as A
import mixaug_ref as M
import scans_ref as R
import sn_ref
from lidog_amd import data, synth
from lidog_amd.data import cosmix_merge, mix3d_merge
from lidog_amd.train import (AugmentedSynthScans, ItemFace, MixedSynthScans, ScaledSynthScans, _data_from_args,
                             _fit_from_args, parse_args)

pytestmark = pytest.mark.gpu

G16 = M.load_g16()
COSMIX = [x for x in G16 if x[0]["method"] == "cosmix"]
ROT, SCALE = M.ROT, M.SCALE
AUGS = [ROT, SCALE]
INTS = ("coordinates", "index", "sem_labels", "sampled_idx")


@functools.lru_cache(maxsize=None)
def _host_scans(name):
    return M.case_scans(next(c for c, _ in G16 if c["name"] == name))


def _device(scan):
    d = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in scan.items() if k != "idx"}
    d["idx"] = torch.tensor(int(scan["idx"]))
    return d


def _host(out):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


# ------------------------------------------------------------------ the merge against the reference
@pytest.mark.parametrize("case", COSMIX, ids=[c["name"] for c, _ in COSMIX])
def test_cosmix_merge_with_a_list_equals_the_reference(case):
    c, arr = case
    s0, s1 = (_device(s) for s in _host_scans(c["name"]))
    kw = dict(voxel_size=M.mix_ref.voxel_size(c), class_weights=(arr["w0"], arr["w1"]), sub_p=c["sub_p"],
              augmentations=c["augs"])
    np.random.seed(c["seed"])
    out = cosmix_merge(s0, s1, rng=np.random, **kw)
    assert float(np.random.rand()) == c["next_rand"]
    assert out["source"] == c["source"]
    got = _host(out)
    assert got["coordinates"].dtype == np.int32 and got["index"].dtype == np.int64
    M.check_outputs(got, c, arr, c["name"])
    again = _host(cosmix_merge(s0, s1, rng=np.random.RandomState(c["seed"]), **kw))      # the same bytes on every run
    for k, _ in M.OUTPUTS:
        assert again[k].tobytes() == got[k].tobytes(), k


def test_none_keeps_the_plain_merge_and_the_empty_list_equals_it():
    """augmentations=None is today's path; the empty list draws nothing more and floors in float32 too"""
    c, arr = next(x for x in COSMIX if x[0]["name"] == "empty_list")
    s0, s1 = (_device(s) for s in _host_scans(c["name"]))
    kw = dict(voxel_size=M.mix_ref.voxel_size(c), class_weights=(arr["w0"], arr["w1"]), sub_p=c["sub_p"])
    plain = _host(cosmix_merge(s0, s1, rng=np.random.RandomState(c["seed"]), **kw))
    empty = _host(cosmix_merge(s0, s1, rng=np.random.RandomState(c["seed"]), augmentations=[], **kw))
    for k, _ in M.OUTPUTS:
        assert plain[k].tobytes() == empty[k].tobytes(), k
    M.check_outputs(plain, c, arr, "plain")


def test_float64_xyz_rows_are_copied_whole():
    """after augmented items xyz is float64 with 24-byte rows, and sampled_idx int64"""
    c, arr = next(x for x in COSMIX if x[0]["name"] == "rot_scale")
    h0, h1 = _host_scans(c["name"])
    wide = [dict(s, xyz=s["xyz"].astype(np.float64) + 1e-9 * (t + 1)) for t, s in enumerate((h0, h1))]
    sel, classes, subs, ops = M.case_draws(c, arr)
    want = M.cosmix_aug_np(wide[0], wide[1], sel, classes, subs, ops, M.mix_ref.voxel_size(c))
    out = _host(cosmix_merge(_device(wide[0]), _device(wide[1]), rng=np.random.RandomState(c["seed"]),
                             voxel_size=M.mix_ref.voxel_size(c), class_weights=(arr["w0"], arr["w1"]), sub_p=c["sub_p"],
                             augmentations=c["augs"]))
    assert out["xyz"].dtype == np.float64 and out["xyz"].tobytes() == want["xyz"].tobytes()
    np.testing.assert_array_equal(out["index"], want["index"])


def test_mix3d_merge_returns_the_remaining_keys():
    c, arr = next(x for x in G16 if x[0]["method"] == "mix3d")
    h0, h1 = _host_scans(c["name"])
    out = mix3d_merge(_device(h0), _device(h1), voxel_size=M.mix_ref.voxel_size(c))
    assert set(out) == {"coordinates", "features", "sem_labels", "index", "xyz", "sampled_idx", "idx"}
    M.check_outputs(_host(out), c, arr, "mix3d")
    assert out["xyz"].shape[0] == h0["xyz"].shape[0] + h1["xyz"].shape[0] and tuple(out["idx"].shape) == (2, 1)
    bare = mix3d_merge(*({k: v for k, v in _device(h).items() if k in ("coordinates", "features", "sem_labels")}
                         for h in (h0, h1)), voxel_size=M.mix_ref.voxel_size(c))
    assert set(bare) == {"coordinates", "features", "sem_labels", "index"}            # today's keys, today's values
    assert torch.equal(bare["coordinates"], out["coordinates"]) and torch.equal(bare["index"], out["index"])


# ------------------------------------------------------------------ composed datasets against the numpy composition
def _compare_item(got, want, what):
    got = _host(got)
    for k in INTS:
        g, w = np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)
        assert g.shape == w.shape, f"{what} {k}: {g.shape} against {w.shape}"
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {k}")
    assert np.array_equal(got["features"], want["features"]), what
    g, w = got["xyz"], want["xyz"]
    assert g.dtype == w.dtype == np.float64 and g.shape == w.shape, what
    excess = np.abs(g - w) - want["_xyz_bound"]
    print(what, "rows", g.shape[0], "largest xyz difference", np.abs(g - w).max(), "bound", want["_xyz_bound"].max())
    assert excess.max() <= 0, f"{what}: xyz off by {np.abs(g - w).max()}"


@pytest.mark.parametrize("method", MixedSynthScans.ALL_METHODS)
def test_mixed_items_over_augmented_scans_equal_the_composition(method):
    configs = ("source8k", "source8k")
    ds = MixedSynthScans(3, 3, configs, method=method, seed=11,
                         items=AugmentedSynthScans(3, configs, AUGS, sub_p=0.8, seed=11))
    wants = []
    for i in range(2):
        want, margin = M.mixed_item_np(ds, i)                     # a PointCutMix draw that raises is an error of the inputs
        assert margin > A.MARGIN, f"item {i}: {margin} voxels from a face: choose another seed"
        wants.append(want)
        _compare_item(ds.item(i), want, f"{method} item {i}")
    b = ds.batch([0, 1], "cuda")
    torch.cuda.synchronize()
    assert set(b) == {"coords_int", "source_coordinates0", "source_features0", "source_sem_labels0"}
    coords = np.concatenate([np.concatenate([np.full((w["coordinates"].shape[0], 1), k, np.int32), w["coordinates"]], 1)
                             for k, w in enumerate(wants)])
    np.testing.assert_array_equal(b["coords_int"].cpu().numpy(), coords)
    np.testing.assert_array_equal(b["source_sem_labels0"].cpu().numpy(), np.concatenate([w["sem_labels"] for w in wants]))
    assert b["source_features0"].shape == (coords.shape[0], 1) and b["source_coordinates0"].dtype == torch.float32


SCALING = [np.array([[1.1, 1.2, 1.3], [0.9, 0.8, 0.7]], np.float32), np.array([[2.0, 2.0, 2.0], [0.5, 0.5, 0.5]], np.float32)]


@pytest.mark.parametrize("sources", [1, 2])
def test_scaled_items_over_augmented_scans_equal_the_composition(sources):
    configs = ("source8k",) * sources
    ds = ScaledSynthScans(3, configs, ("nusc35k", "kitti120k"), seed=11, scaling=SCALING[:sources],
                          items=AugmentedSynthScans(3, configs, AUGS, sub_p=0.8, seed=11))
    indices = [0, 2]
    b = ds.batch(indices, "cuda")
    torch.cuda.synchronize()
    wants = []
    for i in indices:
        outs, margin = M.scaled_items_np(ds, i)
        assert margin > A.MARGIN
        wants.append(outs)
    for s in range(sources):
        coords = np.concatenate([np.concatenate([np.full((w[s]["coordinates"].shape[0], 1), k, np.int32),
                                                 w[s]["coordinates"]], 1) for k, w in enumerate(wants)])
        np.testing.assert_array_equal(b["coords_int1" if s else "coords_int"].cpu().numpy(), coords)
        np.testing.assert_array_equal(b[f"source_sem_labels{s}"].cpu().numpy(),
                                      np.concatenate([w[s]["sem_labels"] for w in wants]))
    assert ds.num_sources == sources and ("coords_int1" in b) == (sources == 2)


def test_average_dims_over_an_augmented_face_equals_the_restatement():
    """5 scans: draw_scans takes int(0.2 * 5) = 1, then the item's own draws follow from the same generator.  The
    thresholds are passed (2000 car voxels, clusters of more than 300): a sub-sampled synthetic scan keeps fewer car
    voxels than the reference's defaults ask for."""
    config, seed, kw = "kitti120k_cars", 5, dict(min_pts=2000, min_car_pts=300)
    items = AugmentedSynthScans(5, (config,), AUGS, sub_p=0.8, seed=seed)
    record = []
    got = data.average_dims(ItemFace(items, 0, 5, rng := np.random.RandomState(seed)), rng=rng, record=record, **kw)
    after = rng.rand()
    ref = np.random.RandomState(seed)
    (scan,) = data.draw_scans(ref, 5)
    pts, labels = synth.scan_points_labels(int(scan), config)
    item = M.item_np(pts, labels, data.draw_augmentation(ref, pts.shape[0], 0.8, AUGS), scan, 0.05)
    assert item["_margin"] > A.MARGIN and ref.rand() == after      # draw_scans first, then the item's draws
    car = item["coordinates"][item["sem_labels"] == 0]
    assert car.shape[0] > kw["min_pts"]
    counts, lo, hi = sn_ref.boxes_np(car, sn_ref.dbscan_np(car))
    assert [r[0] for r in record] == [int(scan)]
    np.testing.assert_array_equal(record[0][1], counts)
    np.testing.assert_array_equal(record[0][2], lo)
    np.testing.assert_array_equal(record[0][3], hi)
    want = data.mean_dims(data.box_dims(counts, lo, hi, 0.05, kw["min_car_pts"]))
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------ files
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """two tiny SemanticKITTI-layout trees and the label map as JSON"""
    root = str(tmp_path_factory.mktemp("mixaug"))
    maps = R.fixture_maps(R.load_g15()[1])
    a = R.write_kitti_tree(os.path.join(root, "a"), maps, {"00": 2, "01": 1, "08": 1}, whole=True)
    b = R.write_kitti_tree(os.path.join(root, "b"), maps, {"00": 1, "01": 1, "08": 1}, whole=True)
    return a, b, R.write_label_map_json(os.path.join(root, "kitti.json"), maps, "SemanticKITTI")


def _bytes(batch):
    return {k: v.cpu().numpy().tobytes() for k, v in batch.items()}


def test_cli_files_cosmix_with_source_augment_makes_reproducible_batches(trees):
    a, b, label_map = trees
    argv = ["--model", "MinkUNet34", "--files", f"SemanticKITTI={a}", f"SemanticKITTI={b}", "--label-maps", label_map,
            label_map, "--version", "mini", "--mix", "cosmix", "--source-augment", ROT, SCALE]
    train, val = _data_from_args(parse_args(argv))
    assert isinstance(train, MixedSynthScans) and train.method == "cosmix" and train.augmentations == AUGS
    assert len(train) == 3 and set(val) == {"SemanticKITTI:0", "SemanticKITTI:1"}
    counts = train.items.class_counts()
    assert all(np.array_equal(w, c) for w, c in zip(train.class_weights, counts))
    first = train.batch([0, 1], "cuda")
    torch.cuda.synchronize()
    assert set(first) == {"coords_int", "source_coordinates0", "source_features0", "source_sem_labels0"}
    assert first["coords_int"].dtype == torch.int32 and first["coords_int"][:, 0].unique().tolist() == [0, 1]
    again = _data_from_args(parse_args(argv))[0].batch([0, 1], "cuda")
    torch.cuda.synchronize()
    assert _bytes(first) == _bytes(again)
    p = train.plan(0, "cuda")
    assert p["scans"] == train.pairs.pair(0) and len(p["items"][0]["ops"]) == 2 and p["merge"]["source"] in (0, 1)


@pytest.mark.parametrize("sources", [1, 2])
def test_cli_files_sn_with_target_files_makes_reproducible_batches(trees, sources, monkeypatch):
    a, b, label_map = trees
    # the tiny trees hold no cars of the reference's size: the statistics' thresholds are lowered for this run alone
    own = data.average_dims
    monkeypatch.setattr(data, "average_dims", lambda d, **kw: _dims_or_unit(own, d, **kw))
    files = [f"SemanticKITTI={a}", f"SemanticKITTI={b}"][:sources]
    argv = ["--model", "MinkUNet34", "--files"] + files + ["--label-maps"] + [label_map] * sources + [
        "--version", "mini", "--source-augment", ROT, SCALE, "--sn-target-files", f"SemanticKITTI={b}",
        "--sn-target-label-maps", label_map]
    train, val = _data_from_args(parse_args(argv))
    assert isinstance(train, ScaledSynthScans) and train.num_sources == sources and len(train.scaling) == sources
    assert train.items.augmentations == AUGS and all(s.shape == (1, 3) for s in train.scaling)
    first = train.batch([0], "cuda")
    torch.cuda.synchronize()
    keys = {"coords_int", "source_coordinates0", "source_features0", "source_sem_labels0"}
    if sources == 2:
        keys |= {"coords_int1", "source_coordinates1", "source_features1", "source_sem_labels1"}
    assert set(first) == keys
    again = _data_from_args(parse_args(argv))[0].batch([0], "cuda")
    torch.cuda.synchronize()
    assert _bytes(first) == _bytes(again)


def _dims_or_unit(average_dims, dataset, **kw):
    """average_dims; a dataset without a car-sized cluster (the tiny trees) measures a fixed size, after the same draws"""
    try:
        return average_dims(dataset, **kw)
    except ValueError:
        return np.array([1.8, 1.5, 4.2], np.float32) * (1.0 + 0.1 * len(dataset))


# ------------------------------------------------------------------ training
@pytest.mark.timeout(300)
def test_two_cosmix_steps_over_augmented_items_repeat(tmp_path):
    from lidog_amd.trainer import SourceStep
    argv = ["--model", "MinkUNet34", "--mix", "cosmix", "--source-augment", ROT, SCALE, "--config", "source8k",
            "--epochs", "1", "--scans", "2", "--batch", "1"]
    losses = []
    for run in range(2):
        fit = _fit_from_args(parse_args(argv + ["--save-dir", str(tmp_path / str(run))]))
        fit.log = lambda *_: None
        assert isinstance(fit.train_data, MixedSynthScans) and isinstance(fit.train_data.items, AugmentedSynthScans)
        assert type(fit.step) is SourceStep and fit.step.num_sources == 1
        hist = fit.run()
        assert len(hist) == 1 and len(hist[0]["losses"]) == 2 and np.isfinite(hist[0]["losses"]).all()
        losses.append(np.asarray(hist[0]["losses"], dtype=np.float64))
    print("losses", losses[0], losses[1])
    assert losses[0].tobytes() == losses[1].tobytes()
