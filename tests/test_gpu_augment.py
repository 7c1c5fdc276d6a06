"""The training augmentation on the GPU: lidog_amd.data.augment_item equals the reference's item on every G13 case and
augment_ref's restatement on full-size scans (integer outputs exactly, float64 xyz within the bound of the arithmetic,
face / threshold margins asserted on every input), the stable compaction equals np.flatnonzero, empty and full
sub-samples, items made twice and next to a queued training step, and --augment fits that validate, save and resume."""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

import augment_ref as A
from lidog_amd import data
from lidog_amd.data import augment_item, augment_points, draw_augmentation

pytestmark = pytest.mark.gpu

META, G13 = A.load_g13()
CASES = sorted(A.CASES)
BOTH = [A.ROT, A.SCALE]


def _device(pts, feats, labels):
    return {"points": torch.from_numpy(pts).cuda(), "features": torch.from_numpy(feats).cuda(),
            "sem_labels": torch.from_numpy(labels).cuda()}


def _host(item):
    return {k: v.cpu().numpy() for k, v in item.items()}


@functools.lru_cache(maxsize=None)
def _full_scan(config, scan):
    return A.make_points(config, scan)


def _check(got, want, bound, what):
    assert got["coordinates"].dtype == np.int32 and got["index"].dtype == np.int64
    assert got["sampled_idx"].dtype == np.int64 and got["inverse_map"].dtype == np.int64
    A.compare(got, want, bound, what)


# ------------------------------------------------------------------ the reference's items
@pytest.mark.parametrize("name", CASES)
def test_item_equals_the_reference(name):
    case = A.CASES[name]
    pts, feats, labels = A.case_input(case)
    draws = A.case_draws(name, G13)
    p, mag = A.transform_np(pts[draws["sampled_idx"]], draws["ops"])
    face, thr = A.margins(p, A.VOXEL, case["form"] == "bev")
    assert face > A.MARGIN and thr > A.MARGIN
    np.random.seed(case["seed"])                    # the draws are made here, not read from the fixture
    mine = draw_augmentation(np.random, pts.shape[0], case["sub_p"], case["augs"])
    assert np.array_equal(mine["sampled_idx"], draws["sampled_idx"])
    assert all(np.array_equal(g, w) for (_, g), (_, w) in zip(mine["ops"], draws["ops"]))
    item = augment_item(_device(pts, feats, labels), mine, A.VOXEL, bounds=case["form"] == "bev", ignore_label=A.IGNORE,
                        bev=A.BEV if case["form"] == "bev" else None, bev_from=case["bev_from"])
    got = _host(item)
    want = A.case_outputs(name, G13)
    assert got["coordinates"].shape[0] == META["cases"][name]["voxels"]
    if mag is None:
        bound = None
    else:       # the bound of the kept first points: through the restatement's own bookkeeping
        bound = A.augment_np(pts, feats, labels, draws, A.VOXEL, case["form"] == "bev")["_xyz_bound"]
    _check(got, want, bound, name)


# ------------------------------------------------------------------ full-size scans against the restatement
@pytest.mark.parametrize("config,scan,form,augs,sub_p,seed", [
    ("kitti120k", 0, "bev", BOTH, 0.8, 7), ("kitti120k", 1, "bev", BOTH, 0.8, 8), ("kitti120k", 2, "plain", BOTH, 0.8, 9),
    ("kitti120k", 3, "bev", [A.SCALE, A.ROT], 0.8, 10), ("kitti120k", 4, "bev", [A.SCALE], 0.8, 11),
    ("kitti120k", 5, "plain", [], 0.8, 12), ("kitti120k", 6, "bev", [A.ROT], None, 13),
    ("nusc35k", 0, "bev", BOTH, 0.8, 14), ("nusc35k", 1, "plain", BOTH, 0.8, 15), ("nusc35k", 2, "plain", BOTH, 1.0, 16),
    ("nusc35k", 3, "bev", [A.SCALE], 0.8, 17), ("nusc35k", 4, "plain", [A.SCALE, A.ROT], None, 18)])
def test_full_size_item_equals_the_restatement(config, scan, form, augs, sub_p, seed):
    pts, feats, labels = _full_scan(config, scan)
    draws = draw_augmentation(np.random.RandomState(seed), pts.shape[0], sub_p, augs)
    bev = A.BEV if form == "bev" else None
    for bev_from in (("voted", "first") if form == "bev" and scan % 2 == 0 else ("voted",)):
        want = A.augment_np(pts, feats, labels, draws, A.VOXEL, form == "bev", A.IGNORE, bev, bev_from)
        face, thr = want["_margins"]
        assert face > A.MARGIN and thr > A.MARGIN, (face, thr)
        got = _host(augment_item(_device(pts, feats, labels), draws, A.VOXEL, bounds=form == "bev",
                                 ignore_label=A.IGNORE, bev=bev, bev_from=bev_from))
        assert got["coordinates"].shape[0] > 0.5 * draws["sampled_idx"].shape[0]
        _check(got, want, want["_xyz_bound"], f"{config}/{scan}/{form}/{bev_from}")


# ------------------------------------------------------------------ the kernel: stable compaction, sizes, dtypes
def _masked_points(mask, rng):
    """points inside the bounds where mask, outside them (beyond a bound, or in the ego box) elsewhere"""
    n = mask.shape[0]
    inside = np.stack([rng.uniform(4, 55, n) * rng.choice([-1, 1], n), rng.uniform(3, 55, n) * rng.choice([-1, 1], n),
                       rng.uniform(-9, 7, n)], axis=1)
    kind = rng.integers(0, 4, n)
    outside = inside.copy()
    outside[kind == 0, 0] = 61.5
    outside[kind == 1, 1] = -60.0            # on the threshold: strict comparison drops it
    outside[kind == 2, 2] = 8.0
    outside[kind == 3, :2] = rng.uniform(-1.9, 1.9, (int((kind == 3).sum()), 2))
    return np.where(mask[:, None], inside, outside).astype(np.float32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 100003])
def test_compaction_equals_flatnonzero(n):
    rng = np.random.default_rng(n)
    for mask in (rng.random(n) < 0.5, rng.random(n) < 0.03, np.ones(n, bool), np.zeros(n, bool)):
        pts = torch.from_numpy(_masked_points(mask, rng)).cuda()
        labels = torch.arange(n, dtype=torch.int32, device="cuda") * 3
        rows, xyz, src, lab, info = augment_points(pts, None, [], A.VOXEL, bounds=True, labels=labels)
        kept, bad = info.cpu().tolist()
        want = np.flatnonzero(mask)
        assert bad == 0 and kept == want.shape[0]
        np.testing.assert_array_equal(src.cpu().numpy()[:kept], want)
        np.testing.assert_array_equal(lab.cpu().numpy()[:kept], want * 3)
        assert torch.equal(xyz[:kept], pts[torch.from_numpy(want).cuda()])
        c = np.floor(pts.cpu().numpy()[want] / np.float32(A.VOXEL)).astype(np.int32)
        np.testing.assert_array_equal(rows.cpu().numpy()[:kept], np.concatenate([np.zeros((kept, 1), np.int32), c], 1))
        rows2, _, src2, _, info2 = augment_points(pts, None, [], A.VOXEL, bounds=True, labels=labels)
        assert torch.equal(src2[:kept], src[:kept]) and torch.equal(rows2[:kept], rows[:kept])
        assert info2.cpu().tolist() == [kept, 0]


def test_compaction_follows_the_sampled_order():
    rng = np.random.default_rng(3)
    n = 50000
    mask = rng.random(n) < 0.6
    pts = _masked_points(mask, rng)
    perm = rng.permutation(n)[:40000]
    idx = torch.from_numpy(perm.astype(np.int32)).cuda()
    _, _, src, _, info = augment_points(torch.from_numpy(pts).cuda(), idx, [], A.VOXEL, bounds=True)
    kept = info.cpu().tolist()[0]
    np.testing.assert_array_equal(src.cpu().numpy()[:kept], perm[mask[perm]])


def test_point_arithmetic_follows_numpy_dtype_rules():
    pts, _, _ = _full_scan("nusc35k", 5)
    d = draw_augmentation(np.random.RandomState(2), pts.shape[0], None, [A.SCALE, A.ROT, A.SCALE, A.ROT])
    dev = torch.from_numpy(pts).cuda()
    for ops in ([], d["ops"][:1], d["ops"][1:2], d["ops"][:2], d["ops"][1:3], d["ops"]):
        want, mag = A.transform_np(pts, ops)
        rows, xyz, src, _, _ = augment_points(dev, None, ops, A.VOXEL)
        got = xyz.cpu().numpy()
        assert got.dtype == want.dtype
        assert np.array_equal(got, want)       # the plain chain on both sides: bit for bit, float64 included
        assert A.margins(want)[0] > A.MARGIN
        c = np.floor(want / np.asarray(A.VOXEL, dtype=want.dtype)).astype(np.int32)
        np.testing.assert_array_equal(rows.cpu().numpy()[:, 1:], c)
        assert torch.equal(src.cpu(), torch.arange(pts.shape[0], dtype=torch.int32))


def test_empty_and_full_subsamples():
    pts, feats, labels = _full_scan("nusc35k", 6)
    scan = _device(pts, feats, labels)
    empty = _device(pts[:0], feats[:0], labels[:0])
    for bounds in (False, True):
        bev = A.BEV if bounds else None
        for sc, n, sub_p in ((empty, 0, 0.8), (empty, 0, None), (_device(pts[:1], feats[:1], labels[:1]), 1, 0.8)):
            d = draw_augmentation(np.random.RandomState(1), n, sub_p, BOTH)      # n = 0 and int(sub_p * n) = 0
            if sub_p is not None:
                assert d["sampled_idx"].shape == (0,)
            out = augment_item(sc, d, A.VOXEL, bounds=bounds, bev=bev)
            assert out["coordinates"].shape == (0, 3) and out["xyz"].shape == (0, 3) and out["xyz"].dtype == torch.float64
            assert out["features"].shape == (0, 1) and out["inverse_map"].shape == (0,)
            if bounds:
                assert bool((out["bev_labels"] == -1).all()) and out["bev_labels"].shape == (A.BEV[1], A.BEV[1])
        d = draw_augmentation(np.random.RandomState(2), pts.shape[0], 1.0, BOTH)       # sub_p = 1.0: a permutation
        assert np.array_equal(np.sort(d["sampled_idx"]), np.arange(pts.shape[0]))
        want = A.augment_np(pts, feats, labels, d, A.VOXEL, bounds, A.IGNORE, bev)
        assert min(want["_margins"]) > A.MARGIN
        _check(_host(augment_item(scan, d, A.VOXEL, bounds=bounds, bev=bev)), want, want["_xyz_bound"], "sub_p 1.0")


def test_refusals():
    pts, feats, labels = _full_scan("nusc35k", 6)
    d = draw_augmentation(np.random.RandomState(1), 100, 0.8, [])
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        augment_item({"points": torch.from_numpy(pts), "features": torch.from_numpy(feats),
                      "sem_labels": torch.from_numpy(labels)}, d)
    scan = _device(pts[:50], feats[:50], labels[:50])
    with pytest.raises(ValueError, match="outside the scan"):
        augment_item(scan, d)                    # drawn for 100 rows
    with pytest.raises(KeyError):
        augment_item({"points": scan["points"]}, d)
    with pytest.raises(RuntimeError, match="at most 4"):
        augment_points(scan["points"], None, [(A.SCALE, np.ones(3))] * 5)


def _digest(item):
    h = hashlib.sha1()
    for k in sorted(item):
        h.update(np.ascontiguousarray(item[k].cpu().numpy()).tobytes())
    return h.hexdigest()


def _reachable(obj):
    """the test's own walk over a batch: every CUDA tensor, nested ones included"""
    if torch.is_tensor(obj):
        return [obj] if obj.is_cuda else []
    if isinstance(obj, dict):
        return [t for v in obj.values() for t in _reachable(v)]
    if isinstance(obj, (list, tuple)):
        return [t for v in obj for t in _reachable(v)]
    return []


def test_item_twice_and_next_to_a_queued_training_step():
    """Fit.run's situation: a training step is queued on the caller's stream, the next batch is made on the merge stream
    without waiting for it, the batch before is dropped.  The items equal the ones made on an idle device."""
    from lidog_amd.train import AugmentedSynthScans, bev_image_size, build_model, build_step
    pts, feats, labels = _full_scan("kitti120k", 7)
    scan = _device(pts, feats, labels)
    d = draw_augmentation(np.random.RandomState(4), pts.shape[0], 0.8, BOTH)
    first = _digest(augment_item(scan, d, A.VOXEL, bounds=True, bev=A.BEV))
    assert _digest(augment_item(scan, d, A.VOXEL, bounds=True, bev=A.BEV)) == first
    size = bev_image_size(50.0)
    ds = AugmentedSynthScans(4, "nusc35k", BOTH, seed=9, bev=(50.0, size))
    flat = lambda b: {f"{k}/{j}": t for k, v in b.items() for j, t in enumerate(_reachable(v))}
    quiet = []
    for i in range(4):
        quiet.append(_digest(flat(ds.batch([i], "cuda"))))
        torch.cuda.synchronize()
    torch.manual_seed(0)
    model, step, _ = build_step(build_model("MinkUNet34BEV"), "MinkUNet34BEV", lr=1e-3)
    assert torch.cuda.current_stream() != data.merge_stream("cuda")
    busy, kept = [], []
    cur = ds.batch([0], "cuda")
    for i in range(4):                                   # no synchronisation inside: the host runs ahead of the device
        nxt = ds.batch([i + 1], "cuda") if i < 3 else None
        out = step.training_step(cur, epoch=0, prefetch=nxt)
        kept.append({k: t + 0 for k, t in flat(cur).items()})      # read on the caller's stream, behind the step
        item = augment_item(scan, d, A.VOXEL, bounds=True, bev=A.BEV)        # and a single item next to the queued step
        busy.append({k: v + 0 for k, v in item.items()})
        cur = nxt
    torch.cuda.synchronize()
    assert np.isfinite(float(out["loss"]))
    assert [_digest(k) for k in kept] == quiet
    assert all(_digest(b) == first for b in busy)


def test_every_tensor_of_a_batch_is_handed_over(monkeypatch):
    """every CUDA tensor reachable from the batch, the nested BEV label images included, is recorded on the caller's
    stream when the batch crosses from the merge stream (else the allocator may reuse it under a queued step)"""
    from lidog_amd.train import AugmentedSynthScans, bev_image_size
    seen = []
    real = torch.Tensor.record_stream

    def record(t, stream):
        seen.append((t.data_ptr(), stream))
        return real(t, stream)

    monkeypatch.setattr(torch.Tensor, "record_stream", record)
    cur = torch.cuda.current_stream()
    assert cur != data.merge_stream("cuda")
    for configs in ("nusc35k", ("nusc35k", "source8k")):
        ds = AugmentedSynthScans(2, configs, BOTH, seed=2, bev=(50.0, bev_image_size(50.0)))
        seen.clear()
        b = ds.batch([0, 1], "cuda")
        tensors = _reachable(b)
        nested = [t for v in b.values() if isinstance(v, dict) for t in _reachable(v)]
        assert len(nested) == ds.num_sources and len(tensors) == 5 * ds.num_sources
        for t in tensors:
            assert (t.data_ptr(), cur) in seen
    torch.cuda.synchronize()
    # the merges' and the single item's dicts cross the same way
    pts, feats, labels = _full_scan("nusc35k", 6)
    seen.clear()
    item = augment_item(_device(pts, feats, labels), draw_augmentation(np.random.RandomState(1), pts.shape[0], 0.8, BOTH),
                        A.VOXEL, bounds=True, bev=A.BEV)
    assert all((t.data_ptr(), cur) in seen for t in _reachable(item)) and len(_reachable(item)) == 10


# ------------------------------------------------------------------ training
def _recording(fit, log):
    inner = fit.train_data.batch

    def batch(indices, device):
        b = inner(indices, device)
        log.append((fit.train_data.epoch, tuple(int(i) for i in indices), _digest(
            {k: v for k, v in b.items() if torch.is_tensor(v)} | {f"bev_{k}": v["block8"] for k, v in b.items()
                                                                 if isinstance(v, dict)})))
        return b

    fit.train_data.batch = batch


@pytest.mark.timeout(600)
@pytest.mark.parametrize("model", ["MinkUNet34BEV", "MinkUNet34"])
def test_cli_augment_fit_validate_resume(model, tmp_path):
    from lidog_amd.train import AugmentedSynthScans, SynthScans, _fit_from_args, parse_args
    argv = ["--model", model, "--augment", "RandomRotation", "RandomScale", "--config", "nusc35k", "--scans", "2",
            "--batch", "1", "--val-scans", "1", "--check-val-every-n-epoch", "1"]
    fit = _fit_from_args(parse_args(argv + ["--epochs", "2", "--save-dir", str(tmp_path / "a")]))
    fit.log = lambda *_: None
    assert isinstance(fit.train_data, AugmentedSynthScans) and type(fit.val_data) is SynthScans     # never augmented
    assert (fit.train_data.bev is not None) == (model == "MinkUNet34BEV")
    whole = []
    _recording(fit, whole)
    hist = fit.run()
    assert len(hist) == 2 and all(np.isfinite(h["losses"]).all() for h in hist) and fit.train_data.epoch == 1
    assert all(np.isfinite(h["validation"]["sem_loss"]) for h in hist) and os.path.exists(hist[1]["checkpoint"])
    assert len({d for _, _, d in whole}) == 4                   # every item of every epoch is another point set
    # one epoch, then a resumed run for the second
    one = _fit_from_args(parse_args(argv + ["--epochs", "1", "--save-dir", str(tmp_path / "b")]))
    one.log = lambda *_: None
    one.run()
    again = _fit_from_args(parse_args(argv + ["--epochs", "2", "--save-dir", str(tmp_path / "b"), "--auto-resume"]))
    again.log = lambda *_: None
    assert again.epoch == 1
    resumed = []
    _recording(again, resumed)
    h2 = again.run()
    assert len(h2) == 1 and h2[0]["epoch"] == 1
    assert sorted(resumed) == sorted(x for x in whole if x[0] == 1) and len(resumed) == 2
    assert np.isfinite(h2[0]["losses"]).all()


def test_batch_keys_and_bev_labels():
    from lidog_amd.train import AugmentedSynthScans, bev_image_size
    size = bev_image_size(50.0)
    ds = AugmentedSynthScans(3, "nusc35k", BOTH, seed=5, bev=(50.0, size))
    b = ds.batch([2, 0], "cuda")
    torch.cuda.synchronize()
    assert set(b) == {"coords_int", "source_coordinates0", "source_features0", "source_sem_labels0", "source_bev_labels0"}
    img = b["source_bev_labels0"]["block8"]
    assert img.shape == (2, size, size) and img.dtype == torch.int64 and int(img.max()) >= 0
    assert b["coords_int"].dtype == torch.int32 and b["coords_int"][:, 0].unique().tolist() == [0, 1]
    assert b["source_sem_labels0"].dtype == torch.int64
    x = b["coords_int"][:, 1:].float() * 0.05                  # the bounds filter ran: nothing in the ego box
    assert not bool(((x[:, 0] > -2.9) & (x[:, 0] < 2.9) & (x[:, 1] > -1.9) & (x[:, 1] < 1.9)).any())
    for s, i in enumerate((2, 0)):                              # each item equals the restatement with the dataset's draws
        pts, labels = ds.points(0, i)
        (_, _, draws), = ds.item(i)
        want = A.augment_np(pts, np.ones((pts.shape[0], 1), np.float32), labels, draws, 0.05, True, -1, (50.0, size))
        rows = b["coords_int"][:, 0] == s
        np.testing.assert_array_equal(b["coords_int"][rows][:, 1:].cpu().numpy(), want["coordinates"])
        np.testing.assert_array_equal(b["source_sem_labels0"][rows].cpu().numpy(), want["sem_labels"])
        np.testing.assert_array_equal(img[s].cpu().numpy(), want["bev_labels"])
    plain = AugmentedSynthScans(3, "nusc35k", BOTH, seed=5).batch([2, 0], "cuda")
    assert "source_bev_labels0" not in plain and plain["coords_int"].shape[0] > b["coords_int"].shape[0]


@pytest.mark.timeout(300)
def test_two_source_step():
    from lidog_amd.train import AugmentedSynthScans, _fit_from_args, parse_args
    fit = _fit_from_args(parse_args(["--model", "MinkUNet34BEV", "--augment", "RandomRotation", "RandomScale", "--sources",
                                     "nusc35k", "nusc35k", "--scans", "2", "--batch", "2", "--epochs", "1"]))
    fit.log = lambda *_: None
    assert isinstance(fit.train_data, AugmentedSynthScans) and fit.step.num_sources == 2
    b = fit.train_data.batch([0, 1], "cuda")
    assert {"coords_int", "coords_int1", "source_bev_labels0", "source_bev_labels1"} <= set(b)
    hist = fit.run()
    assert len(hist) == 1 and len(hist[0]["losses"]) == 1 and np.isfinite(hist[0]["losses"]).all()
