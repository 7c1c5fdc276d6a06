"""Test-time augmentation on the GPU: lidog_tta_vote at block edges, with special values and with inverse entries out of
range, against the float64 restatement (tta_ref) and the torch composition; the rows of tta.view_batch bit for bit
against the restatement; eval_target --tta end to end on three tiny SemanticKITTI files."""
import glob
import json
import os
import shutil

import numpy as np
import pytest
import torch

import pointlabels_ref as P
import tta_ref as R
from lidog_amd import eval_target, evaluate, scans, tta
from lidog_amd.checkpoint import load_lightning_checkpoint, save_lightning_checkpoint
from lidog_amd.train import build_model

pytestmark = pytest.mark.gpu

V = 3                                           # accumulations of the kernel tests: first, then two adds
KS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
POISON = -12345.5


def _views(k, m, c, seed, n_views=V):
    """[(logits float32 [m, c] = 4 randn, inverse int64 [k] with repeats)] on the host, seeded"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n_views):
        logits = 4 * torch.randn(m, c, generator=g)
        inverse = torch.randint(0, m, (k,), generator=g) if m else torch.zeros(0, dtype=torch.int64)
        out.append((logits, inverse))
    return out


def _kernel(views, mode, c, poison=float("nan")):
    k = views[0][1].shape[0]
    acc = torch.full((k, c), poison, dtype=torch.float32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    for v, (logits, inverse) in enumerate(views):
        tta.vote(logits.cuda(), inverse.cuda(), acc, mode, first=v == 0, err=err)
    return acc, err


def _torch_composition(views, mode, c):
    """index_select -> softmax / one-hot -> add_ on the device"""
    acc = None
    for logits, inverse in views:
        x = logits.cuda()
        if mode == "prob":
            s = torch.softmax(x, dim=1)
        elif mode == "vote":
            s = torch.nn.functional.one_hot(x.argmax(dim=1), c).float() if x.shape[0] else x
        else:
            s = x
        s = s.index_select(0, inverse.cuda())
        acc = s.clone() if acc is None else acc.add_(s)
    return acc


# ------------------------------------------------------------------ 1. the kernel at edge sizes
@pytest.mark.parametrize("c", [2, 7, 19, 20])
def test_vote_edge_sizes(c):
    bound = R.prob_bound(V, c)
    worst = 0.0
    for k in KS:
        for m in sorted({1, 5, k} - {0}):       # m = 1: every point goes to one row
            views = _views(k, m, c, seed=1000 * c + 7 * k + m)
            for mode in tta.MODES:
                acc, err = _kernel(views, mode, c)      # the NaN poison is overwritten by first = 1
                assert err.item() == 0 and acc.shape == (k, c)
                if k == 0:
                    continue
                want = _torch_composition(views, mode, c)
                if mode != "prob":
                    assert torch.equal(acc, want), (k, m, mode)     # bit for bit
                else:
                    ref = R.vote([(l.numpy(), i.numpy()) for l, i in views], "prob")
                    d = float(np.abs(acc.cpu().numpy().astype(np.float64) - ref).max())
                    worst = max(worst, d)
                    assert d <= bound, (k, m, d, bound)
    print(f"C = {c}: worst |prob - float64| = {worst:.3e}, bound {bound:.3e}")


def test_first_overwrites_and_later_views_add():
    views = _views(300, 40, 7, seed=3, n_views=2)
    for mode in tta.MODES:
        acc = torch.full((300, 7), float("inf"), dtype=torch.float32, device="cuda")
        one = tta.vote(views[0][0].cuda(), views[0][1].cuda(), acc, mode, first=True)
        assert one is acc and bool(torch.isfinite(acc).all())
        first = acc.clone()
        tta.vote(views[1][0].cuda(), views[1][1].cuda(), acc, mode, first=False)
        second = torch.empty_like(acc)
        tta.vote(views[1][0].cuda(), views[1][1].cuda(), second, mode, first=True)
        assert torch.equal(acc, first + second)                     # one plain fp32 add per element
        again = torch.full((300, 7), POISON, dtype=torch.float32, device="cuda")
        tta.vote(views[0][0].cuda(), views[0][1].cuda(), again, mode, first=True)
        assert torch.equal(again, first)                            # the same bytes on every run


# ------------------------------------------------------------------ 2. labels
def test_labels_equal_float64_outside_the_margin():
    k, m, c, nv = 40000, 9000, 7, 4
    views = _views(k, m, c, seed=11, n_views=nv)
    ref = R.vote([(l.numpy(), i.numpy()) for l, i in views], "prob")
    top = np.sort(ref, axis=1)
    sure = top[:, -1] - top[:, -2] > 2 * R.prob_bound(nv, c)
    left_out = int((~sure).sum())
    print(f"points inside twice the bound: {left_out} of {k}")
    assert left_out <= k // 1000                                    # at most 0.1 %
    acc, err = _kernel(views, "prob", c)
    assert err.item() == 0
    got = acc.argmax(dim=1).cpu().numpy()
    assert np.array_equal(got[sure], ref.argmax(axis=1)[sure])
    # the route of the evaluation: point_labels over acc with every kept row its own "voxel"
    ids, _ = evaluate.point_labels(acc, [0, k], [0, k], [0, k], torch.arange(k, dtype=torch.int32, device="cuda"),
                                   torch.arange(k, dtype=torch.int64, device="cuda"))
    assert np.array_equal(ids.cpu().numpy().astype(np.int64)[sure], ref.argmax(axis=1)[sure])


# ------------------------------------------------------------------ 3. special values
def test_special_values_stay_in_their_rows():
    c, m, k = 7, 12, 700
    g = torch.Generator().manual_seed(5)
    views = _views(k, m, c, seed=5, n_views=2)
    nan, inf = float("nan"), float("inf")
    l0 = views[0][0]
    l0[1, 3] = nan                                                  # a NaN
    l0[2, 0] = inf                                                  # +inf: inf - inf
    l0[3, 5] = -inf                                                 # -inf beside finite values: probability 0
    l0[4, :] = -inf                                                 # nothing but -inf
    l0[5, 2] = nan
    l0[5, 4] = nan                                                  # two NaN: the first one is voted for
    l0[6, 1] = inf
    l0[6, 2] = nan
    l0[7, 6] = inf
    l0[7, 0] = inf
    views[0] = (l0, torch.arange(k) % m)
    views[1] = (views[1][0], torch.randint(0, m, (k,), generator=g))
    for mode in tta.MODES:
        acc, err = _kernel(views, mode, c)
        assert err.item() == 0
        want = _torch_composition(views, mode, c) if mode != "vote" else \
            torch.from_numpy(R.vote([(l.numpy(), i.numpy()) for l, i in views], "vote")).float().cuda()
        assert torch.equal(torch.isnan(acc), torch.isnan(want)), mode
        a, w = acc.cpu().numpy().astype(np.float64), want.cpu().numpy().astype(np.float64)
        ok = ~np.isnan(w)
        if mode == "prob":
            assert np.abs(a[ok] - w[ok]).max() <= 2 * R.prob_bound(2, c)      # two fp32 softmaxes side by side
            rows = np.isnan(a).all(axis=1)
            assert np.array_equal(rows, np.isin(np.arange(k) % m, [1, 2, 4, 5, 6, 7]))      # whole rows, only those
            assert not np.isnan(a[~rows]).any()
            ref = R.vote([(l.numpy(), i.numpy()) for l, i in views], "prob")
            assert np.abs(a[~rows] - ref[~rows]).max() <= R.prob_bound(2, c)
            hit = (np.arange(k) % m == 3) & ~rows
            s1 = R.scores(views[1][0].numpy(), "prob")[views[1][1].numpy()]
            assert np.abs(a[hit, 5] - s1[hit, 5]).max() <= R.prob_bound(2, c)   # exp(-inf) added exactly 0
        else:
            assert np.array_equal(a[ok], w[ok]), mode
    # vote: the first NaN of a row wins, then the first maximum
    acc = torch.empty((m, c), dtype=torch.float32, device="cuda")
    tta.vote(l0.cuda(), torch.arange(m, device="cuda"), acc, "vote", first=True)
    top = acc.argmax(dim=1).cpu().tolist()
    assert bool((acc.sum(dim=1) == 1).all())
    assert top[1] == 3 and top[5] == 2 and top[6] == 2 and top[2] == 0 and top[7] == 0 and top[4] == 0
    assert top == P.argmax_np(l0.numpy()).tolist()


# ------------------------------------------------------------------ 4. inverse entries out of range
@pytest.mark.parametrize("mode", tta.MODES)
def test_out_of_range_inverse_is_reported_and_skipped(mode):
    c, m, k = 7, 50, 1025
    views = _views(k, m, c, seed=9, n_views=2)
    bad = [0, 63, 64, 500, 1024]
    broken = views[1][1].clone()
    broken[bad] = torch.tensor([-1, m, -1, m, 2 ** 40])
    acc = torch.full((k, c), POISON, dtype=torch.float32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    tta.vote(views[0][0].cuda(), broken.cuda(), acc, mode, first=True, err=err)
    assert err.item() == 1
    good = torch.ones(k, dtype=torch.bool, device="cuda")
    good[bad] = False
    want = _torch_composition([(views[0][0], views[1][1])], mode, c)
    assert bool((acc[bad] == POISON).all())                         # neither read nor written
    if mode == "prob":
        assert float((acc - want)[good].abs().max()) <= 2 * R.prob_bound(1, c)
    else:
        assert torch.equal(acc[good], want[good])
    before = acc.clone()
    tta.vote(views[1][0].cuda(), broken.cuda(), acc, mode, first=False, err=err)
    assert err.item() == 1 and torch.equal(acc[bad], before[bad]) and not torch.equal(acc[good], before[good])
    with pytest.raises(ValueError, match="outside the view's voxel rows"):
        tta.vote(views[0][0].cuda(), broken.cuda(), acc, mode, first=True)
    clean = torch.zeros(1, dtype=torch.int32, device="cuda")
    tta.vote(views[0][0].cuda(), views[0][1].cuda(), acc, mode, first=True, err=clean)
    assert clean.item() == 0


# ------------------------------------------------------------------ 5. views
VOXEL = 0.05
VIEW_NAMES = ("rotz90", "rotz180+flipx", "flipy", "scale0.95", "rotz7.5")


def _hand_points(seed):
    """points on voxel faces, exact multiples of the voxel size, negative coordinates, several points per voxel"""
    rng = np.random.RandomState(seed)
    q = np.float32(VOXEL)
    cells = rng.randint(-40, 40, size=(60, 3))
    faces = (cells.astype(np.float32) * q)                          # the float32 product: on or beside a face
    exact = cells[:20].astype(np.float64) * 0.05                    # the float64 multiple, rounded to float32
    inside = (cells[:40] + rng.rand(40, 3)).astype(np.float32) * q
    twins = inside[:15] + np.float32(1e-4)
    axes = np.array([[0, 0, 0], [0.05, 0, 0], [-0.05, 0, 0], [0, -0.05, 0.05], [1.0, -1.0, 0.5], [-2.0, 2.0, -0.5],
                     [0.1, 0.2, 0.3], [-0.1, -0.2, -0.3], [0.15, -0.15, 0.35]])
    return np.concatenate([faces, exact.astype(np.float32), inside, twins, axes.astype(np.float32)]).astype(np.float32)


def _item(points):
    pts = torch.from_numpy(points).cuda()
    n = points.shape[0]
    return {"points": pts, "plain": True, "kept": n, "voxel_size": VOXEL, "path": "hand-made",
            "inverse_map": torch.zeros(n, dtype=torch.int64, device="cuda")}


@pytest.mark.parametrize("name", VIEW_NAMES)
def test_view_rows_equal_the_restatement(name):
    scans_np = [_hand_points(1), _hand_points(2)[::-1].copy()]      # two scans in one batch
    items = [_item(p) for p in scans_np]
    (view,) = tta.parse_views([name])[1:]
    coords, feats, inverse = tta.view_batch(items, view)
    want = np.concatenate([R.view_rows(p, R.view_ops(name), VOXEL, batch=b) for b, p in enumerate(scans_np)])
    assert coords.dtype == torch.int32 and coords.shape[1] == 4 and inverse.dtype == torch.int64
    assert feats.dtype == torch.float32 and feats.shape == (coords.shape[0], 1) and bool((feats == 1).all())
    assert inverse.shape[0] == want.shape[0] and int(inverse.min()) >= 0 and int(inverse.max()) < coords.shape[0]
    got = coords[inverse].cpu().numpy()
    assert np.array_equal(got, want)                                # every point sits in the row of its floored coordinate
    uniq = np.unique(want, axis=0)
    assert coords.shape[0] == uniq.shape[0] < want.shape[0]         # one row per voxel, several points in some
    assert np.array_equal(np.unique(coords.cpu().numpy(), axis=0), uniq)
    n0 = scans_np[0].shape[0]
    assert bool((coords[inverse[:n0]][:, 0] == 0).all()) and bool((coords[inverse[n0:]][:, 0] == 1).all())
    if name == "rotz90":                                            # an exact permutation: (x, y, z) -> (y, -x, z)
        p = scans_np[0]
        perm = np.stack([p[:, 1], -p[:, 0], p[:, 2]], axis=1).astype(np.float64)
        assert np.array_equal(want[:n0, 1:], np.floor(perm / 0.05).astype(np.int32))
    # the identity view gives the voxels of the plain item
    coords0, _, inverse0 = tta.view_batch(items, tta.View("identity"))
    plain = np.concatenate([R.view_rows(p, [], VOXEL, batch=b) for b, p in enumerate(scans_np)])
    assert np.array_equal(coords0[inverse0].cpu().numpy(), plain)
    for broken in (dict(items[0], plain=False), {k: v for k, v in items[0].items() if k != "points"},
                   dict(items[0], kept=items[0]["kept"] - 1)):
        with pytest.raises(ValueError, match="test-time augmentation need one query per kept row"):
            tta.view_batch([broken], view)


# ------------------------------------------------------------------ 6. end to end
OUT_IDS = [10, 30, 40, 48, 72, 50, 70]          # the id written for every common class: not the identity, injective
FILL = 250
BATCHES = [[0, 1], [2]]                         # --batch 2 over three scans
RUNS = {"plain": [], "logit": ["--tta", "rotz180", "flipy", "--tta-mode", "logit"], "rot4": ["--tta", "rot4"]}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("tta"))
    tree, label_map, lut = P.write_tiny_kitti_tree(os.path.join(root, "kitti"))
    inv = os.path.join(root, "common2kitti.json")
    with open(inv, "w") as f:
        json.dump({"learning_map_inv": dict({str(c): i for c, i in enumerate(OUT_IDS)}, **{"-1": FILL})}, f)
    torch.manual_seed(5)
    model = build_model("MinkUNet34")
    ckpts = {}
    for name in RUNS:
        os.makedirs(os.path.join(root, name, "checkpoints"))
        ckpts[name] = os.path.join(root, name, "checkpoints", "fresh.ckpt")
    save_lightning_checkpoint(model, ckpts["plain"])
    res = {}
    for name, extra in RUNS.items():
        if name != "plain":
            shutil.copyfile(ckpts["plain"], ckpts[name])
        res[name] = eval_target.main(
            ["--checkpoint", ckpts[name], "--model", "MinkUNet34", "--sources", "SemanticKITTI", "--target-files",
             f"SemanticKITTI={tree}", "--label-maps", label_map, "--batch", "2", "--rows", "scan", "--point-level",
             "--save-labels", "--save-predictions", "--inverse-label-map", inv] + extra)
    return {"root": root, "tree": tree, "lut": lut, "ckpts": ckpts, "res": res}


def _label_file(runs, name, f):
    return os.path.join(runs["root"], name, "predictions", "SemanticKITTI", "sequences", "08", "predictions", f"{f:06d}.label")


def _records(runs, f):
    return np.fromfile(os.path.join(runs["tree"], "sequences", "08", "velodyne", f"{f:06d}.bin"), np.float32).reshape(-1, 4)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _model_and_data(runs):
    model = build_model("MinkUNet34")
    load_lightning_checkpoint(model, runs["ckpts"]["plain"])
    model.eval()
    data = scans.FileScans(scans.listing("SemanticKITTI", runs["tree"], "validation"), runs["lut"], keep_raw=True)
    return model, data


def _own(pitems):
    return torch.cat([torch.arange(it["kept"], dtype=torch.int64, device="cuda") for it in pitems])


def test_voxel_level_outputs_are_those_of_the_plain_run(runs):
    plain = os.path.join(runs["root"], "plain")
    voxel_files = sorted(os.path.relpath(p, plain) for p in glob.glob(os.path.join(plain, "predictions", "**", "*.ply"),
                                                                      recursive=True))
    assert len(voxel_files) == 6                                    # preds and labels of three scans
    for name in ("logit", "rot4"):
        top = os.path.join(runs["root"], name)
        for rel in voxel_files + [os.path.join("results", "SemanticKITTI-TO-SemanticKITTI.csv")]:
            assert _bytes(os.path.join(top, rel)) == _bytes(os.path.join(plain, rel)), (name, rel)
        assert sorted(os.listdir(os.path.join(top, "results"))) == [
            "SemanticKITTI-TO-SemanticKITTI-points-tta.csv", "SemanticKITTI-TO-SemanticKITTI.csv"]
        r, p = runs["res"][name][0], runs["res"]["plain"][0]
        assert np.array_equal(r["counts"], p["counts"]) and np.array_equal(r["iou_rows"], p["iou_rows"])
        assert r["points_csv"].endswith("-points-tta.csv")
        with open(r["points_csv"]) as f:
            table = f.read().splitlines()
        assert len(table) == 2 and table[0] == ",".join(["source", "target"] + list(evaluate.CLASS_NAMES) + ["mean"])
    assert sorted(os.listdir(os.path.join(plain, "results"))) == [
        "SemanticKITTI-TO-SemanticKITTI-points.csv", "SemanticKITTI-TO-SemanticKITTI.csv"]
    assert runs["res"]["logit"][0]["tta_views"] == ["identity", "rotz180", "flipy"]
    assert runs["res"]["logit"][0]["tta_mode"] == "logit"
    assert runs["res"]["rot4"][0]["tta_views"] == ["identity", "rotz90", "rotz180", "rotz270"]
    assert runs["res"]["rot4"][0]["tta_mode"] == "prob" and "tta_views" not in runs["res"]["plain"][0]


def test_logit_run_equals_the_composition_of_its_pieces(runs):
    model, data = _model_and_data(runs)
    run = evaluate.Predictor(model)
    lut = torch.tensor(OUT_IDS, dtype=torch.int32, device="cuda")
    views = tta.parse_views(["rotz180", "flipy"])
    counts = []
    batches = [data.batch(ids, "cuda") for ids in BATCHES]
    differ = 0
    for k, (ids, b) in enumerate(zip(BATCHES, batches)):
        nxt = batches[k + 1]["coords_int"] if k + 1 < len(batches) else None
        with torch.no_grad():
            _, logits = run(b["coords_int"], b["source_features0"], nxt)
            pitems = [data.point_item(i) for i in ids]
            pin = evaluate.point_inputs(pitems)
            inv0 = torch.cat([it["inverse_map"].long() + int(pin["vox_off"][s]) for s, it in enumerate(pitems)])
            acc = logits[inv0].clone()
            for view in views[1:]:
                coords, feats, inverse = tta.view_batch(pitems, view)
                out = evaluate._forward(model, coords, feats)
                assert out.F.shape == (coords.shape[0], 7)
                acc += out.F[inverse]
        want, cnt = evaluate.point_labels(acc, pin["row_off"], pin["kept_off"], pin["kept_off"], pin["keep_row"],
                                          _own(pitems), lut, FILL, pin["labels_raw"], pin["lut"], pin["label_mask"])
        plain, _ = evaluate.point_labels(logits, pin["row_off"], pin["kept_off"], pin["vox_off"], pin["keep_row"],
                                         pin["inverse_map"], lut, FILL)
        differ += int((want != plain).sum())
        counts.append(cnt.cpu().numpy())
        want = want.cpu().numpy()
        for s, i in enumerate(ids):
            got = np.fromfile(_label_file(runs, "logit", i), dtype="<u4")
            assert np.array_equal(got, want[int(pin["row_off"][s]):int(pin["row_off"][s + 1])]), i
    print(f"records whose voted label differs from the plain one: {differ}")
    res = runs["res"]["logit"][0]
    assert np.array_equal(res["point_counts"], np.concatenate(counts)) and res["point_counts"].sum() > 0
    assert res["label_files"] == 3 and res["label_paths"] == [_label_file(runs, "logit", f) for f in range(3)]


def test_rot4_run_writes_well_formed_files(runs):
    res = runs["res"]["rot4"][0]
    assert res["label_files"] == 3
    for f in range(3):
        rec = _records(runs, f)
        keep = P.radius_mask_np(rec[:, :3], 50.0)
        path = _label_file(runs, "rot4", f)
        assert os.path.getsize(path) == 4 * rec.shape[0]            # exactly one uint32 per record, in file order
        got = np.fromfile(path, dtype="<u4")
        assert (got[~keep] == FILL).all() and np.isin(got[keep], OUT_IDS).all() and keep.any() and (~keep).any()
    assert res["point_counts"].shape == (3, 7, 7) and res["point_counts"].sum() == \
        runs["res"]["plain"][0]["point_counts"].sum()               # the same labelled points, voted classes


def test_no_views_reproduce_the_plain_bytes(runs):
    model, data = _model_and_data(runs)
    lut = torch.tensor(OUT_IDS, dtype=torch.int32, device="cuda")
    for name, views in (("none", None), ("empty", [])):
        folder = os.path.join(runs["root"], name, "predictions")
        writer = evaluate.PointLabelWriter(folder, "SemanticKITTI", "SemanticKITTI", data.listings[0].files)
        points = evaluate.PointPath.of(data, "cuda", out_lut=lut, fill=FILL, with_labels=True, on_point_labels=writer,
                                       tta=views, tta_mode="vote")
        res = evaluate.TargetEvaluator(model).run(evaluate.dataset_batches(data, 2, "cuda"), len(data), rows="scan",
                                                  points=points)
        assert "tta_views" not in res and "tta_mode" not in res
        assert np.array_equal(res["point_counts"], runs["res"]["plain"][0]["point_counts"])
        for f in range(3):
            assert _bytes(_label_file(runs, name, f)) == _bytes(_label_file(runs, "plain", f))


def test_constant_logits_give_the_plain_labels_in_every_mode(runs):
    _, data = _model_and_data(runs)
    data.batch([0, 1, 2], "cuda")
    torch.cuda.synchronize()
    pitems = [data.point_item(i) for i in range(3)]
    pin = evaluate.point_inputs(pitems)
    table = torch.stack([torch.roll(torch.arange(7.) - 3, s) for s in range(3)]).cuda()     # per scan, every class another value

    def const(batch_index):
        return table[batch_index.long()].contiguous()

    scan_of_voxel = torch.cat([torch.full((it["voxels"],), s) for s, it in enumerate(pitems)]).cuda()
    plain, plain_counts = evaluate.point_labels(const(scan_of_voxel), pin["row_off"], pin["kept_off"], pin["vox_off"],
                                                pin["keep_row"], pin["inverse_map"], labels_raw=pin["labels_raw"],
                                                lut=pin["lut"], label_mask=pin["label_mask"], fill=FILL)
    inv0 = torch.cat([it["inverse_map"].long() + int(pin["vox_off"][s]) for s, it in enumerate(pitems)])
    built = [tta.view_batch(pitems, v) for v in tta.parse_views(["rot4", "flipx", "flipy", "scale0.95", "rotz7.5+flipx"])[1:]]
    for mode in tta.MODES:
        for n_views in (1, 2, len(built) + 1):
            acc = torch.empty((inv0.shape[0], 7), dtype=torch.float32, device="cuda")
            err = torch.zeros(1, dtype=torch.int32, device="cuda")
            tta.vote(const(scan_of_voxel), inv0, acc, mode, first=True, err=err)
            for coords, _, inverse in built[:n_views - 1]:
                tta.vote(const(coords[:, 0]), inverse, acc, mode, first=False, err=err)
            assert err.item() == 0
            got, counts = evaluate.point_labels(acc, pin["row_off"], pin["kept_off"], pin["kept_off"], pin["keep_row"],
                                                _own(pitems), labels_raw=pin["labels_raw"], lut=pin["lut"],
                                                label_mask=pin["label_mask"], fill=FILL)
            assert torch.equal(got, plain) and torch.equal(counts, plain_counts), (mode, n_views)
    assert int(plain_counts.sum()) > 0
