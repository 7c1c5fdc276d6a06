"""Point labels from interpolated logits (PointPath(interp="trilinear"), eval_target --point-interp) on three tiny
SemanticKITTI files: evaluate.point_logits is features_at_coordinates at the kept points, whose floored queries are the
voxels the points were put into; logits that are constant per scan give the labels of the nearest path; the default
`nearest` writes the bytes of a run without the flag; a trilinear run end to end writes well-formed files that equal
what the interpolated logits of the same model give."""
import csv
import json
import os
import shutil

import numpy as np
import pytest
import torch

import pointlabels_ref as P
from lidog_amd import eval_target, evaluate, scans
from lidog_amd.checkpoint import load_lightning_checkpoint, save_lightning_checkpoint
from lidog_amd.train import build_model

pytestmark = pytest.mark.gpu

OUT_IDS = [10, 30, 40, 48, 72, 50, 70]          # the id written for every common class: not the identity, injective
FILL = 250
BATCHES = [[0, 1], [2]]                         # --batch 2 over three scans
RUNS = ("plain", "nearest", "trilinear")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("interp"))
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
    for name in RUNS[1:]:
        shutil.copyfile(ckpts["plain"], ckpts[name])

    def argv(name):
        return ["--checkpoint", ckpts[name], "--model", "MinkUNet34", "--sources", "SemanticKITTI", "--target-files",
                f"SemanticKITTI={tree}", "--label-maps", label_map, "--batch", "2", "--rows", "scan", "--point-level",
                "--save-labels", "--inverse-label-map", inv]

    res = {"plain": eval_target.main(argv("plain")),
           "nearest": eval_target.main(argv("nearest") + ["--point-interp", "nearest"]),
           "trilinear": eval_target.main(argv("trilinear") + ["--point-interp", "trilinear"])}
    return {"root": root, "tree": tree, "lut": lut, "ckpts": ckpts, "res": res}


def _label_file(runs, name, f):
    return os.path.join(runs["root"], name, "predictions", "SemanticKITTI", "sequences", "08", "predictions", f"{f:06d}.label")


def _records(runs, f):
    return np.fromfile(os.path.join(runs["tree"], "sequences", "08", "velodyne", f"{f:06d}.bin"), np.float32).reshape(-1, 4)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_queries_point_logits_and_constant_logits(runs):
    import lidog_amd.me as ME
    from lidog_amd._lib import call, ptr
    data = scans.FileScans(scans.listing("SemanticKITTI", runs["tree"], "validation"), runs["lut"], keep_raw=True)
    b = data.batch([0, 1, 2], "cuda")
    torch.cuda.synchronize()
    pitems = [data.point_item(i) for i in range(3)]
    pin = evaluate.point_inputs(pitems)
    coords = b["coords_int"]
    query = evaluate.point_queries(pitems)
    kept = int(pin["kept_off"][-1])
    assert query.shape == (kept, 4) and query.dtype == torch.float32
    # the floor of every kept point's query is the coordinate of the voxel the point was put into
    rows = torch.empty((kept, 4), dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    call("lidog_field_floor", ptr(query), kept, 1, ptr(rows), ptr(err))
    assert err.item() == 0
    vox = torch.cat([pin["inverse_map"][int(pin["kept_off"][s]):int(pin["kept_off"][s + 1])].long() + int(pin["vox_off"][s])
                     for s in range(3)])
    assert torch.equal(rows, coords[vox])
    for s in range(3):                      # every scan's points, in load_scan's order, under its batch index
        part = query[int(pin["kept_off"][s]):int(pin["kept_off"][s + 1])]
        assert bool((part[:, 0] == s).all()) and part.shape[0] == pitems[s]["points"].shape[0] > pitems[s]["voxels"]
    # point_logits = features_at_coordinates of the stride-1 logits
    g = torch.Generator().manual_seed(4)
    feats = torch.randn(coords.shape[0], 7, generator=g).cuda()
    st = ME.SparseTensor(features=feats, coordinates=coords)
    pl = evaluate.point_logits(st, pitems)
    assert pl.shape == (kept, 7) and torch.equal(pl, st.features_at_coordinates(query))
    assert bool(torch.isfinite(pl).all()) and not torch.equal(pl, feats[vox])
    # logits constant per scan (every class another value): a positive sum of weights keeps the arg-max, so both paths
    # write the same labels and count the same confusion
    const = torch.stack([torch.roll(torch.arange(7.) - 3, s) for s in range(3)]).cuda()[coords[:, 0].long()].contiguous()
    near, near_counts = evaluate.point_labels(const, pin["row_off"], pin["kept_off"], pin["vox_off"], pin["keep_row"],
                                              pin["inverse_map"], labels_raw=pin["labels_raw"], lut=pin["lut"],
                                              label_mask=pin["label_mask"], fill=FILL)
    pl = evaluate.point_logits(ME.SparseTensor(const, coordinate_manager=st.coordinate_manager, coordinate_map_key=1),
                               pitems)
    own = torch.cat([torch.arange(it["kept"], dtype=torch.int64, device="cuda") for it in pitems])
    tri, tri_counts = evaluate.point_labels(pl, pin["row_off"], pin["kept_off"], pin["kept_off"], pin["keep_row"], own,
                                            labels_raw=pin["labels_raw"], lut=pin["lut"], label_mask=pin["label_mask"],
                                            fill=FILL)
    near_h, tri_h, keep_h = near.cpu().numpy(), tri.cpu().numpy(), pin["keep_row"].cpu().numpy()
    bad = np.nonzero(near_h != tri_h)[0]
    print(f"records whose labels differ: {bad.shape[0]} of {near_h.shape[0]}")
    for r in bad[:5]:
        s_of = int(np.searchsorted(pin["row_off"], r, side="right")) - 1
        row = int(pin["kept_off"][s_of]) + int(keep_h[r])
        print(f"  record {r} scan {s_of}: nearest {near_h[r]} trilinear {tri_h[r]} logits {pl[row].tolist()} "
              f"query {query[row].tolist()}")
    assert np.array_equal(near_h, tri_h)
    assert torch.equal(near_counts, tri_counts) and int(near_counts.sum()) > 0
    want = torch.cat([torch.full((pitems[s]["kept"],), (6 + s) % 7) for s in range(3)])      # where roll put the 3
    assert torch.equal(pl.argmax(dim=1).cpu(), want)
    # an item that cannot supply one query per kept row is refused, not guessed
    for broken in (dict(pitems[0], plain=False), {k: v for k, v in pitems[0].items() if k != "points"},
                   dict(pitems[0], points=pitems[0]["points"][:-1])):
        with pytest.raises(ValueError, match="one query per kept row"):
            evaluate.point_queries([broken])


def test_nearest_is_byte_identical_to_a_run_without_the_flag(runs):
    for f in range(3):
        assert _bytes(_label_file(runs, "nearest", f)) == _bytes(_label_file(runs, "plain", f))
    for suffix in ("", "-points"):
        name = f"SemanticKITTI-TO-SemanticKITTI{suffix}.csv"
        assert _bytes(os.path.join(runs["root"], "nearest", "results", name)) == \
            _bytes(os.path.join(runs["root"], "plain", "results", name))
    a, b = runs["res"]["plain"][0], runs["res"]["nearest"][0]
    assert np.array_equal(a["point_counts"], b["point_counts"]) and np.array_equal(a["counts"], b["counts"])


def test_trilinear_run_end_to_end(runs):
    res = runs["res"]["trilinear"][0]
    model = build_model("MinkUNet34")
    load_lightning_checkpoint(model, runs["ckpts"]["trilinear"])
    model.eval()
    data = scans.FileScans(scans.listing("SemanticKITTI", runs["tree"], "validation"), runs["lut"], keep_raw=True)
    run = evaluate.Predictor(model)
    out_ids = np.asarray(OUT_IDS, dtype=np.uint32)
    class_of = {i: c for c, i in enumerate(OUT_IDS)}
    counts = np.zeros((3, 7, 7), dtype=np.int64)
    differ = 0
    batches = [data.batch(ids, "cuda") for ids in BATCHES]
    for k, (ids, b) in enumerate(zip(BATCHES, batches)):
        nxt = batches[k + 1]["coords_int"] if k + 1 < len(batches) else None
        _, logits = run(b["coords_int"], b["source_features0"], nxt)
        pitems = [data.point_item(i) for i in ids]
        with torch.no_grad():
            pl = evaluate.point_logits(run.output, pitems)
        pred = pl.cpu().max(dim=1)[1].numpy()
        vpred = logits.cpu().max(dim=1)[1].numpy()
        start = vstart = 0
        for i, item in zip(ids, pitems):
            rec = _records(runs, i)
            keep = P.radius_mask_np(rec[:, :3], 50.0)
            path = _label_file(runs, "trilinear", i)
            assert os.path.getsize(path) == 4 * rec.shape[0]         # exactly one uint32 per record, in file order
            got = np.fromfile(path, dtype="<u4")
            want = np.full(rec.shape[0], FILL, dtype=np.uint32)
            want[keep] = out_ids[pred[start:start + item["kept"]]]
            assert np.array_equal(got, want), i
            assert (got[~keep] == FILL).all() and np.isin(got[keep], out_ids).all()
            nearest = out_ids[vpred[vstart + item["inverse_map"].cpu().numpy()]]
            differ += int((nearest != got[keep]).sum())
            raw = np.fromfile(os.path.join(runs["tree"], "sequences", "08", "labels", f"{i:06d}.label"), dtype=np.int32)
            true = runs["lut"][raw & 0xFFFF].astype(np.int64)[keep]
            mine = np.array([class_of[int(v)] for v in got[keep]])
            sel = true != -1                                         # unlabelled records stay left out
            counts[i] = np.bincount(true[sel] * 7 + mine[sel], minlength=49).reshape(7, 7)
            start += item["kept"]
            vstart += item["voxels"]
        assert start == pl.shape[0] and vstart == logits.shape[0]
    print(f"records whose trilinear label differs from the nearest one: {differ}")
    assert np.array_equal(res["point_counts"], counts) and counts.sum() > 0
    assert np.array_equal(res["counts"], runs["res"]["plain"][0]["counts"])      # the voxel level is untouched
    assert res["label_files"] == 3 and res["label_paths"] == [_label_file(runs, "trilinear", f) for f in range(3)]
    rows = evaluate.iou_rows(evaluate.point_iou_counts(counts), "scan")
    assert np.array_equal(res["point_iou_rows"], rows)
    with open(res["points_csv"], newline="") as f:
        table = list(csv.reader(f))
    assert table[0] == ["source", "target"] + list(evaluate.CLASS_NAMES) + ["mean"] and len(table) == 2
    assert _bytes(os.path.join(runs["root"], "trilinear", "results", "SemanticKITTI-TO-SemanticKITTI.csv")) == \
        _bytes(os.path.join(runs["root"], "plain", "results", "SemanticKITTI-TO-SemanticKITTI.csv"))
