"""The G13 fixture of the reference's training augmentation (sub_p / augmentation_list) and a numpy restatement of one
augmented item, which the CPU tests hold against the fixture and the GPU tests hold lidog_amd.data.augment_item against
on full-size scans.

G13 (`make_g13`, build container only: it needs the reference, scipy and the CPU oracle standing in for MinkowskiEngine).
utils/common/augmentation.py imports torchvision, which is absent, and the datasets read files, so the generator reads
the reference's files when it runs, takes RandomRotation, RandomScale, Dataset.random_sample, filter_bounds and
PC2ImgConverter.getBEVImageNew out of them with `ast`, executes them in a namespace of its own and composes them in the
order of __getitem__ (semantickitti_bev.py:209-252 with bounds and BEV labels, synth4d.py:141-166 without,
nuscenes_bev.py:252-261 for BEV labels from the first-point labels) on the oracle's sparse_quantize: the reference's own
code decides the expected values, none of its text is kept.  Recorded per case: the seed, the draws (`sampled_idx`, R,
scales), the next np.random.rand() after the item, and every output.

Exactness: numpy computes `coords @ R` with the machine's BLAS, whose three-term sums differ in the last bits from the
plain (a0 b0 + a1 b1) + a2 b2 chain of the kernel and of `transform_np`.  Integer outputs are compared exactly, which
holds as long as no transformed coordinate sits within rounding of a voxel face or a bounds threshold: `margins` measures
that and generator and tests assert MARGIN on every input; `xyz` is compared within `xyz_bound`."""
import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
G13 = os.path.join(HERE, "golden", "g13_augment.npz")
VOXEL, IGNORE = 0.05, -1
BEV = (50.0, 167)
MARGIN = 1e-9                      # voxels to the nearest voxel face, metres to the nearest bounds threshold
U = 2.0 ** -53
ROT, SCALE = "RandomRotation", "RandomScale"
INT_OUTPUTS = ("coordinates", "index", "inverse_map", "sampled_idx", "sem_labels", "voted_labels", "bev_labels",
               "bev_selected_idx")

# name -> dict(config, scan, dense, sparse, shrink, form ('bev' | 'plain'), augs, sub_p, bev_from, seed)
# an input is `dense` leading rows of the scan (the lowest beams: several points per voxel) and `sparse` rows spread over
# the rest; `shrink` multiplies the points (float32) to push the dense ring into the ego box
def _case(config, scan, form, augs, seed, sub_p=0.8, bev_from="voted", dense=360, sparse=220, shrink=1.0):
    return dict(config=config, scan=scan, form=form, augs=list(augs), seed=seed, sub_p=sub_p, bev_from=bev_from,
                dense=dense, sparse=sparse, shrink=shrink)


CASES = {
    "kitti_bev_rot_scale": _case("kitti120k", 0, "bev", [ROT, SCALE], 7),
    "kitti_bev_rot_scale_s1": _case("kitti120k", 1, "bev", [ROT, SCALE], 11),
    "kitti_bev_rot": _case("kitti120k", 3, "bev", [ROT], 13),
    "kitti_bev_scale": _case("kitti120k", 4, "bev", [SCALE], 14),
    "kitti_bev_scale_rot": _case("kitti120k", 5, "bev", [SCALE, ROT], 15),
    "kitti_bev_empty_list": _case("kitti120k", 6, "bev", [], 16),
    "kitti_bev_all_rows": _case("kitti120k", 7, "bev", [ROT, SCALE], 17, sub_p=None),
    "kitti_bev_first_labels": _case("kitti120k", 8, "bev", [ROT, SCALE], 18, bev_from="first"),
    "kitti_bev_ego_box": _case("kitti120k", 9, "bev", [ROT, SCALE], 19, shrink=0.6),
    "kitti_bev_none_kept": _case("kitti120k", 10, "bev", [ROT, SCALE], 20, sparse=0, dense=400, shrink=0.3),
    "kitti_plain_rot_scale": _case("kitti120k", 0, "plain", [ROT, SCALE], 21),
    "kitti_plain_scale": _case("kitti120k", 1, "plain", [SCALE], 22),
    "kitti_plain_empty_list": _case("kitti120k", 2, "plain", [], 23),
    "nusc_bev_rot_scale": _case("nusc35k", 0, "bev", [ROT, SCALE], 24),
    "nusc_bev_first_labels": _case("nusc35k", 1, "bev", [ROT, SCALE], 25, bev_from="first"),
    "nusc_bev_scale_rot": _case("nusc35k", 2, "bev", [SCALE, ROT], 26),
    "nusc_bev_ego_box": _case("nusc35k", 3, "bev", [ROT], 27, shrink=0.6),
    "nusc_plain_rot_scale": _case("nusc35k", 0, "plain", [ROT, SCALE], 28),
    "nusc_plain_all_rows": _case("nusc35k", 2, "plain", [SCALE, ROT], 30, sub_p=None),
    "nusc_plain_scale_s1": _case("nusc35k", 3, "plain", [SCALE], 31),
}


# ------------------------------------------------------------------ inputs
def make_points(config, scan, dense=None, sparse=None, shrink=1.0, label_noise=0.15):
    """(points float32 [n,3], features float32 [n,1] = the row number, labels int64 [n]) of synthetic scan `scan`;
    dense / sparse None: the whole scan (without the few rows that have a coordinate within 1e-6 of 0).  `label_noise`
    of the labels are redrawn from -1..6, so that voxels of several points disagree and the vote has work to do."""
    sys.path.insert(0, REPO)
    from lidog_amd import synth
    pts, labels = synth.scan_points_labels(scan, config)
    off_face = (np.abs(pts) > 1e-6).all(axis=1)      # the beams at azimuth 0 and pi have y = 0 or 1e-15: on the face y = 0 under every scale
    pts, labels = pts[off_face], labels[off_face]
    if dense is not None:
        rest = np.arange(dense, pts.shape[0])
        rows = np.concatenate([np.arange(dense), rest[::max(len(rest) // max(sparse, 1), 1)][:sparse]])
        pts, labels = pts[rows], labels[rows]
    rng = np.random.default_rng([int(scan), 13])
    noisy = rng.random(pts.shape[0]) < label_noise
    labels = np.where(noisy, rng.integers(-1, 7, pts.shape[0]), labels).astype(np.int64)
    pts = np.ascontiguousarray(pts * np.float32(shrink), dtype=np.float32)
    return pts, np.arange(pts.shape[0], dtype=np.float32).reshape(-1, 1), labels


def case_input(case):
    return make_points(case["config"], case["scan"], case["dense"], case["sparse"], case["shrink"])


# ------------------------------------------------------------------ one item restated in numpy
def transform_np(points, ops):
    """(transformed points, per element Sum_k |p_k| |R_kj| times the scales applied after the rotation, or None while
    float32): the rotation as the plain float64 chain, the scale through numpy's own dtype rules"""
    p = np.array(points, dtype=np.float32)
    mag = None
    for name, par in ops:
        par = np.asarray(par, dtype=np.float64)
        if name == ROT:
            x = p.astype(np.float64)
            R = par.reshape(3, 3)
            p = np.stack([(x[:, 0] * R[0, j] + x[:, 1] * R[1, j]) + x[:, 2] * R[2, j] for j in range(3)], axis=1)
            mag = np.abs(x) @ np.abs(R)
        else:
            p = p.copy()
            for k in range(3):
                p[:, k] = p[:, k] * par[k:k + 1]
            if mag is not None:
                mag = mag * np.abs(par)[None, :]
    return p, mag


def xyz_bound(mag):
    """both sides round a three-term float64 dot product (3 u each, relative to Sum |p_k R_kj|) and one product"""
    return 8 * U * mag


def in_bounds_np(p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    keep = (-60 < x) & (x < 60) & (-60 < y) & (y < 60) & (-10 < z) & (z < 8)
    return keep & ~((-3 < x) & (x < 3) & (-2 < y) & (y < 2))


def margins(p, voxel=VOXEL, bounds=False):
    """(voxels to the nearest voxel face, metres to the nearest bounds threshold or inf) over all coordinates of p"""
    if p.shape[0] == 0:
        return np.inf, np.inf
    t = p.astype(np.float64) / np.float64(np.asarray(voxel, dtype=p.dtype))
    face = float(np.abs(t - np.round(t)).min())
    thr = np.inf
    if bounds:
        x, y, z = (p[:, k].astype(np.float64) for k in range(3))
        thr = float(min(np.abs(np.abs(x) - 60).min(), np.abs(np.abs(y) - 60).min(), np.abs(z + 10).min(),
                        np.abs(z - 8).min(), np.abs(np.abs(x) - 3).min(), np.abs(np.abs(y) - 2).min()))
    return face, thr


def quantize_np(p, labels, voxel=VOXEL, ignore_label=IGNORE):
    """ME.utils.sparse_quantize: (coords int32 [m,3], voted labels, index of the first point of every voxel in point
    order, inverse map); a voxel whose points disagree votes ignore_label"""
    c = np.floor(p / np.asarray(voxel, dtype=p.dtype)).astype(np.int32)
    if c.shape[0] == 0:
        e = np.zeros(0, np.int64)
        return c.reshape(0, 3), labels[:0], e, e
    _, first, inv = np.unique(c, axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    index, inverse = first[order].astype(np.int64), rank[inv].astype(np.int64)
    voted = labels[index].copy()
    voted[np.unique(inverse[labels != labels[index][inverse]])] = ignore_label
    return c[index], voted, index, inverse


def bev_np(coords, labels, bound, img_size, voxel=VOXEL, z_range=(-10.0, 8.0)):
    """getBEVImageNew on `(coords * voxel).astype(float32)`: the last valid point of a pixel wins"""
    grid = (bound - (-bound)) / img_size
    S = int((bound - (-bound)) / grid)
    img = -np.ones((S, S), np.int32)
    idx = -np.ones((S, S), np.int32)
    v = (coords * voxel).astype(np.float32)
    lo, hi = np.float32(-bound), np.float32(bound)
    ok = (labels != -1) & (lo < v[:, 0]) & (v[:, 0] < hi) & (lo < v[:, 1]) & (v[:, 1] < hi)
    ok &= (np.float32(z_range[0]) < v[:, 2]) & (v[:, 2] < np.float32(z_range[1]))
    rows = np.nonzero(ok)[0]
    px = np.floor((v[rows, 0] - (-bound)) / grid).astype(np.int64)
    py = np.floor(S - (v[rows, 1] - (-bound)) / grid).astype(np.int64) - 1
    img[py, px] = labels[rows]
    idx[py, px] = rows
    return img, idx


def augment_np(points, features, labels, draws, voxel=VOXEL, bounds=False, ignore_label=IGNORE, bev=None,
               bev_from="voted"):
    """the item of lidog_amd.data.augment_item in numpy, plus `_margins` (face, threshold) and `_xyz_bound`"""
    sampled = np.asarray(draws["sampled_idx"], dtype=np.int64)
    p, mag = transform_np(points[sampled], draws["ops"])
    lab = labels[sampled]
    face, thr = margins(p, voxel, bounds)
    if bounds:
        keep = in_bounds_np(p)
        p, lab, sampled = p[keep], lab[keep], sampled[keep]
        mag = mag[keep] if mag is not None else None
    coords, voted, index, inverse = quantize_np(p, lab, voxel, ignore_label)
    out = {"coordinates": coords, "xyz": p[index], "features": features[sampled[index]], "sem_labels": lab[index],
           "sampled_idx": sampled[index], "inverse_map": inverse, "index": index, "voted_labels": voted,
           "_margins": (face, thr), "_xyz_bound": xyz_bound(mag[index]) if mag is not None else None}
    if bev is not None:
        img, idx = bev_np(coords, voted if bev_from == "voted" else lab[index], bev[0], bev[1], voxel)
        out["bev_labels"], out["bev_selected_idx"] = img.astype(np.int64), idx.astype(np.int64)
    return out


def compare(got, want, bound, what=""):
    """every integer output exactly, features exactly, xyz within `bound` (None: exactly, same dtype)"""
    for k in INT_OUTPUTS:
        if k in want:
            assert k in got, f"{what}: no '{k}'"
            g, w = np.asarray(got[k]), np.asarray(want[k])
            assert g.shape == w.shape, f"{what} {k}: shape {g.shape} against {w.shape}"
            assert np.array_equal(g.astype(np.int64), w.astype(np.int64)), f"{what}: {k} differs"
    assert np.array_equal(np.asarray(got["features"]), np.asarray(want["features"])), f"{what}: features differ"
    g, w = np.asarray(got["xyz"]), np.asarray(want["xyz"])
    assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: xyz {g.dtype}{g.shape} against {w.dtype}{w.shape}"
    if bound is None:
        assert np.array_equal(g, w), f"{what}: float32 xyz differs"
    else:
        excess = np.abs(g - w) - bound
        assert excess.size == 0 or excess.max() <= 0, f"{what}: xyz off by {np.abs(g - w).max()} (bound {bound.max()})"


# ------------------------------------------------------------------ the fixture
def load_g13():
    """(meta dict, {array name: array})"""
    z = np.load(G13, allow_pickle=False)
    return json.loads(str(z["meta_json"])), {k: z[k] for k in z.files if k != "meta_json"}


def case_draws(name, arrays):
    """the recorded draws of a case in draw_augmentation's layout"""
    ops, r, s = [], 0, 0
    for a in CASES[name]["augs"]:
        if a == ROT:
            ops.append((a, arrays[f"{name}__R"].reshape(-1, 3, 3)[r]))
            r += 1
        else:
            ops.append((a, arrays[f"{name}__scale"].reshape(-1, 3)[s]))
            s += 1
    return {"sampled_idx": arrays[f"{name}__draw_idx"].astype(np.int64), "ops": ops}


def case_outputs(name, arrays):
    pre = name + "__out_"
    return {k[len(pre):]: v for k, v in arrays.items() if k.startswith(pre)}


# ------------------------------------------------------------------ generator (needs the reference and scipy)
def _lift(path, wanted):
    """{name: ast node} of the top-level classes / functions, or `Class.method` entries, named in `wanted`"""
    with open(path) as f:
        tree = ast.parse(f.read())
    found = {}
    for node in tree.body:
        if isinstance(node, (ast.ClassDef, ast.FunctionDef)) and node.name in wanted:
            found[node.name] = node
        if isinstance(node, ast.ClassDef):
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef) and f"{node.name}.{sub.name}" in wanted:
                    found[f"{node.name}.{sub.name}"] = sub
    assert set(found) == set(wanted), sorted(set(wanted) - set(found))
    return found


def _reference_functions(ref):
    from scipy.linalg import expm, norm
    if not hasattr(np, "int"):
        np.int = int                          # semantickitti_bev.py still uses the removed alias
    aug = _lift(os.path.join(ref, "utils/common/augmentation.py"), ("RandomRotation", "RandomScale"))
    ds = _lift(os.path.join(ref, "utils/datasets/dataset.py"), ("BaseDataset.random_sample",))
    kb = _lift(os.path.join(ref, "utils/datasets/semantickitti_bev.py"),
               ("SemanticKITTIBEVDataset.filter_bounds", "PC2ImgConverter.__init__", "PC2ImgConverter.getBEVImageNew"))
    holder = ast.ClassDef(name="Lifted", bases=[], keywords=[], decorator_list=[],
                          body=[ds["BaseDataset.random_sample"], kb["SemanticKITTIBEVDataset.filter_bounds"]])
    conv = ast.ClassDef(name="Converter", bases=[], keywords=[], decorator_list=[],
                        body=[kb["PC2ImgConverter.__init__"], kb["PC2ImgConverter.getBEVImageNew"]])
    mod = ast.Module(body=[aug["RandomRotation"], aug["RandomScale"], holder, conv], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"np": np, "expm": expm, "norm": norm}
    exec(compile(mod, "reference", "exec"), ns)
    return ns


def make_g13(ref):
    sys.path.insert(0, REPO)
    import oracle.me_cpu as OME
    from lidog_amd import data as D
    ns = _reference_functions(ref)
    meta, arrays = {"voxel": VOXEL, "ignore": IGNORE, "bev": list(BEV), "cases": {}}, {}
    for name, case in CASES.items():
        pts, feats, labels = case_input(case)
        ds = ns["Lifted"]()
        ds.sub_p = case["sub_p"]
        ds.grid_bounds = [[-60, 60], [-60, 60], [-10, 8]]
        transforms = [ns[a]() if a == ROT else ns[a](0.9, 1.1) for a in case["augs"]]
        recorded = {"R": [], "scale": []}
        np.random.seed(case["seed"])
        # ---- __getitem__ of the training datasets, phase 'train', augmentations not None
        sampled_idx = ds.random_sample(pts)
        draw_idx = sampled_idx.copy()
        points, colors, sem = pts[sampled_idx], feats[sampled_idx], labels[sampled_idx]
        for t in transforms:                  # ComposeBEV.__call__: t(img, None, is_bev=True)
            points, tr = t(points, None, is_bev=True)
            recorded["R" if isinstance(t, ns[ROT]) else "scale"].append(np.asarray(tr, dtype=np.float64).reshape(-1))
        transformed = points
        if case["form"] == "bev":
            keep = ds.filter_bounds(points)
            points, sem, colors, sampled_idx = points[keep], sem[keep], colors[keep], sampled_idx[keep]
        rec = {k: case[k] for k in case}
        try:
            q, _, voted, voxel_idx, inverse = OME.utils.sparse_quantize(
                points, colors, labels=sem, ignore_label=IGNORE, quantization_size=VOXEL, return_index=True,
                return_inverse=True)
            out = {"coordinates": q, "xyz": points[voxel_idx], "features": colors[voxel_idx], "sem_labels": sem[voxel_idx],
                   "sampled_idx": sampled_idx[voxel_idx], "inverse_map": inverse, "index": voxel_idx,
                   "voted_labels": voted}
            if case["form"] == "bev":
                grid = (BEV[0] - (-BEV[0])) / BEV[1]
                conv = ns["Converter"](imgChannel=1, xRange=[-BEV[0], BEV[0]], yRange=[-BEV[0], BEV[0]], zRange=[-10, 8],
                                       xGridSize=grid, yGridSize=grid, zGridSize=0.3)
                bev_points = (q * VOXEL).astype(np.float32)
                img, idx = conv.getBEVImageNew(bev_points, voted if case["bev_from"] == "voted" else out["sem_labels"])
                out["bev_labels"], out["bev_selected_idx"] = img, idx
            rec["outcome"] = "ok"
        except Exception as e:               # recorded, as G11 / G12 record their raising cases
            out, rec["outcome"], rec["error"] = {}, "raises", f"{type(e).__name__}: {e}"
        rec["next_rand"] = float(np.random.rand())
        # ---- the draws replay through draw_augmentation, and the restatement agrees under the fixture's rules
        np.random.seed(case["seed"])
        draws = D.draw_augmentation(np.random, pts.shape[0], case["sub_p"], case["augs"])
        assert np.array_equal(draws["sampled_idx"], draw_idx) and float(np.random.rand()) == rec["next_rand"], name
        for (a, par), want in zip(draws["ops"], [recorded["R" if a == ROT else "scale"].pop(0) for a in case["augs"]]):
            assert np.array_equal(np.asarray(par).reshape(-1), want), (name, a)
        assert pts.shape[0] < 1 << 15
        arrays[f"{name}__draw_idx"] = draw_idx.astype(np.int16)
        if [p for a, p in draws["ops"] if a == ROT]:
            arrays[f"{name}__R"] = np.stack([p for a, p in draws["ops"] if a == ROT])
        if [p for a, p in draws["ops"] if a == SCALE]:
            arrays[f"{name}__scale"] = np.stack([p for a, p in draws["ops"] if a == SCALE])
        face, thr = margins(transformed, VOXEL, case["form"] == "bev")
        assert face > MARGIN and thr > MARGIN, f"{name}: margins {face} / {thr}: replace this input"
        rec.update(rows_in=int(pts.shape[0]), sampled=int(len(draw_idx)), kept=int(points.shape[0]),
                   face_margin=face, threshold_margin=None if np.isinf(thr) else thr, xyz_dtype=str(points.dtype))
        if rec["outcome"] == "ok":
            rec["voxels"] = int(out["coordinates"].shape[0])
            rec["voted_ignore"] = int((out["voted_labels"] == IGNORE).sum() - (out["sem_labels"] == IGNORE).sum())
            mine = augment_np(pts, feats, labels, draws, VOXEL, case["form"] == "bev", IGNORE,
                              BEV if case["form"] == "bev" else None, case["bev_from"])
            compare(mine, out, mine["_xyz_bound"], name)
            small = {"coordinates": np.int16, "index": np.int16, "inverse_map": np.int16, "sampled_idx": np.int16,
                     "sem_labels": np.int8, "voted_labels": np.int8, "bev_labels": np.int8, "bev_selected_idx": np.int16,
                     "features": np.float32}
            for k, v in out.items():
                v = np.asarray(v)
                if k in small:
                    assert np.array_equal(v.astype(small[k]).astype(v.dtype), v), (name, k)
                    v = v.astype(small[k])
                arrays[f"{name}__out_{k}"] = v
        meta["cases"][name] = rec
        print(name, rec["outcome"], rec.get("error", ""), "rows", rec["rows_in"], rec["sampled"], rec["kept"],
              rec.get("voxels"), "vote->ignore", rec.get("voted_ignore"), "margins %.2e %s" % (face, thr))
    np.savez_compressed(G13, meta_json=np.array(json.dumps(meta)), **arrays)
    print(G13, os.path.getsize(G13), "bytes")
