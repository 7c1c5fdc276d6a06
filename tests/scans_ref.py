"""The G15 fixture of the reference's file datasets (SemanticKITTI, nuScenes, Synth4D), the tiny file trees it is made
over, and a numpy restatement of the first mile of a scan, which the CPU tests hold against the fixture and the GPU tests
hold lidog_amd.scans against at sizes the fixture does not cover.

Trees (`write_trees`): written from seeds, the same bytes wherever they are written, so the GPU tests write them again
where the reference is absent.  Per file ~900 points of a synthetic `source8k` scan in shuffled order, 80 points beyond
50 m (a `source8k` scan ends at 49.93 m: without them the radius mask keeps everything) and 64 points on the shell
r = 50 (1 +- 3e-7), where the float32 rounding of the squared radius decides.  Raw label ids are drawn per class through
the inverse of the label map; SemanticKITTI labels carry random instance ids in the upper 16 bits; the Synth4D files are
float64 / int64 arrays of 3, 4 or 6 columns, one has no label file and one holds negative ids inside [-L, 0).

G15 (`make_g15`, build container only: it needs the reference, PyYAML, tqdm and the CPU oracle standing in for
MinkowskiEngine).  The reference's dataset modules are imported as they are, with stub modules for what is absent
(MinkowskiEngine -> the CPU oracle, torchvision.transforms, the nuScenes devkit -> an index over the tree's pair list),
so its own __init__ (listing, LUT construction), load_label_kitti / load_label_nusc, the cached `data` dict of
__getitem__, the validation-phase item and get_dataset_stats decide the expected values; none of its text is kept."""
import json
import os
import pickle
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
G15 = os.path.join(GOLDEN, "g15_scans.npz")
VOXEL, IGNORE, IN_RADIUS = 0.05, -1, 50.0
MAPS = {"SemanticKITTI": "semantickitti2common.yaml", "nuScenes": "nuscenes2common.yaml",
        "Synth4D": "synth4d2common.yaml"}
DATASETS = ("SemanticKITTI", "nuScenes", "Synth4D-kitti", "Synth4D-nuscenes")
PHASES = ("train", "validation")
NEAR, DENSE, FAR, SHELL = 900, 360, 80, 64


def map_of(dataset):
    return "Synth4D" if dataset.startswith("Synth4D") else dataset


# ------------------------------------------------------------------ the trees
# SemanticKITTI: frames per sequence of the `mini` split
KITTI_FRAMES = {"00": 2, "01": 1, "08": 2}
NUSC_FILES = {"train": ["n015-a", "n008-b"], "validation": ["n015-c"]}
NUSC_SCENES = {"train": {"scene-0002": ["n015-a"], "scene-0001": ["n008-b"]}, "validation": {"scene-0003": ["n015-c"]}}
# Synth4D: {folder: {phase: {town: ids in the pickle's order}}}; towns and ids deliberately unsorted
SYNTH4D = {
    "kitti_synth": {"train": {"Town06": [10, 9], "Town03": [12, 3]}, "validation": {"Town03": [20], "Town06": [21]}},
    "nuscenes_synth": {"train": {"Town03": [5, 1]}, "validation": {"Town03": [2]}},
}
SYNTH4D_COLUMNS = {"kitti_synth": 4, "nuscenes_synth": 3}
SYNTH4D_WIDE = ("kitti_synth", "Town03", 12)          # this file has 6 columns
SYNTH4D_NO_LABELS = ("kitti_synth", "Town06", 21)     # this file has no label file
SYNTH4D_NEGATIVE = ("nuscenes_synth", "Town03", 1)    # this file holds negative ids inside [-L, 0)
FOLDER_OF = {"Synth4D-kitti": "kitti_synth", "Synth4D-nuscenes": "nuscenes_synth"}


def make_scan(seed, shell=True, whole=False):
    """(points float32 [n,3], classes int64 [n] in -1..6) from a seed: NEAR rows of synthetic scan `seed` (source8k,
    its DENSE leading rows among them), FAR rows at 50.5-70 m and SHELL rows at r = 50 (1 +- 3e-7), shuffled"""
    sys.path.insert(0, REPO)
    from lidog_amd import synth
    pts, labels = synth.scan_points_labels(int(seed), "source8k")
    rng = np.random.default_rng([int(seed), 15])
    # the leading rows are the lowest beams, several points per voxel: the voxel vote and the inverse map have work to do
    if not whole:       # whole: every row of the scan (the end-to-end tests' source8k-sized frames)
        rows = np.concatenate([np.arange(DENSE), DENSE + rng.choice(pts.shape[0] - DENSE, NEAR - DENSE, replace=False)])
        pts, labels = pts[rows], labels[rows]

    def sphere(n, r):
        d = rng.normal(size=(n, 3))
        d[:, 2] *= 0.1
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return (d * np.asarray(r)[:, None]).astype(np.float32)

    parts, labs = [pts, sphere(FAR, rng.uniform(50.5, 70.0, FAR))], [labels, rng.integers(-1, 7, FAR)]
    if shell:
        parts.append(sphere(SHELL, 50.0 * (1.0 + rng.uniform(-3e-7, 3e-7, SHELL))))
        labs.append(rng.integers(-1, 7, SHELL))
    pts, labels = np.concatenate(parts), np.concatenate(labs)
    order = rng.permutation(pts.shape[0])
    return np.ascontiguousarray(pts[order], dtype=np.float32), labels[order].astype(np.int64), rng


def raw_ids(rng, classes, keys, vals):
    """a raw id per point whose mapped class is the point's class, drawn among the map's keys of that class"""
    out = np.zeros(classes.shape[0], dtype=np.int64)
    for c in np.unique(classes):
        pool = keys[vals == c]
        assert pool.size, f"no raw id maps to class {c}"
        sel = classes == c
        out[sel] = pool[rng.integers(0, pool.size, int(sel.sum()))]
    return out


def _seed(*parts):
    return 1000 + sum((i + 1) * 131 * int(p) for i, p in enumerate(parts))


def write_kitti_tree(root, maps, frames=None, whole=False):
    """a SemanticKITTI tree under `root`: frames = {sequence: number of frames}"""
    keys, vals = maps["SemanticKITTI"]
    for seq, n in (KITTI_FRAMES if frames is None else frames).items():
        for d in ("velodyne", "labels"):
            os.makedirs(os.path.join(root, "sequences", seq, d), exist_ok=True)
        for f in range(n):
            pts, cls, rng = make_scan(_seed(1, int(seq), f), whole=whole)
            rec = np.concatenate([pts, rng.random((pts.shape[0], 1), dtype=np.float32)], axis=1)
            raw = raw_ids(rng, cls, keys, vals).astype(np.uint32) | (rng.integers(0, 1 << 16, cls.shape[0]).astype(np.uint32) << 16)
            rec.astype(np.float32).tofile(os.path.join(root, "sequences", seq, "velodyne", f"{f:06d}.bin"))
            raw.view(np.int32).tofile(os.path.join(root, "sequences", seq, "labels", f"{f:06d}.label"))
    return root


def write_label_map_json(path, maps, name):
    """the label map `name` as a JSON file lidog_amd.scans.load_label_map reads (no PyYAML needed)"""
    keys, vals = maps[name]
    with open(path, "w") as f:
        json.dump({"learning_map": {str(int(k)): int(v) for k, v in zip(keys, vals)}}, f)
    return path


def write_trees(root, maps):
    """writes the three trees and the split pickles under `root`; maps: {map name: (keys, values)}.
    Returns {'SemanticKITTI': path, 'nuScenes': path, 'Synth4D': path, 'splits': path}."""
    out = {"SemanticKITTI": os.path.join(root, "kitti"), "nuScenes": os.path.join(root, "nusc"),
           "Synth4D": os.path.join(root, "synth4d"), "splits": os.path.join(root, "splits")}
    write_kitti_tree(out["SemanticKITTI"], maps)
    keys, vals = maps["nuScenes"]
    os.makedirs(os.path.join(out["nuScenes"], "samples", "LIDAR_TOP"), exist_ok=True)
    os.makedirs(os.path.join(out["nuScenes"], "lidarseg", "v1.0-trainval"), exist_ok=True)
    for phase, names in NUSC_FILES.items():
        lines = []
        for k, name in enumerate(names):
            pts, cls, rng = make_scan(_seed(2, PHASES.index(phase), k))
            rec = np.concatenate([pts, rng.random((pts.shape[0], 1), dtype=np.float32) * 255,
                                  rng.integers(0, 32, (pts.shape[0], 1)).astype(np.float32)], axis=1)
            p, l = f"samples/LIDAR_TOP/{name}.pcd.bin", f"lidarseg/v1.0-trainval/{name}_lidarseg.bin"
            rec.astype(np.float32).tofile(os.path.join(out["nuScenes"], p))
            raw_ids(rng, cls, keys, vals).astype(np.uint8).tofile(os.path.join(out["nuScenes"], l))
            lines.append(f"{p} {l}\n")
        with open(os.path.join(out["nuScenes"], "train.txt" if phase == "train" else "val.txt"), "w") as f:
            f.writelines(lines)
    keys, vals = maps["Synth4D"]
    L = int(keys.max()) + 100
    for folder, phases in SYNTH4D.items():
        os.makedirs(os.path.join(out["splits"], folder), exist_ok=True)
        for phase, towns in phases.items():
            split = {t: (list(ids) if phase == "train" else np.asarray(ids, dtype=np.int64)) for t, ids in towns.items()}
            with open(os.path.join(out["splits"], folder,
                                   "training_split.pkl" if phase == "train" else "validation_split.pkl"), "wb") as f:
                pickle.dump(split, f)
            for town, ids in towns.items():
                for d in ("velodyne", "labels"):
                    os.makedirs(os.path.join(out["Synth4D"], folder, town, d), exist_ok=True)
                for i in ids:
                    pts, cls, rng = make_scan(_seed(3, len(folder), int(town[4:6]), i), shell=False)
                    cols = 6 if (folder, town, i) == SYNTH4D_WIDE else SYNTH4D_COLUMNS[folder]
                    arr = np.concatenate([pts.astype(np.float64), rng.random((pts.shape[0], cols - 3))], axis=1)
                    np.save(os.path.join(out["Synth4D"], folder, town, "velodyne", f"{i}.npy"), arr)
                    if (folder, town, i) == SYNTH4D_NO_LABELS:
                        continue
                    raw = raw_ids(rng, cls, keys, vals)
                    if (folder, town, i) == SYNTH4D_NEGATIVE:
                        wrap = rng.random(raw.shape[0]) < 0.2
                        raw = np.where(wrap, raw - L, raw)          # lut[raw - L] is lut[raw]
                        raw[:3] = (-1, -L, -100)                     # the table's last, first and an unset entry
                    np.save(os.path.join(out["Synth4D"], folder, town, "labels", f"{i}.npy"), raw.reshape(-1, 1))
    return out


def tree_root(trees, dataset):
    return trees[map_of(dataset)]


# ------------------------------------------------------------------ the first mile restated in numpy
def load_scan_np(points_raw, labels_raw, lut, stride, mask=None, in_radius=None):
    """(points float32 [m,3], labels int32 [m], mapped labels of ALL rows int32 [n]) as the reference's __getitem__
    makes its cached `data` dict: numpy's own indexing (an id outside the table raises IndexError) and numpy's own
    float32 `np.sum(np.square(points), axis=1) < in_R ** 2`"""
    pcd = np.ascontiguousarray(points_raw).reshape(-1).view(np.float32).reshape((-1, stride))
    if labels_raw is None:
        mapped = np.zeros(pcd.shape[0], dtype=np.int32)
    else:
        idx = np.asarray(labels_raw).reshape(-1)
        if mask is not None:
            idx = idx & mask
        mapped = np.asarray(lut)[idx].astype(np.int32)
    points, labels = pcd[:, :3], mapped
    if in_radius is not None:
        keep = np.sum(np.square(points), axis=1) < in_radius ** 2
        points, labels = points[keep], labels[keep]
    return np.ascontiguousarray(points), labels, mapped


def counts_np(mapped, num_classes, ignore_label=IGNORE):
    """get_dataset_stats' contribution of one label file"""
    w = np.zeros(num_classes)
    lbl, count = np.unique(mapped, return_counts=True)
    keep = (lbl != ignore_label) & (lbl >= 0) & (lbl < num_classes)
    w[lbl[keep]] += count[keep]
    return w


def item_np(points, labels, voxel=VOXEL, ignore_label=IGNORE):
    """the validation-phase item: every point, voxelised; features are ones, labels those of the first point"""
    import augment_ref
    coords, _, index, inverse = augment_ref.quantize_np(points, labels, voxel, ignore_label)
    return {"coordinates": coords, "features": np.ones((index.shape[0], 1), np.float32), "sem_labels": labels[index],
            "inverse_map": inverse, "index": index}


def read_np(dataset, points_path, labels_path):
    """(points_raw, labels_raw or None, stride, mask, in_radius) of a file pair, read as the reference reads it"""
    if dataset == "SemanticKITTI":
        return (np.fromfile(points_path, dtype=np.float32), np.fromfile(labels_path, dtype=np.int32), 4, 0xFFFF,
                IN_RADIUS)
    if dataset == "nuScenes":
        return np.fromfile(points_path, dtype=np.float32), np.fromfile(labels_path, np.uint8), 5, None, IN_RADIUS
    pts = np.load(points_path).astype(np.float32)
    labels = np.load(labels_path).astype(np.int32).reshape([-1]) if os.path.exists(labels_path) else None
    return pts, labels, pts.shape[1], None, None


# ------------------------------------------------------------------ the fixture
def load_g15():
    """(meta dict, {array name: array})"""
    z = np.load(G15, allow_pickle=False)
    return json.loads(str(z["meta_json"])), {k: z[k] for k in z.files if k != "meta_json"}


def fixture_maps(arrays):
    return {m: (arrays[f"mapkeys_{m}"].astype(np.int64), arrays[f"mapvals_{m}"].astype(np.int64)) for m in MAPS}


def case_name(dataset, phase, i):
    return f"{dataset}_{phase}_{i}"


def case_outputs(name, arrays, prefix):
    pre = f"{name}__{prefix}_"
    return {k[len(pre):]: v for k, v in arrays.items() if k.startswith(pre)}


# ------------------------------------------------------------------ generator (needs the reference)
class _Index:
    """what NuScenesDataset.__init__ asks of the devkit, over NUSC_SCENES"""

    def __init__(self, dataroot):
        self.dataroot = dataroot
        self.tables = {"scene": {}, "sample": {}, "sample_data": {}, "lidarseg": {}}
        self.scene = []
        for scenes in NUSC_SCENES.values():
            for scene, names in scenes.items():
                rec = {"name": scene, "token": "tok-" + scene, "first_sample_token": f"{scene}/0"}
                self.scene.append(rec)
                self.tables["scene"][rec["token"]] = rec
                for k, name in enumerate(names):
                    tok = f"{scene}/{k}"
                    self.tables["sample"][tok] = {"data": {"LIDAR_TOP": "sd-" + tok},
                                                  "next": f"{scene}/{k + 1}" if k + 1 < len(names) else ""}
                    self.tables["sample_data"]["sd-" + tok] = {"filename": f"samples/LIDAR_TOP/{name}.pcd.bin"}
                    self.tables["lidarseg"]["sd-" + tok] = {"filename": f"lidarseg/v1.0-trainval/{name}_lidarseg.bin"}

    def get(self, table, token):
        return self.tables[table][token]


def _reference_datasets(ref):
    sys.path.insert(0, REPO)
    import oracle.me_cpu as OME
    sys.modules["MinkowskiEngine"] = OME
    tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tvt.Compose = type("Compose", (), {})
    tv.transforms = tvt
    nus, nus_u, nus_s = (types.ModuleType(n) for n in ("nuscenes", "nuscenes.utils", "nuscenes.utils.splits"))
    nus.NuScenes = _Index
    nus_s.create_splits_scenes = lambda: {"train": list(NUSC_SCENES["train"]), "val": list(NUSC_SCENES["validation"]),
                                          "mini_train": [], "mini_val": []}
    nus.utils, nus_u.splits = nus_u, nus_s
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "nuscenes": nus, "nuscenes.utils": nus_u,
                        "nuscenes.utils.splits": nus_s})
    sys.path.insert(0, ref)
    import utils.datasets.nuscenes as N
    import utils.datasets.semantickitti as K
    import utils.datasets.synth4d as S
    return K.SemanticKITTIDataset, N.NuScenesDataset, S.Synth4DDataset


def _reference_dataset(classes, dataset, phase, trees):
    K, N, S = classes
    kw = dict(phase=phase, mapping_path=os.path.join(GOLDEN, MAPS[map_of(dataset)]), voxel_size=VOXEL,
              ignore_label=IGNORE, use_cache=True, in_radius=IN_RADIUS)
    if dataset == "SemanticKITTI":
        return K(version="mini", dataset_path=trees["SemanticKITTI"] + os.sep, **kw)
    if dataset == "nuScenes":
        return N(nusc=_Index(trees["nuScenes"]), version="v1.0-trainval", dataset_path=trees["nuScenes"], **kw)
    folder = FOLDER_OF[dataset]
    split = os.path.join(trees["splits"], folder, "training_split.pkl" if phase == "train" else "validation_split.pkl")
    return S(version="full", dataset_path=trees["Synth4D"], split_path=split,
             sensor="hdl64e" if folder == "kitti_synth" else "hdl32e", **kw)


def make_g15(ref):
    import tempfile

    import yaml
    classes = _reference_datasets(ref)
    meta = {"voxel": VOXEL, "ignore": IGNORE, "in_radius": IN_RADIUS, "listings": {}, "cases": {}, "stats": {}}
    arrays, maps = {}, {}
    for m, f in MAPS.items():
        lm = yaml.safe_load(open(os.path.join(GOLDEN, f)))["learning_map"]
        maps[m] = (np.array(list(lm.keys()), dtype=np.int64), np.array(list(lm.values()), dtype=np.int64))
        arrays[f"mapkeys_{m}"], arrays[f"mapvals_{m}"] = maps[m][0].astype(np.int16), maps[m][1].astype(np.int8)
    with tempfile.TemporaryDirectory() as root:
        trees = write_trees(root, maps)
        for dataset in DATASETS:
            for phase in PHASES:
                ds = _reference_dataset(classes, dataset, phase, trees)
                lut = np.asarray(ds.learning_map)
                key = f"lut_{map_of(dataset)}"
                assert key not in arrays or np.array_equal(arrays[key], lut)
                arrays[key] = lut.astype(np.int32)
                if dataset.startswith("Synth4D"):
                    pairs = [(p, os.path.join(os.path.dirname(p), "../labels", os.path.basename(p))) for p in ds.path_list]
                else:
                    pairs = list(zip(ds.pcd_path, ds.label_path))
                base = tree_root(trees, dataset)
                meta["listings"][f"{dataset}_{phase}"] = [[os.path.relpath(os.path.normpath(p), base),
                                                          os.path.relpath(os.path.normpath(l), base)] for p, l in pairs]
                try:
                    stats = ds.get_dataset_stats()
                    arrays[f"{dataset}_{phase}__stats"] = np.asarray(stats, dtype=np.float64)
                    meta["stats"][f"{dataset}_{phase}"] = "ok"
                except FileNotFoundError as e:
                    meta["stats"][f"{dataset}_{phase}"] = "raises FileNotFoundError"
                for i, (p, l) in enumerate(pairs):
                    name = case_name(dataset, phase, i)
                    item = ds[i]
                    data = ds.CACHE[i]
                    pts = np.asarray(data["points"])
                    lab = np.asarray(data["sem_labels" if "sem_labels" in data else "labels"])
                    assert pts.dtype == np.float32 and lab.dtype == np.int32, (name, pts.dtype, lab.dtype)
                    out = {"coordinates": item["coordinates"], "features": item["features"],
                           "sem_labels": item["sem_labels"], "inverse_map": item["inverse_map"],
                           "index": item["sampled_idx"]}
                    out = {k: np.asarray(v) for k, v in out.items()}
                    # ---- the restatement agrees with the reference on its own files
                    raw_p, raw_l, stride, mask, radius = read_np(dataset, p, l)
                    mine_p, mine_l, mapped = load_scan_np(raw_p, raw_l, lut, stride, mask, radius)
                    assert np.array_equal(mine_p.view(np.uint32), pts.view(np.uint32)) and np.array_equal(mine_l, lab), name
                    mine = item_np(mine_p, mine_l)
                    for k in out:
                        assert np.array_equal(np.asarray(mine[k]).astype(np.int64), out[k].astype(np.int64)), (name, k)
                    n = raw_p.size // stride
                    meta["cases"][name] = {"dataset": dataset, "phase": phase, "index": i, "rows": int(n),
                                           "kept": int(pts.shape[0]), "voxels": int(out["coordinates"].shape[0]),
                                           "labels_file": os.path.exists(l)}
                    arrays[f"{name}__data_points"] = np.ascontiguousarray(pts)
                    arrays[f"{name}__data_labels"] = lab.astype(np.int8)
                    small = {"coordinates": np.int16, "features": np.float32, "sem_labels": np.int8,
                             "inverse_map": np.int16, "index": np.int16}
                    for k, v in out.items():
                        assert np.array_equal(v.astype(small[k]).astype(v.dtype), v), (name, k)
                        arrays[f"{name}__item_{k}"] = v.astype(small[k])
                    print(name, "rows", n, "kept", pts.shape[0], "voxels", out["coordinates"].shape[0])
    np.savez_compressed(G15, meta_json=np.array(json.dumps(meta)), **arrays)
    print(G15, os.path.getsize(G15), "bytes")
