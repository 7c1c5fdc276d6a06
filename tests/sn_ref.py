"""The G12 fixture of the reference's SN car-size scaling baseline: sklearn's DBSCAN labels as get_average_dims
(train_scaling_based.py:35-87) obtains them, the statistics get_average_dims / get_scaling_params (:90-129) return, and
the items of SingleSNSourceDataset.__getitem__ / MultiSNSourceDataset.merge_data (utils/datasets/sn_scaling.py); plus
the inputs both the generator and the tests build, and a numpy restatement of DBSCAN for small inputs.

G12 (`make_g12`, build container only: it needs the reference, sklearn and the CPU oracle standing in for
MinkowskiEngine).  train_scaling_based.py cannot be imported (it imports pytorch_lightning at the top), so the generator
reads that file when it runs, takes the two function definitions get_average_dims and get_scaling_params out of it with
`ast` and executes them in a namespace holding np, torch, os and a recording subclass of sklearn's DBSCAN: the
reference's own code decides the expected values, none of its text is kept.  Recorded:
  lattice   random lattice point sets whose neighbour counts straddle min_samples, sklearn's labels, and per case
            whether the integer predicate d^2 <= (eps / voxel)^2 would label it differently (`flag`)
  edge      n < min_samples, one full cell, noise points, a border point between two clusters
  stats     per statistics case: the drawn scans, per clustered scan sklearn's labels of its car voxels and the integer
            boxes and counts of its clusters, the kept [width, height, length] rows, the float32 result (or: raises)
  scaling   get_scaling_params for 1 x 1, 1 x 2 and 2 x 2 (sources x targets)
  items     scaled items with identifying features, the captured np.random.choice draws and the first-point index"""
import ast
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
G12 = os.path.join(HERE, "golden", "g12_sn.npz")
VOXEL, EPS, MIN_SAMPLES = 0.05, 0.5, 10
N_SCANS = 20                      # scans of every stub dataset: 4 are drawn

# name -> (configuration, first scan seed, dataset name)
DATASETS = {
    "kitti": ("kitti120k_cars", 0, "SemanticKITTIDataset"),
    "kitti_b": ("kitti120k_cars", 1000, "SemanticPOSSDataset"),
    "kitti_c": ("kitti120k_cars", 2000, "SynLiDARDataset"),
    "nusc": ("nusc35k_cars", 0, "NuScenesDataset"),
    "nusc_b": ("nusc35k_cars", 1000, "NuScenesDataset"),
    "nusc_other_name": ("nusc35k_cars", 0, "Synth4DDataset"),     # 5000 / 1000 apply: no cluster qualifies, it raises
}
STATS = (("kitti", 3), ("kitti", 12), ("kitti_b", 5), ("nusc", 4), ("nusc", 32), ("nusc_b", 5), ("nusc_other_name", 0))
SCALING = ((("kitti",), ("nusc",), 3), (("kitti",), ("nusc", "kitti_b"), 4), (("kitti", "kitti_c"), ("nusc", "kitti_b"), 5))
OUTPUTS = (("coordinates", np.int32), ("features", np.float32), ("sem_labels", np.int64), ("index", np.int64))


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


class StubDataset:
    """what get_average_dims and the two SN datasets read from a source dataset, over synthetic scans"""

    def __init__(self, key, n=N_SCANS):
        self.config, self.first, self.name = DATASETS[key]
        self.n, self.voxel_size, self.ignore_label, self.class2names = n, VOXEL, -1, None
        self.served = []

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        import torch
        sys.path.insert(0, REPO)
        from lidog_amd import synth
        vox, labels = synth.scan_voxels(self.first + int(i), self.config)
        self.served.append(int(i))
        return {"coordinates": torch.from_numpy(vox), "sem_labels": torch.from_numpy(labels)}


def car_voxels(key, i):
    """int32 [n, 3]: the car voxels (class 0) of scan i of dataset `key`, in scan order"""
    sys.path.insert(0, REPO)
    from lidog_amd import synth
    config, first, _ = DATASETS[key]
    vox, labels = synth.scan_voxels(first + int(i), config)
    return np.ascontiguousarray(vox[labels == 0], dtype=np.int32)


def make_item_scan(config, scan_seed, tag, limit=None):
    """one scan with features that identify the row and the scan (row number + 10^6 * tag), as mix_ref.make_scan"""
    sys.path.insert(0, REPO)
    from lidog_amd import synth
    vox, labels = synth.scan_voxels(scan_seed, config)
    if limit is not None:
        vox, labels = vox[:limit], labels[:limit]
    n = vox.shape[0]
    row = np.arange(n, dtype=np.float32)
    return {"coordinates": vox.astype(np.int32), "features": (row + np.float32(tag * 1_000_000)).reshape(-1, 1),
            "sem_labels": labels.astype(np.int64),
            "xyz": np.stack([row, np.full(n, tag, np.float32), row * np.float32(-0.5)], axis=1),
            "sampled_idx": np.arange(n, dtype=np.int64) + tag * 10_000_000, "idx": np.int64(scan_seed)}


# scaled items: (kind, [(configuration, scan seed, limit)], seed of the draws); the scale rows come from SCALING
ITEMS = (("single", [("kitti120k_cars", 2, None)], 0), ("single", [("nusc35k_cars", 4, None)], 0),
         ("single", [("kitti120k_cars", 3, 4000)], 0), ("single", [("nusc35k_cars", 5, 4000)], 0),
         ("multi", [("kitti120k_cars", 4, None), ("kitti120k_cars", 2005, None)], 1),
         ("multi", [("kitti120k_cars", 5, 3000), ("kitti120k_cars", 2006, 3000)], 2),
         ("multi", [("kitti120k_cars", 6, 3000), ("kitti120k_cars", 2007, 3000)], 3))


# ------------------------------------------------------------------ DBSCAN restated (small inputs: all pairs)
def neighbour_matrix(coords, voxel=VOXEL, eps=EPS, integer=False):
    """[n, n] bool.  sklearn's predicate: on x = float32(c) * float32(voxel), sum_k (double(x_i) - double(x_j))^2 <=
    eps^2 in float64, summed in axis order; `integer`: d^2 <= (eps / voxel)^2 on the lattice instead"""
    c = np.asarray(coords)
    if integer:
        d = c[:, None, :].astype(np.int64) - c[None, :, :].astype(np.int64)
        return (d * d).sum(-1) <= int(round((eps / voxel) ** 2))
    x = (c.astype(np.float32) * np.float32(voxel)).astype(np.float64)
    d = x[:, None, :] - x[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= eps * eps


def dbscan_np(coords, voxel=VOXEL, eps=EPS, min_samples=MIN_SAMPLES, integer=False):
    """labels of DBSCAN as a function of the neighbour graph: core = at least min_samples neighbours (itself included);
    clusters = components of the core graph, numbered by their smallest core row; a border row takes the smallest
    cluster number among its core neighbours; -1 otherwise"""
    n = len(coords)
    if n == 0:
        return np.zeros(0, np.int64)
    nb = neighbour_matrix(coords, voxel, eps, integer)
    core = nb.sum(1) >= min_samples
    labels = np.full(n, -1, np.int64)
    k = 0
    for i in range(n):
        if not core[i] or labels[i] >= 0:
            continue
        stack = [i]
        labels[i] = k
        while stack:
            a = stack.pop()
            for b in np.nonzero(nb[a] & core & (labels < 0))[0]:
                labels[b] = k
                stack.append(b)
        k += 1
    big = np.iinfo(np.int64).max
    for i in np.nonzero(~core)[0]:
        m = np.where(nb[i] & core, labels, big).min()
        labels[i] = -1 if m == big else m
    return labels


def boxes_np(coords, labels):
    """(counts int64 [k], lo, hi int32 [k, 3]) of the clusters 0..k-1"""
    k = int(labels.max()) + 1 if len(labels) else 0
    counts = np.array([(labels == c).sum() for c in range(k)], dtype=np.int64)
    lo = np.array([coords[labels == c].min(0) for c in range(k)], dtype=np.int32).reshape(k, 3)
    hi = np.array([coords[labels == c].max(0) for c in range(k)], dtype=np.int32).reshape(k, 3)
    return counts, lo, hi


# ------------------------------------------------------------------ inputs of the label cases
def lattice_case(seed):
    """~165 distinct lattice points in a 40^3-voxel box at a random offset: ~10.8 neighbours within 10 voxels each"""
    rng = np.random.default_rng([int(seed), 12])
    n = int(rng.integers(150, 181))
    cells = rng.choice(40 ** 3, n, replace=False)
    pts = np.stack([cells // 1600, (cells // 40) % 40, cells % 40], axis=1)
    return (pts + rng.integers(-1200, 1200, 3)).astype(np.int32)


def edge_cases():
    rng = np.random.default_rng(12)
    out = {}
    out["n9"] = np.stack([np.arange(9), np.zeros(9, int), np.zeros(9, int)], axis=1)       # fewer than min_samples
    cells = rng.choice(1000, 200, replace=False)                                             # 200 points in one cell
    out["one_cell"] = np.stack([cells // 100, (cells // 10) % 10, cells % 10], axis=1) + np.array([-400, 30, 7])
    blob = np.stack(np.meshgrid(np.arange(5), np.arange(3), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    far = np.array([[40, 40, 40], [-60, 3, 9], [41, 40, 40], [0, -80, 0], [25, 0, 0]])
    out["noise"] = np.concatenate([far[:2], blob, far[2:], blob + np.array([0, 100, 0])])
    # a sparse point with four neighbours in each of two dense blobs: the first cluster (number 0) claims it
    a, b = blob + np.array([-14, 0, 0]), blob + np.array([8, 0, 0])
    out["border_two_clusters"] = np.concatenate([np.array([[-1, 5, 0]]), a, b])
    return {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in out.items()}


def load_g12():
    """(meta dict, {array name: array})"""
    z = np.load(G12, allow_pickle=False)
    return json.loads(str(z["meta_json"])), {k: z[k] for k in z.files if k != "meta_json"}


def lattice_cases(arrays):
    """[(coords int32, labels int64, flag)] of the recorded lattice cases"""
    st = arrays["lat_start"]
    return [(arrays["lat_coords"][st[i]:st[i + 1]].astype(np.int32), arrays["lat_labels"][st[i]:st[i + 1]].astype(np.int64),
             bool(arrays["lat_flag"][i])) for i in range(len(st) - 1)]


# ------------------------------------------------------------------ generator (needs the reference and sklearn)
def _reference_functions(ref, dbscan_cls):
    import torch
    with open(os.path.join(ref, "train_scaling_based.py")) as f:
        tree = ast.parse(f.read())
    wanted = ("get_average_dims", "get_scaling_params")
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    assert [n.name for n in body] == list(wanted)
    ns = {"np": np, "torch": torch, "os": os, "DBSCAN": dbscan_cls}
    exec(compile(ast.Module(body=body, type_ignores=[]), "train_scaling_based.py", "exec"), ns)
    return ns["get_average_dims"], ns["get_scaling_params"]


def make_g12(ref):
    import importlib.util

    import torch
    from sklearn.cluster import DBSCAN
    sys.path.insert(0, REPO)
    import oracle.me_cpu as OME
    from lidog_amd import data as D

    calls = []

    class Recording(DBSCAN):
        def fit_predict(self, X, y=None, **kw):
            labels = super().fit_predict(X, y, **kw)
            calls.append((np.asarray(X), labels))
            return labels

    get_average_dims, get_scaling_params = _reference_functions(ref, Recording)
    meta, arrays = {"voxel": VOXEL, "eps": EPS, "min_samples": MIN_SAMPLES, "n_scans": N_SCANS}, {}

    def sk(coords):
        x = torch.from_numpy(np.asarray(coords, dtype=np.int32)) * VOXEL
        return DBSCAN(eps=EPS, min_samples=MIN_SAMPLES).fit_predict(x)

    # ---- lattice cases: the first 14 flagged and the first 30 unflagged of 300
    picked, n_flag, n_plain = [], 0, 0
    for seed in range(300):
        c = lattice_case(seed)
        want = sk(c)
        assert np.array_equal(dbscan_np(c), want), f"lattice {seed}: the restatement differs from sklearn"
        flag = not np.array_equal(dbscan_np(c, integer=True), want)
        if (flag and n_flag < 14) or (not flag and n_plain < 30):
            picked.append((seed, c, want, flag))
            n_flag, n_plain = n_flag + flag, n_plain + (not flag)
    start = np.concatenate([[0], np.cumsum([len(c) for _, c, _, _ in picked])])
    arrays.update(lat_coords=np.concatenate([c for _, c, _, _ in picked]).astype(np.int16), lat_start=start.astype(np.int32),
                  lat_labels=np.concatenate([l for _, _, l, _ in picked]).astype(np.int16),
                  lat_flag=np.array([f for _, _, _, f in picked], dtype=np.uint8))
    meta["lattice_seeds"] = [s for s, _, _, _ in picked]
    print("lattice:", len(picked), "cases,", n_flag, "flagged")

    # ---- edge cases
    meta["edge"] = []
    for name, c in edge_cases().items():
        want = sk(c)
        assert np.array_equal(dbscan_np(c), want), name
        arrays[f"edge_{name}_labels"] = want.astype(np.int16)
        meta["edge"].append(name)
        print("edge", name, len(c), "labels", sorted(set(want.tolist())))
    lab = arrays["edge_border_two_clusters_labels"]
    assert lab[0] == 0 and set(lab[1:31].tolist()) == {0} and set(lab[31:].tolist()) == {1}
    nb = neighbour_matrix(edge_cases()["border_two_clusters"])
    assert nb[0, 1:31].any() and nb[0, 31:].any() and nb[0].sum() < MIN_SAMPLES

    # ---- statistics
    meta["stats"] = []
    for k, (key, seed) in enumerate(STATS):
        ds = StubDataset(key)
        calls.clear()
        np.random.seed(seed)
        rec = {"dataset": key, "seed": seed}
        try:
            result = get_average_dims(ds)
            rec["outcome"] = "ok"
        except ValueError as e:
            result, rec["outcome"], rec["error"] = None, "raises", str(e)
        np.random.seed(seed)
        drawn = D.draw_scans(np.random, len(ds))
        assert ds.served == drawn.tolist()
        rec["drawn"] = drawn.tolist()
        min_pts, min_car_pts = D.sn_thresholds(ds.name)
        rec["scans"], rows, j = [], [], 0
        for i in drawn:
            car = car_voxels(key, i)
            if len(car) <= min_pts:
                rec["scans"].append({"scan": int(i), "car_voxels": int(len(car)), "clustered": False})
                continue
            X, labels = calls[j]
            assert np.array_equal(X, (torch.from_numpy(car) * VOXEL).numpy())
            counts, lo, hi = boxes_np(car, labels)
            kept = D.box_dims(counts, lo, hi, VOXEL, min_car_pts)
            arrays.update({f"s{k}_{j}_labels": labels.astype(np.int16), f"s{k}_{j}_counts": counts, f"s{k}_{j}_lo": lo,
                           f"s{k}_{j}_hi": hi})
            rec["scans"].append({"scan": int(i), "car_voxels": int(len(car)), "clustered": True, "slot": j,
                                 "clusters": int(len(counts)), "noise": int((labels == -1).sum()),
                                 "too_small": int((counts <= min_car_pts).sum()),
                                 "wrong_shape": int((counts > min_car_pts).sum()) - len(kept), "kept": len(kept),
                                 "labels_sha1": digest(labels.astype(np.int16))})
            rows += kept
            j += 1
        assert j == len(calls)
        arrays[f"s{k}_rows"] = np.concatenate(rows, axis=0) if rows else np.zeros((0, 3), np.float32)
        if result is not None:      # the integer boxes reproduce the reference's float32 result bit for bit
            assert result.dtype == np.float32 and np.array_equal(D.mean_dims(rows), result)
            arrays[f"s{k}_result"] = result
        else:
            assert not rows
        meta["stats"].append(rec)
        print("stats", key, seed, rec["outcome"], None if result is None else result.tolist(),
              [(s["scan"], s["car_voxels"], s.get("kept"), s.get("too_small"), s.get("wrong_shape"), s.get("noise"))
               for s in rec["scans"]])

    # ---- scale factors (the reference caches the dimensions by dataset name under the working directory)
    meta["scaling"] = []
    cwd = os.getcwd()
    for k, (src, tgt, seed) in enumerate(SCALING):
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            try:
                np.random.seed(seed)
                out = get_scaling_params([StubDataset(s) for s in src], [StubDataset(t) for t in tgt])
            finally:
                os.chdir(cwd)
        assert len(out) == len(src) and all(a.dtype == np.float32 and a.shape == (len(tgt), 3) for a in out)
        arrays[f"p{k}_scaling"] = np.stack(out)
        meta["scaling"].append({"sources": list(src), "targets": list(tgt), "seed": seed})
        print("scaling", src, tgt, np.stack(out).tolist())

    # ---- scaled items
    saved = sys.modules.get("MinkowskiEngine")
    sys.modules["MinkowskiEngine"] = OME
    try:
        spec = importlib.util.spec_from_file_location("ref_sn_scaling", os.path.join(ref, "utils/datasets/sn_scaling.py"))
        sn = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sn)
        meta["items"] = _items(sn, OME, arrays)
    finally:
        if saved is None:
            sys.modules.pop("MinkowskiEngine", None)
        else:
            sys.modules["MinkowskiEngine"] = saved

    np.savez_compressed(G12, meta_json=np.array(json.dumps(meta)), **arrays)
    print(G12, os.path.getsize(G12), "bytes")


def item_scaling(arrays, kind, which):
    """the scaling list of an item case: single -> the 1 x 1 factors (kitti -> nusc, > 1) or their inverse (< 1: voxels
    merge); multi -> the 2 x 2 factors"""
    if kind == "multi":
        return [a for a in arrays["p2_scaling"]]
    s = arrays["p0_scaling"]
    return [s[0]] if which == 0 else [(np.float32(1) / s[0]).astype(np.float32)]


def _items(sn, OME, arrays):
    import torch

    def torch_scan(s):
        d = {k: torch.from_numpy(np.asarray(v)) for k, v in s.items() if k != "idx"}
        d["idx"] = torch.tensor(int(s["idx"]))
        d["inverse_map"] = torch.arange(s["coordinates"].shape[0])
        return d

    class OneScan:
        ignore_label, class2names, voxel_size = -1, None, VOXEL

        def __init__(self, scan):
            self.scan = scan

        def __len__(self):
            return 1

        def __getitem__(self, i):
            return torch_scan(self.scan)

    out = []
    for k, (kind, scans, seed) in enumerate(ITEMS):
        data = [make_item_scan(c, s, tag, limit) for tag, (c, s, limit) in enumerate(scans)]
        which = 0 if scans[0][0].startswith("kitti") else 1
        scaling = item_scaling(arrays, kind, which)
        draws, quantized = [], []
        own_choice, own_quantize = np.random.choice, OME.utils.sparse_quantize

        def choice(*a, **kw):
            r = own_choice(*a, **kw)
            draws.append(int(r))
            return r

        def quantize(*a, **kw):
            r = own_quantize(*a, **kw)
            quantized.append(r)
            return r

        if kind == "single":
            ds = sn.SingleSNSourceDataset(OneScan(data[0]), scaling)
        else:
            ds = sn.MultiSNSourceDataset([OneScan(d) for d in data], scaling)     # its constructor shuffles: before the seed
        np.random.seed(seed)
        np.random.choice, OME.utils.sparse_quantize = choice, quantize
        try:
            if kind == "single":
                got = [ds[0]]
            else:
                m = ds.merge_data(torch_scan(data[0]), torch_scan(data[1]))
                got = [{"coordinates": m[f"source_coordinates{s}"], "features": m[f"source_features{s}"],
                        "sem_labels": m[f"source_sem_labels{s}"]} for s in (0, 1)]
        finally:
            np.random.choice, OME.utils.sparse_quantize = own_choice, own_quantize
        rec = {"kind": kind, "scans": [list(s) for s in scans], "seed": seed, "which": which, "draws": draws, "parts": []}
        for s, g in enumerate(got):
            o = {name: g[name].numpy() for name in ("coordinates", "features", "sem_labels")}
            o["index"] = np.asarray(quantized[s][-1])
            o = {name: o[name].astype(dt) for name, dt in OUTPUTS}
            n_in = data[s]["coordinates"].shape[0]
            full = scans[s][2] is not None
            if full:
                arrays.update({f"i{k}_{s}_{name}": a for name, a in o.items()})
            rec["parts"].append({"rows_in": int(n_in), "rows": int(o["coordinates"].shape[0]), "full": full,
                                 "digests": {name: digest(a) for name, a in o.items()}})
        out.append(rec)
        print("item", kind, scans, draws, [(p["rows_in"], p["rows"]) for p in rec["parts"]])
    return out
