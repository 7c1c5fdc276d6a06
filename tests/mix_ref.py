"""The G11 fixture of the reference's scan mixing: PointCutMixSourceDataset.merge_data (utils/datasets/pointcutmix.py:43-135)
and CoSMixSourceDataset.merge_data (utils/datasets/cosmix.py:50-171), and the scans both the generator and the tests build.

G11 (`make_g11`, build container only: it imports the reference) runs the reference's own merge_data, with the CPU
oracle (oracle/me_cpu) standing in for MinkowskiEngine, on stub datasets over synthetic scan pairs, after
`np.random.seed(seed)`.  The reference's random draws are captured by wrapping np.random.choice during the run, the
first point of every merged voxel by wrapping the oracle's sparse_quantize.  Per case it records the draws, the counts
the draws were made from (cells of the drawn source's 10 m quantisation, or its class counts), and the merged scan:
full arrays for a few small cases, sha1 digests and lengths otherwise.  A case whose draw raises (fewer than 4
qualifying cells) is recorded as raising.  Features, xyz and sampled_idx identify the row and the scan, so a wrong
gather cannot pass."""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
G11 = os.path.join(HERE, "golden", "g11_mix.npz")
NUM_CLASSES = 7
SOURCE1 = 1 << 20          # lidog_amd.synth.SOURCE1_SEED: scan seeds of the second source
OUTPUTS = (("coordinates", np.int32), ("features", np.float32), ("sem_labels", np.int64), ("xyz", np.float32),
           ("sampled_idx", np.int64), ("index", np.int64))


def _case(method, pair, seeds, sub_p=0.8, one_class=False, limit=None, full=False):
    return [dict(method=method, config0=pair[0], scan0=pair[1], config1=pair[2], scan1=pair[3], seed=s, sub_p=sub_p,
                 one_class=one_class, limit=limit, full=full and i == 0) for i, s in enumerate(seeds)]


KITTI = ("kitti120k", 0, "kitti120k", SOURCE1)
NUSC = ("nusc35k", 1, "nusc35k", SOURCE1 + 1)
SMALL = ("source8k", 2, "source8k", SOURCE1 + 2)
CROSS = ("kitti120k", 3, "nusc35k", SOURCE1 + 3)
CASES = (_case("pointcutmix", KITTI, (0, 1, 2)) + _case("pointcutmix", NUSC, (0, 1)) +
         _case("pointcutmix", SMALL, (0, 1), full=True) + _case("pointcutmix", CROSS, (3,)) +
         # fewer than 4 cells of more than 300 rows in either scan: the draw raises whichever scan is drawn
         _case("pointcutmix", SMALL, (0, 1), limit=1000) +
         _case("cosmix", KITTI, (0, 1, 2)) + _case("cosmix", NUSC, (0, 1)) + _case("cosmix", SMALL, (0, 1)) +
         _case("cosmix", SMALL, (3, 4), sub_p=None, full=True) + _case("cosmix", CROSS, (3,)) +
         # one labelled class in either scan: int(1 / 2) = 0 classes drawn, the merge is the target re-quantised
         _case("cosmix", SMALL, (5, 6), one_class=True, full=True))


def make_scan(config, scan_seed, tag, one_class=False, limit=None):
    """numpy arrays of one scan of the pair (tag 0 / 1): the synthetic voxels and labels of lidog_amd.synth, features /
    xyz / sampled_idx that identify the row and the scan"""
    sys.path.insert(0, REPO)
    from lidog_amd import synth
    vox, labels = synth.scan_voxels(scan_seed, config)
    if limit is not None:
        vox, labels = vox[:limit], labels[:limit]
    if one_class:
        labels = np.where(labels >= 0, 3, -1)
    n = vox.shape[0]
    row = np.arange(n, dtype=np.float32)
    return {"coordinates": vox.astype(np.int32),
            "features": (row + np.float32(tag * 1_000_000)).reshape(-1, 1),
            "sem_labels": labels.astype(np.int64),
            "xyz": np.stack([row, np.full(n, tag, np.float32), row * np.float32(-0.5)], axis=1),
            "sampled_idx": np.arange(n, dtype=np.int64) + tag * 10_000_000,
            "idx": np.int64(scan_seed)}


def class_weights(scan):
    """per-class weights of a case's source: its own label counts plus a ramp, so that no two classes weigh the same"""
    lab = scan["sem_labels"]
    return (np.bincount(lab[lab >= 0], minlength=NUM_CLASSES) + 1000.0 * np.arange(1, NUM_CLASSES + 1)).astype(np.float64)


def case_scans(c):
    s0 = make_scan(c["config0"], c["scan0"], 0, c["one_class"], c["limit"])
    s1 = make_scan(c["config1"], c["scan1"], 1, c["one_class"], c["limit"])
    return s0, s1


def voxel_size(c):
    from lidog_amd import synth
    return synth.CONFIGS[c["config0"]]["voxel"]      # the reference's self.voxel_size = source_dataset0.voxel_size


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_g11():
    """[(case dict with the recorded fields, {array name: array})]"""
    z = np.load(G11, allow_pickle=False)
    meta = json.loads(str(z["cases_json"]))
    out = []
    for k, c in enumerate(meta):
        arrays = {name[len(f"c{k}_"):]: z[name] for name in z.files if name.startswith(f"c{k}_")}
        out.append((c, arrays))
    return out


# ------------------------------------------------------------------ generator (needs the reference)
def _load_reference(ref, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _StubDataset:
    """what the two mixing datasets read from their source datasets"""

    def __init__(self, voxel, weights, sub_p):
        self.ignore_label, self.class2names, self.voxel_size = -1, None, voxel
        self.sem_weights, self.sub_p, self.augmentations = weights, sub_p, None

    def __len__(self):
        return 1


def _torch_scan(s):
    import torch
    d = {k: torch.from_numpy(np.asarray(v)) for k, v in s.items() if k != "idx"}
    d["idx"] = torch.tensor(int(s["idx"]))
    d["inverse_map"] = torch.arange(s["coordinates"].shape[0])
    return d


def make_g11(ref):
    sys.path.insert(0, REPO)
    import oracle.me_cpu as OME
    saved = sys.modules.get("MinkowskiEngine")
    sys.modules["MinkowskiEngine"] = OME
    try:
        pcm = _load_reference(ref, "utils/datasets/pointcutmix.py", "ref_pointcutmix")
        cos = _load_reference(ref, "utils/datasets/cosmix.py", "ref_cosmix")
        meta, arrays = [], {}
        for k, c in enumerate(CASES):
            rec, arr = _run_case(pcm, cos, OME, c)
            meta.append(rec)
            arrays.update({f"c{k}_{name}": a for name, a in arr.items()})
            print(k, c["method"], c["config0"], c["seed"], rec["outcome"], rec.get("rows"))
    finally:
        if saved is None:
            sys.modules.pop("MinkowskiEngine", None)
        else:
            sys.modules["MinkowskiEngine"] = saved
    np.savez_compressed(G11, cases_json=np.array(json.dumps(meta)), **arrays)
    print(G11, os.path.getsize(G11), "bytes")


def _run_case(pcm, cos, OME, c):
    s0, s1 = case_scans(c)
    voxel = voxel_size(c)
    w = (class_weights(s0), class_weights(s1))
    stubs = [_StubDataset(voxel, w[0], c["sub_p"]), _StubDataset(voxel, w[1], c["sub_p"])]
    cls = pcm.PointCutMixSourceDataset if c["method"] == "pointcutmix" else cos.CosMixSourceDataset
    ds = cls(stubs)                                   # its constructor shuffles: before the seed below
    draws, quantized = [], []
    own_choice, own_quantize = np.random.choice, OME.utils.sparse_quantize

    def choice(*a, **kw):
        r = own_choice(*a, **kw)
        draws.append(np.asarray(r))
        return r

    def quantize(*a, **kw):
        r = own_quantize(*a, **kw)
        quantized.append(r)
        return r

    np.random.seed(c["seed"])
    np.random.choice, OME.utils.sparse_quantize = choice, quantize
    merged, raised = None, None
    try:
        merged = ds.merge_data(_torch_scan(s0), _torch_scan(s1))
    except ValueError as e:
        raised = str(e)
    finally:
        np.random.choice, OME.utils.sparse_quantize = own_choice, own_quantize
    sel = int(draws[0])
    src = (s0, s1)[sel]
    if c["method"] == "pointcutmix":
        inverse = np.asarray(quantized[0][-1])        # the source's 10 m quantisation, return_inverse
        counts = np.bincount(inverse)
    else:
        lab = src["sem_labels"]
        counts = np.bincount(lab[lab >= 0], minlength=NUM_CLASSES)
    rec = dict(c, outcome="raises" if raised is not None else "ok", source=sel,
               choice=[int(x) for x in draws[1]] if len(draws) > 1 else None,
               subs=[[int(len(d)), digest(d.astype(np.int64))] for d in draws[2:]])
    arr = {"counts": counts.astype(np.int64), "w0": w[0], "w1": w[1]}
    if raised is not None:
        rec["error"] = raised
        return rec, arr
    out = {k: merged[k].numpy() for k in ("coordinates", "features", "sem_labels", "xyz", "sampled_idx")}
    out["index"] = np.asarray(quantized[-1][-1])     # the first point of every merged voxel (return_index)
    out = {k: out[k].astype(dt) for k, dt in OUTPUTS}
    rec["rows"] = int(out["coordinates"].shape[0])
    rec["digests"] = {k: digest(a) for k, a in out.items()}
    rec["idx"] = merged["idx"].numpy().tolist()
    if c["full"]:
        arr.update(out)
    return rec, arr
