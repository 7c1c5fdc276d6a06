"""Scans read from files: SemanticKITTI, Synth4D and nuScenes (a pair list), for training and evaluation.

What the reference's datasets do between the file and the voxelised item (utils/datasets/semantickitti.py, nuscenes.py,
synth4d.py and their *_bev.py training forms), with the per-point work on the GPU:

  load_label_map, label_lut   the `learning_map` of a *2common.yaml file as the int32 look-up table (semantickitti.py:58-63)
  load_scan                   the file's bytes, uploaded unmodified -> the cached `data` dict of __getitem__: records
                              unpacked, labels masked and mapped, radius mask, kept rows compacted in order, optional
                              per-class label statistics (csrc/scanload.hip, lidog_scan_load).  One device -> host read
                              per scan: the four words of `info`.
  label_counts                get_dataset_stats on a label file alone (semantickitti.py:199-213)
  keep_rows                   the row every record of a file has in load_scan's output, -1 where the radius mask dropped
                              it (csrc/pointlabels.hip, lidog_scan_keep_rows): the way back from a voxel to the file's
                              points, for lidog_amd.evaluate.point_labels
  semantickitti_files, synth4d_files, pair_list_files, listing     the file listings, in the reference's order
  FileScans                   a dataset over one or two listings: validation form (every kept point, voxelised) and
                              training form (sub_p / augmentations, bounds filter and BEV labels), items through
                              lidog_amd.data.augment_item, batches with the keys of synth.make_batch

FakeKITTI / FakeSynth4D-kitti / FakeSynth4D-nuscenes are the Raycast baseline's pre-generated datasets (fake_kitti.py,
fake_synth4d.py): SemanticKITTI-layout records, written by `python -m lidog_amd.raycast`.  FileScans(raycast=) resamples
the scans of any training listing on the fly instead (lidog_amd.raycast).

The library ships no label map of its own: the user passes the reference's *2common.yaml (or the same as JSON).
"""
import json
import os
import pickle

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr
from .data import (NUSCENES_NAME, augment_item, check_augmentations, collate_items, draw_augmentation, merge_stream,
                   on_merge_stream)

NAMES = ("SemanticKITTI", "Synth4D-kitti", "Synth4D-nuscenes", "nuScenes", "FakeKITTI", "FakeSynth4D-kitti",
         "FakeSynth4D-nuscenes")
# per dataset: how a file is laid out and what the reference's dataset does with it.  `stride`: floats per point record
# (None: whatever the .npy array holds); `labels`: the label file's dtype; `mask`: AND-mask on the raw label (the
# instance id sits in SemanticKITTI's upper 16 bits); `radius`: the reference masks SemanticKITTI (semantickitti.py:110)
# and nuScenes (nuscenes.py:157-160) and never Synth4D (synth4d.py:106-137); `bev_from`: which labels the training
# form's BEV image is made of (semantickitti_bev.py:249 the voted ones, nuscenes_bev.py:261 the first point's)
FORMATS = {
    "SemanticKITTI": dict(stride=4, labels=np.int32, mask=0xFFFF, radius=True, bev_from="voted"),
    "nuScenes": dict(stride=5, labels=np.uint8, mask=None, radius=True, bev_from="first"),
    "Synth4D-kitti": dict(stride=None, labels=np.int32, mask=None, radius=False, bev_from="voted", folder="kitti_synth"),
    "Synth4D-nuscenes": dict(stride=None, labels=np.int32, mask=None, radius=False, bev_from="voted",
                             folder="nuscenes_synth"),
    # the Raycast baseline's pre-generated data (lidog_amd.raycast writes it): plain SemanticKITTI-layout records.
    # FakeKITTI masks by radius (fake_kitti.py:110), FakeSynth4D never does; the hdl32e form of fake_synth4d.py reads
    # its labels as int8 (:119), raw ids up to 127, read here as uint8.  `fake`: <town>/velodyne/<id:06d>.bin directly
    # under the root, labels in <town>/labels/<id:06d>.label (fake_synth4d.py:79-83)
    "FakeKITTI": dict(stride=4, labels=np.int32, mask=0xFFFF, radius=True, bev_from="voted"),
    "FakeSynth4D-kitti": dict(stride=4, labels=np.int32, mask=None, radius=False, bev_from="voted",
                              folder="kitti_synth", fake=True),
    "FakeSynth4D-nuscenes": dict(stride=4, labels=np.uint8, mask=None, radius=False, bev_from="voted",
                                 folder="nuscenes_synth", fake=True),
}
SEMANTICKITTI_SPLITS = {      # semantickitti.py:42-50, semantickitti_bev.py:73-79
    "full": {"train": ["00", "01", "02", "03", "04", "05", "06", "07", "09", "10"], "validation": ["08"]},
    "mini": {"train": ["00", "01"], "validation": ["08"]},
}
PHASES = ("train", "validation")
_LABEL_KINDS = {torch.int32: 1, torch.uint8: 2}


# ------------------------------------------------------------------ label maps
def load_label_map(path):
    """the `learning_map` of a label-map file ({raw id: class}): a .json file, or a .yaml file read through PyYAML"""
    if path.lower().endswith(".json"):
        with open(path) as f:
            maps = json.load(f)
    else:
        try:
            import yaml
        except ImportError as e:
            raise ImportError(f"{path}: reading a YAML label map needs PyYAML; convert the file to JSON instead") from e
        with open(path) as f:
            maps = yaml.safe_load(f)
    if not isinstance(maps, dict) or "learning_map" not in maps:
        raise ValueError(f"{path}: no 'learning_map' entry")
    return {int(k): int(v) for k, v in maps["learning_map"].items()}


def label_lut(learning_map):
    """semantickitti.py:58-63: int32 -ones(max_key + 100) with the map written in"""
    max_key = max(learning_map.keys())
    lut = -np.ones((max_key + 100), dtype=np.int32)
    lut[list(learning_map.keys())] = list(learning_map.values())
    return lut


# ------------------------------------------------------------------ the first mile, on the device
def _as_words(t, what, name):
    """a device tensor of raw bytes (uint8) or of float32 as flat float32"""
    _lib.require_gpu(t, what)
    t = t.contiguous().reshape(-1)
    if t.dtype == torch.uint8:
        if t.shape[0] % 4:
            raise ValueError(f"{name}: {t.shape[0]} bytes of points are no whole number of float32")
        return t.view(torch.float32)
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: {what} must be float32 or raw bytes, not {t.dtype}")
    return t


def _launch(points, labels_raw, lut, stride, label_mask, in_radius, counts, n, dev):
    """lidog_scan_load on the current stream -> (points_out, labels_out, info), nothing read back"""
    kind = 0
    if labels_raw is not None:
        kind = _LABEL_KINDS[labels_raw.dtype]
        _lib.require_gpu(lut, "the look-up table")
        if lut.dtype != torch.int32 or lut.dim() != 1 or lut.shape[0] < 1:
            raise ValueError("lut must be a non-empty int32 [L] tensor")
        lut = lut.contiguous()
    if counts is not None:
        _lib.require_gpu(counts, "counts")
        if counts.dtype != torch.int64 or counts.dim() != 1 or not counts.is_contiguous():
            raise ValueError("counts must be a contiguous int64 [num_classes] tensor")
    info = torch.empty(4, dtype=torch.int32, device=dev)
    out_p = out_l = ws = None
    if points is not None:
        out_p = torch.empty((n, 3), dtype=torch.float32, device=dev)
        out_l = torch.empty(n, dtype=torch.int32, device=dev)
        ws = torch.empty(_lib.load().lidog_scan_load_ws(n), dtype=torch.int32, device=dev)
    mask = -1 if label_mask is None else int(np.array(label_mask, dtype=np.uint32).astype(np.int32))
    r2 = float(np.float32(float(in_radius) ** 2)) if in_radius is not None else 0.0
    call("lidog_scan_load", ptr(points), int(stride), ptr(labels_raw), kind, mask, n,
         ptr(lut) if kind else None, lut.shape[0] if kind else 0, 1 if in_radius is not None else 0, r2, ptr(out_p),
         ptr(out_l), ptr(counts), counts.shape[0] if counts is not None else 0, ptr(info), ptr(ws))
    return out_p, out_l, info


def _check_labels(labels_raw, name):
    if labels_raw is None:
        return None
    _lib.require_gpu(labels_raw, "labels")
    if labels_raw.dtype not in _LABEL_KINDS:
        raise ValueError(f"{name}: labels must be int32 or uint8, not {labels_raw.dtype}")
    return labels_raw.contiguous().reshape(-1)


def load_scan(points_raw, labels_raw, lut, point_stride, label_mask=None, in_radius=None, counts=None,
              use_intensity=False, name="scan"):
    """One scan from its files' bytes, all on the GPU (lidog_scan_load).
    points_raw: the point file as uploaded, float32 or raw bytes, `point_stride` floats per record (4 SemanticKITTI,
    5 nuScenes, the array's width for Synth4D).  labels_raw: int32 or uint8 [n], or None (no label file: label 0 for
    every row, unmapped, synth4d.py:115-116).  lut: int32 [L] (label_lut); label_mask: AND-mask on an int32 label before
    the look-up (0xFFFF for SemanticKITTI) or None.  in_radius: keep rows with x^2 + y^2 + z^2 < float32(in_radius^2),
    evaluated as numpy does on float32; None: no mask.  counts: int64 [num_classes] on the device, ADDED to with the
    mapped labels of all rows of the file (get_dataset_stats).
    Returns the scan dict lidog_amd.data.augment_item takes: `points` float32 [m,3], `features` float32 ones [m,1],
    `sem_labels` int32 [m], rows in file order.  Raises ValueError for sizes that do not fit (before anything is
    launched) and for a non-finite kept coordinate, IndexError for a raw label outside the table, as numpy's indexing.
    One device -> host read: `info`."""
    if use_intensity:
        raise NotImplementedError("use_intensity: the reference reads points[:, 3] of a [n, 3] array, and no "
                                  "configuration sets it")
    stride = int(point_stride)
    if stride < 3:
        raise ValueError(f"{name}: point_stride = {stride} (at least 3)")
    words = _as_words(points_raw, "points", name)
    if words.shape[0] % stride:
        raise ValueError(f"{name}: {words.shape[0] * 4} bytes of points are no multiple of the {4 * stride}-byte record")
    n = words.shape[0] // stride
    labels_raw = _check_labels(labels_raw, name)
    if labels_raw is not None and labels_raw.shape[0] != n:
        raise ValueError(f"{name}: points and labels have shape {n} and {labels_raw.shape[0]}")
    dev = words.device
    pts, lab, info = _launch(words, labels_raw, lut, stride, label_mask, in_radius, counts, n, dev)
    m, bad_labels, odd, _ = info.cpu().tolist()
    if bad_labels:
        raise IndexError(f"{name}: {bad_labels} raw labels are out of bounds for the label map of size {lut.shape[0]}")
    if odd:
        raise ValueError(f"{name}: {odd} points with a non-finite coordinate")
    pts, lab = pts[:m], lab[:m]
    return {"points": pts, "features": torch.ones((m, 1), dtype=torch.float32, device=dev), "sem_labels": lab}


def label_counts(labels_raw, lut, counts, label_mask=None, name="labels"):
    """get_dataset_stats on one label file: counts (int64 [num_classes], device) += the mapped labels.  Returns the
    device `info` (info[1] = labels outside the table); nothing is read back here."""
    labels_raw = _check_labels(labels_raw, name)
    if labels_raw is None or counts is None:
        raise ValueError("label_counts needs labels and counts")
    return _launch(None, labels_raw, lut, 0, label_mask, None, counts, labels_raw.shape[0], labels_raw.device)[2]


def keep_rows(points_raw, point_stride, in_radius=None, name="scan"):
    """(keep_row int32 [n], m int32 [1]) on the device (lidog_scan_keep_rows): keep_row[i] = the row record i of the file
    has in load_scan's `points`, -1 if the radius mask dropped it; m = the number of kept rows.  points_raw, point_stride
    and in_radius as load_scan takes them: the same float32 test, the same stable compaction, so
    points[keep_row >= 0] is load_scan's `points` bit for bit.  Nothing is read back."""
    stride = int(point_stride)
    if stride < 3:
        raise ValueError(f"{name}: point_stride = {stride} (at least 3)")
    words = _as_words(points_raw, "points", name)
    if words.shape[0] % stride:
        raise ValueError(f"{name}: {words.shape[0] * 4} bytes of points are no multiple of the {4 * stride}-byte record")
    n = words.shape[0] // stride
    dev = words.device
    keep = torch.empty(n, dtype=torch.int32, device=dev)
    m = torch.empty(1, dtype=torch.int32, device=dev)
    ws = None
    if in_radius is not None and n:
        ws = torch.empty(_lib.load().lidog_scan_keep_rows_ws(n), dtype=torch.int32, device=dev)
    r2 = float(np.float32(float(in_radius) ** 2)) if in_radius is not None else 0.0
    call("lidog_scan_keep_rows", ptr(words), stride, n, 1 if in_radius is not None else 0, r2, ptr(keep), ptr(m),
         ptr(ws))
    return keep, m


# ------------------------------------------------------------------ file listings
class Listing:
    """`files`: [(points file, label file)] of one dataset and phase, in the reference's order"""

    def __init__(self, name, files, phase):
        if name not in FORMATS:
            raise ValueError(f"dataset {name!r} (one of {NAMES})")
        self.name, self.files, self.phase, self.format = name, list(files), phase, FORMATS[name]

    def __len__(self):
        return len(self.files)

    def first(self, n):
        return Listing(self.name, self.files[:n] if n is not None else self.files, self.phase)


def _phase(phase):
    if phase not in PHASES:
        raise ValueError(f"phase {phase!r} (one of {PHASES})")
    return phase


def semantickitti_files(root, phase="train", version="full"):
    """semantickitti.py:65-72: `root/sequences/SS/{velodyne/NNNNNN.bin, labels/NNNNNN.label}`, the sequences of the split
    in order, frames 0 .. len(listdir(labels)) - 1"""
    if version not in SEMANTICKITTI_SPLITS:
        raise NotImplementedError(f"version {version!r} (one of {tuple(SEMANTICKITTI_SPLITS)})")
    files = []
    for sequence in SEMANTICKITTI_SPLITS[version][_phase(phase)]:
        seq = os.path.join(root, "sequences", sequence)
        if not os.path.isdir(os.path.join(seq, "labels")):
            raise FileNotFoundError(f"{seq}: sequence {sequence} of the {version} {phase} split has no labels folder")
        for f in range(len(os.listdir(os.path.join(seq, "labels")))):
            files.append((os.path.join(seq, "velodyne", f"{f:06d}.bin"), os.path.join(seq, "labels", f"{f:06d}.label")))
    return files


def load_obj(path):
    """synth4d.py:15-17"""
    with open(path, "rb") as f:
        return pickle.load(f)


def synth4d_files(root, name, splits_dir, phase="train"):
    """synth4d.py:52-83: `root/{kitti_synth|nuscenes_synth}/<town>/velodyne/<id>.npy` over the towns of the split
    pickle `<splits_dir>/<folder>/{training|validation}_split.pkl` in its order, np.sort of every town's ids; labels in
    `../labels/<id>.npy`.  The BEV configurations' pairing of sensor and split (initialization.py:339-413)."""
    folder = FORMATS[name]["folder"]
    split = load_obj(os.path.join(splits_dir, folder,
                                  "training_split.pkl" if _phase(phase) == "train" else "validation_split.pkl"))
    files = []
    if FORMATS[name].get("fake"):       # fake_synth4d.py:79-83: the same split, SemanticKITTI-style records
        for town in split.keys():
            for f in np.sort(split[town]):
                files.append((os.path.join(root, town, "velodyne", str(f).zfill(6) + ".bin"),
                              os.path.join(root, town, "labels", str(f).zfill(6) + ".label")))
        return files
    for town in split.keys():
        pc_path = os.path.join(root, folder, town, "velodyne")
        for f in np.sort(split[town]):
            files.append((os.path.join(pc_path, str(f) + ".npy"), os.path.join(pc_path, "../labels", str(f) + ".npy")))
    return files


def pair_list_files(root, phase="train"):
    """this project's index of a nuScenes tree: `root/train.txt` / `root/val.txt`, one `<points file> <label file>` per
    line, relative to root, in the order the scans are to be read"""
    path = os.path.join(root, "train.txt" if _phase(phase) == "train" else "val.txt")
    files = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 2:
                raise ValueError(f"{path}:{ln}: expected `<points file> <label file>`")
            files.append((os.path.join(root, parts[0]), os.path.join(root, parts[1])))
    return files


def listing(name, root, phase="train", version="full", synth4d_splits=None, limit=None):
    """the Listing of a dataset and phase, its first `limit` files.  `version` is SemanticKITTI's split; Synth4D's
    'mini' (a random draw of 100 scans per town, synth4d.py:66-70) is not restated: --limit-files serves that end."""
    if name in ("SemanticKITTI", "FakeKITTI"):
        files = semantickitti_files(root, phase, version)
    elif name == "nuScenes":
        files = pair_list_files(root, phase)
    elif name in FORMATS:
        if synth4d_splits is None:
            raise ValueError(f"{name} needs the folder of the split pickles (the reference's utils/datasets/_split)")
        files = synth4d_files(root, name, synth4d_splits, phase)
    else:
        raise ValueError(f"dataset {name!r} (one of {NAMES})")
    return Listing(name, files, phase).first(limit)


# ------------------------------------------------------------------ reading the files (host: bytes only)
def _read_bytes(path, record, what):
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.shape[0] % record:
        raise ValueError(f"{path}: {raw.shape[0]} bytes are no multiple of the {record}-byte {what} record")
    return raw


def read_files(fmt, points_path, labels_path, points=True):
    """(points array or None, labels array or None, point stride) as the reference's readers take them from the files:
    np.fromfile for SemanticKITTI / nuScenes (the bytes as they are), np.load(..).astype for Synth4D, whose missing label
    file means None"""
    if fmt["stride"] is not None:
        pts = _read_bytes(points_path, 4 * fmt["stride"], "point") if points else None
        if fmt.get("fake") and not os.path.exists(labels_path):     # fake_synth4d.py:111-112: zeros, unmapped
            return pts, None, fmt["stride"]
        labels = _read_bytes(labels_path, np.dtype(fmt["labels"]).itemsize, "label").view(fmt["labels"])
        return pts, labels, fmt["stride"]
    pts = stride = None
    if points:
        pts = np.load(points_path).astype(np.float32)
        if pts.ndim != 2 or pts.shape[1] < 3:
            raise ValueError(f"{points_path}: an array of shape {pts.shape} (expected [n, >= 3])")
        stride = pts.shape[1]
    labels = np.load(labels_path).astype(np.int32).reshape([-1]) if os.path.exists(labels_path) else None
    return pts, labels, stride


# ------------------------------------------------------------------ the dataset
class FileScans:
    """One or two listings as a dataset with `__len__`, `set_epoch`, `batch(indices, device)` and `class_counts()`.

    phase 'validation' (always the plain dataset, also for the BEV model: initialization.py:364-375, 434-442): every
    kept point, no bounds filter, voxelised; one listing.
    phase 'train': as AugmentedSynthScans.  With `augmentations` (a list over RandomRotation / RandomScale, the empty
    one included) every item draws int(sub_p * m) of its points in random order and transforms them; with None nothing
    is drawn (semantickitti_bev.py:211).  `bev=(bound, image size)`: the bounds filter with the ego box and BEV labels,
    from the voted labels for SemanticKITTI / Synth4D, from the first point's for nuScenes.  Two listings are paired by
    MultiSynthScans.pair's rule, each source's item made on its own, source 0 first.  The draws of item i in epoch e come
    from np.random.RandomState([seed, e, i]).  An index past the shorter listing's end takes a random scan of that
    listing from pair's own generator, which moves with every call: only for i < min(len) is a batch made twice the same
    batch, before and after a resume included.  `luts`: one int32 look-up table per listing.  `use_cache` keeps loaded
    scans on the device (the reference's CACHE of the `data` dict; off in every configuration).
    `raycast` (training only; a raycast.SensorSpec, a sensor's name or JSON file) resamples every scan to that sensor as
    seen from `raycast_origin` right after load_scan, before the cache, the draws and augment_item: the draws see the
    resampled point count (lidog_amd.raycast).
    `keep_raw` (validation only, an attribute that may be set later): every item made also leaves what the point-level
    evaluation needs, the uploaded file included, for point_item to hand out once.
    Items are made on data.merge_stream; per scan the host waits once for `info`, then for the sizes augment_item reads."""

    def __init__(self, listings, luts, voxel_size=0.05, augmentations=None, sub_p=0.8, seed=1234, bev=None,
                 ignore_label=-1, in_radius=50.0, use_cache=False, use_intensity=False, keep_raw=False, raycast=None,
                 raycast_origin=None):
        listings = [listings] if isinstance(listings, Listing) else list(listings)
        luts = [luts] if isinstance(luts, np.ndarray) else list(luts)
        if len(listings) not in (1, 2):
            raise NotImplementedError(f"{len(listings)} sources (the reference takes one or two)")
        if len(luts) != len(listings):
            raise ValueError(f"{len(luts)} look-up tables for {len(listings)} listings")
        if use_intensity:
            raise NotImplementedError("use_intensity: the reference reads points[:, 3] of a [n, 3] array, and no "
                                      "configuration sets it")
        phases = {l.phase for l in listings}
        if len(phases) != 1:
            raise ValueError("listings of different phases")
        self.phase = phases.pop()
        if self.phase == "validation" and len(listings) != 1:
            raise ValueError("a validation dataset is one listing (every source is validated on its own)")
        self.listings, self.num_sources = listings, len(listings)
        self.luts = [np.ascontiguousarray(l, dtype=np.int32) for l in luts]
        self.train = self.phase == "train"
        self.augmentations = check_augmentations(augmentations) if (self.train and augmentations is not None) else None
        self.sub_p = sub_p
        self.bev = bev if self.train else None
        self.voxel_size, self.ignore_label, self.in_radius = voxel_size, ignore_label, in_radius
        self.seed, self.epoch, self.use_cache = int(seed), 0, bool(use_cache)
        self.pairs = None
        if self.num_sources == 2:
            from .train import MultiSynthScans       # the pairing rule lives with the synthetic datasets
            self.pairs = MultiSynthScans(len(listings[0]), len(listings[1]), seed=seed)
        self._cache, self._dev_luts = {}, {}
        if keep_raw and self.train:
            raise ValueError("keep_raw: only the validation form keeps every point of a file")
        self.keep_raw, self._raw, self._point_items = bool(keep_raw), {}, {}
        self.raycast, self.raycast_origin = None, raycast_origin
        if raycast is not None:
            if not self.train:
                raise ValueError("raycast: only training scans are resampled, a target is validated as it is")
            from .raycast import sensor
            self.raycast = sensor(raycast)

    def __len__(self):
        return max(len(l) for l in self.listings)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def item_rng(self, i):
        return np.random.RandomState([self.seed, self.epoch, int(i)])

    def _lut(self, s, device):
        key = (s, str(device))
        if key not in self._dev_luts:
            self._dev_luts[key] = torch.from_numpy(self.luts[s]).to(device)
        return self._dev_luts[key]

    def scan(self, s, j, device):
        """the scan dict of file j of source s on `device` (load_scan), uploaded on the current stream"""
        key = (s, int(j), str(device))
        if key in self._cache:
            return self._cache[key]
        lst = self.listings[s]
        fmt = lst.format
        points_path, labels_path = lst.files[j]
        pts, labels, stride = read_files(fmt, points_path, labels_path)
        pts = torch.from_numpy(pts).to(device)
        labels = torch.from_numpy(labels).to(device) if labels is not None else None
        radius = self.in_radius if fmt["radius"] else None
        scan = load_scan(pts, labels, self._lut(s, device), stride, fmt["mask"], radius, name=points_path)
        if self.raycast is not None:    # the Raycast baseline: the scan as the target's sensor would have recorded it
            from .raycast import raycast_scan
            scan = raycast_scan(scan, self.raycast, self.raycast_origin)
        if self.keep_raw:       # the uploaded words themselves: the point path reads them again, nothing is copied
            words = _as_words(pts, "points", points_path)
            self._raw[key] = {"points_raw": words, "labels_raw": _check_labels(labels, points_path),
                              "stride": int(stride), "mask": fmt["mask"], "lut": self._lut(s, device),
                              "in_radius": radius, "rows": words.shape[0] // int(stride), "path": points_path}
        if self.use_cache:
            self._cache[key] = scan
        return scan

    def draws(self, rng, m):
        """the draws of one item of m points: the reference's sequence with an augmentation list, nothing otherwise"""
        if self.augmentations is None:
            return {"sampled_idx": np.arange(m), "ops": []}
        return draw_augmentation(rng, m, self.sub_p, self.augmentations)

    def _items(self, i, device):
        rng = self.item_rng(i)
        js = (int(i),) if self.pairs is None else self.pairs.pair(i)
        row = []
        for s, j in enumerate(js):
            scan = self.scan(s, j, device)
            row.append(augment_item(scan, self.draws(rng, scan["points"].shape[0]), voxel_size=self.voxel_size,
                                    bounds=self.bev is not None, ignore_label=self.ignore_label, bev=self.bev,
                                    bev_from=self.listings[s].format["bev_from"]))
            raw = self._raw.get((s, j, str(device))) if self.keep_raw else None
            if raw is not None:
                if not self.use_cache:
                    del self._raw[(s, j, str(device))]
                # `points`: load_scan's kept points themselves (no second upload), `plain`: rows in file order, untouched
                self._point_items[int(i)] = dict(raw, inverse_map=row[-1]["inverse_map"],
                                                 kept=int(scan["points"].shape[0]), points=scan["points"],
                                                 voxel_size=self.voxel_size, plain=self.augmentations is None,
                                                 voxels=int(row[-1]["coordinates"].shape[0]))
        return row

    def point_item(self, i, device="cuda"):
        """What the point-level evaluation needs of validation item i, made by the last item(i) / batch([.. i ..]) with
        `keep_raw` set; nothing is read or uploaded again.  A dict: `points_raw` (the file's float32 words), `labels_raw`
        (int32 / uint8 [rows] or None), `stride`, `mask`, `lut` (device int32), `in_radius` (None: no mask), `rows`,
        `kept`, `voxels` (the sizes of the file, of load_scan's output and of the item), `inverse_map` (kept row -> voxel
        row of the item), `path`, and for evaluate.point_queries `points` (load_scan's kept points, float32 [kept, 3]),
        `voxel_size` and `plain` (no augmentation touched the rows).  Handed out once: the file's words are dropped with the caller's reference."""
        if int(i) not in self._point_items:
            raise KeyError(f"item {i} was not made with keep_raw set (or its point inputs were taken already)")
        item = self._point_items.pop(int(i))
        cur = torch.cuda.current_stream(torch.device(device))
        for t in item.values():         # made on the merge stream, read on the caller's
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(cur)
        return item

    # ---- the item provider of lidog_amd.train.MixedSynthScans / ScaledSynthScans (see train.PlainSynthItems)
    @property
    def voxel(self):
        return self.voxel_size

    def draw_item(self, s, j, rng, device="cuda"):
        """the draws of file j of source s: the number of kept points is known once the file is loaded, so this needs the
        device; the loaded scan is kept for make_item"""
        device = torch.device("cuda" if device is None else device)
        scan = on_merge_stream(lambda: self.scan(s, j, device), device, wait=False)
        self._last = ((s, int(j), str(device)), scan)
        return self.draws(rng, scan["points"].shape[0])

    def make_item(self, s, j, draws, device):
        from .train import merge_scan
        device = torch.device(device)
        key, scan = getattr(self, "_last", (None, None))
        if key != (s, int(j), str(device)):
            scan = self.scan(s, j, device)
        self._last = (None, None)
        return merge_scan(augment_item(scan, draws, voxel_size=self.voxel_size, bounds=self.bev is not None,
                                       ignore_label=self.ignore_label), j)

    def class_weights(self, n=None, num_classes=None):
        w = self.class_counts()
        return (w,) if isinstance(w, np.ndarray) else tuple(w)

    def face_name(self, s):
        name = self.listings[s].name
        return NUSCENES_NAME if name == "nuScenes" else name

    def item(self, i, device="cuda"):
        """the items (one per source, lidog_amd.data.augment_item's dict) of index i in the current epoch"""
        device = torch.device(device)
        return on_merge_stream(lambda: self._items(i, device), device, wait=False)

    def batch(self, indices, device):
        device = torch.device(device)
        # the files are uploaded on the merge stream itself: it does not wait for the caller's stream
        return on_merge_stream(
            lambda: collate_items([self._items(i, device) for i in indices], self.bev is not None),
            device, wait=False)

    def class_counts(self, device="cuda"):
        """get_dataset_stats (semantickitti.py:199-213, synth4d.py:203-220) of every listing: float64
        [lut.max() + 1] per-class counts of the mapped labels of ALL points of all label files, the ignore label left
        out; one array for one listing, a tuple for two.  The counts are added on the device (integers) and read once
        per listing, with the label-error words of all files."""
        device = torch.device(device)
        out = []
        for s, lst in enumerate(self.listings):
            with torch.cuda.stream(merge_stream(device)):
                lut = self._lut(s, device)
                counts = torch.zeros(int(self.luts[s].max()) + 1, dtype=torch.int64, device=device)
                infos = []
                for _, labels_path in lst.files:
                    if lst.format["stride"] is None and not os.path.exists(labels_path):
                        raise FileNotFoundError(labels_path)       # np.load in get_dataset_stats
                    labels = read_files(lst.format, None, labels_path, points=False)[1]
                    infos.append(label_counts(torch.from_numpy(labels).to(device), lut, counts, lst.format["mask"],
                                              name=labels_path))
                bad = torch.stack(infos)[:, 1].cpu().numpy() if infos else np.zeros(0, np.int32)
                host = counts.cpu().numpy()
            if bad.any():
                raise IndexError(f"{lst.files[int(np.flatnonzero(bad)[0])][1]}: raw labels out of bounds for the label "
                                 f"map of size {self.luts[s].shape[0]}")
            out.append(host.astype(np.float64))
        return out[0] if len(out) == 1 else tuple(out)


def parse_files(entries):
    """['NAME=PATH', ...] of --files / --target-files -> [(name, path)]"""
    out = []
    for e in entries:
        name, sep, path = e.partition("=")
        if not sep or not path or name not in FORMATS:
            raise ValueError(f"{e!r}: expected NAME=PATH with NAME one of {NAMES}")
        out.append((name, path))
    return out


def luts_from_files(paths):
    return [label_lut(load_label_map(p)) for p in paths]


def add_file_arguments(ap, flag, what):
    """--files / --target-files and what goes with them (shared with lidog_amd.eval_target)"""
    ap.add_argument(flag, nargs="+", default=None, metavar="NAME=PATH",
                    help=f"{what} scans read from files (lidog_amd.scans): one or two entries, NAME one of SemanticKITTI, "
                         "Synth4D-kitti, Synth4D-nuscenes, nuScenes (a pair list train.txt / val.txt under PATH), or "
                         "FakeKITTI, FakeSynth4D-kitti, FakeSynth4D-nuscenes (written by lidog_amd.raycast)")
    ap.add_argument("--label-maps", nargs="+", default=None, metavar="FILE",
                    help="one label map per entry: a .yaml / .json file with a learning_map (the reference's *2common.yaml)")
    ap.add_argument("--synth4d-splits", default=None, metavar="DIR",
                    help="folder of the Synth4D split pickles (the reference's utils/datasets/_split)")
    ap.add_argument("--version", default="full", choices=["full", "mini"], help="SemanticKITTI split")
    ap.add_argument("--limit-files", type=int, default=None, metavar="N", help="first N files of every listing")


def check_file_arguments(ap, entries, a, flag):
    """[(name, path)] of a parsed --files / --target-files, or ap.error"""
    try:
        files = parse_files(entries)
    except ValueError as e:
        ap.error(f"{flag}: {e}")
    if len(files) > 2:
        ap.error(f"{flag}: {len(files)} entries (the reference takes one or two)")
    if a.label_maps is None or len(a.label_maps) != len(files):
        ap.error(f"{flag} needs --label-maps with one file per entry")
    if any("Synth4D" in n for n, _ in files) and a.synth4d_splits is None:
        ap.error(f"{flag}: a Synth4D entry needs --synth4d-splits")
    if a.limit_files is not None and a.limit_files < 1:
        ap.error("--limit-files must be positive")
    return files
