"""Device-side data path feeding the hot path.

  sparse_quantize  ME.utils.sparse_quantize as called at utils/datasets/semantickitti_bev.py:232-238
                   (floor(p / voxel) -> first point of every voxel, label vote, index + inverse maps)
  collate          ME.utils.SparseCollation (utils/collation/collation.py:309-310): batch index in column 0
  bev_labels       PC2ImgConverter.getBEVImageNew (utils/datasets/semantickitti_bev.py:433-464) on the voxel
                   coordinates (bev_points = quantized_coords * voxel_size, :244)

The reference runs these in DataLoader worker processes with numpy; at >50 scans/s per GPU that becomes the
bottleneck, and both are the same hash / winner-map kernels as the hot path.

  pointcutmix_merge, cosmix_merge   PointCutMix / CoSMix scan mixing (utils/datasets/pointcutmix.py, cosmix.py), below
  polarmix_merge, lasermix_merge    the sensor-aware mixes PolarMix / LaserMix, defined in include/lidog_amd.h, below
  average_dims, scaling_params, sn_scale  the SN car-size scaling baseline (train_scaling_based.py:35-129,
                   utils/datasets/sn_scaling.py)
  draw_augmentation, augment_item   sub_p / augmentation_list of the training datasets (dataset.py:58-72,
                   utils/common/augmentation.py, semantickitti_bev.py:209-252, synth4d.py:141-162), at the end
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr


def sparse_quantize(points, features=None, labels=None, ignore_label=-100, quantization_size=0.05,
                    return_index=False, return_inverse=False):
    """points float32 [n,3] on the GPU -> same tuple layout as ME.utils.sparse_quantize:
    (coords int32 [m,3], [features[index]], [voxel_labels], [index], [inverse])."""
    _lib.require_gpu(points, "points")
    points = points.contiguous().float()
    n = points.shape[0]
    q = np.broadcast_to(np.asarray(quantization_size, dtype=np.float32), (3,))
    rows = torch.empty((n, 4), dtype=torch.int32, device=points.device)
    call("lidog_voxel_floor", ptr(points), n, float(q[0]), float(q[1]), float(q[2]), 0, ptr(rows))
    return quantize_rows(rows, features, labels, ignore_label, return_index, return_inverse)


def quantize_rows(rows, features=None, labels=None, ignore_label=-100, return_index=False, return_inverse=False):
    """sparse_quantize from ready-made voxel rows (int32 [n,4]: batch, x, y, z; contiguous, on the GPU), as
    lidog_voxel_floor or lidog_augment_points write them: first point of every voxel, label vote, index and inverse maps.
    One device -> host read after the last launch: the number of voxels together with the range flag."""
    n = rows.shape[0]
    dev = rows.device
    cap = _lib.load().lidog_hash_capacity(n)
    keys = torch.empty(cap, dtype=torch.int64, device=dev)
    vals = torch.empty(cap, dtype=torch.int32, device=dev)
    first = torch.empty(n, dtype=torch.int32, device=dev)
    sizes = torch.zeros(2, dtype=torch.int64, device=dev)      # (voxels, range flag in the low word): read together
    call("lidog_coords_insert", ptr(rows), n, ptr(keys), ptr(vals), cap, ptr(first), ptr(sizes[:1]), ptr(sizes[1:]))
    uniq = torch.empty(n, dtype=torch.int32, device=dev)
    inv = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().lidog_coords_compact_ws(n), dtype=torch.int32, device=dev)
    call("lidog_coords_compact", ptr(first), n, ptr(keys), ptr(vals), cap, ptr(rows), ptr(uniq), ptr(inv), ptr(ws))
    m, bad = sizes.cpu().tolist()
    if bad:
        raise ValueError("voxel coordinates out of the supported range: -65536 <= x, y, z <= 65535, 0 <= batch <= 4095 "
                         "(a NaN or infinite point counts as out of range)")
    uniq = uniq[:m]
    index = uniq.long()
    out = [rows[index][:, 1:].contiguous()]
    if features is not None:
        out.append(features[index])
    if labels is not None:
        lab = labels.to(torch.int32).contiguous()
        vlab = torch.empty(m, dtype=torch.int32, device=dev)
        call("lidog_label_vote", ptr(lab), ptr(uniq.contiguous()), ptr(inv), n, m, int(ignore_label), ptr(vlab))
        out.append(vlab.to(labels.dtype))
    if return_index:
        out.append(index)
    if return_inverse:
        out.append(inv.long())
    return out[0] if len(out) == 1 else tuple(out)


def collate(scans):
    """list of (coords int [n_i,3], feats [n_i,C], labels [n_i]) on the GPU -> (coords [N,4] float32 with the batch
    index in column 0, feats, labels), i.e. ME.utils.SparseCollation(dtype=torch.float32)."""
    coords = torch.cat([torch.cat([torch.full((c.shape[0], 1), b, dtype=c.dtype, device=c.device), c], dim=1)
                        for b, (c, _, _) in enumerate(scans)], dim=0)
    return coords.float(), torch.cat([f for _, f, _ in scans], dim=0), torch.cat([l for _, _, l in scans], dim=0)


_LABEL_LUTS = {}


def label_luts(bound, img_size, voxel, z_range=(-10.0, 8.0)):
    """pixel of an integer voxel coordinate under getBEVImageNew's float32 arithmetic:
    x = float32(c * voxel); lo < x < hi; px = floor((x - lo) / grid); py = floor(S - (y - lo) / grid) - 1."""
    key = (float(bound), int(img_size), float(voxel), tuple(z_range))
    if key not in _LABEL_LUTS:
        grid = (bound - (-bound)) / img_size                   # python float, as in semantickitti_bev.py:144-145
        S = int((bound - (-bound)) / grid)                     # maxImgWidth / maxImgHeight (:340-341)
        lo_c = -int(1.3 * bound / voxel)
        c = np.arange(lo_c, -lo_c, dtype=np.int64)
        v = (c * voxel).astype(np.float32)                     # (quantized_coords * voxel_size).astype(np.float32)
        inb = (np.float32(-bound) < v) & (v < np.float32(bound))
        t = (v - np.float32(-bound)) / np.float32(grid)
        px = np.floor(t).astype(np.int64)
        py = np.floor(np.float32(S) - t).astype(np.int64) - 1
        px = np.where(px < 0, px + S, px)                      # numpy indexing wraps negatives like torch
        py = np.where(py < 0, py + S, py)
        lut_x = np.where(inb & (px >= 0) & (px < S), px, -1).astype(np.int32)
        lut_y = np.where(inb & (py >= 0) & (py < S), py, -1).astype(np.int32)
        lut_z = ((np.float32(z_range[0]) < v) & (v < np.float32(z_range[1]))).astype(np.int32)
        _LABEL_LUTS[key] = (lut_x, lut_y, lut_z, lo_c, S)
    return _LABEL_LUTS[key]


_DEV_LABEL_LUTS = {}


def bev_labels(coords, labels, bound=50.0, img_size=167, voxel=0.05, batch_size=None):
    """coords int32 [N,4] (batch, x, y, z) on the GPU, labels [N] -> (img_labels int64 [B,S,S], point_idx int32
    [B,S,S]) exactly as getBEVImageNew applied scan by scan (ignore label -1 skipped, last point wins).
    `batch_size`: number of scans in the batch when the caller knows it (a collate function does): nothing is read
    back from the device then."""
    _lib.require_gpu(coords, "coordinates")
    dev = coords.device
    key = (float(bound), int(img_size), float(voxel), str(dev))
    if key not in _DEV_LABEL_LUTS:
        lx, ly, lz, lo, S = label_luts(bound, img_size, voxel)
        _DEV_LABEL_LUTS[key] = (torch.from_numpy(lx).to(dev), torch.from_numpy(ly).to(dev),
                                torch.from_numpy(lz).to(dev), lo, S)
    lx, ly, lz, lo, S = _DEV_LABEL_LUTS[key]
    coords = coords.contiguous()
    lab = labels.to(torch.int32).contiguous()
    B = int(batch_size) if batch_size is not None else int(coords[:, 0].max().item()) + 1
    counts = torch.bincount(coords[:, 0].long(), minlength=B)
    start = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    start[1:] = torch.cumsum(counts, 0)
    pidx = torch.full((B, S, S), -1, dtype=torch.int32, device=dev)
    img = torch.empty((B, S, S), dtype=torch.int64, device=dev)
    call("lidog_bev_label_raster", ptr(coords), ptr(lab), coords.shape[0], ptr(lx), ptr(ly), ptr(lz), lo, lx.shape[0],
         B, S, ptr(start), ptr(pidx), ptr(img))
    return img, pidx


def mix3d_merge(scan0, scan1, voxel_size=0.05, ignore_label=-1):
    """Mix3DSourceDataset.merge_data (utils/datasets/mix3D.py:44-87): union of two voxelised scans, re-quantised.
    scan = dict(coordinates int [n,3], features [n,C], sem_labels [n]) on the GPU.  As in the reference the
    coordinates go through float32 (`coordinates * voxel_size`, then floor(x / voxel_size)), and the label of a
    merged voxel is the label of its FIRST point (the voted labels returned by sparse_quantize are discarded).  Scans
    that carry `xyz` / `sampled_idx` / `idx` also give the reference's `xyz` (the unfiltered concatenation),
    `sampled_idx` (of the voxels' first points) and `idx` [2, 1]."""
    coords = torch.cat([scan0["coordinates"], scan1["coordinates"]], dim=0).float() * voxel_size
    feats = torch.cat([scan0["features"], scan1["features"]], dim=0)
    labels = torch.cat([scan0["sem_labels"], scan1["sem_labels"]], dim=0)
    q, _, _, idx = sparse_quantize(coords, feats, labels=labels, ignore_label=ignore_label,
                                   quantization_size=voxel_size, return_index=True)
    out = {"coordinates": q, "features": feats[idx], "sem_labels": labels[idx], "index": idx}
    # the reference's remaining keys (mix3D.py:61-86), when the scans carry them: xyz is NOT filtered by the voxels
    for k in ("xyz", "sampled_idx", "idx"):
        if (k in scan0) != (k in scan1):
            raise KeyError(f"'{k}' in one scan only")
    if "xyz" in scan0:
        out["xyz"] = torch.cat([scan0["xyz"], scan1["xyz"]], dim=0)
    if "sampled_idx" in scan0:
        out["sampled_idx"] = torch.cat([scan0["sampled_idx"], scan1["sampled_idx"]], dim=0)[idx]
    if "idx" in scan0:
        out["idx"] = torch.cat([scan0["idx"].view(1, -1), scan1["idx"].view(1, -1)], dim=0)
    return out


# ------------------------------------------------------------------ scan mixing: PointCutMix and CoSMix
# PointCutMixSourceDataset.merge_data (utils/datasets/pointcutmix.py:43-135) and CoSMixSourceDataset.merge_data
# (utils/datasets/cosmix.py:50-171), which pair their sources as MultiBEVSourceDataset (lidog_amd.train.MultiSynthScans).
# The random draws are made on the host in the reference's exact sequence (rng: numpy's legacy RandomState, or the
# np.random module itself), so that `np.random.seed(s)` then a merge here selects the same source, cells or classes and
# sub-samples as the reference's merge_data after the same seed.  The device does the per-point work (mix.hip): the
# counts the draws need, the stable split of the source rows into the drawn cells / classes, the merged point set, and
# the re-quantisation.  Device -> host reads: the counts of the draws and the sizes sparse_quantize reads back.

_MERGE_STREAMS = {}


def merge_stream(device=None):
    """the stream the merges of `device` run on.  A caller that makes a merge's input tensors on this stream and calls
    the merge with it current (lidog_amd.train.MixedSynthScans) keeps the merge's read-backs off any work queued on its
    other streams, a training step among them."""
    dev = torch.device("cuda") if device is None else torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _MERGE_STREAMS:
        _MERGE_STREAMS[idx] = torch.cuda.Stream(device=idx)
    return _MERGE_STREAMS[idx]


def on_merge_stream(work, device, inputs=(), wait=True):
    """run `work()` on merge_stream(device) and hand its result (a dict or list of tensors) to the caller's current stream
    with an event; the caching allocator is told about every tensor that crosses streams, nested ones included (a batch
    holds its BEV label images in a dict of their own).  wait=True: the merge stream first waits for the work queued on
    the caller's stream, where `inputs` may have been made; wait=False: work() makes its own inputs on the merge stream,
    and nothing queued on the caller's stream delays it."""
    cur = torch.cuda.current_stream(device)
    side = merge_stream(device)
    if side == cur:
        return work()
    if wait:
        side.wait_stream(cur)
    for t in _device_tensors(list(inputs)):
        t.record_stream(side)
    with torch.cuda.stream(side):
        out = work()
    cur.wait_stream(side)
    for t in _device_tensors(out):
        t.record_stream(cur)
    return out


def _device_tensors(obj):
    """every CUDA tensor reachable from obj through dicts, lists and tuples (a batch nests its BEV label images)"""
    if torch.is_tensor(obj):
        return [obj] if obj.is_cuda else []
    if isinstance(obj, dict):
        obj = list(obj.values())
    if isinstance(obj, (list, tuple)):
        return [t for v in obj for t in _device_tensors(v)]
    return []


def draw_source(rng):
    """`selected_source = np.random.choice([0, 1])` (pointcutmix.py:66, cosmix.py:90); the other scan is the target"""
    return int(rng.choice([0, 1]))


def draw_cells(rng, counts, min_points=300, n_cells=4):
    """pointcutmix.py:91-92: `np.random.choice(vox_idx[count > 300], 4, replace=False)` over the cells of the source's
    cell_size quantisation (counts[c] = source rows in cell c); raises ValueError when fewer than n_cells qualify"""
    counts = np.asarray(counts)
    vox_idx = np.arange(counts.shape[0])
    return rng.choice(vox_idx[counts > min_points], n_cells, replace=False)


def draw_classes(rng, counts, weights, sub_p, augmentations=None):
    """cosmix.py:108-136 (random_sample :53-63): the classes present in the source (counts[c] = its rows of class c), `int(len / 2)` of them
    drawn with p = weights[class_idx] * (1 / weights[class_idx].sum()), then for each drawn class, in order, the
    sub-sample `np.random.choice(np.arange(n_c), int(sub_p * n_c), replace=False)` (sub_p None: arange(n_c)) and, with
    `augmentations` (a list of names, the empty one included), the list's own draws (draw_ops) right after it.
    Returns (classes, [sub-sample of each class]), with a list also [ops of each class]."""
    counts = np.asarray(counts)
    weights = np.asarray(weights, dtype=np.float64)
    class_idx = np.nonzero(counts)[0]
    sampling_weights = weights[class_idx] * (1 / weights[class_idx].sum())
    classes = rng.choice(class_idx, int(len(class_idx) / 2), p=sampling_weights, replace=False)
    subs, ops = [], []
    for c in classes:
        n_c = int(counts[c])
        subs.append(rng.choice(np.arange(n_c), int(sub_p * n_c), replace=False) if sub_p is not None
                    else np.arange(n_c))
        if augmentations is not None:
            ops.append(draw_ops(rng, augmentations))
    return (classes, subs) if augmentations is None else (classes, subs, ops)


_MERGE_COLUMNS = ("features", "sem_labels", "xyz", "sampled_idx")


def _check_scans(scan0, scan1):
    for s, scan in enumerate((scan0, scan1)):
        for k in ("coordinates", "features", "sem_labels"):
            if k not in scan:
                raise KeyError(f"scan {s} has no '{k}'")
        for k in ("coordinates",) + _MERGE_COLUMNS:
            if k in scan:
                _lib.require_gpu(scan[k], f"scan {s} '{k}'")
    for k in ("xyz", "sampled_idx", "idx"):
        if (k in scan0) != (k in scan1):
            raise KeyError(f"'{k}' in one scan only")
    return (scan0, scan1)


def _device_counts(keys, nbins):
    """counts of keys in [0, nbins) (lidog_mix_histogram), read back: one small device -> host copy"""
    counts = torch.empty(max(nbins, 1), dtype=torch.int32, device=keys.device)
    call("lidog_mix_histogram", ptr(keys), keys.shape[0], nbins, ptr(counts))
    return counts[:nbins].cpu().numpy().astype(np.int64)


def _split(keys, slot_of_key, n_slots):
    """(rows grouped by slot, slot_start) of lidog_mix_split"""
    dev = keys.device
    n = keys.shape[0]
    table = torch.from_numpy(np.ascontiguousarray(slot_of_key, dtype=np.int32)).to(dev)
    rows = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    start = torch.empty(n_slots + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().lidog_mix_split_ws(n, n_slots), dtype=torch.int32, device=dev)
    call("lidog_mix_split", ptr(keys), n, ptr(table), table.shape[0], n_slots, ptr(rows), ptr(start), ptr(ws))
    return rows, start


def _merge_columns(tgt, src, total):
    """the merged columns of a gather: ({name: empty [total, ...]}, the (target, source, merged) pointer triples, the
    32-bit words per row, the contiguous inputs the pointers belong to)"""
    dev = tgt["coordinates"].device
    cols, ptrs, words, inputs = {}, [], [], []
    for k in _MERGE_COLUMNS:
        if k not in tgt:
            continue
        t = tgt[k].contiguous()
        s = src[k].to(t.dtype).contiguous()
        row_bytes = int(np.prod(t.shape[1:], dtype=np.int64)) * t.element_size()
        if row_bytes % 4 or t.shape[1:] != s.shape[1:]:
            raise NotImplementedError(f"'{k}': rows of {row_bytes} bytes ({t.dtype}, {tuple(t.shape[1:])}) "
                                      f"against {tuple(s.shape[1:])} (whole 32-bit words and equal shapes only)")
        cols[k] = torch.empty((total,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
        ptrs += [t.data_ptr(), s.data_ptr(), cols[k].data_ptr()]
        words.append(row_bytes // 4)
        inputs += [t, s]
    return cols, ptrs, words, inputs


def _merge(scan0, scan1, sel, voxel_size, rows, start, n_take, subs=None, class_ops=None):
    """target rows, then the selected source rows (lidog_mix_gather), re-quantised at voxel_size; the reference's dict.
    class_ops (one op list per slot, as draw_ops returns them; [] when no class was drawn): CoSMix's in-merge
    augmentation, lidog_mix_gather_aug writes the voxel rows itself."""
    src, tgt = (scan0, scan1) if sel == 0 else (scan1, scan0)
    dev = tgt["coordinates"].device
    nt = tgt["coordinates"].shape[0]
    total = nt + n_take
    coords_t = tgt["coordinates"].to(torch.int32).contiguous()
    coords_s = src["coordinates"].to(torch.int32).contiguous()
    cols, ptrs, words, _inputs = _merge_columns(tgt, src, total)
    perm = take = None
    n_slots = 0 if start is None else start.shape[0] - 1
    if subs is not None and n_slots:
        take_start = np.concatenate([[0], np.cumsum([len(p) for p in subs])]).astype(np.int32)
        buf = torch.from_numpy(np.concatenate([take_start] + [np.asarray(p, dtype=np.int32) for p in subs])).to(dev)
        take, perm = buf[:n_slots + 1], buf[n_slots + 1:]
    col_ptrs = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
    col_words = (ctypes.c_int32 * max(len(words), 1))(*words)
    if class_ops is None:
        merged = torch.empty((total, 3), dtype=torch.float32, device=dev)
        call("lidog_mix_gather", ptr(coords_t), nt, ptr(coords_s), ptr(rows), ptr(start), ptr(perm), ptr(take), n_slots,
             n_take, float(np.float32(voxel_size)), ptr(merged), len(words), col_ptrs, col_words)
        q, index = sparse_quantize(merged, quantization_size=voxel_size, return_index=True)
    else:
        q, index = _gather_aug(coords_t, coords_s, rows, start, perm, take, n_slots, n_take, subs, class_ops, voxel_size,
                               len(words), col_ptrs, col_words)
    out = {"coordinates": q}
    for k in ("xyz", "features", "sem_labels"):
        if k in cols:
            out[k] = cols[k][index]
    if "idx" in scan0:
        out["idx"] = torch.cat([scan0["idx"].view(1, -1), scan1["idx"].view(1, -1)], dim=0)
    if "sampled_idx" in cols:
        out["sampled_idx"] = cols["sampled_idx"][index]
    out["index"] = index
    out["source"] = sel
    return out


def _gather_aug(coords_t, coords_s, rows, start, perm, take, n_slots, n_take, subs, class_ops, voxel_size, n_cols,
                col_ptrs, col_words):
    """lidog_mix_gather_aug, then quantize_rows: (voxel coordinates, first point of every voxel).  The dtype the
    reference floors in: a class's rows leave a rotation as float64 (`float32_tensor @ float64_ndarray`), and torch.cat
    promotes the whole concatenation, the float32 target rows included, once one class tensor is float64, an EMPTY one
    too ([0, 3] tensors take part in cat's type promotion).  No class drawn, or no rotation in the list: float32."""
    dev = coords_t.device
    nt, total = coords_t.shape[0], coords_t.shape[0] + n_take
    names = [a for a, _ in class_ops[0]] if class_ops else []
    if any([a for a, _ in ops] != names for ops in class_ops) or len(class_ops) != n_slots:
        raise ValueError("cosmix_merge: one op list per drawn class, over the same names")
    if len(names) > 4:
        raise NotImplementedError(f"cosmix_merge: {len(names)} augmentations (at most 4)")
    kinds = (ctypes.c_int32 * max(len(names), 1))(*[AUGMENTATIONS.index(a) for a in names])
    params = np.zeros((max(n_slots, 1), max(len(names), 1), 9), dtype=np.float64)
    for s_, ops in enumerate(class_ops):
        for o, (a, p) in enumerate(ops):
            p = np.asarray(p, dtype=np.float64).reshape(-1)
            if p.shape[0] != (9 if a == "RandomRotation" else 3) or not np.all(np.isfinite(p)):
                raise ValueError(f"cosmix_merge: parameters of {a}: {p}")
            params[s_, o, :p.shape[0]] = p
    f64 = 1 if (n_slots and "RandomRotation" in names) else 0
    if n_slots and (take is None or perm is None):
        raise ValueError("cosmix_merge: the augmented gather needs every class's sub-sample")
    slot_params = torch.from_numpy(params).to(dev) if n_slots and names else None
    q3 = np.broadcast_to(np.asarray(voxel_size, dtype=np.float64), (3,))
    vrows = torch.empty((total, 4), dtype=torch.int32, device=dev)
    call("lidog_mix_gather_aug", ptr(coords_t), nt, ptr(coords_s), coords_s.shape[0], ptr(rows), ptr(start), ptr(perm),
         ptr(take), n_slots, n_take, float(np.float32(voxel_size)), kinds, len(names), ptr(slot_params), f64,
         float(q3[0]), float(q3[1]), float(q3[2]), ptr(vrows), n_cols, col_ptrs, col_words)
    return quantize_rows(vrows, return_index=True)


def pointcutmix_merge(scan0, scan1, voxel_size=0.05, ignore_label=-1, rng=np.random, cell_size=10.0, min_points=300,
                      n_cells=4):
    """PointCutMixSourceDataset.merge_data (utils/datasets/pointcutmix.py:43-135) on the GPU.
    scan = dict of device tensors: coordinates int [n,3], features [n,C], sem_labels [n], optionally xyz [n,3],
    sampled_idx [n], idx.  One scan (`source`, drawn first) is quantised at cell_size (float32 coordinates
    `coordinates * voxel_size`, as the reference); n_cells of its cells holding more than min_points rows are drawn, and
    the other scan's rows followed by the rows of those cells (cell by cell in the order drawn, ascending rows inside a
    cell) are re-quantised at voxel_size.  features / xyz / sem_labels / sampled_idx are those of the first point of
    every voxel (no label vote, as the reference).  Returns the reference's dict plus `index` (the first point of every
    voxel in the concatenation) and `source`.  Raises ValueError when fewer than n_cells cells qualify, as the
    reference's np.random.choice.  `ignore_label` is the reference's argument; its label vote is discarded."""
    scans = _check_scans(scan0, scan1)
    sel = draw_source(rng)
    dev = scan0["coordinates"].device

    def work():
        src = scans[sel]
        n = src["coordinates"].shape[0]
        points = src["coordinates"].to(torch.float32) * voxel_size
        cells, inverse = sparse_quantize(points, quantization_size=cell_size, return_inverse=True)
        inverse = inverse.to(torch.int32)
        counts = _device_counts(inverse, cells.shape[0])
        chosen = draw_cells(rng, counts, min_points, n_cells)
        slot_of_cell = np.full(cells.shape[0], -1, dtype=np.int32)
        slot_of_cell[chosen] = np.arange(len(chosen), dtype=np.int32)
        rows, start = _split(inverse, slot_of_cell, len(chosen))
        n_take = int(counts[chosen].sum())
        assert n_take <= n
        return _merge(scan0, scan1, sel, voxel_size, rows, start, n_take)

    return on_merge_stream(work, dev, [t for s in scans for t in s.values()])


def cosmix_merge(scan0, scan1, voxel_size=0.05, class_weights=None, sub_p=0.8, ignore_label=-1, rng=np.random,
                 augmentations=None):
    """CoSMixSourceDataset.merge_data (utils/datasets/cosmix.py:50-171) on the GPU; scans as pointcutmix_merge.
    class_weights = (w0, w1): per-class point counts of each source's training set (Synth4DDataset.get_dataset_stats,
    synth4d.py:203-220).  Of the classes present in the drawn source (labels in [0, len(w)); -1 is never a class) half
    are drawn with probability proportional to their weight; each class's rows (ascending) are sub-sampled by a random
    permutation prefix of int(sub_p * n_c) rows (sub_p None: all of them, in order) and appended, class by class in the
    order drawn, to the other scan's rows; the union is re-quantised at voxel_size.  Returns the reference's dict plus
    `index` and `source`.
    augmentations: the source datasets' `augmentation_list` (20 of the reference's configurations set it under the
    mixing datasets: mix3D/, pointcutmix/, cosmix/, SN/), a list over RandomRotation / RandomScale, the empty one
    included: every pasted class is transformed by draws of its own made right after its sub-sample (cosmix.py:128-136);
    `xyz` is sub-sampled but not transformed.  With a rotation in the list and a class drawn the reference floors the
    whole concatenation, the target's rows too, in float64, which moves about 40 % of the target's voxels by one: kept.
    None: no transform and nothing drawn for it.  Anything but a list of names raises NotImplementedError."""
    if augmentations is not None:
        if not isinstance(augmentations, (list, tuple)) or not all(isinstance(a, str) for a in augmentations):
            raise NotImplementedError("cosmix_merge: augmentations must be None or a list of names over "
                                      f"{AUGMENTATIONS}, not {type(augmentations).__name__}")
        augmentations = check_augmentations(augmentations)
    if class_weights is None or len(class_weights) != 2:
        raise ValueError("cosmix_merge needs class_weights = (w0, w1), one per-class count array per source")
    scans = _check_scans(scan0, scan1)
    sel = draw_source(rng)
    weights = np.asarray(class_weights[sel], dtype=np.float64)
    dev = scan0["coordinates"].device

    def work():
        labels = scans[sel]["sem_labels"].to(torch.int32).contiguous()
        counts = _device_counts(labels, weights.shape[0])
        drawn = draw_classes(rng, counts, weights, sub_p, augmentations)
        classes, subs = drawn[0], drawn[1]
        class_ops = drawn[2] if augmentations is not None else None
        for c, p in zip(classes, subs):      # the gather reads rows[slot_start[s] + p]: p must lie inside the class
            if len(p) and (int(np.min(p)) < 0 or int(np.max(p)) >= int(counts[c])):
                raise RuntimeError("cosmix_merge: a sub-sample index outside its class")
        if len(classes) == 0:
            return _merge(scan0, scan1, sel, voxel_size, None, None, 0, class_ops=class_ops)
        slot_of_class = np.full(weights.shape[0], -1, dtype=np.int32)
        slot_of_class[classes] = np.arange(len(classes), dtype=np.int32)
        rows, start = _split(labels, slot_of_class, len(classes))
        n_take = int(sum(len(p) for p in subs))
        # with the transforms the gather needs every class's extent: sub_p None passes its identity sub-samples
        return _merge(scan0, scan1, sel, voxel_size, rows, start, n_take,
                      subs if sub_p is not None or class_ops is not None else None, class_ops=class_ops)

    return on_merge_stream(work, dev, [t for s in scans for t in s.values()])


# ------------------------------------------------------------------ sensor-aware scan mixing: PolarMix and LaserMix
# PolarMix (Xiao et al., NeurIPS 2022) and LaserMix (Kong et al., CVPR 2023) are not in the reference; include/lidog_amd.h
# defines both in exact arithmetic on the voxel centres (X, Y, Z) = (2x + 1, 2y + 1, 2z + 1), the sensor at the origin,
# and tests/sensormix_ref.py restates that in numpy.  The host makes the draws and the float64 constants (directions,
# squared tangents, cosines and sines); the device writes one key per row, selects the three row lists (kept base rows,
# taken donor rows, pasted donor rows) and gathers the merged voxel rows (csrc/sensormix.hip), which quantize_rows then
# reduces to the first row of every voxel.  One device -> host read of the three sizes, one of quantize_rows.

SENSORMIX_MAX_AREAS = 8         # 3 bits of band: at most 7 interior boundaries


def draw_polarmix(rng, swap_prob=0.5, paste_prob=1.0):
    """PolarMix's host draws, always all six in this order: the donor scan, the sector's start azimuth alpha in
    [-pi, 0) (the sector is the half-plane alpha .. alpha + pi), the two paste rotations omega1 in [0, 2pi/3) and
    omega2 in [2pi/3, 4pi/3), whether the sector is swapped, whether the instance classes are pasted"""
    sel = draw_source(rng)
    alpha = (rng.random_sample() - 1) * np.pi
    omega1 = rng.random_sample() * 2 * np.pi / 3
    omega2 = (rng.random_sample() + 1) * 2 * np.pi / 3
    swap = bool(rng.random_sample() < swap_prob)
    paste = bool(rng.random_sample() < paste_prob)
    return {"source": sel, "alpha": float(alpha), "omega1": float(omega1), "omega2": float(omega2), "swap": swap,
            "paste": paste}


def draw_lasermix(rng, areas=(3, 4, 5, 6)):
    """LaserMix's host draws: the scan whose odd bands are taken, then the number of inclination bands"""
    sel = draw_source(rng)
    return {"source": sel, "n_areas": int(rng.choice(areas))}


def band_bounds(pitch, n_areas):
    """(t2, neg) of the n_areas - 1 interior boundaries of the pitch range (degrees) cut into n_areas equal bands:
    tan(theta)^2 and tan(theta) < 0, float64 and int32, as lidog_sensormix_keys takes them"""
    lo, hi = float(pitch[0]), float(pitch[1])
    if not (-90.0 < lo < hi < 90.0):
        raise ValueError(f"pitch range {pitch}: -90 < lo < hi < 90 degrees")
    if not 1 <= int(n_areas) <= SENSORMIX_MAX_AREAS:
        raise ValueError(f"{n_areas} inclination bands (1 .. {SENSORMIX_MAX_AREAS})")
    t = np.tan(np.linspace(np.radians(lo), np.radians(hi), int(n_areas) + 1)[1:-1])
    return t * t, (t < 0).astype(np.int32)


def instance_mask(instance_classes):
    """the uint32 class mask of lidog_sensormix_keys"""
    mask = 0
    for c in instance_classes:
        if not 0 <= int(c) < 32:
            raise ValueError(f"instance class {c}: 0 .. 31 (label -1 is never pasted)")
        mask |= 1 << int(c)
    return mask


def _key_set(pred):
    """the keys k in [0, 32) of lidog_sensormix_keys with pred(sector bit, band, instance bit), as a bit set"""
    return sum(1 << k for k in range(32) if pred(k & 1, (k >> 1) & 7, (k >> 4) & 1))


def _sensor_merge(scan0, scan1, sel, a, b, bounds, mask, keep, take, paste, copies):
    """base = the scan that is not `sel`: its rows whose key is in `keep`, then the donor's rows with a key in `take`,
    then for every (c, s) of `copies` the donor's rows with a key in `paste` rotated about z; quantised.  The dict of
    _merge plus `counts`, the sizes of those segments."""
    donor, base = (scan0, scan1) if sel == 0 else (scan1, scan0)
    dev = base["coordinates"].device
    nb, nd = base["coordinates"].shape[0], donor["coordinates"].shape[0]
    coords_b = base["coordinates"].to(torch.int32).contiguous()
    coords_d = donor["coordinates"].to(torch.int32).contiguous()
    labels_b = base["sem_labels"].to(torch.int32).contiguous() if mask else None
    labels_d = donor["sem_labels"].to(torch.int32).contiguous() if mask else None
    t2, neg = bounds
    t2 = (ctypes.c_double * max(len(t2), 1))(*[float(v) for v in t2])
    n_bounds = len(neg)
    neg = (ctypes.c_int32 * max(n_bounds, 1))(*[int(v) for v in neg])
    keys = torch.empty(max(nb + nd, 1), dtype=torch.int32, device=dev)
    meta = torch.empty(8, dtype=torch.int32, device=dev)           # the three (start, size) pairs, then the range flag
    call("lidog_sensormix_keys", ptr(coords_b), ptr(labels_b), nb, ptr(coords_d), ptr(labels_d), nd, float(a[0]),
         float(a[1]), float(b[0]), float(b[1]), 0, t2, neg, n_bounds, mask, ptr(keys), ptr(meta[6:]))
    lists = torch.empty(max(nb + 2 * nd, 1), dtype=torch.int32, device=dev)
    rows_keep, rows_take, rows_paste = lists[:nb], lists[nb:nb + nd], lists[nb + nd:nb + 2 * nd]
    ws = torch.empty(_lib.load().lidog_sensormix_select_ws(nb, nd), dtype=torch.int32, device=dev)
    call("lidog_sensormix_select", ptr(keys[:nb]), nb, ptr(keys[nb:nb + nd]), nd, keep, take, paste, ptr(rows_keep),
         ptr(rows_take), ptr(rows_paste), ptr(meta), ptr(ws))
    m = meta.cpu().tolist()
    if m[6]:
        raise ValueError("voxel coordinates out of the range of the sensor-aware mixes: |x|, |y|, |z| < 2^24")
    n_keep, n_take, n_paste = m[1], m[3], m[5]
    n_copies = len(copies) if n_paste else 0
    total = n_keep + n_take + n_copies * n_paste
    cols, ptrs, words, _inputs = _merge_columns(base, donor, total)
    col_ptrs = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
    col_words = (ctypes.c_int32 * max(len(words), 1))(*words)
    cs = (ctypes.c_double * max(2 * len(copies), 1))(*[float(v) for c_s in copies for v in c_s])
    vrows = torch.empty((total, 4), dtype=torch.int32, device=dev)
    call("lidog_sensormix_gather", ptr(coords_b), nb, ptr(coords_d), nd, ptr(rows_keep), n_keep, ptr(rows_take), n_take,
         ptr(rows_paste), n_paste, cs, len(copies), ptr(vrows), len(words), col_ptrs, col_words)
    q, index = quantize_rows(vrows, return_index=True)
    out = {"coordinates": q}
    for k in ("xyz", "features", "sem_labels"):
        if k in cols:
            out[k] = cols[k][index]
    if "idx" in scan0:
        out["idx"] = torch.cat([scan0["idx"].view(1, -1), scan1["idx"].view(1, -1)], dim=0)
    if "sampled_idx" in cols:
        out["sampled_idx"] = cols["sampled_idx"][index]
    out["index"] = index
    out["source"] = sel
    out["counts"] = (n_keep, n_take) + (n_paste,) * len(copies)
    return out


def lasermix_merge(scan0, scan1, rng=np.random, pitch=(-25.0, 3.0), areas=(3, 4, 5, 6), draws=None):
    """LaserMix on the GPU; scans as pointcutmix_merge.  Draws (draw_lasermix; `draws`: a ready dict, nothing is drawn)
    the scan `source` and n_areas; the pitch range (degrees, the sensor's vertical field of view) is cut into n_areas
    equal inclination bands, rows below the range counting to band 0 and rows above it to the last one.  Merged rows:
    the OTHER scan's rows in even bands, ascending, then scan `source`'s rows in odd bands, ascending.  A voxel lies in
    the same band in both scans, so the union holds no voxel twice; quantize_rows still gives the usual `index`.
    Returns the dict of the other merges plus `counts` = (base rows kept, rows taken).  The inclination is that of the
    voxel centre seen from the coordinate origin: the scans must be in their sensor's frame."""
    scans = _check_scans(scan0, scan1)
    d = draw_lasermix(rng, areas) if draws is None else draws
    bounds = band_bounds(pitch, d["n_areas"])
    dev = scan0["coordinates"].device

    def work():
        return _sensor_merge(scan0, scan1, d["source"], (1.0, 0.0), (1.0, 0.0), bounds, 0,
                             _key_set(lambda s, band, i: band % 2 == 0), _key_set(lambda s, band, i: band % 2 == 1), 0,
                             ())

    return on_merge_stream(work, dev, [t for s in scans for t in s.values()])


def polarmix_merge(scan0, scan1, rng=np.random, instance_classes=(0, 1), swap_prob=0.5, paste_prob=1.0, draws=None):
    """PolarMix on the GPU; scans as pointcutmix_merge.  Draws (draw_polarmix, always all six; `draws`: a ready dict,
    nothing is drawn) the donor scan `source`, alpha, omega1, omega2, swap and paste.  The sector is the half-plane of
    azimuths alpha .. alpha + pi.  Merged rows: the other (base) scan's rows, ascending, with `swap` only those outside
    the sector; with `swap` the donor's rows inside the sector; with `paste` the donor's rows whose label is in
    instance_classes (the whole donor scan; label -1 never) three times: as they are, rotated about z by omega1 and by
    omega2.  quantize_rows keeps the first row of every voxel.  features / sem_labels / xyz / sampled_idx are copied
    from the source row: `xyz` is NOT rotated (as CoSMix's in-merge augmentation leaves it).  Returns the dict of the
    other merges plus `counts` = (base rows kept, sector rows, then the instance rows once per copy)."""
    scans = _check_scans(scan0, scan1)
    mask = instance_mask(instance_classes)
    d = draw_polarmix(rng, swap_prob, paste_prob) if draws is None else draws
    a = (float(np.cos(d["alpha"])), float(np.sin(d["alpha"])))
    copies = ((1.0, 0.0),) + tuple((float(np.cos(d[k])), float(np.sin(d[k]))) for k in ("omega1", "omega2"))
    dev = scan0["coordinates"].device

    def work():
        keep = _key_set(lambda s, band, i: not s) if d["swap"] else 0xFFFFFFFF
        take = _key_set(lambda s, band, i: s) if d["swap"] else 0
        paste = _key_set(lambda s, band, i: i) if d["paste"] else 0
        return _sensor_merge(scan0, scan1, d["source"], a, (-a[0], -a[1]), ((), ()), mask if d["paste"] else 0, keep,
                             take, paste, copies)

    return on_merge_stream(work, dev, [t for s in scans for t in s.values()])


# ------------------------------------------------------------------ SN (statistical normalisation): car-size scaling
# train_scaling_based.py:35-129 and utils/datasets/sn_scaling.py.  At start-up the car voxels (class 0) of 20 % of every
# dataset's scans are clustered (lidog_amd.cluster.dbscan in place of sklearn's DBSCAN) and the mean (width, height,
# length) of the car-shaped clusters gives one per-axis scale per (source, target) pair; every training item is then
# scaled and re-quantised.  `c -> float32(c) * float32(voxel)` is monotone, so the device returns integer boxes and
# counts and the host finishes the handful of floats with the reference's own numpy expressions: bit-equal by
# construction.  The reference's names are kept: "height" is the y extent, "l" the z extent of a cluster.

NUSCENES_NAME = "NuScenesDataset"      # the dataset name that switches get_average_dims to min_pts 2000, min_car_pts 300


def draw_scans(rng, n):
    """train_scaling_based.py:37-38: 20 % of the scans, drawn with replacement"""
    selected_idx = np.arange(n)
    return rng.choice(selected_idx, int(0.2 * selected_idx.shape[0]))


def sn_thresholds(name, min_pts=5000, min_car_pts=1000):
    """train_scaling_based.py:40-42"""
    return (2000, 300) if name == NUSCENES_NAME else (min_pts, min_car_pts)


def box_dims(counts, lo, hi, voxel_size, min_car_pts):
    """train_scaling_based.py:61-85 from the integer boxes of one scan's clusters (counts [k], lo / hi [k, 3]): the
    float32 rows [[width, height, length]] of the clusters of more than min_car_pts voxels that look like a car"""
    rows = []
    lo_f = torch.from_numpy(np.ascontiguousarray(lo, dtype=np.int32)) * voxel_size     # `coordinates * voxel_size`:
    hi_f = torch.from_numpy(np.ascontiguousarray(hi, dtype=np.int32)) * voxel_size     # an int tensor times a float
    lo_f, hi_f = lo_f.numpy(), hi_f.numpy()
    for c in range(len(counts)):
        if counts[c] > min_car_pts:
            w = hi_f[c, 0] - lo_f[c, 0]
            height = hi_f[c, 1] - lo_f[c, 1]
            l = hi_f[c, 2] - lo_f[c, 2]
            length = np.max([w, l])
            width = np.min([w, l])
            if 1 < width < 4 and 1 < height < 4 and 3 < length < 7:
                rows.append(np.array([width, height, length])[np.newaxis, ...])
    return rows


def mean_dims(rows):
    """train_scaling_based.py:87; no kept box: the ValueError np.concatenate raises on an empty list"""
    return np.mean(np.concatenate(rows, axis=0), axis=0)


def average_dims(dataset, rng=np.random, min_pts=5000, min_cluster_pts=50, min_car_pts=1000, car_class=0,
                 device="cuda", record=None):
    """get_average_dims (train_scaling_based.py:35-87) with the clustering on the GPU.  `dataset`: `len`, `name`,
    `voxel_size` and items with `coordinates` (int [n, 3]) and `sem_labels` ([n]), tensors or arrays anywhere (they are
    moved to `device`).  The scans are drawn on the host in the reference's sequence, so `np.random.seed(s)` selects
    the same scans; a scan is clustered only with MORE than min_pts car voxels, a cluster counts only with MORE than
    min_car_pts voxels (2000 / 300 for a dataset named 'NuScenesDataset'); min_cluster_pts is accepted and unused, as
    in the reference.  Returns the float32 mean [width, height, length] of the kept boxes; none kept: ValueError.
    `record`: a list that receives (scan, counts, lo, hi) of every clustered scan."""
    from . import cluster
    selected = draw_scans(rng, len(dataset))
    min_pts, min_car_pts = sn_thresholds(dataset.name, min_pts, min_car_pts)
    voxel = dataset.voxel_size
    dev = torch.device(device)
    rows = []

    def work(item):
        coords = torch.as_tensor(item["coordinates"]).to(dev)
        labels = torch.as_tensor(item["sem_labels"]).to(dev)
        car = torch.nonzero(labels == car_class).view(-1)
        if car.shape[0] <= min_pts:           # the shape is known to the host: torch.nonzero has read it
            return None
        car_pts = coords[car].to(torch.int32).contiguous()
        labels, k = cluster.dbscan_count(car_pts, voxel, eps=0.5, min_samples=10)
        counts, lo, hi = cluster.cluster_boxes(car_pts, labels, k)
        return [counts.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()]

    for s in selected:
        item = dataset[int(s)]
        if dev.type == "cuda":                # what comes back is host arrays: nothing to hand to the caller's stream
            side = merge_stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                boxes = work(item)
        else:
            boxes = work(item)
        if boxes is None:
            continue
        if record is not None:
            record.append((int(s), *boxes))
        rows += box_dims(*boxes, voxel, min_car_pts)
    return mean_dims(rows)


def scaling_params(sources, targets, cache_dir=None, **kw):
    """get_scaling_params (train_scaling_based.py:90-129): one float32 [n_targets, 3] array per source, target / source
    per component.  An entry of `sources` / `targets` is either the average dimensions of a dataset (an array of 3) or
    a dataset, whose average_dims(dataset, **kw) is then computed, sources first, and with `cache_dir` kept in
    `<cache_dir>/<dataset.name.lower()>.npy` as the reference keeps it in utils/datasets/_avg_sizes."""
    def dims(d):
        if isinstance(d, np.ndarray):
            return d
        if cache_dir is None:
            return average_dims(d, **kw)
        os.makedirs(cache_dir, exist_ok=True)
        path = os.path.join(cache_dir, d.name.lower() + ".npy")
        if not os.path.exists(path):
            np.save(path, average_dims(d, **kw))
        return np.load(path)

    source_avg_shape = [dims(d) for d in sources]
    target_avg_shape = [dims(d) for d in targets]
    scaling_set = []
    for s_avg_tmp in source_avg_shape:
        scaling_tmp = []
        for t_avg_tmp in target_avg_shape:
            scaling_tmp.append(np.array([t_avg_tmp[0] / s_avg_tmp[0], t_avg_tmp[1] / s_avg_tmp[1],
                                         t_avg_tmp[2] / s_avg_tmp[2]])[np.newaxis, ...])
        scaling_set.append(np.concatenate(scaling_tmp, axis=0))
    return scaling_set


def draw_scaling(rng, scaling_list, num_sources):
    """the scale rows of one item.  One source (SingleSNSourceDataset.__getitem__, sn_scaling.py:46-51):
    `len(self.scaling_list) > 1` tests the number of SOURCES, which is one, so the first target's row is always taken
    and nothing is drawn.  Two sources (MultiSNSourceDataset.merge_data, :124-131): one target row per source, drawn with
    np.random.choice, source 0 first."""
    if num_sources == 1:
        if len(scaling_list) > 1:
            return [scaling_list[rng.choice(np.arange(len(scaling_list)))][0]]
        return [scaling_list[0][0]]
    i0 = rng.choice(np.arange(scaling_list[0].shape[0]))
    i1 = rng.choice(np.arange(scaling_list[1].shape[0]))
    return [scaling_list[0][i0], scaling_list[1][i1]]


def sn_scale(scan, scaling, voxel_size=0.05, ignore_label=-1):
    """The item of SingleSNSourceDataset.__getitem__ (sn_scaling.py:36-71), one half of MultiSNSourceDataset.merge_data
    (:107-175): x = coordinates * voxel_size in float32, x[:, k] *= float32(scaling[k]) in float32, re-quantised at
    voxel_size; features and labels are those of the FIRST point of every voxel (the voted labels are discarded, as in
    mix3d_merge); xyz / sampled_idx / idx pass through untouched, as in the reference.  `scan`: dict of device tensors
    (coordinates int [n, 3], features [n, C], sem_labels [n]).  Returns the reference's dict plus `index`, the first
    point of every voxel.  `ignore_label` is the reference's argument; its label vote is discarded."""
    for k in ("coordinates", "features", "sem_labels"):
        if k not in scan:
            raise KeyError(f"scan has no '{k}'")
        _lib.require_gpu(scan[k], f"scan '{k}'")
    sc = np.asarray(scaling, dtype=np.float32).reshape(3)
    dev = scan["coordinates"].device

    def work():
        coords = scan["coordinates"].to(torch.int32).contiguous()
        n = coords.shape[0]
        x = torch.empty((n, 3), dtype=torch.float32, device=dev)
        call("lidog_sn_scale_coords", ptr(coords), n, float(np.float32(voxel_size)), float(sc[0]), float(sc[1]),
             float(sc[2]), ptr(x))
        q, index = sparse_quantize(x, quantization_size=voxel_size, return_index=True)
        out = {"coordinates": q, "features": scan["features"][index], "sem_labels": scan["sem_labels"][index]}
        for k in ("xyz", "idx", "sampled_idx"):
            if k in scan:
                out[k] = scan[k]
        out["index"] = index
        return out

    return on_merge_stream(work, dev, [t for t in scan.values()])


# ------------------------------------------------------------------ training augmentation: sub_p and augmentation_list
# With a non-null `augmentation_list` a training dataset's __getitem__ (semantickitti_bev.py:209-252, synth4d.py:141-162)
# draws int(sub_p * n) of the scan's points in random order, rotates and scales them (float64 from the rotation on),
# filters them by the bounds and the ego box (BEV datasets), and voxelises what is left: the first point of a voxel
# wins, so the random order matters.  The host makes the draws in the reference's sequence; lidog_augment_points does
# the per-point work and the existing hash / vote / BEV-label kernels the rest.  Device -> host reads per item: the
# number of rows the bounds filter kept (BEV form only: it sizes the hash table), then the number of voxels.

AUGMENTATIONS = ("RandomRotation", "RandomScale")
SCALE_RANGE = (0.9, 1.1)               # get_augmentations: RandomScale(0.9, 1.1)


def check_augmentations(augmentation_list):
    """get_augmentations (utils/common/augmentation.py:61-69): any list over RandomRotation / RandomScale, the empty
    one included; another name raises NotImplementedError"""
    names = list(augmentation_list)
    for a in names:
        if a not in AUGMENTATIONS:
            raise NotImplementedError(f"augmentation {a!r} (one of {AUGMENTATIONS})")
    return names


def rotation_matrix(axis, theta):
    """RandomRotation._M: expm(cross(eye(3), axis / norm(axis) * theta)), scipy's expm when scipy imports; otherwise the
    closed form of the same exponential (Rodrigues), which agrees with it to a few 1e-17"""
    axis = np.asarray(axis, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    try:
        from scipy.linalg import expm, norm
    except ImportError:
        v = axis / np.sqrt(np.sum(axis * axis)) * theta
        K = np.cross(np.eye(3), v)
        a = float(np.sqrt(np.sum(v * v)))
        if a == 0.0:
            return np.eye(3)
        return np.eye(3) + (np.sin(a) / a) * K + ((1.0 - np.cos(a)) / (a * a)) * (K @ K)
    return expm(np.cross(np.eye(3), axis / norm(axis) * theta))


def draw_ops(rng, augmentation_list):
    """the draws of one pass through the list, in order: RandomRotation's `rand(3)`, `rand(1)`, RandomScale's three
    `rand(1)` (utils/common/augmentation.py:12-34).  Returns [(name, float64 parameters)]: R [3, 3] for a rotation,
    [s_x, s_y, s_z] for a scale.  Shared by the items (draw_augmentation) and CoSMix's pasted classes (draw_classes)."""
    ops = []
    for a in check_augmentations(augmentation_list):
        if a == "RandomRotation":
            axis = rng.rand(3) - 0.5
            theta = np.pi / 4 * (rng.rand(1) - 0.5)
            ops.append((a, np.ascontiguousarray(rotation_matrix(axis, theta), dtype=np.float64)))
        else:
            scale, bias = SCALE_RANGE[1] - SCALE_RANGE[0], SCALE_RANGE[0]
            ops.append((a, np.concatenate([scale * rng.rand(1) + bias for _ in range(3)]).astype(np.float64)))
    return ops


def draw_augmentation(rng, n, sub_p, augmentation_list):
    """The draws of one training item in the reference's sequence (rng: a legacy RandomState or the np.random module):
    random_sample's `choice(arange(n), int(sub_p * n), replace=False)` (sub_p None: nothing drawn, every row in order),
    then per list entry RandomRotation's `rand(3)`, `rand(1)` or RandomScale's three `rand(1)`.  Returns
    {'sampled_idx': int64 [k], 'ops': [(name, float64 parameters)]}: R [3, 3] for a rotation, [s_x, s_y, s_z] for a
    scale."""
    names = check_augmentations(augmentation_list)
    n = int(n)
    sampled_idx = rng.choice(np.arange(n), int(sub_p * n), replace=False) if sub_p is not None else np.arange(n)
    return {"sampled_idx": np.asarray(sampled_idx, dtype=np.int64), "ops": draw_ops(rng, names)}


def augment_points(points, sampled_idx, ops, voxel_size=0.05, bounds=False, labels=None, batch=0):
    """lidog_augment_points: points float32 [n,3] and labels (int32 [n], optional) on the GPU, sampled_idx int32 [k] on
    the GPU or None (every row in order), ops as draw_augmentation returns them.  Returns (rows int32 [k,4], xyz [k,3]
    float64 with a rotation in the list, else float32, src int32 [k], labels int32 [k] or None, info int32 [2]) on the
    device; with `bounds` only the first info[0] rows are meaningful."""
    _lib.require_gpu(points, "points")
    dev = points.device
    if points.dtype != torch.float32 or not points.is_contiguous():
        raise ValueError("augment_points: points must be contiguous float32 [n, 3]")
    n = points.shape[0]
    k = n if sampled_idx is None else sampled_idx.shape[0]
    kinds = (ctypes.c_int32 * max(len(ops), 1))(*[AUGMENTATIONS.index(a) for a, _ in ops])
    params = np.zeros((max(len(ops), 1), 9), dtype=np.float64)
    for o, (a, p) in enumerate(ops):
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if p.shape[0] != (9 if a == "RandomRotation" else 3) or not np.all(np.isfinite(p)):
            raise ValueError(f"augment_points: parameters of {a}: {p}")
        params[o, :p.shape[0]] = p
    f64 = bool(_lib.load().lidog_augment_is_f64(kinds, len(ops)))
    q = np.broadcast_to(np.asarray(voxel_size, dtype=np.float64), (3,))
    rows = torch.empty((k, 4), dtype=torch.int32, device=dev)
    xyz = torch.empty((k, 3), dtype=torch.float64 if f64 else torch.float32, device=dev)
    src = torch.empty(k, dtype=torch.int32, device=dev)
    lab_out = torch.empty(k, dtype=torch.int32, device=dev) if labels is not None else None
    info = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().lidog_augment_ws(k), dtype=torch.int32, device=dev) if bounds else None
    call("lidog_augment_points", ptr(points), n, ptr(sampled_idx), k, kinds, params.ctypes.data, len(ops),
         1 if bounds else 0, float(q[0]), float(q[1]), float(q[2]), int(batch), ptr(labels), ptr(rows), ptr(xyz),
         ptr(src), ptr(lab_out), ptr(info), ptr(ws))
    return rows, xyz, src, lab_out, info


def augment_item(scan, draws, voxel_size=0.05, bounds=False, ignore_label=-1, bev=None, bev_from="voted"):
    """One augmented training item (semantickitti_bev.py:209-277 with `bounds`, synth4d.py:141-190 without) on the GPU.
    scan: dict of device tensors `points` float32 [n,3], `features` [n,C], `sem_labels` [n]; draws: what
    draw_augmentation returned.  Returns the reference's item: `coordinates` int32 [m,3], `xyz` [m,3] (the transformed
    first point of every voxel, float64 with a rotation in the list), `features`, `sem_labels` (the label of the voxel's
    FIRST point), `sampled_idx` (its row in the scan), `inverse_map`, plus `index` (its row among the kept rows) and
    `voted_labels` (the label vote of sparse_quantize).  bev=(bound, img_size): also `bev_labels` / `bev_selected_idx`
    [S, S] from the voted labels (semantickitti_bev.py:244-252, the default) or with bev_from='first' from the
    first-point labels (nuscenes_bev.py:252-261)."""
    for k in ("points", "features", "sem_labels"):
        if k not in scan:
            raise KeyError(f"scan has no '{k}'")
        _lib.require_gpu(scan[k], f"scan '{k}'")
    if bev_from not in ("voted", "first"):
        raise ValueError(f"bev_from = {bev_from!r} ('voted' or 'first')")
    points = scan["points"]
    n = points.shape[0]
    dev = points.device
    idx = np.asarray(draws["sampled_idx"])
    if idx.ndim != 1 or (idx.shape[0] and (int(idx.min()) < 0 or int(idx.max()) >= n)):
        raise ValueError("augment_item: sampled_idx outside the scan")
    ops = list(draws["ops"])

    def work():
        sampled = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)
        labels = scan["sem_labels"].to(torch.int32).contiguous()
        rows, xyz, src, lab, info = augment_points(points, sampled, ops, voxel_size, bounds, labels)
        if bounds:      # the hash table and every later launch are sized by the number of kept rows
            kept, bad = info.cpu().tolist()
            if bad:
                raise RuntimeError("augment_item: a sampled index outside the scan reached the device")
            rows, xyz, src, lab = rows[:kept], xyz[:kept], src[:kept], lab[:kept]
        _, voted, index, inverse = quantize_rows(rows, labels=lab, ignore_label=ignore_label, return_index=True,
                                                 return_inverse=True)
        first = src[index].long()
        out = {"coordinates": rows[index][:, 1:].contiguous(), "xyz": xyz[index], "features": scan["features"][first],
               "sem_labels": scan["sem_labels"][first], "sampled_idx": first, "inverse_map": inverse, "index": index,
               "voted_labels": voted.to(scan["sem_labels"].dtype)}
        if bev is not None:
            bound, img_size = bev
            img, pidx = bev_labels(rows[index].contiguous(), voted if bev_from == "voted" else lab[index], bound=bound,
                                   img_size=img_size, voxel=voxel_size, batch_size=1)
            out["bev_labels"], out["bev_selected_idx"] = img[0], pidx[0].long()
        return out

    return on_merge_stream(work, dev, [points, scan["features"], scan["sem_labels"]])


def collate_items(items, with_bev):
    """the batch of `items[b][s]`, the item (augment_item) of source s at batch position b: the keys of
    synth.make_batch; `source_bev_labels{s}` only with_bev.  Shared by lidog_amd.train.AugmentedSynthScans and
    lidog_amd.scans.FileScans."""
    batch = {}
    for s in range(len(items[0])):
        coords, feats, labels, bev = [], [], [], []
        for b, row in enumerate(items):
            m = row[s]
            c = m["coordinates"]
            coords.append(torch.cat([torch.full((c.shape[0], 1), b, dtype=torch.int32, device=c.device), c], dim=1))
            feats.append(m["features"])
            labels.append(m["sem_labels"].long())
            if with_bev:
                bev.append(m["bev_labels"])
        coords = torch.cat(coords)
        batch["coords_int1" if s else "coords_int"] = coords
        batch.update({f"source_coordinates{s}": coords.float(), f"source_features{s}": torch.cat(feats),
                      f"source_sem_labels{s}": torch.cat(labels)})
        if with_bev:
            batch[f"source_bev_labels{s}"] = {"block8": torch.stack(bev)}
    return batch


# ------------------------------------------------------------------ MixStyle (include/lidog_amd.h, csrc/mixstyle.hip)
MIXSTYLE_STAGES = ("block1", "block2", "block3", "block4")
MIXSTYLE_DEFAULT_STAGES = ("block1", "block2")


def check_mixstyle_arguments(layers, p=0.5, alpha=0.1):
    """the checks of the models, build_step / Fit and the command line; returns the stage names as a tuple"""
    layers = tuple(layers)
    for name in layers:
        if name not in MIXSTYLE_STAGES:
            raise ValueError(f"mixstyle stage {name!r}: one of {', '.join(MIXSTYLE_STAGES)}")
    if len(set(layers)) != len(layers):
        raise ValueError(f"mixstyle stages {list(layers)}: every stage once")
    if not (isinstance(p, (int, float)) and 0 <= p <= 1):           # a NaN fails the comparison
        raise ValueError(f"mixstyle_p {p}: a probability, 0 <= p <= 1")
    if not (isinstance(alpha, (int, float)) and 0 < alpha < float("inf")):
        raise ValueError(f"mixstyle_alpha {alpha}: the Beta distribution's parameter is positive and finite")
    return layers


def draw_mixstyle(rng, B, p=0.5, alpha=0.1):
    """The draws of one MixStyle call on a batch of B scans (rng: a legacy RandomState), in a fixed order:
    `random_sample()` -- the gate: a value >= p returns None and nothing more is drawn --, then `beta(alpha, alpha, B)`,
    then `permutation(B)`.  Returns (lam float32 [B], partner int32 [B]): scan b is mixed with scan partner[b]."""
    if rng.random_sample() >= p:
        return None
    lam = rng.beta(alpha, alpha, int(B))
    partner = rng.permutation(int(B))
    return np.asarray(lam, dtype=np.float32), np.asarray(partner, dtype=np.int32)
