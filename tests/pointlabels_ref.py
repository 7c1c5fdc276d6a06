"""A numpy restatement of the point-level path (lidog_amd.scans.keep_rows, lidog_amd.evaluate.point_labels;
csrc/pointlabels.hip): the float32 radius mask as numpy evaluates it, the keep index as a cumulative sum, the arg-max,
the two gathers and the confusion as a bincount.  tests/test_pointlabels_cpu.py pins it to hand-written cases;
tests/test_gpu_pointlabels.py and tests/test_gpu_eval_points.py hold the kernels to it.  Everything is integers or bit
patterns: comparisons are exact."""
import numpy as np

ERR_SCAN, ERR_LABEL, ERR_INVERSE, ERR_KEEP = 1, 2, 4, 8


def radius_mask_np(points, in_radius):
    """the reference's mask on a float32 [n, 3] array: every product and sum rounded to float32, a strict comparison"""
    p = np.asarray(points, dtype=np.float32)
    return np.sum(np.square(p), axis=1) < np.float32(in_radius) ** 2


def keep_rows_np(points_raw, stride, in_radius=None):
    """(keep_row int32 [n], kept count): the row of every record among the kept ones, -1 for a dropped record"""
    rec = np.ascontiguousarray(points_raw).reshape(-1).view(np.float32).reshape(-1, stride)
    with np.errstate(over="ignore", invalid="ignore"):
        keep = radius_mask_np(rec[:, :3], in_radius) if in_radius is not None else np.ones(rec.shape[0], bool)
    keep_row = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    return keep_row, int(keep.sum())


def argmax_np(logits):
    """the first maximal index; in a row holding a NaN the first NaN (numpy's argmax, torch's CPU max)"""
    x = np.asarray(logits, dtype=np.float32)
    return np.argmax(x, axis=1).astype(np.int64) if x.shape[0] else np.zeros(0, np.int64)


def map_labels_np(labels_raw, lut, mask=None):
    """(mapped int64 [n], bad bool [n]): numpy's `lut[raw & mask]`, where an IndexError would be raised `bad` is set"""
    idx = np.asarray(labels_raw).astype(np.int64).reshape(-1)
    if mask is not None:
        idx = idx & mask
    L = len(lut)
    idx = np.where(idx < 0, idx + L, idx)
    bad = (idx < 0) | (idx >= L)
    return np.where(bad, -1, np.asarray(lut, dtype=np.int64)[np.where(bad, 0, idx)]), bad


def point_labels_np(logits, row_off, kept_off, vox_off, keep_row, inverse_map, out_lut=None, fill=0, labels_raw=None,
                    lut=None, mask=None, ignore_label=-1):
    """(labels_out uint32 [N], counts int64 [B, C, C] or None, error word): out_lut[argmax(logits)[inverse_map[keep_row]]]
    per record, `fill` for a dropped one; counts = bincount of (label, prediction) over the kept records whose mapped
    label is a class other than ignore_label.  A value that cannot be used as an index (a keep_row outside the scan's
    kept rows, an inverse_map entry outside its voxel rows, a raw label outside the table) sets its bit; the record
    keeps `fill` and is not counted."""
    logits = np.asarray(logits, dtype=np.float32)
    c = logits.shape[1]
    pred = argmax_np(logits)
    out_lut = np.arange(c, dtype=np.int64) if out_lut is None else np.asarray(out_lut, dtype=np.int64)
    keep_row, inverse_map = np.asarray(keep_row, dtype=np.int64), np.asarray(inverse_map, dtype=np.int64)
    b, n = len(row_off) - 1, keep_row.shape[0]
    out = np.full(n, fill, dtype=np.uint32)
    counts = None
    err = 0
    mapped = bad = None
    if labels_raw is not None:
        counts = np.zeros((b, c, c), dtype=np.int64)
        mapped, bad = map_labels_np(labels_raw, lut, mask)
        if bad.any():
            err |= ERR_LABEL
    for s in range(b):
        rows = np.arange(row_off[s], row_off[s + 1])
        kr = keep_row[rows]
        nk, nv = kept_off[s + 1] - kept_off[s], vox_off[s + 1] - vox_off[s]
        wrong = (kr != -1) & ((kr < 0) | (kr >= nk))
        if wrong.any():
            err |= ERR_KEEP
        ok = (kr >= 0) & (kr < nk)
        v = np.full(rows.shape[0], -1, dtype=np.int64)
        v[ok] = inverse_map[kept_off[s] + kr[ok]]
        wrong = ok & ((v < 0) | (v >= nv))
        if wrong.any():
            err |= ERR_INVERSE
        ok &= (v >= 0) & (v < nv)
        if bad is not None:
            ok &= ~bad[rows]
        p = pred[vox_off[s] + v[ok]]
        out[rows[ok]] = out_lut[p].astype(np.uint32)
        if counts is not None:
            l = mapped[rows[ok]]
            sel = (l != ignore_label) & (l >= 0) & (l < c)
            counts[s] = np.bincount(l[sel] * c + p[sel], minlength=c * c).reshape(c, c)
    return out, counts, err


# ------------------------------------------------------------------ a tiny tree for the GPU tests
def write_tiny_kitti_tree(root, frames=3, rows=400):
    """a SemanticKITTI tree of `frames` files in sequence 08, `rows` records each: the leading rows of
    scans_ref.make_scan (shuffled: dense rows that share voxels, rows beyond 50 m, rows on the shell)"""
    import os

    import scans_ref as R
    _, g15 = R.load_g15()
    maps = R.fixture_maps(g15)
    keys, vals = maps["SemanticKITTI"]
    for d in ("velodyne", "labels"):
        os.makedirs(os.path.join(root, "sequences", "08", d), exist_ok=True)
    for f in range(frames):
        pts, cls, rng = R.make_scan(4000 + f)
        pts, cls = pts[:rows + 37 * f], cls[:rows + 37 * f]
        rec = np.concatenate([pts, rng.random((pts.shape[0], 1), dtype=np.float32)], axis=1).astype(np.float32)
        raw = R.raw_ids(rng, cls, keys, vals).astype(np.uint32) | (rng.integers(0, 1 << 16, cls.shape[0]).astype(np.uint32) << 16)
        rec.tofile(os.path.join(root, "sequences", "08", "velodyne", f"{f:06d}.bin"))
        raw.view(np.int32).tofile(os.path.join(root, "sequences", "08", "labels", f"{f:06d}.label"))
    # (the tree, its label map as a JSON file, the map's look-up table)
    return root, R.write_label_map_json(os.path.join(root, "kitti.json"), maps, "SemanticKITTI"), g15["lut_SemanticKITTI"]
