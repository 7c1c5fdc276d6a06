"""Evaluation path: forward-only inference and the reference's mIoU definition.

  test_step      utils/pipelines/trainer_lighting_bev.py:265-323  -- per-scan per-class Jaccard over ALL points
                 (sklearn.metrics.jaccard_score with labels 0..C-1, so points labelled -1 still enlarge the union
                 of the class they are predicted as), -1 for classes absent from the scan's labels
  test_epoch_end utils/pipelines/trainer_lighting_bev.py:325-383  -- -1 -> NaN, nan-mean over scans per class,
                 x100, nan-mean over classes
Everything stays on the device (the reference moves predictions to the CPU for sklearn).

eval_target (second half of this file): confusion / TargetEvaluator take the metric from logits to integer counts in
one HIP kernel (csrc/evalstats.hip) and read the counts once per target; iou_rows turns them into test_step's rows on
the host, per loader batch as the reference or per scan as evaluate() above.

Point level (third part): point_labels takes a batch's voxel logits back to every record of the scan files, in file order
(csrc/pointlabels.hip), with the per-scan confusion counts over the kept, labelled points; TargetEvaluator.run(points=...)
adds both to a target's evaluation, and the label-file helpers write what the SemanticKITTI API reads."""
import torch

from . import me as ME
from . import precision as _precision
from . import tta as _tta
from . import calibration as _calibration


def per_class_iou(preds, labels, num_classes=7, ignore_label=-1):
    """[C] IoU per class, -1 where the class does not occur in `labels`."""
    preds, labels = preds.long().view(-1), labels.long().view(-1)
    iou = torch.empty(num_classes, dtype=torch.float64, device=preds.device)
    cls = torch.arange(num_classes, device=preds.device).view(-1, 1)
    p, l = preds.view(1, -1) == cls, labels.view(1, -1) == cls
    inter = (p & l).sum(dim=1).double()
    union = (p | l).sum(dim=1).double()
    iou = torch.where(union > 0, inter / union.clamp(min=1), torch.zeros_like(inter))   # zero_division=0
    present = l.any(dim=1)
    return torch.where(present, iou, -torch.ones_like(iou))


def mean_iou(per_scan_iou):
    """[n_scans, C] with -1 for absent classes -> (per-class IoU in percent, mean IoU), NaN-aware"""
    x = per_scan_iou.clone().double()
    x[x == -1] = float("nan")
    per_class = torch.nanmean(x, dim=0) * 100
    return per_class, torch.nanmean(per_class)


@torch.no_grad()
def predict(model, coords, feats, manager=None, precision=None, kernels=None):
    """validation / test forward: is_train=False (no BEV head, running BN statistics), arg-max class per voxel.
    `precision`: None (whatever is current: fp32 unless the caller opened lidog_amd.precision.bf16_inference), "fp32" or
    "bf16" (the eligible convolutions on the bf16 kernels; `kernels`: a precision.Bf16Kernels of the model packed
    earlier, else the weights are packed in this call); anything else is a ValueError before any launch.
    After the first call the coordinate maps of a batch are built in one go from the recorded trace of map uses
    (ME.CoordinateManager.prepare: one host synchronisation instead of one per kernel map); `manager`: a manager
    prepared ahead of time for these coordinates (Predictor / evaluate() build the next batch's while the current
    forward pass runs)."""
    out = _forward(model, coords, feats, manager, precision, kernels)
    return out.F.max(dim=1)[1], out.F


def _forward(model, coords, feats, manager=None, precision=None, kernels=None):
    """predict()'s forward pass; returns the model's output SparseTensor (the stride-1 logits on the batch's manager)"""
    scope = _precision.scope(model, precision, kernels)
    was_training = model.training
    model.eval()
    trace = getattr(model, "_lidog_eval_trace", None)
    if manager is None and trace is not None:
        manager = ME.CoordinateManager.prepare(coords, trace)
    if manager is not None:
        st = ME.SparseTensor(features=feats, coordinates=coords, coordinate_manager=manager)
    else:
        st = ME.SparseTensor(coordinates=coords, features=feats)
    with scope:
        out = model(st)
    model._lidog_eval_trace = st.coordinate_manager.trace
    model.train(was_training)
    return out[0] if isinstance(out, tuple) else out


class Predictor:
    """predict() over a stream of batches with the NEXT batch's coordinate maps built on the side stream while
    the current forward pass runs: p = Predictor(model); preds, logits = p(coords, feats, next_coords).
    `precision="bf16"`: the weights are packed ONCE, here (`kernels`, a precision.Bf16Kernels); call kernels.refresh()
    after changing the weights."""

    def __init__(self, model, precision=None):
        self.model, self._next, self.precision = model, None, precision
        self.output = None      # the last call's output SparseTensor (point_logits interpolates on its map)
        self.kernels = _precision.Bf16Kernels(model) if _precision.resolve(precision) else None

    def __call__(self, coords, feats, next_coords=None):
        mgr = None
        if self._next is not None and self._next[0] is coords:
            mgr = self._next[1]
        self._next = None
        # the next batch's coordinates are valid NOW: its maps only wait for what is queued so far, not for the
        # forward pass that is about to be launched
        ready = torch.cuda.Event()
        ready.record()
        self.output = _forward(self.model, coords, feats, mgr, self.precision, self.kernels)
        out = (self.output.F.max(dim=1)[1], self.output.F)
        trace = getattr(self.model, "_lidog_eval_trace", None)
        if next_coords is not None and trace is not None:
            self._next = (next_coords, ME.CoordinateManager.prepare(next_coords, trace, ready))
        return out


@torch.no_grad()
def evaluate(model, batches, num_classes=7, ignore_label=-1, precision=None):
    """batches: iterable of dicts with coords_int [N,4], source_features0, source_sem_labels0; one IoU row per SCAN.
    (The reference's eval_target.py builds its loaders with batch_size * 2 and test_step computes one row per loader
    batch: that table is TargetEvaluator's rows="batch"; rows="scan" gives this function's.)"""
    rows = []
    run = Predictor(model, precision)
    batches = list(batches)
    for i, b in enumerate(batches):
        coords = b["coords_int"]
        nxt = batches[i + 1]["coords_int"] if i + 1 < len(batches) else None
        preds, _ = run(coords, b["source_features0"], nxt)
        labels = b["source_sem_labels0"]
        for s in range(int(coords[:, 0].max().item()) + 1):
            sel = coords[:, 0] == s
            rows.append(per_class_iou(preds[sel], labels[sel], num_classes, ignore_label))
    return mean_iou(torch.stack(rows))


def write_results_csv(save_dir, source_names, target_name, per_scan_iou, class_names, first_target=True,
                      file_targets=None):
    """The result file of test_epoch_end (utils/pipelines/trainer_lighting_bev.py:325-383):
    `<save_dir>/results/<source>-TO-<target>.csv`, appended; header `source,target,<class names>,mean` before the first
    target's row; per-class IoU = nan-mean over scans (-1 = class absent from the scan) x 100, rounded to 2 decimals with a
    decimal COMMA, last column the nan-mean over classes.  `per_scan_iou`: [n_scans, C] as returned by per_class_iou;
    `class_names`: the C names (the reference takes `training_dataset.class2names[1:]`).  `file_targets`: the target
    part of the file name when it is not this row's target: with two targets the reference names the file after both,
    concatenated, and each row after its own (trainer_lighting.py:264-313).  Returns the path."""
    import csv
    import os
    import numpy as np
    os.makedirs(os.path.join(save_dir, "results"), exist_ok=True)
    path = os.path.join(save_dir, "results",
                        f"{source_names}-TO-{target_name if file_targets is None else file_targets}.csv")
    if not torch.is_tensor(per_scan_iou):
        per_scan_iou = torch.from_numpy(np.asarray(per_scan_iou, dtype=np.float64))
    x = per_scan_iou.detach().double().cpu().numpy().copy()
    x[x == -1] = np.nan
    per_class = np.nanmean(x, axis=0) * 100
    average = np.nanmean(per_class, axis=0)
    with open(path, "a") as f:
        w = csv.writer(f)
        if first_target:
            w.writerow(["source", "target"] + list(class_names) + ["mean"])
        w.writerow([source_names, target_name] + [str(round(p, 2)).replace(".", ",") for p in per_class] +
                   [str(round(float(average), 2)).replace(".", ",")])
    return path


# ---------------------------------------------------------------------------------------------------------------------
# eval_target: the metric from logits to integer counts on the device (csrc/evalstats.hip), the IoU rows on the host
# ---------------------------------------------------------------------------------------------------------------------
MAX_CLASSES = 32

# class2names[1:] of the reference's common label space, and the colours of the prediction dump: PALETTE[0] is the
# ignore label's, a class takes PALETTE[class + 1] (as the reference indexes its color_map).  The colours are this
# project's own.
CLASS_NAMES = ("vehicle", "person", "road", "sidewalk", "terrain", "manmade", "vegetation")
PALETTE = ((0, 0, 0), (30, 120, 255), (255, 40, 40), (200, 60, 200), (90, 30, 150), (150, 240, 80), (255, 200, 0),
           (0, 160, 60))


def palette(num_classes=7):
    """[num_classes + 1, 3] uint8: PALETTE, extended deterministically past 7 classes"""
    import numpy as np
    p = [PALETTE[i] if i < len(PALETTE) else ((53 * i) % 256, (97 * i + 80) % 256, (193 * i + 160) % 256)
         for i in range(num_classes + 1)]
    return np.asarray(p, dtype=np.uint8)


def check_scan_error(err, what="confusion"):
    """raises when a kernel met a batch index outside [0, n_scans) (one read of a device word)"""
    if int(err.item()) != 0:
        raise ValueError(f"{what}: a row's batch index lies outside [0, n_scans); such rows were not counted")


def confusion(logits, labels, coords, n_scans, out=None, ignore_label=-1, err=None):
    """(preds [N] int64, counts [n_scans, C + 1, C] int64) of lidog_eval_confusion, on the device: preds = torch's CPU
    `logits.max(dim=1)[1]`; counts[scan, label + 1, pred], row 0 for every label outside 0..C-1 and the ignore label.
    `out`: counts to ADD to (a contiguous [n_scans, C + 1, C] int64 tensor or slice of one).  `err`: an int32 [1] device
    word the caller checks later with check_scan_error (nothing is read back here); without it this call checks, which
    costs one synchronisation."""
    from ._lib import call, ptr, require_gpu
    require_gpu(logits, "logits")
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError(f"confusion: logits must be float32 [N, C], got {logits.dtype} {tuple(logits.shape)}")
    n, c = logits.shape
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError(f"confusion: {c} classes (at most {MAX_CLASSES})")
    if labels.shape != (n,) or labels.dtype != torch.int64:
        raise ValueError(f"confusion: labels must be int64 [{n}], got {labels.dtype} {tuple(labels.shape)}")
    if coords.shape != (n, 4) or coords.dtype != torch.int32:
        raise ValueError(f"confusion: coords must be int32 [{n}, 4], got {coords.dtype} {tuple(coords.shape)}")
    n_scans = int(n_scans)
    if out is None:
        out = torch.zeros((n_scans, c + 1, c), dtype=torch.int64, device=logits.device)
    elif out.shape != (n_scans, c + 1, c) or out.dtype != torch.int64 or not out.is_contiguous() or \
            out.device != logits.device:
        raise ValueError(f"confusion: out must be a contiguous int64 [{n_scans}, {c + 1}, {c}] tensor on {logits.device}")
    own_err = err is None
    if own_err:
        err = torch.zeros(1, dtype=torch.int32, device=logits.device)
    preds = torch.empty(n, dtype=torch.int64, device=logits.device)
    call("lidog_eval_confusion", ptr(logits.contiguous()), ptr(labels.contiguous()), ptr(coords.contiguous()), n, c,
         n_scans, int(ignore_label), ptr(preds), ptr(out), ptr(err))
    if own_err:
        check_scan_error(err)
    return preds, out


def pack_predictions(coords, preds, labels, n_scans, ignore_label=-1, err=None):
    """The prediction dump of test_step as ONE int32 device buffer (lidog_eval_pack): buf[s] = first record of scan s,
    buf[n_scans] = number of records, then [records, 5] = (x, y, z, prediction, label) of the rows with label !=
    ignore_label, grouped by scan in ascending row order.  unpack_predictions splits the host copy."""
    from . import _lib
    from ._lib import call, ptr, require_gpu
    require_gpu(coords, "coords")
    n, n_scans = coords.shape[0], int(n_scans)
    dev = coords.device
    own_err = err is None
    if own_err:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    buf = torch.empty(n_scans + 1 + 5 * n, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().lidog_eval_pack_ws(n, n_scans), dtype=torch.int32, device=dev)
    call("lidog_eval_pack", ptr(coords.contiguous()), ptr(preds.contiguous()), ptr(labels.contiguous()), n, n_scans,
         int(ignore_label), ptr(buf), ptr(err), ptr(ws))
    if own_err:
        check_scan_error(err, "pack_predictions")
    return buf


def unpack_predictions(buf, n_scans):
    """host copy of pack_predictions' buffer (the one copy of a batch) -> list of [k_s, 5] int32 arrays, one per scan"""
    host = buf.cpu().numpy()
    start = host[:n_scans + 1]
    rec = host[n_scans + 1:n_scans + 1 + 5 * int(start[n_scans])].reshape(-1, 5)
    return [rec[start[s]:start[s + 1]] for s in range(n_scans)]


# ------------------------------------------------------------------ point level: one label per record of a scan file
MAX_POINT_SCANS = 64      # of one point_labels call: the scans' offsets travel with the launch
POINT_ERRORS = ((1, "a file row outside every scan's range of rows"),
                (2, "a raw label outside the label map's table"),
                (4, "an inverse_map entry outside its scan's voxel rows"),
                (8, "a keep_row entry outside its scan's kept rows"))


def check_point_error(err, what="point_labels"):
    """raises when lidog_point_labels set a bit of its error word (one read of a device word)"""
    e = int(err.item())
    if e:
        raise ValueError(f"{what}: " + "; ".join(m for b, m in POINT_ERRORS if e & b) +
                         f" (error word {e}); such records keep the fill id and were not counted")


def _offsets(name, off, n_scans, total, what):
    import numpy as np
    o = np.asarray(off, dtype=np.int64).reshape(-1)
    if o.shape[0] != n_scans + 1 or o[0] != 0 or (np.diff(o) < 0).any() or int(o[-1]) != total:
        raise ValueError(f"point_labels: {name} must hold {n_scans + 1} non-decreasing offsets from 0 to the {total} "
                         f"{what}, got {o.tolist()}")
    return o


def point_labels(logits, row_off, kept_off, vox_off, keep_row, inverse_map, out_lut=None, fill=0, labels_raw=None,
                 lut=None, label_mask=None, ignore_label=-1, counts=None, err=None):
    """(labels_out uint32 [N], counts) of lidog_point_labels, on the device: one id per record of every file of a loader
    batch, in file order.  logits float32 [V, C]: the batch's voxel rows, scan after scan; row_off / kept_off / vox_off:
    B + 1 host integers each (B <= 64; they travel with the launch, no copy is queued), where every scan's file rows,
    kept rows (load_scan's output) and voxel rows start;
    keep_row int32 [N] (scans.keep_rows of every file, concatenated); inverse_map int64 or int32 [kept] (kept row ->
    voxel row within its item).  labels_out = out_lut[arg-max of the record's voxel] (out_lut int32 [C] on the device,
    None: the class itself), `fill` for a record the radius mask dropped.  The arg-max is confusion()'s: the first
    maximal index, the first NaN.
    labels_raw (int32 or uint8 [N], the files' label words concatenated) with lut / label_mask as scans.load_scan takes
    them: counts [B, C, C] int64 (`counts`: a contiguous tensor or slice to ADD to, else zeros) += the confusion (label,
    prediction) over the kept records whose mapped label is a class other than ignore_label; without labels_raw the
    counts are returned as given.  `err`: an int32 [1] device word the caller checks later with check_point_error
    (nothing is read back here); without it this call checks, which costs one synchronisation."""
    import numpy as np
    from . import _lib
    from ._lib import call, ptr, require_gpu
    require_gpu(logits, "logits")
    dev = logits.device
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError(f"point_labels: logits must be float32 [V, C], got {logits.dtype} {tuple(logits.shape)}")
    v, c = logits.shape
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError(f"point_labels: {c} classes (at most {MAX_CLASSES})")
    for name, t, dtypes in (("keep_row", keep_row, (torch.int32,)), ("inverse_map", inverse_map, (torch.int32, torch.int64))):
        require_gpu(t, name)
        if t.dim() != 1 or t.dtype not in dtypes or t.device != dev:
            raise ValueError(f"point_labels: {name} must be a 1-d {' or '.join(str(d) for d in dtypes)} tensor on {dev}, "
                             f"got {t.dtype} {tuple(t.shape)} on {t.device}")
    n, kept = keep_row.shape[0], inverse_map.shape[0]
    b = len(row_off) - 1
    if not 1 <= b <= MAX_POINT_SCANS:
        raise ValueError(f"point_labels: {b} scans (1..{MAX_POINT_SCANS})")
    offs = np.stack([_offsets("row_off", row_off, b, n, "file rows"), _offsets("kept_off", kept_off, b, kept, "kept rows"),
                     _offsets("vox_off", vox_off, b, v, "voxel rows")])
    if out_lut is None:
        out_lut = torch.arange(c, dtype=torch.int32, device=dev)
    require_gpu(out_lut, "out_lut")
    if out_lut.shape != (c,) or out_lut.dtype != torch.int32 or out_lut.device != dev:
        raise ValueError(f"point_labels: out_lut must be int32 [{c}] on {dev}")
    fill = int(fill)
    if not 0 <= fill < 2 ** 32:
        raise ValueError(f"point_labels: fill = {fill} is no uint32")
    kind, mask = 0, -1
    if labels_raw is not None:
        require_gpu(labels_raw, "labels_raw")
        kinds = {torch.int32: 1, torch.uint8: 2}
        if labels_raw.dtype not in kinds or labels_raw.shape != (n,) or labels_raw.device != dev:
            raise ValueError(f"point_labels: labels_raw must be int32 or uint8 [{n}] on {dev}, got {labels_raw.dtype} "
                             f"{tuple(labels_raw.shape)}")
        kind = kinds[labels_raw.dtype]
        if lut is None or not lut.is_cuda or lut.dtype != torch.int32 or lut.dim() != 1 or lut.shape[0] < 1:
            raise ValueError("point_labels: lut must be a non-empty int32 [L] tensor on the GPU")
        if label_mask is not None:
            mask = int(np.array(label_mask, dtype=np.uint32).astype(np.int32))
        if counts is None:
            counts = torch.zeros((b, c, c), dtype=torch.int64, device=dev)
        elif counts.shape != (b, c, c) or counts.dtype != torch.int64 or not counts.is_contiguous() or \
                counts.device != dev:
            raise ValueError(f"point_labels: counts must be a contiguous int64 [{b}, {c}, {c}] tensor on {dev}")
    own_err = err is None
    if own_err:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(n, dtype=torch.uint32, device=dev)
    ws = torch.empty(_lib.load().lidog_point_labels_ws(v), dtype=torch.int32, device=dev)
    call("lidog_point_labels", ptr(logits.contiguous()), v, c, b, offs[0].ctypes.data, offs[1].ctypes.data, offs[2].ctypes.data, n, kept,
         ptr(keep_row.contiguous()), ptr(inverse_map.long().contiguous()), ptr(out_lut.contiguous()), fill,
         ptr(labels_raw.contiguous()) if kind else None, kind, mask, ptr(lut.contiguous()) if kind else None,
         lut.shape[0] if kind else 0, int(ignore_label), ptr(out), ptr(counts) if kind else None, ptr(err), ptr(ws))
    if own_err:
        check_point_error(err)
    return out, counts


POINT_INTERP = ("nearest", "trilinear")


def point_queries(items):
    """float32 [kept, 4] rows (scan's position in the batch, x, y, z): the kept points of every scan of a loader batch
    (FileScans.point_item's `points`, load_scan's output) divided by the voxel size in the float32 true division the
    voxeliser uses, so the floor of a query is the voxel its point was put into.  An item that cannot supply one such
    query per kept row (not a FileScans validation item, an augmented one, or one whose rows were cut to the BEV bounds)
    is a ValueError."""
    import numpy as np
    out = []
    for b, it in enumerate(items):
        pts = it.get("points")
        if pts is None or not it.get("plain", False) or pts.shape[0] != it["kept"] or \
                it["inverse_map"].shape[0] != pts.shape[0]:
            raise ValueError(f"{it.get('path', f'scan {b}')}: trilinear point labels need one query per kept row: a "
                             "FileScans validation item without augmentations and without the BEV bounds cut "
                             "(use interp='nearest' for this dataset)")
        q = np.broadcast_to(np.asarray(it["voxel_size"], dtype=np.float64), (3,)).astype(np.float32)
        rows = torch.empty((pts.shape[0], 4), dtype=torch.float32, device=pts.device)
        rows[:, 0] = float(b)
        rows[:, 1:] = pts / torch.from_numpy(q).to(pts.device)        # tensor / tensor: a true division per element
        out.append(rows)
    return torch.cat(out) if out else None


def point_logits(logits, items, err=None):
    """float32 [kept, C]: the stride-1 logits of a loader batch (`logits`: the model's output ME.SparseTensor)
    interpolated trilinearly at its kept points (point_queries of the batch's point_item dicts, scan after scan).
    Missing neighbours add nothing; `err` as SparseTensor.features_at_coordinates takes it."""
    return logits.features_at_coordinates(point_queries(items), err=err)


def point_inputs(items, with_labels=True):
    """The arguments of point_labels for a loader batch from its scans' FileScans.point_item dicts, in batch order: the
    keep index of every file (scans.keep_rows, on the words already uploaded) and the concatenations.  Nothing is read
    back: every offset is a size the host already knows.  A dict of row_off, kept_off, vox_off, keep_row, inverse_map,
    labels_raw, lut, label_mask; labels_raw is None unless with_labels, and a file without labels is a ValueError then."""
    import numpy as np
    from . import scans as _scans
    if not items:
        raise ValueError("point_inputs: no scans")
    keep = [_scans.keep_rows(it["points_raw"], it["stride"], it["in_radius"], name=it["path"])[0] for it in items]
    out = {"row_off": np.concatenate([[0], np.cumsum([it["rows"] for it in items])]).astype(np.int64),
           "kept_off": np.concatenate([[0], np.cumsum([it["kept"] for it in items])]).astype(np.int64),
           "vox_off": np.concatenate([[0], np.cumsum([it["voxels"] for it in items])]).astype(np.int64),
           "keep_row": torch.cat(keep), "inverse_map": torch.cat([it["inverse_map"] for it in items]),
           "labels_raw": None, "lut": None, "label_mask": None}
    if with_labels:
        missing = [it["path"] for it in items if it["labels_raw"] is None]
        if missing:
            raise ValueError(f"{missing[0]}: no label file, so no point-level confusion (labels can still be saved)")
        if len({(it["labels_raw"].dtype, it["mask"], it["lut"].data_ptr()) for it in items}) != 1:
            raise ValueError("point_inputs: the scans of a batch must share label dtype, mask and look-up table")
        out.update(labels_raw=torch.cat([it["labels_raw"] for it in items]), lut=items[0]["lut"],
                   label_mask=items[0]["mask"])
    return out


class PointPath:
    """What TargetEvaluator.run(points=...) needs for the point level.  `items(ids)`: the FileScans.point_item dicts of a
    batch's dataset indices (the dataset has `keep_raw` set); `out_lut`: int32 [C] class -> id to write (None: the class
    itself) and `fill`: the id of records beyond the radius; `with_labels`: count the point confusion (needs every
    file's labels); `on_point_labels(first_scan, labels_out, row_off)`: called per batch with the dataset index of its
    first scan, the host copy of its ids (numpy uint32, file order) and the B + 1 row offsets of its scans; asking for it
    costs one device -> host copy per batch.  `interp`: "nearest" (every point takes its voxel's class) or "trilinear" (the
    class of the logits interpolated at the point's own position between the voxels, point_logits).  `tta`: a list of
    view names or tta.View objects (lidog_amd.tta.parse_views; None or empty: nothing changes): the model also runs over
    every view of a batch and a point takes the arg-max of its accumulated scores, `tta_mode` "prob" (softmax),
    "logit" or "vote" (one-hot of every view's arg-max); nearest only."""

    def __init__(self, items, out_lut=None, fill=0, with_labels=True, on_point_labels=None, interp="nearest", tta=None,
                 tta_mode="prob"):
        if interp not in POINT_INTERP:
            raise ValueError(f"PointPath: interp={interp!r} (one of {', '.join(POINT_INTERP)})")
        if tta_mode not in _tta.MODES:
            raise ValueError(f"PointPath: tta_mode={tta_mode!r} (one of {', '.join(_tta.MODES)})")
        self.interp, self.tta_mode = interp, tta_mode
        self.tta = _tta.parse_views(tta) if tta is not None and len(tta) else None       # the identity first
        if self.tta is not None and interp == "trilinear":
            raise ValueError("PointPath: tta with interp='trilinear' (every view would need its own interpolation; "
                             "test-time augmentation is nearest only)")
        self.items, self.out_lut, self.fill = items, out_lut, int(fill)
        self.with_labels, self.on_point_labels = bool(with_labels), on_point_labels

    @classmethod
    def of(cls, data, device="cuda", **kw):
        """over a scans.FileScans validation dataset, which from here on keeps the uploaded files of the items it makes"""
        data.keep_raw = True
        return cls(lambda ids: [data.point_item(i, device) for i in ids], **kw)


def point_iou_counts(point_counts):
    """[n, C, C] point confusion -> the [n, C + 1, C] layout iou_rows takes; row 0 (labels outside the classes) stays
    empty: the point level leaves unlabelled points out altogether"""
    import numpy as np
    m = np.asarray(point_counts, dtype=np.int64)
    return np.concatenate([np.zeros((m.shape[0], 1, m.shape[2]), np.int64), m], axis=1)


def iou_rows(counts, rows="batch", batch_of_scan=None):
    """IoU rows of test_step from confusion counts [n_scans, C + 1, C], on the host in float64.  Per row and class:
    tp / (true + pred - tp) as one division, 0 where the denominator is 0, -1 where the class is absent from the row's
    labels: sklearn's jaccard_score(preds, labels, average=None, labels=arange(C), zero_division=0.) followed by
    test_step's masking; a point labelled -1 still enlarges the union of the class it is predicted as.
    rows="batch": the counts of a loader batch's scans are summed first, one row per batch, as the reference, whose
    test_step sees a whole batch (eval_target.py:162-167 builds the loaders with batch_size * 2); `batch_of_scan`
    [n_scans] gives every scan's batch (non-decreasing; None: all scans are one batch).  rows="scan": one row per scan,
    what evaluate() computes."""
    import numpy as np
    m = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    m = m.astype(np.int64)
    if m.ndim != 3 or m.shape[1] != m.shape[2] + 1:
        raise ValueError(f"iou_rows: counts must be [n_scans, C + 1, C], got {m.shape}")
    if rows == "batch":
        b = np.zeros(m.shape[0], np.int64) if batch_of_scan is None else np.asarray(batch_of_scan, dtype=np.int64)
        if b.shape != (m.shape[0],):
            raise ValueError(f"iou_rows: batch_of_scan must hold {m.shape[0]} entries")
        ids = np.unique(b)
        m = np.stack([m[b == i].sum(axis=0) for i in ids]) if m.shape[0] else m
    elif rows != "scan":
        raise ValueError(f"iou_rows: rows={rows!r} (one of 'batch', 'scan')")
    c = m.shape[2]
    tp = m[:, 1:, :][:, np.arange(c), np.arange(c)]
    true = m[:, 1:, :].sum(axis=2)
    pred = m.sum(axis=1)
    den = true + pred - tp
    iou = np.where(den > 0, tp.astype(np.float64) / np.where(den > 0, den, 1).astype(np.float64), 0.0)
    return np.where(true > 0, iou, -1.0)


def mean_iou_rows(rows):
    """test_epoch_end's arithmetic on the host: -1 -> NaN, nan-mean over rows x 100, nan-mean over classes"""
    import warnings
    import numpy as np
    x = np.array(rows, dtype=np.float64)
    x[x == -1] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # a class absent from every row: NaN, as the reference
        per_class = np.nanmean(x, axis=0) * 100
        return per_class, float(np.nanmean(per_class, axis=0))


def dataset_batches(data, batch_size, device="cuda"):
    """(batch, scan indices) over a dataset in order, as an unshuffled DataLoader: the last batch may be short"""
    for i in range(0, len(data), batch_size):
        ids = list(range(i, min(i + batch_size, len(data))))
        yield data.batch(ids, device), ids


class TargetEvaluator:
    """The loop of trainer.test over one target: Predictor with the next batch's coordinate maps in flight, the metric
    of every batch added by lidog_eval_confusion into ONE preallocated [n_scans_total, C + 1, C] tensor.  Nothing is read
    from the device per batch unless predictions are saved; the counts (and the error word) cross to the host once, at
    the end.  A batch's scan count is the number of its dataset indices.

        ev = TargetEvaluator(model)
        res = ev.run(dataset_batches(data, 8), n_scans=len(data))          # rows="batch": the reference's table
    `on_predictions(index, records)`: called per scan with its [k, 5] int32 records (x, y, z, prediction, label) of the
    labelled voxels; asking for it costs one device -> host copy per batch."""

    def __init__(self, model, num_classes=7, ignore_label=-1, precision=None, adapter=None):
        """`precision`: None / "fp32" / "bf16" as predict(); with "bf16" every run() packs the weights once (`kernels`
        holds the last run's table).  `adapter`: a lidog_amd.adapt.TestTimeAdapter of `model` that run() calls in place
        of its Predictor (test-time adaptation: fp32 only, and no test-time augmentation next to it); None changes
        nothing."""
        if adapter is not None and _precision.resolve(precision):
            raise ValueError("TargetEvaluator: precision='bf16' with an adapter (test-time adaptation is fp32 only)")
        _precision.resolve(precision)
        self.model, self.num_classes, self.ignore_label = model, int(num_classes), int(ignore_label)
        self.precision, self.kernels, self.adapter = precision, None, adapter

    @torch.no_grad()
    def run(self, batches, n_scans, rows="batch", on_predictions=None, points=None, calibration=None, calib_bins=15):
        """`batches`: iterable of (batch dict, scan indices); `n_scans`: scans of all batches together.  Returns a dict:
        counts [n_scans, C + 1, C] (numpy), batch_of_scan, rows (IoU rows), per_class (percent), mean, scans.
        `points` (a PointPath; None changes nothing): every batch's logits also go through point_labels; the dict then
        carries point_counts [n_scans, C, C], point_rows / point_per_class / point_mean (iou_rows / mean_iou_rows with
        the same `rows`), and points.on_point_labels sees every batch's ids.  The point counts and their error word
        cross to the host at the end, with the voxel ones.  With points.tta every batch is also run once per further
        view and the point level takes the accumulated scores (_vote); the voxel-level counts and `on_predictions` stay
        view 0's, and the dict gains tta_views (the names, identity first) and tta_mode.
        `calibration` (None builds nothing and launches nothing): a list of (name, beta) entries, beta None for the raw
        softmax or an inverse temperature as calibration.CalibrationTable.add takes it; every batch's voxel logits (an
        adapter's: those it returns for the batch) go into one CalibrationTable of `calib_bins` bins per entry, one
        launch each, and the dict gains calibration = {name: calibration.metrics_from_table(...)}.  The tables cross to
        the host at the end, with the counts."""
        import numpy as np
        if rows not in ("batch", "scan"):
            raise ValueError(f"rows={rows!r} (one of 'batch', 'scan')")
        c = self.num_classes
        if self.adapter is not None and points is not None and points.tta is not None:
            raise ValueError("TargetEvaluator: an adapter with points.tta (the further views would not be adapted)")
        run = self.adapter if self.adapter is not None else Predictor(self.model, self.precision)
        self.kernels = run.kernels
        it = iter(batches)
        cur = next(it, None)
        counts = err = pcounts = perr = ferr = terr = None
        tables = None
        if calibration is not None:
            calibration = [(str(name), beta) for name, beta in calibration]
            if len({name for name, _ in calibration}) != len(calibration):
                raise ValueError("TargetEvaluator: two calibration entries share a name")
        batch_of_scan = []
        done = 0
        nb = 0
        while cur is not None:
            nxt = next(it, None)
            b, ids = cur
            coords = b["coords_int"]
            if counts is None:
                counts = torch.zeros((int(n_scans), c + 1, c), dtype=torch.int64, device=coords.device)
                err = torch.zeros(1, dtype=torch.int32, device=coords.device)
                if points is not None:
                    pcounts = torch.zeros((int(n_scans), c, c), dtype=torch.int64, device=coords.device)
                    perr = torch.zeros(1, dtype=torch.int32, device=coords.device)
                    ferr = torch.zeros(1, dtype=torch.int32, device=coords.device)
                    terr = torch.zeros(1, dtype=torch.int32, device=coords.device)
                if calibration is not None:
                    tables = [_calibration.CalibrationTable(calib_bins, coords.device) for _ in calibration]
            k = len(ids)
            if done + k > counts.shape[0]:
                raise ValueError(f"TargetEvaluator: more than n_scans = {n_scans} scans in the batches")
            _, logits = run(coords, b["source_features0"], nxt[0]["coords_int"] if nxt is not None else None)
            labels = b["source_sem_labels0"]
            preds, _ = confusion(logits, labels, coords, k, out=counts[done:done + k], ignore_label=self.ignore_label,
                                 err=err)
            if tables is not None:
                for table, (_, beta) in zip(tables, calibration):
                    table.add(logits, labels, beta=beta, ignore_label=self.ignore_label)
            if on_predictions is not None:
                buf = pack_predictions(coords, preds, labels, k, self.ignore_label, err=err)
                for idx, rec in zip(ids, unpack_predictions(buf, k)):
                    on_predictions(idx, rec)
            if points is not None:
                items = points.items(ids)
                pin = point_inputs(items, points.with_labels)
                plogits, vox_off, inverse = logits, pin["vox_off"], pin["inverse_map"]
                if points.interp == "trilinear" or points.tta is not None:
                    # one row of scores per kept point: every kept row is its own "voxel".  Interpolated logits, or the
                    # scores accumulated over the views (never both: PointPath refuses the pair)
                    plogits = point_logits(run.output, items, err=ferr) if points.interp == "trilinear" else \
                        self._vote(run, logits, items, pin, points, terr)
                    vox_off = pin["kept_off"]
                    inverse = torch.cat([torch.arange(it["kept"], dtype=torch.int64, device=coords.device)
                                         for it in items])
                ids_out, _ = point_labels(plogits, pin["row_off"], pin["kept_off"], vox_off, pin["keep_row"],
                                          inverse, points.out_lut, points.fill, pin["labels_raw"], pin["lut"],
                                          pin["label_mask"], self.ignore_label, pcounts[done:done + k], perr)
                if points.on_point_labels is not None:
                    points.on_point_labels(ids[0], ids_out.cpu().numpy(), pin["row_off"])
            batch_of_scan += [nb] * k
            done += k
            nb += 1
            cur = nxt
        if counts is None:
            raise ValueError("TargetEvaluator: no batches")
        check_scan_error(err, "TargetEvaluator")
        counts = counts[:done].cpu().numpy()                     # the one read of a target
        batch_of_scan = np.asarray(batch_of_scan, dtype=np.int64)
        r = iou_rows(counts, rows, batch_of_scan)
        per_class, mean = mean_iou_rows(r)
        res = {"counts": counts, "batch_of_scan": batch_of_scan, "rows": r, "per_class": per_class, "mean": mean,
               "scans": done}
        if tables is not None:
            res["calibration"] = {name: table.result() for (name, _), table in zip(calibration, tables)}
        if points is not None:
            check_point_error(perr, "TargetEvaluator")
            if points.interp == "trilinear":
                ME.field_error(ferr.item(), "TargetEvaluator: point queries")
            pc = pcounts[:done].cpu().numpy()
            pr = iou_rows(point_iou_counts(pc), rows, batch_of_scan)
            p_class, p_mean = mean_iou_rows(pr)
            res.update(point_counts=pc, point_rows=pr, point_per_class=p_class, point_mean=p_mean)
            if points.tta is not None:
                _tta.check_vote_error(terr, "TargetEvaluator")
                res.update(tta_views=[v.name for v in points.tta], tta_mode=points.tta_mode)
        return res

    def _vote(self, run, logits, items, pin, points, terr):
        """float32 [kept, C]: the scores of every kept point of a loader batch accumulated over the views of
        points.tta (csrc/tta.hip).  View 0 is the regular forward's `logits`; every further view is built by
        tta.view_batch and goes through _forward on the recorded map trace with a manager of its own, so the
        Predictor's prefetch of the next loader batch stays untouched.  The views are voted in view order."""
        dev = logits.device
        inverse = torch.cat([it["inverse_map"].long() + int(pin["vox_off"][s]) for s, it in enumerate(items)])
        acc = torch.empty((inverse.shape[0], logits.shape[1]), dtype=torch.float32, device=dev)
        _tta.vote(logits, inverse, acc, points.tta_mode, first=True, err=terr)
        for view in points.tta[1:]:
            coords, feats, inverse = _tta.view_batch(items, view)
            out = _forward(self.model, coords, feats, None, self.precision, run.kernels)
            _tta.vote(out.F.contiguous(), inverse, acc, points.tta_mode, first=False, err=terr)
        return acc


# ------------------------------------------------------------------ point clouds of the prediction dump
_PLY_FIELDS = (("x", "<f8", "double"), ("y", "<f8", "double"), ("z", "<f8", "double"),
               ("red", "u1", "uchar"), ("green", "u1", "uchar"), ("blue", "u1", "uchar"))


def write_ply(path, points, colors):
    """binary little-endian PLY: `double x y z`, `uchar red green blue` (the properties of the point clouds test_step
    writes; open3d's exact bytes are not pinned).  points [n, 3], colors [n, 3] uint8; n = 0 writes an empty cloud."""
    import numpy as np
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    colors = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)
    if points.shape[0] != colors.shape[0]:
        raise ValueError(f"write_ply: {points.shape[0]} points, {colors.shape[0]} colours")
    v = np.empty(points.shape[0], dtype=np.dtype([(n, t) for n, t, _ in _PLY_FIELDS]))
    for i, n in enumerate("xyz"):
        v[n] = points[:, i]
    for i, n in enumerate(("red", "green", "blue")):
        v[n] = colors[:, i]
    header = ["ply", "format binary_little_endian 1.0", "comment lidog_amd prediction dump",
              f"element vertex {points.shape[0]}"] + [f"property {p} {n}" for n, _, p in _PLY_FIELDS] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(v.tobytes())
    return path


def read_ply(path):
    """(points [n, 3] float64, colors [n, 3] uint8) of a file written by write_ply"""
    import numpy as np
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    n = [int(l.split()[2]) for l in lines if l.startswith("element vertex ")][0]
    props = [tuple(l.split()[1:]) for l in lines if l.startswith("property ")]
    if props != [(p, name) for name, _, p in _PLY_FIELDS]:
        raise ValueError(f"{path}: properties {props} (this reader takes double x y z, uchar red green blue)")
    v = np.frombuffer(raw, dtype=np.dtype([(name, t) for name, t, _ in _PLY_FIELDS]), count=n, offset=end)
    return (np.stack([v["x"], v["y"], v["z"]], axis=1).reshape(-1, 3),
            np.stack([v["red"], v["green"], v["blue"]], axis=1).reshape(-1, 3))


# ------------------------------------------------------------------ label files of the point level
def load_inverse_label_map(path):
    """the `learning_map_inv` of a label-map file ({common class: id to write}; entry -1, if present, is the id of the
    records beyond the radius): a .json or .yaml file, read as scans.load_label_map reads its own"""
    import json
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
    if not isinstance(maps, dict) or "learning_map_inv" not in maps:
        raise ValueError(f"{path}: no 'learning_map_inv' entry")
    return {int(k): int(v) for k, v in maps["learning_map_inv"].items()}


def inverse_lut(mapping=None, num_classes=7, max_id=2 ** 31 - 1):
    """(out_lut int32 [num_classes] numpy, fill) of an inverse label map: the identity where the map says nothing, fill =
    its entry -1 or 0.  Keys outside -1 .. num_classes - 1 and ids outside 0 .. max_id (0xFFFF for a SemanticKITTI label
    file, whose upper half is the instance id) are a ValueError."""
    import numpy as np
    lut = np.arange(num_classes, dtype=np.int32)
    fill = 0
    for k, v in (mapping or {}).items():
        if not -1 <= k < num_classes:
            raise ValueError(f"inverse label map: class {k} outside -1 .. {num_classes - 1}")
        if not 0 <= v <= max_id:
            raise ValueError(f"inverse label map: id {v} of class {k} outside 0 .. {max_id}")
        if k == -1:
            fill = int(v)
        else:
            lut[k] = v
    return lut, fill


def label_file_path(folder, target, dataset, idx, points_path):
    """where the ids of scan `idx` go.  SemanticKITTI (points file .../sequences/SS/velodyne/NNNNNN.bin):
    `<folder>/<target>/sequences/SS/predictions/NNNNNN.label`, the layout the SemanticKITTI API reads; any other
    dataset: `<folder>/<target>/point_labels/<idx>.label`"""
    import os
    if dataset == "SemanticKITTI":
        parts = os.path.normpath(points_path).split(os.sep)
        if len(parts) < 4 or parts[-4] != "sequences" or parts[-2] != "velodyne":
            raise ValueError(f"{points_path}: not a .../sequences/SS/velodyne/NNNNNN.bin path")
        return os.path.join(folder, target, "sequences", parts[-3], "predictions",
                            os.path.splitext(parts[-1])[0] + ".label")
    return os.path.join(folder, target, "point_labels", f"{idx}.label")


def write_label_file(path, ids):
    """little-endian uint32, one per record, in file order: exactly 4 bytes per record"""
    import os
    import numpy as np
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.ascontiguousarray(ids).astype("<u4").tofile(path)
    return path


class PointLabelWriter:
    """PointPath's on_point_labels: one label file per scan of a batch (label_file_path), from the batch's one host copy.
    `files`: the listing's (points file, label file) pairs."""

    def __init__(self, folder, target, dataset, files):
        self.folder, self.target, self.dataset, self.files = folder, target, dataset, list(files)
        self.written = []

    def __call__(self, first_scan, labels_out, row_off):
        for s in range(len(row_off) - 1):
            idx = int(first_scan) + s
            path = label_file_path(self.folder, self.target, self.dataset, idx, self.files[idx][0])
            self.written.append(write_label_file(path, labels_out[int(row_off[s]):int(row_off[s + 1])]))
