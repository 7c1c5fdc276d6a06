"""Test-time augmentation at the point level: a checkpoint runs over several rotated, flipped or scaled views of every
scan, and every POINT takes the class the views agree on (evaluate.PointPath(tta=...), eval_target --tta).

A view is a `+`-joined list of atoms applied left to right: `rotz<deg>` (rotation about z, `coords @ R` as
RandomRotation applies its matrix, R = [[c, -s, 0], [s, c, 0], [0, 0, 1]]; multiples of 90 degrees have entries that are
exactly 0 and +-1), `flipx` / `flipy` (RandomScale by [-1, 1, 1] / [1, -1, 1]) and `scale<f>` (RandomScale by
[f, f, f], f > 0).  The identity is always view 0 and is never named.  A view is DEFINED as the voxel rows
data.augment_points writes for those operations (bounds=False): a rotation makes the coordinates float64, a pure flip or
scale keeps float32, as for a training item.  No transform kernel of its own.

    views = parse_views(["rot4", "flipx+scale0.95"])          # identity, rotz90, rotz180, rotz270, flipx+scale0.95
    coords, feats, inverse = view_batch(items, views[1])      # one quantize_rows for the loader batch
    vote(logits, inverse, acc, "prob", first=False, err=err)  # csrc/tta.hip: acc[p] += softmax(logits[inverse[p]])
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr
from .data import augment_points, quantize_rows

MAX_VIEWS = 16                         # the identity included
MAX_ATOMS = 4                          # of one view: AUG_MAX_OPS of csrc/aug_ops.h
MODES = ("prob", "logit", "vote")      # lidog_tta_vote's mode 0, 1, 2
PRESETS = {"rot4": ("rotz90", "rotz180", "rotz270"), "flip4": ("flipx", "flipy", "flipx+flipy")}
IDENTITY = "identity"


def rotz_matrix(deg):
    """R of `rotz<deg>`; for a multiple of 90 degrees the entries are exactly 0 and +-1, so the view permutes coordinates"""
    deg = float(deg)
    q = math.fmod(deg, 360.0)
    if q % 90.0 == 0.0:
        c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(q // 90.0) % 4]
    else:
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=np.float64) + 0.0       # no negative zero


def _atom(atom, view):
    """(operation of augment_points, its matrix M with coords' = coords @ M) of one atom"""
    if atom in ("flipx", "flipy"):
        s = np.array([-1.0, 1.0, 1.0] if atom == "flipx" else [1.0, -1.0, 1.0])
        return ("RandomScale", s), np.diag(s)
    for prefix in ("rotz", "scale"):
        if atom.startswith(prefix):
            try:
                v = float(atom[len(prefix):])
            except ValueError:
                break
            if prefix == "rotz":
                if not math.isfinite(v):
                    raise ValueError(f"tta view {view!r}: {atom!r} is no finite angle")
                r = rotz_matrix(v)
                return ("RandomRotation", r), r
            if not math.isfinite(v) or v <= 0.0:
                raise ValueError(f"tta view {view!r}: {atom!r}: the scale must be finite and positive")
            s = np.array([v, v, v], dtype=np.float64)
            return ("RandomScale", s), np.diag(s)
    raise ValueError(f"tta view {view!r}: unknown atom {atom!r} (rotz<deg>, flipx, flipy, scale<f>, joined with '+'; "
                     f"presets: {', '.join(PRESETS)})")


class View:
    """One view: `name`, `ops` (what data.augment_points takes) and `matrix` (float64 [3, 3], the product of the
    operations: two views are equal when their matrices are)."""

    def __init__(self, name):
        self.name = str(name)
        self.ops, self.matrix = [], np.eye(3)
        if self.name != IDENTITY:
            if self.name.count("+") >= MAX_ATOMS:
                raise ValueError(f"tta view {self.name!r}: more than {MAX_ATOMS} atoms (what lidog_augment_points takes)")
            for atom in self.name.split("+"):
                op, m = _atom(atom, self.name)
                self.ops.append(op)
                self.matrix = self.matrix @ m

    @property
    def f64(self):
        """the dtype rule of the augmentations: a rotation in the list makes the transformed coordinates float64"""
        return any(a == "RandomRotation" for a, _ in self.ops)

    def __eq__(self, other):
        return isinstance(other, View) and np.array_equal(self.matrix, other.matrix)

    def __hash__(self):
        return hash(self.matrix.tobytes())

    def __repr__(self):
        return f"View({self.name!r})"


def parse_views(names):
    """[View]: the identity first, then the named views with the presets expanded, in the order given.  A ValueError
    names an unknown atom, a bad scale, a view equal to the identity or to an earlier one (after expansion; equal means
    the same matrix, so `rotz360`, `flipx+flipx` and a second `rotz-90` beside `rotz270` are refused), and a list of
    more than MAX_VIEWS views."""
    if isinstance(names, (str, View)):
        names = [names]
    views = [View(IDENTITY)]
    for n in names:
        for v in ([n] if isinstance(n, View) else [View(x) for x in PRESETS.get(n, (n,))]):
            if v.name == IDENTITY or v == views[0]:
                raise ValueError(f"tta view {v.name!r} is the identity, which is always view 0 and is never named")
            for u in views[1:]:
                if v == u:
                    raise ValueError(f"tta view {v.name!r} equals view {u.name!r}")
            views.append(v)
    if len(views) > MAX_VIEWS:
        raise ValueError(f"tta: {len(views)} views with the identity (at most MAX_VIEWS = {MAX_VIEWS}); the last is "
                         f"{views[-1].name!r}")
    return views


def view_batch(items, view):
    """One view of a loader batch from its scans' FileScans.point_item dicts: (coords int32 [m, 4] (batch, x, y, z) as
    evaluate._forward takes them, feats float32 ones [m, 1], inverse int64 [kept_total]: kept row -> voxel row of THIS
    view's tensor, batch-global).  The rows of every scan are written under its batch index by data.augment_points and
    the whole batch goes through one data.quantize_rows.  The items must be what evaluate.point_queries takes."""
    if isinstance(view, str):
        view = View(view)
    if not items:
        raise ValueError("view_batch: no scans")
    rows = []
    for b, it in enumerate(items):
        pts = it.get("points")
        if pts is None or not it.get("plain", False) or pts.shape[0] != it["kept"] or \
                it["inverse_map"].shape[0] != pts.shape[0]:
            raise ValueError(f"{it.get('path', f'scan {b}')}: test-time augmentation need one query per kept row: a "
                             "FileScans validation item without augmentations and without the BEV bounds cut "
                             "(use interp='nearest' for this dataset)")
        rows.append(augment_points(pts.contiguous(), None, view.ops, it["voxel_size"], bounds=False, batch=b)[0])
    rows = torch.cat(rows) if len(rows) > 1 else rows[0]
    _, index, inverse = quantize_rows(rows, return_index=True, return_inverse=True)
    coords = rows[index].contiguous()
    return coords, torch.ones((coords.shape[0], 1), dtype=torch.float32, device=coords.device), inverse


def check_vote_error(err, what="tta.vote"):
    """raises when lidog_tta_vote set its error word (one read of a device word)"""
    e = int(err.item())
    if e:
        raise ValueError(f"{what}: an inverse entry outside the view's voxel rows (error word {e}); such points were "
                         "left out of the vote")


def vote(logits, inverse, acc, mode="prob", first=False, err=None):
    """lidog_tta_vote: acc [k, C] float32 (=, with `first`, or +=) the scores of logits [m, C] float32 at inverse int64
    [k]: the softmax (mode "prob"), the logits ("logit") or the one-hot of the arg-max ("vote").  Everything on the GPU;
    acc is changed in place and returned.  `err`: an int32 [1] device word the caller checks later with
    check_vote_error; without it this call checks, which costs one synchronisation."""
    if mode not in MODES:
        raise ValueError(f"tta.vote: mode={mode!r} (one of {', '.join(MODES)})")
    for name, t in (("logits", logits), ("inverse", inverse), ("acc", acc)):
        _lib.require_gpu(t, name)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError(f"tta.vote: logits must be float32 [m, C], got {logits.dtype} {tuple(logits.shape)}")
    m, c = logits.shape
    if inverse.dim() != 1 or inverse.dtype != torch.int64 or inverse.device != logits.device:
        raise ValueError(f"tta.vote: inverse must be int64 [k] on {logits.device}, got {inverse.dtype} "
                         f"{tuple(inverse.shape)} on {inverse.device}")
    k = inverse.shape[0]
    if acc.shape != (k, c) or acc.dtype != torch.float32 or not acc.is_contiguous() or acc.device != logits.device:
        raise ValueError(f"tta.vote: acc must be a contiguous float32 [{k}, {c}] tensor on {logits.device}")
    own_err = err is None
    if own_err:
        err = torch.zeros(1, dtype=torch.int32, device=logits.device)
    call("lidog_tta_vote", ptr(logits.contiguous()), m, c, ptr(inverse.contiguous()), k, MODES.index(mode),
         1 if first else 0, ptr(acc), ptr(err))
    if own_err:
        check_vote_error(err)
    return acc
