"""Test-time augmentation restated in numpy (float64 where arithmetic rounds): the view matrices and flips, the voxel
rows of a view (the transform in the dtype numpy's rules give, the division by the voxel size, the floor) and the three
vote modes.  A restatement of this project's own definitions (lidog_amd/tta.py, csrc/tta.hip, csrc/aug_ops.h)."""
import math

import numpy as np

PRESETS = {"rot4": ["rotz90", "rotz180", "rotz270"], "flip4": ["flipx", "flipy", "flipx+flipy"]}
U24 = 2.0 ** -24


def rotz(deg):
    """[[c, -s, 0], [s, c, 0], [0, 0, 1]] with exact 0 / +-1 entries at the multiples of 90 degrees"""
    exact = {0: (1.0, 0.0), 90: (0.0, 1.0), 180: (-1.0, 0.0), 270: (0.0, -1.0)}
    d = deg % 360
    c, s = exact[int(d)] if d in exact else (math.cos(math.radians(deg)), math.sin(math.radians(deg)))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) + 0.0


def view_ops(name):
    """[("rot", R [3, 3]) | ("scale", s [3])] of a view name, left to right"""
    ops = []
    for atom in name.split("+"):
        if atom == "flipx":
            ops.append(("scale", np.array([-1.0, 1.0, 1.0])))
        elif atom == "flipy":
            ops.append(("scale", np.array([1.0, -1.0, 1.0])))
        elif atom.startswith("rotz"):
            ops.append(("rot", rotz(float(atom[4:]))))
        elif atom.startswith("scale"):
            ops.append(("scale", np.full(3, float(atom[5:]))))
        else:
            raise ValueError(atom)
    return ops


def expand(names):
    return ["identity"] + [v for n in names for v in PRESETS.get(n, [n])]


def transform(points, ops):
    """the points of a view: float32 until the first rotation, float64 from there on.  A rotation is the float64 chain
    (p0 R0j + p1 R1j) + p2 R2j of the widened row; a scale is one float64 product, rounded back to float32 while the
    array still is float32 (numpy's in-place column assignment)."""
    p = np.array(points, dtype=np.float32)
    for kind, par in ops:
        if kind == "rot":
            x = p.astype(np.float64)
            p = np.stack([(x[:, 0] * par[0, j] + x[:, 1] * par[1, j]) + x[:, 2] * par[2, j] for j in range(3)], axis=1)
        elif p.dtype == np.float64:
            p = p * par[None, :]
        else:
            p = (p.astype(np.float64) * par[None, :]).astype(np.float32)
    return p


def view_rows(points, ops, voxel, batch=0):
    """int32 [n, 4] (batch, x, y, z): floor(p / voxel) in p's own dtype, the voxel size rounded to that dtype"""
    p = transform(points, ops)
    q = np.broadcast_to(np.asarray(voxel, dtype=np.float64), (3,)).astype(p.dtype)
    c = np.floor(p / q[None, :]).astype(np.int32)
    return np.concatenate([np.full((c.shape[0], 1), batch, dtype=np.int32), c], axis=1)


def first_argmax(x):
    """[n] the first maximal index of every row, the first NaN in a row holding one"""
    x = np.asarray(x)
    nan = np.isnan(x)
    return np.where(nan.any(axis=1), nan.argmax(axis=1), np.where(nan, -np.inf, x).argmax(axis=1))


def scores(logits, mode):
    """float64 [m, C] of fp32 logits: the softmax with the row maximum subtracted, the logits, or the arg-max one-hot"""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    if mode == "logit":
        return x
    if mode == "vote":
        return np.eye(x.shape[1])[first_argmax(x)]
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)


def vote(views, mode):
    """float64 [k, C]: sum over `views` = [(logits [m_v, C], inverse [k])] of scores(logits)[inverse], in view order"""
    acc = None
    for logits, inverse in views:
        s = scores(logits, mode)[np.asarray(inverse, dtype=np.int64)]
        acc = s if acc is None else acc + s
    return acc


def prob_bound(n_views, n_classes):
    """absolute bound of the fp32 `prob` accumulation against vote(..., "prob"): V (C + 4 + V) 2^-24.  Per view and
    class, in units of 2^-24: the fp32 subtraction moves exp by at most e^-1, expf by at most 2 (ulp of a value <= 1),
    the class-order sum by C - 1, the division by 1/2; each of the V accumulating adds rounds a sum <= V, V / 2.  The
    derivation with the terms this list leaves out: DESIGN.md 3z."""
    return n_views * (n_classes + 4 + n_views) * U24
