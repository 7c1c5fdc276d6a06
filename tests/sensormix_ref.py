"""PolarMix and LaserMix restated in numpy, from the definitions in include/lidog_amd.h alone.

Neither method is in the reference, so there is no fixture: this restatement is what the kernels and the merges of
lidog_amd.data are compared with, bit for bit.  numpy rounds every float64 product, sum and difference on its own, which
is the arithmetic the header asks for; the `*_fused` forms evaluate the same expressions with ONE rounding (exact
rational arithmetic, then float), which is what a fused multiply-add would give: the tests use them to find rows where
the two disagree.

  centres(coords)                       X, Y, Z = 2c + 1 as int64
  in_range(coords)                      |c| < 2^24 per row
  sector(coords, a, b, wide)            the sector predicate
  band(coords, t2, neg)                 the number of boundaries a row is at or above
  keys(coords, labels, ...)             the int32 key of lidog_sensormix_keys
  rotate(coords, c, s)                  the voxel of a pasted row
  select(keys, key_set)                 ascending rows whose key is in a 32-bit key set
  gather_rows(...)                      the merged voxel rows [total, 4] and (is_donor, source row) of every merged row
  first_rows(rows)                      quantize_rows' index: the first row of every voxel, ascending
  lasermix_np / polarmix_np             the whole merges, from draws (draw_lasermix_np / draw_polarmix_np)
"""
from fractions import Fraction

import numpy as np

LIMIT = 1 << 24
COLUMNS = ("features", "sem_labels", "xyz", "sampled_idx")


def centres(coords):
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    return 2 * c[:, 0] + 1, 2 * c[:, 1] + 1, 2 * c[:, 2] + 1


def in_range(coords):
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    return (np.abs(c) < LIMIT).all(axis=1)


def sector(coords, a, b, wide=0):
    X, Y, _ = centres(coords)
    Xd, Yd = X.astype(np.float64), Y.astype(np.float64)
    sa = np.float64(a[0]) * Yd - np.float64(a[1]) * Xd          # two rounded products, one rounded difference
    sb = np.float64(b[0]) * Yd - np.float64(b[1]) * Xd
    return ((sa >= 0) | (sb < 0)) if wide else ((sa >= 0) & (sb < 0))


def band(coords, t2, neg):
    X, Y, Z = centres(coords)
    zz = (Z * Z).astype(np.float64)
    rr = (X * X + Y * Y).astype(np.float64)
    out = np.zeros(X.shape[0], dtype=np.int64)
    for t, n in zip(t2, neg):
        lim = np.float64(t) * rr
        out += ((Z > 0) | (zz <= lim)) if n else ((Z > 0) & (zz >= lim))
    return out


def keys(coords, labels, a=(1.0, 0.0), b=(1.0, 0.0), wide=0, t2=(), neg=(), mask=0):
    """(keys int32 [n], flag): rows out of range keep the key -1 here and set the flag"""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    ok = in_range(c)
    safe = np.where(ok[:, None], c, 0)
    lab = np.full(c.shape[0], -1, np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    inst = (lab >= 0) & (lab < 32) & (((int(mask) >> np.clip(lab, 0, 31)) & 1) == 1)
    k = sector(safe, a, b, wide).astype(np.int64) | (band(safe, t2, neg) << 1) | (inst.astype(np.int64) << 4)
    return np.where(ok, k, -1).astype(np.int32), int(not ok.all())


def rotate(coords, c, s):
    v = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    U, V = v[:, 0].astype(np.float64) + 0.5, v[:, 1].astype(np.float64) + 0.5
    c, s = np.float64(c), np.float64(s)
    x = c * U - s * V
    y = s * U + c * V
    return np.stack([np.floor(x).astype(np.int64), np.floor(y).astype(np.int64), v[:, 2]], axis=1)


# ---- the same expressions as a compiler could contract them: one product exact inside a fused multiply-add
def sector_value_exact(x, y, a):
    """sa of voxel (x, y) for direction a as (two rounded products and a rounded difference, fma(ax, Y, -fl(ay X)),
    fma(-ay, X, fl(ax Y))), the fused forms evaluated in exact rational arithmetic and rounded once"""
    X, Y = 2 * int(x) + 1, 2 * int(y) + 1
    p1, p2 = float(np.float64(a[0]) * np.float64(Y)), float(np.float64(a[1]) * np.float64(X))
    two = float(np.float64(p1) - np.float64(p2))
    fma_first = float(Fraction(float(a[0])) * Y - Fraction(p2))       # fma(ax, Y, -fl(ay X))
    fma_second = float(Fraction(p1) - Fraction(float(a[1])) * X)      # fma(-ay, X, fl(ax Y))
    return two, fma_first, fma_second


def rotate_x_exact(x, y, c, s):
    """x' = c U - s V of voxel (x, y) in the same three forms"""
    U, V = Fraction(2 * int(x) + 1, 2), Fraction(2 * int(y) + 1, 2)
    p1, p2 = float(np.float64(c) * np.float64(float(U))), float(np.float64(s) * np.float64(float(V)))
    two = float(np.float64(p1) - np.float64(p2))
    fma_first = float(Fraction(float(c)) * U - Fraction(p2))
    fma_second = float(Fraction(p1) - Fraction(float(s)) * V)
    return two, fma_first, fma_second


# ---- selection, gather, quantisation
def key_set(pred):
    return sum(1 << k for k in range(32) if pred(k & 1, (k >> 1) & 7, (k >> 4) & 1))


def select(keys_, kset):
    k = np.asarray(keys_, dtype=np.int64)
    ok = (k >= 0) & (k < 32)
    return np.nonzero(ok & (((int(kset) >> np.clip(k, 0, 31)) & 1) == 1))[0].astype(np.int32)


def gather_rows(coords_b, coords_d, keep, take, paste, copies):
    """(rows int32 [total, 4], is_donor bool [total], src int64 [total])"""
    cb = np.asarray(coords_b, dtype=np.int64).reshape(-1, 3)
    cd = np.asarray(coords_d, dtype=np.int64).reshape(-1, 3)
    parts = [cb[keep], cd[take]]
    src = [np.asarray(keep, np.int64), np.asarray(take, np.int64)]
    donor = [np.zeros(len(keep), bool), np.ones(len(take), bool)]
    if len(paste):
        for c, s in copies:
            parts.append(cd[paste] if (c, s) == (1.0, 0.0) else rotate(cd[paste], c, s))
            src.append(np.asarray(paste, np.int64))
            donor.append(np.ones(len(paste), bool))
    vox = np.concatenate(parts, axis=0)
    rows = np.concatenate([np.zeros((vox.shape[0], 1), np.int64), vox], axis=1).astype(np.int32)
    return rows, np.concatenate(donor), np.concatenate(src)


def gather_col(base_col, donor_col, is_donor, src):
    """a merged column: the source row's entry, unchanged, in the base scan's dtype"""
    b = np.asarray(base_col)
    d = np.asarray(donor_col).astype(b.dtype)
    out = np.empty((len(src),) + b.shape[1:], dtype=b.dtype)
    out[~is_donor] = b[src[~is_donor]]
    out[is_donor] = d[src[is_donor]]
    return out


def first_rows(rows):
    """index of quantize_rows: the smallest row number of every voxel, ascending"""
    r = np.asarray(rows)
    if r.shape[0] == 0:
        return np.zeros(0, np.int64)
    _, first = np.unique(r, axis=0, return_index=True)
    return np.sort(first).astype(np.int64)


def merge_np(scan0, scan1, sel, a, b, t2, neg, mask, keep_set, take_set, paste_set, copies):
    donor, base = (scan0, scan1) if sel == 0 else (scan1, scan0)
    kb, fb = keys(base["coordinates"], base["sem_labels"], a, b, 0, t2, neg, mask)
    kd, fd = keys(donor["coordinates"], donor["sem_labels"], a, b, 0, t2, neg, mask)
    assert not (fb or fd)
    keep, take, paste = select(kb, keep_set), select(kd, take_set), select(kd, paste_set)
    rows, is_donor, src = gather_rows(base["coordinates"], donor["coordinates"], keep, take, paste, copies)
    index = first_rows(rows)
    out = {"coordinates": rows[index][:, 1:].astype(np.int32)}
    for k in COLUMNS:
        if k in base:
            out[k] = gather_col(base[k], donor[k], is_donor, src)[index]
    if "idx" in scan0:
        out["idx"] = np.array([[int(scan0["idx"])], [int(scan1["idx"])]], dtype=np.int64)
    out["index"] = index
    out["source"] = sel
    out["counts"] = (len(keep), len(take)) + (len(paste),) * len(copies)
    out["_rows"], out["_is_donor"], out["_src"] = rows, is_donor, src
    return out


def draw_source_np(rng):
    return int(rng.choice([0, 1]))


def draw_lasermix_np(rng, areas=(3, 4, 5, 6)):
    sel = draw_source_np(rng)
    return {"source": sel, "n_areas": int(rng.choice(areas))}


def draw_polarmix_np(rng, swap_prob=0.5, paste_prob=1.0):
    sel = draw_source_np(rng)
    alpha = (rng.random_sample() - 1) * np.pi
    omega1 = rng.random_sample() * 2 * np.pi / 3
    omega2 = (rng.random_sample() + 1) * 2 * np.pi / 3
    swap = bool(rng.random_sample() < swap_prob)
    paste = bool(rng.random_sample() < paste_prob)
    return {"source": sel, "alpha": float(alpha), "omega1": float(omega1), "omega2": float(omega2), "swap": swap,
            "paste": paste}


def bounds_np(pitch, n_areas):
    """(angles, t2, neg) of the interior boundaries"""
    th = np.linspace(np.radians(pitch[0]), np.radians(pitch[1]), n_areas + 1)[1:-1]
    t = np.tan(th)
    return th, t * t, (t < 0).astype(np.int32)


def lasermix_np(scan0, scan1, draws, pitch=(-25.0, 3.0)):
    _, t2, neg = bounds_np(pitch, draws["n_areas"])
    return merge_np(scan0, scan1, draws["source"], (1.0, 0.0), (1.0, 0.0), t2, neg, 0,
                    key_set(lambda s, bnd, i: bnd % 2 == 0), key_set(lambda s, bnd, i: bnd % 2 == 1), 0, ())


def polarmix_np(scan0, scan1, draws, instance_classes=(0, 1)):
    mask = sum(1 << int(c) for c in instance_classes) if draws["paste"] else 0
    a = (float(np.cos(draws["alpha"])), float(np.sin(draws["alpha"])))
    copies = ((1.0, 0.0),) + tuple((float(np.cos(draws[k])), float(np.sin(draws[k]))) for k in ("omega1", "omega2"))
    keep = key_set(lambda s, bnd, i: not s) if draws["swap"] else 0xFFFFFFFF
    take = key_set(lambda s, bnd, i: s) if draws["swap"] else 0
    paste = key_set(lambda s, bnd, i: i) if draws["paste"] else 0
    return merge_np(scan0, scan1, draws["source"], a, (-a[0], -a[1]), (), (), mask, keep, take, paste, copies)
