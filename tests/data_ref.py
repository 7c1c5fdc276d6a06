"""Yardstick for the data path in front of the network: voxel rows, first-occurrence quantisation, the label vote and
the BEV label image, in plain numpy, plus the edge inputs that tests/test_data_ref_cpu.py and
tests/test_gpu_data_edge.py share.  It imports neither the package nor the oracle.  Every result is an integer array, so
every comparison against it is np.array_equal.

  voxel_rows(points, q)        np.floor(points / float32(q)) on a float32 array (ME.utils.sparse_quantize's floor)
  quantize(rows)               unique rows in first-occurrence order, index (smallest row of each voxel), inverse
  vote(labels, index, inverse, ignore)   the first point's label if every point of the voxel agrees, else `ignore`
  bev_image(coords, labels, bound, img_size, voxel, B)   PC2ImgConverter.getBEVImageNew scan by scan, from the rule in
                               lidog_amd.data.label_luts' docstring: no look-up tables, so the tables are under test too

`variant=` switches one function to a deliberately WRONG rule.  Only the tests of the yardstick itself pass it: they show
that each wrong rule changes the result on an edge input below, so the same input catches that error in a kernel."""
import numpy as np

COORD_LO, COORD_HI = -65536, 65535          # the range of the coordinate hash (lidog_pack): 17 bits per axis
BATCH_HI = 4095
Z_RANGE = (-10.0, 8.0)


# ------------------------------------------------------------------ voxel rows
def voxel_rows(points, q, variant=None):
    """int32 [n, 3] = np.floor(points / q) with points and q float32: one correctly rounded float32 division per
    coordinate, then the floor.  A NaN or infinite quotient becomes INT32_MIN, as numpy's cast gives it on x86.
    Wrong variants: 'trunc' (rounds toward zero), 'reciprocal' (multiplies by float32(1 / q)), 'float64' (divides in
    double)."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    q64 = np.broadcast_to(np.asarray(q, dtype=np.float64), (3,))
    q = q64.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if variant is None:
            f = np.floor(p / q)
        elif variant == "trunc":
            f = np.trunc(p / q)
        elif variant == "reciprocal":
            f = np.floor(p * (np.float32(1.0) / q))
        elif variant == "float64":
            f = np.floor(p.astype(np.float64) / q64)
        else:
            raise ValueError(variant)
        out = np.full(f.shape, np.iinfo(np.int32).min, dtype=np.int32)
        ok = np.isfinite(f) & (np.abs(f) < 2.0 ** 31)
        out[ok] = f[ok].astype(np.int32)
    return out


def in_range(rows):
    """rows [n, 3] (x, y, z) or [n, 4] (batch, x, y, z): True where the coordinate hash accepts the row"""
    rows = np.asarray(rows)
    xyz = rows[:, -3:]
    ok = np.all((xyz >= COORD_LO) & (xyz <= COORD_HI), axis=1)
    if rows.shape[1] == 4:
        ok &= (rows[:, 0] >= 0) & (rows[:, 0] <= BATCH_HI)
    return ok


# ------------------------------------------------------------------ quantisation
def quantize(rows, variant=None):
    """rows int [n, k] -> (unique rows [m, k] in the order of their first occurrence, index int64 [m]: the smallest row
    number of every voxel, inverse int64 [n]: the voxel of every row).  rows[index][inverse] == rows.
    Wrong variant: 'last' (the LARGEST row number of every voxel, voxels ordered by it)."""
    rows = np.ascontiguousarray(rows)
    n = rows.shape[0]
    if n == 0:
        return rows.copy(), np.zeros(0, np.int64), np.zeros(0, np.int64)
    order = np.lexsort(rows.T[::-1])                       # stable: equal rows stay in ascending row number
    srt = rows[order]
    new = np.ones(n, dtype=bool)
    new[1:] = np.any(srt[1:] != srt[:-1], axis=1)
    group = np.cumsum(new) - 1                             # group of every sorted row
    m = int(group[-1]) + 1
    rep = np.empty(m, dtype=np.int64)
    if variant is None:
        rep[group[::-1]] = order[::-1]                     # the first (smallest) row number of a group is written last
    elif variant == "last":
        rep[group] = order
    else:
        raise ValueError(variant)
    by_rep = np.argsort(rep, kind="stable")                # voxels in the order of their representative row
    rank = np.empty(m, dtype=np.int64)
    rank[by_rep] = np.arange(m)
    index = rep[by_rep]
    inverse = np.empty(n, dtype=np.int64)
    inverse[order] = rank[group]
    return rows[index], index, inverse


def vote(labels, index, inverse, ignore, variant=None):
    """voxel labels [m], in the labels' dtype: labels[index[j]] when every point of voxel j carries it, else `ignore`.
    Wrong variant: 'majority' (the most frequent label of the voxel, ties to the smallest)."""
    labels = np.asarray(labels)
    first = labels[index]
    if variant is None:
        disagree = labels != first[inverse]
        mixed = np.zeros(index.shape[0], dtype=bool)
        mixed[inverse[disagree]] = True
        return np.where(mixed, np.asarray(ignore, dtype=labels.dtype), first).astype(labels.dtype)
    if variant != "majority":
        raise ValueError(variant)
    out = np.empty(index.shape[0], dtype=labels.dtype)
    for j in range(index.shape[0]):
        vals, counts = np.unique(labels[inverse == j], return_counts=True)
        out[j] = vals[np.argmax(counts)]
    return out


# ------------------------------------------------------------------ BEV label image
def image_side(bound, img_size):
    """maxImgWidth / maxImgHeight: int(2 * bound / grid) with grid = 2 * bound / img_size in python floats.  Not always
    img_size: (25, 83) gives 82."""
    grid = (bound - (-bound)) / img_size
    return int((bound - (-bound)) / grid)


def bev_pixels(xyz, bound, img_size, voxel, variant=None):
    """xyz int [n, 3] voxel coordinates -> (px, py int64 [n], keep bool [n]).  x = float32(c * voxel); a point is kept
    when -bound < x < bound, -bound < y < bound and -10 < z < 8, all strict; px = floor((x + bound) / grid),
    py = floor(S - (y + bound) / grid) - 1 in float32; a negative index wraps once by S, as numpy indexing does.  An
    index that still lies outside the image (numpy would raise IndexError) drops the point.
    Wrong variants: 'closed' (<= in the bounds), 'nowrap' (a negative index drops the point)."""
    S = image_side(bound, img_size)
    grid = np.float32((bound - (-bound)) / img_size)
    lo, hi = np.float32(-bound), np.float32(bound)
    zlo, zhi = np.float32(Z_RANGE[0]), np.float32(Z_RANGE[1])
    p = (np.asarray(xyz).astype(np.float64) * voxel).astype(np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    if variant == "closed":
        keep = (lo <= x) & (x <= hi) & (lo <= y) & (y <= hi) & (zlo <= z) & (z <= zhi)
    else:
        keep = (lo < x) & (x < hi) & (lo < y) & (y < hi) & (zlo < z) & (z < zhi)
    px = np.floor((x - lo) / grid).astype(np.int64)
    py = np.floor(np.float32(S) - (y - lo) / grid).astype(np.int64) - 1
    if variant != "nowrap":
        px = np.where(px < 0, px + S, px)
        py = np.where(py < 0, py + S, py)
    keep = keep & (px >= 0) & (px < S) & (py >= 0) & (py < S)
    return px, py, keep


def bev_image(coords, labels, bound, img_size, voxel, B, variant=None):
    """coords int [N, 4] (batch, x, y, z), labels [N] -> (img int64 [B, S, S], point_idx int32 [B, S, S]), both -1 where
    no point fell.  Scan by scan, point by point in row order: a point with label -1 is skipped, a later point
    overwrites an earlier one, point_idx counts from the scan's first row.
    Wrong variants: 'first' (an occupied pixel is never overwritten), and those of bev_pixels."""
    coords = np.asarray(coords).reshape(-1, 4)
    labels = np.asarray(labels)
    S = image_side(bound, img_size)
    img = np.full((B, S, S), -1, dtype=np.int64)
    idx = np.full((B, S, S), -1, dtype=np.int32)
    for b in range(B):
        rows = np.nonzero(coords[:, 0] == b)[0]
        px, py, keep = bev_pixels(coords[rows, 1:], bound, img_size, voxel,
                                  variant if variant in ("closed", "nowrap") else None)
        lab = labels[rows]
        for j in np.nonzero(keep & (lab != -1))[0]:
            if variant == "first" and idx[b, py[j], px[j]] >= 0:
                continue
            img[b, py[j], px[j]] = lab[j]
            idx[b, py[j], px[j]] = j
    return img, idx


# ------------------------------------------------------------------ edge inputs: voxel rows
GRID_Q = {"scalar": 0.05, "per_axis": (0.05, 0.1, 0.2)}


def grid_points(q):
    """float32(k * q) for every k in COORD_LO ... COORD_HI, per axis: points ON the voxel boundaries, where voxel centres
    re-quantised by a merge sit and random LiDAR points never do.  float32 [131072, 3]."""
    k = np.arange(COORD_LO, COORD_HI + 1, dtype=np.float64)
    q = np.broadcast_to(np.asarray(q, dtype=np.float64), (3,))
    return (k[:, None] * q[None, :]).astype(np.float32)


def below_grid_points(q):
    """the largest float32 below every point of grid_points(q)"""
    return np.nextafter(grid_points(q), np.float32(-np.inf))


def special_points(q):
    """+-0.0, the smallest and a larger denormal of either sign, the largest float32 below 0 / q / -q, and both ends of
    the coordinate range approached from inside.  float32 [n, 3], every row in range."""
    q = np.broadcast_to(np.asarray(q, dtype=np.float64), (3,))
    tiny = np.float32(1e-45)
    vals = [np.float32(0.0), np.float32(-0.0), tiny, -tiny, np.float32(1e-40), np.float32(-1e-40),
            np.float32(1.1754942e-38), np.float32(-1.1754942e-38)]
    rows = [[v, v, v] for v in vals]
    rows += [[vals[i], vals[(i + 1) % 8], vals[(i + 3) % 8]] for i in range(8)]
    for k in (COORD_LO + 0.5, COORD_LO + 0.999, COORD_HI + 0.001, COORD_HI + 0.5, -1.5, -0.5, 0.5, 1.5):
        rows.append(list((k * q).astype(np.float32)))
    return np.asarray(rows, dtype=np.float32)


def past_the_ends(q):
    """{name: one point}: one voxel past either end of the range"""
    q = np.broadcast_to(np.asarray(q, dtype=np.float64), (3,))
    return {"below_lo": ((COORD_LO - 0.5) * q).astype(np.float32)[None, :] * np.float32([1, 0, 0]),
            "above_hi": ((COORD_HI + 1.5) * q).astype(np.float32)[None, :] * np.float32([0, 0, 1])}


# ------------------------------------------------------------------ edge inputs: sizes and row patterns
# around the 64-lane wave, the 256-thread block, the 1024-row scan block, the capacity steps of lidog_hash_capacity
# (1024 slots up to n = 512, doubling from 513) and the carry of scan_block_offsets across chunks of 256 block sums
# (n > 262 144); 263 169 = 257 * 1024 + 1
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 262144, 262145, 263169)
PATTERNS = ("distinct", "same", "triple")


def _scatter(v):
    """distinct in-range (x, y, z) for distinct v < 2^20, in no monotone order"""
    s = (np.asarray(v, dtype=np.int64) * 2654435761) % (1 << 20)
    return np.stack([(s & 1023) - 512, (s >> 10) - 300, (s % 7) - 3], axis=1)


def size_rows(n, pattern):
    """rows int32 [n, 4], batch 0.  'distinct': every row its own voxel; 'same': one voxel; 'triple': row i in voxel
    i mod ceil(n / 3), so about three rows per voxel, ceil(n / 3) rows apart: more than 1024 (another scan block, another
    workgroup) for the three large sizes."""
    i = np.arange(n, dtype=np.int64)
    if pattern == "distinct":
        xyz = _scatter(i)
    elif pattern == "same":
        xyz = np.tile(np.array([[3, -4, 5]], dtype=np.int64), (n, 1))
    elif pattern == "triple":
        xyz = _scatter(i % max(-(-n // 3), 1))
    else:
        raise ValueError(pattern)
    return np.concatenate([np.zeros((n, 1), np.int64), xyz], axis=1).astype(np.int32)


def size_columns(n, seed=0):
    """(features float32 [n, 2], labels int64 [n] in -1 ... 6) that go with size_rows(n, .)"""
    rng = np.random.default_rng(1000 + seed + n)
    return rng.standard_normal((n, 2)).astype(np.float32), rng.integers(-1, 7, n)


# ------------------------------------------------------------------ edge inputs: label vote
def vote_case(ignore):
    """(rows int32 [n, 4], labels int64 [n], {name: voxel row (x, y, z)}).  Voxels:
      ignore_first_agree   every point carries `ignore`: the vote is `ignore` because that is the common label
      ignore_first_mixed   the first point carries `ignore`, the other four carry 3
      last_dissents        600 points, every fifth row over 3 000 rows (12 blocks of 256): label 2, the very last one 4
      unanimous            600 points of label 5 next to it, the control
    and a filler voxel per remaining row."""
    n = 3100
    xyz = np.stack([np.arange(n) + 100, np.zeros(n, np.int64), np.zeros(n, np.int64)], axis=1)    # fillers
    lab = np.arange(n) % 7
    named = {"ignore_first_agree": (1, 1, 1), "ignore_first_mixed": (2, 2, 2), "last_dissents": (-3, -3, -3),
             "unanimous": (-4, 4, -4)}
    a = np.array([5, 702, 1999]); xyz[a] = named["ignore_first_agree"]; lab[a] = ignore
    m = np.array([6, 7, 303, 1503, 2998]); xyz[m] = named["ignore_first_mixed"]; lab[m] = 3; lab[6] = ignore
    d = 10 + 5 * np.arange(600); xyz[d] = named["last_dissents"]; lab[d] = 2; lab[d[-1]] = 4
    u = 11 + 5 * np.arange(600); xyz[u] = named["unanimous"]; lab[u] = 5
    assert d[-1] - d[0] > 2048 and len(set(map(tuple, xyz[[a[0], m[0], d[0], u[0]]]))) == 4
    rows = np.concatenate([np.zeros((n, 1), np.int64), xyz], axis=1).astype(np.int32)
    return rows, lab.astype(np.int64), named


# ------------------------------------------------------------------ edge inputs: BEV label image
BEV_GEOMETRIES = ((50.0, 167), (30.0, 100))
BEV_VOXEL = 0.05


def lut_lo(bound, voxel=BEV_VOXEL):
    """lowest coordinate of the look-up tables of lidog_amd.data.label_luts; they cover lut_lo ... -lut_lo - 1"""
    return -int(1.3 * bound / voxel)


def bev_scan(bound, seed, voxel=BEV_VOXEL):
    """one scan's (xyz int64 [n, 3], labels int64 [n], {name: row numbers}) with, in this order:
      bulk        3 000 random voxels over 1.1 x the bounds, labels -1 ... 6
      lut_ends    voxels at lut_lo - 1, lut_lo, -lut_lo - 1 and -lut_lo on each axis (the other two coordinates inside)
      bounds      x and y at +-bound / voxel (dropped: the bounds are strict) and one voxel inside
      z_ends      z at -200 and 160 (dropped), -199 and 159 (kept)
      wrap_row    a line of voxels along x whose y gives pixel row -1, which numpy wraps to S - 1
      one_pixel   20 000 rows in one pixel, labelled ones and -1 alternating, the last row -1
    The named groups use pixels of their own where they can; the bulk is drawn first, so the groups win theirs."""
    rng = np.random.default_rng(seed)
    c = int(round(bound / voxel))
    lo = lut_lo(bound, voxel)
    groups, xyz, lab = {}, [], []

    def add(name, pts, labels):
        start = sum(len(p) for p in xyz)
        pts = np.asarray(pts, dtype=np.int64).reshape(-1, 3)
        xyz.append(pts)
        lab.append(np.broadcast_to(np.asarray(labels, dtype=np.int64), (pts.shape[0],)).copy())
        groups[name] = np.arange(start, start + pts.shape[0])

    n = 3000
    add("bulk", np.stack([rng.integers(-int(1.1 * c), int(1.1 * c), n), rng.integers(-int(1.1 * c), int(1.1 * c), n),
                          rng.integers(-220, 180, n)], axis=1), rng.integers(-1, 7, n))
    ends = [lo - 1, lo, -lo - 1, -lo]
    add("lut_ends", [[e, 40, 0] for e in ends] + [[40, e, 0] for e in ends] + [[40, 80, e] for e in ends], 1)
    add("bounds", [[-c, 120, 0], [-c + 1, 120, 0], [c - 1, 120, 0], [c, 120, 0],
                   [160, -c, 0], [160, -c + 1, 0], [160, c - 1, 0], [160, c, 0]], [2, 3, 4, 5, 2, 3, 4, 5])
    add("z_ends", [[200, 200, -200], [240, 200, -199], [280, 200, 159], [320, 200, 160]], [6, 5, 4, 3])
    xs = np.arange(-c + 5, c - 5, 37)
    add("wrap_row", np.stack([xs, np.full_like(xs, c - 1), np.zeros_like(xs)], axis=1), np.arange(xs.shape[0]) % 7)
    k = 20000
    labels = np.where(np.arange(k) % 2 == 0, np.arange(k) // 2 % 7, -1)
    add("one_pixel", np.stack([np.full(k, -400), np.full(k, -400), np.arange(k) % 300 - 190], axis=1), labels)
    return np.concatenate(xyz), np.concatenate(lab), groups


def bev_batch(bound, empty=(1, 3), B=4):
    """(coords int32 [N, 4], labels int64 [N], {scan: groups}) of B scans, those in `empty` without a row; the others
    are bev_scan with a seed of their own, every second one in reverse row order"""
    coords, labels, groups = [], [], {}
    for b in range(B):
        if b in empty:
            continue
        xyz, lab, g = bev_scan(bound, seed=7 + b)
        if (b // 2) % 2:
            xyz, lab = xyz[::-1], lab[::-1]
            g = {k: xyz.shape[0] - 1 - v for k, v in g.items()}
        coords.append(np.concatenate([np.full((xyz.shape[0], 1), b, np.int64), xyz], axis=1))
        labels.append(lab)
        groups[b] = g
    return np.concatenate(coords).astype(np.int32), np.concatenate(labels).astype(np.int64), groups
