"""DBSCAN restated so that it scales (numpy only), and the inputs of the cluster edge-case tests.

The definition is sn_ref.dbscan_np's: core = at least min_samples neighbours, the row itself included; clusters = the
components of the core graph, numbered by their smallest core row; a border row takes the smallest cluster number among
its core neighbours; -1 otherwise.  The predicate is the same as well: on x = float32(c) * float32(voxel),
(dx*dx + dy*dy) + dz*dz <= eps*eps in float64.  Only the way candidate pairs are found differs: rows are binned into
cubic cells of ceil(eps / voxel) voxels and sorted by cell key, a row's candidates are the rows of the 27 cells around
its own (9 key ranges, by searchsorted, in chunks), and every candidate goes through the exact predicate.  Components
come from min-label hooking and pointer jumping over the core-core pairs, all vectorised.

tests/test_cluster_ref_cpu.py checks the restatement against sn_ref.dbscan_np, against the sklearn labels recorded in
G12 (up to 18 454 rows) and, where sklearn imports, against sklearn itself on every case below."""
import functools

import numpy as np

VOXEL, EPS, MIN_SAMPLES = 0.05, 0.5, 10
CHUNK = 1 << 21                    # candidate pairs per chunk


# ------------------------------------------------------------------ the restatement
def cell_edge(voxel, eps):
    """cell edge in voxels, as lidog_dbscan takes it: ceil(eps / float32(voxel)), at least 1"""
    return max(int(np.ceil(eps / float(np.float32(voxel)))), 1)


def cell_keys(coords, voxel=VOXEL, eps=EPS):
    """(keys int64 [n], cells per axis int64 [3]): key = (cx * ny + cy) * nz + cz over the input's bounding box"""
    c = np.asarray(coords).astype(np.int64).reshape(-1, 3)
    cell = cell_edge(voxel, eps)
    lo = c.min(0)
    dims = (c.max(0) - lo) // cell + 1
    q = (c - lo) // cell
    return (q[:, 0] * dims[1] + q[:, 1]) * dims[2] + q[:, 2], dims


def neighbour_pairs(coords, voxel=VOXEL, eps=EPS):
    """(a, b) int64: every ordered pair of distinct rows within eps of each other, grouped by nothing in particular"""
    c = np.asarray(coords).astype(np.int64).reshape(-1, 3)
    n = len(c)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    cell = cell_edge(voxel, eps)
    keys, dims = cell_keys(c, voxel, eps)
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    q = (c[order] - c.min(0)) // cell
    x = (c[order].astype(np.float32) * np.float32(voxel)).astype(np.float64)
    # the cells (nx, ny, z0..z1) are consecutive keys: 9 ranges per row
    z0, z1 = np.maximum(q[:, 2] - 1, 0), np.minimum(q[:, 2] + 1, dims[2] - 1)
    lo, hi = np.zeros((9, n), np.int64), np.zeros((9, n), np.int64)
    for r in range(9):
        nx, ny = q[:, 0] + (r // 3 - 1), q[:, 1] + (r % 3 - 1)
        ok = (nx >= 0) & (nx < dims[0]) & (ny >= 0) & (ny < dims[1])
        base = (nx * dims[1] + ny) * dims[2]
        lo[r] = np.where(ok, np.searchsorted(keys, base + z0, side="left"), 0)
        hi[r] = np.where(ok, np.searchsorted(keys, base + z1 + 1, side="left"), 0)
    cnt = hi - lo                                      # [9, n]
    ends = np.cumsum(cnt.sum(0))
    eps2 = float(eps) * float(eps)
    out_a, out_b = [], []
    r0 = 0
    while r0 < n:
        before = ends[r0 - 1] if r0 else 0
        r1 = max(int(np.searchsorted(ends, before + CHUNK, side="right")), r0 + 1)
        k = cnt[:, r0:r1].T.ravel()                    # row-major: row, then range
        total = int(k.sum())
        src = np.repeat(np.repeat(np.arange(r0, r1), 9), k)
        first = np.repeat(lo[:, r0:r1].T.ravel() - (np.cumsum(k) - k), k)
        dst = first + np.arange(total)
        d = x[src] - x[dst]
        hit = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= eps2) & (src != dst)
        out_a.append(order[src[hit]])
        out_b.append(order[dst[hit]])
        r0 = r1
    return np.concatenate(out_a), np.concatenate(out_b)


def components(n, a, b):
    """root int64 [n]: the smallest row of every row's component under the edges (a, b)"""
    p = np.arange(n, dtype=np.int64)
    while len(a):
        pa, pb = p[a], p[b]
        live = pa != pb
        if not live.any():
            break
        a, b, pa, pb = a[live], b[live], pa[live], pb[live]
        m = np.minimum(pa, pb)
        np.minimum.at(p, pa, m)                        # hook the larger root under the smaller
        np.minimum.at(p, pb, m)
        while True:                                    # pointer jumping
            pp = p[p]
            if np.array_equal(pp, p):
                break
            p = pp
    return p


def dbscan(coords, voxel=VOXEL, eps=EPS, min_samples=MIN_SAMPLES):
    """labels int64 [n] of distinct integer rows"""
    n = len(coords)
    if n == 0:
        return np.zeros(0, np.int64)
    a, b = neighbour_pairs(coords, voxel, eps)
    core = np.bincount(a, minlength=n) + 1 >= min_samples
    cc = core[a] & core[b]
    root = components(n, a[cc], b[cc])
    is_root = core & (root == np.arange(n))
    number = np.cumsum(is_root) - is_root              # roots before the row: the order of the smallest core row
    labels = np.full(n, -1, np.int64)
    labels[core] = number[root[core]]
    big = np.iinfo(np.int64).max
    best = np.full(n, big, np.int64)
    bd = ~core[a] & core[b]
    np.minimum.at(best, a[bd], labels[b[bd]])
    border = ~core & (best != big)
    labels[border] = best[border]
    return labels


def census(coords, labels, voxel=VOXEL, eps=EPS, min_samples=MIN_SAMPLES):
    """{clusters, core, border, noise} of a labelled input"""
    n = len(coords)
    a, _ = neighbour_pairs(coords, voxel, eps)
    core = np.bincount(a, minlength=n) + 1 >= min_samples if n else np.zeros(0, bool)
    return {"clusters": int(labels.max()) + 1 if n else 0, "core": int(core.sum()),
            "border": int((~core & (labels >= 0)).sum()), "noise": int((labels < 0).sum())}


def boxes(coords, labels, k=None):
    """(counts int64 [k], lo int32 [k, 3], hi int32 [k, 3]) of the labels 0..k-1; a label without rows keeps count 0,
    lo INT_MAX and hi INT_MIN; labels outside 0..k-1 are left out"""
    coords, labels = np.asarray(coords).astype(np.int64), np.asarray(labels).astype(np.int64)
    if k is None:
        k = int(labels.max()) + 1 if len(labels) else 0
    k = max(int(k), 0)
    counts = np.zeros(k, np.int64)
    lo = np.full((k, 3), np.iinfo(np.int32).max, np.int64)
    hi = np.full((k, 3), np.iinfo(np.int32).min, np.int64)
    keep = (labels >= 0) & (labels < k)
    np.add.at(counts, labels[keep], 1)
    np.minimum.at(lo, labels[keep], coords[keep])
    np.maximum.at(hi, labels[keep], coords[keep])
    return counts, lo.astype(np.int32), hi.astype(np.int32)


# ------------------------------------------------------------------ inputs
def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def snake(n, lane=200):
    """n rows of a path of unit steps in the z = 0 plane, in path order: lanes of `lane` voxels along x, two voxels
    apart in y, joined at alternating ends by one voxel.  Rows i and j are within 1.2 voxels only when |i - j| <= 1"""
    i = np.arange(n)
    r, pos = i // (lane + 1), i % (lane + 1)
    along = np.minimum(pos, lane - 1)
    x = np.where(r % 2 == 0, along, lane - 1 - along)
    y = 2 * r + (pos == lane)
    return _i32(np.stack([x, y, np.zeros(n, np.int64)], axis=1))


def random_voxels(rng, n, box):
    """n distinct voxels of a box (bx, by, bz), in random order, from 0"""
    bx, by, bz = (int(b) for b in box)
    cells = rng.choice(bx * by * bz, n, replace=False)
    return np.stack([cells // (by * bz), (cells // bz) % by, cells % bz], axis=1)


def blob():
    return np.stack(np.meshgrid(np.arange(3), np.arange(2), np.arange(2), indexing="ij"), -1).reshape(-1, 3)


def straddle_side(n, ratio, mean=10.8):
    """edge of the cube in which n random voxels have `mean` neighbours within `ratio` voxels (sn_ref.lattice_case: 165
    rows in 40^3 at ratio 10)"""
    return max(int(round(ratio * (n * 4.18879 / mean) ** (1.0 / 3.0))), 1)


@functools.lru_cache(maxsize=None)
def sizes_rows(n=4097):
    """distinct voxels whose every prefix has about the same density: row i is drawn from a cube of 1000 * (i + 1)
    voxels (the first five of 5^3), about 4 neighbours within 10 voxels, so that min_samples 4 gives core, border and
    noise rows"""
    rng = np.random.default_rng([7, 12])
    m = 2 * n
    side = np.ceil((1000.0 * (np.arange(m) + 1)) ** (1.0 / 3.0))
    side[:5] = 5                                     # the first five within eps of each other: a cluster from n = 4 on
    pts = np.floor((rng.random((m, 3)) - 0.5) * side[:, None]).astype(np.int64)
    _, first = np.unique(pts, axis=0, return_index=True)
    pts = pts[np.sort(first)][:n]
    assert len(pts) == n
    return _i32(pts)


SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
SIZES_MIN_SAMPLES = 4
HIGH_Z = 239                       # 24 cells of 10 voxels; 240 makes 25 and more than 2^32 cells in all


def high_keys(z_top=HIGH_Z):
    """four blobs at the corners of x, y in [-65535, 65535], z in [0, z_top], and 200 isolated rows between them"""
    rng = np.random.default_rng([9, 12])
    b = blob()
    lo, hi = -65535, 65535
    corners = [b + [lo, lo, 0], b + [hi - 2, lo, z_top - 1], b + [lo, hi - 1, z_top - 1], b + [hi - 2, hi - 1, z_top - 1]]
    cells = rng.choice(120 * 120, 200, replace=False)          # a 1000-voxel pitch: nothing within 10 voxels
    iso = np.stack([-60000 + 1000 * (cells // 120), -60000 + 1000 * (cells % 120), rng.integers(0, HIGH_Z + 1, 200)], axis=1)
    pts = np.concatenate(corners + [iso])
    return _i32(pts[rng.permutation(len(pts))])


def _ratio_rows(seed, ratio, n=4000):
    rng = np.random.default_rng([seed, 12])
    if ratio < 1:                                    # every voxel is alone: any distinct rows
        return random_voxels(rng, n, (20, 20, 20)) - 10
    if ratio < 2:                                    # 6 face neighbours: 69 % of an 18^3 cube, 5.1 rows within eps
        return random_voxels(rng, n, (18, 18, 18)) - 9
    s = straddle_side(n, ratio)
    return random_voxels(rng, n, (s, s, s)) - s // 2


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (coords int32 [n, 3], voxel, eps, min_samples)}, fixed seeds; built once"""
    out = {}
    chain = snake(20003)
    out["chain_in_order-ms2"] = (chain, VOXEL, 0.06, 2)
    out["chain_in_order-ms3"] = (chain, VOXEL, 0.06, 3)
    out["chain_reversed-ms3"] = (_i32(chain[::-1]), VOXEL, 0.06, 3)
    # A reversed path is again a path in row order.  Here the even positions of the path take the rows of the first half
    # and the odd positions those of the second: no row of the first half has a smaller neighbour, every row of the
    # second half hangs under one of the first, and the ten thousand basins of two or three rows are left to the unions
    pos = np.arange(len(chain))
    rows = np.where(pos % 2 == 0, pos // 2, (len(chain) + 1) // 2 + pos // 2)
    out["chain_interleaved-ms3"] = (_i32(chain[np.argsort(rows)]), VOXEL, 0.06, 3)
    rng = np.random.default_rng([1, 12])
    long_chain = snake(100003)
    out["chain_permuted-ms2"] = (_i32(long_chain[rng.permutation(len(long_chain))] - [5000, 3000, 7]), VOXEL, 0.06, 2)
    rng = np.random.default_rng([2, 12])
    out["cube_ratio3"] = (_i32(random_voxels(rng, 32 ** 3, (32, 32, 32))), VOXEL, 0.15, 10)
    rng = np.random.default_rng([3, 12])
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 1, 3) * 40
    pts = (g + blob()[None]).reshape(-1, 3) - 200
    out["blobs1000"] = (_i32(pts[rng.permutation(len(pts))]), VOXEL, EPS, MIN_SAMPLES)
    rng = np.random.default_rng([4, 12])
    out["straddle60k"] = (_i32(random_voxels(rng, 60000, (285, 285, 285)) - 142), VOXEL, EPS, MIN_SAMPLES)
    # thin grids: the same mean of 10.8 rows within 10 voxels, in a plane (341^2) and on a line (7800)
    rng = np.random.default_rng([5, 12])
    slab = random_voxels(rng, 4000, (341, 341, 1)) + [-170, -170, 33]
    out["thin_slab_z"] = (_i32(slab), VOXEL, EPS, MIN_SAMPLES)
    for axis, name in enumerate("xyz"):
        box = [1, 1, 1]
        box[axis] = 7800
        line = random_voxels(rng, 4000, box) + [-21, 5, 40]
        line[:, axis] -= 3900
        out[f"thin_line_{name}"] = (_i32(line), VOXEL, EPS, MIN_SAMPLES)
    # cell sizes: eps / voxel = 0.6, 1.2, 3, 13, 100
    out["ratio0.6-ms1"] = (_i32(_ratio_rows(60, 0.6)), VOXEL, 0.03, 1)
    out["ratio0.6-ms2"] = (_i32(_ratio_rows(60, 0.6)), VOXEL, 0.03, 2)
    out["ratio1.2"] = (_i32(_ratio_rows(61, 1.2)), VOXEL, 0.06, 5)
    out["ratio3"] = (_i32(_ratio_rows(62, 3)), VOXEL, 0.15, MIN_SAMPLES)
    out["ratio13"] = (_i32(_ratio_rows(63, 13)), 0.02, 0.26, MIN_SAMPLES)
    out["ratio100"] = (_i32(_ratio_rows(64, 100)), VOXEL, 5.0, MIN_SAMPLES)
    out["high_keys"] = (high_keys(), VOXEL, EPS, MIN_SAMPLES)
    for n in SIZES:
        out[f"sizes{n}"] = (sizes_rows()[:n], VOXEL, EPS, SIZES_MIN_SAMPLES)
    return out


CASE_NAMES = tuple(["chain_in_order-ms2", "chain_in_order-ms3", "chain_reversed-ms3", "chain_interleaved-ms3", "chain_permuted-ms2",
                    "cube_ratio3",
                    "blobs1000", "straddle60k", "thin_slab_z", "thin_line_x", "thin_line_y", "thin_line_z", "ratio0.6-ms1",
                    "ratio0.6-ms2", "ratio1.2", "ratio3", "ratio13", "ratio100", "high_keys"] + [f"sizes{n}" for n in SIZES])
PERMUTED = ("blobs1000", "straddle60k", "chain_permuted-ms2")


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's labels of a case: computed once, shared, never written to"""
    c, voxel, eps, ms = cases()[name]
    labels = dbscan(c, voxel, eps, ms)
    labels.setflags(write=False)
    return labels


@functools.lru_cache(maxsize=None)
def permuted(name):
    """(coords, labels) of one further row permutation of a case"""
    c, voxel, eps, ms = cases()[name]
    c = _i32(c[np.random.default_rng([len(name), 99]).permutation(len(c))])
    labels = dbscan(c, voxel, eps, ms)
    labels.setflags(write=False)
    return c, labels


def synthetic_labels(k, n=100003):
    """(coords int32 [n, 3], labels int32 [n]): random rows with coordinates up to +-65535, labels -1..k-1 with every
    fifth label left without rows when k > 4, and the extreme coordinates present"""
    rng = np.random.default_rng([k, 13])
    coords = rng.integers(-65535, 65536, (n, 3))
    coords[0], coords[n - 1] = -65535, 65535
    labels = rng.integers(-1, k, n)
    if k > 4:
        labels[(labels >= 0) & (labels % 5 == 3)] = -1
    labels[0], labels[n - 1] = 0, k - 1 if (k <= 4 or (k - 1) % 5 != 3) else 0
    return _i32(coords), _i32(labels)
