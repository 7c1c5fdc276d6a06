"""A numpy restatement of the Raycast resampler's definition, with float64 angles, for the tests of
lidog_amd.raycast.  It takes any object with `elevations`, `n_az`, `az0`, `min_range`, `max_range` and builds its own
edges and tables, so it does not depend on SensorSpec's methods.

It also says, per point, whether the point is AMBIGUOUS: within TOL = 1e-9 rad of a column or row edge.  A double near
pi has an ulp of 4.4e-16 and the two libms' atan2 differ by a few ulp; 1e-9 leaves six orders of margin and excludes
practically only exact coincidences (a source azimuth that IS a target column edge).  `tainted` are the cells an
ambiguous point could enter: its own and the ones across every edge it is near."""
import functools
from types import SimpleNamespace

import numpy as np

TOL = 1e-9


def edges_of(elevations):
    el = np.asarray(elevations, dtype=np.float64)
    out = np.empty(el.shape[0] + 1, dtype=np.float64)
    out[1:-1] = (el[:-1] + el[1:]) / 2
    out[0] = el[0] - (el[1] - el[0]) / 2
    out[-1] = el[-1] + (el[-1] - el[-2]) / 2
    return out


def raycast_ref(points, spec, origin=None, snap=True):
    """-> SimpleNamespace(points [m,3] float32, rows [m] int32, cells [n] int32 (-1: dropped), out_cells [m] (the cell of
    every output row), ambiguous [n] bool, tainted (sorted unique cells an ambiguous point could enter), occupied)"""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    o = np.zeros(3, np.float32) if origin is None else np.asarray(origin, dtype=np.float32).reshape(3)
    q = (p - o[None, :]).astype(np.float32)
    qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
    r2 = ((qx * qx + qy * qy) + qz * qz).astype(np.float32)          # every product and sum rounded on its own
    el_tab = np.asarray(spec.elevations, dtype=np.float64)
    n_beams, n_az, az0 = el_tab.shape[0], int(spec.n_az), float(spec.az0)
    with np.errstate(invalid="ignore"):
        in_range = r2 > 0
        in_range &= ~(r2 < np.float32(float(spec.min_range) ** 2))
        if spec.max_range is not None:
            in_range &= ~(r2 >= np.float32(float(spec.max_range) ** 2))
        dx, dy, dz = qx.astype(np.float64), qy.astype(np.float64), qz.astype(np.float64)
        az = np.arctan2(dy, dx)
        el = np.arctan2(dz, np.sqrt(dx * dx + dy * dy))
        step = 2 * np.pi / n_az
        t = (az - az0) / step + 0.5
        edges = edges_of(el_tab)
        in_fov = (el >= edges[0]) & (el < edges[-1])
    keep = in_range & in_fov
    tk = np.where(keep, t, 0.0)
    c = np.mod(np.floor(tk).astype(np.int64), n_az)
    b = np.clip(np.searchsorted(edges, np.where(keep, el, edges[0]), side="right") - 1, 0, n_beams - 1)
    cells = np.where(keep, b * n_az + c, -1).astype(np.int32)

    # ambiguity: the distance to the nearest column edge (t an integer) and to the nearest row edge, in radians
    finite = in_range & np.isfinite(az) & np.isfinite(el)
    tf = np.where(finite, t, 0.25)
    elf = np.where(finite, el, 0.0)
    col_d = (tf - np.rint(tf)) * step                                # > 0: just inside the upper column
    k = np.clip(np.searchsorted(edges, elf), 1, n_beams)             # the two edges around el
    d_lo, d_hi = np.abs(elf - edges[k - 1]), np.abs(edges[k] - elf)
    row_near = np.where(d_lo <= d_hi, k - 1, k)
    row_amb = np.minimum(d_lo, d_hi) < TOL
    col_amb = np.abs(col_d) < TOL
    # a point outside the FOV by more than TOL enters no cell whatever its column
    outside = finite & ~row_amb & ~((elf >= edges[0]) & (elf < edges[-1]))
    ambiguous = finite & (col_amb | row_amb) & ~outside
    tainted = set()
    for i in np.flatnonzero(ambiguous):
        cf = int(np.floor(tf[i]))
        cols = {cf % n_az} | ({int(np.rint(tf[i])) % n_az, (int(np.rint(tf[i])) - 1) % n_az} if col_amb[i] else set())
        if row_amb[i]:
            e = int(row_near[i])                                     # rows on both sides of edge e
            rows_ = {r for r in (e - 1, e) if 0 <= r < n_beams}
        else:
            rows_ = {int(np.clip(np.searchsorted(edges, elf[i], side="right") - 1, 0, n_beams - 1))}
        tainted |= {r * n_az + cc for r in rows_ for cc in cols}
    tainted = np.array(sorted(tainted), dtype=np.int64)

    # winners: the smallest (bits(r2), row) of every cell, output in ascending cell order
    idx = np.flatnonzero(keep)
    key = (r2[idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    order = np.lexsort((key, cells[idx]))
    sc = cells[idx][order]
    first = np.ones(sc.shape[0], dtype=bool)
    first[1:] = sc[1:] != sc[:-1]
    rows = idx[order][first].astype(np.int32)
    out_cells = sc[first].astype(np.int64)
    if snap:
        azc = az0 + np.arange(n_az) * (2 * np.pi / n_az)
        cos_el, sin_el, cos_az, sin_az = np.cos(el_tab), np.sin(el_tab), np.cos(azc), np.sin(azc)
        ob, oc = out_cells // n_az, out_cells % n_az
        r = np.sqrt(dx[rows] * dx[rows] + dy[rows] * dy[rows] + dz[rows] * dz[rows])
        rc = r * cos_el[ob]
        out = np.stack([rc * cos_az[oc], rc * sin_az[oc], r * sin_el[ob]], axis=1).astype(np.float32)
    else:
        out = q[rows]
    return SimpleNamespace(points=np.ascontiguousarray(out.reshape(-1, 3)), rows=rows, cells=cells,
                           out_cells=out_cells, ambiguous=ambiguous, tainted=tainted,
                           occupied=int(out_cells.shape[0]))


def brute_force_winners(points, cells):
    """{cell: row} by a plain loop over the points: the smallest float32 r2 of the cell, the first row among equals"""
    p = np.asarray(points, dtype=np.float32)
    best = {}
    for i, cell in enumerate(np.asarray(cells)):
        if cell < 0:
            continue
        r2 = np.float32(np.float32(p[i, 0] * p[i, 0] + p[i, 1] * p[i, 1]) + p[i, 2] * p[i, 2])
        if cell not in best or r2 < best[cell][0]:
            best[int(cell)] = (r2, i)
    return {c: i for c, (_, i) in best.items()}


def spec_like(elevations, n_az, az0=0.0, min_range=0.0, max_range=None):
    return SimpleNamespace(elevations=np.asarray(elevations, dtype=np.float64), n_az=n_az, az0=az0, min_range=min_range,
                           max_range=max_range)


# the realistic cases of the GPU tests: (source configuration, target sensor), seed 0, origin_between
REALISTIC = (("kitti120k", "nusc35k"), ("nusc35k", "kitti120k"), ("kitti120k", "source8k"))
# the output points the restatement gives on the CPU
REALISTIC_COUNTS = {("kitti120k", "nusc35k"): 24787, ("nusc35k", "kitti120k"): 23980, ("kitti120k", "source8k"): 8000}
CAP = 0.01          # at most this share of the occupied cells may be excluded from the comparison of output rows


@functools.lru_cache(maxsize=None)
def realistic(source, target, snap=True):
    """(points float32 [n,3], labels int64 [n], spec, origin, the reference's result) of scan seed 0; computed once and
    shared: leave it unchanged"""
    from lidog_amd import raycast, synth
    pts, labels = synth.scan_points_labels(0, source)
    spec = raycast.sensor(target)
    origin = raycast.origin_between(source, target)
    return pts, labels, spec, origin, raycast_ref(pts, spec, origin, snap)


def sensor_8x125():
    """The 8-beam x 125-column sensor source8k scans are resampled to in the tests.  source8k fires at azimuths
    2 pi k / 500, and with az0 = 0 the column edges 2 pi (4 j + 2) / 500 of a 125-column sensor are exactly such
    azimuths: a quarter of the points would sit ON an edge, where the column is decided by the last bit of atan2 (the
    restatement marks a third of the occupied cells as enterable by an ambiguous point).  az0 = pi / 500 puts every
    edge midway between two source azimuths; the row edges never coincide (14 i = 30 j + 15 has no solution)."""
    from lidog_amd.raycast import SensorSpec
    return SensorSpec(np.deg2rad(np.linspace(-24.8, 2.0, 8)), 125, az0=np.pi / 500, name="beams8x125")
