"""Synthetic LiDAR scans for benchmarks and parity tests (SURVEY.md 8(d) generator).

A spinning sensor at height h above a ground plane, 64 azimuth sectors each closed by a wall at a
random distance; points are the nearer of ground hit and wall hit plus range noise.  Scan i uses
seed i.  Voxelisation follows the dataset code (utils/datasets/semantickitti_bev.py:155-172,187,
232-238): drop points beyond 50 m, apply the bounds filter, floor(p / voxel), keep the first point of
every voxel; features are ones (use_intensity=False, :191-194); labels are uniform in [-1, 6].
"""
import os

import numpy as np
import torch

CONFIGS = {
    # name: beams, azimuths, elevation range (deg), sensor height, voxel size, bounds filter
    "kitti120k": dict(n_beams=64, n_az=1875, elev=(-24.8, 2.0), h=1.73, voxel=0.05, lidog_bounds=True),
    "source8k": dict(n_beams=16, n_az=500, elev=(-24.8, 2.0), h=1.73, voxel=0.1, lidog_bounds=False),
    "nusc35k": dict(n_beams=32, n_az=1090, elev=(-30.0, 10.0), h=1.84, voxel=0.05, lidog_bounds=False),
    "highres524k": dict(n_beams=128, n_az=4096, elev=(-24.8, 2.0), h=1.73, voxel=0.02, lidog_bounds=True),
    # the same sensors over a scene with parked cars (`cars`: size factor of the boxes): the scans of the SN car-size
    # scaling baseline (train_scaling_based.py), whose statistics need voxels labelled car (class 0)
    "kitti120k_cars": dict(n_beams=64, n_az=1875, elev=(-24.8, 2.0), h=1.73, voxel=0.05, lidog_bounds=True, cars=1.0,
                           dataset="SemanticKITTIDataset"),
    "nusc35k_cars": dict(n_beams=32, n_az=1090, elev=(-30.0, 10.0), h=1.84, voxel=0.05, lidog_bounds=False, cars=1.1,
                         dataset="NuScenesDataset"),
}
CAR_CLASS = 0


def car_boxes(seed, scale=1.0):
    """axis-aligned car-sized boxes resting on the ground, drawn from the scan's seed (a stream of its own: the scan's
    other draws do not move): 1 to 7 boxes, centre 5-14 m from the sensor, 3.8-5.0 x 1.6-2.0 x 1.4-1.8 m times `scale`,
    the long side along x or y.  Rows (cx, cy, half x, half y, height)."""
    rng = np.random.default_rng([int(seed), 0xCA5])
    n = int(rng.integers(1, 8))
    dist, ang = rng.uniform(5.0, 14.0, n), rng.uniform(0.0, 2 * np.pi, n)
    size = np.stack([rng.uniform(3.8, 5.0, n), rng.uniform(1.6, 2.0, n), rng.uniform(1.4, 1.8, n)], axis=1) * scale
    along_y = rng.random(n) < 0.35
    hx = np.where(along_y, size[:, 1], size[:, 0]) / 2
    hy = np.where(along_y, size[:, 0], size[:, 1]) / 2
    return np.stack([dist * np.cos(ang), dist * np.sin(ang), hx, hy, size[:, 2]], axis=1)


def _box_range(boxes, h, dirs):
    """range at which each ray (unit directions [..., 3] from the sensor at the origin, ground at z = -h) enters the
    nearest box (slab test), inf where it enters none"""
    best = np.full(dirs.shape[:-1], np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / dirs
        for cx, cy, hx, hy, height in boxes:
            lo = np.array([cx - hx, cy - hy, -h]) * inv
            hi = np.array([cx + hx, cy + hy, -h + height]) * inv
            t0 = np.nanmax(np.minimum(lo, hi), axis=-1)
            t1 = np.nanmin(np.maximum(lo, hi), axis=-1)
            best = np.where((t0 > 0) & (t0 <= t1), np.minimum(best, t0), best)
    return best


def scan_points(seed, n_beams, n_az, elev, h, **_):
    return _scan(seed, n_beams, n_az, elev, h)[:2]


def _scan(seed, n_beams, n_az, elev, h, boxes=None, details=False):
    """(points, the scan's generator after its draws, per point: hit a box); `details`: also per point (hit the ground,
    azimuth sector, beam)"""
    rng = np.random.default_rng(seed)
    el = np.deg2rad(np.linspace(elev[0], elev[1], n_beams))
    # evenly spaced azimuths (a spinning sensor fires at a fixed angular step): this is the generator behind the
    # per-stride voxel counts of SURVEY.md 8(d) / BASELINE.md (seed 0, kitti120k: 88 117 / 51 939 / 25 521 / 10 354 /
    # 3 777), asserted by tests/test_oracle_cpu.py::test_synth_matches_baseline_counts and by bench.py
    az = np.linspace(0.0, 2 * np.pi, n_az, endpoint=False)
    wall = rng.uniform(5.0, 50.0, 64)
    EL, AZ = np.meshgrid(el, az, indexing="ij")
    sector = np.minimum((AZ / (2 * np.pi) * 64).astype(np.int64), 63)
    r_wall = wall[sector] / np.cos(EL)
    with np.errstate(divide="ignore"):
        r_ground = np.where(EL < 0, h / np.sin(-EL), np.inf)
    r = np.minimum(r_ground, r_wall)
    car = np.zeros(EL.shape, dtype=bool)
    if boxes is not None:     # a box is hit before ground or wall
        dirs = np.stack([np.cos(EL) * np.cos(AZ), np.cos(EL) * np.sin(AZ), np.sin(EL)], axis=-1)
        r_box = _box_range(boxes, h, dirs)
        car = r_box < r
        r = np.minimum(r, r_box)
    r = r + rng.normal(0.0, 0.02, EL.shape)
    pts = np.stack([r * np.cos(EL) * np.cos(AZ), r * np.cos(EL) * np.sin(AZ), r * np.sin(EL)], axis=-1)
    pts = pts.reshape(-1, 3).astype(np.float32)
    keep = (pts ** 2).sum(axis=1) < 50.0 ** 2
    if details:
        ground = (r_ground < r_wall) & ~car
        beam = np.broadcast_to(np.arange(n_beams)[:, None], EL.shape)
        return pts[keep], rng, car.reshape(-1)[keep], (ground.reshape(-1)[keep], sector.reshape(-1)[keep],
                                                      beam.reshape(-1)[keep])
    return pts[keep], rng, car.reshape(-1)[keep]


GROUND_CLASS = 1
UNLABELLED_SHARE = 0.08     # of the (sector, band of 8 beams) patches of a scan


def scan_points_labels(seed, config="kitti120k"):
    """(points float32 [n,3], labels int64 [n]): the points of scan_points / scan_voxels of the same seed with one label
    per POINT, what the training augmentation starts from (it re-voxelises the points of every item).  Spatially
    coherent, so that the label vote of sparse_quantize leaves most voxels labelled: the ground is GROUND_CLASS, the
    wall of every azimuth sector has one class of its own (2..6, and 0 where the configuration has no cars), a box is
    CAR_CLASS, and UNLABELLED_SHARE of the (sector, band of 8 beams) patches are -1.  The labels are drawn from a
    generator stream of their own (as car_boxes): no other function's output moves."""
    cfg = CONFIGS[config]
    boxes = car_boxes(seed, cfg["cars"]) if cfg.get("cars") is not None else None
    pts, _, car, (ground, sector, beam) = _scan(seed, cfg["n_beams"], cfg["n_az"], cfg["elev"], cfg["h"], boxes=boxes,
                                                details=True)
    rng = np.random.default_rng([int(seed), 0x1AB])
    classes = np.array([2, 3, 4, 5, 6] if boxes is not None else [0, 2, 3, 4, 5, 6])
    wall_class = classes[rng.integers(0, len(classes), 64)]
    bands = (cfg["n_beams"] + 7) // 8
    unlabelled = rng.random((64, bands)) < UNLABELLED_SHARE
    labels = np.where(ground, GROUND_CLASS, wall_class[sector]).astype(np.int64)
    labels[car] = CAR_CLASS
    labels[unlabelled[sector, beam // 8]] = -1
    return pts, labels


def voxelize(pts, voxel, lidog_bounds, return_index=False):
    """`return_index`: also the row (of `pts`) of the first point of every voxel"""
    rows = np.arange(pts.shape[0])
    if lidog_bounds:
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        keep = (np.abs(x) < 60) & (np.abs(y) < 60) & (z > -10) & (z < 8) & ~((np.abs(x) < 3) & (np.abs(y) < 2))
        pts, rows = pts[keep], rows[keep]
    vox = np.floor(pts / np.float32(voxel)).astype(np.int32)
    _, first = np.unique(vox, axis=0, return_index=True)
    first = np.sort(first)
    return (vox[first], rows[first]) if return_index else vox[first]


# voxels per tensor stride 1/2/4/8/16 of scan seed 0
BASELINE_COUNTS = {
    "kitti120k": (88117, 51939, 25521, 10354, 3777),
    "source8k": (6948, 5033, 3205, 1691, 763),
    "highres524k": (460962, 302486, 144935, 58803, 20581),
    "nusc35k+mix3d": (51943, 37745, 25811, 14387, 6939),
}


def stride_counts(vox):
    """voxels at tensor stride 1, 2, 4, 8, 16 (floor division, as the strided coordinate maps)"""
    return (len(vox),) + tuple(len(np.unique(np.floor_divide(vox, s), axis=0)) for s in (2, 4, 8, 16))


def scan_voxels(seed, config="kitti120k"):
    """(coords int32 [n,3], labels int64 [n]) of synthetic scan `seed`"""
    cfg = CONFIGS[config]
    if cfg.get("cars") is not None:
        return _car_scan_voxels(seed, cfg)
    pts, rng = scan_points(seed, **cfg)
    vox = voxelize(pts, cfg["voxel"], cfg["lidog_bounds"])
    labels = rng.integers(-1, 7, vox.shape[0])
    return vox, labels


def _car_scan_voxels(seed, cfg):
    """a `_cars` configuration: a voxel whose first point hit a box is a car (class 0); every other voxel draws its
    label from -1, 1..6, so no other voxel is"""
    pts, rng, car = _scan(seed, cfg["n_beams"], cfg["n_az"], cfg["elev"], cfg["h"], boxes=car_boxes(seed, cfg["cars"]))
    vox, first = voxelize(pts, cfg["voxel"], cfg["lidog_bounds"], return_index=True)
    labels = rng.integers(-1, 6, vox.shape[0])
    labels[labels >= 0] += 1
    labels[car[first]] = CAR_CLASS
    return vox, labels


def mix3d_voxels(seed, config="nusc35k"):
    """Mix3D-style union of scans 2*seed and 2*seed+1, re-voxelised (utils/datasets/mix3D.py:44-87)"""
    a, la = scan_voxels(2 * seed, config)
    b, lb = scan_voxels(2 * seed + 1, config)
    vox = np.concatenate([a, b])
    lab = np.concatenate([la, lb])
    _, first = np.unique(vox, axis=0, return_index=True)
    first = np.sort(first)
    return vox[first], lab[first]


# scan seeds of a batch's second source start here (make_batch(seeds1=...)): the same configuration on both sources, as
# in the reference's single-dataset configs (['Synth4D-kitti', 'Synth4D-kitti']), still gives two different sets of scans
SOURCE1_SEED = 1 << 20


def make_batch(seeds, config="kitti120k", device="cpu", bev_size=167, mix3d=False, seeds1=None, config1=None):
    """Collated batch with the keys of CollateFNSingleSourceBEVMultiLevel (collation.py:318-325).
    `seeds1`: scan indices of a second source (configuration `config1`, default `config`; scan seed SOURCE1_SEED +
    index): adds the `source_*1` keys of CollateFNMultiSourceBEVMultiLevel (collation.py:328-418) and `coords_int1`."""
    coords, labels, bev, feats = _collate(seeds, config, device, bev_size, mix3d)
    batch = {"source_coordinates0": coords.float(), "source_features0": feats, "source_sem_labels0": labels,
             "source_bev_labels0": {"block8": bev}, "coords_int": coords}
    if seeds1 is not None:
        coords, labels, bev, feats = _collate([SOURCE1_SEED + int(s) for s in seeds1], config1 or config, device,
                                              bev_size, mix3d)
        batch.update({"source_coordinates1": coords.float(), "source_features1": feats, "source_sem_labels1": labels,
                      "source_bev_labels1": {"block8": bev}, "coords_int1": coords})
    return batch


def _collate(seeds, config, device, bev_size, mix3d):
    coords, labels = [], []
    for b, s in enumerate(seeds):
        v, l = (mix3d_voxels if mix3d else scan_voxels)(s, config)
        coords.append(np.concatenate([np.full((v.shape[0], 1), b, np.int32), v], axis=1))
        labels.append(l)
    coords, labels = np.concatenate(coords), np.concatenate(labels)
    coords = torch.from_numpy(coords).to(device)
    labels = torch.from_numpy(labels).long().to(device)
    rng = np.random.default_rng(1000003 + int(seeds[0]))
    bev = torch.from_numpy(rng.integers(-1, 7, (len(seeds), bev_size, bev_size))).long().to(device)
    feats = torch.ones((coords.shape[0], 1), dtype=torch.float32, device=device)
    return coords, labels, bev, feats
