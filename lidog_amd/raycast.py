"""The Raycast baseline (configs/raycast/*): a source scan re-sampled so that it looks as if the target's sensor had
recorded it, as a point-splat range image on the GPU (csrc/raycast.hip, lidog_raycast).

  SensorSpec, SENSORS, sensor      a target sensor: beam elevations, azimuth columns, range limits; the built-in ones (one
                                   per synth.CONFIGS entry, `hdl32e`) or a JSON file
  origin_between                   the target sensor's position in the source frame for two synthetic configurations
  raycast_points, raycast_scan     the resampler on device tensors / on the scan dict of scans.load_scan
  write_fake, main                 `python -m lidog_amd.raycast`: a "Fake" dataset on disk, in the layout the reference's
                                   utils/datasets/fake_{kitti,synth4d}.py read (scans.FORMATS Fake*)

Every cell of the target's (beam, azimuth) grid keeps the nearest source point that falls into it.  Points are splatted,
not surfaces: a denser target sensor leaves cells empty.  Occlusion is resolved per cell only.  `origin` is a translation
only.  The reference ships the readers of such data and no generator; the HDL-64E's non-uniform beam table is not
shipped here either: pass it as a JSON file.
"""
import argparse
import json
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib, synth
from ._lib import call, ptr


@dataclass(frozen=True, eq=False)
class SensorSpec:
    """elevations: float64 radians, strictly ascending, at least 2 beams; n_az azimuth columns, column 0 centred on az0;
    points nearer than min_range or at / beyond max_range (None: no limit) are dropped"""
    elevations: np.ndarray
    n_az: int
    az0: float = 0.0
    min_range: float = 0.0
    max_range: float = None
    name: str = "sensor"
    _tables: dict = field(default_factory=dict, repr=False, compare=False)

    def __post_init__(self):
        el = np.ascontiguousarray(np.asarray(self.elevations, dtype=np.float64).reshape(-1))
        object.__setattr__(self, "elevations", el)
        object.__setattr__(self, "n_az", int(self.n_az))
        if el.shape[0] < 2 or not np.all(np.isfinite(el)) or not np.all(np.diff(el) > 0):
            raise ValueError(f"{self.name}: elevations must be at least 2 finite, strictly ascending angles")
        if el[0] < -np.pi / 2 or el[-1] > np.pi / 2:
            raise ValueError(f"{self.name}: elevations outside [-pi/2, pi/2] (radians)")
        if self.n_az < 1 or el.shape[0] * self.n_az >= 2 ** 31 - 1:
            raise ValueError(f"{self.name}: n_az = {self.n_az}")
        if not (abs(float(self.az0)) <= 2 * np.pi):
            raise ValueError(f"{self.name}: az0 = {self.az0} outside [-2 pi, 2 pi]")
        if not (float(self.min_range) >= 0) or (self.max_range is not None
                                                and not (float(self.max_range) > float(self.min_range))):
            raise ValueError(f"{self.name}: min_range = {self.min_range}, max_range = {self.max_range}")

    @property
    def n_beams(self):
        return self.elevations.shape[0]

    @property
    def n_cells(self):
        return self.n_beams * self.n_az

    def edges(self):
        """float64 [n_beams + 1]: interior edges are the midpoints between neighbouring beams, the outer ones lie half
        the first / last gap beyond the first / last beam"""
        el = self.elevations
        mid = (el[:-1] + el[1:]) / 2
        return np.concatenate([[el[0] - (el[1] - el[0]) / 2], mid, [el[-1] + (el[-1] - el[-2]) / 2]])

    def azimuths(self):
        """float64 [n_az]: the centre of every column"""
        return self.az0 + np.arange(self.n_az) * (2 * np.pi / self.n_az)

    def host_tables(self):
        """(edges, cos_el, sin_el, cos_az, sin_az) float64, made by numpy: the device evaluates no transcendental for
        positions"""
        az = self.azimuths()
        return self.edges(), np.cos(self.elevations), np.sin(self.elevations), np.cos(az), np.sin(az)

    def device_tables(self, device):
        key = str(torch.device(device))
        if key not in self._tables:
            self._tables[key] = tuple(torch.from_numpy(np.ascontiguousarray(t)).to(device) for t in self.host_tables())
        return self._tables[key]

    def to_json(self):
        d = {"elevations_deg": np.rad2deg(self.elevations).tolist(), "elevations_rad": self.elevations.tolist(),
             "n_az": self.n_az, "az0": float(self.az0), "min_range": float(self.min_range), "name": self.name}
        if self.max_range is not None:
            d["max_range"] = float(self.max_range)
        return d


def _config_sensor(name):
    cfg = synth.CONFIGS[name]
    return SensorSpec(np.deg2rad(np.linspace(cfg["elev"][0], cfg["elev"][1], cfg["n_beams"])), cfg["n_az"], name=name)


SENSORS = {name: _config_sensor(name) for name in synth.CONFIGS}
# the Velodyne HDL-32E's data sheet: 32 beams from -30.67 to +10.67 degrees, uniformly spaced
SENSORS["hdl32e"] = SensorSpec(np.deg2rad(np.linspace(-30.67, 10.67, 32)), 1090, name="hdl32e")


def sensor_from_json(path):
    """{"elevations_deg": [...], "n_az": ..., "az0", "min_range", "max_range", "name"}; `elevations_rad`, when present,
    takes precedence (what SensorSpec.to_json writes: the radians themselves, so a round trip is exact)"""
    with open(path) as f:
        d = json.load(f)
    if not isinstance(d, dict) or "n_az" not in d or not ("elevations_deg" in d or "elevations_rad" in d):
        raise ValueError(f"{path}: a sensor file needs 'elevations_deg' and 'n_az'")
    el = np.asarray(d["elevations_rad"], dtype=np.float64) if "elevations_rad" in d else \
        np.deg2rad(np.asarray(d["elevations_deg"], dtype=np.float64))
    return SensorSpec(el, d["n_az"], az0=float(d.get("az0", 0.0)), min_range=float(d.get("min_range", 0.0)),
                      max_range=d.get("max_range"), name=str(d.get("name", os.path.splitext(os.path.basename(path))[0])))


def sensor(name_or_json_path):
    """a built-in sensor by name (SENSORS), or the sensor of a JSON file"""
    if isinstance(name_or_json_path, SensorSpec):
        return name_or_json_path
    if name_or_json_path in SENSORS:
        return SENSORS[name_or_json_path]
    if os.path.isfile(name_or_json_path):
        return sensor_from_json(name_or_json_path)
    raise ValueError(f"sensor {name_or_json_path!r}: one of {sorted(SENSORS)} or a JSON file (the HDL-64E's "
                     "non-uniform beam table is not shipped: write it as {\"elevations_deg\": [...], \"n_az\": ...})")


def origin_between(source_config, target_config):
    """the target sensor's position in the source sensor's frame for two synth.CONFIGS entries: both stand over the
    same ground point at their own heights"""
    return np.array([0.0, 0.0, synth.CONFIGS[target_config]["h"] - synth.CONFIGS[source_config]["h"]], dtype=np.float32)


def _origin(origin, device):
    if origin is None:
        return None
    if torch.is_tensor(origin):
        o = origin.to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    else:
        o = torch.from_numpy(np.ascontiguousarray(np.asarray(origin, dtype=np.float32).reshape(-1))).to(device)
    if o.shape[0] != 3:
        raise ValueError("origin must have 3 components")
    return o


def _launch(points, spec, origin, snap, return_cells):
    """lidog_raycast on the current stream -> (points_out [cap, 3], rows [cap], cells or None, m int32 [1]); nothing is
    read back"""
    _lib.require_gpu(points, "points")
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"raycast: points must be float32 [n, 3], not {points.dtype} {tuple(points.shape)}")
    points = points.contiguous()
    dev = points.device
    n = points.shape[0]
    cap = min(n, spec.n_cells)
    edges, cos_el, sin_el, cos_az, sin_az = spec.device_tables(dev)
    origin = _origin(origin, dev)
    out = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    rows = torch.empty(cap, dtype=torch.int32, device=dev)
    cells = torch.empty(n, dtype=torch.int32, device=dev) if return_cells else None
    m = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().lidog_raycast_ws(n, spec.n_cells), dtype=torch.int32, device=dev) if n else None
    min2 = float(np.float32(float(spec.min_range) ** 2))
    max2 = float(np.float32(float(spec.max_range) ** 2)) if spec.max_range is not None else 0.0
    call("lidog_raycast", ptr(points), n, ptr(origin), ptr(edges), spec.n_beams, spec.n_az, float(spec.az0), min2,
         1 if spec.max_range is not None else 0, max2, 1 if snap else 0, ptr(cos_el), ptr(sin_el), ptr(cos_az),
         ptr(sin_az), ptr(cells), ptr(out), ptr(rows), ptr(m), ptr(ws))
    return out, rows, cells, m


def raycast_points(points, spec, origin=None, snap=True, return_cells=False):
    """points float32 [n, 3] on the GPU resampled to `spec` (a SensorSpec, a name or a JSON file) as seen from `origin`
    (float32 [3], the target sensor's position in the points' frame; None: 0).  Returns (points_out float32 [m, 3] in
    ascending cell order, rows int32 [m]: the winning source row of every output point[, cells int32 [n]: the cell of
    every source row, -1 for a dropped one]).  snap: every winner is placed on its cell's ray, as a ray cast does;
    otherwise points_out = (points - origin)[rows].  One device -> host read: m."""
    spec = sensor(spec)
    out, rows, cells, m = _launch(points, spec, origin, snap, return_cells)
    m = int(m.cpu())
    return (out[:m], rows[:m], cells) if return_cells else (out[:m], rows[:m])


def raycast_scan(scan, spec, origin=None, snap=True):
    """The scan dict of scans.load_scan / data.augment_item (`points`, `features`, `sem_labels`) resampled: labels follow
    `rows`, features are ones; `rows` int32 [m] is added.  Runs on the current stream (the callers are on
    data.merge_stream); one device -> host read: m."""
    for k in ("points", "sem_labels"):
        if k not in scan:
            raise KeyError(f"scan has no '{k}'")
    pts, rows = raycast_points(scan["points"], spec, origin, snap)
    _lib.require_gpu(scan["sem_labels"], "scan 'sem_labels'")
    return {"points": pts, "features": torch.ones((pts.shape[0], 1), dtype=torch.float32, device=pts.device),
            "sem_labels": scan["sem_labels"][rows.long()], "rows": rows}


# ------------------------------------------------------------------ "Fake" datasets on disk
FAKE_OF = {"SemanticKITTI": "FakeKITTI", "Synth4D-kitti": "FakeSynth4D-kitti", "Synth4D-nuscenes": "FakeSynth4D-nuscenes"}


def resample_file(points, labels_raw, spec, origin=None, snap=True, device="cuda"):
    """the device part of the writer: points float32 [n, 3] and the raw label words [n] of one file (numpy) ->
    (points_out float32 [m, 3], labels_out [m] of the labels' dtype), the labels gathered by `rows` on the device"""
    dev = torch.device(device)
    pts, rows = raycast_points(torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(dev), spec, origin,
                               snap)
    lab = torch.from_numpy(np.ascontiguousarray(labels_raw)).to(dev)[rows.long()]
    return pts.cpu().numpy(), lab.cpu().numpy()


def fake_paths(name, out_dir, points_path):
    """where the resampled scan of `points_path` (a file of dataset `name`) goes under out_dir: SemanticKITTI keeps
    sequences/SS/{velodyne,labels}/NNNNNN.{bin,label}; Synth4D's <town>/velodyne/<id>.npy becomes
    <town>/{velodyne,labels}/<id:06d>.{bin,label} (fake_synth4d.py: str(f).zfill(6))"""
    folder, base = os.path.split(os.path.normpath(points_path))
    group = os.path.basename(os.path.dirname(folder))        # the sequence, or the town
    stem = os.path.splitext(base)[0]
    if name == "SemanticKITTI":
        root = os.path.join(out_dir, "sequences", group)
    else:
        root, stem = os.path.join(out_dir, group), stem.zfill(6)
    return os.path.join(root, "velodyne", stem + ".bin"), os.path.join(root, "labels", stem + ".label")


def write_fake(listing, spec, out_dir, origin=None, snap=True, device="cuda"):
    """Every scan of a scans.Listing (SemanticKITTI or Synth4D) resampled to `spec` and written as a Fake dataset: points
    as float32 x, y, z, 0; labels the RAW label word of the winning point, int32, or uint8 for Synth4D-nuscenes (the
    reference's reader reads int8 there: a raw id above 127 raises ValueError).  A scan without a label file gets
    none, as the reference's reader expects.  Returns the number of files written."""
    from . import scans
    if listing.name not in FAKE_OF:
        raise ValueError(f"a Fake dataset is written from one of {tuple(FAKE_OF)}, not {listing.name}")
    spec = sensor(spec)
    small = listing.name == "Synth4D-nuscenes"
    for points_path, labels_path in listing.files:
        pts, labels, stride = scans.read_files(listing.format, points_path, labels_path)
        pts = pts.view(np.float32).reshape(-1, stride)[:, :3] if pts.dtype == np.uint8 else pts[:, :3]
        have = labels is not None
        if not have:
            labels = np.zeros(pts.shape[0], dtype=np.int32)
        if labels.shape[0] != pts.shape[0]:
            raise ValueError(f"{points_path}: points and labels have shape {pts.shape[0]} and {labels.shape[0]}")
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        out_p, out_l = resample_file(pts, labels, spec, origin, snap, device)
        if small:
            if out_l.size and (int(out_l.max()) > 127 or int(out_l.min()) < 0):
                raise ValueError(f"{labels_path}: raw label {int(out_l.max())} does not fit the int8 the reference's "
                                 "FakeSynth4D-nuscenes reader reads")
            out_l = out_l.astype(np.uint8)
        p_out, l_out = fake_paths(listing.name, out_dir, points_path)
        os.makedirs(os.path.dirname(p_out), exist_ok=True)
        os.makedirs(os.path.dirname(l_out), exist_ok=True)
        rec = np.zeros((out_p.shape[0], 4), dtype=np.float32)
        rec[:, :3] = out_p
        rec.tofile(p_out)
        if have:
            out_l.tofile(l_out)
    return len(listing.files)


def parse_args(argv=None):
    from . import scans
    ap = argparse.ArgumentParser(description="write a Fake dataset: every scan resampled to a target sensor")
    ap.add_argument("--files", required=True, metavar="NAME=PATH", help=f"the source dataset, NAME one of {tuple(FAKE_OF)}")
    ap.add_argument("--raycast-to", required=True, metavar="NAME|FILE.json",
                    help=f"the target sensor: one of {sorted(SENSORS)} or a JSON file")
    ap.add_argument("--raycast-origin", nargs=3, type=float, default=None, metavar=("X", "Y", "Z"),
                    help="the target sensor's position in the source frame (default 0 0 0)")
    ap.add_argument("--no-snap", action="store_true", help="keep the winners where they are instead of on their cell's ray")
    ap.add_argument("--out", required=True, metavar="DIR")
    ap.add_argument("--phases", nargs="+", default=list(scans.PHASES), choices=list(scans.PHASES))
    ap.add_argument("--synth4d-splits", default=None, metavar="DIR")
    ap.add_argument("--version", default="full", choices=["full", "mini"], help="SemanticKITTI split")
    ap.add_argument("--limit-files", type=int, default=None, metavar="N", help="first N files of every listing")
    a = ap.parse_args(argv)
    name, sep, path = a.files.partition("=")
    if not sep or not path or name not in FAKE_OF:
        ap.error(f"--files: {a.files!r}: expected NAME=PATH with NAME one of {tuple(FAKE_OF)}")
    if name.startswith("Synth4D") and a.synth4d_splits is None:
        ap.error("--files: a Synth4D entry needs --synth4d-splits")
    try:
        a.spec = sensor(a.raycast_to)
    except ValueError as e:
        ap.error(f"--raycast-to: {e}")
    a.files = (name, path)
    return a


def main(argv=None):
    from . import scans
    a = parse_args(argv)
    name, path = a.files
    for phase in a.phases:
        lst = scans.listing(name, path, phase, version=a.version, synth4d_splits=a.synth4d_splits, limit=a.limit_files)
        n = write_fake(lst, a.spec, a.out, origin=a.raycast_origin, snap=not a.no_snap)
        print(f"{FAKE_OF[name]} {phase}: {n} scans -> {a.out}")


if __name__ == "__main__":
    main()
