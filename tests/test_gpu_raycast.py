"""The Raycast resampler on the GPU (csrc/raycast.hip through lidog_amd.raycast) against raycast_ref's numpy restatement
of the definition: the smallest shapes at which it can go wrong, then whole synthetic scans between the sensors of the
configurations.

What is compared how.  The cell of every source row equals the restatement's for every point that is not AMBIGUOUS
(within 1e-9 rad of a column or row edge, where the last bits of the two libms' atan2 decide: raycast_ref).  The output
rows are compared on the cells no ambiguous point could enter; such cells may be at most 1 % of the occupied cells or
the test fails (a condition on the case, asserted on the restatement alone in test_raycast_cpu.py as well).  Where
nothing is ambiguous, which is every case but nusc35k -> kitti120k, everything is compared with torch.equal: cells, rows
and points, snapped points included (float64 multiplies and square root are IEEE on both sides)."""
import numpy as np
import pytest
import torch

import raycast_ref as RR
from lidog_amd import raycast, synth

pytestmark = pytest.mark.gpu

FIVE = np.deg2rad([-25.0, -10.0, -4.0, 0.1, 3.0])            # a non-uniform table


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ray(az, el, r):
    az, el, r = np.broadcast_arrays(np.asarray(az, np.float64), np.asarray(el, np.float64), np.asarray(r, np.float64))
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=1).astype(np.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(pts, spec, origin=None, snap=True, ref=None, exact=True):
    """device against restatement; exact: nothing may be ambiguous and everything is compared.  Returns (ref, points_out,
    rows, cells) of the device."""
    ref = RR.raycast_ref(pts, spec, origin, snap) if ref is None else ref
    out, rows, cells = raycast.raycast_points(_cuda(pts), spec, origin, snap, return_cells=True)
    torch.cuda.synchronize()
    n = pts.shape[0]
    assert out.dtype == torch.float32 and rows.dtype == torch.int32 and cells.dtype == torch.int32
    assert out.shape == (rows.shape[0], 3) and cells.shape == (n,)
    sure = ~ref.ambiguous
    if exact:
        assert sure.all() and len(ref.tainted) == 0
    else:
        assert len(ref.tainted) <= RR.CAP * ref.occupied             # the cap: a condition, not a measurement
    got_cells = cells.cpu().numpy()
    assert np.array_equal(got_cells[sure], ref.cells[sure])
    got_rows, got_pts = rows.cpu().numpy(), out.cpu().numpy()
    got_out_cells = got_cells[got_rows].astype(np.int64)
    assert np.all(np.diff(got_out_cells) > 0)                         # ascending cell order, one row per cell
    keep_g, keep_r = ~np.isin(got_out_cells, ref.tainted), ~np.isin(ref.out_cells, ref.tainted)
    assert np.array_equal(got_out_cells[keep_g], ref.out_cells[keep_r])
    assert np.array_equal(got_rows[keep_g], ref.rows[keep_r])
    assert np.array_equal(got_pts[keep_g].view(np.uint32), ref.points[keep_r].view(np.uint32))
    if exact:
        assert rows.shape[0] == ref.occupied
    return ref, out, rows, cells


# ------------------------------------------------------------------ the smallest shapes
@pytest.mark.parametrize("snap", [True, False])
def test_empty_and_single(snap):
    spec = raycast.SensorSpec(FIVE, 7)
    out, rows, cells = raycast.raycast_points(torch.zeros((0, 3), device="cuda"), spec, snap=snap, return_cells=True)
    assert out.shape == (0, 3) and rows.shape == (0,) and cells.shape == (0,)
    ref, out, rows, _ = _check(_ray([1.0], [-0.17], [9.0]), spec, snap=snap)
    assert rows.tolist() == [0] and ref.occupied == 1
    _check(_ray([1.0], [0.5], [9.0]), spec, snap=snap)               # one point, outside: m = 0


def test_one_cell_takes_4096_points():
    spec = raycast.SensorSpec(np.deg2rad([-10.0, 0.0, 10.0]), 16)
    rng = np.random.default_rng(1)
    r = 5.0 + 0.001 * rng.permutation(4096)
    pts = _ray(0.1 + rng.uniform(-0.01, 0.01, 4096), rng.uniform(-0.01, 0.01, 4096), r)
    ref, _, rows, cells = _check(pts, spec)
    r2 = ((pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) + pts[:, 2] * pts[:, 2]).astype(np.float32)
    first = int(np.flatnonzero(r2 == r2.min())[0])
    assert rows.tolist() == [first] and cells.unique().tolist() == [16]
    same = np.repeat(_ray([0.1], [0.0], [7.0]), 4096, axis=0)        # all-equal r2: the smallest row
    _, _, rows, _ = _check(same, spec)
    assert rows.tolist() == [0]
    same = np.concatenate([_ray([0.1], [0.0], [7.5]), same])         # ... also when row 0 is not among them
    assert _check(same, spec)[2].tolist() == [1]


@pytest.mark.parametrize("n_beams,n_az", [(2, 1), (5, 1), (2, 3), (5, 64)])
def test_small_grids(n_beams, n_az):
    el = np.deg2rad([-8.0, 6.0]) if n_beams == 2 else FIVE
    spec = raycast.SensorSpec(el, n_az, az0=0.2, min_range=1.0, max_range=45.0)
    rng = np.random.default_rng([n_beams, n_az])
    pts = _ray(rng.uniform(-np.pi, np.pi, 1500), np.deg2rad(rng.uniform(-40, 20, 1500)), rng.uniform(0.2, 50.0, 1500))
    for snap in (True, False):
        ref, *_ = _check(pts, spec, snap=snap)
        assert 0 < ref.occupied <= n_beams * n_az and (ref.cells == -1).any()


def test_axis_origin_and_signed_zero():
    spec = raycast.SensorSpec(np.deg2rad([60.0, 85.0]), 8)           # the top edge lies beyond the zenith
    pts = np.array([[0, 0, 5.0], [0, 0, -5.0], [0, 0, 0], [-0.0, 0.0, 6.0], [1e-30, 0, 1e-30], [3.0, 0.0, 20.0]],
                   dtype=np.float32)
    ref, _, rows, cells = _check(pts, spec)
    assert cells.tolist() == [8, -1, -1, 12, -1, 8] and rows.tolist() == [0, 3]
    # the point at the origin of a shifted sensor, and NaN / infinite rows, enter no cell
    odd = np.array([[1, 2, 3], [np.nan, 0, 1], [0, np.nan, 1], [0, 1, np.nan], [np.inf, 0, 0], [2.0, 0.0, 6.0]],
                   dtype=np.float32)
    out, rows, cells = raycast.raycast_points(_cuda(odd), spec, origin=[1.0, 2.0, 3.0], return_cells=True)
    assert cells[:5].tolist() == [-1] * 5 and rows.tolist() == [5]


def test_everything_outside():
    spec = raycast.SensorSpec(np.deg2rad([-5.0, 0.0, 5.0]), 32, max_range=10.0)
    rng = np.random.default_rng(2)
    pts = np.concatenate([_ray(rng.uniform(-3, 3, 700), np.deg2rad(rng.uniform(9, 80, 700)), 5.0),
                          _ray(rng.uniform(-3, 3, 700), 0.0, rng.uniform(10.5, 90.0, 700))])
    ref, out, rows, cells = _check(pts, spec)
    assert out.shape == (0, 3) and rows.shape == (0,) and bool((cells == -1).all())


def test_origin_moves_points_across_rows():
    spec = raycast.SensorSpec(np.deg2rad([-15.0, -5.0, 5.0]), 90)
    pts = _ray(np.linspace(-3.0, 3.0, 257), np.deg2rad(2.0), 5.0)
    _, _, _, at_zero = _check(pts, spec)
    _, out, rows, lifted = _check(pts, spec, origin=np.array([0.0, 0.0, 1.0], np.float32))
    assert bool((at_zero // 90 == 2).all()) and bool((lifted // 90 == 1).all())
    _check(pts, spec, origin=torch.tensor([0.3, -0.2, 1.0]), snap=False)     # a tensor, sideways as well


@pytest.mark.parametrize("spec", [raycast.SensorSpec(FIVE, 333, az0=-0.4), raycast.SENSORS["hdl32e"]],
                         ids=["five_beams", "hdl32e"])
def test_ten_thousand_points_inside_their_cells(spec):
    """angles drawn at cell centres +- at most a quarter cell: nothing is ambiguous, everything is bit-equal"""
    rng = np.random.default_rng(7)
    n = 10000
    b, c = rng.integers(0, spec.n_beams, n), rng.integers(0, spec.n_az, n)
    edges = spec.edges()
    half = np.minimum(spec.elevations - edges[:-1], edges[1:] - spec.elevations)[b]
    el = spec.elevations[b] + rng.uniform(-0.5, 0.5, n) * half
    az = spec.azimuths()[c] + rng.uniform(-0.25, 0.25, n) * (2 * np.pi / spec.n_az)
    pts = _ray(az, el, rng.uniform(2.0, 40.0, n))
    for snap in (False, True):
        ref, out, rows, cells = _check(pts, spec, snap=snap)
        assert torch.equal(cells.cpu(), torch.from_numpy((b * spec.n_az + c).astype(np.int32)))
        assert torch.equal(rows.cpu(), torch.from_numpy(ref.rows)) and torch.equal(_bits(out).cpu(),
                                                                                   _bits(torch.from_numpy(ref.points)))
    assert ref.occupied < n                                           # cells were contested


# ------------------------------------------------------------------ whole scans, seed 0
@pytest.mark.parametrize("source,target", RR.REALISTIC)
def test_realistic_scans(source, target):
    pts, labels, spec, origin, ref = RR.realistic(source, target)
    _, out, rows, _ = _check(pts, spec, origin, ref=ref, exact=not ref.ambiguous.any())
    assert abs(rows.shape[0] - RR.REALISTIC_COUNTS[(source, target)]) <= len(ref.tainted)
    scan = {"points": _cuda(pts), "sem_labels": _cuda(labels), "features": torch.ones((pts.shape[0], 1), device="cuda")}
    got = raycast.raycast_scan(scan, spec, origin)
    assert set(got) == {"points", "features", "sem_labels", "rows"} and torch.equal(got["rows"], rows)
    assert torch.equal(_bits(got["points"]), _bits(out)) and got["sem_labels"].dtype == torch.int64
    assert torch.equal(got["sem_labels"].cpu(), torch.from_numpy(labels)[rows.cpu().long()])
    assert got["features"].shape == (rows.shape[0], 1) and bool((got["features"] == 1).all())
    again = raycast.raycast_points(_cuda(pts), spec, origin)         # run to run: the same bytes
    assert torch.equal(again[1], rows) and torch.equal(_bits(again[0]), _bits(out))


def test_source8k_to_the_8x125_sensor_and_identity():
    pts, _ = synth.scan_points_labels(0, "source8k")
    ref, _, rows, _ = _check(pts, RR.sensor_8x125())
    assert ref.occupied == 1000
    _, out, rows, _ = _check(pts, raycast.sensor("source8k"), snap=False)     # to its own sensor: every point
    assert torch.equal(rows.sort().values.cpu(), torch.arange(pts.shape[0], dtype=torch.int32))
    assert torch.equal(_bits(out).cpu(), _bits(torch.from_numpy(pts))[rows.cpu().long()])


def test_on_another_stream():
    pts, _, spec, origin, ref = RR.realistic("kitti120k", "source8k")
    want = raycast.raycast_points(_cuda(pts), spec, origin, return_cells=True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = _cuda(pts)
        got = raycast.raycast_points(dev, spec, origin, return_cells=True)
    side.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(_bits(g), _bits(w))
