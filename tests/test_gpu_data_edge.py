"""The oldest data-path kernels (lidog_voxel_floor, lidog_coords_insert / _compact as data.quantize_rows drives them,
lidog_label_vote, lidog_bev_label_raster with the host tables of data.label_luts) against the numpy yardstick of
tests/data_ref.py on the inputs LiDAR-shaped test data never produces: points ON the voxel boundaries, row counts
around every block size and capacity step and past the 262 144 rows where the scan carries across chunks, duplicates
far apart, votes decided by the first or the last point, empty scans, the ends of the look-up tables and of the strict
bounds, a wrapped pixel row, 10 000 points in one pixel, and inputs that must be refused.  Integer results: every
comparison is array_equal.  tests/test_data_ref_cpu.py holds the yardstick to the oracle and the reference's golden
images, and shows that each wrong rule it knows changes the result on an input used here."""
import functools

import numpy as np
import pytest
import torch

import data_ref as R

pytestmark = pytest.mark.gpu

RANGE_MESSAGE = "-65536 <= x, y, z <= 65535"
SENTINEL = -7


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(ref, got):
    got = got.cpu().numpy()
    return ref.shape == got.shape and np.array_equal(ref, got)


def _raw_floor(points, q, batch, pad=8):
    """lidog_voxel_floor through the C ABI into a buffer pre-filled with SENTINEL, `pad` rows longer than needed"""
    from lidog_amd._lib import call, ptr
    n = points.shape[0]
    q = np.broadcast_to(np.asarray(q, dtype=np.float32), (3,))
    rows = torch.full((n + pad, 4), SENTINEL, dtype=torch.int32, device="cuda")
    call("lidog_voxel_floor", ptr(_cuda(points)), n, float(q[0]), float(q[1]), float(q[2]), batch, ptr(rows))
    return rows


def _raw_quantize(rows, pad=64):
    """lidog_coords_insert + lidog_coords_compact as data.quantize_rows calls them, with unique_rows and inverse pre-filled
    with SENTINEL and `pad` entries longer than needed: (voxels, range flag, unique_rows, inverse)"""
    from lidog_amd._lib import call, load, ptr
    n = rows.shape[0]
    cap = load().lidog_hash_capacity(n)
    keys = torch.empty(cap, dtype=torch.int64, device="cuda")
    vals = torch.empty(cap, dtype=torch.int32, device="cuda")
    first = torch.full((n + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    sizes = torch.zeros(2, dtype=torch.int64, device="cuda")
    call("lidog_coords_insert", ptr(rows), n, ptr(keys), ptr(vals), cap, ptr(first), ptr(sizes[:1]), ptr(sizes[1:]))
    uniq = torch.full((n + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    inv = torch.full((n + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    ws = torch.empty(load().lidog_coords_compact_ws(n), dtype=torch.int32, device="cuda")
    call("lidog_coords_compact", ptr(first), n, ptr(keys), ptr(vals), cap, ptr(rows), ptr(uniq), ptr(inv), ptr(ws))
    m, bad = sizes.cpu().tolist()
    return m, bad, uniq, inv


# ------------------------------------------------------------------ voxel rows
@pytest.mark.timeout(60)
@pytest.mark.parametrize("name", list(R.GRID_Q))
def test_voxel_rows_on_the_grid(name):
    """float32(k q) for every k of the coordinate range, the largest float32 below each, +-0.0, denormals and both ends
    of the range: k_voxel_floor is a true float32 division (9 829 of these floor to k - 1, a multiply by 1 / q or a
    float64 division moves thousands of them), and the quantisation on top of it equals the yardstick's"""
    from lidog_amd.data import sparse_quantize
    q = R.GRID_Q[name]
    below = R.below_grid_points(q)
    below = below[R.in_range(R.voxel_rows(below, q))]
    for pts in (R.grid_points(q), below, R.special_points(q)):
        n = pts.shape[0]
        ref = R.voxel_rows(pts, q)
        got = _raw_floor(pts, q, batch=3).cpu().numpy()
        assert np.array_equal(got[:n, 1:], ref) and (got[:n, 0] == 3).all() and (got[n:] == SENTINEL).all()
        uniq, index, inverse = R.quantize(ref)
        c, i, v = sparse_quantize(_cuda(pts), quantization_size=q, return_index=True, return_inverse=True)
        assert c.dtype == torch.int32 and i.dtype == torch.int64 and v.dtype == torch.int64
        assert _same(uniq, c) and _same(index, i) and _same(inverse, v)


@pytest.mark.timeout(60)
def test_both_ends_of_the_range_are_accepted():
    """rows at -65536 and 65535 on every axis and batch 0 and 4095, duplicates included, through quantize_rows"""
    from lidog_amd.data import quantize_rows
    lo, hi = R.COORD_LO, R.COORD_HI
    rows = np.array([[0, lo, lo, lo], [R.BATCH_HI, hi, hi, hi], [0, lo, hi, 0], [R.BATCH_HI, 0, lo, hi], [0, lo, lo, lo],
                     [R.BATCH_HI, hi, hi, hi], [0, hi, lo, lo], [1, lo, lo, lo]], dtype=np.int32)
    uniq, index, inverse = R.quantize(rows)
    c, i, v = quantize_rows(_cuda(rows), return_index=True, return_inverse=True)
    assert _same(uniq[:, 1:], c) and _same(index, i) and _same(inverse, v) and index.shape[0] == 6


# ------------------------------------------------------------------ sizes
@pytest.mark.timeout(60)
@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_sizes(pattern, n):
    """every row its own voxel, one voxel, and about three rows per voxel far apart, at row counts around the wave, the
    256-thread block, the 1 024-row scan block, the capacity steps of the hash table and the 262 144 rows past which
    scan_block_offsets carries across chunks of 256 block sums"""
    from lidog_amd.data import quantize_rows
    rows = R.size_rows(n, pattern)
    feats, labels = R.size_columns(n)
    uniq, index, inverse = R.quantize(rows)
    voted = R.vote(labels, index, inverse, -1)
    m = index.shape[0]
    d_rows = _cuda(rows)
    got_m, bad, u1, v1 = _raw_quantize(d_rows)
    assert (got_m, bad) == (m, 0)
    assert _same(index.astype(np.int32), u1[:m]) and bool((u1[m:] == SENTINEL).all())       # past m: untouched
    assert _same(inverse.astype(np.int32), v1[:n]) and bool((v1[n:] == SENTINEL).all())
    _, _, u2, v2 = _raw_quantize(d_rows)
    assert torch.equal(u1, u2) and torch.equal(v1, v2)                                       # the same bytes twice
    c, f, l, i, v = quantize_rows(d_rows, _cuda(feats), _cuda(labels), -1, True, True)
    assert _same(uniq[:, 1:], c) and _same(feats[index], f) and _same(voted, l) and _same(index, i) and _same(inverse, v)
    assert torch.equal(d_rows[i][v], d_rows)
    assert _same(rows, d_rows)                                                               # the input is not written


# ------------------------------------------------------------------ label vote
@pytest.mark.timeout(60)
@pytest.mark.parametrize("ignore", [-1, -100, 255])
@pytest.mark.parametrize("dtype", ["int64", "int32"])
def test_label_vote(dtype, ignore):
    """a voxel whose first point carries ignore_label (with and without agreement), and a voxel of 600 points over twelve
    256-thread blocks whose very last point alone disagrees; a majority vote fails both"""
    from lidog_amd.data import quantize_rows
    rows, labels, named = R.vote_case(ignore)
    labels = labels.astype(dtype)
    uniq, index, inverse = R.quantize(rows)
    ref = R.vote(labels, index, inverse, ignore)
    c, got, i, v = quantize_rows(_cuda(rows), labels=_cuda(labels), ignore_label=ignore, return_index=True,
                                 return_inverse=True)
    assert got.dtype == getattr(torch, dtype)
    assert _same(uniq[:, 1:], c) and _same(index, i) and _same(inverse, v) and _same(ref, got)
    got = got.cpu().numpy()
    at = {k: int(np.nonzero(np.all(uniq[:, 1:] == xyz, axis=1))[0][0]) for k, xyz in named.items()}
    assert got[at["ignore_first_agree"]] == ignore and got[at["ignore_first_mixed"]] == ignore
    assert got[at["last_dissents"]] == ignore and got[at["unanimous"]] == 5


# ------------------------------------------------------------------ refusals
def _valid_points(n=5000, seed=11):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-50, 50, (n, 3)).astype(np.float32)
    pts[n // 2:] = pts[:n - n // 2] + np.float32(0.003)             # duplicates: the vote and the compaction have work
    return pts, rng.integers(-1, 7, n)


def _refused_points():
    pts, _ = _valid_points()
    n = pts.shape[0]
    out = {}
    for name, row in (("far_first", 0), ("far_middle", n // 2), ("far_last", n - 1)):
        p = pts.copy()
        p[row, row % 3] = -4000.0 if row else 4000.0                # |x| > 3 276.8 m at 5 cm voxels
        out[name] = p
    for name, value in (("nan", np.nan), ("plus_inf", np.inf), ("minus_inf", -np.inf), ("beyond_int32", 1e12),
                        ("overflowing_quotient", 3e38)):
        p = pts.copy()
        p[1234, 1] = value
        out[name] = p
    for name, p in R.past_the_ends(0.05).items():
        out[name] = np.concatenate([pts[:100], p, pts[100:200]])
    return out


def _assert_quantises(pts, labels):
    from lidog_amd.data import sparse_quantize
    uniq, index, inverse = R.quantize(R.voxel_rows(pts, 0.05))
    c, l, i, v = sparse_quantize(_cuda(pts), labels=_cuda(labels), ignore_label=-1, quantization_size=0.05,
                                 return_index=True, return_inverse=True)
    assert _same(uniq, c) and _same(R.vote(labels, index, inverse, -1), l) and _same(index, i) and _same(inverse, v)


# method="thread": a kernel that never ends blocks the read-back inside the HIP runtime, where no signal handler runs
@pytest.mark.timeout(60, method="thread")
@pytest.mark.parametrize("name", ["far_first", "far_middle", "far_last", "nan", "plus_inf", "minus_inf", "beyond_int32",
                                  "overflowing_quotient", "below_lo", "above_hi"])
def test_sparse_quantize_refuses_a_point_outside_the_range(name):
    """one point of 5 000 outside the range, or not finite: ValueError with the true range, not a kernel that probes an
    open-addressing table for a key that was never inserted, and not voxel 0 for a NaN; the next call is right"""
    from lidog_amd.data import sparse_quantize
    pts = _refused_points()[name]
    assert not R.in_range(R.voxel_rows(pts, 0.05)).all()
    with pytest.raises(ValueError, match=RANGE_MESSAGE):
        sparse_quantize(_cuda(pts), quantization_size=0.05, return_index=True, return_inverse=True)
    _assert_quantises(*_valid_points())


@pytest.mark.timeout(60, method="thread")
@pytest.mark.parametrize("batch", [4096, -1])
def test_quantize_rows_refuses_a_batch_index_outside_the_range(batch):
    from lidog_amd.data import quantize_rows
    rows = R.size_rows(5000, "triple")
    rows[2500, 0] = batch
    with pytest.raises(ValueError, match="0 <= batch <= 4095"):
        quantize_rows(_cuda(rows), return_index=True)
    _assert_quantises(*_valid_points())


@pytest.mark.timeout(60, method="thread")
@pytest.mark.parametrize("value", [4000.0, float("nan"), float("inf")], ids=["far", "nan", "inf"])
@pytest.mark.parametrize("ops", ["float32", "float64"])
def test_augment_item_refuses_a_point_outside_the_range(ops, value):
    """lidog_augment_points writes its voxel rows by the rule of lidog_voxel_floor, on its float32 path (no rotation in
    the list) and its float64 path (a rotation, here the identity): without the bounds filter such a point raises"""
    from lidog_amd.data import augment_item
    pts, labels = _valid_points()
    draws = {"sampled_idx": np.arange(pts.shape[0]),
             "ops": [] if ops == "float32" else [("RandomRotation", np.eye(3))]}
    scan = {"points": _cuda(pts), "features": torch.ones(pts.shape[0], 1, device="cuda"), "sem_labels": _cuda(labels)}
    good = augment_item(scan, draws, voxel_size=0.05, bounds=False)
    # the identity leaves the values as they are but makes them float64, and the floor follows the dtype
    rows = R.voxel_rows(pts, 0.05) if ops == "float32" else np.floor(pts.astype(np.float64) / 0.05).astype(np.int32)
    uniq, index, inverse = R.quantize(rows)
    assert _same(uniq, good["coordinates"]) and _same(index, good["index"]) and _same(inverse, good["inverse_map"])
    bad = pts.copy()
    bad[4321, 2] = value
    scan["points"] = _cuda(bad)
    with pytest.raises(ValueError, match=RANGE_MESSAGE):
        augment_item(scan, draws, voxel_size=0.05, bounds=False)
    torch.cuda.synchronize()
    _assert_quantises(pts, labels)


# ------------------------------------------------------------------ BEV label images
BEV_CASES = ("trailing_empty", "inferred", "all_ignored", "no_rows")


@functools.lru_cache(maxsize=None)
def _bev_case(bound, size, case):
    """(coords, labels, batch_size argument, yardstick images)"""
    coords, labels, _ = R.bev_batch(bound)                         # scans 0 and 2; scans 1 and 3 have no row
    B, batch_size = 4, 4
    if case == "inferred":
        B, batch_size = 3, None                                    # the largest batch index is 2
    elif case == "all_ignored":
        labels = np.full_like(labels, -1)
    elif case == "no_rows":
        coords, labels, B, batch_size = coords[:0], labels[:0], 2, 2
    return coords, labels, batch_size, R.bev_image(coords, labels, bound, size, R.BEV_VOXEL, B)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("case", BEV_CASES)
@pytest.mark.parametrize("bound,size", R.BEV_GEOMETRIES)
def test_bev_edge_batch(bound, size, case):
    """four scans of which the second and the last are empty (and the same rows with the number of scans inferred), every
    label -1, no row at all: voxels on and past the ends of the look-up tables, on the strict bounds in x, y and z, a line
    of voxels in the pixel row numpy wraps from -1 to S - 1, 20 000 rows in one pixel of which every second is labelled,
    point indices that count from the scan's own first row"""
    from lidog_amd.data import bev_labels
    coords, labels, batch_size, (ref_img, ref_idx) = _bev_case(bound, size, case)
    img, idx = bev_labels(_cuda(coords).reshape(-1, 4), _cuda(labels), bound=bound, img_size=size, voxel=R.BEV_VOXEL,
                          batch_size=batch_size)
    assert img.dtype == torch.int64 and idx.dtype == torch.int32
    for b in range(ref_img.shape[0]):
        assert _same(ref_img[b], img[b]) and _same(ref_idx[b], idx[b]), f"scan {b}"
    assert _same(ref_img, img) and _same(ref_idx, idx)
    if case in ("trailing_empty", "inferred"):
        assert (ref_img[0] >= 0).sum() > 1000 and (ref_img[2] >= 0).sum() > 1000 and (ref_img[1] == -1).all()
    else:
        assert (ref_img == -1).all()
    again = bev_labels(_cuda(coords).reshape(-1, 4), _cuda(labels), bound=bound, img_size=size, voxel=R.BEV_VOXEL,
                       batch_size=batch_size)
    assert torch.equal(again[0], img) and torch.equal(again[1], idx)
