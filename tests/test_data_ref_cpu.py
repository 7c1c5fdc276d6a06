"""The yardstick of tests/data_ref.py against what the suite already trusts (the oracle's sparse_quantize, the reference's
own BEV label images in tests/golden/g7_bev_labels.npz), the host tables of lidog_amd.data.label_luts against it over
their whole range, and the edge inputs of tests/test_gpu_data_edge.py against the conditions they are meant to meet:
each deliberately wrong variant of the yardstick must change the result on the named GPU case.  No GPU."""
import numpy as np
import pytest

import data_ref as R
from helpers import GOLDEN


# ------------------------------------------------------------------ 1. the yardstick against the oracle and the golden
def _oracle_inputs(seed, extra):
    from lidog_amd import synth
    pts, rng = synth.scan_points(seed, **synth.CONFIGS["source8k"])
    pts = np.concatenate([pts, pts[:extra] + np.float32(0.004)])
    labels = rng.integers(-1, 7, pts.shape[0])
    feats = rng.standard_normal((pts.shape[0], 2)).astype(np.float32)
    return pts, feats, labels


@pytest.mark.parametrize("q", [0.05, 0.1, (0.05, 0.1, 0.2)])
def test_yardstick_equals_the_oracles_sparse_quantize(q):
    """the inputs of test_sparse_quantize_matches_oracle (tests/test_gpu_data.py), all five outputs"""
    import oracle.me_cpu as OME
    pts, feats, labels = _oracle_inputs(3, 500)
    ref = OME.utils.sparse_quantize(pts, feats, labels=labels, ignore_label=-1, quantization_size=q,
                                    return_index=True, return_inverse=True)
    assert len(ref) == 5
    rows = R.voxel_rows(pts, q)
    uniq, index, inverse = R.quantize(rows)
    voted = R.vote(labels, index, inverse, -1)
    for r, g in zip(ref, (uniq, feats[index], voted, index, inverse)):
        assert np.array_equal(np.asarray(r), g)
    assert (voted == -1).sum() > (labels[index] == -1).sum()       # the vote really turned voxels to ignore
    assert np.array_equal(rows[index][inverse], rows)


@pytest.mark.parametrize("bound,size", R.BEV_GEOMETRIES)
def test_bev_image_equals_the_references_golden_images(bound, size):
    g7 = np.load(f"{GOLDEN}/g7_bev_labels.npz")
    tag = str(int(bound))
    vox, labels = g7[f"vox_{tag}"], g7[f"labels_{tag}"]
    coords = np.concatenate([np.zeros((vox.shape[0], 1), np.int32), vox], axis=1)
    img, idx = R.bev_image(coords, labels, bound, size, R.BEV_VOXEL, 1)
    assert img.shape == (1, size, size)
    assert np.array_equal(img[0], g7[f"img_{tag}"]) and np.array_equal(idx[0], g7[f"idx_{tag}"])
    assert (img >= 0).sum() > 1000


# ------------------------------------------------------------------ 2. the host tables against the yardstick
@pytest.mark.parametrize("bound,size,side", [(50.0, 167, 167), (30.0, 100, 100), (25.0, 83, 82)])
def test_label_luts_give_the_yardsticks_pixels_over_their_whole_range(bound, size, side):
    """every coordinate the tables hold, one axis at a time with the other two inside.  At (25, 83) the image side is
    int(50 / (50 / 83)) = 82, not 83: pinned here, because the tables, the kernels and the yardstick all size by it."""
    from lidog_amd.data import label_luts
    lut_x, lut_y, lut_z, lo, S = label_luts(bound, size, R.BEV_VOXEL)
    assert S == side == R.image_side(bound, size)
    assert lo == R.lut_lo(bound) and lut_x.shape[0] == -2 * lo == lut_y.shape[0] == lut_z.shape[0]
    c = np.arange(lo, -lo, dtype=np.int64)
    zero = np.zeros_like(c)
    px, _, keep = R.bev_pixels(np.stack([c, zero, zero], axis=1), bound, size, R.BEV_VOXEL)
    assert np.array_equal(lut_x, np.where(keep, px, -1))
    _, py, keep = R.bev_pixels(np.stack([zero, c, zero], axis=1), bound, size, R.BEV_VOXEL)
    assert np.array_equal(lut_y, np.where(keep, py, -1))
    _, _, keep = R.bev_pixels(np.stack([zero, zero, c], axis=1), bound, size, R.BEV_VOXEL)
    assert np.array_equal(lut_z, keep.astype(np.int32))
    assert (lut_x >= 0).sum() > 0 and lut_x.max() == S - 1 and lut_y.max() == S - 1
    assert lut_x[0] == lut_x[-1] == -1 and lut_z[0] == lut_z[-1] == 0       # the ends lie outside: 1.3 x the bound


def _lut_image(coords, labels, bound, size, B):
    """the rule of k_bev_label_winner / k_bev_label_fill restated on the host over label_luts' tables"""
    from lidog_amd.data import label_luts
    lut_x, lut_y, lut_z, lo, S = label_luts(bound, size, R.BEV_VOXEL)
    n_lut = lut_x.shape[0]
    img = np.full((B, S, S), -1, np.int64)
    idx = np.full((B, S, S), -1, np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(coords[:, 0], minlength=B))])
    for i in range(coords.shape[0]):
        b, ix, iy, iz = coords[i, 0], coords[i, 1] - lo, coords[i, 2] - lo, coords[i, 3] - lo
        if labels[i] == -1 or min(ix, iy, iz) < 0 or max(ix, iy, iz) >= n_lut:
            continue
        if lut_x[ix] < 0 or lut_y[iy] < 0 or lut_z[iz] == 0:
            continue
        j = i - start[b]
        if j > idx[b, lut_y[iy], lut_x[ix]]:
            idx[b, lut_y[iy], lut_x[ix]] = j
            img[b, lut_y[iy], lut_x[ix]] = labels[i]
    return img, idx


@pytest.mark.parametrize("bound,size", R.BEV_GEOMETRIES)
def test_table_driven_raster_equals_the_yardstick_on_the_edge_batch(bound, size):
    coords, labels, _ = R.bev_batch(bound)
    ref = R.bev_image(coords, labels, bound, size, R.BEV_VOXEL, 4)
    got = _lut_image(coords, labels, bound, size, 4)
    assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])


# ------------------------------------------------------------------ 3. the edge inputs meet their conditions
@pytest.mark.parametrize("name", list(R.GRID_Q))
def test_grid_points_sit_where_the_three_divisions_disagree(name):
    q = R.GRID_Q[name]
    pts = R.grid_points(q)
    rows = R.voxel_rows(pts, q)
    k = np.arange(R.COORD_LO, R.COORD_HI + 1)
    assert pts.shape == (131072, 3) and R.in_range(rows).all()
    assert np.isin(rows - k[:, None], (-1, 0)).all()
    assert ((rows[:, 0] == k - 1).sum()) >= 1000                   # float32 division floors float32(k q) to k - 1
    for variant in ("reciprocal", "float64", "trunc"):
        differ = np.any(R.voxel_rows(pts, q, variant) != rows, axis=1).sum()
        assert differ >= 1000, (variant, differ)
    if name == "scalar":        # the figures DESIGN.md section 4 quotes for this input
        assert (rows[:, 0] == k - 1).sum() == 9829
        assert (R.voxel_rows(pts, q, "reciprocal")[:, 0] != rows[:, 0]).sum() == 9829
        assert (R.voxel_rows(pts, q, "float64")[:, 0] != rows[:, 0]).sum() == 42600


@pytest.mark.parametrize("name", list(R.GRID_Q))
def test_points_below_the_grid_and_special_points(name):
    q = R.GRID_Q[name]
    below = R.below_grid_points(q)
    rows = R.voxel_rows(below, q)
    k = np.arange(R.COORD_LO, R.COORD_HI + 1)
    assert np.all(below < R.grid_points(q))
    ok = R.in_range(rows)
    assert (~ok).sum() == 1 and not ok[0]                          # only the point below the lowest boundary leaves
    assert ((rows[ok][:, 0] == k[ok] - 1).sum()) > 100000 and ((rows[ok][:, 0] == k[ok]).sum()) > 1000
    sp = R.special_points(q)
    srows = R.voxel_rows(sp, q)
    assert R.in_range(srows).all()
    assert np.array_equal(srows[:4], [[0, 0, 0], [0, 0, 0], [0, 0, 0], [-1, -1, -1]])     # +-0.0, +-denormal
    assert srows.min() == R.COORD_LO and srows.max() == R.COORD_HI                          # both ends are reached
    assert np.any(R.voxel_rows(sp, q, "trunc") != srows)
    for name_, p in R.past_the_ends(q).items():
        r = R.voxel_rows(p, q)
        assert not R.in_range(r).any()
        assert (r.min() == R.COORD_LO - 1) if name_ == "below_lo" else (r.max() == R.COORD_HI + 1)
    nonfinite = R.voxel_rows(np.float32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e38, 0, 0]]), q)
    assert not R.in_range(nonfinite).any()


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("n", R.SIZES)
def test_size_patterns(n, pattern):
    rows = R.size_rows(n, pattern)
    assert rows.shape == (n, 4) and rows.dtype == np.int32 and R.in_range(rows).all()
    uniq, index, inverse = R.quantize(rows)
    assert np.array_equal(rows[index][inverse], rows) and np.array_equal(uniq, rows[index])
    assert np.all(np.diff(index) > 0)                              # first-occurrence order
    assert np.array_equal(np.unique(rows, axis=0), uniq[np.lexsort(uniq.T[::-1])])
    m = {"distinct": n, "same": min(n, 1), "triple": -(-n // 3)}[pattern]
    assert index.shape[0] == m
    if n:                                                          # index = the smallest row of every voxel
        smallest = np.full(m, n, np.int64)
        np.minimum.at(smallest, inverse, np.arange(n))
        assert np.array_equal(smallest, index)
    if pattern == "triple" and n >= 262144:
        assert np.bincount(inverse).min() >= 2 and -(-n // 3) > 1024
    if pattern != "distinct" and n >= 2:       # the wrong rule shows on every size with a duplicate
        assert not np.array_equal(R.quantize(rows, "last")[1], index)


def test_sizes_cover_the_thresholds_of_the_kernels():
    cap = lambda n: max(1024, 1 << int(np.ceil(np.log2(max(2 * n, 1)))))
    assert cap(512) == 1024 and cap(513) == 2048 and cap(1024) == 2048 and cap(1025) == 4096
    assert {512, 513, 1024, 1025} <= set(R.SIZES)
    assert -(-262144 // 1024) == 256 and -(-262145 // 1024) == 257 and 263169 == 257 * 1024 + 1
    assert {262144, 262145, 263169} <= set(R.SIZES)


@pytest.mark.parametrize("ignore", [-1, -100, 255])
def test_vote_case(ignore):
    rows, labels, named = R.vote_case(ignore)
    uniq, index, inverse = R.quantize(rows)
    voted = R.vote(labels, index, inverse, ignore)
    at = {k: int(np.nonzero(np.all(uniq[:, 1:] == v, axis=1))[0][0]) for k, v in named.items()}
    assert labels[index[at["ignore_first_agree"]]] == ignore and voted[at["ignore_first_agree"]] == ignore
    assert labels[index[at["ignore_first_mixed"]]] == ignore and voted[at["ignore_first_mixed"]] == ignore
    assert voted[at["last_dissents"]] == ignore and voted[at["unanimous"]] == 5
    members = np.nonzero(inverse == at["last_dissents"])[0]
    assert members.shape[0] == 600 and members[-1] // 256 - members[0] // 256 >= 8
    assert np.all(labels[members[:-1]] == 2) and labels[members[-1]] == 4
    wrong = R.vote(labels, index, inverse, ignore, "majority")
    assert wrong[at["last_dissents"]] == 2 and wrong[at["ignore_first_mixed"]] == 3
    others = np.setdiff1d(np.arange(index.shape[0]), list(at.values()))
    assert np.array_equal(voted[others], labels[index[others]])    # single-point voxels keep their label


# ------------------------------------------------------------------ 4. the BEV edge batch meets its conditions
@pytest.mark.parametrize("bound,size", R.BEV_GEOMETRIES)
def test_bev_edge_batch(bound, size):
    coords, labels, groups = R.bev_batch(bound)
    S = R.image_side(bound, size)
    assert set(groups) == {0, 2} and coords[:, 0].max() == 2
    img, idx = R.bev_image(coords, labels, bound, size, R.BEV_VOXEL, 4)
    assert (img[1] == -1).all() and (img[3] == -1).all() and (idx[1] == -1).all() and (idx[3] == -1).all()
    lo = R.lut_lo(bound)
    for b in (0, 2):
        rows = np.nonzero(coords[:, 0] == b)[0]
        xyz, lab, g = coords[rows, 1:], labels[rows], groups[b]
        px, py, keep = R.bev_pixels(xyz, bound, size, R.BEV_VOXEL)
        ends = xyz[g["lut_ends"]]
        assert {lo - 1, lo, -lo - 1, -lo} <= set(ends.ravel().tolist()) and not keep[g["lut_ends"]].any()
        kept = keep[np.sort(g["bounds"])] if b == 0 else keep[np.sort(g["bounds"])][::-1]
        assert kept.tolist() == [False, True, True, False] * 2    # strict at +-bound, one voxel inside is kept
        zk = keep[np.sort(g["z_ends"])] if b == 0 else keep[np.sort(g["z_ends"])][::-1]
        assert zk.tolist() == [False, True, True, False]
        w = g["wrap_row"]
        raw = np.floor(np.float32(S) - ((xyz[w, 1] * R.BEV_VOXEL).astype(np.float32) + np.float32(bound))
                       / np.float32(2 * bound / size)).astype(np.int64) - 1
        assert (raw == -1).all() and keep[w].all() and (py[w] == S - 1).all() and w.shape[0] > 20
        one = np.sort(g["one_pixel"])
        assert one.shape[0] == 20000 and (lab[one] != -1).sum() == 10000 and keep[one].all()
        assert np.unique(px[one]).shape[0] == 1 and np.unique(py[one]).shape[0] == 1
        last = one[lab[one] != -1][-1]
        assert idx[b, py[last], px[last]] == last and img[b, py[last], px[last]] == lab[last]
        assert last != one[-1] or lab[one[-1]] != -1
        assert idx[b].max() > 3000                                 # indices count from the scan's own first row
    assert idx[2].max() < (coords[:, 0] == 2).sum()


# ------------------------------------------------------------------ 5. every wrong variant shows on a named GPU case
WRONG = [("trunc", "test_voxel_rows_on_the_grid[scalar]"),
         ("last", "test_sizes[triple-1025]"),
         ("majority", "test_label_vote[int64--1]"),
         ("first", "test_bev_edge_batch[50.0-167-trailing_empty]"),
         ("closed", "test_bev_edge_batch[50.0-167-trailing_empty]"),
         ("nowrap", "test_bev_edge_batch[50.0-167-trailing_empty]")]


@pytest.mark.parametrize("variant,gpu_case", WRONG)
def test_wrong_variant_differs_on_the_input_of_a_gpu_case(variant, gpu_case):
    """`gpu_case` names the test of tests/test_gpu_data_edge.py that runs the same input through the kernels (checked
    against that file's source, so a renamed test does not leave a stale name here)"""
    import os
    src = open(os.path.join(os.path.dirname(__file__), "test_gpu_data_edge.py")).read()
    assert f"def {gpu_case.split('[')[0]}(" in src
    if variant == "trunc":
        pts = R.grid_points(R.GRID_Q["scalar"])
        assert not np.array_equal(R.voxel_rows(pts, 0.05, variant), R.voxel_rows(pts, 0.05))
    elif variant == "last":
        rows = R.size_rows(1025, "triple")
        assert not np.array_equal(R.quantize(rows, variant)[1], R.quantize(rows)[1])
    elif variant == "majority":
        rows, labels, _ = R.vote_case(-1)
        _, index, inverse = R.quantize(rows)
        assert not np.array_equal(R.vote(labels, index, inverse, -1, variant), R.vote(labels, index, inverse, -1))
    else:
        coords, labels, groups = R.bev_batch(50.0)
        ref = R.bev_image(coords, labels, 50.0, 167, R.BEV_VOXEL, 4)
        bad = R.bev_image(coords, labels, 50.0, 167, R.BEV_VOXEL, 4, variant)
        assert not np.array_equal(ref[0], bad[0]) and not np.array_equal(ref[1], bad[1])
        if variant != "first":      # and it is the named group that shows it, not the bulk
            only = np.nonzero(coords[:, 0] == 0)[0][groups[0]["bounds" if variant == "closed" else "wrap_row"]]
            r1 = R.bev_image(coords[only], labels[only], 50.0, 167, R.BEV_VOXEL, 1)
            b1 = R.bev_image(coords[only], labels[only], 50.0, 167, R.BEV_VOXEL, 1, variant)
            assert not np.array_equal(r1[1], b1[1])
