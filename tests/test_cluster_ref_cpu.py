"""tests/cluster_ref.py, the DBSCAN restatement the GPU edge-case tests compare with, is itself tested here: against the
all-pairs restatement sn_ref.dbscan_np, against the sklearn labels recorded in G12 (up to 18 454 rows), against sklearn
where it imports, and by a census per case, so that no case passes while missing the path it is there for."""
import time

import numpy as np
import pytest

import cluster_ref
import sn_ref

META, G12 = sn_ref.load_g12()
LATTICE = sn_ref.lattice_cases(G12)
CAR_SCANS = [(k, s) for k, r in enumerate(META["stats"]) for s in r["scans"] if s["clustered"]]
SMALL = [n for n in cluster_ref.SIZES if n <= 1025]
SECONDS = 10.0                    # per case, on the CPU


def _labels(name):
    c, voxel, eps, ms = cluster_ref.cases()[name]
    return c, cluster_ref.expected(name), cluster_ref.census(c, cluster_ref.expected(name), voxel, eps, ms)


# ------------------------------------------------------------------ against the all-pairs restatement
def test_equals_dbscan_np_on_the_g12_lattice_and_edge_inputs():
    for coords, _, _ in LATTICE:
        np.testing.assert_array_equal(cluster_ref.dbscan(coords), sn_ref.dbscan_np(coords))
    for name, coords in sn_ref.edge_cases().items():
        np.testing.assert_array_equal(cluster_ref.dbscan(coords), sn_ref.dbscan_np(coords), err_msg=name)


def test_equals_dbscan_np_on_fresh_lattice_seeds():
    for seed in range(1000, 1050):
        coords = sn_ref.lattice_case(seed)
        np.testing.assert_array_equal(cluster_ref.dbscan(coords), sn_ref.dbscan_np(coords), err_msg=str(seed))


def test_equals_dbscan_np_on_other_parameters():
    coords, _, _ = LATTICE[1]
    for eps, ms, voxel in ((0.3, 4, 0.05), (0.5, 1, 0.05), (1.0, 10, 0.1), (0.26, 3, 0.02)):
        np.testing.assert_array_equal(cluster_ref.dbscan(coords, voxel, eps, ms), sn_ref.dbscan_np(coords, voxel, eps, ms),
                                      err_msg=str((eps, ms, voxel)))
    assert cluster_ref.dbscan(np.zeros((0, 3), np.int32)).shape == (0,)


@pytest.mark.parametrize("n", SMALL)
def test_equals_dbscan_np_on_the_sizes_inputs(n):
    c, voxel, eps, ms = cluster_ref.cases()[f"sizes{n}"]
    assert len(c) == n
    np.testing.assert_array_equal(cluster_ref.expected(f"sizes{n}"), sn_ref.dbscan_np(c, voxel, eps, ms))


# ------------------------------------------------------------------ against sklearn's recorded labels
def test_equals_the_recorded_sklearn_labels_of_the_lattice_and_edge_cases():
    assert len(LATTICE) == 44 and len(META["edge"]) == 4
    for coords, want, _ in LATTICE:
        np.testing.assert_array_equal(cluster_ref.dbscan(coords), want)
    for name in META["edge"]:
        np.testing.assert_array_equal(cluster_ref.dbscan(sn_ref.edge_cases()[name]), G12[f"edge_{name}_labels"], err_msg=name)


@pytest.mark.parametrize("case", CAR_SCANS,
                         ids=[f"{META['stats'][k]['dataset']}-seed{META['stats'][k]['seed']}-scan{s['scan']}" for k, s in CAR_SCANS])
def test_equals_the_recorded_sklearn_labels_of_the_car_scans(case):
    k, s = case
    car = sn_ref.car_voxels(META["stats"][k]["dataset"], s["scan"])
    assert car.shape[0] == s["car_voxels"]
    got = cluster_ref.dbscan(car)
    np.testing.assert_array_equal(got, G12[f"s{k}_{s['slot']}_labels"])
    assert sn_ref.digest(got.astype(np.int16)) == s["labels_sha1"]
    for a, name in zip(cluster_ref.boxes(car, got), ("counts", "lo", "hi")):
        np.testing.assert_array_equal(a, G12[f"s{k}_{s['slot']}_{name}"])


def test_there_are_19_car_scans():
    assert len(CAR_SCANS) == 19 and max(s["car_voxels"] for _, s in CAR_SCANS) == 18454


# ------------------------------------------------------------------ against sklearn itself
@pytest.mark.parametrize("name", cluster_ref.CASE_NAMES)
def test_equals_sklearn_on_every_case(name):
    DBSCAN = pytest.importorskip("sklearn.cluster").DBSCAN
    c, voxel, eps, ms = cluster_ref.cases()[name]
    want = DBSCAN(eps=eps, min_samples=ms).fit_predict(c.astype(np.float32) * np.float32(voxel))
    np.testing.assert_array_equal(cluster_ref.expected(name), want)


@pytest.mark.parametrize("name", cluster_ref.PERMUTED)
def test_equals_sklearn_on_the_permuted_cases(name):
    DBSCAN = pytest.importorskip("sklearn.cluster").DBSCAN
    _, voxel, eps, ms = cluster_ref.cases()[name]
    c, labels = cluster_ref.permuted(name)
    assert not np.array_equal(c, cluster_ref.cases()[name][0])
    np.testing.assert_array_equal(labels, DBSCAN(eps=eps, min_samples=ms).fit_predict(c.astype(np.float32) * np.float32(voxel)))


# ------------------------------------------------------------------ the cases reach what they are there for
def test_case_names_and_distinct_rows():
    assert set(cluster_ref.CASE_NAMES) == set(cluster_ref.cases())
    for name, (c, _, _, _) in cluster_ref.cases().items():
        assert c.dtype == np.int32 and c.ndim == 2 and c.shape[1] == 3 and np.abs(c).max() <= 65535, name
        assert len(np.unique(c, axis=0)) == len(c), name          # distinct rows: cluster.dbscan's contract


@pytest.mark.parametrize("name", cluster_ref.CASE_NAMES)
def test_restatement_finishes_in_time(name):
    c, voxel, eps, ms = cluster_ref.cases()[name]
    t = time.perf_counter()
    cluster_ref.dbscan(c, voxel, eps, ms)
    t = time.perf_counter() - t
    print(f"{name}: {len(c)} rows, {t:.2f} s")
    assert t < SECONDS


def test_census_chains():
    for name, n, border in (("chain_in_order-ms2", 20003, 0), ("chain_in_order-ms3", 20003, 2), ("chain_reversed-ms3", 20003, 2),
                            ("chain_interleaved-ms3", 20003, 2),
                            ("chain_permuted-ms2", 100003, 0)):
        c, labels, cen = _labels(name)
        assert len(c) == n and cen == {"clusters": 1, "core": n - border, "border": border, "noise": 0}, name
        assert (labels == 0).all()
    # the path: consecutive rows one voxel apart, and no other pair within 1.2 voxels (every row has at most 2 neighbours)
    c = cluster_ref.cases()["chain_in_order-ms2"][0].astype(np.int64)
    assert (np.abs(np.diff(c, axis=0)).sum(1) == 1).all() and (c[:, 2] == 0).all()
    a, b = cluster_ref.neighbour_pairs(c, 0.05, 0.06)
    assert len(a) == 2 * (len(c) - 1) and (np.abs(a - b) == 1).all()
    assert np.nonzero(np.bincount(a) + 1 < 3)[0].tolist() == [0, len(c) - 1]       # with min_samples 3 the ends are border rows
    assert np.array_equal(cluster_ref.cases()["chain_reversed-ms3"][0], c[::-1])
    assert cluster_ref.cases()["chain_permuted-ms2"][0].max() < 0
    # interleaved: no row of the first half has a smaller neighbour, every other row has one in the first half
    a, b = cluster_ref.neighbour_pairs(cluster_ref.cases()["chain_interleaved-ms3"][0], 0.05, 0.06)
    half = (len(c) + 1) // 2
    smallest = np.full(len(c), len(c))
    np.minimum.at(smallest, a, b)
    assert (smallest[:half] >= half).all() and (smallest[half:] < half).all()


def test_census_cube():
    c, labels, cen = _labels("cube_ratio3")
    assert len(c) == 32 ** 3 and cen["clusters"] == 1 and cen["noise"] == 0 and (labels == 0).all()
    keys, _ = cluster_ref.cell_keys(c, 0.05, 0.15)
    assert cluster_ref.cell_edge(0.05, 0.15) == 3 and np.bincount(keys).max() == 27


def test_census_blobs():
    c, labels, cen = _labels("blobs1000")
    assert cen == {"clusters": 1000, "core": 12000, "border": 0, "noise": 0}
    assert (np.bincount(labels) == 12).all()


def test_census_straddle():
    c, labels, cen = _labels("straddle60k")
    print(cen)
    assert len(c) == 60000 and cen["clusters"] >= 10 and cen["border"] >= 10000 and cen["noise"] >= 1000


@pytest.mark.parametrize("name", ["thin_slab_z", "thin_line_x", "thin_line_y", "thin_line_z", "ratio1.2", "ratio3", "ratio13",
                                  "ratio100", "sizes4097"])
def test_census_core_border_and_noise(name):
    c, labels, cen = _labels(name)
    print(name, cen)
    assert cen["clusters"] >= 2 and min(cen["core"], cen["border"], cen["noise"]) >= 100


def test_census_thin_grids_and_cell_sizes():
    for name, thin in (("thin_slab_z", [2]), ("thin_line_x", [1, 2]), ("thin_line_y", [0, 2]), ("thin_line_z", [0, 1])):
        c, voxel, eps, _ = cluster_ref.cases()[name]
        _, dims = cluster_ref.cell_keys(c, voxel, eps)
        assert all((dims[d] == 1) == (d in thin) for d in range(3)), (name, dims)
    # 0.26 / float32(0.02) is a little more than 13: the kernel, and cell_edge with it, take cells of 14 voxels
    edges = {name: cluster_ref.cell_edge(v, e) for name, (_, v, e, _) in cluster_ref.cases().items()}
    assert [edges[k] for k in ("ratio0.6-ms1", "ratio0.6-ms2", "ratio1.2", "ratio3", "ratio13", "ratio100")] == [1, 1, 2, 3, 14, 100]
    n = len(cluster_ref.cases()["ratio0.6-ms1"][0])
    np.testing.assert_array_equal(cluster_ref.expected("ratio0.6-ms1"), np.arange(n))
    np.testing.assert_array_equal(cluster_ref.expected("ratio0.6-ms2"), np.full(n, -1))


def test_census_high_keys():
    c, labels, cen = _labels("high_keys")
    assert cen == {"clusters": 4, "core": 48, "border": 0, "noise": 200}
    keys, dims = cluster_ref.cell_keys(c)
    assert dims.tolist() == [13108, 13108, 24] and int(np.prod(dims)) == 4123671936 < 2 ** 32
    assert keys.max() >= 2 ** 31 and (keys >= 2 ** 31).sum() >= 12 and keys.min() == 0
    _, more = cluster_ref.cell_keys(cluster_ref.high_keys(cluster_ref.HIGH_Z + 1))
    assert int(np.prod(more)) > 2 ** 32                          # one more z cell: refused on the device


def test_sizes_are_prefixes_of_one_set():
    rows = cluster_ref.sizes_rows()
    assert len(rows) == 4097 == max(cluster_ref.SIZES)
    for n in cluster_ref.SIZES:
        assert np.array_equal(cluster_ref.cases()[f"sizes{n}"][0], rows[:n])
    # min_samples 4: three rows are noise, four are a cluster
    assert (cluster_ref.expected("sizes3") == -1).all() and (cluster_ref.expected("sizes4") == 0).all()
    assert (cluster_ref.expected("sizes5") == 0).all()


# ------------------------------------------------------------------ boxes
def test_boxes_equal_boxes_np():
    for name in ("blobs1000", "thin_line_x", "sizes4097", "high_keys"):
        c, labels, _ = _labels(name)
        for a, b in zip(cluster_ref.boxes(c, labels), sn_ref.boxes_np(c, labels)):
            assert a.dtype == b.dtype and np.array_equal(a, b), name
    c, labels, _ = _labels("straddle60k")
    k = int(labels.max()) + 1
    for a, b in zip(cluster_ref.boxes(c, labels, k), sn_ref.boxes_np(c, labels)):
        assert np.array_equal(a, b)
    # a smaller k leaves the larger labels out; a label without rows keeps count 0, INT_MAX and INT_MIN
    counts, lo, hi = cluster_ref.boxes(c, labels, 5)
    wc, wlo, whi = sn_ref.boxes_np(c, labels)
    assert np.array_equal(counts, wc[:5]) and np.array_equal(lo, wlo[:5]) and np.array_equal(hi, whi[:5])
    counts, lo, hi = cluster_ref.boxes(c, labels, k + 2)
    assert (counts[k:] == 0).all() and (lo[k:] == np.iinfo(np.int32).max).all() and (hi[k:] == np.iinfo(np.int32).min).all()
    assert [a.shape for a in cluster_ref.boxes(np.zeros((0, 3), np.int32), np.zeros(0, np.int32))] == [(0,), (0, 3), (0, 3)]


@pytest.mark.parametrize("k", [1, 255, 256, 257, 513, 5000])
def test_synthetic_labels(k):
    coords, labels = cluster_ref.synthetic_labels(k)
    assert len(coords) == 100003 and coords.min() == -65535 and coords.max() == 65535
    assert labels.min() == -1 and labels.max() == k - 1
    counts, lo, hi = cluster_ref.boxes(coords, labels, k)
    assert counts.sum() == (labels >= 0).sum() and ((counts == 0).sum() > 0) == (k > 4)
    assert ((counts == 0) == (lo[:, 0] == np.iinfo(np.int32).max)).all()
