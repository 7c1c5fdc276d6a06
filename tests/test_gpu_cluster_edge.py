"""csrc/cluster.hip at scale and at its own boundaries: cluster.dbscan_count equals the cell-binned restatement
(tests/cluster_ref.py, itself tested in tests/test_cluster_ref_cpu.py) label for label on chains, a full cube, a thousand
blobs, 60 000 rows whose neighbour counts straddle min_samples, grids one cell thick, cells of 1 to 100 voxels, cell keys
with the top bit set and sizes around every launch boundary; cluster.cluster_boxes equals cluster_ref.boxes past its
first LDS pass and past one sweep of its grid-stride loop.  Integers: no tolerance anywhere.

One dbscan_count call on one MI355X, HIP events around it, read-back included, one measurement per case: the chains of
20 003 rows 0.63-0.66 ms (in order, reversed, interleaved), chain_permuted 2.37 ms, cube_ratio3 1.22 ms, blobs1000
0.33 ms, straddle60k 1.68 ms, every case of about 4 000 rows or fewer 0.12-0.31 ms (the table is in DESIGN.md 3m).  No
case had to be shrunk: the path of depth n that the hook pass builds on chain_in_order costs well under a millisecond."""
import numpy as np
import pytest
import torch

import cluster_ref
from lidog_amd import cluster
from lidog_amd._lib import call, ptr

pytestmark = pytest.mark.gpu

CHAINS = tuple(n for n in cluster_ref.CASE_NAMES if n.startswith("chain"))
GUARD = 96                         # elements behind each output of the guarded box call
FILL64, FILL32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
INT_MAX, INT_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


def _gpu(a, dtype=torch.int32):
    return torch.from_numpy(np.array(a, order="C")).to(dtype).cuda()          # a copy: the shared labels stay read-only


def _check_dbscan(coords, voxel, eps, ms, want):
    """two runs: the restatement's labels, k = labels.max() + 1, and the same bytes both times"""
    c = _gpu(coords)
    labels, k = cluster.dbscan_count(c, voxel, eps=eps, min_samples=ms)
    assert labels.dtype == torch.int32 and labels.shape == (len(coords),)
    got = labels.cpu().numpy()
    again, k2 = cluster.dbscan_count(c, voxel, eps=eps, min_samples=ms)
    diff = np.nonzero(got != want)[0]
    assert len(diff) == 0, f"{len(diff)} of {len(want)} labels differ, first at row {diff[0]}: {got[diff[0]]} != {want[diff[0]]}"
    assert k == (int(want.max()) + 1 if len(want) else 0) and k2 == k
    assert again.cpu().numpy().tobytes() == got.tobytes()


# ------------------------------------------------------------------ labels
@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", CHAINS)
def test_dbscan_equals_the_restatement_on_the_chains(name):
    c, voxel, eps, ms = cluster_ref.cases()[name]
    _check_dbscan(c, voxel, eps, ms, cluster_ref.expected(name))


@pytest.mark.timeout(60)
@pytest.mark.parametrize("name", [n for n in cluster_ref.CASE_NAMES if n not in CHAINS])
def test_dbscan_equals_the_restatement(name):
    c, voxel, eps, ms = cluster_ref.cases()[name]
    _check_dbscan(c, voxel, eps, ms, cluster_ref.expected(name))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", cluster_ref.PERMUTED)
def test_dbscan_equals_the_restatement_on_one_further_row_order(name):
    _, voxel, eps, ms = cluster_ref.cases()[name]
    c, want = cluster_ref.permuted(name)
    _check_dbscan(c, voxel, eps, ms, want)


@pytest.mark.timeout(60)
def test_dbscan_refuses_one_more_cell_than_the_keys_hold():
    """high_keys has 13108 x 13108 x 24 cells, fewer than 2^32; one more cell along z is more than 2^32"""
    c = _gpu(cluster_ref.high_keys(cluster_ref.HIGH_Z + 1))
    with pytest.raises(ValueError, match="2\\^32 cells"):
        cluster.dbscan(c, cluster_ref.VOXEL)


# ------------------------------------------------------------------ boxes
def _guarded_boxes(c, labels, k):
    """lidog_cluster_boxes on outputs with GUARD more elements behind each: the first k, after checking the rest"""
    n = c.shape[0]
    counts = torch.full((k + GUARD,), FILL64, dtype=torch.int64, device="cuda")
    lo = torch.full((k + GUARD, 3), FILL32, dtype=torch.int32, device="cuda")
    hi = torch.full((k + GUARD, 3), FILL32, dtype=torch.int32, device="cuda")
    call("lidog_cluster_boxes", ptr(c), ptr(labels), n, k, ptr(counts), ptr(lo), ptr(hi))
    assert (counts[k:] == FILL64).all() and (lo[k:] == FILL32).all() and (hi[k:] == FILL32).all(), "written past k"
    return counts[:k], lo[:k], hi[:k]


def _check_boxes(coords, labels, k, read_k=False):
    c, l = _gpu(coords), _gpu(labels)
    want = cluster_ref.boxes(coords, labels, k)
    outs = [cluster.cluster_boxes(c, l, k), _guarded_boxes(c, l, k)]
    if read_k:
        assert k == int(np.max(labels)) + 1
        outs.append(cluster.cluster_boxes(c, l))
    for counts, lo, hi in outs:
        assert counts.dtype == torch.int64 and lo.dtype == torch.int32 and hi.dtype == torch.int32
        assert counts.shape == (k,) and lo.shape == (k, 3) and hi.shape == (k, 3)
        for got, w, what in zip((counts, lo, hi), want, ("counts", "lo", "hi")):
            np.testing.assert_array_equal(got.cpu().numpy(), w, err_msg=what)
    return want


@pytest.mark.timeout(60)
@pytest.mark.parametrize("name", ["blobs1000", "straddle60k"])
def test_boxes_equal_the_restatement_on_the_labels_of(name):
    coords = cluster_ref.cases()[name][0]
    labels = cluster_ref.expected(name)
    counts, _, _ = _check_boxes(coords, labels, int(labels.max()) + 1, read_k=True)
    assert (counts > 0).all()


@pytest.mark.timeout(60)
@pytest.mark.parametrize("k", [1, 255, 256, 257, 513, 5000])
def test_boxes_equal_the_restatement_on_synthetic_labels(k):
    """100 003 rows are more than one sweep of the 256 workgroups; labels -1 and labels without rows included"""
    coords, labels = cluster_ref.synthetic_labels(k)
    counts, lo, hi = _check_boxes(coords, labels, k, read_k=True)
    assert ((counts == 0).sum() > 0) == (k > 4)
    assert lo.min() == -65535 and hi.max() == 65535


@pytest.mark.timeout(60)
@pytest.mark.parametrize("k", [1, 200, 256, 300, 700])
def test_boxes_ignore_labels_from_k_on(k):
    coords, labels = cluster_ref.synthetic_labels(1000)
    assert labels.max() == 999
    _check_boxes(coords, labels, k)


@pytest.mark.timeout(60)
def test_boxes_of_labels_without_rows():
    """count 0, lo INT_MAX and hi INT_MIN (as k_cl_box_init leaves them), also with no rows at all"""
    coords, labels = cluster_ref.synthetic_labels(3, n=1000)
    counts, lo, hi = _check_boxes(coords, labels, 600)
    assert (counts[3:] == 0).all() and (lo[3:] == INT_MAX).all() and (hi[3:] == INT_MIN).all() and (counts[:3] > 0).all()
    counts, lo, hi = _check_boxes(np.zeros((0, 3), np.int32), np.zeros(0, np.int32), 300)
    assert (counts == 0).all() and (lo == INT_MAX).all() and (hi == INT_MIN).all()
    counts, lo, hi = _check_boxes(coords, np.full(len(coords), -1, np.int32), 2)             # noise only
    assert (counts == 0).all() and (lo == INT_MAX).all() and (hi == INT_MIN).all()


@pytest.mark.timeout(60)
def test_boxes_and_labels_take_int64():
    coords, voxel, eps, ms = cluster_ref.cases()["sizes4097"]
    want = cluster_ref.expected("sizes4097")
    c64 = _gpu(coords, torch.int64)
    labels, k = cluster.dbscan_count(c64, voxel, eps=eps, min_samples=ms)
    np.testing.assert_array_equal(labels.cpu().numpy(), want)
    coords, labels = cluster_ref.synthetic_labels(257)
    got = cluster.cluster_boxes(_gpu(coords, torch.int64), _gpu(labels, torch.int64), 257)
    for g, w in zip(got, cluster_ref.boxes(coords, labels, 257)):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
