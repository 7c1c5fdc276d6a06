"""Density clustering on the GPU (csrc/cluster.hip): what the SN baseline's start-up statistics need
(train_scaling_based.py:35-87, get_average_dims: sklearn.cluster.DBSCAN on the car voxels of a scan).

  dbscan         sklearn.cluster.DBSCAN(eps, min_samples).fit_predict(coords * voxel_size), label for label
  cluster_boxes  rows and integer bounding box of every cluster

There is no CPU path: CPU tensors are refused, as everywhere in this package."""
import torch

from . import _lib
from ._lib import call, ptr


def _coords(coords):
    _lib.require_gpu(coords, "coordinates")
    if coords.dim() != 2 or coords.shape[1] != 3:
        raise ValueError(f"coordinates must be [n, 3], got {tuple(coords.shape)}")
    if coords.dtype.is_floating_point or coords.dtype == torch.bool:
        raise TypeError(f"coordinates must be integer voxel coordinates, got {coords.dtype}")
    if coords.dtype == torch.int64:      # no wrap-around on the way to int32: the kernel's range check sees +-65536
        coords = coords.clamp(-65536, 65536)
    return coords.to(torch.int32).contiguous()


def dbscan_count(coords, voxel_size, eps=0.5, min_samples=10):
    """(labels int32 [n], number of clusters): `dbscan` plus the one size it reads back"""
    coords = _coords(coords)
    if not (voxel_size > 0 and eps > 0 and int(min_samples) >= 1):
        raise ValueError(f"voxel_size {voxel_size}, eps {eps} and min_samples {min_samples} must be positive")
    n = coords.shape[0]
    dev = coords.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return labels, 0
    info = torch.empty(2, dtype=torch.int32, device=dev)
    ws_bytes = _lib.load().lidog_dbscan_ws(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    call("lidog_dbscan", ptr(coords), n, float(voxel_size), float(eps), int(min_samples), ptr(labels), ptr(info),
         ptr(ws), ws_bytes)
    err, k = info.tolist()                      # the one device -> host read
    if err == 1:
        raise ValueError("dbscan: voxel coordinates out of the supported range -65535 <= x, y, z <= 65535")
    if err:
        raise ValueError(f"dbscan: the grid of eps-sized cells ({eps} / {voxel_size} voxels) over the input's bounding "
                         "box has more than 2^32 cells")
    return labels, k


def dbscan(coords, voxel_size, eps=0.5, min_samples=10):
    """coords int [n, 3] on the GPU (distinct rows, as a voxelised scan has; |c| <= 65535) -> labels int32 [n], equal to
    sklearn.cluster.DBSCAN(eps=eps, min_samples=min_samples).fit_predict(coords * voxel_size) with `coords * voxel_size`
    the float32 array the reference clusters: -1 is noise, clusters are numbered in the order of their smallest core
    row, a border point belongs to the smallest-numbered cluster it touches.  n = 0 gives empty labels."""
    return dbscan_count(coords, voxel_size, eps, min_samples)[0]


def cluster_boxes(coords, labels, k=None):
    """(counts int64 [k], lo int32 [k, 3], hi int32 [k, 3]): rows and per-axis minimum / maximum coordinate of every
    label 0..k-1 (k = labels.max() + 1 when not given: one read); noise (-1) is left out, and so is every label from k
    on when a smaller k is passed.  A label without rows (also: every label when n = 0) has count 0, lo INT_MAX and hi
    INT_MIN, the values the kernels start from."""
    coords = _coords(coords)
    _lib.require_gpu(labels, "labels")
    labels = labels.to(torch.int32).contiguous()
    n = coords.shape[0]
    if labels.shape != (n,):
        raise ValueError(f"labels must be [{n}], got {tuple(labels.shape)}")
    dev = coords.device
    if k is None:
        k = int(labels.max()) + 1 if n else 0
    k = max(int(k), 0)
    counts = torch.empty(k, dtype=torch.int64, device=dev)
    lo = torch.empty((k, 3), dtype=torch.int32, device=dev)
    hi = torch.empty((k, 3), dtype=torch.int32, device=dev)
    call("lidog_cluster_boxes", ptr(coords), ptr(labels), n, k, ptr(counts), ptr(lo), ptr(hi))
    return counts, lo, hi
