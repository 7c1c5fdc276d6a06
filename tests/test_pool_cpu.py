"""The float64 pooling yardstick (tests/pool_ref.py) against hand-computed cases, and the parts of the pooling feature
that need no GPU: RegionType / KernelGenerator, the C ABI's declarations, bindings and argument checks, the
MinkowskiEngine alias."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pool_ref as P
import sconv_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lidog_pool_rows", "lidog_pool_rows_max", "lidog_pool_rows_max_bwd", "lidog_pool_global_ws",
               "lidog_pool_global", "lidog_pool_global_bwd")
NEW_NAMES = ("MinkowskiMaxPooling", "MinkowskiAvgPooling", "MinkowskiSumPooling", "MinkowskiPoolingTranspose",
             "MinkowskiGlobalSumPooling", "MinkowskiGlobalAvgPooling", "MinkowskiGlobalMaxPooling",
             "MinkowskiGlobalPooling", "MinkowskiLinear", "MinkowskiGELU", "MinkowskiNetwork", "RegionType",
             "KernelGenerator")


# ------------------------------------------------------------------ 1. the yardstick, by hand
def test_block_2x2x2_under_k2s2():
    """eight voxels of one 2^3 window, rows in REVERSED offset order: the list of the one output row walks rows 7 .. 0"""
    offs = R.offsets(2, 1)
    fine = np.concatenate([np.zeros((8, 1), np.int64), offs[::-1]], axis=1)
    coarse = R.strided(fine, 2)
    assert coarse.tolist() == [[0, 0, 0, 0]]
    nbr = R.neighbours(fine, coarse, 2, 1, 2)
    assert nbr[:, 0].tolist() == [7, 6, 5, 4, 3, 2, 1, 0]
    x = torch.tensor([[3., 7.], [1., 0.], [4., 7.], [1., 0.], [5., 0.], [9., 0.], [2., 0.], [6., 0.]])
    y, _ = P.pool64(x, nbr, "sum")
    assert y.tolist() == [[31., 14.]]
    y, _ = P.pool64(x, nbr, "avg")
    assert y.tolist() == [[31. / 8, 14. / 8]]
    y, arg = P.pool64(x, nbr, "max")
    # channel 1: rows 0 and 2 tie at 7; row 2 sits at the lower offset (5 against 7), so it is the first in list order
    assert y.tolist() == [[9., 7.]] and arg.tolist() == [[5, 2]]
    gy = torch.tensor([[2., 10.]])
    gx = P.pool_bwd64(gy, nbr, 8, "max", arg)
    want = torch.zeros(8, 2, dtype=torch.float64)
    want[5, 0], want[2, 1] = 2., 10.
    assert torch.equal(gx, want)
    assert torch.equal(P.pool_bwd64(gy, nbr, 8, "sum"), gy.double().expand(8, 2))
    assert torch.equal(P.pool_bwd64(gy, nbr, 8, "avg"), (gy.double() / 8).expand(8, 2))
    # the transposed pooling returns the one coarse row to all eight voxels
    assert torch.equal(P.unpool64(torch.tensor([[1.5, -2.]]), nbr, 8), torch.tensor([[1.5, -2.]]).double().expand(8, 2))
    assert P.bound(x, nbr, "sum").tolist() == [[8 * P.U * 31, 8 * P.U * 14]]
    assert P.bound(x, nbr, "avg").tolist() == [[P.U * 31 + P.U * 31 / 8, P.U * 14 + P.U * 14 / 8]]
    assert P.bound(x, nbr, "max").tolist() == [[0., 0.]]


def test_line_under_k3s1_with_a_tie():
    """four voxels in a row along x: only the offsets (-1, 0, 0), (0, 0, 0), (1, 0, 0) = 12, 13, 14 have pairs"""
    c = np.array([[0, x, 0, 0] for x in range(4)], dtype=np.int64)
    nbr = R.neighbours(c, c, 3, 1, 1)
    assert sorted(np.nonzero((nbr >= 0).any(axis=1))[0].tolist()) == [12, 13, 14]
    x = torch.tensor([[2.], [5.], [5.], [1.]])
    assert P.pool64(x, nbr, "sum")[0].flatten().tolist() == [7., 12., 11., 6.]
    assert P.pool64(x, nbr, "avg")[0].flatten().tolist() == [3.5, 4., 11. / 3, 3.]
    y, arg = P.pool64(x, nbr, "max")
    # row 1 sees (2, 5, 5): rows 1 and 2 tie, row 1 is the centre offset (13 < 14); row 2 sees (5, 5, 1): row 1 at 12
    assert y.flatten().tolist() == [5., 5., 5., 5.] and arg.flatten().tolist() == [1, 1, 1, 2]
    gy = torch.tensor([[1.], [10.], [100.], [1000.]])
    assert P.pool_bwd64(gy, nbr, 4, "max", arg).flatten().tolist() == [0., 111., 1000., 0.]
    assert P.pool_bwd64(gy, nbr, 4, "sum").flatten().tolist() == [11., 111., 1110., 1100.]
    got = P.pool_bwd64(gy, nbr, 4, "avg").flatten().tolist()
    want = [1 / 2 + 10 / 3, 1 / 2 + 10 / 3 + 100 / 3, 10 / 3 + 100 / 3 + 1000 / 2, 100 / 3 + 1000 / 2]
    assert all(math.isclose(a, b, rel_tol=1e-15) for a, b in zip(got, want))
    # NaN: beats every number, reaches exactly the windows that hold its row, and stays the first
    xn = torch.tensor([[2.], [float("nan")], [float("inf")], [1.]])
    y, arg = P.pool64(xn, nbr, "max")
    assert [math.isnan(v) for v in y.flatten().tolist()] == [True, True, True, False]
    assert y[3, 0].item() == float("inf") and arg.flatten().tolist() == [1, 1, 1, 2]
    # an empty list (a neighbour table without any entry for a row): zeros and arg -1, avg without 0 / 0
    hole = nbr.copy()
    hole[:, 3] = -1
    for mode in ("sum", "avg", "max"):
        y, arg = P.pool64(x, hole, mode)
        assert y[3, 0].item() == 0.0 and (arg is None or arg[3, 0].item() == -1)
    ninf = torch.full((4, 1), -float("inf"))
    y, arg = P.pool64(ninf, nbr, "max")
    assert y.flatten().tolist() == [-float("inf")] * 4 and arg.flatten().tolist() == [0, 0, 1, 2]


def test_two_scans_under_global_max():
    bid = np.array([1, 0, 1, 0, 1])
    nan = float("nan")
    x = torch.tensor([[4., 0.], [2., nan], [4., 1.], [8., nan], [-1., 2.]])
    y, arg = P.global64(x, bid, 2, "max")
    assert y[:, 0].tolist() == [8., 4.] and arg[:, 0].tolist() == [3, 0]        # scan 1: rows 0 and 2 tie -> row 0
    assert math.isnan(y[0, 1].item()) and y[1, 1].item() == 2. and arg[:, 1].tolist() == [1, 4]   # the first NaN
    x0 = x[:, :1]
    assert P.global64(x0, bid, 2, "sum")[0].flatten().tolist() == [10., 7.]
    assert P.global64(x0, bid, 2, "avg")[0].flatten().tolist() == [5., 7. / 3]
    y, arg = P.global64(x0, bid, 3, "max")                                    # a batch index without rows
    assert y.flatten().tolist() == [8., 4., 0.] and arg.flatten().tolist() == [3, 0, -1]
    gy = torch.tensor([[10.], [30.]])
    assert P.global_bwd64(gy, bid, 2, "sum").flatten().tolist() == [30., 10., 30., 10., 30.]
    assert P.global_bwd64(gy, bid, 2, "avg").flatten().tolist() == [10., 5., 10., 5., 10.]
    assert P.global_bwd64(gy, bid, 2, "max", arg[:2]).flatten().tolist() == [30., 0., 0., 10., 0.]
    assert P.global_bound(x0, bid, 2, "sum").flatten().tolist() == [2 * P.U * 10, 3 * P.U * 9]


# ------------------------------------------------------------------ 2. kernel regions
def test_region_type_and_kernel_generator():
    import lidog_amd.me as ME
    assert [ME.RegionType(i) for i in range(3)] == [ME.RegionType.HYPER_CUBE, ME.RegionType.HYPER_CROSS,
                                                    ME.RegionType.CUSTOM]
    g = ME.KernelGenerator(3, 2, 1, is_transpose=True, region_type=ME.RegionType.HYPER_CROSS, region_offsets="ro",
                           expand_coordinates=True, axis_types="at", dimension=3)
    assert (g.kernel_size, g.stride, g.dilation, g.is_transpose, g.region_type, g.region_offsets, g.expand_coordinates,
            g.axis_types, g.dimension) == (3, 2, 1, True, ME.RegionType.HYPER_CROSS, "ro", True, "at", 3)
    d = ME.KernelGenerator()
    assert (d.kernel_size, d.stride, d.dilation, d.is_transpose, d.region_type, d.region_offsets, d.expand_coordinates,
            d.axis_types, d.dimension) == (-1, 1, 1, False, ME.RegionType.HYPER_CUBE, None, False, None, -1)


def test_only_plain_hyper_cubes_are_accepted():
    import lidog_amd.me as ME
    cross = ME.KernelGenerator(3, 1, 1, region_type=ME.RegionType.HYPER_CROSS, dimension=3)
    with pytest.raises(NotImplementedError, match="HYPER_CROSS"):
        ME.MinkowskiConvolution(4, 4, kernel_size=3, kernel_generator=cross, dimension=3)
    with pytest.raises(NotImplementedError, match="HYPER_CROSS"):
        ME.MinkowskiConvolutionTranspose(4, 4, kernel_size=3, kernel_generator=cross, dimension=3)
    for cls in (ME.MinkowskiMaxPooling, ME.MinkowskiAvgPooling, ME.MinkowskiSumPooling):
        with pytest.raises(NotImplementedError, match="HYPER_CROSS"):
            cls(3, 1, kernel_generator=cross, dimension=3)
    with pytest.raises(NotImplementedError, match="CUSTOM"):
        ME.MinkowskiMaxPooling(3, 1, kernel_generator=ME.KernelGenerator(3, region_type=ME.RegionType(2)), dimension=3)
    for kw in ({"axis_types": [0, 0, 0]}, {"region_offsets": torch.zeros(1, 3)}, {"expand_coordinates": True}):
        with pytest.raises(NotImplementedError, match="HYPER_CUBE"):
            ME.MinkowskiAvgPooling(3, 1, kernel_generator=ME.KernelGenerator(3, **kw), dimension=3)
    with pytest.raises(NotImplementedError, match="HYPER_CUBE"):          # per-axis sizes
        ME.MinkowskiSumPooling(3, 1, kernel_generator=ME.KernelGenerator([3, 3, 1]), dimension=3)
    with pytest.raises(NotImplementedError, match="HYPER_CUBE"):          # disagrees with the module
        ME.MinkowskiConvolution(4, 4, kernel_size=3, kernel_generator=ME.KernelGenerator(5), dimension=3)
    # None or a plain hyper-cube changes nothing
    cube = ME.KernelGenerator(2, 2, 1, region_type=ME.RegionType.HYPER_CUBE, dimension=3)
    p = ME.MinkowskiMaxPooling(2, 2, kernel_generator=cube, dimension=3)
    assert (p.kernel_size, p.stride, p.dilation) == (2, 2, 1)
    torch.manual_seed(0)
    a = ME.MinkowskiConvolution(4, 8, kernel_size=2, stride=2, kernel_generator=cube, dimension=3)
    torch.manual_seed(0)
    b = ME.MinkowskiConvolution(4, 8, kernel_size=2, stride=2, dimension=3)
    assert torch.equal(a.kernel, b.kernel) and a.kernel.shape == (8, 4, 8)
    t = ME.MinkowskiPoolingTranspose(2, 2, dimension=3)
    assert (t.kernel_size, t.stride) == (2, 2)
    assert ME.MinkowskiGlobalPooling is ME.MinkowskiGlobalAvgPooling
    assert sorted(ME.MinkowskiLinear(3, 2).state_dict()) == ["linear.bias", "linear.weight"]
    assert ME.MinkowskiNetwork(3).D == 3


# ------------------------------------------------------------------ 3. the C ABI
def test_new_symbols_are_declared_bound_and_exported():
    from lidog_amd import _lib
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    declared = set(re.findall(r"\b(lidog_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (lidog_[a-z0-9_]+)", exported.stdout))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    # the argument lists: what the declaration holds, plus nothing
    for name in NEW_SYMBOLS:
        decl = re.search(r"^(?:int|int64_t) " + name + r"\(([^;]*?)\)\s*;", header, re.S | re.M).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    assert "pool.hip" in __import__("lidog_amd.build", fromlist=["SOURCES"]).SOURCES
    assert _lib.ABI_VERSION == 9 and _lib.load().lidog_abi_version() == 9     # additive entries: the version stays


def test_argument_checks_return_before_any_launch():
    """C >= 1 and the pointers are validated on the host; n == 0 and B == 0 return cleanly (no device is touched)"""
    from lidog_amd import _lib
    L = _lib.load()
    one = ctypes.c_void_p(64)        # never dereferenced: every call below returns from its checks
    assert L.lidog_pool_rows(one, one, one, one, 5, 0, 0, None, one, None) == 2
    assert b"C must be >= 1" in L.lidog_last_error()
    assert L.lidog_pool_rows(None, one, one, one, 5, 4, 0, None, one, None) == 2
    assert L.lidog_pool_rows(None, None, None, None, 0, 4, 1, None, None, None) == 0
    assert L.lidog_pool_rows_max(one, one, one, one, 5, 3, one, None, None) == 2
    assert L.lidog_pool_rows_max(None, None, None, None, 0, 1, None, None, None) == 0
    assert L.lidog_pool_rows_max_bwd(one, None, one, one, one, 5, 3, one, None) == 2
    assert L.lidog_pool_rows_max_bwd(None, None, None, None, None, 0, 1, None, None) == 0
    assert L.lidog_pool_global(one, 5, 0, 2, one, one, 0, one, None, one, 1 << 20, None) == 2
    assert L.lidog_pool_global(one, 5, 4, 2, one, one, 3, one, None, one, 1 << 20, None) == 2       # mode
    assert L.lidog_pool_global(one, 5, 4, 2, one, one, 2, one, None, one, 1 << 20, None) == 2       # max without arg
    assert L.lidog_pool_global(one, 5, 4, 2, one, one, 0, one, None, one, 8, None) == 2             # workspace
    assert L.lidog_pool_global(None, 0, 4, 0, None, None, 1, None, None, None, 0, None) == 0
    assert L.lidog_pool_global_bwd(None, None, 0, 4, 0, None, None, 2, None, None) == 0
    assert L.lidog_pool_global_bwd(one, None, 5, 4, 2, one, one, 2, one, None) == 2
    assert L.lidog_pool_global_ws(0, 2, 4) == 0 and L.lidog_pool_global_ws(5, 2, 0) == 0
    # one partial row per workgroup, a float and an int32 per element: 1 workgroup per scan for a tiny map, 64 at most
    assert L.lidog_pool_global_ws(5, 2, 4) == 2 * 1 * 4 * 8
    assert L.lidog_pool_global_ws(10 ** 6, 4, 256) == 4 * 64 * 256 * 8


# ------------------------------------------------------------------ 4. the alias
def test_names_resolve_under_the_minkowski_engine_alias():
    import sys
    import lidog_amd.me as ME
    saved = {k: sys.modules.get(k) for k in ("MinkowskiEngine", "MinkowskiEngine.utils", "MinkowskiEngine.modules",
                                             "MinkowskiEngine.modules.resnet_block",
                                             "MinkowskiEngine.MinkowskiFunctional")}
    try:
        ME.install_as_minkowski_engine()
        import MinkowskiEngine
        for name in NEW_NAMES:
            assert getattr(MinkowskiEngine, name) is getattr(ME, name), name
        assert MinkowskiEngine.RegionType(1) is MinkowskiEngine.RegionType.HYPER_CROSS
        assert not hasattr(MinkowskiEngine, "MinkowskiAvgUnpooling")      # not a 0.5.4 name
        import MinkowskiEngine.MinkowskiFunctional as MEF                 # utils/models/resunet.py:4
        assert MEF.relu is ME.MinkowskiFunctional.relu
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
