"""The float64 yardstick of the point <-> voxel family (tests/field_ref.py) against hand-computed cases, and the parts
of the feature that need no GPU: the C ABI's declarations, bindings and argument checks, the MinkowskiEngine alias, the
argument checks of the operator layer and of the evaluation flag."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import field_ref as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lidog_field_floor", "lidog_field_lists_ws", "lidog_field_lists", "lidog_field_reduce",
               "lidog_field_gather", "lidog_interp_fwd", "lidog_interp_bwd")
NEW_NAMES = ("TensorField", "SparseTensorQuantizationMode", "MinkowskiInterpolation")


def _block(b=0, origin=(0, 0, 0)):
    """the 8 voxels of a 2^3 block in k order (x fastest): row k is neighbour k of a query inside the block"""
    return np.array([[b, origin[0] + (k & 1), origin[1] + ((k >> 1) & 1), origin[2] + (k >> 2)] for k in range(8)])


# ------------------------------------------------------------------ 1. the yardstick, by hand
def test_centre_of_a_block_weighs_every_corner_an_eighth():
    c = _block()
    q = torch.tensor([[0., 0.5, 0.5, 0.5]])
    nbr, w = F.neighbours(c, q, 1)
    assert nbr[:, 0].tolist() == list(range(8)) and w[:, 0].tolist() == [0.125] * 8
    feats = torch.arange(16.).reshape(8, 2)
    assert F.interp64(feats, nbr, w).tolist() == [[7., 8.]]
    gy = torch.tensor([[8., -16.]])
    assert torch.equal(F.interp_bwd64(gy, nbr, w, 8), torch.tensor([[1., -2.]]).double().expand(8, 2))
    # 8 neighbours: gamma_13 sum |w F|
    g13 = float(F.gamma(13)) + 3 * 2.0 ** -29
    assert F.interp_bound(feats, nbr, w).tolist() == [[g13 * 7., g13 * 8.]]


def test_query_on_a_lattice_point_takes_that_row_alone():
    c = _block()
    nbr, w = F.neighbours(c, torch.tensor([[0., 1., 0., 1.]]), 1)
    # lo = (1, 0, 1): neighbour 0 is row 5 (x = 1, z = 1) with weight 1; the upper neighbours that exist weigh 0
    assert nbr[0, 0] == 5 and w[:, 0].tolist() == [1.] + [0.] * 7
    assert nbr[2, 0] == 7 and (nbr[[1, 3, 4, 5, 6, 7], 0] == -1).all()
    feats = torch.arange(8.).reshape(8, 1)
    assert F.interp64(feats, nbr, w).tolist() == [[5.]]


def test_missing_neighbour_adds_nothing_and_nothing_is_renormalised():
    c = np.delete(_block(), 3, axis=0)               # (1, 1, 0) is gone
    nbr, w = F.neighbours(c, torch.tensor([[0., 0.5, 0.5, 0.5]]), 1)
    assert nbr[:, 0].tolist() == [0, 1, 2, -1, 3, 4, 5, 6]
    ones = torch.ones(7, 1)
    assert F.interp64(ones, nbr, w).tolist() == [[0.875]]
    gF = F.interp_bwd64(torch.tensor([[8.]]), nbr, w, 7)
    assert gF.flatten().tolist() == [1.] * 7
    # another batch index never counts, and a query far away has no neighbour: zeros, bound 0
    nbr, w = F.neighbours(c, torch.tensor([[1., 0.5, 0.5, 0.5], [0., 1000.5, 0.5, 0.5]]), 1)
    assert (nbr == -1).all()
    assert F.interp64(ones, nbr, w).tolist() == [[0.], [0.]] and F.interp_bound(ones, nbr, w).tolist() == [[0.], [0.]]


def test_negative_coordinate_floors_toward_minus_infinity():
    c = np.array([[0, -1, 0, 0], [0, 0, 0, 0]])
    nbr, w = F.neighbours(c, torch.tensor([[0., -0.25, 0., 0.]]), 1)
    # -0.25 lies between -1 and 0: lo = -1, t = 0.75
    assert nbr[:2, 0].tolist() == [0, 1] and w[:2, 0].tolist() == [0.25, 0.75]
    assert F.interp64(torch.tensor([[4.], [8.]]), nbr, w).tolist() == [[7.]]
    # just below a lattice point whose cell is missing: the own cell keeps its (tiny, exact) weight, nothing vanishes
    nbr, w = F.neighbours(np.array([[0, -1, 0, 0]]), torch.tensor([[0., -2.0 ** -44, 0., 0.]]), 1)
    assert nbr[:2, 0].tolist() == [0, -1] and w[:2, 0].tolist() == [2.0 ** -44, 1 - 2.0 ** -44]
    assert F.interp64(torch.tensor([[3.]]), nbr, w).tolist() == [[3 * 2.0 ** -44]]
    rows, err = F.floor_rows(torch.tensor([[0., -0.25, -1., -1.5]]), 1)
    assert rows.tolist() == [[0, -1, -1, -2]] and err == 0
    # tensor stride 4: -0.25 lies between -4 and 0, t = 3.75 / 4
    nbr, w = F.neighbours(np.array([[0, -4, 0, 0], [0, 0, 0, 0]]), torch.tensor([[0., -0.25, 0., 0.]]), 4)
    assert nbr[:2, 0].tolist() == [0, 1] and w[:2, 0].tolist() == [0.0625, 0.9375]
    rows, err = F.floor_rows(torch.tensor([[0., -0.25, 5., 8.]]), 4)
    assert rows.tolist() == [[0, -4, 4, 8]] and err == 0


def test_floor_error_word_and_bad_values():
    nan, inf = float("nan"), float("inf")
    rows, err = F.floor_rows(torch.tensor([[0., nan, 1., 2.]]), 1)
    assert rows.tolist() == [[0, F.INT32_MIN, 1, 2]] and err == F.ERR_NONFINITE
    rows, err = F.floor_rows(torch.tensor([[1., -inf, 3e9, 2.5]]), 1)
    assert rows.tolist() == [[1, F.INT32_MIN, F.INT32_MIN, 2]] and err == F.ERR_NONFINITE
    rows, err = F.floor_rows(torch.tensor([[1., 3e9, 0., 0.]]), 1)          # finite, beyond int32: no bit
    assert rows.tolist() == [[1, F.INT32_MIN, 0, 0]] and err == 0
    for b in (0.5, -1., 4096., nan):
        rows, err = F.floor_rows(torch.tensor([[b, 0., 0., 0.]]), 1)
        assert rows.tolist() == [[-1, 0, 0, 0]] and err == F.ERR_BATCH
    assert F.floor_rows(torch.tensor([[4095., 0., 0., 0.]]), 1)[1] == 0


def test_lists_reduce_and_gather():
    inv = np.array([2, 0, 2, -1, 0, 2, 7])
    row_ptr, row_list = F.lists(inv, 4)
    assert row_ptr.tolist() == [0, 2, 2, 5, 5] and row_list.tolist() == [1, 4, 0, 2, 5]
    good = np.array([2, 0, 2, 0, 2])
    x = torch.tensor([[1.], [10.], [2.], [20.], [6.]])
    assert F.reduce64(x, good, 4, False).flatten().tolist() == [30., 0., 9., 0.]
    assert F.reduce64(x, good, 4, True).flatten().tolist() == [15., 0., 3., 0.]
    v = torch.tensor([[30.], [0.], [9.], [0.]])
    assert F.gather64(v, good).flatten().tolist() == [9., 30., 9., 30., 9.]
    assert F.gather64(v, good, 4, True).flatten().tolist() == [3., 15., 3., 15., 3.]
    # 2 and 3 terms: 1 and 2 roundings
    assert F.reduce_bound(x, good, 4, False).flatten().tolist() == [float(F.gamma(1)) * 30, 0., float(F.gamma(2)) * 9, 0.]
    assert F.gather_bound(v, good).abs().sum().item() == 0.
    assert F.worst_ratio(torch.tensor([1.]), torch.tensor([1.]).double(), torch.tensor([0.]).double()) == 0.
    assert F.worst_ratio(torch.tensor([1.5]), torch.tensor([1.]).double(), torch.tensor([0.]).double()) == float("inf")


# ------------------------------------------------------------------ 2. the C ABI
def test_new_symbols_are_declared_bound_and_exported():
    from lidog_amd import _lib
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    declared = set(re.findall(r"\b(lidog_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (lidog_[a-z0-9_]+)", exported.stdout))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    for name in NEW_SYMBOLS:
        decl = re.search(r"^(?:int|int64_t) " + name + r"\(([^;]*?)\)\s*;", header, re.S | re.M).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    assert "field.hip" in __import__("lidog_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "[ME-mem]" in header
    assert _lib.ABI_VERSION == 9 and _lib.load().lidog_abi_version() == 9     # additive entries: the version stays


def test_argument_checks_return_before_any_launch():
    from lidog_amd import _lib
    L = _lib.load()
    one = ctypes.c_void_p(64)        # never dereferenced: every call below returns from its checks
    assert L.lidog_field_floor(one, 5, 0, one, one, None) == 2
    assert b"tensor stride" in L.lidog_last_error()
    assert L.lidog_field_floor(None, 5, 1, one, one, None) == 2
    assert L.lidog_field_floor(None, 0, 1, None, None, None) == 0
    assert L.lidog_field_lists(one, 5, 3, None, one, one, 1 << 20, None) == 2
    assert L.lidog_field_lists(one, 5, 3, one, one, one, 8, None) == 2             # workspace
    assert L.lidog_field_lists(one, -1, 3, one, one, one, 1 << 20, None) == 2
    assert L.lidog_field_lists_ws(0, 5) == 256 and L.lidog_field_lists_ws(100, 10) >= 3 * 400
    assert L.lidog_field_reduce(one, 5, one, one, 3, 0, 0, one, None) == 2
    assert b"C must be >= 1" in L.lidog_last_error()
    assert L.lidog_field_reduce(None, 5, one, one, 3, 4, 0, one, None) == 2
    assert L.lidog_field_reduce(None, 5, None, None, 0, 4, 1, None, None) == 0
    assert L.lidog_field_gather(one, None, 5, 3, 4, None, one, None) == 2
    assert L.lidog_field_gather(None, None, 0, 3, 4, None, None, None) == 0
    assert L.lidog_interp_fwd(one, 3, 4, one, one, 5, 0, one, None) == 2
    assert L.lidog_interp_fwd(one, 3, 4, None, one, 5, 1, one, None) == 2
    assert L.lidog_interp_fwd(one, 3, 4, one, one, 1 << 28, 1, one, None) == 2     # 8 Q must fit an int32
    assert L.lidog_interp_fwd(None, 3, 4, None, None, 0, 1, None, None) == 0
    assert L.lidog_interp_bwd(one, one, 5, None, one, 3, 4, 1, one, None) == 2
    assert L.lidog_interp_bwd(None, None, 5, None, None, 0, 4, 1, None, None) == 0


# ------------------------------------------------------------------ 3. the operator layer, without a device
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
        for name in ("slice", "cat_slice", "features_at_coordinates", "interpolate"):
            assert callable(getattr(MinkowskiEngine.SparseTensor, name)), name
        modes = MinkowskiEngine.SparseTensorQuantizationMode
        assert [m.name for m in modes] == ["RANDOM_SUBSAMPLE", "UNWEIGHTED_AVERAGE", "UNWEIGHTED_SUM", "MAX_POOL"]
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_argument_checks_that_need_no_device():
    import lidog_amd.me as ME
    f, c = torch.zeros(2, 3), torch.zeros(2, 4)
    with pytest.raises(TypeError, match="minkowski_algorithm"):
        ME.TensorField(f, c, minkowski_algorithm=1)
    with pytest.raises(TypeError, match="SparseTensorQuantizationMode"):
        ME.TensorField(f, c, quantization_mode=1)
    with pytest.raises(NotImplementedError, match="tensor_stride"):
        ME.TensorField(f, c, tensor_stride=2)
    with pytest.raises(RuntimeError, match="GPU"):          # no CPU path
        ME.TensorField(f, c)
    for kw in ({"return_kernel_map": True}, {"return_weights": True}):
        with pytest.raises(NotImplementedError):
            ME.MinkowskiInterpolation(**kw)
    assert isinstance(ME.MinkowskiInterpolation(), torch.nn.Module)
    import inspect
    sig = inspect.signature(ME.TensorField.__init__)
    assert list(sig.parameters)[1:7] == ["features", "coordinates", "tensor_stride", "coordinate_manager",
                                         "quantization_mode", "device"]
    assert sig.parameters["quantization_mode"].default is ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE
    assert list(inspect.signature(ME.TensorField.sparse).parameters) == ["self", "tensor_stride", "quantization_mode"]
    # SparseTensor keeps its signature: averaging lives in TensorField only
    assert "quantization_mode" not in inspect.signature(ME.SparseTensor.__init__).parameters
    with pytest.raises(ValueError, match="NaN"):
        ME.field_error(2)
    with pytest.raises(ValueError, match="batch"):
        ME.field_error(1)
    ME.field_error(0)


def test_point_interp_flag_and_point_path_argument():
    from lidog_amd import eval_target, evaluate
    import inspect
    assert inspect.signature(evaluate.PointPath.__init__).parameters["interp"].default == "nearest"
    assert callable(evaluate.point_logits)
    with pytest.raises(ValueError, match="interp"):
        evaluate.PointPath(3, "cpu", interp="cubic")
    src = open(os.path.join(REPO, "lidog_amd", "eval_target.py")).read()
    assert "--point-interp" in src and '"nearest", "trilinear"' in src
