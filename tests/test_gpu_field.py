"""The point <-> voxel family on the GPU (csrc/field.hip behind lidog_field_floor / _lists / _reduce / _gather and
lidog_interp_fwd / _bwd, and TensorField / slice / cat_slice / features_at_coordinates / interpolate /
MinkowskiInterpolation of lidog_amd.me on top of them) against the float64 yardstick tests/field_ref.py on the edge-case
scenes of tests/sconv_ref.py.

Every assertion is either an exact equality the contract promises (the floored rows, the neighbour table, the lists,
sums / averages / slices of integers |v| <= 15, two runs of every kernel, the module path against the C ABI) or the
derived bound of field_ref (nothing in it is measured on the kernels).  Results are pre-filled with NaN: a row left
unwritten fails.  References are computed once per case at the largest channel count and cut by column: every kernel
treats a channel alone.

Channel counts: 1, 3, 7 (scalar kernels), 4, 32, 100 (float4 kernels; 100: the last wave of a workgroup partly idle).
Query / point counts 0, 1, 63, 64, 65 (around a wave), 257 (more than a workgroup of rows at C = 1)."""
import numpy as np
import pytest
import torch

import field_ref as F
import sconv_ref as R

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
CHANNELS = (1, 3, 4, 7, 32, 100)
CMAX = max(CHANNELS)
COUNTS = (0, 1, 63, 64, 65, 257)
SCENES = ("tiny_1", "isolated", "dense_cube_odd", "line_x129", "twin_scans", "range_ends")
STRIDES = (1, 2, 4)
_CMS, _OPS = {}, {}


# ------------------------------------------------------------------ helpers
def _manager(name):
    import lidog_amd.me as ME
    if name not in _CMS:
        c = torch.from_numpy(R.scene(name)).cuda()
        _CMS[name] = ME.SparseTensor(coordinates=c, features=torch.ones((c.shape[0], 1), device="cuda")).coordinate_manager
    return _CMS[name]


def _map_coords(cm, s):
    """int64 numpy [M, 4]: the coordinates of the manager's map of tensor stride s (built through manager.stride)"""
    t = 1
    while t < s:
        cm.stride(t, 2 * t)
        t *= 2
    return cm.maps[s].coords.cpu().numpy().astype(np.int64)


def _operands(n, what):
    """[n, CMAX] on the CPU, shared and left unchanged: `int` = integers |v| <= 15 (sums exact), `randn`, `randn2`"""
    if what not in _OPS:
        g = torch.Generator().manual_seed({"int": 21, "randn": 22, "randn2": 23}[what])
        _OPS[what] = torch.randint(-15, 16, (50000, CMAX), generator=g).float() if what == "int" else \
            torch.randn(50000, CMAX, generator=g)
    return _OPS[what][:n]


def _dev(t, C=None):
    """every float operand the C ABI tests own: the first C columns of t, or (C None) t itself"""
    return (t if C is None else t[:, :C].contiguous()).cuda()


def _nan(*shape, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full(shape, -7, dtype=dtype, device="cuda")
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _fill(shape, value, dtype):
    """the error word and the byte workspace; value None: uninitialised (torch.empty)"""
    if value is None:
        return torch.empty(shape, dtype=dtype, device="cuda")
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _exact(got, ref64, what):
    assert torch.equal(got.double().cpu(), ref64), f"{what}: not bit-exact"


def _inside(got, ref64, bnd, what):
    r = F.worst_ratio(got, ref64, bnd)
    print(f"{what}: error / bound {r:.3g}")
    assert r <= 1.0, f"{what}: error / bound {r:.3g} (or a row left unwritten)"


def _queries(coords, s, nq, seed):
    """float32 [nq, 4] around the rows of a map: on lattice points, between them (also below the lowest and above the
    highest voxel of the scene: negative coordinates, neighbours beyond the range), and far from every voxel"""
    rng = np.random.default_rng(seed)
    rows = coords[rng.integers(0, coords.shape[0], nq)]
    q = rows.astype(np.float64)
    kind = np.arange(nq) % 5
    shift = rng.integers(-12 * s, 12 * s, (nq, 3)) / 8.0          # multiples of 1/8, up to 1.5 cells away
    shift[kind == 0] = 0.                                         # exactly on a lattice point
    shift[kind == 1] = rng.integers(-s, s + 1, (int((kind == 1).sum()), 3))      # on integer positions inside a coarse cell
    shift[kind == 2] = rng.random((int((kind == 2).sum()), 3)) * s               # any float32 fraction
    q[:, 1:] += shift
    q[kind == 4, 1:] += 5000.                                     # no neighbour at all
    return torch.from_numpy(q.astype(np.float32))


def _floor(query, s):
    from lidog_amd._lib import call, ptr
    rows = _nan(query.shape[0], 4, dtype=torch.int32)
    err = _fill((1,), 0, torch.int32)
    call("lidog_field_floor", ptr(query), query.shape[0], s, ptr(rows), ptr(err))
    return rows, int(err.item())


def _lists(inv, m):
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    inv = inv.reshape(-1).contiguous()
    n = inv.shape[0]
    row_ptr = _nan(m + 1, dtype=torch.int32)
    row_list = _nan(max(n, 1), dtype=torch.int32)
    nbytes = _lib.load().lidog_field_lists_ws(n, m)
    ws = _fill((nbytes,), None, torch.uint8)
    call("lidog_field_lists", ptr(inv), n, m, ptr(row_ptr), ptr(row_list), ptr(ws), nbytes)
    return row_ptr, row_list


def _check_lists(got, inv, m, what):
    row_ptr, row_list = got
    ref_ptr, ref_list = F.lists(inv, m)
    assert row_ptr.cpu().tolist() == ref_ptr.tolist(), f"{what}: row_ptr"
    assert row_list.cpu()[:len(ref_list)].tolist() == ref_list.tolist(), f"{what}: row_list"


def _reduce(x, lists, m, mean):
    from lidog_amd._lib import call, ptr
    y = _nan(m, x.shape[1])
    call("lidog_field_reduce", ptr(x), x.shape[0], ptr(lists[0]), ptr(lists[1]), m, x.shape[1], mean, ptr(y))
    return y


def _gather(x, inv, row_ptr=None):
    from lidog_amd._lib import call, ptr
    y = _nan(inv.shape[0], x.shape[1])
    call("lidog_field_gather", ptr(x), ptr(inv), inv.shape[0], x.shape[0], x.shape[1], ptr(row_ptr), ptr(y))
    return y


def _interp(feats, query, nbr, s):
    from lidog_amd._lib import call, ptr
    y = _nan(query.shape[0], feats.shape[1])
    call("lidog_interp_fwd", ptr(feats), feats.shape[0], feats.shape[1], ptr(query), ptr(nbr), query.shape[0], s, ptr(y))
    return y


def _interp_bwd(gy, query, lists, m, s):
    from lidog_amd._lib import call, ptr
    gF = _nan(m, gy.shape[1])
    call("lidog_interp_bwd", ptr(gy), ptr(query), query.shape[0], ptr(lists[0]), ptr(lists[1]), m, gy.shape[1], s, ptr(gF))
    return gF


def _interp_case(cm, coords, s, query, what, channels=CHANNELS):
    """neighbour table, lists, forward and gradient of one (map, queries) pair through the C ABI, every channel count"""
    import lidog_amd.me as ME
    m, nq = coords.shape[0], query.shape[0]
    nbr_ref, w = F.neighbours(coords, query, s)
    qd = _dev(query)
    nbr = ME.interpolation_neighbours(cm, s, qd)
    assert nbr.shape == (8, nq) and nbr.cpu().tolist() == nbr_ref.tolist(), f"{what}: neighbour table"
    lists = _lists(nbr, m)
    _check_lists(lists, nbr_ref, m, what)
    assert torch.equal(_lists(nbr, m)[0], lists[0]) and \
        torch.equal(_lists(nbr, m)[1][:int(lists[0][m])], lists[1][:int(lists[0][m])])
    feats, gy = _operands(m, "randn"), _operands(nq, "randn2")
    ref, bnd = F.interp64(feats, nbr_ref, w), F.interp_bound(feats, nbr_ref, w)
    gref, gbnd = F.interp_bwd64(gy, nbr_ref, w, m), F.interp_bwd_bound(gy, nbr_ref, w, m)
    none = torch.as_tensor((nbr_ref < 0).all(axis=0))
    for C in channels:
        x, g = _dev(feats, C), _dev(gy, C)
        y = _interp(x, qd, nbr, s)
        _inside(y, ref[:, :C], bnd[:, :C], f"{what} C={C} forward")
        assert not bool(y.cpu()[none].any()), f"{what}: a query without neighbours must give zeros"
        assert torch.equal(_interp(x, qd, nbr, s), y), f"{what} C={C}: two forward runs differ"
        gF = _interp_bwd(g, qd, lists, m, s)
        _inside(gF, gref[:, :C], gbnd[:, :C], f"{what} C={C} gradient")
        assert torch.equal(_interp_bwd(g, qd, lists, m, s), gF), f"{what} C={C}: two gradient runs differ"
    return nbr_ref, w


# ------------------------------------------------------------------ 1. floor
@pytest.mark.parametrize("s", STRIDES)
def test_floor_against_the_yardstick(s):
    g = torch.Generator().manual_seed(5)
    q = (torch.rand(257, 4, generator=g) - 0.5) * 300
    q[:, 0] = torch.randint(0, 4096, (257,), generator=g).float()
    q[:40, 1:] = torch.randint(-40, 40, (40, 3), generator=g).float()        # lattice points, negative ones too
    q[40] = torch.tensor([0., -0.25, -1e-30, 65535.75])
    q[41] = torch.tensor([4095., 3e9, -3e9, 2147483520.])                     # beyond int32 (finite): INT32_MIN, no bit
    rows, err = _floor(_dev(q), s)
    ref, ref_err = F.floor_rows(q, s)
    assert err == ref_err == 0 and rows.cpu().tolist() == ref.tolist()
    for bad, bit in (([0., NAN, 1., 2.], 2), ([0., 1., -INF, 2.], 2), ([0.5, 1., 1., 1.], 1), ([-1., 1., 1., 1.], 1),
                     ([4096., 1., 1., 1.], 1), ([NAN, 1., INF, 1.], 3)):
        qb = q.clone()
        qb[100] = torch.tensor(bad)
        rows, err = _floor(_dev(qb), s)
        ref, ref_err = F.floor_rows(qb, s)
        assert err == ref_err == bit and rows.cpu().tolist() == ref.tolist(), bad
    assert _floor(_dev(torch.zeros((0, 4))), s)[1] == 0


# ------------------------------------------------------------------ 2. interpolation through the C ABI
@pytest.mark.parametrize("s", STRIDES)
@pytest.mark.parametrize("name", SCENES)
def test_interpolation_against_float64(name, s):
    cm = _manager(name)
    coords = _map_coords(cm, s)
    query = _queries(coords, s, 257, 100 + s)
    if name == "twin_scans":       # the same position in the other scan: another row, never the other scan's
        query[:64, 0] = 1 - query[:64, 0]
    nbr, _ = _interp_case(cm, coords, s, query, f"{name} stride {s}")
    if name != "tiny_1":
        assert (nbr >= 0).any() and (nbr < 0).all(axis=0).any()
    if name == "range_ends" and s == 1:   # the upper neighbours of the last voxel lie beyond the coordinate range
        top = torch.tensor([[0., 65535.5, 65535.5, 65535.5], [4095., -65536.5, -65536., -65535.5]])
        nb, _ = F.neighbours(coords, top, 1)
        assert (nb[1:, 0] == -1).all() and nb[0, 0] >= 0 and (nb[[0, 2, 4, 6], 1] == -1).all()
        _interp_case(cm, coords, 1, top, "range_ends, at the ends", channels=(1, 4))


def test_a_query_in_one_scan_never_sees_the_other():
    """twin_scans holds the same voxels under batch 0 and 1: with features 1 / 2 per scan, a lattice-point query gives
    exactly its own scan's value"""
    import lidog_amd.me as ME
    cm = _manager("twin_scans")
    coords = _map_coords(cm, 1)
    feats = torch.from_numpy(coords[:, :1] + 1.0).float().cuda().expand(-1, 4).contiguous()
    q = torch.from_numpy(coords[:257].astype(np.float32)).cuda()
    x = ME.SparseTensor(feats, coordinate_manager=cm, coordinate_map_key=1)
    y = x.features_at_coordinates(q)
    assert torch.equal(y, feats[:257])


@pytest.mark.parametrize("nq", COUNTS)
def test_query_counts_module_path_equals_the_abi(nq):
    import lidog_amd.me as ME
    cm = _manager("dense_cube_odd")
    coords = _map_coords(cm, 2)
    m = coords.shape[0]
    query = _queries(coords, 2, nq, 7 + nq)
    nbr_ref, w = F.neighbours(coords, query, 2)
    qd = query.cuda()
    for C in (4, 7):
        feats = _dev(_operands(m, "randn"), C).requires_grad_(True)
        gy = _dev(_operands(nq, "randn2"), C)
        x = ME.SparseTensor(feats, coordinate_manager=cm, coordinate_map_key=2)
        y = x.features_at_coordinates(qd)
        assert y.shape == (nq, C)
        y.backward(gy)
        nbr = ME.interpolation_neighbours(cm, 2, qd)
        assert torch.equal(y.detach(), _interp(feats.detach(), qd, nbr, 2))
        assert torch.equal(feats.grad, _interp_bwd(gy, qd, _lists(nbr, m), m, 2))
        _inside(y, F.interp64(feats, nbr_ref, w), F.interp_bound(feats, nbr_ref, w), f"nq={nq} C={C} forward")
        _inside(feats.grad, F.interp_bwd64(gy, nbr_ref, w, m), F.interp_bwd_bound(gy, nbr_ref, w, m),
                f"nq={nq} C={C} gradient")
        z = ME.MinkowskiInterpolation()(x, qd)
        assert torch.equal(z.detach(), y.detach())


def test_hot_row_gradient():
    """300 queries in one cell (longer than a wave and a workgroup) next to 257 others: the list of that cell's rows"""
    cm = _manager("dense_cube_odd")
    coords = _map_coords(cm, 1)
    rng = np.random.default_rng(3)
    hot = np.tile(coords[0].astype(np.float64), (300, 1))
    hot[:, 1:] += rng.random((300, 3))
    query = torch.cat([torch.from_numpy(hot.astype(np.float32)), _queries(coords, 1, 257, 9)])
    query = query[torch.from_numpy(rng.permutation(557))]
    nbr, _ = _interp_case(cm, coords, 1, query, "hot row", channels=(1, 4, 7))
    assert (nbr == 0).sum() >= 300


def test_dense_cube_through_the_occupancy_bitmap():
    """36^3 = 46 656 rows: the manager builds an occupancy bitmap for this map, and the neighbour search goes through
    it.  Queries inside, on the faces, and 1000 cells outside the box (the bitmap's index is negative there: absent)."""
    import lidog_amd.me as ME
    r = np.arange(36)
    x, y, z = np.meshgrid(r, r, r, indexing="ij")
    v = np.stack([np.zeros(36 ** 3, np.int64), x.ravel() - 10, y.ravel() + 3, z.ravel() - 20], axis=1)
    v = v[np.random.default_rng(1).permutation(v.shape[0])].astype(np.int32)
    c = torch.from_numpy(v).cuda()
    cm = ME.SparseTensor(coordinates=c, features=torch.ones((c.shape[0], 1), device="cuda")).coordinate_manager
    coords = v.astype(np.int64)
    rng = np.random.default_rng(2)
    inside = np.concatenate([np.zeros((100, 1)), rng.random((100, 3)) * 34 + np.array([-10, 3, -20])], axis=1)
    faces = inside.copy()
    faces[:50, 1] = -10 - rng.random(50)          # the cell below the box: only upper x neighbours
    faces[50:, 3] = 15 + rng.random(50)           # the last cell: only lower z neighbours
    faces[::7, 2] = 38.                           # exactly on the top face
    outside = inside.copy()
    outside[:, 1 + np.arange(100) % 3] += np.where(np.arange(100) % 2 == 0, 1000., -1000.)
    query = torch.from_numpy(np.concatenate([inside, faces, outside]).astype(np.float32))
    nbr, _ = _interp_case(cm, coords, 1, query, "36^3 cube", channels=(1, 4))
    assert cm.maps[1].bits is not None, "the occupancy-bitmap path was not taken"
    assert ((nbr[:, :100] >= 0).sum(axis=0) == 8).all() and (nbr[:, 200:] == -1).all()
    part = (nbr[:, 100:200] >= 0).sum(axis=0)
    assert ((part > 0) & (part < 8)).any()


# ------------------------------------------------------------------ 3. fields: lists, reduce, gather, the modules
def _field_points(n, seed, hot=0):
    """float32 [n + hot, 4] points inside the voxels of dense_cube_odd (several per voxel), `hot` more in ONE voxel;
    (points, inverse int64, voxel rows int64 [M, 4] in first-occurrence order)"""
    coords = R.scene("dense_cube_odd").astype(np.int64)
    rng = np.random.default_rng(seed)
    rows = coords[rng.integers(0, max(n // 3, 1), n)]
    p = np.concatenate([rows, np.tile(coords[5], (hot, 1))]).astype(np.float64)
    p[:, 1:] += rng.integers(0, 8, (n + hot, 3)) / 8.0
    p = p[rng.permutation(n + hot)].astype(np.float32)
    floor, err = F.floor_rows(torch.from_numpy(p), 1)
    assert err == 0
    first, inv = {}, np.empty(n + hot, np.int64)
    for i, row in enumerate(map(tuple, floor.tolist())):
        inv[i] = first.setdefault(row, len(first))
    vox = np.array(list(first), dtype=np.int64).reshape(-1, 4)
    return torch.from_numpy(p), inv, vox


@pytest.mark.parametrize("n,hot", [(c, 0) for c in COUNTS] + [(257, 300)])
def test_field_lists_reduce_gather(n, hot):
    import lidog_amd.me as ME
    pts, inv, vox = _field_points(n, 30 + n, hot)
    N, m = n + hot, vox.shape[0]
    if hot:
        assert np.bincount(inv).max() >= 300
    inv_d = torch.from_numpy(inv).int().cuda()
    lists = _lists(inv_d, m)
    _check_lists(lists, inv, m, f"n={N}")
    xi, xr, gr = _operands(N, "int"), _operands(N, "randn"), _operands(m, "randn2")
    field = ME.TensorField(_dev(xi, 4), pts.cuda()) if N else None
    if N:
        assert field.inverse_mapping().cpu().tolist() == inv.tolist()
        st = field.sparse()
        assert st.C.cpu().tolist() == vox.tolist() and st.coordinate_manager is field.coordinate_manager
    for C in CHANNELS:
        for mean in (0, 1):
            what = f"n={N} C={C} {'mean' if mean else 'sum'}"
            x = _dev(xi, C)
            y = _reduce(x, lists, m, mean)
            _exact(y, F.reduce64(xi[:, :C], inv, m, mean).float().double(), what + " of integers")
            assert torch.equal(_reduce(x, lists, m, mean), y), what + ": two runs differ"
            x = _dev(xr, C)
            y = _reduce(x, lists, m, mean)
            _inside(y, F.reduce64(xr[:, :C], inv, m, mean), F.reduce_bound(xr[:, :C], inv, m, mean), what)
            g = _dev(gr, C)
            gx = _gather(g, inv_d, lists[0] if mean else None)
            _inside(gx, F.gather64(gr[:, :C], inv, m, mean), F.gather_bound(gr[:, :C], inv, m, mean), what + " gather")
            assert torch.equal(_gather(g, inv_d, lists[0] if mean else None), gx), what + ": two gathers differ"
            if N and C in (4, 7):      # the module path: the same bits, forward and gradient
                mode = ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE if mean else \
                    ME.SparseTensorQuantizationMode.UNWEIGHTED_SUM
                feats = _dev(xr, C).requires_grad_(True)
                out = field._like(feats).sparse(quantization_mode=mode)
                assert torch.equal(out.F.detach(), y)
                out.F.backward(g)
                assert torch.equal(feats.grad, gx)
        if N:
            v = _dev(xi[:m], C).requires_grad_(True)          # slice: integers in, the same integers out
            sl = ME.SparseTensor(v, coordinate_manager=field.coordinate_manager, coordinate_map_key=1).slice(field)
            assert isinstance(sl, ME.TensorField) and sl.C is field.C
            _exact(sl.F.detach(), F.gather64(xi[:m, :C], inv), f"n={N} C={C} slice")
            assert torch.equal(sl.F.detach(), _gather(v.detach(), inv_d))
            gp = _dev(xi, C)
            sl.F.backward(gp)                                 # its gradient: the ordered segment sum, exact on integers
            _exact(v.grad, F.reduce64(xi[:, :C], inv, m, False), f"n={N} C={C} slice gradient")


def test_subsample_cat_slice_and_modes():
    import lidog_amd.me as ME
    pts, inv, vox = _field_points(257, 77)
    m = vox.shape[0]
    first = np.full(m, -1)
    for i in range(256, -1, -1):
        first[inv[i]] = i
    x = _dev(_operands(257, "randn"), 7).requires_grad_(True)
    field = ME.TensorField(x, pts.cuda(), quantization_mode=ME.SparseTensorQuantizationMode.RANDOM_SUBSAMPLE)
    assert field.F is x and field.features is x and field.C is field.coordinates and field.shape == (257, 7)
    assert field.device == x.device
    st = field.sparse()
    assert torch.equal(st.F.detach(), x.detach()[torch.from_numpy(first).cuda()])
    g = _dev(_operands(m, "randn2"), 7)
    st.F.backward(g)
    want = torch.zeros(257, 7, device="cuda")
    want[torch.from_numpy(first).cuda()] = g
    assert torch.equal(x.grad, want)
    # what SparseTensor does with the same duplicates
    rows, _ = F.floor_rows(pts, 1)
    plain = ME.SparseTensor(features=x.detach(), coordinates=torch.from_numpy(rows).int().cuda())
    assert torch.equal(plain.F, st.F.detach()) and torch.equal(plain.C, st.C)
    with pytest.raises(NotImplementedError, match="MAX_POOL"):
        field.sparse(quantization_mode=ME.SparseTensorQuantizationMode.MAX_POOL)
    with pytest.raises(NotImplementedError, match="tensor_stride"):
        field.sparse(tensor_stride=2)
    # cat_slice = [F[inverse] | field.F], differentiable in both
    v = _dev(_operands(m, "int"), 3).requires_grad_(True)
    x2 = _dev(_operands(257, "int"), 4).requires_grad_(True)
    cs = ME.SparseTensor(v, coordinate_manager=field.coordinate_manager, coordinate_map_key=1).cat_slice(field._like(x2))
    assert torch.equal(cs.F.detach(), torch.cat([v.detach()[torch.from_numpy(inv).cuda()], x2.detach()], dim=1))
    gc = _dev(_operands(257, "int"), 7)
    cs.F.backward(gc)
    assert torch.equal(x2.grad, gc[:, 3:])
    _exact(v.grad, F.reduce64(gc[:, :3].cpu(), inv, m, False), "cat_slice gradient")
    # int32 coordinates are converted
    ints = ME.TensorField(x.detach(), torch.from_numpy(rows).int().cuda())
    assert ints.C.dtype == torch.float32 and ints.inverse_mapping().cpu().tolist() == inv.tolist()


# ------------------------------------------------------------------ 4. autograd end to end
def _conv64(x, W, nbr):
    y = torch.zeros((nbr.shape[1], W.shape[2]), dtype=torch.float64)
    for k in range(nbr.shape[0]):
        rows = torch.as_tensor(nbr[k], dtype=torch.long)
        have = torch.nonzero(rows >= 0).flatten()
        if have.numel():
            y = y.index_add(0, have, x[rows[have]] @ W[k])
    return y


def _chain64(x, W, inv, m, nbr3, nbr8, w8, g_slice, g_interp):
    """loss of TensorField -> sparse (average) -> 3^3 convolution -> slice and -> interpolate, in float64 torch"""
    inv_t = torch.as_tensor(inv, dtype=torch.long)
    cnt = torch.bincount(inv_t, minlength=m).double().unsqueeze(1)
    v = torch.zeros((m, x.shape[1]), dtype=torch.float64).index_add(0, inv_t, x) / cnt
    out = _conv64(v, W, nbr3)
    loss = (out[inv_t] * g_slice).sum()
    for k in range(8):
        rows = torch.as_tensor(nbr8[k], dtype=torch.long)
        have = torch.nonzero(rows >= 0).flatten()
        if have.numel():
            loss = loss + (torch.as_tensor(w8[k])[have].unsqueeze(1) * out[rows[have]] * g_interp[have]).sum()
    return loss


def test_autograd_field_to_convolution_to_points():
    """Gradients of the point features and of the kernel through TensorField -> sparse -> MinkowskiConvolution(3) ->
    slice and -> interpolate against float64.  Bound: the composition of linear maps with R roundings along a path errs
    by at most gamma_R times the same chain evaluated on absolute values (Higham 3.3 applied stage by stage): the
    average (cnt - 1 additions, a division), the convolution in any order (27 Cin products and additions), the slice (a
    copy) or the interpolation (5 + 8), the gradients' segment sums (the longest list) and the final sum of both
    branches; nothing in it is measured."""
    import lidog_amd.me as ME
    Cin, Cout = 4, 8
    pts, inv, vox = _field_points(257, 55, hot=70)
    N, m = pts.shape[0], vox.shape[0]
    torch.manual_seed(3)
    conv = ME.MinkowskiConvolution(Cin, Cout, kernel_size=3, dimension=3).cuda()
    x = _dev(_operands(N, "randn"), Cin).requires_grad_(True)
    g1, g2 = _dev(_operands(N, "randn2"), Cout), _dev(_operands(N, "randn")[:, 50:], Cout)
    field = ME.TensorField(x, pts.cuda())
    out = conv(field.sparse())
    loss = (out.slice(field).F * g1).sum() + (out.interpolate(field).F * g2).sum()
    loss.backward()
    nbr3 = R.neighbours(vox, vox, 3, 1, 1)
    nbr8, w8 = F.neighbours(vox, pts, 1)
    x64 = x.detach().double().cpu().requires_grad_(True)
    W64 = conv.kernel.detach().double().cpu().requires_grad_(True)
    ref = _chain64(x64, W64, inv, m, nbr3, nbr8, w8, g1.double().cpu(), g2.double().cpu())
    ref.backward()
    xa = x64.detach().abs().requires_grad_(True)
    Wa = W64.detach().abs().requires_grad_(True)
    _chain64(xa, Wa, inv, m, nbr3, nbr8, np.abs(w8), g1.double().cpu().abs(), g2.double().cpu().abs()).backward()
    longest = int(np.bincount(inv).max()) + int(np.bincount(nbr8[nbr8 >= 0], minlength=m).max())
    rounds = (longest + 1) + 2 * 27 * max(Cin, Cout) + 13 + longest + 27 + 2
    rounds_w = rounds + N + m        # the kernel's gradient also sums over every pair of the map
    _inside(x.grad, x64.grad, float(F.gamma(rounds)) * xa.grad, "gradient of the point features")
    _inside(conv.kernel.grad, W64.grad, float(F.gamma(rounds_w)) * Wa.grad, "gradient of the kernel")


# ------------------------------------------------------------------ 5. error paths
def test_error_paths():
    import lidog_amd.me as ME
    cm = _manager("dense_cube_odd")
    m = cm.maps[1].n
    x = ME.SparseTensor(torch.ones((m, 4), device="cuda"), coordinate_manager=cm, coordinate_map_key=1)
    good = torch.tensor([[0., 1., 7., 0.5]], device="cuda")
    assert x.features_at_coordinates(good).shape == (1, 4)
    nan_q = torch.tensor([[0., 1., NAN, 0.5]], device="cuda")
    with pytest.raises(ValueError, match="NaN or infinite"):
        x.features_at_coordinates(nan_q)
    with pytest.raises(ValueError, match="batch column"):
        x.features_at_coordinates(torch.tensor([[0.5, 1., 7., 0.5]], device="cuda"))
    # a deferred check: the word collects the bits, the rows of the bad queries are zeros
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = x.features_at_coordinates(torch.cat([good, nan_q, torch.tensor([[7.5, 1., 7., 0.5]], device="cuda")]), err=err)
    assert err.item() == 3 and y[0].abs().sum().item() > 0 and not bool(y[1:].any())
    with pytest.raises(ValueError, match="NaN"):
        ME.field_error(err.item())
    with pytest.raises(ValueError, match=r"\[N, 4\]"):
        x.features_at_coordinates(torch.zeros((3, 3), device="cuda"))
    # finite queries outside the coordinate range simply have no neighbours
    far = torch.tensor([[0., 1e6, 7., 0.5], [0., -3e9, 7., 0.5]], device="cuda")
    assert not bool(x.features_at_coordinates(far).any())
    with pytest.raises(ValueError, match="NaN or infinite"):
        ME.TensorField(torch.ones((1, 2), device="cuda"), nan_q).sparse()
    with pytest.raises(ValueError, match="batch column"):
        ME.TensorField(torch.ones((1, 2), device="cuda"), torch.tensor([[0.5, 1., 7., 0.5]], device="cuda")).sparse()
    # slicing a foreign map
    pts, inv, vox = _field_points(64, 91)
    field = ME.TensorField(torch.ones((64, 4), device="cuda"), pts.cuda())
    with pytest.raises(ValueError, match="slice: valid only"):       # before .sparse(): no map at all
        x.slice(field)
    st = field.sparse()
    with pytest.raises(ValueError, match="slice: valid only"):       # another manager
        x.slice(field)
    with pytest.raises(ValueError, match="slice: valid only"):
        x.cat_slice(field)
    coarse = ME.MinkowskiAvgPooling(2, 2, dimension=3)(st)           # the right manager, the wrong tensor stride
    with pytest.raises(ValueError, match="slice: valid only"):
        coarse.slice(field)
    assert coarse.interpolate(field).F.shape == (64, 4)              # interpolation works on any map of any manager
    assert x.interpolate(field).F.shape == (64, 4)
    with pytest.raises(ValueError, match="feature rows|do not match"):
        ME.TensorField(torch.ones((3, 4), device="cuda"), pts.cuda())
