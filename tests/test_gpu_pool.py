"""Sparse pooling on the GPU (csrc/pool.hip behind lidog_pool_rows[_max|_max_bwd] and lidog_pool_global[_bwd], and the
modules of lidog_amd.me on top of them) against the float64 yardstick tests/pool_ref.py on the edge-case scenes of
tests/sconv_ref.py.

Every assertion is either an exact equality the contract promises (sum and max of small integers, the argmax, max's
gradient of integers, two runs, the module path against the C ABI, MinkowskiLinear against the 1x1 convolution) or the
derived bound of pool_ref (nothing in it is measured on the kernels).  Results are pre-filled with NaN: a row left
unwritten fails.  The references are computed once per map at the largest channel count and cut by column: pooling
treats every channel alone.

Channel counts: 1 (scalar path), 3 (scalar, a remainder), 4 (one float4), 32 (a full wave of float4 per 8 rows), 100
(float4, the last wave of a workgroup partly idle)."""
import pytest
import torch

import pool_ref as P
import sconv_ref as R

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
CHANNELS = (1, 3, 4, 32, 100)
CMAX = max(CHANNELS)
FWD_KINDS = ("k2s2", "k3s1", "k3s2", "k3s1d2", "k5s1")
BWD_KINDS = ("k2s2", "k3s1", "k3s2")
SCENES = ("dense_cube_odd", "isolated", "line_x129", "tiny_1", "tiny_127", "tiny_129", "twin_scans", "range_ends")
MODES = ("sum", "avg", "max")
_CMS, _OPS = {}, {}


# ------------------------------------------------------------------ helpers
def _manager(name):
    import lidog_amd.me as ME
    if name not in _CMS:
        c = torch.from_numpy(R.scene(name)).cuda()
        _CMS[name] = ME.SparseTensor(coordinates=c, features=torch.ones((c.shape[0], 1), device="cuda")).coordinate_manager
    return _CMS[name]


def _map(name, kind):
    ks, stride, dil, _ = R.KINDS[kind]
    return _manager(name).kernel_map(1, stride, ks, dil)


def _operands(n, what):
    """[n, CMAX] on the CPU, shared and left unchanged: `int` = integers |v| <= 15 (sums exact, ties certain), `randn`"""
    if what not in _OPS:
        g = torch.Generator().manual_seed(11 if what == "int" else 12)
        _OPS[what] = torch.randint(-15, 16, (6000, CMAX), generator=g).float() if what == "int" else \
            torch.randn(6000, CMAX, generator=g)
    return _OPS[what][:n]


def _dev(t, C):
    return t[:, :C].contiguous().cuda()


def _nan(*shape, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full(shape, -7, dtype=dtype, device="cuda")
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _fill(shape, value, dtype):
    """the byte workspace of the global pooling"""
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _side(m, side):
    import lidog_amd.me as ME
    return ME._pool_side(m, side)


def _rows(x, lists, mode, counts=None):
    """lidog_pool_rows through the C ABI on explicit lists (row_ptr, row_list, other, n)"""
    from lidog_amd._lib import call, ptr
    row_ptr, row_list, other, n = lists
    y = _nan(n, x.shape[1])
    call("lidog_pool_rows", ptr(x), ptr(row_ptr), ptr(row_list), ptr(other), n, x.shape[1], 1 if mode == "avg" else 0,
         ptr(counts), ptr(y))
    return y


def _rows_max(x, lists):
    from lidog_amd._lib import call, ptr
    row_ptr, row_list, other, n = lists
    y, arg = _nan(n, x.shape[1]), _nan(n, x.shape[1], dtype=torch.int32)
    call("lidog_pool_rows_max", ptr(x), ptr(row_ptr), ptr(row_list), ptr(other), n, x.shape[1], ptr(y), ptr(arg))
    return y, arg


def _rows_max_bwd(gy, arg, lists):
    from lidog_amd._lib import call, ptr
    row_ptr, row_list, other, n = lists
    gx = _nan(n, gy.shape[1])
    call("lidog_pool_rows_max_bwd", ptr(gy), ptr(arg), ptr(row_ptr), ptr(row_list), ptr(other), n, gy.shape[1], ptr(gx))
    return gx


def _forward(x, m, mode):
    if mode == "max":
        return _rows_max(x, _side(m, "out"))
    return _rows(x, _side(m, "out"), mode), None


def _exact(got, ref64, what):
    assert torch.equal(got.double().cpu(), ref64), f"{what}: not bit-exact"


def _inside(got, ref64, bnd, what):
    r = P.worst_ratio(got, ref64, bnd)
    print(f"{what}: error / bound {r:.3g}")
    assert r <= 1.0, f"{what}: error / bound {r:.3g} (or a row left unwritten)"
    return r


# ------------------------------------------------------------------ 1. local forward, through the C ABI
@pytest.mark.parametrize("kind", FWD_KINDS)
@pytest.mark.parametrize("name", SCENES)
def test_local_forward_against_float64(name, kind, record_property):
    cin, cout, nbr = R.scene_map(name, kind)
    n_in = cin.shape[0]
    m = _map(name, kind)
    assert (m.n_in, m.n_out) == (n_in, nbr.shape[1])
    xi, xr = _operands(n_in, "int"), _operands(n_in, "randn")
    ref = {(w, mode): P.pool64(x, nbr, mode) for w, x in (("int", xi), ("randn", xr)) for mode in MODES}
    bnd = {(w, mode): P.bound(x, nbr, mode) for w, x in (("int", xi), ("randn", xr)) for mode in ("sum", "avg")}
    worst = dict.fromkeys(MODES, 0.0)
    for C in CHANNELS:
        for w, x in (("int", xi), ("randn", xr)):
            xd = _dev(x, C)
            for mode in MODES:
                what = f"{name} {kind} C={C} {w} {mode}"
                y, arg = _forward(xd, m, mode)
                yref, aref = ref[w, mode]
                if mode == "max":
                    _exact(y, yref[:, :C], what)
                    assert torch.equal(arg.long().cpu(), aref[:, :C]), f"{what}: argmax"
                elif mode == "sum" and w == "int":
                    _exact(y, yref[:, :C], what)
                else:
                    worst[mode] = max(worst[mode], _inside(y, yref[:, :C], bnd[w, mode][:, :C], what))
                y2, arg2 = _forward(xd, m, mode)
                assert torch.equal(y, y2) and (arg is None or torch.equal(arg, arg2)), f"{what}: two calls differ"
    for mode, v in worst.items():
        record_property(f"worst_ratio_{mode}", v)


# ------------------------------------------------------------------ 2. local backward and transposed pooling
@pytest.mark.parametrize("kind", BWD_KINDS)
@pytest.mark.parametrize("name", SCENES)
def test_local_backward_against_float64(name, kind, record_property):
    """gradients gathered from the input side: sum and avg through lidog_pool_rows (avg with the other side's counts),
    max through lidog_pool_rows_max_bwd on the argmax of integer operands (ties in nearly every window)"""
    cin, cout, nbr = R.scene_map(name, kind)
    n_in, n_out = cin.shape[0], nbr.shape[1]
    m = _map(name, kind)
    gi, gr = _operands(n_out, "int"), _operands(n_out, "randn")
    xi = _operands(n_in, "int").flip(0)        # the forward operand of max: other numbers than the gradient
    _, aref = P.pool64(xi, nbr, "max")
    ref = {(w, mode): P.pool_bwd64(g, nbr, n_in, mode, aref) for w, g in (("int", gi), ("randn", gr)) for mode in MODES}
    bnd = {(w, mode): P.bound_bwd(g, nbr, n_in, mode) for w, g in (("int", gi), ("randn", gr)) for mode in ("sum", "avg")}
    # a tied window reaches exactly one input: with a gradient of ones every non-empty window hands out exactly 1
    ones_ref = P.pool_bwd64(torch.ones(n_out, CMAX), nbr, n_in, "max", aref)
    assert ones_ref.sum(0).tolist() == [float((P.counts(nbr) > 0).sum())] * CMAX
    lists_in, counts_out = _side(m, "in"), m.rows("out")[0]
    worst = dict.fromkeys(MODES, 0.0)
    for C in CHANNELS:
        _, arg = _rows_max(_dev(xi, C), _side(m, "out"))
        assert torch.equal(arg.long().cpu(), aref[:, :C])
        for w, g in (("int", gi), ("randn", gr)):
            gd = _dev(g, C)
            for mode in MODES:
                what = f"{name} {kind} C={C} {w} {mode}-backward"
                if mode == "max":
                    gx = _rows_max_bwd(gd, arg, lists_in)
                else:
                    gx = _rows(gd, lists_in, "sum", counts_out if mode == "avg" else None)
                if w == "int" and mode != "avg":
                    _exact(gx, ref[w, mode][:, :C], what)
                else:   # the selected terms of max-backward are a subset of sum-backward's: its bound holds
                    b = bnd[w, "sum" if mode == "max" else mode][:, :C]
                    worst[mode] = max(worst[mode], _inside(gx, ref[w, mode][:, :C], b, what))
    for mode, v in worst.items():
        record_property(f"worst_ratio_{mode}_backward", v)


@pytest.mark.parametrize("name", SCENES)
def test_pooling_transpose_returns_to_the_fine_map(name, record_property):
    """MinkowskiPoolingTranspose(2, 2) after MinkowskiAvgPooling(2, 2): the fine map again, every fine row the average
    of the coarse rows that reach it (here: its one window); its gradient against the yardstick on the exchanged map"""
    import lidog_amd.me as ME
    cin, cout, nbr = R.scene_map(name, "k2s2")
    n, n_c = cin.shape[0], cout.shape[0]
    coords = torch.from_numpy(cin).cuda()
    worst = 0.0
    for C in CHANNELS:
        x = _dev(_operands(n, "randn"), C).requires_grad_()
        st = ME.SparseTensor(x, coordinates=coords)
        down = ME.MinkowskiAvgPooling(2, 2, dimension=3)(st)
        assert down.coordinate_map_key == 2 and down.F.shape == (n_c, C)
        mid = down.F.detach().requires_grad_()
        up = ME.MinkowskiPoolingTranspose(2, 2, dimension=3)(
            ME.SparseTensor(mid, coordinate_manager=st.coordinate_manager, coordinate_map_key=2))
        assert up.coordinate_map_key == 1 and up.F.shape == (n, C) and up.C is st.C
        nbr_t = R.transpose_map(nbr, n)
        worst = max(worst, _inside(up.F, P.unpool64(mid, nbr, n), P.bound(mid, nbr_t, "avg"), f"{name} C={C} unpool"))
        g = _dev(_operands(n, "randn").flip(0), C)
        up.F.backward(g)
        worst = max(worst, _inside(mid.grad, P.pool_bwd64(g, nbr_t, n_c, "avg"), P.bound_bwd(g, nbr_t, n_c, "avg"),
                                   f"{name} C={C} unpool-backward"))
    with pytest.raises(ValueError, match="transposed convolution must land on an existing finer coordinate map"):
        ME.MinkowskiPoolingTranspose(2, 2, dimension=3)(st)
    record_property("worst_ratio_unpool", worst)


# ------------------------------------------------------------------ 3. non-finite inputs and empty lists
@pytest.mark.parametrize("C", (3, 4, 100))
@pytest.mark.parametrize("kind", ("k3s1", "k2s2", "k3s2"))
def test_nan_and_inf_reach_exactly_the_windows_that_hold_them(kind, C):
    name = "dense_cube_odd"
    cin, cout, nbr = R.scene_map(name, kind)
    n_in = cin.shape[0]
    m = _map(name, kind)
    x = _operands(n_in, "randn")[:, :C].clone()
    r_nan, r_inf, c_nan, c_inf = 0, 5, C - 1, 0         # row 0 has the most neighbours of its scene (sconv_ref._finish)
    x[r_nan, c_nan], x[r_inf, c_inf] = NAN, INF
    hit_nan = torch.from_numpy(R.touched(nbr, [r_nan]))
    hit_inf = torch.from_numpy(R.touched(nbr, [r_inf]))
    assert 0 < int(hit_nan.sum()) < nbr.shape[1] and 0 < int(hit_inf.sum()) < nbr.shape[1]
    xd = x.cuda()
    y, arg = _rows_max(xd, _side(m, "out"))
    y, arg = y.cpu(), arg.long().cpu()
    nan_at = torch.zeros_like(y, dtype=torch.bool)
    nan_at[hit_nan, c_nan] = True
    assert torch.equal(torch.isnan(y), nan_at) and bool((arg[hit_nan, c_nan] == r_nan).all())
    inf_at = torch.zeros_like(nan_at)
    inf_at[hit_inf, c_inf] = True
    assert torch.equal(torch.isinf(y), inf_at) and bool((arg[hit_inf, c_inf] == r_inf).all())
    yref, aref = P.pool64(x, nbr, "max")
    assert torch.equal(y.double().nan_to_num(nan=1e300), yref.nan_to_num(nan=1e300)) and torch.equal(arg, aref)
    for mode in ("sum", "avg"):
        s = _rows(xd, _side(m, "out"), mode).cpu()
        assert torch.equal(torch.isnan(s), nan_at) and torch.equal(torch.isinf(s), inf_at), mode
        assert bool((s[inf_at] == INF).all())
        x0 = x.clone()
        x0[r_nan, c_nan], x0[r_inf, c_inf] = 0.0, 0.0
        fin = ~(nan_at | inf_at)
        err = (s.double() - P.pool64(x0, nbr, mode)[0]).abs()
        assert bool((err[fin] <= P.bound(x0, nbr, mode)[fin]).all()), mode
    # the gradient of max hands a NaN / inf window's gradient to the row that holds the NaN / inf
    g = _operands(nbr.shape[1], "int")[:, :C].contiguous()
    gx = _rows_max_bwd(g.cuda(), arg.int().cuda(), _side(m, "in"))
    _exact(gx, P.pool_bwd64(g, nbr, n_in, "max", aref), f"{kind} C={C} max-backward with NaN")


def _walk(lists, x, mode):
    """what the kernels are specified to do on explicit lists, row by row in float64 (only for the doctored lists of
    the test below: the neighbour tables of sconv_ref have no row without pairs)"""
    row_ptr, row_list, other, n = lists
    row_ptr, row_list, other = row_ptr.cpu().tolist(), row_list.cpu().tolist(), other.cpu().tolist()
    x = x.double().cpu()
    y = torch.zeros((n, x.shape[1]), dtype=torch.float64)
    arg = torch.full((n, x.shape[1]), -1, dtype=torch.long)
    for r in range(n):
        rows = [other[row_list[j]] for j in range(row_ptr[r], row_ptr[r + 1])]
        if not rows:
            continue
        v = x[rows]
        if mode == "max":
            at = (v == v.max(0).values).int().argmax(0)
            y[r], arg[r] = v.gather(0, at.unsqueeze(0))[0], torch.tensor(rows)[at]
        else:
            y[r] = v.sum(0) / (len(rows) if mode == "avg" else 1)
    return y, arg


@pytest.mark.parametrize("C", (1, 4, 100))
def test_rows_without_pairs_and_all_minus_inf(C):
    """a row_ptr with empty ranges at the first row, in the middle and at the last row (the pairs of an emptied row go to
    its successor, so every index stays one the map owns): zeros, arg = -1, no 0 / 0 in avg"""
    m = _map("line_x129", "k3s1")
    row_ptr, row_list, other, n = _side(m, "out")
    rp = row_ptr.clone()
    rp[1] = rp[0]
    rp[65] = rp[64]
    rp[n] = rp[n - 1]
    lists = (rp, row_list, other, n)
    empty = [0, 64, n - 1]
    x = _dev(_operands(m.n_in, "int"), C)
    for mode in MODES:
        if mode == "max":
            y, arg = _rows_max(x, lists)
            assert arg[empty].eq(-1).all()
            assert torch.equal(arg.long().cpu(), _walk(lists, x, mode)[1])
        else:
            y = _rows(x, lists, mode)
        assert bool((y[empty] == 0).all()) and bool(torch.isfinite(y).all()), mode
        ref = _walk(lists, x, mode)[0]
        if mode == "avg":
            # <= 6 integer terms: the sum is exact, the division is rounded once
            assert bool(((y.double().cpu() - ref).abs() <= P.U * ref.abs()).all())
        else:
            _exact(y, ref, f"doctored lists {mode}")
    # every list of the real map: a window of -inf only returns -inf, at its first entry
    ninf = _dev(torch.full((m.n_in, C), -INF), C)
    y, arg = _rows_max(ninf, _side(m, "out"))
    _, _, nbr = R.scene_map("line_x129", "k3s1")
    yref, aref = P.pool64(ninf, nbr, "max")
    assert bool((y == -INF).all()) and torch.equal(arg.long().cpu(), aref)


# ------------------------------------------------------------------ 4. global pooling
def _global_scene(name):
    """(coordinates on the GPU, manager) of a scene, or of the four-scan source8k batch"""
    import lidog_amd.me as ME
    if name == "source8k_x4":
        from lidog_amd import synth
        c = synth.make_batch([0, 1, 2, 3], "source8k", "cuda")["coords_int"]
        cm = ME.SparseTensor(coordinates=c, features=torch.ones((c.shape[0], 1), device="cuda")).coordinate_manager
        return cm.maps[1].coords, cm          # the rows the manager kept (duplicates dropped)
    return torch.from_numpy(R.scene(name)).cuda(), _manager(name)


def _global(x, segs, mode):
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    perm, seg_off, bid, B = segs
    n, C = x.shape
    y = _nan(B, C)
    arg = _nan(B, C, dtype=torch.int32) if mode == "max" else None
    nbytes = _lib.load().lidog_pool_global_ws(n, B, C)
    ws = _fill((max(nbytes, 1),), 0xFF, torch.uint8)      # NaN partials until written
    call("lidog_pool_global", ptr(x), n, C, B, ptr(perm), ptr(seg_off), {"sum": 0, "avg": 1, "max": 2}[mode], ptr(y),
         ptr(arg), ptr(ws), nbytes)
    return y, arg


def _global_bwd(gy, arg, n, segs, mode):
    from lidog_amd._lib import call, ptr
    perm, seg_off, bid, B = segs
    gx = _nan(n, gy.shape[1])
    call("lidog_pool_global_bwd", ptr(gy), ptr(arg), n, gy.shape[1], B, ptr(bid), ptr(seg_off),
         {"sum": 0, "avg": 1, "max": 2}[mode], ptr(gx))
    return gx


@pytest.mark.parametrize("name", ("twin_scans", "one_and_many", "source8k_x4"))
def test_global_pooling_against_float64(name, record_property):
    coords, cm = _global_scene(name)
    bid = coords[:, 0].cpu().numpy()
    n, B = coords.shape[0], int(bid.max()) + 1
    segs = cm.segments(1)
    assert segs[3] == B
    xs = {"int": _operands(n, "int") if n <= 6000 else _operands(6000, "int").repeat(-(-n // 6000), 1)[:n],
          "randn": _operands(n, "randn") if n <= 6000 else _operands(6000, "randn").repeat(-(-n // 6000), 1)[:n]}
    gy = _operands(B, "randn").flip(1)
    ref = {(w, mode): P.global64(x, bid, B, mode) for w, x in xs.items() for mode in MODES}
    bnd = {(w, mode): P.global_bound(x, bid, B, mode) for w, x in xs.items() for mode in ("sum", "avg")}
    worst = dict.fromkeys(MODES, 0.0)
    for C in CHANNELS:
        gd = _dev(gy, C)
        for w, x in xs.items():
            xd = _dev(x, C)
            for mode in MODES:
                what = f"{name} C={C} {w} global {mode}"
                y, arg = _global(xd, segs, mode)
                yref, aref = ref[w, mode]
                if mode == "max":
                    _exact(y, yref[:, :C], what)
                    assert torch.equal(arg.long().cpu(), aref[:, :C]), f"{what}: argmax"
                elif mode == "sum" and w == "int":
                    _exact(y, yref[:, :C], what)
                else:
                    worst[mode] = max(worst[mode], _inside(y, yref[:, :C], bnd[w, mode][:, :C], what))
                y2, arg2 = _global(xd, segs, mode)
                assert torch.equal(y, y2) and (arg is None or torch.equal(arg, arg2)), f"{what}: two calls differ"
                gx = _global_bwd(gd, arg, n, segs, mode)
                gref = P.global_bwd64(gd, bid, B, mode, None if aref is None else aref[:, :C])
                _inside(gx, gref, P.global_bwd_bound(gd, bid, B, mode), what + " backward")
    for mode, v in worst.items():
        record_property(f"worst_ratio_global_{mode}", v)


@pytest.mark.parametrize("name", ("twin_scans", "one_and_many", "source8k_x4"))
def test_global_modules_origin_map_and_linear(name):
    """the result lies on the origin map -- (b, 0, 0, 0), tensor stride 0, one row per scan in batch order whatever the
    order of the input rows -- and MinkowskiLinear on it is the 1x1 convolution's bits"""
    import lidog_amd.me as ME
    coords, _ = _global_scene(name)
    n, C = coords.shape[0], 32
    bid = coords[:, 0].cpu().numpy()
    B = int(bid.max()) + 1
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(n, C, generator=gen)        # no two rows alike: the maximum's row does not depend on the row order
    shuffle = torch.randperm(n, generator=gen)
    outs, leaves = {}, {}
    for tag, rows in (("as given", torch.arange(n)), ("shuffled", shuffle)):
        leaves[tag] = x[rows].cuda().requires_grad_()
        st = ME.SparseTensor(leaves[tag], coordinates=coords[rows.cuda()].contiguous())
        for cls, mode in ((ME.MinkowskiGlobalSumPooling, "sum"), (ME.MinkowskiGlobalAvgPooling, "avg"),
                          (ME.MinkowskiGlobalMaxPooling, "max"), (ME.MinkowskiGlobalPooling, "avg")):
            out = cls()(st)
            assert out.coordinate_map_key == 0 and out.tensor_stride == [0, 0, 0] and out.F.shape == (B, C)
            assert out.C.cpu().tolist() == [[b, 0, 0, 0] for b in range(B)]
            assert out.C is cls()(st).C, "the origin map is created once per manager"
            yref, _ = P.global64(x, bid, B, mode)
            _inside(out.F, yref, P.global_bound(x, bid, B, mode), f"{name} {tag} {mode}")
            outs[tag, mode] = out
    assert torch.equal(outs["as given", "max"].F, outs["shuffled", "max"].F)
    # autograd through the module: the gradient of the shuffled rows is the shuffled gradient of max
    g = _dev(_operands(B, "randn"), C)
    grads = {}
    for tag in ("as given", "shuffled"):
        (grads[tag],) = torch.autograd.grad(outs[tag, "max"].F, leaves[tag], g)
    assert torch.equal(grads["as given"][shuffle.cuda()], grads["shuffled"])
    # MinkowskiLinear: state-dict keys of ME, the bits of MinkowskiConvolution(kernel_size=1, bias=True)
    feat = outs["as given", "max"]
    lin = ME.MinkowskiLinear(C, 5).cuda()
    conv = ME.MinkowskiConvolution(C, 5, kernel_size=1, bias=True, dimension=3).cuda()
    assert sorted(lin.state_dict()) == ["linear.bias", "linear.weight"]
    with torch.no_grad():
        conv.kernel.copy_(lin.linear.weight.t())
        conv.bias.copy_(lin.linear.bias.view(1, -1))
    src = ME.SparseTensor(feat.F.detach().requires_grad_(), coordinate_manager=feat.coordinate_manager,
                          coordinate_map_key=0)
    a, b = lin(src), conv(src)
    assert a.coordinate_map_key == 0 and torch.equal(a.F, b.F) and a.F.shape == (B, 5)
    go = _dev(_operands(B, "randn").flip(0), 5)
    ga = torch.autograd.grad(a.F, [src.F, lin.linear.weight, lin.linear.bias], go)
    gb = torch.autograd.grad(b.F, [src.F, conv.kernel, conv.bias], go)
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1].t(), gb[1]) and torch.equal(ga[2].view(1, -1), gb[2])
    # and it is a linear layer: C products and C additions per element, (C + 2) u sum |terms| (sconv_ref.bound, K = 1)
    f64, w64, b64 = feat.F.detach().double(), lin.linear.weight.detach().double(), lin.linear.bias.detach().double()
    err = (a.F.detach().double() - (f64 @ w64.t() + b64)).abs()
    assert bool((err <= (C + 2) * P.U * (f64.abs() @ w64.abs().t() + b64.abs())).all())


# ------------------------------------------------------------------ 5. modules under autograd
@pytest.mark.parametrize("C", (3, 32))
@pytest.mark.parametrize("name", ("dense_cube_odd", "twin_scans", "tiny_129"))
@pytest.mark.parametrize("cls,args,mode", [("MinkowskiMaxPooling", (2, 2), "max"), ("MinkowskiAvgPooling", (3, 1), "avg"),
                                           ("MinkowskiSumPooling", (3, 2), "sum")])
def test_modules_equal_the_c_abi_bit_for_bit(cls, args, mode, name, C):
    import lidog_amd.me as ME
    coords = torch.from_numpy(R.scene(name)).cuda()
    n = coords.shape[0]
    xv = _dev(_operands(n, "randn"), C)
    runs = []
    for _ in range(2):
        x = xv.clone().requires_grad_()
        st = ME.SparseTensor(x, coordinates=coords)
        out = getattr(ME, cls)(*args, dimension=3)(st)
        g = _dev(_operands(out.F.shape[0], "randn").flip(0), C)
        out.F.backward(g)
        runs.append((out.F.detach(), x.grad.detach()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    # the map of a convolution with the same arguments
    conv = ME.MinkowskiConvolution(C, 4, kernel_size=args[0], stride=args[1], dimension=3).cuda()
    co = conv(st)
    assert out.coordinate_map_key == co.coordinate_map_key == args[1] and out.C is co.C
    m = st.coordinate_manager.kernel_map(1, args[1], args[0], 1)
    assert st.coordinate_manager.trace[0] == ((1, args[1], args[0], 1), 0, 0)
    y, arg = _forward(xv, m, mode)
    assert torch.equal(runs[0][0], y)
    if mode == "max":
        gx = _rows_max_bwd(g, arg, _side(m, "in"))
    else:
        gx = _rows(g, _side(m, "in"), "sum", m.rows("out")[0] if mode == "avg" else None)
    assert torch.equal(runs[0][1], gx)


def test_gelu_and_functional_relu_act_on_the_features():
    import lidog_amd.me as ME
    coords = torch.from_numpy(R.scene("tiny_129")).cuda()
    x = _dev(_operands(129, "randn"), 32)
    st = ME.SparseTensor(x.clone(), coordinates=coords)
    out = ME.MinkowskiFunctional.relu(st)
    assert torch.equal(out.F, torch.relu(x)) and torch.equal(st.F, x) and out.coordinate_map_key == 1
    assert torch.equal(ME.MinkowskiGELU()(st).F, torch.nn.functional.gelu(x))


# ------------------------------------------------------------------ 6. a small classifier
def _classifier(seed=0):
    import lidog_amd.me as ME
    import torch.nn as nn

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = ME.MinkowskiConvolution(1, 32, kernel_size=3, stride=2, dimension=3)
            self.bn = ME.MinkowskiBatchNorm(32)
            self.relu = ME.MinkowskiReLU(inplace=True)
            self.pool = ME.MinkowskiMaxPooling(2, 2, dimension=3)
            self.block = ME.BasicBlock(32, 32, dimension=3)
            self.gelu = ME.MinkowskiGELU()
            self.glob = ME.MinkowskiGlobalMaxPooling()
            self.fc = ME.MinkowskiLinear(32, 2)

        def forward(self, x):
            x = self.pool(self.relu(self.bn(self.conv(x))))
            return self.fc(self.glob(self.gelu(self.block(x))))

    torch.manual_seed(seed)
    return Net().cuda()


def _two_scans():
    from lidog_amd import synth
    b = synth.make_batch([0, 1], "source8k", "cuda")
    return b["coords_int"], b["source_features0"]


def test_a_small_classifier_trains_and_prepares():
    import lidog_amd.me as ME
    coords, feats = _two_scans()
    target = torch.tensor([0, 1], device="cuda")
    net = _classifier().train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    # (c) first: the same weights through a lazy and through a prepared manager
    lazy_in = ME.SparseTensor(feats, coordinates=coords)
    lazy = net(lazy_in)
    trace = lazy_in.coordinate_manager.trace
    assert [t for t in trace if t[1] == 0] == [((2, 4, 2, 1), 0, 0)] and trace[-1] == (("identity", 0), 32, 2)
    cm = ME.CoordinateManager.prepare(coords, trace)
    assert (2, 4, 2, 1) in cm.kmaps and set(cm.kmaps[(2, 4, 2, 1)]._rows) == {"out", "in"}
    prepared = net(ME.SparseTensor(feats, coordinates=coords, coordinate_manager=cm))
    assert lazy.F.shape == (2, 2) and lazy.coordinate_map_key == 0
    assert torch.equal(lazy.F, prepared.F), "prepared and lazy managers differ"
    losses = []
    for it in range(20):
        opt.zero_grad()
        logits = net(ME.SparseTensor(feats, coordinates=coords))
        loss = torch.nn.functional.cross_entropy(logits.F, target)
        loss.backward()
        if it == 0:     # (a) every parameter receives a finite gradient
            for name, p in net.named_parameters():
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
                assert p.grad.shape == p.shape, name
            assert bool(net.fc.linear.weight.grad.abs().sum() > 0) and bool(net.conv.kernel.grad.abs().sum() > 0)
        opt.step()
        losses.append(float(loss.detach()))
    print("losses", [round(v, 4) for v in losses])
    assert losses[-1] < losses[0], losses                               # (b)
    # (d) the trunk executor still takes MinkUNet34
    from helpers import seeded_state_dict
    from lidog_amd import synth
    from lidog_amd.train import build_model, build_step
    unet = build_model("MinkUNet34", bound_2d=50.0, device="cpu")
    unet.load_state_dict(seeded_state_dict(unet, seed=5), strict=False)
    _, step, _ = build_step(unet.cuda().train(), "MinkUNet34")
    step.training_step(synth.make_batch([3, 4], "source8k", "cuda"))
    assert step.last_path == "_TrunkFnBackward"


# ------------------------------------------------------------------ 7. fp32 under bf16
def test_linear_and_pooling_stay_fp32_under_a_bf16_context():
    import lidog_amd.me as ME
    from lidog_amd import precision
    coords, feats = _two_scans()
    net = _classifier().eval()
    with torch.no_grad():
        st = ME.SparseTensor(feats, coordinates=coords)
        mid = net.relu(net.bn(net.conv(st)))
        outside = net.pool(mid).F.clone()
        plain = net(ME.SparseTensor(feats, coordinates=coords)).F.clone()
        with precision.bf16_inference(net) as ctx:
            inside = net.pool(mid).F.clone()
            logits = net(ME.SparseTensor(feats, coordinates=coords))
        assert ctx.routes[net.fc] == {precision.FP32}
        assert ctx.routes[net.conv] == {precision.FP32}                  # Cin = 1: not eligible, as before
        assert not any(isinstance(k, ME._PoolBase) for k in ctx.routes)  # pooling has no matrix operand: not counted
        assert any(r in precision.BF16_ROUTES for r in ctx.routes[net.block.conv1])
        assert not precision.eligible(net.fc)
    assert torch.equal(inside, outside)
    assert bool(torch.isfinite(logits.F).all()) and not torch.equal(logits.F, plain)    # the block did run in bf16
