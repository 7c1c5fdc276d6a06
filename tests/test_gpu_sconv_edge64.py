"""The sparse convolution's forward pass and data gradient -- the gathered GEMM (lidog_sconv_gemm on both cores, with one
or several units per workgroup, _small / _cin8 / _cout8, _in_bn, _addend), the reductions (lidog_sconv_reduce[_stats],
lidog_sconv_reduce_rows[_stats|_bn|_bwdstats]), the stem (lidog_sconv_cin1) and the output-stationary kernels
(lidog_sconv_os[_stats|_bn|_stats_in_bn]) -- and the coordinate maps under them, on the edge-case scenes of
tests/sconv_ref.py against its float64 yardstick, which is built from the coordinates alone.

Every assertion is one of three kinds: the derived bound sconv_ref.bound (nothing in it is measured on the kernels), an
exact equality the project already promises (the forms of one convolution among each other, the CPU oracle's exact mode,
the device maps and the neighbour sets), or a bar quoted from tests/test_gpu_sconv_os.py (the float64 statistics sums
within 1e-10 |ref| + 1e-9 of the float64 column sums of the kernel's own output, the row count exact, the mean within
rtol 1e-5 / atol 1e-6).

Outputs, product rows, sums and workspaces are pre-filled with NaN: a row, a partial or a column left unwritten fails.
Poisoned rows (NaN, +Inf) in the inputs must reach exactly the rows whose neighbour set meets them: the kernels load
from a clamped index and mask afterwards, which is right only while the mask is a select (0 * Inf is NaN) and the padded
rows of the last 128-row tile reach neither a store nor a statistics sum.  No index leaves its range in any of this.

range_ends goes through ME.SparseTensor with the batch indices 0 and 4095 and coordinates -65536 and 65535, the ends of
the range include/lidog_amd.h documents."""
import numpy as np
import pytest
import torch

import sconv_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
# the network's channel tiles (minkunet.py:PLANES) and the generic fallbacks
SHAPES = [(32, 32), (64, 64), (96, 96), (128, 96), (256, 128), (384, 256), (1, 32), (96, 7), (20, 12), (5, 7)]
FULL = ("dense_cube", "line_x129", "isolated")
CASES = [(s, a, b) for s in R.SCENES for a, b in (SHAPES if s in FULL else SHAPES[:1] + SHAPES[3:4])]
IDS = [f"{s}-{a}x{b}" for s, a, b in CASES]
POISON_SCENES = ("dense_cube", "isolated", "line_x129", "twin_scans")
POISON = [(s, a, b) for s in POISON_SCENES for a, b in ((32, 32), (128, 96), (20, 12))] + \
    [(s, a, b) for s in ("isolated", "line_x129") for a, b in ((96, 7), (5, 7), (1, 32))]     # _cout8, _small, _cin8
_CMS = {}


@pytest.fixture(autouse=True)
def _restore_switches():
    from lidog_amd import _lib
    yield
    L = _lib.load()
    L.lidog_set_sparse_core(1)
    L.lidog_sconv_gemm_units(1, 0)


def _cm(name):
    """a fresh coordinate manager of a scene"""
    import lidog_amd.me as ME
    c = torch.from_numpy(R.scene(name)).cuda()
    st = ME.SparseTensor(coordinates=c, features=torch.ones((c.shape[0], 1), device="cuda"))
    return ME, st.coordinate_manager


def _map(name, kind):
    """the device kernel map fine -> coarse of a map kind, on one manager per scene shared by the C ABI tests"""
    if name not in _CMS:
        _CMS[name] = _cm(name)[1]
    ks, stride, dil, _ = R.KINDS[kind]
    return _CMS[name].kernel_map(1, stride, ks, dil)


def _operands(n_in, n_out, K, Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = _dev(torch.randn(n_in, Cin, generator=g))
    W = _dev(torch.randn(K, Cin, Cout, generator=g) * 0.1)
    b = _dev(torch.randn(Cout, generator=g))
    gy = _dev(torch.randn(n_out, Cout, generator=g))
    ad = _dev(torch.randn(n_in, Cin, generator=g))
    return x, W, b, gy, ad


def _dev(t):
    """every float operand the tests own"""
    return t.cuda()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _all_equal(forms, what):
    names = list(forms)
    for name in names[1:]:
        assert torch.equal(forms[names[0]], forms[name]), f"{what}: {name} differs from {names[0]}"
    return forms[names[0]]


def _inside(got, ref, bnd, what):
    assert bool(torch.isfinite(got).all()), f"{what}: a row was left unwritten (NaN) or is not finite"
    r = R.worst_ratio(got, ref, bnd)
    assert r <= 1.0, f"{what}: error / bound {r:.3g}"
    return r


def _sums_bar(sums, out, n, what):
    """tests/test_gpu_sconv_os.py: the float64 sums against the float64 column sums of the kernel's own output"""
    ref = torch.cat([out.double().sum(0), (out.double() ** 2).sum(0)])
    assert bool(((sums[:-1] - ref).abs() <= 1e-10 * ref.abs() + 1e-9).all()), f"{what}: sums"
    assert sums[-1].item() == n, f"{what}: row count"


# ------------------------------------------------------------------ a. maps
def _check_map(m, nbr, n_in, what):
    K, n_out = nbr.shape
    assert (m.K, m.n_in, m.n_out) == (K, n_in, n_out), what
    assert np.array_equal(m.nbr.cpu().numpy(), nbr), f"{what}: neighbour table"
    k_off, pin, pout = R.pairs(nbr)
    P = int(k_off[-1])
    assert [int(v) for v in m.k_off_host] == k_off.tolist() and m.k_off.cpu().tolist() == k_off.tolist(), f"{what}: k_off"
    assert m.P == P and np.array_equal(m.pair_in.cpu().numpy(), pin) and np.array_equal(m.pair_out.cpu().numpy(), pout), \
        f"{what}: pair lists"
    ks = np.repeat(np.arange(K), np.diff(k_off))
    for side, rows, n in (("out", pout, n_out), ("in", pin, n_in)):
        want = np.full((K, n), -1, dtype=np.int64)
        want[ks, rows] = np.arange(P)
        pos = m.pos_out if side == "out" else m.pos_in
        assert np.array_equal(pos.cpu().numpy(), want), f"{what}: pos_{side}"
        row_ptr, row_list = m.rows(side)
        assert np.array_equal(row_ptr.cpu().numpy(), np.concatenate([[0], np.cumsum((want >= 0).sum(axis=0))])), \
            f"{what}: row_ptr {side}"
        assert np.array_equal(row_list.cpu().numpy()[:P], want.T[want.T >= 0]), f"{what}: row_list {side}"
    t = m.tiles.cpu().numpy()[:, :m.n_tiles].astype(np.int64)
    order = np.argsort(t[1], kind="stable")
    tk, r0, nr = t[0][order], t[1][order], t[2][order]
    assert (nr > 0).all() and (nr <= 128).all() and nr.sum() == P, f"{what}: tiles"
    assert (r0 >= k_off[tk]).all() and (r0 + nr <= k_off[tk + 1]).all() and (r0[1:] == (r0 + nr)[:-1]).all(), \
        f"{what}: a tile straddles an offset or leaves a gap"


@pytest.mark.parametrize("name", list(R.SCENES))
def test_device_maps_equal_the_neighbour_sets(name):
    """every map kind of every scene: neighbour table, k_off, pair lists, position tables, per-row lists, tiles and the
    strided coordinates; the 3^3 map both probed and taken from the 5^3 table (lidog_kernel_map_subset)"""
    coords = R.scene(name)
    ME, cm = _cm(name)
    _, cm5 = _cm(name)
    cm5.kernel_map(1, 1, 5)
    assert np.array_equal(cm.maps[1].coords.cpu().numpy(), coords)
    assert cm.batch_size == int(coords[:, 0].max()) + 1
    for kind, (ks, stride, dil, transposed) in R.KINDS.items():
        if transposed:
            # the k2 s2 map with input and output exchanged, as MinkowskiConvolutionTranspose reads it: gather from
            # pair_out, scatter to pair_in, every fine row exactly once
            coarse, fine, nbr_t = R.scene_map(name, kind)
            m = cm.kernel_map(1, stride, ks, dil)
            src, dst = m.pair_out.cpu().numpy().astype(np.int64), m.pair_in.cpu().numpy().astype(np.int64)
            kk = np.repeat(np.arange(m.K), np.diff(np.asarray(m.k_off_host, dtype=np.int64)))
            got = np.full((m.K, fine.shape[0]), -1, dtype=np.int64)
            got[kk, dst] = src
            assert np.array_equal(got, nbr_t), f"{name} {kind}: exchanged map"
            assert np.array_equal(np.sort(dst), np.arange(fine.shape[0])), f"{name} {kind}: a fine row without one parent"
            assert np.array_equal((m.pos_in.cpu().numpy() >= 0), nbr_t >= 0), f"{name} {kind}: pos_in"
            continue
        fine, coarse, nbr = R.scene_map(name, kind)
        for tag, mgr in (("probed", cm), ("after 5^3", cm5)) if kind == "k3s1" else (("probed", cm),):
            _check_map(mgr.kernel_map(1, stride, ks, dil), nbr, fine.shape[0], f"{name} {kind} {tag}")
        if stride > 1:
            assert np.array_equal(cm.maps[stride].coords.cpu().numpy(), R.strided(coords, stride)), f"{name}: stride {stride}"


# ------------------------------------------------------------------ b. module path
ORACLE_BUDGET = 6e9     # multiply-adds of one pass of the CPU oracle's scalar chains (a second or two)


def _oracle_affordable(nbr, Cin, Cout):
    """every map kind is held to the bound at every shape; the equality with the oracle's exact mode where its scalar
    chains stay within ORACLE_BUDGET (all but the 5^3 map of dense blocks at 384 -> 256)"""
    return int((nbr >= 0).sum()) * Cin * Cout <= ORACLE_BUDGET


def _oracle(name, kind, x, W, b, gy, ad):
    import oracle.me_cpu as OME
    OME.set_mode("exact")
    ks, stride, dil, transposed = R.KINDS[kind]
    K, Cin, Cout = W.shape
    coords = torch.from_numpy(R.scene(name))
    cm = OME.SparseTensor(coordinates=coords, features=torch.zeros(coords.shape[0], 1)).coordinate_manager
    if transposed:
        cm.stride(1, stride)
        conv = OME.MinkowskiConvolutionTranspose(Cin, Cout, kernel_size=ks, stride=stride, bias=True, dimension=3)
    else:
        conv = OME.MinkowskiConvolution(Cin, Cout, kernel_size=ks, stride=stride, dilation=dil, bias=True, dimension=3)
    with torch.no_grad():
        conv.kernel.copy_(W.cpu())
        conv.bias.copy_(b.cpu().view(1, -1))
    xin = x.cpu().clone().requires_grad_(True)
    out = conv(OME.SparseTensor(features=xin, coordinate_manager=cm, coordinate_map_key=stride if transposed else 1))
    out.F.backward(gy.cpu())
    return out.F.detach(), xin.grad + ad.cpu() if ad is not None else xin.grad


def _module(ME, name, kind, x, W, b, gy, ad, stats):
    ks, stride, dil, transposed = R.KINDS[kind]
    K, Cin, Cout = W.shape
    _, cm = _cm(name)        # a fresh manager: the sorted-rows decision of its maps follows ME._SCONV_OS
    cls = ME.MinkowskiConvolutionTranspose if transposed else ME.MinkowskiConvolution
    conv = cls(Cin, Cout, kernel_size=ks, stride=stride, dilation=dil, bias=True, dimension=3).cuda()
    with torch.no_grad():
        conv.kernel.copy_(W.view_as(conv.kernel))
        conv.bias.copy_(b.view(1, -1))
    if transposed:
        cm.stride(1, stride)
    xg = x.clone().requires_grad_(True)
    st = ME.SparseTensor(xg, coordinate_manager=cm, coordinate_map_key=stride if transposed else 1)
    req = ME.StatsRequest(torch.nn.BatchNorm1d(Cout).cuda(), False, 0.1) if stats else None
    if ad is not None:
        out, alias = conv(st, stats=req, skip=True)
        torch.autograd.backward([out.F, alias.F], [gy, ad])
    else:
        out = conv(st, stats=req)
        out.F.backward(gy)
    torch.cuda.synchronize()
    return out.F.detach(), xg.grad, req, cm


@pytest.mark.parametrize("name,Cin,Cout", CASES, ids=IDS)
def test_module_path_forward_and_backward(name, Cin, Cout, monkeypatch, record_property):
    """MinkowskiConvolution / ConvolutionTranspose with bias, forward and backward, on both sparse cores and with the
    output-stationary kernel wherever legal (ME._SCONV_OS = 2) and nowhere (0); skip=True and a statistics request as
    BasicBlock / conv_bn use them (3^3 with Cin == Cout; statistics where Cout % 4 == 0, which every path with a
    reduction pass must fuse).  Every map kind at every shape inside the bound; torch.equal to the oracle's exact mode
    (wherever its scalar chains are affordable, _oracle_affordable); every variant bit-equal to the first; the
    output-stationary kernel taken exactly where ME._SCONV_OS = 2 makes it legal."""
    import lidog_amd.me as ME
    from lidog_amd import _lib
    L = _lib.load()
    monkeypatch.setattr(ME, "_OS_HINT", {})
    worst = 0.0
    for kind in R.KINDS:
        ks, stride, dil, transposed = R.KINDS[kind]
        cin, cout, nbr = R.scene_map(name, kind)
        x, W, b, gy, ad = _operands(cin.shape[0], cout.shape[0], ks ** 3, Cin, Cout, Cin * 131 + Cout + len(kind))
        if not (kind == "k3s1" and Cin == Cout):
            ad = None
        stats = Cout % 4 == 0
        # the paths that go through a reduction pass or the output-stationary kernel fuse the statistics
        fused = stats and not transposed and not (Cin == 1 and Cout in (16, 32, 64))
        y_ref, y_bnd = R.conv64(x, W, b, nbr), R.bound(x, W, b, nbr)
        nbr_t, Wt = R.transpose_map(nbr, cin.shape[0]), W.transpose(1, 2)
        g_ref, g_bnd = R.dgrad64(gy, W, nbr, ad, n_in=cin.shape[0]), R.bound(gy, Wt, None, nbr_t, ad)
        y_orc = g_orc = None
        if _oracle_affordable(nbr, Cin, Cout):
            y_orc, g_orc = _oracle(name, kind, x, W, b, gy, ad)
        else:
            assert (kind, Cin, Cout) == ("k5s1", 384, 256), "only that case may go without the oracle"
        first = None
        for core in (1, 0):
            os_legal = kind in ("k3s1", "k3s1d2") and core == 1 and Cin % 32 == 0 and Cout % 32 == 0
            for os_mode in (2, 0) if os_legal else (0,):
                monkeypatch.setattr(ME, "_SCONV_OS", os_mode)
                assert L.lidog_set_sparse_core(core) == 0
                y, g, req, cm = _module(ME, name, kind, x, W, b, gy, ad, stats)
                what = f"{name} {kind} {Cin}->{Cout} core {core} os {os_mode}"
                m = cm.kernel_map(1, stride, ks, dil)
                took_os = ME._os_rows(m, transposed, Cin, Cout) is not None
                assert took_os == (os_legal and os_mode == 2), f"{what}: output-stationary kernel taken: {took_os}"
                worst = max(worst, _inside(y, y_ref, y_bnd, what + " forward"), _inside(g, g_ref, g_bnd, what + " dgrad"))
                if first is None:
                    first = (y, g)
                    if y_orc is not None:
                        assert torch.equal(y.cpu(), y_orc), f"{what}: forward differs from the oracle's exact mode"
                        assert torch.equal(g.cpu(), g_orc), f"{what}: data gradient differs from the oracle's exact mode"
                else:
                    assert torch.equal(y, first[0]) and torch.equal(g, first[1]), f"{what}: differs from the first variant"
                if stats:
                    assert (req.sums is not None) == fused, f"{what}: statistics fused: {req.sums is not None}"
                if fused:
                    _sums_bar(req.sums, y, y.shape[0], what)
    record_property("worst_error_over_bound", worst)


# ------------------------------------------------------------------ c / d / e. the C ABI on the 3^3 map of a scene
class Forms:
    """every form of one 3^3 convolution through the C ABI; each method takes its input and returns {name: result}
    with outputs, product rows, sums and workspaces pre-filled with NaN"""

    def __init__(self, name, Cin, Cout):
        import lidog_amd.me as ME
        from lidog_amd import _lib
        from test_gpu_sconv_os import _sorted
        self.ME, self.L = ME, _lib.load()
        self.name, self.Cin, self.Cout = name, Cin, Cout
        self.m = m = _map(name, "k3s1")
        self.n = m.n_out
        self.nbr = R.scene_map(name, "k3s1")[2]
        self.nbr_t = R.transpose_map(self.nbr, self.n)
        self.x, self.W, self.b, self.gy, self.ad = _operands(self.n, self.n, 27, Cin, Cout, Cin * 977 + Cout)
        self.Wt = _dev(self.W.transpose(1, 2).contiguous())
        self.mfma = Cin % 32 == 0 and Cout % 32 == 0
        self.sorted = _sorted(m) if self.mfma else None
        g = torch.Generator().manual_seed(Cin + 7 * Cout)
        for C, tag in ((Cin, "in"), (Cout, "out")):       # BatchNorm vectors over the input / output channels
            setattr(self, "bn_" + tag, tuple(_dev(v) for v in (
                torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5,
                torch.randn(C, generator=g) * 0.3)))          # mean, invstd, weight, bias
        self.res = _dev(torch.randn(self.n, Cout, generator=g))
        self.pre = _dev(torch.randn(self.n, Cin, generator=g) * 2 + 0.5)

    # ---- building blocks
    def product(self, A, gather, B, Cin, Cout, core=1, units=(1, 0)):
        from lidog_amd._lib import call, ptr
        m = self.m
        T = _nan(m.P, Cout)
        assert self.L.lidog_set_sparse_core(core) == 0
        self.L.lidog_sconv_gemm_units(*units)
        call("lidog_sconv_gemm", ptr(A), ptr(gather), ptr(B), None, ptr(m.tiles[0]), ptr(m.tiles[1]), ptr(m.tiles[2]),
             m.n_tiles, Cin, Cout, ptr(T), None, A.shape[0])            # the true a_rows, as the callers pass it
        self.L.lidog_set_sparse_core(1)
        self.L.lidog_sconv_gemm_units(1, 0)
        return T

    def products(self, A, gather, B, Cin, Cout):
        """the product rows on both cores and for every way the units fall onto the workgroups"""
        out = {"mfma one unit": self.product(A, gather, B, Cin, Cout, 1, (0, 0)),
               "vector fma": self.product(A, gather, B, Cin, Cout, 0)}
        for slots in (1, 7, 0):
            out[f"units(1, {slots})"] = self.product(A, gather, B, Cin, Cout, 1, (1, slots))
        return out

    def reduce_rows(self, T, side, C, bias, addend):
        from lidog_amd._lib import call, ptr
        rp, rl = self.m.rows(side)
        out = _nan(self.n, C)
        call("lidog_sconv_reduce_rows", ptr(T), ptr(rp), ptr(rl), self.n, C, ptr(bias), ptr(addend), ptr(out))
        return out

    def reduce_pos(self, T, side, C, bias, addend):
        from lidog_amd._lib import call, ptr
        pos = self.m.pos_out if side == "out" else self.m.pos_in
        out = _nan(self.n, C)
        call("lidog_sconv_reduce", ptr(T), ptr(pos), self.n, 27, C, ptr(bias), ptr(addend), ptr(out))
        return out

    def os(self, A, B, reverse, bias, addend, Cin, Cout):
        from lidog_amd._lib import call, ptr
        perm, wm, order = self.sorted
        out = _nan(self.n, Cout)
        call("lidog_sconv_os", ptr(A), ptr(self.m.nbr), self.n, 27, ptr(perm), ptr(wm), ptr(order), ptr(B), reverse,
             ptr(bias), ptr(addend), Cin, Cout, ptr(out))
        return out

    # ---- c. forward and data gradient
    def forward(self, x):
        Cin, Cout, m = self.Cin, self.Cout, self.m
        T = self.product(x, m.pair_in, self.W, Cin, Cout)
        out = {"gemm + reduce": self.reduce_pos(T, "out", Cout, self.b, None)}
        if Cout % 4 == 0:
            out["gemm + reduce_rows"] = self.reduce_rows(T, "out", Cout, self.b, None)
        if self.mfma:
            out["os"] = self.os(x, self.W, 0, self.b, None, Cin, Cout)
        return out

    def addend(self):
        return self.ad if self.Cin % 4 == 0 else None

    def dgrad(self, gy):
        Cin, Cout, m = self.Cin, self.Cout, self.m
        T = self.product(gy, m.pair_out, self.Wt, Cout, Cin)
        ad = self.addend()
        out = {"gemm + reduce": self.reduce_pos(T, "in", Cin, None, ad)}
        if Cin % 4 == 0:
            out["gemm + reduce_rows"] = self.reduce_rows(T, "in", Cin, None, ad)
            out["gemm + reduce_rows_bwdstats"] = self.bwdstats(T, False)["out"]
        if self.mfma:
            out["os mirrored"] = self.os(gy, self.Wt, 1, None, ad, Cout, Cin)
        return out

    # ---- d. fused epilogues
    def stats(self, x=None, T=None):
        """{form: (out, sums [2 Cout + 1], mean, invstd)} of the forward pass with the BatchNorm statistics of its
        result; `T`: the product rows, for the two reductions alone"""
        from lidog_amd._lib import call, ptr
        L, n, Cin, Cout, m = self.L, self.n, self.Cin, self.Cout, self.m
        T = self.product(x, m.pair_in, self.W, Cin, Cout) if T is None else T
        rp, rl = m.rows("out")
        res = {}
        for form in ("reduce_rows_stats", "reduce_stats") + (("os_stats",) if self.mfma and x is not None else ()):
            out, su, me, inv = _nan(n, Cout), _nan(2 * Cout + 1, dtype=torch.float64), _nan(Cout), _nan(Cout)
            tail = (ptr(out), ptr(su))
            fin = (float(n), 1e-5, 0.1, ptr(me), ptr(inv), None, None)
            if form == "reduce_rows_stats":
                ws = _nan(L.lidog_sconv_reduce_stats_ws(n, Cout), dtype=torch.float64)
                call("lidog_sconv_reduce_rows_stats", ptr(T), ptr(rp), ptr(rl), n, Cout, ptr(self.b), *tail, ptr(ws), *fin)
            elif form == "reduce_stats":
                ws = _nan(L.lidog_sconv_reduce_stats_ws(n, Cout), dtype=torch.float64)
                call("lidog_sconv_reduce_stats", ptr(T), ptr(m.pos_out), n, 27, Cout, ptr(self.b), *tail, ptr(ws), *fin)
            else:
                perm, wm, order = self.sorted
                ws = _nan(L.lidog_sconv_os_stats_ws(n, Cout), dtype=torch.float64)
                call("lidog_sconv_os_stats", ptr(x), ptr(m.nbr), n, 27, ptr(perm), ptr(wm), ptr(order), ptr(self.W),
                     ptr(self.b), Cin, Cout, *tail, ptr(ws), *fin)
            res[form] = (out, su, me, inv)
        return res

    def eval_bn(self, x, residual, relu, T=None):
        """{form: out} of convolution + evaluation-mode BatchNorm (+ residual) (+ ReLU) in one launch"""
        from lidog_amd._lib import call, ptr
        n, Cin, Cout, m = self.n, self.Cin, self.Cout, self.m
        mean, invstd, w, b = self.bn_out
        T = self.product(x, m.pair_in, self.W, Cin, Cout) if T is None else T
        rp, rl = m.rows("out")
        res = {"reduce_rows_bn": _nan(n, Cout)}
        call("lidog_sconv_reduce_rows_bn", ptr(T), ptr(rp), ptr(rl), n, Cout, ptr(self.b), ptr(mean), ptr(invstd), ptr(w),
             ptr(b), ptr(residual), relu, ptr(res["reduce_rows_bn"]))
        res["reduce_rows + bn_apply"] = _nan(n, Cout)     # the two-pass sequence the fused forms replace
        call("lidog_bn_apply", ptr(self.reduce_rows(T, "out", Cout, self.b, None)), n, Cout, 1, ptr(mean), ptr(invstd),
             ptr(w), ptr(b), ptr(residual), relu, ptr(res["reduce_rows + bn_apply"]))
        if self.mfma and x is not None:
            perm, wm, order = self.sorted
            res["os_bn"] = _nan(n, Cout)
            call("lidog_sconv_os_bn", ptr(x), ptr(m.nbr), n, 27, ptr(perm), ptr(wm), ptr(order), ptr(self.W), ptr(self.b),
                 Cin, Cout, ptr(mean), ptr(invstd), ptr(w), ptr(b), ptr(residual), relu, ptr(res["os_bn"]))
        return res

    def bwdstats(self, T, relu):
        """{"out", "sums", "dw", "db"} of the data-gradient reduction with the BatchNorm-backward sums of the layer
        before in its epilogue; `relu`: that layer's ReLU mask recomputed from its input (relu_w, relu_b)"""
        from lidog_amd._lib import call, ptr
        n, C = self.n, self.Cin
        mean, invstd, w, b = self.bn_in
        rp, rl = self.m.rows("in")
        out, su, dw, db = _nan(n, C), _nan(2 * C + 1, dtype=torch.float64), _nan(C), _nan(C)
        ws = _nan(self.L.lidog_bn_reduce_ws(C, 1), dtype=torch.float64)
        call("lidog_sconv_reduce_rows_bwdstats", ptr(T), ptr(rp), ptr(rl), n, C, ptr(self.addend()), ptr(out), ptr(self.pre),
             None, None, ptr(mean), ptr(invstd), ptr(w) if relu else None, ptr(b) if relu else None, ptr(su), ptr(ws),
             float(n), ptr(dw), ptr(db))
        return {"out": out, "sums": su, "dw": dw, "db": db}

    def bwd_two_pass(self, T, relu):
        from lidog_amd._lib import call, ptr
        n, C = self.n, self.Cin
        mean, invstd, w, b = self.bn_in
        out = self.reduce_rows(T, "in", C, None, self.addend())
        su, dw, db = _nan(2 * C + 1, dtype=torch.float64), _nan(C), _nan(C)
        ws = _nan(self.L.lidog_bn_reduce_ws(C, 1), dtype=torch.float64)
        call("lidog_bn_bwd_reduce", ptr(out), ptr(self.pre), None, n, C, 1, ptr(mean), ptr(invstd), ptr(su), ptr(ws),
             float(n), ptr(dw), ptr(db), ptr(w) if relu else None, ptr(b) if relu else None)
        return {"out": out, "sums": su, "dw": dw, "db": db}

    def apply_bn(self, xraw, relu):
        from lidog_amd._lib import call, ptr
        mean, invstd, w, b = self.bn_in
        y = _nan(self.n, self.Cin)
        call("lidog_bn_apply_bits", ptr(xraw), self.n, self.Cin, 1, ptr(mean), ptr(invstd), ptr(w), ptr(b), None, relu,
             ptr(y), None)
        return y

    def wgrad(self, A, G, core=1, in_bn=None):
        """lidog_sconv_wgrad[_in_bn] over 128-pair items; gW and the partial slots pre-filled with NaN"""
        from lidog_amd._lib import call, ptr
        m, Cin, Cout = self.m, self.Cin, self.Cout
        items, n_items, item_off = self.ME._wgrad_items_host(m.k_off_host, 128)
        items = torch.from_numpy(np.ascontiguousarray(items)).cuda()
        item_off = torch.from_numpy(item_off).cuda()
        partial = _nan(max(self.L.lidog_sconv_wgrad_slabs(Cin, Cout, n_items), 1), Cin, Cout)
        gW = _nan(27, Cin, Cout)
        assert self.L.lidog_set_sparse_core(core) == 0
        head = (ptr(A), ptr(m.pair_in), ptr(G), ptr(m.pair_out), ptr(items), n_items, ptr(item_off), 27, Cin, Cout,
                ptr(partial), ptr(gW))
        if in_bn is None:
            call("lidog_sconv_wgrad", *head)
        else:
            call("lidog_sconv_wgrad_in_bn", *head, *(ptr(v) for v in self.bn_in), in_bn)
        self.L.lidog_set_sparse_core(1)
        return gW

    def in_bn(self, xraw, relu):
        """{form: (folded, two-step)}: the three forms that apply the BatchNorm (+ ReLU) of the layer before in their
        staging, and lidog_bn_apply_bits followed by the plain entry point"""
        from lidog_amd._lib import call, ptr
        L, n, Cin, Cout, m = self.L, self.n, self.Cin, self.Cout, self.m
        vec = tuple(ptr(v) for v in self.bn_in)
        y = self.apply_bn(xraw, relu)
        res = {}
        T = _nan(m.P, Cout)
        call("lidog_sconv_gemm_in_bn", ptr(xraw), ptr(m.pair_in), ptr(self.W), None, ptr(m.tiles[0]), ptr(m.tiles[1]),
             ptr(m.tiles[2]), m.n_tiles, Cin, Cout, ptr(T), None, *vec, relu, xraw.shape[0])
        res["gemm_in_bn"] = (T, self.product(y, m.pair_in, self.W, Cin, Cout))
        perm, wm, order = self.sorted
        out, su, me, inv = _nan(n, Cout), _nan(2 * Cout + 1, dtype=torch.float64), _nan(Cout), _nan(Cout)
        ws = _nan(L.lidog_sconv_os_stats_ws(n, Cout), dtype=torch.float64)
        call("lidog_sconv_os_stats_in_bn", ptr(xraw), ptr(m.nbr), n, 27, ptr(perm), ptr(wm), ptr(order), ptr(self.W),
             ptr(self.b), Cin, Cout, ptr(out), ptr(su), ptr(ws), float(n), 1e-5, 0.1, ptr(me), ptr(inv), None, None, *vec,
             relu)
        plain = self.stats(y)["os_stats"]
        res["os_stats_in_bn"] = (out, plain[0])
        res["os_stats_in_bn sums"] = (su, plain[1])
        res["os_stats_in_bn mean"] = (me, plain[2])
        res["os_stats_in_bn invstd"] = (inv, plain[3])
        res["wgrad_in_bn"] = (self.wgrad(xraw, self.gy, 1, relu), self.wgrad(y, self.gy, 1))
        return res


@pytest.mark.parametrize("name,Cin,Cout", CASES, ids=IDS)
def test_c_abi_forward_and_data_gradient(name, Cin, Cout, record_property):
    """lidog_sconv_gemm (both cores; one unit per workgroup and lidog_sconv_gemm_units(1, slots), slots 1, 7, 0) +
    lidog_sconv_reduce_rows, + lidog_sconv_reduce (the `pos` form), and lidog_sconv_os forward and mirrored with addend:
    bit-equal to each other, every row written, inside the bound"""
    f = Forms(name, Cin, Cout)
    m = f.m
    _all_equal(f.products(f.x, m.pair_in, f.W, Cin, Cout), f"{name} forward product rows")
    _all_equal(f.products(f.gy, m.pair_out, f.Wt, Cout, Cin), f"{name} data-gradient product rows")
    y = _all_equal(f.forward(f.x), f"{name} {Cin}->{Cout} forward")
    r1 = _inside(y, R.conv64(f.x, f.W, f.b, f.nbr), R.bound(f.x, f.W, f.b, f.nbr), f"{name} {Cin}->{Cout} forward")
    g = _all_equal(f.dgrad(f.gy), f"{name} {Cin}->{Cout} data gradient")
    ad = f.addend()
    r2 = _inside(g, R.dgrad64(f.gy, f.W, f.nbr, ad, n_in=f.n), R.bound(f.gy, f.Wt, None, f.nbr_t, ad),
                 f"{name} {Cin}->{Cout} data gradient")
    record_property("worst_error_over_bound", max(r1, r2))


@pytest.mark.parametrize("Cin,Cout", [(32, 32), (128, 96), (256, 128), (20, 12), (5, 7)])
@pytest.mark.parametrize("name", ["isolated", "dense_cube", "dense_cube_odd"])
def test_k2_s2_direct_scatter_writes_every_row(name, Cin, Cout, record_property):
    """the single_out / single_in paths (transposed k2 s2 forward, k2 s2 data gradient) scatter the product rows straight
    into a torch.empty result: parents with 1, 2, 4 or 8 children, every fine row written once, on both cores; and the
    k2 s2 forward over the coarse rows by both reductions"""
    import lidog_amd.me as ME
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    L = _lib.load()
    m = _map(name, "k2s2")
    fine, coarse, nbr = R.scene_map(name, "k2s2")
    nbr_t = R.scene_map(name, "tr_k2s2")[2]
    n_f, n_c = fine.shape[0], coarse.shape[0]
    assert (m.n_in, m.n_out, m.P) == (n_f, n_c, n_f)
    x_c, W, b, gy_c, _ = _operands(n_c, n_c, 8, Cin, Cout, Cin + 3 * Cout)
    Wt = _dev(W.transpose(1, 2).contiguous())
    up, down = {}, {}
    for core in (1, 0):
        assert L.lidog_set_sparse_core(core) == 0
        up[core], down[core] = _nan(n_f, Cout), _nan(n_f, Cin)
        ME._gemm(x_c, m.pair_out, W, b, m, Cin, Cout, up[core], m.pair_in)          # transposed forward
        ME._gemm(gy_c, m.pair_out, Wt, None, m, Cout, Cin, down[core], m.pair_in)   # data gradient of the strided one
    L.lidog_set_sparse_core(1)
    y = _all_equal(up, f"{name} transposed k2 s2 forward")
    r1 = _inside(y, R.conv64(x_c, W, b, nbr_t), R.bound(x_c, W, b, nbr_t), f"{name} {Cin}->{Cout} transposed k2 s2 forward")
    g = _all_equal(down, f"{name} k2 s2 data gradient")
    r2 = _inside(g, R.conv64(gy_c, Wt, None, nbr_t), R.bound(gy_c, Wt, None, nbr_t), f"{name} {Cout}->{Cin} k2 s2 dgrad")
    # k2 s2 forward: product rows, then the coarse rows' reduction in both forms
    x_f = _dev(torch.randn(n_f, Cin, generator=torch.Generator().manual_seed(Cin)))
    T = _nan(m.P, Cout)
    ME._gemm(x_f, m.pair_in, W, None, m, Cin, Cout, T, None)
    forms = {"reduce": _nan(n_c, Cout)}
    call("lidog_sconv_reduce", ptr(T), ptr(m.pos_out), n_c, 8, Cout, ptr(b), None, ptr(forms["reduce"]))
    if Cout % 4 == 0:
        rp, rl = m.rows("out")
        forms["reduce_rows"] = _nan(n_c, Cout)
        call("lidog_sconv_reduce_rows", ptr(T), ptr(rp), ptr(rl), n_c, Cout, ptr(b), None, ptr(forms["reduce_rows"]))
    r3 = _inside(_all_equal(forms, f"{name} k2 s2 forward"), R.conv64(x_f, W, b, nbr), R.bound(x_f, W, b, nbr),
                 f"{name} {Cin}->{Cout} k2 s2 forward")
    record_property("worst_error_over_bound", max(r1, r2, r3))


@pytest.mark.parametrize("name,C", [(s, 32) for s in R.SCENES] + [(s, c) for s in FULL for c in (16, 64)])
def test_stem_cin1_against_the_two_pass_path(name, C, record_property):
    """lidog_sconv_cin1 on the 5^3 map (straight from the neighbour table) against lidog_sconv_gemm + both reductions"""
    import lidog_amd.me as ME
    from lidog_amd._lib import call, ptr
    m = _map(name, "k5s1")
    nbr = R.scene_map(name, "k5s1")[2]
    n = m.n_out
    x, W, b, _, _ = _operands(n, n, 125, 1, C, C)
    forms = {"cin1": _nan(n, C), "gemm + reduce": _nan(n, C), "gemm + reduce_rows": _nan(n, C)}
    call("lidog_sconv_cin1", ptr(x), ptr(m.nbr), ptr(W), ptr(b), n, 125, C, ptr(forms["cin1"]))
    T = _nan(m.P, C)
    ME._gemm(x, m.pair_in, W, None, m, 1, C, T, None)
    call("lidog_sconv_reduce", ptr(T), ptr(m.pos_out), n, 125, C, ptr(b), None, ptr(forms["gemm + reduce"]))
    rp, rl = m.rows("out")
    call("lidog_sconv_reduce_rows", ptr(T), ptr(rp), ptr(rl), n, C, ptr(b), None, ptr(forms["gemm + reduce_rows"]))
    y = _all_equal(forms, f"{name} stem 1->{C}")
    record_property("worst_error_over_bound", _inside(y, R.conv64(x, W, b, nbr), R.bound(x, W, b, nbr), f"{name} stem 1->{C}"))


@pytest.mark.parametrize("name", list(R.SCENES))
def test_gemm_addend_in_place(name, record_property):
    """lidog_sconv_gemm_addend with addend == T, the in-place use the executor makes (the classifier's data gradient,
    7 -> 96, onto rows that hold another gradient): the bits of lidog_sconv_gemm followed by addend + product, over the
    3^3 rule book and over rows taken in place (no gather index); each product row inside the bound of its one offset"""
    import lidog_amd.me as ME
    from lidog_amd._lib import call, ptr
    m = _map(name, "k3s1")
    n, Cin, Cout = m.n_out, 7, 96
    x, W, _, _, _ = _operands(n, n, 27, Cin, Cout, 5)
    worst = 0.0
    for gather, mm, rows in ((m.pair_in, m, m.P), (None, ME._IdentityMap(n, "cuda"), n)):
        K = mm.K
        ad = _dev(torch.randn(rows, Cout, generator=torch.Generator().manual_seed(rows)))
        T0 = _nan(rows, Cout)
        ME._gemm(x, gather, W, None, mm, Cin, Cout, T0, None)
        T = _dev(ad.clone())
        call("lidog_sconv_gemm_addend", ptr(x), ptr(gather), ptr(W), ptr(mm.tiles[0]), ptr(mm.tiles[1]), ptr(mm.tiles[2]),
             mm.n_tiles, Cin, Cout, ptr(T), ptr(T), None)
        assert torch.equal(T, ad + T0), f"{name}: in place differs from product, then addend + product"
        k_off = [int(v) for v in mm.k_off_host]
        for k in range(K):
            a, e = k_off[k], k_off[k + 1]
            if e > a:
                src = (gather[a:e].long().cpu().numpy() if gather is not None else np.arange(a, e))[None, :]
                ref = R.conv64(x, W[k:k + 1], None, src) + ad[a:e].double()
                worst = max(worst, _inside(T[a:e], ref, R.bound(x, W[k:k + 1], None, src, ad[a:e]), f"{name} offset {k}"))
    record_property("worst_error_over_bound", worst)


D_CASES = [(s, a, b) for s, a, b in CASES if a % 4 == 0 and b % 4 == 0]


@pytest.mark.parametrize("name,Cin,Cout", D_CASES, ids=[f"{s}-{a}x{b}" for s, a, b in D_CASES])
def test_fused_epilogues(name, Cin, Cout, record_property):
    """The statistics forms (lidog_sconv_reduce_rows_stats, lidog_sconv_reduce_stats -- the `pos` form, which no caller
    uses -- and lidog_sconv_os_stats): the convolution bit-equal to the plain reduction, the sums to the bars of
    tests/test_gpu_sconv_os.py.  The evaluation-mode BatchNorm forms (lidog_sconv_reduce_rows_bn, lidog_sconv_os_bn;
    residual and ReLU on and off): bit-equal to each other and to the two-pass sequence lidog_sconv_reduce_rows +
    lidog_bn_apply, and against float64 of the formula

        y = relu(((c - mean) * invstd) * w + b + residual),          c = the convolution with its bias,

    with the bound derived as sconv_ref.bound is: the computed c is off by at most bound(c), which the affine chain
    scales by |invstd w|; the chain itself rounds 4 times (subtract, two products, add; 5 with a residual), so every
    term of (|c| + |mean|) |invstd w| + |b| + |residual| carries at most 4 (5) factors (1 + d) and bound(c) |invstd w|
    one of them; gamma_5 <= 6 u.  The ReLU is exact and 1-Lipschitz.  Together
        |y - y64| <= bound(c) |invstd w| (1 + 6 u) + 6 u ((|c| + |mean|) |invstd w| + |b| + |residual|).
    The three _in_bn forms against lidog_bn_apply_bits + the plain entry point, and lidog_sconv_reduce_rows_bwdstats
    against lidog_sconv_reduce_rows + lidog_bn_bwd_reduce: bit-equal, as include/lidog_amd.h promises."""
    f = Forms(name, Cin, Cout)
    n, what = f.n, f"{name} {Cin}->{Cout}"
    plain = f.forward(f.x)["gemm + reduce_rows"]
    st = f.stats(f.x)
    for form, (out, su, me, inv) in st.items():
        assert torch.equal(out, plain), f"{what} {form}: convolution differs from lidog_sconv_reduce_rows"
        _sums_bar(su, out, n, f"{what} {form}")
        assert torch.allclose(me, out.double().mean(0).float(), rtol=1e-5, atol=1e-6), f"{what} {form}: mean"
        assert bool(torch.isfinite(inv).all()), f"{what} {form}: invstd"
    # evaluation-mode BatchNorm epilogue
    mean, invstd, w, b = (v.double() for v in f.bn_out)
    c64, cb = R.conv64(f.x, f.W, f.b, f.nbr), R.bound(f.x, f.W, f.b, f.nbr)
    scale = (invstd * w).abs()
    worst = 0.0
    for residual, relu in ((f.res, 1), (None, 1), (f.res, 0), (None, 0)):
        y = _all_equal(f.eval_bn(f.x, residual, relu), f"{what} eval BatchNorm residual {residual is not None} relu {relu}")
        y64 = ((c64 - mean) * invstd) * w + b
        mag = (c64.abs() + mean.abs()) * scale + b.abs()
        if residual is not None:
            y64, mag = y64 + residual.double(), mag + residual.double().abs()
        if relu:
            y64 = y64.clamp(min=0)
        worst = max(worst, _inside(y, y64, cb * scale * (1 + 6 * R.U) + 6 * R.U * mag, f"{what} eval BatchNorm"))
    record_property("worst_error_over_bound_eval_bn", worst)
    # the BatchNorm of the layer before applied in the staging
    if f.mfma:
        for relu in (1, 0):
            for form, (folded, two_step) in f.in_bn(f.pre, relu).items():
                assert torch.equal(folded, two_step), f"{what} {form} relu {relu}: differs from bn_apply_bits + plain"
    # BatchNorm-backward sums in the data gradient's epilogue
    T = f.product(f.gy, f.m.pair_out, f.Wt, Cout, Cin)
    for relu in (True, False):
        one, two = f.bwdstats(T, relu), f.bwd_two_pass(T, relu)
        for key in one:
            assert torch.equal(one[key], two[key]), f"{what} bwdstats relu {relu}: {key}"
        assert bool(torch.isfinite(one["sums"]).all()) and one["sums"][-1].item() == n


# ------------------------------------------------------------------ e. poisoned rows
def _poisoned(t, rows, value):
    t = t.clone()
    t[torch.as_tensor(sorted(rows), device=t.device)] = value
    return t


def _rows_hit(got, clean, hit, what):
    """rows in `hit` are non-finite in every element, every other row carries the bits of the clean run"""
    hit = torch.as_tensor(np.asarray(hit), device=got.device)
    assert bool((~torch.isfinite(got[hit])).all()), f"{what}: a row that meets a poisoned row came out finite"
    assert torch.equal(got[~hit], clean[~hit]), f"{what}: a row that meets no poisoned row changed"


@pytest.mark.parametrize("value", [NAN, float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("name,Cin,Cout", POISON, ids=[f"{s}-{a}x{b}" for s, a, b in POISON])
def test_poisoned_rows_reach_exactly_their_neighbours(name, Cin, Cout, value):
    """R = {row 0, a middle row, the last row} of x (forward), gy (data gradient), and row 0 of the product rows T (the
    two reductions) set to NaN / +Inf: only values change, every index stays in range.  The evaluation-mode BatchNorm and
    the _in_bn forms run without ReLU here (max(NaN, 0) may legitimately be 0); with ReLU they are covered on clean
    inputs above."""
    f = Forms(name, Cin, Cout)
    n, m, what = f.n, f.m, f"{name} {Cin}->{Cout} {value}"
    rows = {0, n // 2, n - 1}
    hit_out, hit_in = R.touched(f.nbr, rows), R.touched(f.nbr_t, rows)
    k_off, pin, pout = R.pairs(f.nbr)
    xp, gp = _poisoned(f.x, rows, value), _poisoned(f.gy, rows, value)
    # product rows
    for A, Ap, gather, B, ci, co, src in ((f.x, xp, m.pair_in, f.W, Cin, Cout, pin), (f.gy, gp, m.pair_out, f.Wt, Cout, Cin, pout)):
        clean, bad = f.products(A, gather, B, ci, co), f.products(Ap, gather, B, ci, co)
        for form in clean:
            _rows_hit(bad[form], clean[form], np.isin(src, list(rows)), f"{what} product rows {form}")
    # forward and data gradient, every form
    clean, bad = f.forward(f.x), f.forward(xp)
    for form in clean:
        _rows_hit(bad[form], clean[form], hit_out, f"{what} forward {form}")
    clean, bad = f.dgrad(f.gy), f.dgrad(gp)
    for form in clean:
        _rows_hit(bad[form], clean[form], hit_in, f"{what} data gradient {form}")
    if Cin % 4 == 0:
        T = f.product(gp, m.pair_out, f.Wt, Cout, Cin)
        one = f.bwdstats(T, False)
        assert not bool(torch.isfinite(one["sums"][:-1]).any()) and one["sums"][-1].item() == n, f"{what} bwdstats sums"
        assert not bool(torch.isfinite(one["dw"]).any()) and not bool(torch.isfinite(one["db"]).any()), f"{what} bwdstats dw / db"
    # statistics and evaluation-mode BatchNorm epilogues
    if Cout % 4 == 0:
        clean, bad = f.stats(f.x), f.stats(xp)
        for form in clean:
            assert bool(torch.isfinite(clean[form][1]).all()), f"{what} {form}: a padded row reached the clean sums"
            _rows_hit(bad[form][0], clean[form][0], hit_out, f"{what} {form}")
            assert not bool(torch.isfinite(bad[form][1][:-1]).any()) and bad[form][1][-1].item() == n, f"{what} {form} sums"
        for residual in (f.res, None):
            clean, bad = f.eval_bn(f.x, residual, 0), f.eval_bn(xp, residual, 0)
            for form in clean:
                _rows_hit(bad[form], clean[form], hit_out, f"{what} {form}")
    if f.mfma:
        clean, bad = f.in_bn(f.pre, 0), f.in_bn(_poisoned(f.pre, rows, value), 0)
        _rows_hit(bad["gemm_in_bn"][0], clean["gemm_in_bn"][0], np.isin(pin, list(rows)), f"{what} gemm_in_bn")
        _rows_hit(bad["os_stats_in_bn"][0], clean["os_stats_in_bn"][0], hit_out, f"{what} os_stats_in_bn")
        assert not bool(torch.isfinite(bad["os_stats_in_bn sums"][0][:-1]).any()), f"{what} os_stats_in_bn sums"
        hit_k = np.array([np.isin(pin[k_off[k]:k_off[k + 1]], list(rows)).any() for k in range(27)])
        _rows_hit(bad["wgrad_in_bn"][0], clean["wgrad_in_bn"][0], hit_k, f"{what} wgrad_in_bn")
    # row 0 of the product rows, for the reductions alone: pair 0 belongs to one output row
    for side, C, bias, ad, pair_rows in (("out", Cout, f.b, None, pout), ("in", Cin, None, f.addend(), pin)):
        gather, B = (m.pair_in, f.W) if side == "out" else (m.pair_out, f.Wt)
        T = f.product(f.x if side == "out" else f.gy, gather, B, *((Cin, Cout) if side == "out" else (Cout, Cin)))
        Tp = _poisoned(T, {0}, value)
        hit = np.zeros(n, bool)
        hit[pair_rows[0]] = True
        _rows_hit(f.reduce_pos(Tp, side, C, bias, ad), f.reduce_pos(T, side, C, bias, ad), hit, f"{what} reduce {side}, T row 0")
        if C % 4 == 0:
            _rows_hit(f.reduce_rows(Tp, side, C, bias, ad), f.reduce_rows(T, side, C, bias, ad), hit,
                      f"{what} reduce_rows {side}, T row 0")
        if side == "out" and C % 4 == 0:
            clean, bad = f.stats(T=T), f.stats(T=Tp)
            for form in clean:
                _rows_hit(bad[form][0], clean[form][0], hit, f"{what} {form}, T row 0")
                assert not bool(torch.isfinite(bad[form][1][:-1]).any()), f"{what} {form} sums, T row 0"
            clean, bad = f.eval_bn(None, f.res, 0, T=T), f.eval_bn(None, f.res, 0, T=Tp)
            _rows_hit(bad["reduce_rows_bn"], clean["reduce_rows_bn"], hit, f"{what} reduce_rows_bn, T row 0")
        if side == "in" and C % 4 == 0:
            _rows_hit(f.bwdstats(Tp, False)["out"], f.bwdstats(T, False)["out"], hit, f"{what} bwdstats, T row 0")
    # weight gradient, both cores: an offset whose pairs avoid R keeps its bits
    for core in (1, 0):
        clean = f.wgrad(f.x, f.gy, core)
        assert bool(torch.isfinite(clean).all()), f"{what} core {core}: weight gradient not written"
        if name == "isolated":
            assert bool((clean[torch.arange(27) != 13] == 0).all()), f"{what} core {core}: an empty offset is not exactly 0"
        for A, G, src in ((xp, f.gy, pin), (f.x, gp, pout)):
            bad = f.wgrad(A, G, core)
            hit = np.array([np.isin(src[k_off[k]:k_off[k + 1]], list(rows)).any() for k in range(27)])
            _rows_hit(bad, clean, hit, f"{what} core {core} weight gradient")
            if name == "isolated":
                assert bool((bad[torch.arange(27) != 13] == 0).all()), f"{what} core {core}: poisoned, k != 13 must stay 0"


def _stem_forms(m, x, W, b, C):
    """{form: out} of the 1 -> C convolution over the 5^3 map: lidog_sconv_cin1 and the two-pass path, NaN-prefilled"""
    import lidog_amd.me as ME
    from lidog_amd._lib import call, ptr
    n = m.n_out
    forms = {"cin1": _nan(n, C), "gemm + reduce": _nan(n, C), "gemm + reduce_rows": _nan(n, C)}
    call("lidog_sconv_cin1", ptr(x), ptr(m.nbr), ptr(W), ptr(b), n, 125, C, ptr(forms["cin1"]))
    T = _nan(m.P, C)
    ME._gemm(x, m.pair_in, W, None, m, 1, C, T, None)
    call("lidog_sconv_reduce", ptr(T), ptr(m.pos_out), n, 125, C, ptr(b), None, ptr(forms["gemm + reduce"]))
    rp, rl = m.rows("out")
    call("lidog_sconv_reduce_rows", ptr(T), ptr(rp), ptr(rl), n, C, ptr(b), None, ptr(forms["gemm + reduce_rows"]))
    return forms


def _scatter_forms(m, A, B, bias, Cin, Cout):
    """{core: out [n_fine, Cout]} of the gathered GEMM over the exchanged k2 s2 map scattered straight into a NaN-filled
    result (gather pair_out, scatter pair_in): the transposed forward, and with the transposed kernels the strided
    convolution's data gradient"""
    import lidog_amd.me as ME
    from lidog_amd import _lib
    L = _lib.load()
    out = {}
    for core in (1, 0):
        assert L.lidog_set_sparse_core(core) == 0
        out[core] = _nan(m.n_in, Cout)
        ME._gemm(A, m.pair_out, B, bias, m, Cin, Cout, out[core], m.pair_in)
    L.lidog_set_sparse_core(1)
    return out


def _addend_in_place(mm, gather, x, W, ad, Cin, Cout):
    """lidog_sconv_gemm_addend with addend == T on a copy of `ad`"""
    from lidog_amd._lib import call, ptr
    T = ad.clone()
    call("lidog_sconv_gemm_addend", ptr(x), ptr(gather), ptr(W), ptr(mm.tiles[0]), ptr(mm.tiles[1]), ptr(mm.tiles[2]),
         mm.n_tiles, Cin, Cout, ptr(T), ptr(T), None)
    return T


@pytest.mark.parametrize("value", [NAN, float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("name", POISON_SCENES)
def test_poisoned_rows_on_the_stem_the_scatters_and_the_addend_form(name, value):
    """the remaining paths of c under the same poison.  lidog_sconv_cin1 loads x[idx < 0 ? 0 : idx] and skips the
    missing neighbours afterwards: with x[0] non-finite a mask by multiplication shows on every row that misses a
    neighbour.  The k2 s2 scatters and lidog_sconv_gemm_addend (both gather modes) must carry a poisoned input row to
    exactly the rows that read it."""
    import lidog_amd.me as ME
    # the stem on the 5^3 map
    m5, nbr5 = _map(name, "k5s1"), R.scene_map(name, "k5s1")[2]
    n = m5.n_out
    rows = {0, n // 2, n - 1}
    hit = R.touched(nbr5, rows)
    for C in (16, 32, 64):
        x, W, b, _, _ = _operands(n, n, 125, 1, C, C + 1)
        clean, bad = _stem_forms(m5, x, W, b, C), _stem_forms(m5, _poisoned(x, rows, value), W, b, C)
        for form in clean:
            assert bool(torch.isfinite(clean[form]).all())
            _rows_hit(bad[form], clean[form], hit, f"{name} stem 1->{C} {form} {value}")
    # the direct scatters of the k2 s2 map, both ways
    m2, nbr_t = _map(name, "k2s2"), R.scene_map(name, "tr_k2s2")[2]
    n_c = m2.n_out
    rows_c = {0, n_c // 2, n_c - 1}
    hit = R.touched(nbr_t, rows_c)
    for Cin, Cout in ((32, 32), (128, 96), (20, 12), (5, 7)):
        x_c, W, b, gy_c, _ = _operands(n_c, n_c, 8, Cin, Cout, Cin + 5 * Cout)
        Wt = W.transpose(1, 2).contiguous()
        for A, B, bias, ci, co, tag in ((x_c, W, b, Cin, Cout, "transposed forward"), (gy_c, Wt, None, Cout, Cin, "k2 s2 dgrad")):
            clean, bad = _scatter_forms(m2, A, B, bias, ci, co), _scatter_forms(m2, _poisoned(A, rows_c, value), B, bias, ci, co)
            for core in clean:
                assert bool(torch.isfinite(clean[core]).all())
                _rows_hit(bad[core], clean[core], hit, f"{name} {ci}->{co} {tag} core {core} {value}")
    # the addend form in place, with and without a gather index
    m3 = _map(name, "k3s1")
    n, Cin, Cout = m3.n_out, 7, 96
    rows = {0, n // 2, n - 1}
    x, W, _, _, _ = _operands(n, n, 27, Cin, Cout, 5)
    pin = m3.pair_in.cpu().numpy()
    for gather, mm, hit in ((m3.pair_in, m3, np.isin(pin, list(rows))),
                            (None, ME._IdentityMap(n, "cuda"), np.isin(np.arange(n), list(rows)))):
        ad = torch.randn(hit.shape[0], Cout, generator=torch.Generator().manual_seed(3)).cuda()
        clean = _addend_in_place(mm, gather, x, W, ad, Cin, Cout)
        assert bool(torch.isfinite(clean).all())
        _rows_hit(_addend_in_place(mm, gather, _poisoned(x, rows, value), W, ad, Cin, Cout), clean, hit,
                  f"{name} gemm_addend gather {gather is not None} {value}")
