"""The BEV head's convolution kernels through the C ABI against the float64 yardstick (tests/bev_ref.py), under the
exact bar (integer operands: the fp32 result must equal the float64 one), the precision bar (random operands: the
elementwise fp32 summation bound and a Frobenius bar that rejects operands rounded to tf32) and the written bar (every
output pre-filled with NaN):
  - dense k3 s2 p1 forward / data gradient / weight gradient (csrc/conv2d.hip): 96- and 128-row tiles with partial
    last tiles, empty stride-2 parity classes (H or W of 1), k_chunk tails, weight gradients with one split (gw written
    directly), several splits and a split count capped by the workspace;
  - the 1x1 classifier kernels k_pw_* with the workspace lidog_amd.bev computes;
  - the support-restricted kernels (csrc/conv2d_sparse.hip) for Cin 1 .. 128, cells on the row-bitmask word edges and
    the padding border, empty images and channels, full density, B = 0;
  - the argument checks, which must refuse before any launch and leave the output untouched."""
import re

import pytest
import torch

import bev_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _fill(shape, value, dtype=torch.float32):
    """every output and workspace of the kernel tests; value None: uninitialised (torch.empty)"""
    if value is None:
        return torch.empty(shape, dtype=dtype, device="cuda")
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _dev(t):
    """every float operand of the kernel tests"""
    return t.cuda()


def _gen(*key):
    s = 0
    for k in key:
        s = s * 1009 + int(k)
    return torch.Generator().manual_seed(s)


def _operands(kind, g, shape, role):
    """exact: small integers (inputs zero-heavy like ReLU output); precise: random fp32"""
    if kind == "exact":
        if role == "x":
            return R.exact_operands(shape, g, 0, 3, 0.6)
        return R.exact_operands(shape, g, -2, 2, 0.3 if role == "gy" else 0.0)
    return torch.randn(shape, generator=g) * (0.1 if role == "w" else 1.0)


def _check(kind, got, ref, abs_terms, K, what, record, mask=None):
    if mask is not None:
        got, ref, abs_terms = got[mask], ref[mask], abs_terms[mask]
    if kind == "exact":
        R.assert_exact(got, ref, abs_terms, what)
    else:
        r_elem, r_fro = R.assert_precision(got, ref, abs_terms, K, what)
        record(f"{what}_elem", round(r_elem, 5))
        record(f"{what}_fro", round(r_fro, 5))


def _call(*a):
    from lidog_amd._lib import call
    call(*a)


def _p(t):
    from lidog_amd._lib import ptr
    return ptr(t)


# ------------------------------------------------------------------ dense k3 s2 p1
# (B, Cin, H, W, Cout, wgrad workspace in slabs or None = what lidog_amd.bev passes)
#  weight-gradient splits (1024 / tiles, <= ceil(B Ho Wo / 128), <= workspace / slab):
#  (1,1) (1,9) (2,2) (3,5) (17,9) -> 1 split, gw written directly; B Ho Wo < 32: one partial stage
#  (64,65) Cin 256 -> 25 splits; (67,131) -> 18 / 43 splits; (64,65) Cin 128 Cout 40 -> 9 splits
#  ws 3 slabs -> capped to 3 splits; ws 1 slab -> capped to 1 split over 3 168 pixels
K3_CASES = [
    (1, 32, 1, 1, 32, None),      # every class but (0, 0) empty
    (3, 96, 1, 9, 96, None),      # 96-row data-gradient tiles, partial forward row tile; py = 1 classes empty
    (1, 128, 2, 2, 128, None),
    (3, 192, 3, 5, 256, None),    # 96-row tiles, two row tiles
    (1, 320, 17, 9, 96, None),    # 128-row tiles, partial third one
    (3, 256, 64, 65, 32, None),
    (3, 256, 64, 65, 32, 3),
    (1, 256, 64, 65, 32, 1),
    (1, 96, 67, 131, 256, None),
    (3, 320, 67, 131, 128, None),
    (2, 32, 17, 9, 8, None),      # Cout 8 / 40: forward and weight gradient only (the data gradient needs Cout % 32)
    (1, 128, 64, 65, 40, None),
]


@pytest.mark.parametrize("kind", ["exact", "precise"])
@pytest.mark.parametrize("B,Cin,H,W,Cout,ws_slabs", K3_CASES)
def test_conv2d_k3s2_kernels_vs_float64(B, Cin, H, W, Cout, ws_slabs, kind, record_property):
    g = _gen(B, Cin, H, W, Cout, ws_slabs or 0, kind == "exact")
    x = _dev(_operands(kind, g, (B, Cin, H, W), "x"))
    w = _dev(_operands(kind, g, (Cout, Cin, 3, 3), "w"))
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = _dev(_operands(kind, g, (B, Cout, Ho, Wo), "gy"))
    x64, w64, gy64 = x.double(), w.double(), gy.double()

    y = _fill((B, Cout, Ho, Wo), NAN)
    _call("lidog_conv2d_fwd", _p(x), _p(w), None, B, Cin, H, W, Cout, 3, 2, 1, _p(y))
    a, K = R.conv3s2_abs_terms(x64, w64, gy64, "fwd")
    _check(kind, y, R.conv3s2_fwd64(x64, w64), a, K, "fwd", record_property)

    if Cout % 32 == 0:
        gx = _fill(x.shape, NAN)
        ws = _fill((9 * Cin * Cout,), None)
        _call("lidog_conv2d_dgrad", _p(gy), _p(w), B, Cin, H, W, Cout, 3, 2, 1, _p(gx), _p(ws))
        a, K = R.conv3s2_abs_terms(x64, w64, gy64, "dgrad")
        _check(kind, gx, R.conv3s2_dgrad64(gy64, w64, H, W), a, K, "dgrad", record_property)

    gw = _fill(w.shape, NAN)
    n_ws = 32 * w.numel() if ws_slabs is None else ws_slabs * w.numel()
    ws = _fill((n_ws,), NAN)
    _call("lidog_conv2d_wgrad", _p(x), _p(gy), B, Cin, H, W, Cout, 3, 2, 1, _p(gw), None, _p(ws), n_ws)
    a, K = R.conv3s2_abs_terms(x64, w64, gy64, "wgrad")
    _check(kind, gw, R.conv3s2_wgrad64(x64, gy64), a, K, "wgrad", record_property)


# ------------------------------------------------------------------ 1x1 classifier
PW_CASES = [
    (1, 1, 1, 1, 1, True),
    (2, 3, 1, 3, 2, False),
    (4, 256, 15, 17, 7, True),      # 255 pixels
    (1, 256, 1, 257, 8, False),
    (2, 256, 33, 33, 7, True),      # 1 089: the G3 image
    (4, 3, 100, 100, 8, True),      # bound 30
    (2, 256, 167, 167, 7, True),    # bound 50
    (1, 1, 167, 167, 2, False),
]


@pytest.mark.parametrize("kind", ["exact", "precise"])
@pytest.mark.parametrize("B,Cin,H,W,Cout,bias", PW_CASES)
def test_conv2d_1x1_kernels_vs_float64(B, Cin, H, W, Cout, bias, kind, record_property):
    g = _gen(B, Cin, H, W, Cout, bias, kind == "exact")
    x = _dev(_operands(kind, g, (B, Cin, H, W), "x"))
    w = _dev(_operands(kind, g, (Cout, Cin, 1, 1), "w"))
    b = _dev(_operands(kind, g, (Cout,), "b")) if bias else None
    gy = _dev(_operands(kind, g, (B, Cout, H, W), "gy"))
    x64, w64, gy64 = x.double(), w.double(), gy.double()
    b64 = b.double() if bias else None

    y = _fill((B, Cout, H, W), NAN)
    _call("lidog_conv2d_fwd", _p(x), _p(w), _p(b), B, Cin, H, W, Cout, 1, 1, 0, _p(y))
    a = R.pw_fwd64(x64.abs(), w64.abs(), None if b64 is None else b64.abs())
    _check(kind, y, R.pw_fwd64(x64, w64, b64), a, Cin + (1 if bias else 0), "fwd", record_property)

    gx = _fill(x.shape, NAN)
    _call("lidog_conv2d_dgrad", _p(gy), _p(w), B, Cin, H, W, Cout, 1, 1, 0, _p(gx), None)
    _check(kind, gx, R.pw_dgrad64(gy64, w64), R.pw_dgrad64(gy64.abs(), w64.abs()), Cout, "dgrad", record_property)

    gw = _fill(w.shape, NAN)
    gb = _fill((Cout,), NAN) if bias else None
    n_ws = 4 * B * (w.numel() + Cout)                      # lidog_amd.bev._Conv2dFn
    ws = _fill((n_ws,), NAN)
    _call("lidog_conv2d_wgrad", _p(x), _p(gy), B, Cin, H, W, Cout, 1, 1, 0, _p(gw), _p(gb), _p(ws), n_ws)
    rw, rb = R.pw_wgrad64(x64, gy64)
    aw, ab = R.pw_wgrad64(x64.abs(), gy64.abs())
    _check(kind, gw, rw, aw, B * H * W, "wgrad", record_property)
    if bias:
        _check(kind, gb, rb, ab, B * H * W, "gbias", record_property)


# ------------------------------------------------------------------ refusals
def _refusals():
    """(name, entry, argument builder, message fragment); every one returns on the host before any launch"""
    B, Cin, H, W, Cout = 1, 32, 8, 8, 32

    def t(*shape):
        return torch.zeros(shape, device="cuda")

    x, w3, w1, b = t(B, Cin, H, W), t(Cout, Cin, 3, 3), t(8, Cin, 1, 1), t(Cout)
    y3, gy3 = t(B, Cout, 4, 4), t(B, Cout, 4, 4)
    ws = t(9 * 128 * 256)
    out = lambda *s: torch.full(s, 7.0, device="cuda")   # noqa: E731
    sup = torch.zeros((B, 129, H, W), dtype=torch.int32, device="cuda")
    act = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    return [
        ("k3 with bias", "lidog_conv2d_fwd", lambda o: (x, w3, b, B, Cin, H, W, Cout, 3, 2, 1, o), out(B, Cout, 4, 4),
         "without bias"),
        ("k5", "lidog_conv2d_fwd", lambda o: (x, t(Cout, Cin, 5, 5), None, B, Cin, H, W, Cout, 5, 2, 2, o),
         out(B, Cout, 4, 4), "k3 s2 p1"),
        ("k3 stride 1", "lidog_conv2d_fwd", lambda o: (x, w3, None, B, Cin, H, W, Cout, 3, 1, 1, o), out(B, Cout, 8, 8),
         "k3 s2 p1"),
        ("k3 stride 1 dgrad", "lidog_conv2d_dgrad", lambda o: (gy3, w3, B, Cin, H, W, Cout, 3, 1, 1, o, ws),
         out(B, Cin, H, W), "k3 s2 p1"),
        ("k5 wgrad", "lidog_conv2d_wgrad", lambda o: (x, gy3, B, Cin, H, W, Cout, 5, 2, 2, o, None, ws, ws.numel()),
         out(Cout, Cin, 5, 5), "k3 s2 p1"),
        ("1x1 Cout 9", "lidog_conv2d_fwd", lambda o: (x, t(9, Cin, 1, 1), None, B, Cin, H, W, 9, 1, 1, 0, o),
         out(B, 9, H, W), "Cout <= 8"),
        ("1x1 Cout 9 dgrad", "lidog_conv2d_dgrad", lambda o: (t(B, 9, H, W), t(9, Cin, 1, 1), B, Cin, H, W, 9, 1, 1, 0,
                                                               o, None), out(B, Cin, H, W), "Cout <= 8"),
        ("1x1 Cout 9 wgrad", "lidog_conv2d_wgrad", lambda o: (x, t(B, 9, H, W), B, Cin, H, W, 9, 1, 1, 0, o, None, ws,
                                                               ws.numel()), out(9, Cin, 1, 1), "Cout <= 8"),
        ("1x1 stride 2", "lidog_conv2d_fwd", lambda o: (x, w1, None, B, Cin, H, W, 8, 1, 2, 0, o), out(B, 8, 4, 4),
         "stride 1"),
        ("fwd Cin 20", "lidog_conv2d_fwd", lambda o: (t(B, 20, H, W), t(Cout, 20, 3, 3), None, B, 20, H, W, Cout, 3, 2, 1,
                                                       o), out(B, Cout, 4, 4), "Cin*9 must be a multiple of 32"),
        ("dgrad Cout 40", "lidog_conv2d_dgrad", lambda o: (t(B, 40, 4, 4), t(40, Cin, 3, 3), B, Cin, H, W, 40, 3, 2, 1, o,
                                                           ws), out(B, Cin, H, W), "Cout must be a multiple of 32"),
        ("wgrad Cout 12", "lidog_conv2d_wgrad", lambda o: (x, t(B, 12, 4, 4), B, Cin, H, W, 12, 3, 2, 1, o, None, ws,
                                                           ws.numel()), out(12, Cin, 3, 3), "multiple of 8"),
        ("wgrad workspace", "lidog_conv2d_wgrad", lambda o: (x, gy3, B, Cin, H, W, Cout, 3, 2, 1, o, None, ws,
                                                             9 * Cin * Cout - 1), out(Cout, Cin, 3, 3), "workspace too small"),
        ("1x1 wgrad workspace", "lidog_conv2d_wgrad", lambda o: (x, t(B, 8, H, W), B, Cin, H, W, 8, 1, 1, 0, o, None, ws,
                                                                 4 * B * (8 * Cin + 8) - 1), out(8, Cin, 1, 1),
         "needs a workspace"),
        ("support Cin 129", "lidog_conv2d_support", lambda o: (sup, B, 129, H, W, o), torch.full((1 << 16,), 7,
                                                                                                dtype=torch.int32,
                                                                                                device="cuda"),
         "Cin <= 128"),
        ("fwd_sparse Cin 129", "lidog_conv2d_fwd_sparse", lambda o: (t(B, 129, H, W), t(128, 129, 3, 3), act, B, 129, H,
                                                                     W, 128, o, ws), out(B, 128, 4, 4), "Cin <= 128"),
        ("fwd_sparse Cout 96", "lidog_conv2d_fwd_sparse", lambda o: (x, t(96, Cin, 3, 3), act, B, Cin, H, W, 96, o, ws),
         out(B, 96, 4, 4), "Cout a multiple of 128"),
        ("dgrad_sparse Cin 129", "lidog_conv2d_dgrad_sparse", lambda o: (gy3, t(Cout, 129, 3, 3), act, B, 129, H, W, Cout,
                                                                         o, ws), out(B, 129, H, W), "Cin <= 128"),
        ("wgrad_sparse Cin 129", "lidog_conv2d_wgrad_sparse", lambda o: (t(B, 129, H, W), gy3, act, B, 129, H, W, Cout,
                                                                         o, ws, ws.numel()), out(Cout, 129, 3, 3),
         "Cin <= 128"),
        ("wgrad_sparse workspace", "lidog_conv2d_wgrad_sparse", lambda o: (x, gy3, act, B, Cin, H, W, Cout, o, ws, 10),
         out(Cout, Cin, 3, 3), "workspace too small"),
    ]


def test_conv2d_entry_points_refuse_unsupported_arguments():
    """each refusal raises RuntimeError with its message and leaves the output buffer untouched"""
    for name, entry, args, o, msg in _refusals():
        before = o.clone()
        with pytest.raises(RuntimeError, match=re.escape(msg)):
            _call(entry, *[_p(a) if isinstance(a, torch.Tensor) else a for a in args(o)])
        torch.cuda.synchronize()
        assert torch.equal(o, before), name


# ------------------------------------------------------------------ support-restricted kernels
def _support(B, C, H, W, pattern, g):
    """bool [B, C, H, W]: "edges" = the four corners and the cells at x in {62, 63, 64, 65, W - 1} (row-bitmask word
    edges) on the first, middle and last rows (padding border) plus a few short runs, with every third channel empty and
    image 1 empty; "runs" = horizontal runs of a LiDAR-like density, every fourth channel and image 1 empty;
    "full" = everything"""
    if pattern == "full":
        return torch.ones((B, C, H, W), dtype=torch.bool)
    seeds = torch.rand((B, C, H, W), generator=g) < (0.01 if pattern == "runs" else 0.003)
    sup = seeds.clone()
    for s in range(1, 6):
        sup[..., s:] |= seeds[..., :-s]
    if pattern == "edges":
        xs = sorted({0, W - 1} | {x for x in (62, 63, 64, 65) if x < W})
        for y in sorted({0, H // 2, H - 1}):
            for x in xs:
                sup[:, :, y, x] = True
        sup[:, 2::3] = False
    else:
        sup[:, 3::4] = False
    if B > 1:
        sup[1] = False
    return sup


SPARSE_CASES = [
    (3, 1, 5, 64, 128, "edges"),
    (2, 8, 9, 65, 256, "edges"),
    (3, 33, 7, 128, 128, "edges"),
    (1, 96, 12, 131, 256, "runs"),
    (2, 100, 6, 131, 128, "edges"),
    (1, 128, 10, 64, 128, "full"),
    (2, 128, 33, 70, 256, "runs"),
]


@pytest.mark.parametrize("kind", ["exact", "precise"])
@pytest.mark.parametrize("B,Cin,H,W,Cout,pattern", SPARSE_CASES)
def test_conv2d_over_support_vs_float64(B, Cin, H, W, Cout, pattern, kind, record_property):
    """forward and weight gradient everywhere, data gradient wherever the support needs it (the kernel writes only
    there), against float64 -- not only against the dense kernels, which share the tile code"""
    from lidog_amd._lib import load
    g = _gen(B, Cin, H, W, Cout, kind == "exact")
    sup = _support(B, Cin, H, W, pattern, g)
    support = torch.where(sup, torch.randint(0, 1000, sup.shape, generator=g), torch.full(sup.shape, -1)).int().cuda()
    x = _dev(_operands(kind, g, (B, Cin, H, W), "x") * sup)
    w = _dev(_operands(kind, g, (Cout, Cin, 3, 3), "w"))
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = _dev(_operands(kind, g, (B, Cout, Ho, Wo), "gy"))
    x64, w64, gy64 = x.double(), w.double(), gy.double()
    L = load()
    act = _fill((L.lidog_conv2d_support_ws(B, Cin, H, W),), None, torch.int32)
    _call("lidog_conv2d_support", _p(support), B, Cin, H, W, _p(act))
    ws = _fill((9 * Cin * Cout,), None)

    y = _fill((B, Cout, Ho, Wo), NAN)
    _call("lidog_conv2d_fwd_sparse", _p(x), _p(w), _p(act), B, Cin, H, W, Cout, _p(y), _p(ws))
    a, K = R.conv3s2_abs_terms(x64, w64, gy64, "fwd")
    _check(kind, y, R.conv3s2_fwd64(x64, w64), a, K, "fwd", record_property)

    gx = _fill(x.shape, NAN)
    _call("lidog_conv2d_dgrad_sparse", _p(gy), _p(w), _p(act), B, Cin, H, W, Cout, _p(gx), _p(ws))
    a, K = R.conv3s2_abs_terms(x64, w64, gy64, "dgrad")
    need = sup.cuda()
    _check(kind, gx, R.conv3s2_dgrad64(gy64, w64, H, W), a, K, "dgrad", record_property, mask=need)

    n_ws = L.lidog_conv2d_wgrad_sparse_ws(B, Cin, H, W, Cout)
    gw = _fill(w.shape, NAN)
    wsw = _fill((n_ws,), NAN)
    _call("lidog_conv2d_wgrad_sparse", _p(x), _p(gy), _p(act), B, Cin, H, W, Cout, _p(gw), _p(wsw), n_ws)
    a, K = R.conv3s2_abs_terms(x64, w64, gy64, "wgrad")
    _check(kind, gw, R.conv3s2_wgrad64(x64, gy64), a, K, "wgrad", record_property)


@pytest.mark.parametrize("Cin", [1, 96, 128])
def test_conv2d_over_support_of_an_empty_batch(Cin):
    """B = 0 on all three support-restricted entries: each returns 0; the weight gradient comes back as zeros (its
    Kd == 0 branch), the forward and data gradient have nothing to write"""
    from lidog_amd._lib import load
    H, W, Cout = 9, 70, 128
    L = load()
    act = _fill((max(1, L.lidog_conv2d_support_ws(0, Cin, H, W)),), 0, torch.int32)
    x = _dev(torch.zeros((0, Cin, H, W), device="cuda"))
    gy = _dev(torch.zeros((0, Cout, 5, 35), device="cuda"))
    w = _dev(torch.randn((Cout, Cin, 3, 3), device="cuda"))
    support = torch.zeros((0, Cin, H, W), dtype=torch.int32, device="cuda")
    ws = _fill((9 * Cin * Cout,), None)
    _call("lidog_conv2d_support", _p(support), 0, Cin, H, W, _p(act))
    _call("lidog_conv2d_fwd_sparse", _p(x), _p(w), _p(act), 0, Cin, H, W, Cout, None, _p(ws))
    _call("lidog_conv2d_dgrad_sparse", _p(gy), _p(w), _p(act), 0, Cin, H, W, Cout, None, _p(ws))
    gw = _fill(w.shape, NAN)
    n_ws = max(1, L.lidog_conv2d_wgrad_sparse_ws(0, Cin, H, W, Cout))
    wsw = _fill((n_ws,), None)
    _call("lidog_conv2d_wgrad_sparse", _p(x), _p(gy), _p(act), 0, Cin, H, W, Cout, _p(gw), _p(wsw), n_ws)
    torch.cuda.synchronize()
    assert torch.equal(gw, torch.zeros_like(gw))
