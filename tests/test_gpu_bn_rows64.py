"""BatchNorm over rows ([n, C], hw = 1: the 62 MinkowskiBatchNorms of the trunk; csrc/bn.hip k_colreduce_nc4 /
k_colreduce_strided, the in-kernel finish of stats_tail.h / k_bn_finalize, k_bn_apply{,4}, k_bn_apply4_sync,
k_bn_bwd_apply{,4}, k_bn_eval_invstd) through the C ABI against the float64 yardstick of tests/sparse_ref.py (bev_ref's
BatchNorm on [n, C, 1, 1]), and the statistics epilogues of the convolutions (lidog_sconv_reduce_rows_stats,
lidog_sconv_os_stats, lidog_sconv_reduce_rows_bwdstats) at bench size against the float64 values of their own rows.

Bars: the double sums within gamma_n = 1.01 n 2^-53 sum|terms| (a lost or doubled row fails it) and sums[2C] == n;
mean within 1 fp32 ulp of the float64 value plus what the sums carry in, invstd within 1 ulp plus the propagated
E[x^2] - E[x]^2 error (sparse_ref.stats_bounds); running statistics (unbiased n / (n - 1), momentum 0.1) within their
fp32 update bound; y, dx from the kernels' own fp32 mean / invstd within a few fp32 roundings per element; dres equal to
the masked dy; outputs pre-filled with NaN.  Data: N(0.5, 2), one channel of mean 1e3 and sigma 1, one constant channel
0.75 (var = 0: invstd = 1 / sqrt(eps), y = b exactly)."""
import numpy as np
import pytest
import torch

import sparse_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS, MOM = 1e-5, 0.1
U = R.U
RB96 = 256 // (96 // 4)          # rows per k_colreduce_nc4 workgroup at C = 96
_BENCH = {}


def _bench():
    """coordinate manager of one bench scan and the stride-1 row count of a bs-4 bench batch (cached per module)"""
    if not _BENCH:
        import lidog_amd.me as ME
        from lidog_amd import synth
        c = synth.make_batch((0,), "kitti120k", "cpu")["coords_int"]
        _BENCH["cm"] = ME.SparseTensor(coordinates=c.cuda(), features=torch.ones((c.shape[0], 1), device="cuda")
                                       ).coordinate_manager
        c4 = synth.make_batch((0, 1, 2, 3), "kitti120k", "cpu")["coords_int"]
        _BENCH["n4"] = int(torch.unique(c4, dim=0).shape[0])
    return _BENCH


CASES = (
    [(C, 5003) for C in (32, 64, 96, 128, 256)] +                  # every BatchNorm width of the network
    [(4, 5003), (12, 5003), (384, 5003), (1024, 5003)] +           # k_colreduce_nc4 row-block edges
    [(1, 5003), (7, 5003), (10, 5003)] +                           # k_colreduce_strided (C % 4 != 0)
    [(96, n) for n in (1, 2, RB96 - 1, RB96, RB96 + 1)] +          # around one row block
    [(96, 512 * RB96 * 4 + d) for d in (-1, 1)] +                  # either side of the forward grid cap
    [(96, 1024 * RB96 + d) for d in (-1, 1)] +                     # either side of the backward grid cap
    [(32, "bench4"), (96, "bench4")]                               # stride-1 rows of a bs-4 bench batch
)


def _fill(shape, value, dtype=torch.float32):
    """every output and workspace the tests own; value None: uninitialised (torch.empty)"""
    if value is None:
        return torch.empty(shape, dtype=dtype, device="cuda")
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _dev(t):
    """every float operand the tests own, and the running statistics the kernels update in place"""
    return t.cuda()


def _data(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, C), generator=g) * 2 + 0.5
    if C >= 2:
        x[:, 0] = torch.randn(n, generator=g) + 1e3      # E[x^2] - E[x]^2 with E[x^2] ~ 1e6 var
        x[:, 1] = 0.75                                   # var = 0
    p = dict(w=torch.rand(C, generator=g) + 0.5, b=torch.randn(C, generator=g),
             rm=torch.randn(C, generator=g), rv=torch.rand(C, generator=g) + 0.5,
             res=torch.randn((n, C), generator=g), dy=torch.randn((n, C), generator=g))
    return _dev(x), {k: _dev(v) for k, v in p.items()}


def _elem_bar(got, ref, scale, what, c=5.05):
    """|got - ref| <= c u scale elementwise (scale: sum of the magnitudes entering the fp32 expression).  Default: y =
    ((x - m) is) w + b (+ res), five roundings: <= 3u |core| + 2u (|core| + |b| + |res|) <= 5u scale, 1 % for the
    second-order terms"""
    err = (got.double() - ref).abs()
    bar = c * U * scale + 1e-38
    r = float((err / bar).max()) if err.numel() else 0.0
    if not bool(torch.isfinite(got).all()):
        r = float("nan")
    assert r <= 1.0, f"{what}: {r:.3g} x its fp32 bound (NaN: never written)"
    return r


def _check_fwd_stats(sums, mean, invstd, rm, rv, x, p, n, what, const_channel=True):
    """sums / mean / invstd / running statistics of x against float64; returns the worst ratios.  const_channel: x[:, 1]
    is the constant 0.75 of _data"""
    C = x.shape[1]
    x64 = x.double()
    s1, s2, cnt, s1_abs = R.bn_sums64(x64)
    assert float(sums[2 * C]) == n, f"{what}: sums[2C] = {float(sums[2 * C])}, want {n}"
    r = [R.assert_sums(sums[:C], s1, s1_abs, n, what + " sum x"), R.assert_sums(sums[C:2 * C], s2, s2, n, what + " sum x^2")]
    r += R.assert_stats(mean, invstd, s1, s2, s1_abs, n, EPS, what)
    m64, var64, _, d_mean, d_var, _ = R.stats_bounds(s1, s2, s1_abs, n, EPS)
    rm64, rv64 = R.running64(p["rm"].double(), p["rv"].double(), m64, var64, n, MOM)
    r += R.assert_running(rm, rv, rm64, rv64, p["rm"], p["rv"], MOM, d_mean, d_var * (n / (n - 1) if n > 1 else 1.0),
                          what)
    if const_channel and C >= 2:   # the constant channel: exact statistics
        assert float(mean[1]) == 0.75 and float(invstd[1]) == float(np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS))))), \
            f"{what}: constant channel mean / invstd"
    return max(r)


def _y_ref(x, mean, invstd, p, res, relu):
    """float64 y from the kernel's own fp32 mean / invstd, and the magnitude scale of its fp32 expression"""
    xc = x.double() - mean.double()
    core = xc * invstd.double() * p["w"].double()
    y = core + p["b"].double()
    scale = core.abs() + p["b"].double().abs()
    if res is not None:
        y = y + res.double()
        scale = scale + res.double().abs()
    return (torch.clamp_min(y, 0.0) if relu else y), scale


def _bits_match(bits, y, n, C, what):
    e = torch.arange(n * C, device="cuda")
    got = (bits.long()[e >> 5] >> (e & 31)) & 1
    assert torch.equal(got.bool(), (y.reshape(-1) > 0)), f"{what}: ReLU bit mask differs from y > 0"


def _bwd(x, dy, y_mask_src, mean, invstd, p, n, C, mode, training=True):
    """lidog_bn_bwd_reduce{,_bits} + lidog_bn_bwd_apply{,_bits} with the ReLU mask from `mode` in y / x / bits / none"""
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    L = _lib.load()
    y, bits = y_mask_src
    ws = _fill((max(L.lidog_bn_reduce_ws(C, 1), 1),), None, torch.float64)
    sums = _fill((2 * C + 1,), NAN, torch.float64)
    dw, db = _fill((C,), NAN), _fill((C,), NAN)
    ry = y if mode == "y" else None
    rw, rb = (p["w"], p["b"]) if mode == "x" else (None, None)
    rbits = bits if mode == "bits" else None
    call("lidog_bn_bwd_reduce_bits", ptr(dy), ptr(x), ptr(ry), ptr(rbits), n, C, 1, ptr(mean), ptr(invstd), ptr(sums),
         ptr(ws), float(n), ptr(dw), ptr(db), ptr(rw), ptr(rb))
    if not training:
        sums.zero_()
    dx, dres = _fill(x.shape, NAN), _fill(x.shape, NAN)
    call("lidog_bn_bwd_apply_bits", ptr(dy), ptr(x), ptr(ry), ptr(rbits), n, C, 1, ptr(mean), ptr(invstd), ptr(p["w"]),
         ptr(sums), float(n), ptr(dx), ptr(dres), None, None, ptr(rb))
    torch.cuda.synchronize()
    return sums, dw, db, dx, dres


def _check_bwd(got, x, dy, mask, mean, invstd, p, n, what, training=True):
    """backward sums / dw / db / dx / dres against float64 from the kernel's statistics and ReLU decisions"""
    sums, dw, db, dx, dres = got
    C = x.shape[1]
    g = dy if mask is None else torch.where(mask, dy, torch.zeros_like(dy))
    assert torch.equal(dres, g), f"{what}: dres is not the masked dy"
    xh32 = (x - mean) * invstd                    # the kernels' fp32 xhat (two correctly rounded operations)
    s_g, s_gx, a_g, a_gx = R.bn_bwd_sums64(dy.double(), xh32.double(), mask)
    r = []
    if training:
        assert float(sums[2 * C]) == n, f"{what}: backward sums[2C]"
        r += [R.assert_sums(sums[:C], s_g, a_g, n, what + " sum g"), R.assert_sums(sums[C:2 * C], s_gx, a_gx, n,
                                                                                  what + " sum g xhat")]
    for got_p, ref_p, ab, name in ((db, s_g, a_g, "db"), (dw, s_gx, a_gx, "dw")):
        err = (got_p.double() - ref_p).abs()
        ratio = float((err / (R.ulp32(ref_p) + R.sums_bar(n, ab) + 1e-38)).max())
        assert ratio <= 1.0, f"{what}: {name} {ratio:.3g} x (1 ulp + gamma_n) (NaN: never written)"
        r.append(ratio)
    # dx = (g - m0 - xhat m1) invstd w, m0 / m1 the fp32 casts of the mean backward sums
    k = (invstd.double() * p["w"].double())
    if training:
        m0, m1 = s_g / n, s_gx / n
        xh = (x.double() - mean.double()) * invstd.double()
        ref = (g.double() - m0 - xh * m1) * k
        scale = (g.double().abs() + m0.abs() + (xh * m1).abs()) * k.abs()
        r.append(_elem_bar(dx, ref, scale, what + " dx", c=8.0))
    else:
        r.append(_elem_bar(dx, g.double() * k, (g.double() * k).abs(), what + " eval dx", c=3.0))
    return max(r)


@pytest.mark.parametrize("C,n", CASES, ids=[f"C{c}_n{n}" for c, n in CASES])
def test_row_batchnorm_vs_float64(C, n, record_property):
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    L = _lib.load()
    if n == "bench4":
        n = _bench()["n4"]
    x, p = _data(n, C, C * 7919 + n)
    ws = _fill((max(L.lidog_bn_reduce_ws(C, 1), 1),), None, torch.float64)
    sums = _fill((2 * C + 1,), NAN, torch.float64)
    mean, invstd = _fill((C,), NAN), _fill((C,), NAN)
    rm, rv = _dev(p["rm"].clone()), _dev(p["rv"].clone())
    call("lidog_bn_stats", ptr(x), n, C, 1, ptr(sums), ptr(ws), float(n), EPS, MOM, ptr(mean), ptr(invstd), ptr(rm),
         ptr(rv))
    torch.cuda.synchronize()
    worst = {"stats": _check_fwd_stats(sums, mean, invstd, rm, rv, x, p, n, f"C{C} n{n}")}
    c4 = C % 4 == 0
    # forward with residual + ReLU (+ the bit mask where the layout has one), and without residual
    y = _fill(x.shape, NAN)
    bits = _fill((max(L.lidog_relu_bits_words(n, C), 1),), -1, torch.int32) if c4 else None
    call("lidog_bn_apply_bits", ptr(x), n, C, 1, ptr(mean), ptr(invstd), ptr(p["w"]), ptr(p["b"]), ptr(p["res"]), 1, ptr(y),
         ptr(bits))
    y_nr = _fill(x.shape, NAN)
    call("lidog_bn_apply", ptr(x), n, C, 1, ptr(mean), ptr(invstd), ptr(p["w"]), ptr(p["b"]), None, 1, ptr(y_nr))
    torch.cuda.synchronize()
    ref, scale = _y_ref(x, mean, invstd, p, p["res"], True)
    worst["y"] = _elem_bar(y, ref, scale, f"C{C} n{n} y (residual, ReLU)")
    ref, scale = _y_ref(x, mean, invstd, p, None, True)
    worst["y"] = max(worst["y"], _elem_bar(y_nr, ref, scale, f"C{C} n{n} y (ReLU)"))
    if C >= 2:
        assert torch.equal(y_nr[:, 1], torch.clamp_min(p["b"][1].expand(n), 0.0)), "constant channel: y != relu(b)"
        assert torch.equal(y[:, 1], torch.clamp_min(p["b"][1] + p["res"][:, 1], 0.0)), "constant channel: y != relu(b + res)"
    if c4:
        _bits_match(bits, y, n, C, f"C{C} n{n}")
    # backward for every ReLU-mask source the layout offers
    modes = [("y", y, y > 0), ("none", None, None)] + ([("bits", y, y > 0), ("x", y_nr, y_nr > 0)] if c4 else [])
    wb = 0.0
    for mode, _, mask in modes:
        got = _bwd(x, p["dy"], (y if mode != "x" else y_nr, bits), mean, invstd, p, n, C, mode)
        wb = max(wb, _check_bwd(got, x, p["dy"], mask, mean, invstd, p, n, f"C{C} n{n} bwd mask {mode}"))
    worst["bwd"] = wb
    # evaluation mode: running statistics as constants
    inv_e = _fill((C,), NAN)
    call("lidog_bn_eval_invstd", ptr(p["rv"]), EPS, C, ptr(inv_e))
    ye = _fill(x.shape, NAN)
    call("lidog_bn_apply", ptr(x), n, C, 1, ptr(p["rm"]), ptr(inv_e), ptr(p["w"]), ptr(p["b"]), None, 0, ptr(ye))
    torch.cuda.synchronize()
    inv64 = 1.0 / torch.sqrt(p["rv"].double() + float(np.float32(EPS)))
    assert bool(((inv_e.double() - inv64).abs() <= R.ulp32(inv64)).all()), "eval invstd not within 1 ulp"
    ref, scale = _y_ref(x, p["rm"], inv_e, p, None, False)
    worst["eval_y"] = _elem_bar(ye, ref, scale, f"C{C} n{n} eval y")
    got = _bwd(x, p["dy"], (ye, None), p["rm"], inv_e, p, n, C, "none", training=False)
    worst["eval_bwd"] = _check_bwd(got, x, p["dy"], None, p["rm"], inv_e, p, n, f"C{C} n{n} eval bwd", training=False)
    for k, v in worst.items():
        record_property(k, v)


@pytest.mark.parametrize("C", [96, 256])
def test_sync_apply_on_one_shard_vs_float64_of_the_whole_batch(C, record_property):
    """lidog_bn_apply_sync on the first half of the rows with the float64-added sums of both halves (the all-reduce),
    against the float64 BatchNorm of the whole batch; an empty shard (n = 0) still writes mean / invstd and moves the
    running statistics"""
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    L = _lib.load()
    n = 2 * 1024 * RB96 + 7
    x, p = _data(n, C, C + 17)
    h = n // 2 + 3
    parts = []
    for lo, hi in ((0, h), (h, n)):
        s = _fill((2 * C + 1,), NAN, torch.float64)
        ws = _fill((L.lidog_bn_reduce_ws(C, 1),), None, torch.float64)
        call("lidog_bn_stats", ptr(x[lo:hi]), hi - lo, C, 1, ptr(s), ptr(ws), float(hi - lo), 0.0, 0.0, None, None, None,
             None)
        parts.append(s)
    sums = parts[0] + parts[1]              # the all-reduce in double; sums[2C] = n
    for shard, rows in (("half", h), ("empty", 0)):
        mean, invstd = _fill((C,), NAN), _fill((C,), NAN)
        rm, rv = _dev(p["rm"].clone()), _dev(p["rv"].clone())
        y = _fill((max(rows, 1), C), NAN)
        bits = _fill((max(L.lidog_relu_bits_words(rows, C), 1),), -1, torch.int32)
        call("lidog_bn_apply_sync", ptr(x), rows, C, ptr(sums), EPS, MOM, ptr(mean), ptr(invstd), ptr(rm), ptr(rv),
             ptr(p["w"]), ptr(p["b"]), ptr(p["res"]), 1, ptr(y), ptr(bits))
        torch.cuda.synchronize()
        record_property(f"{shard}_stats", _check_fwd_stats(sums, mean, invstd, rm, rv, x, p, n, f"sync C{C} {shard}"))
        if rows:
            ref, scale = _y_ref(x[:rows], mean, invstd, p, p["res"][:rows], True)
            record_property(f"{shard}_y", _elem_bar(y, ref, scale, f"sync C{C} y"))
            _bits_match(bits, y, rows, C, f"sync C{C}")


@pytest.mark.parametrize("residual", [True, False], ids=["residual", "no_residual"])
@pytest.mark.parametrize("rows", [0, 1, 70])
@pytest.mark.parametrize("C", [8, 96])
def test_sync_apply_equals_finalize_then_apply_bit_for_bit(C, rows, residual):
    """lidog_bn_apply_sync against lidog_bn_finalize(count = -1) + lidog_bn_apply_bits from the same all-reduced sums
    vector (ReLU on): y, the bit words, mean, invstd and the running statistics with torch.equal.  70 rows leave a
    partial last bit word and a partial last workgroup; an empty shard compares the statistics only."""
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    L = _lib.load()
    n = 141                                  # rows of the whole batch behind the sums; this shard holds `rows` of them
    x, p = _data(n, C, 31 * C + rows)
    sums = _fill((2 * C + 1,), NAN, torch.float64)
    ws = _fill((L.lidog_bn_reduce_ws(C, 1),), None, torch.float64)
    call("lidog_bn_stats", ptr(x), n, C, 1, ptr(sums), ptr(ws), float(n), 0.0, 0.0, None, None, None, None)
    res = p["res"] if residual else None
    got = {}
    for form in ("sync", "two_pass"):
        o = dict(mean=_fill((C,), NAN), invstd=_fill((C,), NAN),
                 rm=_dev(p["rm"].clone()), rv=_dev(p["rv"].clone()), y=_fill((max(rows, 1), C), NAN),
                 bits=_fill((max(L.lidog_relu_bits_words(rows, C), 1),), -1, torch.int32))
        if form == "sync":
            call("lidog_bn_apply_sync", ptr(x), rows, C, ptr(sums), EPS, MOM, ptr(o["mean"]), ptr(o["invstd"]), ptr(o["rm"]),
                 ptr(o["rv"]), ptr(p["w"]), ptr(p["b"]), ptr(res), 1, ptr(o["y"]), ptr(o["bits"]))
        else:
            call("lidog_bn_finalize", ptr(sums), -1.0, C, EPS, MOM, ptr(o["mean"]), ptr(o["invstd"]), ptr(o["rm"]),
                 ptr(o["rv"]))
            call("lidog_bn_apply_bits", ptr(x), rows, C, 1, ptr(o["mean"]), ptr(o["invstd"]), ptr(p["w"]), ptr(p["b"]),
                 ptr(res), 1, ptr(o["y"]), ptr(o["bits"]))
        torch.cuda.synchronize()
        got[form] = o
    assert bool(torch.isfinite(got["sync"]["mean"]).all()) and bool(torch.isfinite(got["sync"]["invstd"]).all())
    for key in ("mean", "invstd", "rm", "rv") + (("y", "bits") if rows else ()):
        assert torch.equal(got["sync"][key], got["two_pass"][key]), f"C{C} rows {rows}: {key} differs from the two-pass form"
    if rows:
        assert bool(torch.isfinite(got["sync"]["y"]).all())
        _bits_match(got["sync"]["bits"], got["sync"]["y"], rows, C, f"sync C{C} rows {rows}")


def _bench_map():
    cm = _bench()["cm"]
    return cm.kernel_map(1, 1, 3)


@pytest.mark.parametrize("C", [32, 96])
def test_fused_statistics_epilogues_at_bench_size(C, record_property):
    """lidog_sconv_reduce_rows_stats, lidog_sconv_os_stats (sorted rows of the bench map) and
    lidog_sconv_reduce_rows_bwdstats: sums / mean / invstd / running statistics and dw / db against the float64 values
    of their own output rows"""
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    from test_gpu_sconv_os import _sorted
    L = _lib.load()
    m = _bench_map()
    n = m.n_out
    g = torch.Generator().manual_seed(C)
    _, p = _data(n, C, C + 5)
    bias = _dev(torch.randn(C, generator=g) + 3.0)
    # reduction of product rows with the statistics in its epilogue
    T = _dev(torch.randn((m.P, C), generator=g))
    rp, rl = m.rows("out")
    out = _fill((n, C), NAN)
    sums = _fill((2 * C + 1,), NAN, torch.float64)
    ws = _fill((L.lidog_sconv_reduce_stats_ws(n, C),), None, torch.float64)
    mean, invstd = _fill((C,), NAN), _fill((C,), NAN)
    rm, rv = _dev(p["rm"].clone()), _dev(p["rv"].clone())
    call("lidog_sconv_reduce_rows_stats", ptr(T), ptr(rp), ptr(rl), n, C, ptr(bias), ptr(out), ptr(sums), ptr(ws),
         float(n), EPS, MOM, ptr(mean), ptr(invstd), ptr(rm), ptr(rv))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    record_property("reduce_rows_stats", _check_fwd_stats(sums, mean, invstd, rm, rv, out, p, n, f"reduce_rows_stats C{C}",
                                                            const_channel=False))
    # output-stationary convolution with the statistics in its epilogue
    perm, wm, order = _sorted(m)
    Cin = 32
    x = _dev(torch.randn((n, Cin), generator=g))
    W = _dev(torch.randn((27, Cin, C), generator=g) * 0.2)
    out2 = _fill((n, C), NAN)
    sums2 = _fill((2 * C + 1,), NAN, torch.float64)
    ws2 = _fill((L.lidog_sconv_os_stats_ws(n, C),), None, torch.float64)
    mean2, invstd2 = _fill((C,), NAN), _fill((C,), NAN)
    rm2, rv2 = _dev(p["rm"].clone()), _dev(p["rv"].clone())
    call("lidog_sconv_os_stats", ptr(x), ptr(m.nbr), n, 27, ptr(perm), ptr(wm), ptr(order), ptr(W), ptr(bias), Cin, C,
         ptr(out2), ptr(sums2), ptr(ws2), float(n), EPS, MOM, ptr(mean2), ptr(invstd2), ptr(rm2), ptr(rv2))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out2).all())
    record_property("os_stats", _check_fwd_stats(sums2, mean2, invstd2, rm2, rv2, out2, p, n, f"os_stats C{C}",
                                                   const_channel=False))
    # data-gradient reduction with the BatchNorm backward sums in its epilogue (pre = the BatchNorm's input rows)
    rpi, rli = m.rows("in")
    Tg = _dev(torch.randn((m.P, C), generator=g))
    pre = out
    y = _fill(pre.shape, NAN)
    call("lidog_bn_apply", ptr(pre), n, C, 1, ptr(mean), ptr(invstd), ptr(p["w"]), ptr(p["b"]), None, 1, ptr(y))
    worst = 0.0
    for mode in ("y", "x", "none"):
        gout = _fill((n, C), NAN)
        s3 = _fill((2 * C + 1,), NAN, torch.float64)
        ws3 = _fill((L.lidog_bn_reduce_ws(C, 1),), None, torch.float64)
        dw, db = _fill((C,), NAN), _fill((C,), NAN)
        ry = y if mode == "y" else None
        rw, rb = (p["w"], p["b"]) if mode == "x" else (None, None)
        call("lidog_sconv_reduce_rows_bwdstats", ptr(Tg), ptr(rpi), ptr(rli), n, C, ptr(p["res"]), ptr(gout), ptr(pre),
             ptr(ry), None, ptr(mean), ptr(invstd), ptr(rw), ptr(rb), ptr(s3), ptr(ws3), float(n), ptr(dw), ptr(db))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(gout).all())
        # the gradient rows themselves are pinned by the two-pass comparison of test_gpu_ops.py; here their sums
        mask = None if mode == "none" else (y > 0)
        worst = max(worst, _check_bwd_sums_only((s3, dw, db), pre, gout, mask, mean, invstd, n,
                                                f"bwdstats C{C} mask {mode}"))
    record_property("reduce_rows_bwdstats", worst)


def _check_bwd_sums_only(got, x, dy, mask, mean, invstd, n, what):
    sums, dw, db = got
    C = x.shape[1]
    xh32 = (x - mean) * invstd
    s_g, s_gx, a_g, a_gx = R.bn_bwd_sums64(dy.double(), xh32.double(), mask)
    assert float(sums[2 * C]) == n, f"{what}: sums[2C]"
    r = [R.assert_sums(sums[:C], s_g, a_g, n, what + " sum g"), R.assert_sums(sums[C:2 * C], s_gx, a_gx, n, what + " sum g xhat")]
    for got_p, ref_p, ab, name in ((db, s_g, a_g, "db"), (dw, s_gx, a_gx, "dw")):
        ratio = float(((got_p.double() - ref_p).abs() / (R.ulp32(ref_p) + R.sums_bar(n, ab) + 1e-38)).max())
        assert ratio <= 1.0, f"{what}: {name} {ratio:.3g} x (1 ulp + gamma_n) (NaN: never written)"
        r.append(ratio)
    return max(r)
