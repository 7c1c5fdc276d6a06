"""Float64 yardstick of the instance norm and of the fused IBN pass (csrc/inorm.hip), written from the definitions in
plain torch, and the bars the kernels are held to.  Everything runs in the dtype and on the device of its inputs
(float64 on the GPU for the GPU tests); tests/test_inorm_ref_cpu.py checks it against F.instance_norm + autograd per
scan and shows that the bars pass a correct fp32 evaluation and fail a moved scan boundary and a dropped row.

Definitions (x [n, C], batch [n] the scan of every row, B scans, n_b rows in scan b):
  mean[b, c] = sum x / n_b,  var[b, c] = sum x^2 / n_b - mean^2 (biased),  invstd = (var + eps)^-1/2,
  xhat = (x - mean[b]) invstd[b],  y = xhat w + bias,
  dx = (g - m0[b] - xhat m1[b]) invstd[b] w,  m0 = sum_b g / n_b,  m1 = sum_b g xhat / n_b,
  dbias = sum g,  dweight = sum g xhat (over all rows).
A scan with no rows has mean 0, invstd 1 / sqrt(eps) and m0 = m1 = 0 (the kernels' documented placeholders).  eps is
the float32 1e-8 widened to double, as the kernels take it.

Bars (each derived next to its function; `sums_bar`, `stats_bounds`, `ulp32`, `U` are those of tests/sparse_ref.py):
  mean / invstd [B, C]   1 fp32 ulp of the float64 value + what double sums of n_b terms carry in; placeholders exact
  coef = (m0, m1)        1 ulp + gamma_{n_b} sum|terms| / n_b; exactly 0 for an empty scan
  dweight / dbias        1 ulp + gamma_n sum|terms|
  y, dx                  elementwise, from the kernel's OWN fp32 mean / invstd / coef: c u (magnitudes entering the fp32
                         expression), c = 5.05 (y) and 8 (dx) as for row BatchNorm (test_gpu_bn_rows64._elem_bar)
  fused dx               the two halves' bars + u (|dx_bn| + |dx_in|) for the final add
A non-finite value in a kernel output makes its ratio NaN, which fails every `<= 1` (outputs are pre-filled with NaN)."""
import math

import numpy as np
import torch

import sparse_ref as R

U = R.U
EPS = float(np.float32(1e-8))                                  # lidog_amd.me.IN_EPS as the C ABI receives it
BN_EPS = float(np.float32(1e-5))
INV_EMPTY = float(np.float32(1.0 / np.sqrt(np.float64(EPS))))  # invstd of var = 0, rounded as the kernels store it
C_Y, C_DX = 5.05, 8.0


# ------------------------------------------------------------------ the launcher's documented shape rules
def rb(C):
    """rows per pass of a reduction workgroup on the float4 path: 256 lanes, C / 4 lanes per row"""
    return 256 // (C // 4)


def per_wg(n, C):
    """sorted rows per reduction workgroup: max(4 RB, ceil(n / 256)) (at most 256 workgroups)"""
    return max(4 * rb(C), -(-n // 256))


def vector_path(C, B):
    """the float4 kernels (and the fused IBN entries): C % 4 == 0, C / 4 <= 256 lanes, 2 B C doubles of LDS <= 4096"""
    return C % 4 == 0 and 4 <= C <= 1024 and 2 * B * C <= 4096


# ------------------------------------------------------------------ float64 definitions
def segments64(batch, B):
    """(perm, seg_off [B + 1], counts [B]): the rows in stable batch order, where each scan starts in that order"""
    b = batch.long()
    counts = torch.bincount(b, minlength=B)
    perm = torch.sort(b, stable=True).indices
    seg_off = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    return perm, seg_off, counts


def _per_scan(v, batch, B):
    return torch.zeros((B, v.shape[1]), dtype=v.dtype, device=v.device).index_add_(0, batch.long(), v)


def in_stats64(x, batch, B, eps=EPS):
    """per (b, c): s1 = sum x, s2 = sum x^2, s1_abs = sum |x|, cnt [B]; from them mean, biased var, invstd (the
    placeholders for a scan with no rows)"""
    s1, s2, s1_abs = _per_scan(x, batch, B), _per_scan(x * x, batch, B), _per_scan(x.abs(), batch, B)
    cnt = torch.bincount(batch.long(), minlength=B)
    nb = cnt.to(x.dtype).clamp_min(1)[:, None]
    mean = s1 / nb
    var = torch.clamp_min(s2 / nb - mean * mean, 0.0)
    return dict(s1=s1, s2=s2, s1_abs=s1_abs, cnt=cnt, mean=mean, var=var, invstd=1.0 / torch.sqrt(var + eps))


def in_bwd_sums64(g, xhat, batch, B):
    """per (b, c): sg = sum g, sgx = sum g xhat and the sum|terms| ag, agx of both; db / dw [C] = their sums over b
    with sum|terms| a_db / a_dw"""
    gx = g * xhat
    sg, sgx, ag, agx = (_per_scan(v, batch, B) for v in (g, gx, g.abs(), gx.abs()))
    return dict(sg=sg, sgx=sgx, ag=ag, agx=agx, db=sg.sum(0), dw=sgx.sum(0), a_db=ag.sum(0), a_dw=agx.sum(0))


def norm_y64(x, mean, invstd, w, b):
    """y = (x - mean) invstd w + b and the magnitude scale |core| + |b| of its fp32 evaluation (operands broadcast)"""
    core = (x - mean) * invstd * w
    return core + b, core.abs() + b.abs()


def norm_dx64(g, x, mean, invstd, w, m0, m1):
    """dx = (g - m0 - xhat m1) invstd w and the scale (|g| + |m0| + |xhat m1|) |invstd w| (operands broadcast)"""
    xh = (x - mean) * invstd
    k = invstd * w
    return (g - m0 - xh * m1) * k, (g.abs() + m0.abs() + (xh * m1).abs()) * k.abs()


def in_y64(x, batch, mean, invstd, w, b):
    i = batch.long()
    return norm_y64(x, mean[i], invstd[i], w[None], b[None])


def in_dx64(g, x, batch, mean, invstd, w, m0, m1):
    """instance-norm data gradient from per-(b, c) mean / invstd / m0 / m1 [B, C]; returns (dx, scale)"""
    i = batch.long()
    return norm_dx64(g, x, mean[i], invstd[i], w[None], m0[i], m1[i])


def ibn_dx64(g_bn, g_in, x, batch, bn_mean, bn_invstd, bn_w, bn_m0, bn_m1, in_mean, in_invstd, in_w, in_m0, in_m1):
    """dx of relu(cat(bn(x), in(x))): the BatchNorm half ([C] statistics) plus the instance-norm half ([B, C]);
    g_* are the ReLU-masked halves of dy.  Returns (dx, bar): every half is the 8-rounding expression of bn_dx_scaled
    (C_DX u scale; the fp32 casts of m0 / m1 are among the eight), the final add rounds their sum once more:
    bar = C_DX u (scale_bn + scale_in) + u (|dx_bn| + |dx_in|)."""
    d_bn, s_bn = norm_dx64(g_bn, x, bn_mean[None], bn_invstd[None], bn_w[None], bn_m0[None], bn_m1[None])
    d_in, s_in = in_dx64(g_in, x, batch, in_mean, in_invstd, in_w, in_m0, in_m1)
    return d_bn + d_in, C_DX * U * (s_bn + s_in) + U * (d_bn.abs() + d_in.abs())


# ------------------------------------------------------------------ bars
def ratio(got, ref, bar):
    """worst |got - ref| / bar; a zero bar demands equality (inf otherwise); NaN if `got` holds a non-finite value"""
    err = (got.double() - ref).abs()
    one = torch.ones_like(err)
    r = torch.where(bar > 0, err / torch.where(bar > 0, bar, one),
                    torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    worst = float(r.max()) if r.numel() else 0.0
    return worst if bool(torch.isfinite(got).all()) else math.nan


def elem_ratio(got, ref, scale, c):
    """|got - ref| <= c u scale elementwise, scale the sum of the magnitudes entering the fp32 expression
    (test_gpu_bn_rows64._elem_bar: y = ((x - m) is) w + b is five roundings, <= 5 u scale, 1 % for second order; dx =
    (g - m0 - ((x - m) is) m1)(is w) with fp32 m0 / m1 is at most 7 u on any of its three terms, <= 8 u scale)"""
    return ratio(got, ref, c * U * scale + 1e-38)


def stats_ratios(mean, invstd, x, batch, B):
    """{'mean', 'invstd'}: kernel fp32 mean / invstd [B, C] against float64.  Bar per (b, c): sparse_ref.stats_bounds
    with n = n_b, i.e. 1 fp32 ulp of the float64 value + gamma_{n_b} sum|x| / n_b for the mean and 1 ulp + the
    propagated E[x^2] - E[x]^2 error for invstd.  A scan with no rows has bar 0: the placeholders exactly."""
    C = x.shape[1]
    s = in_stats64(x.double(), batch, B)
    ref_m, ref_i = s["mean"].clone(), s["invstd"].clone()
    bar_m, bar_i = torch.zeros_like(ref_m), torch.zeros_like(ref_m)
    for b, nb in enumerate(s["cnt"].tolist()):
        if nb == 0:
            ref_m[b], ref_i[b] = 0.0, INV_EMPTY
            continue
        m, _, i, d_m, _, d_i = R.stats_bounds(s["s1"][b], s["s2"][b], s["s1_abs"][b], nb, EPS)
        ref_m[b], ref_i[b] = m, i
        bar_m[b], bar_i[b] = R.ulp32(m) + d_m, R.ulp32(i) + d_i
    return {"mean": ratio(mean.reshape(B, C), ref_m, bar_m), "invstd": ratio(invstd.reshape(B, C), ref_i, bar_i)}


def bwd_ratios(coef, dw, db, g, xhat32, batch, B):
    """{'m0', 'm1', 'dw', 'db'}: coef [2, B, C] and the parameter gradients against the float64 sums of g and
    g xhat32 (xhat32: the kernel's fp32 xhat, two correctly rounded operations, widened exactly).
    m0 / m1 = (sum / n_b) cast to fp32: the double sum is within gamma_{n_b} sum|terms|, the division and the cast
    add less than 1 fp32 ulp: bar = ulp32(ref) + sums_bar(n_b, sum|terms|) / n_b; bar 0 (exactly 0) for an empty scan.
    dw / db = the per-scan double sums added over b and cast: bar = ulp32(ref) + sums_bar(n, sum|terms|)."""
    C, n = g.shape[1], g.shape[0]
    s = in_bwd_sums64(g.double(), xhat32.double(), batch, B)
    cnt = torch.bincount(batch.long(), minlength=B)
    nb = cnt.double().clamp_min(1)[:, None]
    ref0, ref1 = s["sg"] / nb, s["sgx"] / nb
    bar0, bar1 = torch.zeros_like(ref0), torch.zeros_like(ref0)
    for b, k in enumerate(cnt.tolist()):
        if k:
            bar0[b] = R.ulp32(ref0[b]) + R.sums_bar(k, s["ag"][b]) / k
            bar1[b] = R.ulp32(ref1[b]) + R.sums_bar(k, s["agx"][b]) / k
    coef = coef.reshape(2, B, C)
    return {"m0": ratio(coef[0], ref0, bar0), "m1": ratio(coef[1], ref1, bar1),
            "dw": ratio(dw.reshape(C), s["dw"], R.ulp32(s["dw"]) + R.sums_bar(n, s["a_dw"]) + 1e-38),
            "db": ratio(db.reshape(C), s["db"], R.ulp32(s["db"]) + R.sums_bar(n, s["a_db"]) + 1e-38)}


def assert_ratios(ratios, what):
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{what}: x their bars (NaN: never written): {bad}"


def unpack_bits(bits, count):
    """bool [count]: bit e & 31 of word e >> 5 (the layout of lidog_bn_apply_bits over the flattened tensor)"""
    e = torch.arange(count, device=bits.device)
    return ((bits.long()[e >> 5] >> (e & 31)) & 1).bool()


def pack_bits(mask):
    """int32 words of a ReLU mask in that layout (the last word zero-padded)"""
    flat = mask.reshape(-1).long()
    flat = torch.cat([flat, flat.new_zeros((-flat.numel()) % 32)]).reshape(-1, 32)
    words = (flat << torch.arange(32, device=flat.device)).sum(1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


# ------------------------------------------------------------------ inputs
def _uneven(n, k):
    """k uneven positive sizes that add up to n"""
    base = [n * (i + 1) // (k * (k + 1) // 2) for i in range(k)]
    base[-1] += n - sum(base)
    return base


def _at(bounds, n):
    """scan sizes from ascending scan boundaries"""
    e = [0] + list(bounds) + [n]
    return [e[i + 1] - e[i] for i in range(len(e) - 1)]


TINY = [1, 2, 3, 4, 5, 6, 7, 1, 2, 3, 4, 5, 6, 7, 3, 1, 2000]      # 16 scans shorter than RB(32) = 32, then one long
_PW64 = per_wg(5003, 64)                                            # = 4 RB = 64
_N40K = 40003
_PW96 = per_wg(_N40K, 96)                                           # = ceil(n / 256) = 157, no multiple of RB = 10


def _layouts():
    L = []

    def add(name, C, sizes, order="shuffled"):
        L.append(dict(id=f"{name}_C{C}_{order}", C=C, sizes=list(sizes), order=order))

    r = rb(96)
    for s in ([1], [2], [r - 1], [r], [r + 1], [4 * r + 1]):
        add(f"one{s[0]}", 96, s)
    for s in ([3000, 0, 2003], [0, 5003], [5003, 0], [1, 5001, 1]):
        add("x".join(map(str, s)), 32, s)
    add("3000x0x2003", 32, [3000, 0, 2003], "collated")
    add("tiny16", 32, TINY)
    add("tiny16", 32, TINY, "collated")
    # scan boundaries one before / on / one behind a workgroup boundary (per_wg = 4 RB, and per_wg = ceil(n / 256))
    add("wgedge", 64, _at([3 * _PW64 - 1, 10 * _PW64, 40 * _PW64 + 1], 5003))
    add("wgedge", 64, _at([3 * _PW64 - 1, 10 * _PW64, 40 * _PW64 + 1], 5003), "collated")
    add("n40k", 96, _at([50 * _PW96 - 1, 120 * _PW96, 200 * _PW96 + 1], _N40K))
    for C in (128, 256):                                            # either side of the 256-workgroup cap
        for d in (-1, 1):
            n = 256 * 4 * rb(C) + d
            add(f"cap{d:+d}", C, [n // 5, n - n // 5 - 7, 7])
    for C in (4, 12, 20, 32, 64, 96, 128, 256, 384, 1024, 1, 7, 10):
        add("width", C, [2500, 2503])
    add("gate16", 128, _uneven(4000, 16))                           # 2 B C = 4096: float4
    add("gate17", 128, _uneven(4000, 17))                           # 4352: scalar, C % 4 == 0
    add("gate2", 1024, [700, 801])                                  # 4096: float4
    add("gate3", 1024, [500, 0, 601])                               # 6144: scalar
    add("gate9", 256, _uneven(3000, 9))                             # 4608: scalar
    return L


LAYOUTS = _layouts()
assert _PW64 == 64 and _PW96 == 157 and _PW96 % rb(96)


def make_case(lay, device="cpu"):
    """Seeded inputs of one layout: the data of test_gpu_bn_rows64._data per scan -- N(0.5, 2), channel 0 of mean 1e3 and
    sigma 1, channel 1 constant within a scan (0.75 + b / 2: a row counted to the wrong scan shows exactly).  dy is
    random; its channel 1 (C + 1 of the [n, 2C] IBN gradient) is constant within a scan as well, since dx = 0 on a
    constant channel holds only where g - mean_b(g) = 0: dx = (g - mean g) invstd w there."""
    C, sizes = lay["C"], lay["sizes"]
    B, n = len(sizes), sum(sizes)
    g = torch.Generator().manual_seed(C * 7919 + n * 31 + B)
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    x = torch.randn((n, C), generator=g) * 2 + 0.5
    dy, dy2 = torch.randn((n, C), generator=g), torch.randn((n, 2 * C), generator=g)
    if C >= 2:
        x[:, 0] = torch.randn(n, generator=g) + 1e3
        x[:, 1] = 0.75 + 0.5 * batch
        dy[:, 1] = 0.25 * (batch + 1)
        dy2[:, C + 1] = -0.25 * (batch + 1)
    if lay["order"] == "shuffled":
        p = torch.randperm(n, generator=g)
        batch, x, dy, dy2 = batch[p], x[p], dy[p], dy2[p]
    d = dict(x=x.contiguous(), dy=dy.contiguous(), dy2=dy2.contiguous(), batch=batch.to(torch.int32).contiguous(),
             w=torch.rand(C, generator=g) + 0.5, b=torch.randn(C, generator=g),
             bn_w=torch.rand(C, generator=g) + 0.5, bn_b=torch.randn(C, generator=g))
    d = {k: v.to(device) for k, v in d.items()}
    d.update(B=B, C=C, n=n, sizes=sizes)
    return d


# ------------------------------------------------------------------ every output of an entry against the above
def check_in(o, d, what):
    """o: mean, invstd [B C], y, coef [2 B C], dw, db, dx of lidog_in_stats / _apply / _bwd_reduce / _bwd_apply on
    case d.  Returns the worst ratio per bar (all asserted <= 1)."""
    x, batch, B, C = d["x"], d["batch"], d["B"], d["C"]
    i = batch.long()
    r = stats_ratios(o["mean"], o["invstd"], x, batch, B)
    mean, invstd = o["mean"].reshape(B, C), o["invstd"].reshape(B, C)
    xh32 = (x - mean[i]) * invstd[i]                       # the kernels' fp32 xhat
    r.update(bwd_ratios(o["coef"], o["dw"], o["db"], d["dy"], xh32, batch, B))
    m64, i64, coef = mean.double(), invstd.double(), o["coef"].reshape(2, B, C).double()
    ref, scale = in_y64(x.double(), batch, m64, i64, d["w"].double(), d["b"].double())
    r["y"] = elem_ratio(o["y"], ref, scale, C_Y)
    ref, scale = in_dx64(d["dy"].double(), x.double(), batch, m64, i64, d["w"].double(), coef[0], coef[1])
    r["dx"] = elem_ratio(o["dx"], ref, scale, C_DX)
    assert_ratios(r, what)
    if C >= 2 and d["n"]:                                  # the channel that is constant within a scan: exact
        assert torch.equal(xh32[:, 1], torch.zeros_like(xh32[:, 1])), f"{what}: constant channel xhat != 0"
        assert torch.equal(o["y"][:, 1], d["b"][1].expand(d["n"])), f"{what}: constant channel y != bias"
        assert torch.equal(o["dx"][:, 1], torch.zeros_like(o["dx"][:, 1])), f"{what}: constant channel dx != 0"
        assert torch.equal(invstd[:, 1], torch.full_like(invstd[:, 1], INV_EMPTY)), f"{what}: constant channel invstd"
    return r


def check_ibn(o, d, what):
    """o: bn_mean, bn_invstd [C] (lidog_bn_stats), in_mean, in_invstd, y_in (lidog_in_stats / _apply, checked by
    check_in), and y [n, 2C], bits, bn_sums [2C + 1], bn_dw, bn_db, coef, in_dw, in_db, dx of the three lidog_ibn_*
    entries.  ReLU decisions are the kernel's own bits, asserted equal to y > 0.  Without bn_sums (module-level
    callers: autograd does not hand them out) m0 / m1 of the BatchNorm half are the float64 sums over n, as in
    test_gpu_bn_rows64._check_bwd: their fp32 casts are two of the eight roundings of C_DX."""
    x, batch, B, C, n = d["x"], d["batch"], d["B"], d["C"], d["n"]
    i = batch.long()
    y = o["y"]
    mask = unpack_bits(o["bits"], n * 2 * C).reshape(n, 2 * C)
    assert torch.equal(mask, y > 0), f"{what}: ReLU bit mask differs from y > 0"
    assert torch.equal(y[:, C:], torch.relu(o["y_in"])), f"{what}: IN half of y is not relu(lidog_in_apply) bit for bit"
    bm, bi = o["bn_mean"].double(), o["bn_invstd"].double()
    ref, scale = norm_y64(x.double(), bm[None], bi[None], d["bn_w"].double()[None], d["bn_b"].double()[None])
    r = {"y_bn": elem_ratio(y[:, :C], torch.clamp_min(ref, 0.0), scale, C_Y)}
    if C >= 2:
        assert torch.equal(y[:, C + 1], torch.relu(d["b"][1]).expand(n)), f"{what}: constant channel y != relu(bias)"
    g = torch.where(mask, d["dy2"], torch.zeros_like(d["dy2"]))
    g_bn, g_in = g[:, :C], g[:, C:]
    # BatchNorm half: the bars of test_gpu_bn_rows64._check_bwd
    xh_bn = (x - o["bn_mean"]) * o["bn_invstd"]
    s_g, s_gx, a_g, a_gx = R.bn_bwd_sums64(g_bn.double(), xh_bn.double())
    if "bn_sums" in o:
        assert float(o["bn_sums"][2 * C]) == n, f"{what}: bn_sums[2C] = {float(o['bn_sums'][2 * C])}, want {n}"
        r["bn_sum_g"] = R.assert_sums(o["bn_sums"][:C], s_g, a_g, n, what + " bn sum g")
        r["bn_sum_gx"] = R.assert_sums(o["bn_sums"][C:2 * C], s_gx, a_gx, n, what + " bn sum g xhat")
        s_m0, s_m1 = o["bn_sums"][:C].double() / n, o["bn_sums"][C:2 * C].double() / n
    else:
        s_m0, s_m1 = s_g / n, s_gx / n
    r["bn_db"] = ratio(o["bn_db"], s_g, R.ulp32(s_g) + R.sums_bar(n, a_g) + 1e-38)
    r["bn_dw"] = ratio(o["bn_dw"], s_gx, R.ulp32(s_gx) + R.sums_bar(n, a_gx) + 1e-38)
    # instance-norm half
    mean, invstd = o["in_mean"].reshape(B, C), o["in_invstd"].reshape(B, C)
    xh_in = (x - mean[i]) * invstd[i]
    r.update({"in_" + k: v for k, v in bwd_ratios(o["coef"], o["in_dw"], o["in_db"], g_in, xh_in, batch, B).items()})
    coef = o["coef"].reshape(2, B, C).double()
    ref, bar = ibn_dx64(g_bn.double(), g_in.double(), x.double(), batch, bm, bi, d["bn_w"].double(), s_m0, s_m1, mean.double(), invstd.double(), d["w"].double(), coef[0], coef[1])
    r["dx"] = ratio(o["dx"], ref, bar + 1e-38)
    assert_ratios(r, what)
    return r
