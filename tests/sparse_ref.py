"""Float64 yardstick of the 3-D trunk's weight gradient and row BatchNorm, written from the definitions, for comparison
with the HIP kernels of csrc/sconv.hip / csrc/sconv_mfma.hip (lidog_sconv_wgrad, lidog_colsum) and the [rows, C] branch
of csrc/bn.hip.  Everything runs in the dtype and on the device of its inputs (float64 on the GPU for the GPU tests);
tests/test_sparse_ref_cpu.py checks it against autograd of F.conv3d / F.conv_transpose3d on the densified grid.

The bars are those of tests/bev_ref.py (exact, precision, written); the weight gradient applies the precision bar per
offset k with K = P_k, the number of pairs of that offset (`assert_wgrad_precision`).  The BatchNorm sums, which the
kernels accumulate in double, get the bar gamma_n = 1.01 n 2^-53 sum|terms| (`assert_sums`)."""
import math

import torch

from bev_ref import (U, assert_exact, assert_precision, bn2d_bwd64, bn2d_eval_fwd64, bn2d_train_fwd64,  # noqa: F401
                     exact_operands, precision_ratios, round_mantissa)

U64 = 2.0 ** -53


# ------------------------------------------------------------------ sparse convolution weight gradient
def wgrad64(A, pair_a, G, pair_g, k_off, chunk=1 << 18):
    """gW[k] = sum over the pairs p of offset k (k_off[k] <= p < k_off[k+1]) of A[pair_a[p]]^T G[pair_g[p]]  [K, Cin, Cout],
    abs_terms64: the same sum of |A| and |G|, and P_k [K] (int64, host).  The pairs of an offset in chunks of `chunk`
    (a bench-size centre offset would otherwise gather two [P_k, C] copies at once)."""
    k_off = [int(v) for v in k_off]
    K = len(k_off) - 1
    Cin, Cout = A.shape[1], G.shape[1]
    gW = torch.zeros((K, Cin, Cout), dtype=A.dtype, device=A.device)
    ab = torch.zeros_like(gW)
    for k in range(K):
        for p0 in range(k_off[k], k_off[k + 1], chunk):
            p1 = min(k_off[k + 1], p0 + chunk)
            a = A[pair_a[p0:p1].long()]
            g = G[pair_g[p0:p1].long()]
            gW[k] += a.t() @ g
            ab[k] += a.abs().t() @ g.abs()
    P_k = torch.tensor([k_off[k + 1] - k_off[k] for k in range(K)], dtype=torch.int64)
    return gW, ab, P_k


def assert_wgrad_precision(got, ref64, abs64, P_k, what, c=None):
    """the precision bar of bev_ref per offset (K = P_k pairs summed); returns the worst (elementwise, Frobenius)
    ratios.  An offset without pairs must come out exactly 0."""
    worst_e, worst_f = 0.0, 0.0
    for k in range(ref64.shape[0]):
        e, f = assert_precision(got[k], ref64[k], abs64[k], max(int(P_k[k]), 1), f"{what} offset {k}", c)
        worst_e, worst_f = max(worst_e, e), max(worst_f, f)
    return worst_e, worst_f


def colsum64(G):
    """bias gradient of a convolution: column sums of the output gradient [n, C] -> ([C], sum |terms|)"""
    return G.sum(dim=0), G.abs().sum(dim=0)


# ------------------------------------------------------------------ BatchNorm over rows ([n, C], hw = 1)
def _img(x):
    return x.reshape(x.shape[0], x.shape[1], 1, 1)


def bn_rows_train_fwd64(x, weight, bias, running_mean, running_var, momentum, eps, relu):
    """bev_ref.bn2d_train_fwd64 on [n, C] viewed as [n, C, 1, 1]"""
    y, rm, rv, saved = bn2d_train_fwd64(_img(x), weight, bias, running_mean, running_var, momentum, eps, relu)
    return y.reshape(x.shape), rm, rv, saved


def bn_rows_eval_fwd64(x, weight, bias, running_mean, running_var, eps, relu):
    y, saved = bn2d_eval_fwd64(_img(x), weight, bias, running_mean, running_var, eps, relu)
    return y.reshape(x.shape), saved


def bn_rows_bwd64(dy, x, y, weight, saved, training, relu, mask=None):
    """bev_ref.bn2d_bwd64 on rows; `mask` [n, C] bool replaces y > 0 as the ReLU decision"""
    dx, dw, db = bn2d_bwd64(_img(dy), _img(x), None if y is None else _img(y), weight, saved, training, relu,
                            None if mask is None else _img(mask))
    return dx.reshape(x.shape), dw, db


def bn_sums64(x):
    """(sum x [C], sum x^2 [C], n) as the statistics reductions store them, and sum |x| (the sum|terms| of the first
    sum; that of the second is the second sum itself)"""
    return x.sum(dim=0), (x * x).sum(dim=0), x.shape[0], x.abs().sum(dim=0)


def bn_bwd_sums64(dy, xhat, mask=None):
    """(sum g [C], sum g xhat [C]) of the backward reductions, g = dy where `mask` (ReLU decisions) else 0, and
    sum|terms| of both"""
    g = dy if mask is None else torch.where(mask, dy, torch.zeros_like(dy))
    gx = g * xhat
    return g.sum(dim=0), gx.sum(dim=0), g.abs().sum(dim=0), gx.abs().sum(dim=0)


def sums_bar(n, abs_terms):
    """gamma_n of a double summation of n terms: |got - ref| <= 1.01 n 2^-53 sum|terms|"""
    return 1.01 * max(int(n), 1) * U64 * abs_terms


def assert_sums(got, ref, abs_terms, n, what):
    """double sums against the float64 sums; returns the worst ratio to the bar (a lost row moves a sum by one
    term, far outside gamma_n unless the term is zero)"""
    err = (got.double() - ref).abs()
    bar = sums_bar(n, abs_terms)
    r = torch.where(bar > 0, err / torch.where(bar > 0, bar, torch.ones_like(bar)),
                    torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    worst = float(r.max()) if r.numel() else 0.0
    if not bool(torch.isfinite(got).all()):
        worst = math.nan
    assert worst <= 1.0, f"{what}: sums off by {worst:.3g} x the double summation bound (NaN: never written)"
    return worst


def ulp32(v):
    """spacing of float32 at |v| (as float64)"""
    a = v.double().abs().float()
    nxt = torch.nextafter(a, torch.full_like(a, math.inf))
    return (nxt.double() - a.double())


def stats_bounds(s1, s2, s1_abs, n, eps):
    """float64 (mean, invstd) from the float64 sums and the admissible errors of a kernel's fp32 mean / invstd derived
    from double sums that carry gamma_n errors (bar = 1 fp32 ulp of the float64 value plus the propagated error):
      mean   = s1 / n:                         |d mean| <= gamma_n s1_abs / n
      var    = s2 / n - mean^2 (E[x^2] - E[x]^2)  |d var| <= gamma_n E[x^2] + 2 |mean| |d mean| + the double rounding
      invstd = (var + eps)^-1/2                |d invstd| / invstd <= 1/2 |d var| / (var + eps)
    i.e. the relative invstd error 1/2 gamma_n (E[x^2] + m^2) / (var + eps), with s1_abs / n >= |m| in place of |m|.
    Returns (mean, biased var, invstd, d_mean, d_var, d_invstd), all float64."""
    mean = s1 / n
    var = torch.clamp_min(s2 / n - mean * mean, 0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    d_mean = sums_bar(n, s1_abs) / n
    d_var = sums_bar(n, s2) / n + 2.0 * mean.abs() * d_mean + d_mean * d_mean + 4 * U64 * (s2 / n)
    d_inv = 0.5 * d_var / (var + eps) * invstd
    return mean, var, invstd, d_mean, d_var, d_inv


def assert_stats(mean_got, invstd_got, s1, s2, s1_abs, n, eps, what):
    """fp32 mean / invstd within 1 ulp of the float64 value plus what the double sums carry in; returns worst ratios"""
    mean, _, invstd, d_mean, _, d_inv = stats_bounds(s1, s2, s1_abs, n, eps)
    out = []
    for got, ref, d, name in ((mean_got, mean, d_mean, "mean"), (invstd_got, invstd, d_inv, "invstd")):
        err = (got.double() - ref).abs()
        bar = ulp32(ref) + d
        r = float((err / bar).max()) if err.numel() else 0.0
        if not bool(torch.isfinite(got).all()):
            r = math.nan
        assert r <= 1.0, f"{what}: {name} off by {r:.3g} x (1 ulp + propagated sums error) (NaN: never written)"
        out.append(r)
    return out


def running64(rm0, rv0, mean, var_biased, n, momentum):
    """running statistics after one training pass: unbiased variance n / (n - 1) (n = 1: the biased one)"""
    unb = var_biased * n / (n - 1) if n > 1 else var_biased
    return (1.0 - momentum) * rm0 + momentum * mean, (1.0 - momentum) * rv0 + momentum * unb


def assert_running(got_rm, got_rv, rm64, rv64, rm0, rv0, momentum, d_mean, d_unbiased, what):
    """fp32 update r = (1 - m) r0 + m s: a handful of fp32 roundings of terms no larger than |r0| and |s|, plus the
    fp32 cast of s and the error s carries from the double sums (d_mean, d_unbiased = d_var n / (n - 1));
    bar = 4 u (|(1 - m) r0| + |m s|) + m d_s + 1 ulp of the result"""
    out = []
    for got, ref, r0, d_s, name in ((got_rm, rm64, rm0, d_mean, "running_mean"),
                                    (got_rv, rv64, rv0, d_unbiased, "running_var")):
        s = (ref - (1.0 - momentum) * r0.double()) / momentum
        bar = 4 * U * ((1.0 - momentum) * r0.double().abs() + momentum * s.abs()) + momentum * d_s + ulp32(ref)
        err = (got.double() - ref).abs()
        r = float((err / bar).max()) if err.numel() else 0.0
        if not bool(torch.isfinite(got).all()):
            r = math.nan
        assert r <= 1.0, f"{what}: {name} off by {r:.3g} x its fp32 update bound (NaN: never written)"
        out.append(r)
    return out
