"""Float64 yardstick of the 2-D BEV head (lidog_amd.bev.Encoder2D): the convolutions and BatchNorm2d written from their
definitions, for comparison with the HIP kernels of csrc/conv2d.hip, csrc/conv2d_sparse.hip and the NCHW branch of
csrc/bn.hip.  Everything runs in the dtype and on the device of its inputs (float64 on the GPU for the GPU tests);
tests/test_bev_ref_cpu.py checks it against torch.nn.functional in float64.

Also the three bars the kernel tests share:
  exact      integer-valued operands whose partial sums stay below 2^24: any fp32 summation order is exact, so the
             kernel result must equal the float64 result cast to fp32 (`exact_operands`, `assert_exact`);
  precision  random fp32 operands: elementwise |got - ref| <= 1.01 K u sum|terms| (the rigorous bound of any fp32
             summation of K terms, u = 2^-24) and a relative Frobenius error <= PREC_C u sqrt(K) (`precision_ratios`);
  written    outputs are pre-filled with NaN, so an element a kernel never writes fails either bar.

The k3 s2 p1 convolution is the sum of its nine taps; tap (ky, kx) pairs output pixel (yo, xo) with padded input pixel
(2 yo + ky, 2 xo + kx), so every tap is one strided slice of the padded input and one matrix product over channels."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
# Frobenius bar c: relative error <= c u sqrt(K).  fp32 accumulation (recursive, blocked or split) of random terms stays
# near u sqrt(K) / 2; operands rounded to a 10-bit mantissa (tf32) give ~2^-12 whatever K is, i.e. c ~ 4096 / sqrt(K).
# Measured on the MI355X over every kernel and shape of tests/test_gpu_conv2d.py: worst c = 0.76 (dense data gradient);
# the elementwise bound reached 0.99 of itself (one- and two-term sums, where it is tight).
PREC_C = 2.0


def _out(n):
    return (n - 1) // 2 + 1       # k3 s2 p1


def _taps():
    return [(ky, kx) for ky in range(3) for kx in range(3)]


def _tap_slice(xp, ky, kx, Ho, Wo):
    """padded input [B, C, H+2, W+2] -> the pixels tap (ky, kx) reads for the Ho x Wo outputs"""
    return xp[:, :, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2]


def conv3s2_fwd64(x, w):
    """y[b, o, yo, xo] = sum_{c, ky, kx} w[o, c, ky, kx] x[b, c, 2 yo - 1 + ky, 2 xo - 1 + kx] (zero outside);
    differentiable with autograd (encoder2d64)"""
    B, C, H, W = x.shape
    Ho, Wo = _out(H), _out(W)
    xp = F.pad(x, (1, 1, 1, 1))
    y = None
    for ky, kx in _taps():
        t = torch.einsum("oc,bchw->bohw", w[:, :, ky, kx], _tap_slice(xp, ky, kx, Ho, Wo))
        y = t if y is None else y + t
    return y


def conv3s2_dgrad64(gy, w, H, W):
    """gx[b, c, y, x] = sum over the (output pixel, tap) pairs that read (y, x) of w[o, c, ky, kx] gy[b, o, yo, xo]"""
    B, O, Ho, Wo = gy.shape
    C = w.shape[1]
    gxp = torch.zeros((B, C, H + 2, W + 2), dtype=gy.dtype, device=gy.device)
    for ky, kx in _taps():
        _tap_slice(gxp, ky, kx, Ho, Wo).add_(torch.einsum("oc,bohw->bchw", w[:, :, ky, kx], gy))
    return gxp[:, :, 1:H + 1, 1:W + 1]


def conv3s2_wgrad64(x, gy, pix_chunk=1 << 16):
    """gw[o, c, ky, kx] = sum_{b, yo, xo} gy[b, o, yo, xo] x[b, c, 2 yo - 1 + ky, 2 xo - 1 + kx]; the pixels in chunks of
    output rows (the full-size image would otherwise copy nine [B, C, Ho, Wo] slices at once)"""
    B, C, H, W = x.shape
    O, Ho, Wo = gy.shape[1], gy.shape[2], gy.shape[3]
    xp = F.pad(x, (1, 1, 1, 1))
    gw = torch.zeros((O, C, 3, 3), dtype=x.dtype, device=x.device)
    rows = max(1, pix_chunk // max(1, B * Wo))
    for y0 in range(0, Ho, rows):
        y1 = min(Ho, y0 + rows)
        g = gy[:, :, y0:y1]
        xs = xp[:, :, 2 * y0:2 * y1 + 1]          # padded rows 2 y0 .. 2 (y1 - 1) + 2
        for ky, kx in _taps():
            gw[:, :, ky, kx] += torch.einsum("bohw,bchw->oc", g, _tap_slice(xs, ky, kx, y1 - y0, Wo))
    return gw


def conv3s2_abs_terms(x, w, gy, which):
    """sum |terms| of every output element of `which` in {"fwd", "dgrad", "wgrad"} (the convolution of the absolute
    values), with the reduction length K of the bound"""
    if which == "fwd":
        return conv3s2_fwd64(x.abs(), w.abs()), 9 * x.shape[1]
    if which == "dgrad":
        return conv3s2_dgrad64(gy.abs(), w.abs(), x.shape[2], x.shape[3]), 4 * gy.shape[1]
    return conv3s2_wgrad64(x.abs(), gy.abs()), gy.shape[0] * gy.shape[2] * gy.shape[3]


def pw_fwd64(x, w, b=None):
    """1x1 convolution: y[b, o, p] = sum_c w[o, c] x[b, c, p] + bias[o]; w [O, C, 1, 1] or [O, C]"""
    w2 = w.reshape(w.shape[0], -1)
    y = torch.einsum("oc,bchw->bohw", w2, x)
    return y if b is None else y + b.reshape(1, -1, 1, 1)


def pw_dgrad64(gy, w):
    return torch.einsum("oc,bohw->bchw", w.reshape(w.shape[0], -1), gy)


def pw_wgrad64(x, gy):
    """(gw [O, C, 1, 1], gbias [O])"""
    gw = torch.einsum("bohw,bchw->oc", gy, x)
    return gw.reshape(gw.shape[0], gw.shape[1], 1, 1), gy.sum(dim=(0, 2, 3))


def bn2d_train_fwd64(x, weight, bias, running_mean, running_var, momentum, eps, relu):
    """BatchNorm2d in training mode: normalised with the batch mean and the BIASED variance over (b, h, w); running
    statistics updated with the UNBIASED variance, r = (1 - momentum) r + momentum s.
    Returns (y, new running_mean, new running_var, (mean, invstd)) -- the last for bn2d_bwd64."""
    n = x.shape[0] * x.shape[2] * x.shape[3]
    mean = x.mean(dim=(0, 2, 3))
    xc = x - mean.reshape(1, -1, 1, 1)
    var = (xc * xc).sum(dim=(0, 2, 3)) / n
    invstd = 1.0 / torch.sqrt(var + eps)
    y = xc * (invstd * weight).reshape(1, -1, 1, 1) + bias.reshape(1, -1, 1, 1)
    if relu:
        y = torch.clamp_min(y, 0.0)
    unbiased = var * n / (n - 1) if n > 1 else var
    rm = (1.0 - momentum) * running_mean + momentum * mean
    rv = (1.0 - momentum) * running_var + momentum * unbiased
    return y, rm, rv, (mean, invstd)


def bn2d_eval_fwd64(x, weight, bias, running_mean, running_var, eps, relu):
    invstd = 1.0 / torch.sqrt(running_var + eps)
    y = (x - running_mean.reshape(1, -1, 1, 1)) * (invstd * weight).reshape(1, -1, 1, 1) + bias.reshape(1, -1, 1, 1)
    return (torch.clamp_min(y, 0.0) if relu else y), (running_mean, invstd)


def bn2d_bwd64(dy, x, y, weight, saved, training, relu, mask=None):
    """(dx, dweight, dbias) of BatchNorm2d (+ the fused ReLU: dy is masked where the output y is 0, or outside `mask`).
    training: dx = w invstd (dy' - mean(dy') - xhat mean(dy' xhat)); eval: the statistics are constants, dx = w invstd dy'"""
    mean, invstd = saved
    if relu:
        dy = torch.where(y > 0 if mask is None else mask, dy, torch.zeros_like(dy))
    xhat = (x - mean.reshape(1, -1, 1, 1)) * invstd.reshape(1, -1, 1, 1)
    db = dy.sum(dim=(0, 2, 3))
    dw = (dy * xhat).sum(dim=(0, 2, 3))
    k = (weight * invstd).reshape(1, -1, 1, 1)
    if not training:
        return dy * k, dw, db
    n = x.shape[0] * x.shape[2] * x.shape[3]
    dx = k * (dy - (db / n).reshape(1, -1, 1, 1) - xhat * (dw / n).reshape(1, -1, 1, 1))
    return dx, dw, db


class _BN64(torch.autograd.Function):
    """bn2d_train_fwd64 / bn2d_bwd64 as one autograd node (encoder2d64)"""

    @staticmethod
    def forward(ctx, x, weight, bias, mean, invstd, relu, mask):
        y = (x - mean.reshape(1, -1, 1, 1)) * (invstd * weight).reshape(1, -1, 1, 1) + bias.reshape(1, -1, 1, 1)
        if relu:
            y = torch.where(mask, y, torch.zeros_like(y)) if mask is not None else torch.clamp_min(y, 0.0)
        ctx.save_for_backward(x, y, weight, mean, invstd)
        ctx.relu, ctx.mask = relu, mask
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, weight, mean, invstd = ctx.saved_tensors
        dx, dw, db = bn2d_bwd64(dy, x, y, weight, (mean, invstd), True, ctx.relu, ctx.mask)
        return dx, dw, db, None, None, None, None


def encoder2d64(x, p, momentum=0.1, eps=1e-5, keep=None, relu_masks=None):
    """Encoder2D in training mode, the literal composition Conv2d(k3 s2 p1) -> BN -> ReLU, twice, -> Conv2d(k1) + bias,
    in the dtype of x.  `p`: the Encoder2D state_dict keys (parameters may require grad; gradients come from autograd
    through the functions above).  Returns (logits, {running-statistics key: updated value}).  `keep`: optional dict that
    receives (input, output) of each 3x3 convolution under its weight's key, the output with retain_grad().
    `relu_masks`: optional pair of bool masks (output > 0) that replace the ReLU decisions of the two BatchNorms -- a
    kernel's own decisions, for a comparison that is not dominated by outputs within rounding of 0 switching sides."""
    pre = "down1.maxpool_conv.0.double_conv."
    stats = {}
    h = x
    for i, (conv, bn) in enumerate((("0", "1"), ("3", "4"))):
        hin = h
        h = conv3s2_fwd64(h, p[pre + conv + ".weight"])
        if keep is not None and h.requires_grad:
            h.retain_grad()
            keep[pre + conv + ".weight"] = (hin, h)
        k = pre + bn
        with torch.no_grad():
            _, rm, rv, (mean, invstd) = bn2d_train_fwd64(h, p[k + ".weight"], p[k + ".bias"], p[k + ".running_mean"],
                                                        p[k + ".running_var"], momentum, eps, True)
        stats[k + ".running_mean"], stats[k + ".running_var"] = rm, rv
        h = _BN64.apply(h, p[k + ".weight"], p[k + ".bias"], mean, invstd, True,
                        None if relu_masks is None else relu_masks[i])
    return pw_fwd64(h, p["out_conv.conv.weight"], p["out_conv.conv.bias"]), stats


# ------------------------------------------------------------------ bars
def exact_operands(shape, gen, lo, hi, zero_frac, device="cpu"):
    """integer-valued float32 operands in [lo, hi], a fraction zero_frac of them zero (like ReLU output)"""
    v = torch.randint(lo, hi + 1, shape, generator=gen).float()
    if zero_frac > 0:
        v = torch.where(torch.rand(shape, generator=gen) < zero_frac, torch.zeros_like(v), v)
    return v.to(device)


def assert_exact(got, ref64, abs_terms64, what):
    """every partial sum below 2^24 (bounded by sum |terms|), then got must equal the float64 result cast to fp32"""
    assert float(abs_terms64.max()) < 2.0 ** 24, f"{what}: operands too large for the exact bar"
    ok = got == ref64.float()
    if not bool(ok.all()):
        bad = (~ok).nonzero()[:5].tolist()
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements differ from the exact result "
                             f"(first at {bad}; NaN means never written)")


def precision_ratios(got, ref64, abs_terms64, K):
    """(elementwise ratio max |got - ref| / (1.01 K u sum|terms|), Frobenius ratio |got - ref|_F / (|ref|_F u sqrt(K)));
    the bar is ratio_elem <= 1 and ratio_fro <= PREC_C.  NaN (never written) makes both NaN."""
    err = (got.double() - ref64).abs()
    bound = 1.01 * K * U * abs_terms64
    # an element whose terms are all zero must be exactly zero
    elem = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                       torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    r_elem = float(elem.max()) if elem.numel() else 0.0
    if not bool(torch.isfinite(got).all()):
        r_elem = math.nan
    nref = float(torch.linalg.vector_norm(ref64))
    r_fro = float(torch.linalg.vector_norm(err)) / (nref * U * math.sqrt(K)) if nref > 0 else float(err.max() > 0)
    if not bool(torch.isfinite(got).all()):
        r_fro = math.nan
    return r_elem, r_fro


def assert_precision(got, ref64, abs_terms64, K, what, c=None):
    c = PREC_C if c is None else c
    r_elem, r_fro = precision_ratios(got, ref64, abs_terms64, K)
    assert r_elem <= 1.0, f"{what}: elementwise error {r_elem:.3g} x the fp32 summation bound (NaN: never written)"
    assert r_fro <= c, f"{what}: Frobenius error {r_fro:.3g} u sqrt(K), bar {c} (NaN: never written)"
    return r_elem, r_fro


def round_mantissa(t, bits=10):
    """round-to-nearest-even of float32 values to `bits` explicit mantissa bits (bits = 10: tf32)"""
    i = t.float().contiguous().view(torch.int32).long() & 0xFFFFFFFF
    sign, mag = i & 0x80000000, i & 0x7FFFFFFF
    drop = 23 - bits
    mag = ((mag + (1 << (drop - 1)) - 1 + ((mag >> drop) & 1)) >> drop) << drop
    r = sign | mag
    r = torch.where(r >= 1 << 31, r - (1 << 32), r)
    return r.to(torch.int32).view(torch.float32).reshape(t.shape)
