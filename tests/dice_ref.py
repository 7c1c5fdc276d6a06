"""Float64 yardstick of the DICE losses (lidog_amd.losses, csrc/losses.hip), written from the definition of
SoftDICELoss / DICELoss and independent of every lidog_* entry point:

  p  = softmax of the fp32 logits in float64;  rows carrying the ignore label take no part;
  t  = one-hot (DICE) or label-smoothed one-hot (soft): 1 - eps on the label, eps / (C - 1) elsewhere, each rounded to
       float32 as the reference stores them (torch.empty(...) then item assignment);
  I_c = sum_r p t,  U_c = sum_r (p^2 if powerize else p) + sum_r t + 1e-12,  present_c = (label count > 0) or 1;
  loss = 1 - sum_c present_c 2 I_c / U_c / (sum_c present_c + 1e-12), minus 1 with neg_range;
  the gradient by autograd.  The loss depends on the rows only through the class sums, so rows are processed in chunks
  of CHUNK_ROWS: one pass for the sums, then d loss / d sums from autograd on the closed form, then per chunk the
  gradient of sum_c (dL/dI_c I_c + dL/dS_c S_c) -- the same chain rule, without a graph over 5 * 2^20 x 20 logits.

Bars, from the kernels' fp32 arithmetic (u = 2^-24; first order, each multiplied by 1.01):
  softmax    d = x - m rounds (|d| u), expf is within 1 ulp (2u), so each exponential carries (|d| + 2) u and the row
             sum, whose largest term is exp(0) = 1 exactly, (M + 2) u + (C - 1) u; the reciprocal and the product add 2u:
             e_p = (2M + C + 5) u with M = the largest |x - max_row(x)| over the scored rows.  Below the normal range
             (p < 2^-126: saturated logits) the error is absolute instead: TINY per element.
  targets    the kernel forms t_on = 1 - (float)eps and t_off = (float)eps / (C - 1) in fp32, the reference rounds the
             float64 values once: they differ by at most e_t = 3u relative (0 for hard targets).
  sums       each thread adds at most r = ceil(n / (blocks * 256)) rows in fp32, every term non-negative, so a class sum
             keeps the relative bound of its terms plus r u, plus one rounding of the product:
             e_I = e_p + e_t + (r + 1) u,  e_S = (2 e_p + u if powerize else e_p) + r u,  e_T = e_t + r u,
             e_U = max(e_S, e_T) (the partials are added in float64: negligible).
  loss       2 I / U carries e_I + e_U, and so does the sum of the non-negative present terms;  the float64 value is
             then rounded to fp32 (u |1 - iou|) and, with neg_range, offset by -1 in fp32 (u |loss|).
  gradient   coefficients a_c = -2 pres / (den U_c) and b_c = 2 pres I_c / (den U_c^2) rounded to fp32: e_a = e_U + u,
             e_b = e_I + 2 e_U + u; gp_c = a_c t + b_c q (q = 2p or 1); dot = sum_c p_c gp_c in fp32;
             g_c = gout p_c (gp_c - dot): the error of each step propagated with the absolute values of its terms
             (`grad_bound`), since gp_c - dot cancels."""
import math
from types import SimpleNamespace

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
CHUNK_ROWS = 1 << 20
MAX_BLOCKS, ROWS_PER_BLOCK = 1024, 256 * 4     # csrc/losses.hip: dice_blocks


def targets(C, soft, eps):
    """(t_on, t_off) as the reference stores them: float64 values rounded to float32"""
    if not soft:
        return 1.0, 0.0
    return float(torch.tensor(1 - eps, dtype=torch.float32)), float(torch.tensor(eps / (C - 1), dtype=torch.float32))


def rows_per_thread(n):
    nb = min(MAX_BLOCKS, max(1, -(-n // ROWS_PER_BLOCK)))
    return max(1, -(-n // (nb * 256)))


def _chunks(n):
    return [(r0, min(n, r0 + CHUNK_ROWS)) for r0 in range(0, n, CHUNK_ROWS)] or [(0, 0)]


def _rows(logits, target, ignore, r0, r1, C, t_on, t_off):
    x = logits[r0:r1].detach().double()
    t = target[r0:r1].long()
    valid = (t != ignore) if ignore is not None else torch.ones_like(t, dtype=torch.bool)
    onehot = (t.unsqueeze(1) == torch.arange(C, device=t.device)) & valid.unsqueeze(1)
    one = torch.ones((), dtype=torch.float64, device=t.device)
    tw = torch.where(onehot, t_on * one, t_off * one) * valid.unsqueeze(1)
    return x, valid, onehot, tw


def dice64(logits, target, ignore=None, soft=True, eps=0.05, powerize=True, use_tmask=True, neg_range=False, gout=1.0):
    """-> namespace: loss (float64, 0-dim), grad [n, C] float64 (times gout), the class sums I, S, T, cnt, the
    coefficients a, b of the gradient and what the bars need"""
    n, C = logits.shape
    dev = logits.device
    t_on, t_off = targets(C, soft, eps)
    I = torch.zeros(C, dtype=torch.float64, device=dev)
    S, T, cnt = torch.zeros_like(I), torch.zeros_like(I), torch.zeros_like(I)
    M = 0.0
    for r0, r1 in _chunks(n):
        x, valid, onehot, tw = _rows(logits, target, ignore, r0, r1, C, t_on, t_off)
        p = torch.softmax(x, dim=1) * valid.unsqueeze(1)
        I += (p * tw).sum(0)
        S += (p * p if powerize else p).sum(0)
        T += tw.sum(0)
        cnt += onehot.double().sum(0)
        if bool(valid.any()):
            M = max(M, float((x.max(dim=1).values - x.min(dim=1).values)[valid].max()))
    Ig, Sg = I.clone().requires_grad_(True), S.clone().requires_grad_(True)
    pres = (cnt > 0).double() if use_tmask else torch.ones_like(cnt)
    uni = Sg + T + 1e-12
    iou = (pres * 2 * Ig / uni).sum() / (pres.sum() + 1e-12)
    loss = -iou if neg_range else 1 - iou
    dI, dS = torch.autograd.grad(loss, (Ig, Sg))
    grad = torch.empty((n, C), dtype=torch.float64, device=dev)
    for r0, r1 in _chunks(n):
        if r1 == r0:
            continue
        x, valid, onehot, tw = _rows(logits, target, ignore, r0, r1, C, t_on, t_off)
        x.requires_grad_(True)
        p = torch.softmax(x, dim=1) * valid.unsqueeze(1)
        surrogate = (dI * (p * tw).sum(0)).sum() + (dS * (p * p if powerize else p).sum(0)).sum()
        grad[r0:r1] = torch.autograd.grad(surrogate, x)[0] * gout
    den = float(pres.sum()) + 1e-12
    uni = uni.detach()
    return SimpleNamespace(loss=loss.detach(), grad=grad, I=I, S=S, T=T, cnt=cnt, pres=pres, iou=float(iou.detach()),
                           M=M, n=n, C=C, soft=soft, powerize=powerize, neg_range=neg_range, gout=gout, t_on=t_on, t_off=t_off,
                           ignore=ignore, a=-2.0 * pres / den / uni, b=2.0 * pres / den * I / uni ** 2)


def errors(r):
    """the relative bars of the softmax, the targets and the class sums (module docstring)"""
    e_p = (2 * r.M + r.C + 5) * U
    e_t = 3 * U if r.soft else 0.0
    rr = rows_per_thread(r.n)
    e_I = e_p + e_t + (rr + 1) * U
    e_S = (2 * e_p + U if r.powerize else e_p) + rr * U
    e_T = e_t + rr * U
    return dict(e_p=e_p, e_t=e_t, e_I=e_I, e_S=e_S, e_T=e_T, e_U=max(e_S, e_T), r=rr)


def loss_bound(r):
    e = errors(r)
    loss = float(r.loss)
    return 1.01 * ((e["e_I"] + e["e_U"]) * abs(r.iou) + U * abs(1 - r.iou) + (U * abs(loss) if r.neg_range else 0.0))


def grad_bound(r, logits, target):
    """elementwise bound [n, C] of |glogits - grad|, in chunks of rows like dice64"""
    e = errors(r)
    e_p, e_t, e_I, e_U = e["e_p"], e["e_t"], e["e_I"], e["e_U"]
    e_a, e_b = e_U + U, e_I + 2 * e_U + U
    e_q = e_p if r.powerize else 0.0
    go = abs(r.gout)
    out = torch.empty((r.n, r.C), dtype=torch.float64, device=logits.device)
    for r0, r1 in _chunks(r.n):
        if r1 == r0:
            continue
        x, valid, onehot, tw = _rows(logits, target, r.ignore, r0, r1, r.C, r.t_on, r.t_off)
        p = torch.softmax(x, dim=1)
        q = 2 * p if r.powerize else torch.ones_like(p)
        at, bq = (r.a * tw).abs(), (r.b * q).abs()
        gp = r.a * tw + r.b * q
        dgp = at * (e_a + e_t + 2 * U) + bq * (e_b + e_q + 2 * U)
        pg = (p * gp).abs()
        dot = (p * gp).sum(1, keepdim=True)
        ddot = (pg * (e_p + U) + p * dgp).sum(1, keepdim=True) + r.C * U * pg.sum(1, keepdim=True)
        dp = e_p * p + TINY
        b = go * (dp * (gp - dot).abs() + p * (dgp + ddot) + 3 * U * p * (gp.abs() + dot.abs())) + TINY
        out[r0:r1] = 1.01 * b * valid.unsqueeze(1)
    return out


def grad_ratio(got, r, bound):
    """max |got - grad| / bound; an element whose bound is 0 (an ignored row) must be exactly 0"""
    err = (got.double() - r.grad).abs()
    ratio = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                        torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    if not bool(torch.isfinite(got).all()):
        return math.nan
    return float(ratio.max()) if ratio.numel() else 0.0
