"""Float64 yardstick of the Lovasz-softmax loss (lidog_amd.losses.LovaszSoftmaxLoss, csrc/lovasz.hip), in numpy, written
from the definition and independent of every lidog_* entry point.

  A row is valid when its label is not the ignore label and lies in [0, C); m = the valid rows; p = softmax(logits).
  For a class c that a valid row carries (P of them), over the valid rows:
    fg_i = [t_i == c],  e_i = |fg_i - p_ic|;  pi = descending e, ties by ascending row (a stable argsort of -e);
    G = sum fg,  cf_j = sum_{k <= j} fg_pi(k)                                               (integers)
    J(0, .) = 0,  J(j, cf) = 1.0 - float64(G - cf) / float64(G + j - cf)                    (j = 1 .. m)
    g_j = J(j, cf_j) - J(j - 1, cf_j - fg_pi(j)),   loss_c = sum_j e_pi(j) g_j
  loss = sum_c loss_c / P (0 when P = 0).  g is a constant of the gradient, as in the published implementation:
    dL/dp_ic = g_{pi^-1(i)} sign(p_ic - fg_i) / P  (sign(0) = 0; 0 in the invalid rows and the absent classes),
    dL/dx_i = p_i (q_i - <q_i, p_i>) with q = dL/dp, times the upstream gradient `gout`.

  full64            everything from the logits in float64.
  from_errors       the stages behind the sort, from GIVEN errors [C, n] (the kernel's own float32 err_out): g, coef =
                    float32(g) sign and 1 / P with the kernel's bits (g is integers, one division and two subtractions in
                    float64, so numpy has the same bits given the same order, and the same float32 errors with the same
                    tie rule give the same order), and the float64 dot of those errors with g.
  jacobian64        the backward pass in float64 from GIVEN coef and 1 / P.

Bars, from the kernels' fp32 operation sequence (u = 2^-24, first order, each times FACTOR = 1.01; dice_ref's softmax bar):
  p      d = x - max rounds (|d| u), expf is within 1 ulp (2u), the row sum (largest term exp(0) = 1) adds (C - 1) u, the
         reciprocal and the product 2u:  e_p(i) = (2 M_i + C + 5) u relative, M_i = max_c |x_ic - max_row|; below the normal
         range the error is absolute, TINY.
  e      fg = 0: e = |0 - p| = p exactly, so the error of p; fg = 1: e = fl(1 - p), the absolute error of p and one
         rounding of the difference:   E_e(i, c) = e_p(i) p_ic + u e_ic + TINY                        (absolute)
  loss   the Lovasz extension of the Jaccard loss is monotone and adding delta to every error adds at most delta
         (sum_j g_j = J(m) <= 1), so |d loss_c| <= max_i E_e(i, c) whatever the order does, and the mean over the
         present classes keeps max_{i,c} E_e; the float32 result adds u |loss|.
  sum    loss against the float64 dot of the SAME errors: K = m P products and additions in float64 in some order,
         (K + 2) 2^-53 sum |e g| / P, and u |loss| for the float32 result.
  bwd    q = fl(coef invP): u |q|;  dot = sum_c p_c q_c in class order: E_dot = (e_p + 2u + (C - 1) u) sum_c |p_c q_c| +
         C TINY;  D = fl(q_c - dot): u |q_c| + E_dot + u |D|;  glogits = (gout p_c) D: (e_p + 2u) |gout p_c D| +
         |gout| p_c (u |q_c| + E_dot + u |D|) + |gout| TINY |D| + TINY."""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -126
FACTOR = 1.01


def valid_rows(target, C, ignore):
    t = np.asarray(target).astype(np.int64)
    ok = (t >= 0) & (t < C)
    return ok & (t != ignore) if ignore is not None else ok


def softmax64(logits):
    x = np.asarray(logits, dtype=np.float64)
    z = np.exp(x - x.max(axis=1, keepdims=True)) if x.shape[0] else x
    return z / z.sum(axis=1, keepdims=True) if x.shape[0] else z


def errors64(logits, target, ignore):
    """(e [C, n] float64 with 0 in the invalid rows, p [n, C] float64, valid [n])"""
    n, C = logits.shape
    t = np.asarray(target).astype(np.int64)
    ok = valid_rows(t, C, ignore)
    p = softmax64(logits)
    fg = (t[None, :] == np.arange(C)[:, None]) & ok[None, :]
    return np.where(ok[None, :], np.abs(fg.astype(np.float64) - p.T), 0.0), p, ok


def lovasz_g(fg_sorted):
    """g_j of the definition for the 0 / 1 integers fg in sorted order (float64 [m])"""
    fg_sorted = fg_sorted.astype(np.int64)
    m, G = fg_sorted.shape[0], int(fg_sorted.sum())
    j = np.arange(1, m + 1, dtype=np.int64)
    cf = np.cumsum(fg_sorted)
    cf0 = cf - fg_sorted
    j1 = 1.0 - (G - cf).astype(np.float64) / (G + j - cf).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        jp = 1.0 - (G - cf0).astype(np.float64) / (G + (j - 1) - cf0).astype(np.float64)
    jp[:1] = 0.0
    return j1 - jp


def order_of(e_valid):
    """descending e, ties by ascending index"""
    return np.argsort(-e_valid, kind="stable")


def from_errors(err, target, ignore):
    """`err` [C, n] (any float dtype; sorted on as it is).  -> dict: g [n, C] float64 (per row, 0 where coef is), coef
    [n, C] float32, inv_p float32, present [C] bool, loss (float64), abs_sum (sum |e g| / P, for the sum bar), m"""
    C, n = err.shape
    t = np.asarray(target).astype(np.int64)
    ok = valid_rows(t, C, ignore)
    rows = np.nonzero(ok)[0]
    g = np.zeros((n, C), dtype=np.float64)
    coef = np.zeros((n, C), dtype=np.float32)
    present = np.zeros(C, dtype=bool)
    total = 0.0
    for c in range(C):
        fg = (t[rows] == c)
        if not fg.any():
            continue
        present[c] = True
        e = err[c, rows]
        pi = order_of(e)
        gs = lovasz_g(fg[pi])
        g[rows[pi], c] = gs
        es = e[pi]
        gf = gs.astype(np.float32)
        coef[rows[pi], c] = np.where(es == 0, np.float32(0), np.where(fg[pi], -gf, gf))
        total += float(np.sum(es.astype(np.float64) * gs))
    P = int(present.sum())
    inv_p = np.float32(1.0 / P) if P else np.float32(0)
    return dict(g=g, coef=coef, inv_p=inv_p, present=present, P=P, loss=total / P if P else 0.0,
                abs_sum=total / P if P else 0.0, m=int(ok.sum()))


def jacobian64(logits, target, coef, inv_p, ignore, gout=1.0):
    """glogits [n, C] float64 of the backward pass for GIVEN coef [n, C] and 1 / P; -> (grad, bound)"""
    n, C = logits.shape
    ok = valid_rows(target, C, ignore)
    x = np.asarray(logits, dtype=np.float64)
    p = softmax64(logits)
    q = np.asarray(coef, dtype=np.float64).reshape(n, C) * float(inv_p)
    dot = (p * q).sum(axis=1, keepdims=True)
    D = q - dot
    grad = gout * p * D * ok[:, None]
    M = (x.max(axis=1, keepdims=True) - x.min(axis=1, keepdims=True)) if n else np.zeros((0, 1))
    e_p = (2 * M + C + 5) * U
    go = abs(gout)
    e_dot = (e_p + 2 * U + (C - 1) * U) * np.abs(p * q).sum(axis=1, keepdims=True) + C * TINY
    e_D = U * np.abs(q) + e_dot + U * np.abs(D)
    bound = FACTOR * ((e_p + 2 * U) * np.abs(go * p * D) + go * p * e_D + go * TINY * np.abs(D) + TINY) * ok[:, None]
    return grad, bound


def error_bars(logits, target, ignore, factor=FACTOR):
    """E_e [C, n]: how far the kernel's float32 errors may be from errors64's; 0 in the invalid rows"""
    n, C = logits.shape
    e, p, ok = errors64(logits, target, ignore)
    x = np.asarray(logits, dtype=np.float64)
    M = (x.max(axis=1) - x.min(axis=1)) if n else np.zeros(0)
    e_p = (2 * M + C + 5) * U
    return factor * (e_p[None, :] * p.T + U * e + TINY) * ok[None, :]


def full64(logits, target, ignore, gout=1.0):
    """-> dict: loss, grad [n, C] (times gout), e [C, n], g [n, C], P, m, present"""
    n, C = logits.shape
    e, p, ok = errors64(logits, target, ignore)
    r = from_errors(e, target, ignore)
    t = np.asarray(target).astype(np.int64)
    fg = ((t[:, None] == np.arange(C)[None, :]) & ok[:, None]).astype(np.float64)
    q = r["g"] * np.sign(p - fg) / r["P"] if r["P"] else np.zeros((n, C))
    q = q * ok[:, None]
    grad = gout * p * (q - (p * q).sum(axis=1, keepdims=True))
    return dict(loss=r["loss"], grad=grad, e=e, g=r["g"], P=r["P"], m=r["m"], present=r["present"], p=p, valid=ok)


def loss_bound_errors(logits, target, ignore, loss):
    """|kernel loss - full64 loss| <= this: max E_e and the float32 rounding of the result"""
    bars = error_bars(logits, target, ignore)
    return (float(bars.max()) if bars.size else 0.0) + FACTOR * U * abs(loss)


def loss_bound_sum(r):
    """|kernel loss - from_errors(err_out) loss| <= this (`r`: what from_errors returned)"""
    return FACTOR * ((r["m"] * max(r["P"], 1) + 2) * U64 * r["abs_sum"] + U * abs(r["loss"]))


def separated(logits, target, ignore, factor=4.0):
    """the smallest gap between two neighbouring sorted float64 errors of a present class over the sum of their bars
    (`factor` times first order): > 1 means the float32 errors sort the same way, so the kernel's g is full64's"""
    n, C = logits.shape
    e, _, ok = errors64(logits, target, ignore)
    bars = error_bars(logits, target, ignore, factor)
    rows = np.nonzero(ok)[0]
    t = np.asarray(target).astype(np.int64)
    worst = np.inf
    for c in range(C):
        if not (t[rows] == c).any() or rows.size < 2:
            continue
        ec, bc = e[c, rows], bars[c, rows]
        pi = order_of(ec)
        gap = ec[pi][:-1] - ec[pi][1:]
        need = bc[pi][:-1] + bc[pi][1:]
        worst = min(worst, float((gap / need).min()))
    return worst
