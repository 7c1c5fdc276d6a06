"""The calibration arithmetic of include/lidog_amd.h (csrc/calib.hip) restated in numpy: lidog_calib_stats and
lidog_calib_fit_step with its update rule, in float64, and the same row formulas in np.longdouble (on x86-64 an 80-bit
format, eps 1.08e-19) as the yardstick both the kernel's and the float64 restatement's rounding are measured against.
Where a machine's long double is no wider than double (LD_IS_WIDER false) the sums that matter are taken with math.fsum
over the float64 terms instead: exact summation of the float64 rows, which still measures the summation error."""
import math

import numpy as np

Q = 4294967296.0
LD = np.longdouble
LD_IS_WIDER = np.finfo(LD).eps < np.finfo(np.float64).eps
STATE = ("beta", "lo", "hi", "nll", "g", "h", "iterations", "rows")


def labelled(labels, C, ignore_label=-1):
    labels = np.asarray(labels)
    return (labels >= 0) & (labels < C) & (labels != ignore_label)


def taking(x, labels, ignore_label=-1):
    """(rows that take part, labelled rows left out for a NaN or infinite logit)"""
    lab = labelled(labels, x.shape[1], ignore_label)
    finite = np.isfinite(x).all(axis=1)
    return lab & finite, lab & ~finite


def rows(x, labels, beta=1.0, dtype=np.float64):
    """per-row (conf, nll, brier, pred) of rows that all take part, in `dtype`; sums over classes in class order"""
    n, C = x.shape
    xd = x.astype(dtype)
    m = x.max(axis=1).astype(dtype) if n else np.zeros(0, dtype=dtype)
    z = dtype(beta) * (xd - m[:, None])
    e = np.exp(z)
    s = np.zeros(n, dtype=dtype)
    for c in range(C):
        s = s + e[:, c]
    idx = np.arange(n)
    brier = np.zeros(n, dtype=dtype)
    for c in range(C):
        d = e[:, c] / s - (labels == c).astype(dtype)
        brier = brier + d * d
    conf = dtype(1) / s
    nll = np.log(s) - z[idx, labels]
    pred = x.argmax(axis=1) if n else np.zeros(0, dtype=np.int64)           # the first maximal class
    return conf, nll, brier, pred


def stats(x, labels, beta=1.0, n_bins=15, ignore_label=-1):
    """lidog_calib_stats over one batch into fresh accumulators.  dict: table [B, 3] int64, totals [2] int64, nll_sum
    (float64, rows added in row order), nll_exact (the long-double sum of the long-double rows, or math.fsum of the
    float64 rows), err (0 or 2), conf (float64, per row that takes part), take"""
    x = np.asarray(x, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    take, bad = taking(x, labels, ignore_label)
    xt, lt = x[take], labels[take]
    conf, nll, brier, pred = rows(xt, lt, beta)
    B = int(n_bins)
    bins = np.minimum(B - 1, np.floor(conf * B).astype(np.int64))
    table = np.zeros((B, 3), dtype=np.int64)
    np.add.at(table[:, 0], bins, 1)
    np.add.at(table[:, 1], bins, (pred == lt).astype(np.int64))
    np.add.at(table[:, 2], bins, np.rint(conf * Q).astype(np.int64))
    totals = np.array([take.sum(), np.rint(brier * Q).astype(np.int64).sum()], dtype=np.int64)
    nll_sum = float(np.cumsum(nll)[-1]) if nll.size else 0.0                # sequential, in row order
    if LD_IS_WIDER:
        nll_exact = rows(xt, lt, beta, LD)[1].sum(dtype=LD) if nll.size else LD(0)
    else:
        nll_exact = LD(math.fsum(nll))
    return dict(table=table, totals=totals, nll_sum=nll_sum, nll_exact=nll_exact, err=2 if bad.any() else 0, conf=conf,
                take=take, bins=bins)


def edge_distance(conf, n_bins):
    """the smallest distance of a confidence to an interior bin edge k / B (inf when there is none)"""
    if n_bins < 2 or conf.size == 0:
        return math.inf
    t = conf * n_bins
    d = np.abs(t - np.rint(t)) / n_bins
    k = np.rint(t)
    return float(np.min(np.where((k >= 1) & (k <= n_bins - 1), d, np.inf)))


# ------------------------------------------------------------------ the temperature fit
def fit_sums(x, labels, beta, dtype=np.float64, ignore_label=-1):
    """(nll, g, h, N) of lidog_calib_fit_step at `beta`: means over the rows that take part (zeros when N == 0)"""
    x = np.asarray(x, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    take, _ = taking(x, labels, ignore_label)
    xt, lt = x[take], labels[take]
    n, C = xt.shape
    if n == 0:
        return dtype(0), dtype(0), dtype(0), 0
    z = xt.astype(dtype) - xt.max(axis=1).astype(dtype)[:, None]
    e = np.exp(dtype(beta) * z)
    s = np.zeros(n, dtype=dtype)
    ez = np.zeros(n, dtype=dtype)
    for c in range(C):
        s = s + e[:, c]
        ez = ez + e[:, c] * z[:, c]
    mean = ez / s
    var = np.zeros(n, dtype=dtype)
    for c in range(C):
        d = z[:, c] - mean
        var = var + e[:, c] * (d * d)
    zl = z[np.arange(n), lt]
    L = (np.log(s) - dtype(beta) * zl).sum(dtype=dtype)
    G = (mean - zl).sum(dtype=dtype)
    H = (var / s).sum(dtype=dtype)
    return L / n, G / n, H / n, n


def fit_update(state, nll, g, h, n, beta_min, beta_max):
    """the header's bracketed Newton update of state (a dict over STATE), in float64; returns the trace row"""
    beta, lo, hi = state["beta"], state["lo"], state["hi"]
    nxt = beta
    if n > 0:
        if g > 0:
            hi = beta
        elif g < 0:
            lo = beta
        else:
            lo = hi = beta
        if h > 0:
            cand = beta - g / h
        else:
            cand = -math.inf if g > 0 else math.inf if g < 0 else beta
        if cand == beta:
            nxt = beta
        elif lo < cand < hi:
            nxt = cand
        elif g < 0 and cand >= hi and hi == beta_max and beta != beta_max:
            nxt = beta_max
        elif g > 0 and cand <= lo and lo == beta_min and beta != beta_min:
            nxt = beta_min
        else:
            nxt = lo + (hi - lo) * 0.5
        nxt = min(max(nxt, beta_min), beta_max)
    else:
        nll = g = h = 0.0
    state.update(beta=nxt, lo=lo, hi=hi, nll=float(nll), g=float(g), h=float(h), iterations=state["iterations"] + 1.0,
                 rows=float(n))
    return beta, float(nll), float(g)


def fit(x, labels, iters=24, beta_min=0.01, beta_max=100.0, ignore_label=-1):
    """`iters` launches of lidog_calib_fit_step after lidog_calib_fit_init, in float64: (state dict, trace [iters, 3])"""
    state = dict(beta=min(max(1.0, beta_min), beta_max), lo=beta_min, hi=beta_max, nll=0.0, g=0.0, h=0.0,
                 iterations=0.0, rows=0.0)
    trace = np.zeros((iters, 3))
    for i in range(iters):
        nll, g, h, n = fit_sums(x, labels, state["beta"], np.float64, ignore_label)
        trace[i] = fit_update(state, float(nll), float(g), float(h), n, beta_min, beta_max)
    return state, trace


def fit_root(x, labels, start, beta_min=0.01, beta_max=100.0, ignore_label=-1, steps=2):
    """the minimiser of the NLL over [beta_min, beta_max] in long double: the bound where the gradient keeps its sign,
    else `steps` Newton steps from `start` (a float64 iterate that has converged to float64 precision: every step squares
    the error), kept inside the interval.  None when no row takes part."""
    if not taking(np.asarray(x, dtype=np.float32), np.asarray(labels, dtype=np.int64), ignore_label)[0].any():
        return None
    if fit_sums(x, labels, beta_max, LD, ignore_label)[1] <= 0:
        return LD(beta_max)
    if fit_sums(x, labels, beta_min, LD, ignore_label)[1] >= 0:
        return LD(beta_min)
    b = LD(start)
    for _ in range(steps):
        _, g, h, _ = fit_sums(x, labels, b, LD, ignore_label)
        if not h > 0:
            break
        b = min(max(b - g / h, LD(beta_min)), LD(beta_max))
    return b
