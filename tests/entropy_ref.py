"""float64 numpy restatement of the entropy criterion's definition (include/lidog_amd.h, lidog_entropy_fwd / _bwd):
per row  m = max x, s = sum exp(x - m), lse = m + log s, p = exp(x - lse), H = lse - sum p x  (evaluated on the shifted
logits: lse - x_c = log s - (x_c - m), which is the same number and loses nothing to |m|);  row_h = float32(H);
a row takes part when (mask is None or mask[r] != 0) and (margin <= 0 or row_h[r] < margin), on float32 values;
loss = sum of H over those rows / k;  coef = (float32(1 / k), float32(k)), (0, 0) when k == 0;
glogits[r][j] = gout * coef[0] * p_j * ((lse - x_j) - H) in the rows that take part, 0 elsewhere."""
import numpy as np


def rows64(x):
    """(H [n], p [n, C], lse - x [n, C]) in float64 of float32 logits [n, C]"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    z = x - x.max(axis=1, keepdims=True)
    e = np.exp(z)
    s = e.sum(axis=1, keepdims=True)
    logs = np.log(s)
    p = e / s
    H = logs[:, 0] - (p * z).sum(axis=1)
    return H, p, logs - z


def taking(H, mask=None, margin=0.0):
    """bool [n]: participation, decided on np.float32(H) against np.float32(margin)"""
    h32 = np.asarray(H, dtype=np.float64).astype(np.float32)
    take = np.ones(h32.shape[0], dtype=bool) if mask is None else np.asarray(mask) != 0
    margin = np.float32(0.0 if margin is None else margin)
    if margin > 0:
        take = take & (h32 < margin)
    return take


def entropy64(x, mask=None, margin=0.0, gout=1.0):
    """dict: loss (float64), row_h (float64 [n], every row), take (bool [n]), k, coef (float32 [2]), grad (float64
    [n, C], with coef[0] the float32 value the kernel stores and gout as float32)"""
    H, p, lse_x = rows64(x)
    take = taking(H, mask, margin)
    k = int(take.sum())
    coef = np.array([1.0 / k if k else 0.0, k], dtype=np.float64).astype(np.float32)
    loss = float(H[take].sum() / k) if k else 0.0
    grad = np.float64(np.float32(gout)) * np.float64(coef[0]) * p * (lse_x - H[:, None])
    grad[~take] = 0.0
    return {"loss": loss, "row_h": H, "take": take, "k": k, "coef": coef, "grad": grad}


def margin_gap(x, margin):
    """the least |H - margin| over all rows (inf without rows): the tests choose inputs for which it exceeds 1e-3, so
    that float32 and float64 agree on every row's side of the margin"""
    H, _, _ = rows64(x)
    return float(np.abs(H - np.float64(np.float32(margin))).min()) if H.shape[0] else float("inf")
