"""Float64 yardstick of sparse pooling -- local sum / avg / max over a kernel region, their gradients, the transposed
(un)pooling and the per-scan global forms -- written from the formulas of include/lidog_amd.h and from the neighbour
sets of tests/sconv_ref.py alone: plain torch on the CPU, no code of the package under test.
tests/test_pool_cpu.py pins it to hand-computed cases; tests/test_gpu_pool.py holds csrc/pool.hip to it.

A neighbour table nbr [K, n_out] (sconv_ref.neighbours) lists, per offset k ascending, the input row of output row o or
-1.  The LIST of output row o is its entries >= 0 in ascending k: the order the kernels walk.

  sum   y[o] = sum over the list of x[i]
  avg   the same / |list| (the neighbours that exist, not the kernel volume); an empty list gives 0
  max   y[o][c] = max over the list, arg[o][c] = the input row of the FIRST maximum in list order (strict >, so a tie
        stays with the lowest offset); a NaN beats every number and the first NaN stays (torch.amax's value); an empty
        list gives 0 and arg = -1

Bounds (derived, nothing measured): a float32 sum of cnt terms in ANY order carries at most cnt - 1 roundings per term,
so |computed - exact| <= gamma_(cnt-1) sum|x_i| <= cnt u sum|x_i| (Higham 3.1, 4.2; u = 2^-24).  The average adds one
correctly rounded division: sum bound / cnt + u |ref|.  The gradient of the average divides every term before it adds
(one more rounding per term): (cnt + 1) u sum|term|.  max, its gradient and every copy are exact."""
import numpy as np
import torch

from sconv_ref import U, neighbours, scene_map, transpose_map  # noqa: F401  (re-exported for the tests)


def _f64(x):
    return torch.as_tensor(x).detach().double().cpu()


def _idx(nbr_k):
    return torch.as_tensor(np.asarray(nbr_k), dtype=torch.long)


def counts(nbr):
    """[n_out] list lengths"""
    return torch.as_tensor((np.asarray(nbr) >= 0).sum(axis=0), dtype=torch.float64)


def pool64(x, nbr, mode):
    """(y float64 [n_out, C], arg int64 [n_out, C] or None) of sum / avg / max pooling"""
    x = _f64(x)
    nbr = np.asarray(nbr)
    n_out, C = nbr.shape[1], x.shape[1]
    zero = torch.zeros((), dtype=torch.float64)
    if mode in ("sum", "avg"):
        y = torch.zeros((n_out, C), dtype=torch.float64)
        for k in range(nbr.shape[0]):
            i = _idx(nbr[k])
            o = torch.nonzero(i >= 0).flatten()     # only the rows that have this offset: nothing else is touched
            if o.numel():
                y[o] += x[i[o]]
        if mode == "avg":
            cnt = counts(nbr).unsqueeze(1)
            y = torch.where(cnt > 0, y / cnt.clamp(min=1), zero)
        return y, None
    assert mode == "max"
    best = torch.zeros((n_out, C), dtype=torch.float64)
    arg = torch.full((n_out, C), -1, dtype=torch.long)
    for k in range(nbr.shape[0]):
        i = _idx(nbr[k])
        o = torch.nonzero(i >= 0).flatten()
        if not o.numel():
            continue
        v, b, a = x[i[o]], best[o], arg[o]
        take = (a < 0) | (~torch.isnan(b) & ((v > b) | torch.isnan(v)))
        best[o] = torch.where(take, v, b)
        arg[o] = torch.where(take, i[o].unsqueeze(1).expand(-1, C), a)
    return best, arg


def pool_bwd64(gy, nbr, n_in, mode, arg=None):
    """gx float64 [n_in, C]: the gradient of pool64 in x for the output gradient gy [n_out, C].
    sum: gx[i] = sum of gy[o] over the lists that hold i; avg: of gy[o] / |list of o|; max: of gy[o][c] where
    arg[o][c] == i (a tied window reaches exactly one input)."""
    gy = _f64(gy)
    nbr = np.asarray(nbr)
    nbr_t = transpose_map(nbr, n_in)
    if mode == "sum":
        return pool64(gy, nbr_t, "sum")[0]
    if mode == "avg":
        cnt = counts(nbr).unsqueeze(1)
        return pool64(gy / cnt.clamp(min=1), nbr_t, "sum")[0]
    assert mode == "max" and arg is not None
    arg = torch.as_tensor(arg).long().cpu()
    gx = torch.zeros((n_in, gy.shape[1]), dtype=torch.float64)
    rows = torch.arange(n_in).unsqueeze(1)
    zero = torch.zeros((), dtype=torch.float64)
    for k in range(nbr_t.shape[0]):
        o = _idx(nbr_t[k])
        i = torch.nonzero(o >= 0).flatten()
        gx[i] += torch.where(arg[o[i]] == rows[i], gy[o[i]], zero)
    return gx


def unpool64(x, nbr, n_fine):
    """transposed pooling on the exchanged map: nbr [K, n_coarse] is the map fine -> coarse of the strided pooling;
    y[f] = the average of x[c] over the (k, c) with nbr[k][c] == f.  [n_fine, C]"""
    return pool64(x, transpose_map(nbr, n_fine), "avg")[0]


def global64(x, batch_ids, B, mode):
    """(y float64 [B, C], arg int64 [B, C] or None): one reduction per batch index over its rows in ascending row order;
    a batch index without rows gives zeros (arg -1)"""
    x = _f64(x)
    bid = torch.as_tensor(np.asarray(batch_ids), dtype=torch.long)
    C = x.shape[1]
    y = torch.zeros((B, C), dtype=torch.float64)
    arg = torch.full((B, C), -1, dtype=torch.long) if mode == "max" else None
    for b in range(B):
        rows = torch.nonzero(bid == b).flatten()
        if rows.numel() == 0:
            continue
        xb = x[rows]
        if mode == "sum":
            y[b] = xb.sum(0)
        elif mode == "avg":
            y[b] = xb.sum(0) / rows.numel()
        else:
            nan = torch.isnan(xb)
            has_nan = nan.any(0)
            top = torch.where(nan, torch.full_like(xb, -float("inf")), xb).max(0).values
            first_max = (xb == top).int().argmax(0)          # argmax of a 0/1 matrix: the first 1
            first_nan = nan.int().argmax(0)
            at = torch.where(has_nan, first_nan, first_max)
            arg[b] = rows[at]
            y[b] = xb.gather(0, at.unsqueeze(0))[0]
    return y, arg


def global_bwd64(gy, batch_ids, B, mode, arg=None):
    """gx float64 [n, C]: sum: gy[b(i)]; avg: gy[b(i)] / n_b; max: gy[b][c] where arg[b][c] == i else 0"""
    gy = _f64(gy)
    bid = torch.as_tensor(np.asarray(batch_ids), dtype=torch.long)
    g = gy[bid]
    if mode == "sum":
        return g
    if mode == "avg":
        n_b = torch.bincount(bid, minlength=B).double()
        return g / n_b[bid].unsqueeze(1)
    arg = torch.as_tensor(arg).long().cpu()
    rows = torch.arange(bid.numel()).unsqueeze(1)
    return torch.where(arg[bid] == rows, g, torch.zeros((), dtype=torch.float64))


# ------------------------------------------------------------------ bounds
def bound(x, nbr, mode):
    """per-element bound of any float32 evaluation of pool64 (see the module docstring); max is exact: zeros"""
    if mode == "max":
        return torch.zeros((np.asarray(nbr).shape[1], _f64(x).shape[1]), dtype=torch.float64)
    cnt = counts(nbr).unsqueeze(1)
    s = cnt * U * pool64(_f64(x).abs(), nbr, "sum")[0]
    if mode == "sum":
        return s
    return s / cnt.clamp(min=1) + U * pool64(x, nbr, "avg")[0].abs()


def bound_bwd(gy, nbr, n_in, mode):
    """the same for pool_bwd64: sum is a sum over the exchanged map; avg divides every term first (one more rounding
    per term): (cnt_in + 1) u sum |gy[o] / cnt_o|"""
    nbr_t = transpose_map(np.asarray(nbr), n_in)
    if mode == "sum":
        return bound(gy, nbr_t, "sum")
    assert mode == "avg"
    terms = _f64(gy).abs() / counts(nbr).unsqueeze(1).clamp(min=1)
    return (counts(nbr_t).unsqueeze(1) + 1) * U * pool64(terms, nbr_t, "sum")[0]


def global_bound(x, batch_ids, B, mode):
    """bound() with cnt = n_b, the rows of the scan"""
    if mode == "max":
        return torch.zeros((B, _f64(x).shape[1]), dtype=torch.float64)
    n_b = torch.bincount(torch.as_tensor(np.asarray(batch_ids), dtype=torch.long), minlength=B).double().unsqueeze(1)
    s = n_b * U * global64(_f64(x).abs(), batch_ids, B, "sum")[0]
    if mode == "sum":
        return s
    return s / n_b.clamp(min=1) + U * global64(x, batch_ids, B, "avg")[0].abs()


def global_bwd_bound(gy, batch_ids, B, mode):
    """sum and max copy (exact); avg is one correctly rounded division: u |ref|"""
    ref = global_bwd64(gy, batch_ids, B, "avg" if mode == "avg" else "sum")
    return U * ref.abs() if mode == "avg" else torch.zeros_like(ref)


def worst_ratio(got, ref64, bnd):
    """max |got - ref| / bound over the elements; an element with bound 0 must be equal.  inf for a non-finite `got`"""
    got = _f64(got)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref64).abs()
    if bool(((bnd == 0) & (err > 0)).any()):
        return float("inf")
    r = err[bnd > 0] / bnd[bnd > 0]
    return float(r.max()) if r.numel() else 0.0
