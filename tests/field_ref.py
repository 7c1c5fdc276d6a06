"""Float64 yardstick of the point <-> voxel family -- the floor of a field's coordinates, the per-voxel lists, the
ordered segment sum / mean, the gather, trilinear interpolation and its gradient -- written from the formulas of
include/lidog_amd.h alone: numpy and plain torch on the CPU, no code of the package under test.
tests/test_field_cpu.py pins it to hand-computed cases; tests/test_gpu_field.py holds csrc/field.hip to it.

  floor    rows (batch, floor(v / s) * s) in float32; NaN, an infinity or a value no int32 holds gives INT32_MIN;
           error bits: 1 a batch column that is no integer in 0 .. 4095 (the row gets batch -1), 2 a non-finite coordinate
  lists    the entries j of an index table that name row v, ascending j (a stable counting sort); entries outside
           [0, m) are in no list
  reduce   y[v] = x[l0] + x[l1] + ... in list order, mean: / count; an empty list gives 0
  gather   y[p] = x[inv[p]] (/ count of that row)
  interp   per axis lo = floor(x / s) * s, t = (x - lo) / s; neighbour k = bx + 2 by + 4 bz at lo + bit * s, weight
           f_x * f_y * f_z with factor 1 - t (lower) or t (upper), the fraction taken from the lattice point on the side
           of zero (x < 0: r = ((lo + s) - x) / s, factors r and 1 - r); y[q] = sum over the neighbours that exist of
           w_k F[row_k]; no renormalisation; a neighbour in another batch index never counts
  interp gradient   gF[i] = sum over the (k, q) that hit row i of w_k(q) gy[q]

Bounds (derived, nothing measured; u = 2^-24, gamma_n = n u / (1 - n u), Higham 3.1):
  * interpolation with a power-of-two stride: x / s, the floor, lo and the division by s are EXACT; so is x - lo for
    x >= 0 (a float32 minus its own floor has no more significant bits than x) and (lo + s) - x for x < 0 (the mirror
    image).  The OTHER distance is not (-0.3 - (-1) needs two more bits than -0.3 has; -4e-14 - (-1) is 1 in float32 and
    in float64), which is why the contract takes the fraction from the side of zero; the yardstick does the same, in
    float64, so its fraction is the exact one and only its 1 - fraction rounds (2^-53 absolute on a value >= 2^-24: a
    relative 2^-29 per factor, added to the bound as 3 * 2^-29).  A weight is up to three factors 1 - t (one rounding
    each) and two products: at most 5 roundings.  The
    sum is a chain of fmaf from 0 over the cnt neighbours that exist: a term goes through at most cnt more roundings.
    |computed - exact| <= gamma_(5 + cnt) sum |w_k| |F_k|.  The gradient is the same chain over the list of a row (cnt =
    its length).  (Underflow is left out: the tests' values are far from it.)
  * ordered sum of cnt terms from the first element: cnt - 1 roundings, gamma_(cnt - 1) sum |x|; the mean adds one
    correctly rounded division: sum bound / cnt * (1 + u) + u |ref|.
  * gather: a copy, exact; with the division one rounding: u |ref|."""
import numpy as np
import torch

U = 2.0 ** -24
INT32_MIN = -2 ** 31
ERR_BATCH, ERR_NONFINITE = 1, 2


def gamma(n):
    n = torch.as_tensor(n, dtype=torch.float64)
    return n * U / (1 - n * U)


def _f64(x):
    return torch.as_tensor(x).detach().double().cpu()


# ------------------------------------------------------------------ floor
def floor_rows(points, s):
    """(rows int64 [N, 4], error word) of float32 points [N, 4] (batch, x, y, z) under tensor stride s"""
    p = np.asarray(torch.as_tensor(points).detach().cpu().numpy(), dtype=np.float32).reshape(-1, 4)
    s32 = np.float32(s)
    rows = np.empty(p.shape, dtype=np.int64)
    err = 0
    with np.errstate(invalid="ignore", over="ignore"):
        b = p[:, 0]
        good = (b >= 0) & (b <= 4095) & (np.floor(b) == b)
        rows[:, 0] = np.where(good, np.where(good, b, 0).astype(np.int64), -1)
        if not good.all():
            err |= ERR_BATCH
        if not np.isfinite(p[:, 1:]).all():
            err |= ERR_NONFINITE
        f = (np.floor(p[:, 1:] / s32) * s32).astype(np.float32)
        ok = np.isfinite(f) & (f >= -2.0 ** 31) & (f < 2.0 ** 31)
        rows[:, 1:] = np.where(ok, np.where(ok, f, 0).astype(np.int64), INT32_MIN)
    return rows, err


# ------------------------------------------------------------------ lists, reduce, gather
def lists(inv, m):
    """(row_ptr int64 [m + 1], row_list int64 [row_ptr[m]]): the entries of `inv` that name row v, ascending"""
    inv = np.asarray(torch.as_tensor(inv).cpu().numpy(), dtype=np.int64).ravel()
    named = np.nonzero((inv >= 0) & (inv < m))[0]
    order = named[np.argsort(inv[named], kind="stable")]
    row_ptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(inv[named], minlength=m), out=row_ptr[1:])
    return row_ptr, order


def reduce64(x, inv, m, mean):
    """float64 [m, C]: per-voxel sum (mean: / count) of the point rows; an empty voxel gives zeros"""
    x = _f64(x)
    inv = torch.as_tensor(np.asarray(inv), dtype=torch.long)
    y = torch.zeros((m, x.shape[1]), dtype=torch.float64).index_add_(0, inv, x)
    if mean:
        cnt = torch.bincount(inv, minlength=m).double().unsqueeze(1)
        y = torch.where(cnt > 0, y / cnt.clamp(min=1), torch.zeros((), dtype=torch.float64))
    return y


def gather64(x, inv, m=None, mean=False):
    """float64 [N, C]: x[inv[p]], mean: divided by the number of entries of `inv` that name the same row"""
    x = _f64(x)
    inv = torch.as_tensor(np.asarray(inv), dtype=torch.long)
    y = x[inv]
    if mean:
        cnt = torch.bincount(inv, minlength=x.shape[0] if m is None else m).double()
        y = y / cnt[inv].unsqueeze(1)
    return y


def reduce_bound(x, inv, m, mean):
    inv_t = torch.as_tensor(np.asarray(inv), dtype=torch.long)
    cnt = torch.bincount(inv_t, minlength=m).double().unsqueeze(1)
    s = gamma((cnt - 1).clamp(min=0)) * reduce64(_f64(x).abs(), inv, m, False)
    if not mean:
        return s
    return s / cnt.clamp(min=1) * (1 + U) + U * reduce64(x, inv, m, True).abs()


def gather_bound(x, inv, m=None, mean=False):
    ref = gather64(x, inv, m, mean)
    return U * ref.abs() if mean else torch.zeros_like(ref)


# ------------------------------------------------------------------ interpolation
def neighbours(coords, query, s):
    """(nbr int64 [8, Q], w float64 [8, Q]) of float32 queries [Q, 4] on a map `coords` [M, 4] of tensor stride s: the
    row holding neighbour k = bx + 2 by + 4 bz or -1, and the weight of that neighbour (also where it is missing)"""
    coords = np.asarray(torch.as_tensor(coords).cpu().numpy(), dtype=np.int64)
    q32 = np.asarray(torch.as_tensor(query).detach().cpu().numpy(), dtype=np.float32).reshape(-1, 4)
    q = q32.astype(np.float64)
    table = {}
    for i, row in enumerate(coords.tolist()):
        assert tuple(row) not in table, "duplicate map coordinate"
        table[tuple(row)] = i
    with np.errstate(invalid="ignore", over="ignore"):
        x = q[:, 1:]
        lo = np.floor(x / s) * s
        pos = x >= 0
        frac = np.where(pos, x - lo, (lo + s) - x) / s          # exact: the distance on the side of zero
        lower, upper = np.where(pos, 1 - frac, frac), np.where(pos, frac, 1 - frac)
    Q = q.shape[0]
    nbr = np.full((8, Q), -1, dtype=np.int64)
    w = np.zeros((8, Q), dtype=np.float64)
    finite = np.isfinite(q).all(axis=1)
    for k in range(8):
        bit = np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1])
        f = np.where(bit == 1, upper, lower)
        w[k] = f[:, 0] * f[:, 1] * f[:, 2]
        for j in np.nonzero(finite)[0]:
            b = q[j, 0]
            if b != np.floor(b):
                continue
            key = (int(b),) + tuple(int(v) for v in (lo[j] + bit * s))
            nbr[k, j] = table.get(key, -1)
    return nbr, w


def interp64(F, nbr, w):
    """float64 [Q, C]: sum over the neighbours that exist of w_k F[nbr_k]"""
    F = _f64(F)
    Q = nbr.shape[1]
    y = torch.zeros((Q, F.shape[1]), dtype=torch.float64)
    for k in range(8):
        rows = torch.as_tensor(nbr[k], dtype=torch.long)
        have = torch.nonzero(rows >= 0).flatten()
        if have.numel():
            y[have] += torch.as_tensor(w[k])[have].unsqueeze(1) * F[rows[have]]
    return y


def interp_bwd64(gy, nbr, w, m):
    """float64 [m, C]: gF[i] = sum over the (k, q) with nbr[k][q] == i of w_k(q) gy[q]; rows nobody hits get 0"""
    gy = _f64(gy)
    gF = torch.zeros((m, gy.shape[1]), dtype=torch.float64)
    for k in range(8):
        rows = torch.as_tensor(nbr[k], dtype=torch.long)
        have = torch.nonzero(rows >= 0).flatten()
        if have.numel():
            gF.index_add_(0, rows[have], torch.as_tensor(w[k])[have].unsqueeze(1) * gy[have])
    return gF


def interp_bound(F, nbr, w):
    """gamma_(5 + cnt) sum |w_k| |F_k| (module docstring); a query without neighbours: 0, the row must be exact zeros"""
    cnt = torch.as_tensor((nbr >= 0).sum(axis=0), dtype=torch.float64).unsqueeze(1)
    mag = interp64(_f64(F).abs(), nbr, np.abs(w))
    return torch.where(cnt > 0, (gamma(5 + cnt) + 3 * 2.0 ** -29) * mag, torch.zeros((), dtype=torch.float64))


def interp_bwd_bound(gy, nbr, w, m):
    hit = nbr[nbr >= 0]
    cnt = torch.bincount(torch.as_tensor(hit, dtype=torch.long), minlength=m).double().unsqueeze(1)
    mag = interp_bwd64(_f64(gy).abs(), nbr, np.abs(w), m)
    return torch.where(cnt > 0, (gamma(5 + cnt) + 3 * 2.0 ** -29) * mag, torch.zeros((), dtype=torch.float64))


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
