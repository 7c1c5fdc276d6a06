"""Float64 yardstick of the fused optimiser steps (csrc/optim.hip: k_adam / k_sgd behind lidog_adam_step /
lidog_sgd_step) and of the kernel transposes (csrc/sconv.hip), the forward error bounds a correct float32 implementation
is held to, and the data the tests share.  Plain array arithmetic: numpy float64 on the host; the same functions take
torch float64 tensors on any device (the model-size trajectory of tests/test_gpu_optim64.py).
tests/test_optim_ref_cpu.py checks the yardstick against torch.optim in float64, shows that float32 torch.optim and a
float32 numpy chain stay inside the bounds, and that nine wrong variants leave them.

Definitions (one step; every input is the float32 value the kernel reads, widened to double; every scalar is first
rounded to float32, which is what the C ABI receives: 1 - float32(0.999) differs from 0.001 by 1.3e-5 relative):
  g' = g s + wd p                                        (s = grad_scale, the 1 / world size of data-parallel runs)
  Adam   m' = m + (g' - m)(1 - b1),  v' = v b2 + (1 - b2) g'^2,
         p' = p - [lr / bc1] m' / (sqrt(v') / [sqrt(bc2)] + eps),   bc_i = 1 - b_i^step in double from the float32
         betas; the two bracketed factors are rounded to float32 as the entry point rounds them (`abi=False` keeps them
         in double: torch.optim on float64 tensors)
  SGD    buf' = mu buf + g',  p' = p - lr (g' + mu buf')  [nesterov]  |  p - lr buf'

Bounds (`adam_bounds`, `sgd_bounds`): first-order propagation of u = 2^-24 per float32 operation, charged on the
magnitude of that operation's result, along the chain above; derived next to each function, nothing measured.  The
whole is doubled for the order of operations (a lerp written the other way round, a fused multiply-add).  A bar of the
form u |v'| or u (|p| + |update|) is NOT a bound of a correct chain: g s + wd p cancels, and its error u (|g s| + |wd p|)
enters v' through 2 (1 - b2) |g'| and the update through m' and sqrt(v')."""
import functools

import numpy as np

try:
    import torch
except ImportError:   # pragma: no cover
    torch = None

U = 2.0 ** -24
TINY = 2.0 ** -126        # smallest normal float32


# ------------------------------------------------------------------ array plumbing (numpy or torch, same expressions)
def _ns(x):
    return torch if (torch is not None and isinstance(x, torch.Tensor)) else np


def _f64(x):
    if torch is not None and isinstance(x, torch.Tensor):
        return x.double()
    return np.asarray(x, dtype=np.float64)


def f32(s):
    """a python scalar as the C ABI passes it (c_float), widened back to double"""
    return float(np.float32(s))


def bias_corrections(lr, beta1, beta2, step, abi=True):
    """(lr / bc1, sqrt(bc2)) of lidog_adam_step: bc_i in double from the float32 betas, both results rounded to float32"""
    bc1 = 1.0 - f32(beta1) ** int(step)
    bc2 = 1.0 - f32(beta2) ** int(step)
    lr_bc1, bc2_sqrt = f32(lr) / bc1, float(np.sqrt(bc2))
    return (f32(lr_bc1), f32(bc2_sqrt)) if abi else (lr_bc1, bc2_sqrt)


# ------------------------------------------------------------------ Adam
def _adam_chain(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale, abi):
    xp = _ns(p)
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    b1, b2, eps, wd, s = f32(beta1), f32(beta2), f32(eps), f32(wd), f32(grad_scale)
    lr_bc1, bc2s = bias_corrections(lr, beta1, beta2, step, abi)
    c = dict(xp=xp, p=p, m=m, v=v, b1=b1, b2=b2, eps=eps, lr_bc1=lr_bc1, bc2s=bc2s)
    c["gs"], c["wp"] = g * s, wd * p
    c["g1"] = c["gs"] + c["wp"]
    c["d"] = c["g1"] - m
    c["t"] = c["d"] * (1.0 - b1)
    c["m1"] = m + c["t"]
    c["va"], c["vb"] = v * b2, (1.0 - b2) * c["g1"] * c["g1"]
    c["v1"] = c["va"] + c["vb"]
    c["sq"] = xp.sqrt(c["v1"])
    c["q"] = c["sq"] / bc2s
    c["den"] = c["q"] + eps
    c["r"] = c["m1"] / c["den"]
    c["w"] = lr_bc1 * c["r"]
    c["p1"] = p - c["w"]
    return c


def adam64(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, abi=True):
    """one torch.optim.Adam step (L2 decay in the gradient, bias-corrected) in float64 -> (p', m', v')"""
    c = _adam_chain(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale, abi)
    return c["p1"], c["m1"], c["v1"]


def _e_grad(c):
    """g' = fl(fl(g s) + fl(wd p)): one rounding on each product, one on the sum"""
    xp = c["xp"]
    return U * (xp.abs(c["gs"]) + xp.abs(c["wp"]) + xp.abs(c["g1"]))


def adam_bounds(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale=1.0):
    """(e_p, e_m, e_v): |float32 result - float64 yardstick| of a correct float32 Adam step, elementwise.
      e_g = u (|g s| + |wd p| + |g'|)
      m'  = fl(m + fl(fl(g' - m) fl(1 - b1))):   e_m = (1 - b1)(e_g + u |g' - m|) + 2u |t| + u |m'|,  t = (1 - b1)(g' - m)
      v'  = fl(fl(v b2) + fl(fl(fl(1 - b2) g') g')):   e_v = 2 (1 - b2) |g'| e_g + u v b2 + 3u (1 - b2) g'^2 + u v'
      sqrt  (correctly rounded):   e_s = min(e_v / (2 sqrt v'), sqrt(e_v)) + u sqrt v'
            (|sqrt a - sqrt b| <= sqrt |a - b| always; the first-order term alone is unbounded as v' -> 0)
      den = fl(fl(sqrt v' / bc2s) + eps):   e_den = e_s / bc2s + u q + u den
      r   = fl(m' / den~):   e_r = e_m / lo + |m'| e_den / (den lo) + u |r|,  lo = max(den - e_den, eps (1 - 2u)) (the
            computed denominator is never below eps, whatever v' carries)
      p'  = fl(p - fl(lr_bc1 r)):   e_p = lr_bc1 e_r + u |w| + u |p'|
    each doubled for operation order."""
    c = _adam_chain(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale, True)
    xp, ab = c["xp"], c["xp"].abs
    e_g = _e_grad(c)
    k1, k2 = 1.0 - c["b1"], 1.0 - c["b2"]
    e_m = k1 * (e_g + U * ab(c["d"])) + 2 * U * ab(c["t"]) + U * ab(c["m1"])
    e_v = 2 * k2 * ab(c["g1"]) * e_g + U * c["va"] + 3 * U * c["vb"] + U * c["v1"]
    sq_safe = xp.where(c["sq"] > 0, c["sq"], c["sq"] + 1.0)
    e_s = xp.where(c["sq"] > 0, xp.minimum(e_v / (2 * sq_safe), xp.sqrt(e_v)), xp.sqrt(e_v)) + U * c["sq"]
    e_den = e_s / c["bc2s"] + U * c["q"] + U * c["den"]
    floor = c["eps"] * (1 - 2 * U)
    lo = xp.where(c["den"] - e_den > floor, c["den"] - e_den, 0 * c["den"] + floor)
    e_r = e_m / lo + ab(c["m1"]) * e_den / (c["den"] * lo) + U * ab(c["r"])
    e_p = c["lr_bc1"] * e_r + U * ab(c["w"]) + U * ab(c["p1"])
    return 2 * e_p, 2 * e_m, 2 * e_v


def small_denominator_share(v1, beta2, step, eps):
    """share of elements with sqrt(v') / sqrt(bc2) < 100 eps: where eps decides the step, so its placement shows"""
    _, bc2s = bias_corrections(1.0, 0.5, beta2, step)
    x = np.sqrt(np.asarray(v1, dtype=np.float64)) / bc2s < 100 * f32(eps)
    return float(x.mean())


# ------------------------------------------------------------------ SGD
def _sgd_chain(p, g, buf, lr, mu, wd, nesterov, grad_scale):
    xp = _ns(p)
    p, g, buf = _f64(p), _f64(g), _f64(buf)
    lr, mu, wd, s = f32(lr), f32(mu), f32(wd), f32(grad_scale)
    c = dict(xp=xp, p=p, lr=lr, mu=mu, nesterov=bool(nesterov))
    c["gs"], c["wp"] = g * s, wd * p
    c["g1"] = c["gs"] + c["wp"]
    c["bm"] = buf * mu
    c["b1"] = c["bm"] + c["g1"]
    c["mb"] = mu * c["b1"]
    c["st"] = c["g1"] + c["mb"] if nesterov else c["b1"]
    c["w"] = lr * c["st"]
    c["p1"] = p - c["w"]
    return c


def sgd64(p, g, buf, lr, mu, wd, nesterov, grad_scale=1.0):
    """one torch.optim.SGD(dampening=0) step in float64 -> (p', buf'); buf = 0 is torch's first step (buf' = g')"""
    c = _sgd_chain(p, g, buf, lr, mu, wd, nesterov, grad_scale)
    return c["p1"], c["b1"]


def sgd_bounds(p, g, buf, lr, mu, wd, nesterov, grad_scale=1.0):
    """(e_p, e_buf) of a correct float32 SGD step, elementwise:
      buf' = fl(fl(buf mu) + g'):   e_b = e_g + u |buf mu| + u |buf'|
      step = fl(g' + fl(mu buf')):   e_st = e_g + mu e_b + u |mu buf'| + u |step|   [nesterov]   |   e_st = e_b
      p'   = fl(p - fl(lr step)):   e_p = lr e_st + u |lr step| + u |p'|
    each doubled for operation order."""
    c = _sgd_chain(p, g, buf, lr, mu, wd, nesterov, grad_scale)
    ab = c["xp"].abs
    e_g = _e_grad(c)
    e_b = e_g + U * ab(c["bm"]) + U * ab(c["b1"])
    e_st = e_g + c["mu"] * e_b + U * ab(c["mb"]) + U * ab(c["st"]) if c["nesterov"] else e_b
    e_p = c["lr"] * e_st + U * ab(c["w"]) + U * ab(c["p1"])
    return 2 * e_p, 2 * e_b


# ------------------------------------------------------------------ ratios
def worst_ratio(got, ref64, bound):
    """max |got - ref| / bound; an exact result under a zero bound counts 0, a wrong one inf, a non-finite output NaN
    (which fails every `<= 1`)"""
    xp = _ns(ref64)
    if int(np.prod(tuple(ref64.shape))) == 0:
        return 0.0
    got = _f64(got)
    if not bool(xp.isfinite(got).all()):
        return float("nan")
    err = xp.abs(got - ref64)
    one = 0 * bound + 1.0
    r = xp.where(bound > 0, err / xp.where(bound > 0, bound, one), xp.where(err > 0, one * float("inf"), 0 * one))
    return float(r.max())


def ratio_square_sum(got, ref64, bound):
    """(sum of (|got - ref| / bound)^2, count): the parts of a root-mean-square error / bound ratio, so that slices can be
    pooled; a zero bound counts 0 when met exactly and inf when not"""
    xp = _ns(ref64)
    n = int(np.prod(tuple(ref64.shape)))
    if n == 0:
        return 0.0, 0
    err = xp.abs(_f64(got) - ref64)
    one = 0 * bound + 1.0
    r = xp.where(bound > 0, err / xp.where(bound > 0, bound, one), xp.where(err > 0, one * float("inf"), 0 * one))
    return float((r * r).sum()), n


def rms_ratio(got, ref64, bound):
    sq, n = ratio_square_sum(got, ref64, bound)
    return float(np.sqrt(sq / max(n, 1)))


def outside_share(got, ref64, bound):
    """share of elements outside their bound (numpy)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref64)
    return float((~(err <= bound)).mean())


# ------------------------------------------------------------------ transposes
def transpose64(W):
    """[..., Cin, Cout] -> [..., Cout, Cin], exact"""
    return W.transpose(-2, -1) if (torch is not None and isinstance(W, torch.Tensor)) else np.swapaxes(W, -2, -1)


# the kernel shapes of the network ([K, Cin, Cout]: stem, blocks, the strided and transposed convolutions, the 1x1
# classifier and shortcuts) and generic ones that are no multiple of the 32 x 32 tile
NET_SHAPES = [(125, 1, 32), (27, 32, 32), (8, 64, 64), (27, 96, 96), (8, 256, 128), (27, 384, 256), (1, 96, 7),
              (1, 192, 128)]
GENERIC_SHAPES = [(27, 20, 12), (3, 5, 7), (2, 33, 31), (1, 1, 1)]


# ------------------------------------------------------------------ shared data
def _logu(rng, lo, hi, n):
    return 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)


def _sign(rng, n):
    return rng.choice(np.array([-1.0, 1.0]), n)


@functools.lru_cache(maxsize=4)
def _base_data(n, seed):
    """everything of make_data that does not depend on (wd, grad_scale); float64, read-only"""
    rng = np.random.default_rng(seed)
    p = _logu(rng, 1e-3, 1e1, n) * _sign(rng, n)
    g = _logu(rng, 1e-10, 1e2, n) * _sign(rng, n)
    m = _logu(rng, 1e-10, 1e2, n) * _sign(rng, n)
    v = _logu(rng, 1e-20, 1e4, n)
    b = n // 16
    g[0:b] = 0.0
    m[b:2 * b] = 0.0
    v[b:2 * b] = 0.0
    d = _logu(rng, 1e-6, 1e-2, b) * _sign(rng, b)
    d[::4] = 0.0
    t = slice(3 * b, 5 * b)
    g[t] = _logu(rng, 1e-10, 1e-7, 2 * b) * _sign(rng, 2 * b)
    m[t] = _logu(rng, 1e-10, 1e-7, 2 * b) * _sign(rng, 2 * b)
    v[t] = _logu(rng, 1e-20, 1e-16, 2 * b)
    p[t] = _logu(rng, 1e-3, 3e-3, 2 * b) * _sign(rng, 2 * b)
    out = tuple(a.astype(np.float32) for a in (p, g, m, v)) + (d,)
    for a in out:
        a.setflags(write=False)
    return out


def make_data(n, seed, wd=1e-4, grad_scale=1.0):
    """float32 (p, g, m, v) of n elements.  p: log-uniform magnitude 1e-3 .. 1e1; g, m: 1e-10 .. 1e2; v: 1e-20 .. 1e4;
    random signs.  Five blocks of n // 16 elements each at the front (whatever is left is the generic part; a block of a
    tiny n is empty):
      0  g == 0
      1  m == v == 0                                   a parameter's first step
      2  g s = -wd p (1 + d), |d| in 1e-6 .. 1e-2, every fourth d = 0: g' is what the cancellation leaves
      3, 4  |g|, |m| in 1e-10 .. 1e-7, v in 1e-20 .. 1e-16, |p| in 1e-3 .. 3e-3: sqrt(v') / sqrt(bc2) < 100 eps at every
            step count (step 1: v' <= 1e-16 + 1e-3 (1e-7 + 3e-7)^2, sqrt(v') / sqrt(1e-3) < 6e-7)
    Every intermediate of either chain stays a normal float32 or an exact zero (tests/test_optim_ref_cpu.py checks)."""
    p, g, m, v, d = _base_data(int(n), int(seed))
    b = n // 16
    g = g.copy()
    g[2 * b:3 * b] = (-f32(wd) * p[2 * b:3 * b].astype(np.float64) * (1.0 + d) / f32(grad_scale)).astype(np.float32)
    return p.copy(), g, m.copy(), v.copy()
