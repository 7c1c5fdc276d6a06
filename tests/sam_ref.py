"""numpy restatements of the gradient-norm, clipping and SAM kernels (lidog_amd/csrc/sam.hip, declared in
include/lidog_amd.h; lidog_amd.optim.SAM, clip_grad_norm): the squared norm in float64, everything else one float32
operation at a time, rounded on its own, in the order the header states it.  Plus, for comparison on the CPU, the same
two steps as they are usually written with torch (torch is imported only there)."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U32 = 2.0 ** -24         # unit roundoff of float32
U64 = 2.0 ** -53         # ... of float64
MAX_BLOCKS = 2048        # LIDOG_FLAT_MAX_BLOCKS: the grid cap of the three kernels
SWEEP = 1024 * MAX_BLOCKS   # elements one full sweep of a capped grid covers (256 threads x float4 per workgroup)


# ------------------------------------------------------------------ the squared norm
def terms(g, w=None):
    """t_i as the kernel forms it: g, or |w| * g rounded to float32 (adaptive)"""
    g = np.asarray(g, dtype=F32)
    if w is None:
        return g
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.abs(np.asarray(w, dtype=F32)) * g).astype(F32)


FSUM_MAX = 1 << 22       # up to here the restatement's sum is math.fsum's (a python list of the terms)


def sqnorm64(g, w=None):
    """sum t_i^2 in float64.  Every product is exact (two 24-bit significands).  Up to FSUM_MAX terms the sum is
    math.fsum's: correctly rounded, an error of at most U64 relative.  Beyond (the parameter count of a real model),
    where a python list of the terms costs seconds, chunks of FSUM_MAX terms are summed by numpy and the chunk sums by
    math.fsum."""
    t = terms(g, w).astype(F64)
    with np.errstate(over="ignore"):
        sq = t * t
    if not np.all(np.isfinite(sq)):
        return float(np.sum(sq))
    if sq.size <= FSUM_MAX:
        return math.fsum(sq.tolist())
    # numpy's pairwise sum of a chunk of non-negative terms: blocks of 128 summed in 8 lanes, then a binary tree, an
    # error below (16 + 8 + log2(FSUM_MAX / 128)) U64 < 40 U64 relative
    return math.fsum(float(np.sum(sq[i:i + FSUM_MAX])) for i in range(0, sq.size, FSUM_MAX))


def sqnorm_bound(n):
    """relative error of ANY float64 summation order of n non-negative exact terms: (n - 1) U64 to first order (each
    of at most n - 1 additions a partial sum passes through rounds it once, and all partial sums are at most the total);
    1.01 covers the higher orders and the restatement's own error (U64 up to FSUM_MAX terms; beyond, 41 U64 against a
    margin of 0.01 n U64 > 40000 U64)"""
    return 1.01 * max(n, 1) * U64


# ------------------------------------------------------------------ SAM's ascent step
def sam_coef(sqnorm, rho):
    """(float)((double)rho / (sqrt(sqnorm) + 1e-12)); rho reaches the kernel as a float32"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return F32(F64(F32(rho)) / (np.sqrt(F64(sqnorm)) + F64(1e-12)))


def perturb(w, g, sqnorm, rho, adaptive=False):
    """w + e; plain e = coef * g, adaptive e = ((w * w) * g) * coef; an element with g == +-0 keeps w's bits"""
    w, g = np.asarray(w, dtype=F32), np.asarray(g, dtype=F32)
    coef = sam_coef(sqnorm, rho)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if adaptive:
            e = (((w * w).astype(F32) * g).astype(F32) * coef).astype(F32)
        else:
            e = (coef * g).astype(F32)
        moved = (w + e).astype(F32)
    return np.where(g == 0, w, moved).astype(F32)


# ------------------------------------------------------------------ clip_grad_norm_
def clip_coef(sqnorm, max_norm, grad_scale=1.0):
    """min(1.0f, (float)((double)max_norm / (grad_scale * sqrt(sqnorm) + 1e-6))); both scalars reach the kernel as float32"""
    norm = F64(F32(grad_scale)) * np.sqrt(F64(sqnorm))
    with np.errstate(over="ignore"):
        return min(F32(1.0), F32(F64(F32(max_norm)) / (norm + F64(1e-6))))


def clip(g, sqnorm, max_norm, grad_scale=1.0):
    g = np.asarray(g, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (g * clip_coef(sqnorm, max_norm, grad_scale)).astype(F32)


# ------------------------------------------------------------------ the usual torch code, for the CPU comparison
def torch_sam_ascent(params, grads, rho, adaptive=False):
    """the first step of SAM as it is commonly written over a list of parameters: the norm of the per-tensor norms of
    (|p| if adaptive else 1) * g, scale = rho / (norm + 1e-12), p.add_((p^2 if adaptive else 1) * g * scale); a tensor
    without a gradient (None) is skipped.  In place, float32 throughout; returns the norm"""
    import torch
    norms = [((p.abs() if adaptive else 1.0) * g).norm(p=2) for p, g in zip(params, grads) if g is not None]
    norm = torch.norm(torch.stack(norms), p=2)
    scale = rho / (norm + 1e-12)
    with torch.no_grad():
        for p, g in zip(params, grads):
            if g is None:
                continue
            e_w = (torch.pow(p, 2) if adaptive else 1.0) * g * scale.to(p)
            p.add_(e_w)
    return norm


def torch_norm_error(n):
    """relative error of a float32 2-norm over n elements against the exact one, whatever the summation order: each
    square rounds once (U32), a sum of n non-negative terms in any order adds at most (n - 1) U32, the square root halves
    the sum's error and rounds once; a norm of per-tensor norms goes through that twice.  Bounded, without the halving,
    by (n + 8) U32 to first order; 1.01 for the higher orders"""
    return 1.01 * (n + 8) * U32
