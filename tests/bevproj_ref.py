"""Float64 yardstick of the BEV projection (lidog_amd.bev.sparse2super, csrc/bev.hip), written from the definition of
MinkUNetBaseBEV.sparse2super and independent of every lidog_* entry point:

  pixels     oracle.ref_torch.bev_pixels_ref (float32 index arithmetic, strict bounds, row -1 wraps to row H-1);
  winner     the LAST row that targets a pixel (sequential index_put_), via scatter_reduce(amax) of the row index;
  image      dense [H*W, C] per scan, zeros where no row landed, read through .view(C, H, W);
  pooling    F.max_pool2d(..., return_indices=True) in float64 on the device: ties keep the first cell in scan order,
             a NaN is taken whenever it is met (torch's rule), so the last NaN of a window wins;
  backward   max_pool2d's backward routes each window's gradient to its source cell, and index_put's backward is a
             gather: EVERY row that targets a pixel receives that pixel's gradient.

The dense image of a full-size scan at C = 256 is 8 GB in float64, so the planes of the viewed image are built and
pooled in chunks of at most MAX_CHUNK elements; only the pooled image (fp32: a max of fp32 values is one of them) and
the source-cell map (int32, as the kernel keeps it) are kept whole.

Bars (csrc/bev.hip):
  forward    bit-exact: a max is exact and both sides break ties alike (`assert_bits`); winner and pixel maps exact;
  backward   each feature cell receives the sum of the output gradients of the windows whose maximum it is, at most
             K = ceil(pk/ps)^2 of them, added in fp32 in ascending window order.  Integer-valued output gradients:
             exact (bev_ref.assert_exact).  Random ones: bev_ref's precision bar with that K (`windows_per_cell`)."""
import math

import torch
import torch.nn.functional as F

from oracle.ref_torch import bev_image_size, bev_pixels_ref

MAX_CHUNK = 1 << 25     # elements of one chunk of view planes: ~1.3 GB of temporaries on the device


def pool_out(H, pool):
    pk, ps, pp = pool
    return (H + 2 * pp - pk) // ps + 1


def windows_per_cell(pool):
    """the most windows that can cover one cell: the K of the backward's precision bar"""
    pk, ps, _ = pool
    return math.ceil(pk / ps) ** 2


class Proj64:
    """sparse2super64's result: winner [B*H*W] (row index or -1), pixel [n] (b*H*W + py*W + px, or -1 out of bounds),
    out [B, C, Ho, Wo] fp32, src [B, C, Ho, Wo] int32 (feature cell row*C + ch of the window's maximum, -1 for an empty
    pixel's zero), occ [B, C, Ho, Wo] bool (the window holds a cell of an occupied pixel: max_pool2d(occupancy) > 0)"""

    def __init__(self, n, C, B, H, W, pool, winner, pixel, out, src, occ):
        self.n, self.C, self.B, self.H, self.W, self.pool = n, C, B, H, W, pool
        self.winner, self.pixel, self.out, self.src, self.occ = winner, pixel, out, src, occ

    def backward(self, gout):
        """(g64 [n, C] float64, sum of |terms| [n, C] float64): every row gets the gradient of its pixel's cells"""
        cell = torch.zeros(self.n * self.C, dtype=torch.float64, device=gout.device)
        cabs = torch.zeros_like(cell)
        sel = (self.src.flatten() >= 0).nonzero().flatten()     # the few windows with a source cell
        s, g = self.src.flatten()[sel].long(), gout.flatten()[sel].double()
        cell.index_add_(0, s, g)
        cabs.index_add_(0, s, g.abs())
        g64 = torch.zeros((self.n, self.C), dtype=torch.float64, device=gout.device)
        a64 = torch.zeros_like(g64)
        rows = (self.pixel >= 0).nonzero().flatten()
        if rows.numel():
            w = self.winner[self.pixel[rows]]
            idx = (w * self.C).unsqueeze(1) + torch.arange(self.C, device=w.device)
            g64[rows] = cell[idx]
            a64[rows] = cabs[idx]
        return g64, a64


def pixels64(coords, B, bound, voxel):
    """(pixel [n] int64 on coords' device: b*H*W + py*W + px or -1, H); the float32 arithmetic runs on the CPU, where
    bev_pixels_ref was pinned to the reference's own output"""
    c = coords.cpu()
    H = bev_image_size(bound, voxel)
    if c.shape[0] == 0:
        return torch.empty(0, dtype=torch.int64, device=coords.device), H
    inb, px, py = bev_pixels_ref(c[:, 1:].int(), bound, voxel)
    ok = inb & (px >= 0) & (px < H) & (py >= 0) & (py < H)
    b = c[:, 0].long()
    assert bool(((b >= 0) & (b < B)).all()), "batch ids must lie in [0, B)"
    pix = torch.where(ok, (b * H + py) * H + px, torch.full_like(px, -1))
    return pix.to(coords.device), H


def sparse2super64(coords, feats, B, bound, voxel=0.05, pool=(5, 3, 1), max_chunk=MAX_CHUNK):
    """coords int32 [n, 4] (b, x, y, z), feats [n, C] (any float dtype, on the device) -> Proj64"""
    dev = feats.device
    n, C = feats.shape
    pixel, H = pixels64(coords, B, bound, voxel)
    W, HW = H, H * H
    pk, ps, pp = pool
    Ho, Wo = pool_out(H, pool), pool_out(W, pool)
    winner = torch.full((B * HW,), -1, dtype=torch.int64, device=dev)
    rows = (pixel >= 0).nonzero().flatten()
    winner.scatter_reduce_(0, pixel[rows], rows, reduce="amax", include_self=True)
    f64 = feats.detach().double().flatten()
    out = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=dev)
    src = torch.empty((B, C, Ho, Wo), dtype=torch.int32, device=dev)
    occ = torch.empty((B, C, Ho, Wo), dtype=torch.bool, device=dev)
    planes = max(1, max_chunk // HW)
    for b in range(B):
        wb = winner[b * HW:(b + 1) * HW]
        for c0 in range(0, C, planes):
            c1 = min(C, c0 + planes)
            f = torch.arange(c0 * HW, c1 * HW, device=dev)          # flat index of the viewed image
            p = f // C
            w = wb[p]
            cellidx = w * C + (f - p * C)
            del f, p
            full = w >= 0
            zero = torch.zeros((), dtype=torch.float64, device=dev)
            img = torch.where(full, f64[cellidx.clamp(min=0)], zero) if n else zero.expand(cellidx.shape)
            o, idx = F.max_pool2d(img.view(1, c1 - c0, H, W), pk, ps, pp, return_indices=True)
            del img
            o1, _ = F.max_pool2d(full.double().view(1, c1 - c0, H, W), pk, ps, pp, return_indices=True)
            sel = idx[0] + (torch.arange(c1 - c0, device=dev) * HW).view(-1, 1, 1)
            s = cellidx.view(-1)[sel]
            s = torch.where(full.view(-1)[sel], s, torch.full_like(s, -1))
            out[b, c0:c1] = o[0].float()
            src[b, c0:c1] = s.int()
            occ[b, c0:c1] = o1[0] > 0
            del cellidx, full, w, o, idx, o1, sel, s
    return Proj64(n, C, B, H, W, tuple(pool), winner, pixel, out, src, occ)


def assert_bits(got, ref, what):
    """fp32 tensors equal bit for bit, except that any NaN matches any NaN (payloads are not compared)"""
    gi, ri = got.contiguous().view(torch.int32), ref.contiguous().view(torch.int32)
    gn, rn = torch.isnan(got), torch.isnan(ref)
    bad = (gi != ri) & ~(gn & rn)
    if bool(bad.any()):
        first = bad.nonzero()[:5].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ (first at {first}: got "
                             f"{[float(got[tuple(i)]) for i in first]}, want {[float(ref[tuple(i)]) for i in first]})")
