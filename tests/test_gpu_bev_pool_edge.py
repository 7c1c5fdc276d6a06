"""The BEV projection's pooling kernels (csrc/bev.hip: lidog_bev_pool_fwd, lidog_bev_pool_bwd) on edge inputs, bit for bit
against oracle/ref_torch.py:sparse2super_ref and its autograd gradient.

Bound 2.0 m (an 80 x 80 image), so that with C in {4, 7, 96} the cells of a pixel fall inside one viewed row, straddle two
or three of them (80 % C != 0) and cross from one plane of the view into the next; pools with 1, 2, 3 and 8 windows over a
cell along an axis; several rows on one pixel (the last one wins, all of them receive the gradient), rows outside the bound,
a winner in the last pixel of the image, no row and one row, +Inf, NaN and exact ties, the row bitmasks on and off, and the
backward run twice.  Values are compared as bit patterns (a NaN equals itself)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 2.0
POOLS = [(5, 3, 1), (3, 2, 1), (2, 2, 0), (8, 3, 4), (8, 1, 0)]


def _dev(t):
    """every float operand the tests hand to the pooling kernels: the feature rows and the image gradient"""
    return t.cuda()


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


LAST_PIXEL_BOUND = 4.5    # a 180 x 180 image whose last pixel a voxel can reach (at 2.0 m float32 rounding stops at row 78)


def _last_pixel_coordinate(bound=BOUND):
    """integer voxel coordinates (x, y) that land in the last pixel a voxel can reach, and that pixel (py, px)"""
    from lidog_amd.bev import pixel_luts
    lx, ly, lo, H = pixel_luts(bound)
    px, py = int(lx.max()), int(ly.max())
    return int(np.nonzero(lx == px)[0][0]) + lo, int(np.nonzero(ly == py)[0][0]) + lo, py, px


@functools.lru_cache(maxsize=None)
def _scene(B, C, special):
    """coords int32 [n, 4] and feats [n, C] of one scene; CPU tensors, made once"""
    g = torch.Generator().manual_seed(1000 * B + 10 * C + int(special))
    n0 = 260 * B
    xy = torch.randint(-47, 48, (n0, 2), generator=g)            # |c| >= 40 is outside the bound
    far = torch.randint(0, n0, (12,), generator=g)
    xy[far] = xy[far] * 3                                         # beyond the pixel tables, too
    z = torch.randint(0, 4, (n0, 1), generator=g)                 # few z: many rows per pixel
    b = torch.randint(0, B, (n0, 1), generator=g)
    coords = torch.cat([b, xy, z], dim=1)
    x_last, y_last, _, _ = _last_pixel_coordinate()
    forced = torch.tensor([[B - 1, x_last, y_last, 0], [B - 1, x_last, y_last, 1], [B - 1, x_last, y_last, 2],
                           [0, 3, 3, 0], [0, 3, 3, 3], [0, 3, 3, 1]])
    coords = torch.unique(torch.cat([coords, forced]), dim=0)
    coords = coords[torch.randperm(coords.shape[0], generator=g)].to(torch.int32).contiguous()
    n = coords.shape[0]
    feats = torch.randn((n, C), generator=g)
    if special:
        r = torch.rand((n, C), generator=g)
        feats = torch.where(r < 0.35, (feats * 2).round() / 2, feats)       # exact ties, zeros (ties with empty cells)
        feats = torch.where((r >= 0.35) & (r < 0.38), torch.full_like(feats, float("inf")), feats)
        feats = torch.where((r >= 0.38) & (r < 0.41), torch.full_like(feats, float("nan")), feats)
    return coords, feats.contiguous()


@functools.lru_cache(maxsize=None)
def _reference(B, C, special, pool):
    """(image, gradient image, feature gradient) of the reference on the CPU"""
    from oracle.ref_torch import sparse2super_ref
    coords, feats = _scene(B, C, special)
    fr = feats.clone().requires_grad_(True)
    ref = sparse2super_ref(coords, fr, BOUND, pool=pool)
    gout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(7))
    (gref,) = torch.autograd.grad(ref, fr, gout)
    return ref.detach(), gout, gref


def _run(coords, feats, B, pool, gout, rowbits, monkeypatch):
    """(image, feature gradient, the same gradient from a second backward run, row bitmask buffer or None)"""
    from lidog_amd import bev
    monkeypatch.setattr(bev, "SPARSE_CONV1", rowbits)
    fg = _dev(feats.clone()).requires_grad_(True)
    out = bev._Sparse2SuperFn.apply(fg, coords.cuda(), B, BOUND, 0.05, pool)
    gd = _dev(gout)
    g1, = torch.autograd.grad(out, fg, gd, retain_graph=True)
    g2, = torch.autograd.grad(out, fg, gd)
    torch.cuda.synchronize()
    return out.detach(), g1, g2, getattr(out.grad_fn, "_lidog_support", None)


def _check_rowbits(act, out):
    """every cell that is not a plain zero lies in a window the kernel marked"""
    B, C, Ho, Wo = out.shape
    words = (Wo + 63) // 64
    bits = act[: 2 * B * C * Ho * words].cpu().view(torch.int64).view(B, C, Ho, words)
    xo = torch.arange(Wo)
    marked = (bits[..., xo // 64] >> (xo % 64)) & 1
    live = out.cpu().view(torch.int32) != 0
    assert bool((marked[live] == 1).all())


def _check_plain(C, pool, B, monkeypatch):
    coords, feats = _scene(B, C, False)
    ref, gout, gref = _reference(B, C, False, pool)
    # the reference alone: finite, and neither empty nor full
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(gref).all())
    assert 0 < int((ref != 0).sum()) < ref.numel() and 0 < int((gref != 0).sum()) < gref.numel()
    for rowbits in (True, False):
        out, g1, g2, act = _run(coords, feats, B, pool, gout, rowbits, monkeypatch)
        assert _bits_equal(out, ref), f"forward differs (row bitmasks {rowbits})"
        assert _bits_equal(g1, gref), f"backward differs (row bitmasks {rowbits})"
        assert _bits_equal(g1, g2), "two backward runs differ"
        assert (act is not None) == (rowbits and C <= 128)
        if act is not None:
            _check_rowbits(act, out)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("pool", POOLS, ids=lambda p: "k%ds%dp%d" % p)
@pytest.mark.parametrize("C", [4, 7, 96])
def test_pool_bits_match_reference(C, pool, B, monkeypatch):
    _check_plain(C, pool, B, monkeypatch)


def test_pool_pixel_over_more_than_four_viewed_rows(monkeypatch):
    """C = 250 cells of a pixel touch up to five rows of the 80-wide view: the forward's one-wave-per-row kernel"""
    _check_plain(250, (5, 3, 1), 1, monkeypatch)


@pytest.mark.parametrize("pool", [(5, 3, 1), (3, 2, 1), (8, 3, 4)], ids=lambda p: "k%ds%dp%d" % p)
@pytest.mark.parametrize("C", [7, 96])
def test_pool_inf_nan_ties(C, pool, monkeypatch):
    """+Inf, NaN (max_pool2d takes the last NaN of a window, wherever it sits: first cell, last cell, between) and ties
    (the first cell in scan order keeps the gradient)"""
    B = 3
    coords, feats = _scene(B, C, True)
    ref, gout, gref = _reference(B, C, True, pool)
    assert bool(torch.isnan(ref).any()) and bool(torch.isinf(ref).any()) and bool((ref == 0).any())
    assert bool(torch.isfinite(gref).all()) and int((gref != 0).sum()) > 0
    for rowbits in (True, False):
        out, g1, g2, act = _run(coords, feats, B, pool, gout, rowbits, monkeypatch)
        assert _bits_equal(out, ref), f"forward differs (row bitmasks {rowbits})"
        assert _bits_equal(g1, gref), f"backward differs (row bitmasks {rowbits})"
        assert _bits_equal(g1, g2), "two backward runs differ"
        if rowbits:
            _check_rowbits(act, out)


def test_several_rows_on_one_pixel_and_last_pixel():
    """the scene holds what the cases above rely on: shared pixels, rows outside the image, the last pixel"""
    from oracle.ref_torch import bev_pixels_ref
    from lidog_amd.bev import bev_image_size
    coords, _ = _scene(3, 7, False)
    H = bev_image_size(BOUND)
    inb, px, py = bev_pixels_ref(coords[:, 1:], BOUND, 0.05)
    assert 0 < int(inb.sum()) < coords.shape[0]
    lin = (coords[:, 0].long()[inb] * H + py[inb]) * H + px[inb]
    assert torch.unique(lin).numel() < lin.numel()
    _, _, py_last, px_last = _last_pixel_coordinate()
    assert int(lin.max()) == (2 * H + py_last) * H + px_last


@pytest.mark.parametrize("rowbits", [True, False])
@pytest.mark.parametrize("n", [0, 1, 3])
def test_no_row_one_row_last_pixel(n, rowbits, monkeypatch):
    """no row; one row, the winner of the image's very last pixel (bound 4.5 m); three rows on that pixel"""
    from oracle.ref_torch import sparse2super_ref
    from lidog_amd import bev
    B, C, pool, bound = 1, 7, (5, 3, 1), LAST_PIXEL_BOUND
    H = bev.bev_image_size(bound)
    x_last, y_last, py, px = _last_pixel_coordinate(bound)
    assert (py, px) == (H - 1, H - 1)
    coords = torch.tensor([[0, x_last, y_last, z] for z in (2, 0, 1)], dtype=torch.int32)[:n]
    feats = torch.tensor([[1.5, -2.0, 0.0, 3.0, -0.5, 0.25, 8.0], [-1.0, 2.0, 0.5, -3.0, 4.0, 0.0, -8.0],
                          [0.5, 0.5, -0.5, 1.0, 9.0, -0.25, 2.0]])[:n]
    Ho = (H + 2 * pool[2] - pool[0]) // pool[1] + 1
    gout = torch.randn((B, C, Ho, Ho), generator=torch.Generator().manual_seed(3))
    monkeypatch.setattr(bev, "SPARSE_CONV1", rowbits)
    fg = _dev(feats.clone()).requires_grad_(True)
    out = bev._Sparse2SuperFn.apply(fg, coords.cuda(), B, bound, 0.05, pool)
    gd = _dev(gout)
    g1, = torch.autograd.grad(out, fg, gd, retain_graph=True)
    g2, = torch.autograd.grad(out, fg, gd)
    if n == 0:
        assert tuple(out.shape) == (B, C, Ho, Ho) and not bool(out.any()) and tuple(g1.shape) == (0, C)
        return
    fr = feats.clone().requires_grad_(True)
    ref = sparse2super_ref(coords, fr, bound, pool=pool)
    (gref,) = torch.autograd.grad(ref, fr, gout)
    assert int((ref != 0).sum()) > 0 and int((gref != 0).sum()) > 0
    assert _bits_equal(out, ref) and _bits_equal(g1, gref) and _bits_equal(g1, g2)
    if n == 3:
        assert bool((gref[0] == gref[1]).all()) and bool((gref[0] == gref[2]).all())
