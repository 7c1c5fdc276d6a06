"""sparse2super (csrc/bev.hip: winner map, fused view + max-pool, gather backward) against its float64 yardstick
(tests/bevproj_ref.py) at the production geometry -- bound 50 and 30, synthetic kitti120k / nusc35k scans at each BEV
level's tensor stride and channel count -- and at the edges of the kernels' index arithmetic: C = 512 at bound 50
(C H W just under 2^31, the top of the magic division's range), C = 1..4 (one window row crosses several pixels),
W % C = 0, C = 97, C > W, every pool geometry of the three PK instances with and without row bitmasks; empty scans, rows
out of bounds, on the strict bound and on the wrapped row -1, ties, +inf and NaN.

Direct calls pre-fill every output with NaN (argsrc and the pixel map with a sentinel, the bitmasks with ones), so an
element a kernel never writes fails.  Checks: winner and pixel maps exact; the image bit-exact; argsrc equal to the
source-cell map (where a bit is set when the kernel keeps row bitmasks), the bitmasks equal max_pool2d(occupancy) > 0;
the feature gradient exact for integer-valued output gradients and within the precision bar for random ones; a second
run bit-identical."""
import functools

import numpy as np
import pytest
import torch

import bev_ref
import bevproj_ref as P

pytestmark = pytest.mark.gpu

SENTINEL = -7
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _scans(config, B, stride, seed0=0):
    """collated coords of B synthetic scans at tensor stride `stride` (coordinates floored to multiples of it,
    duplicates dropped in first-occurrence order, like a strided coordinate map), on the device"""
    from lidog_amd import synth
    c = synth.make_batch(list(range(seed0, seed0 + B)), config, "cpu")["coords_int"].clone()
    if stride > 1:
        c[:, 1:] = torch.div(c[:, 1:], stride, rounding_mode="floor") * stride
        _, first = np.unique(c.numpy(), axis=0, return_index=True)
        c = c[torch.from_numpy(np.sort(first))]
    return c.cuda()


def _random_coords(B, H, n, seed, dup=1, spread=0.55, batch_ids=None):
    """n rows in B scans, x, y uniform over +-spread H voxels (partly out of bounds for spread > 0.5); each (b, x, y)
    repeated `dup` times with different z: several rows per pixel"""
    g = torch.Generator().manual_seed(seed)
    m = n // dup
    ids = torch.tensor(batch_ids) if batch_ids is not None else torch.arange(B)
    b = ids[torch.randint(0, len(ids), (m,), generator=g)]
    lim = int(spread * H)
    xy = torch.randint(-lim, lim, (m, 2), generator=g)
    c = torch.cat([b.unsqueeze(1), xy], 1).repeat_interleave(dup, 0)
    z = torch.randint(-20, 20, (m * dup, 1), generator=g)
    c = torch.cat([c, z], 1).int()
    return c[torch.randperm(c.shape[0], generator=g)].cuda()


def _features(n, C, seed, kind="rand"):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "ties":
        return torch.randint(-1, 2, (n, C), device="cuda", generator=g).float()
    f = torch.randn(n, C, device="cuda", generator=g)
    if kind == "relu":
        return f.clamp_min(0)
    if kind in ("inf", "nan"):
        hit = torch.rand(n, C, device="cuda", generator=g) < 0.02
        f = torch.where(hit, torch.full_like(f, float("inf") if kind == "inf" else NAN), f)
        if kind == "inf":
            f = torch.where(torch.rand(n, C, device="cuda", generator=g) < 0.01, torch.full_like(f, -float("inf")), f)
    return f


def _kernel(coords, feats, B, bound, pool, rowbits):
    from lidog_amd import bev
    from lidog_amd._lib import call, ptr
    n, C = feats.shape
    lx, ly, lo, H = bev._device_luts(bound, 0.05, "cuda")
    W = H
    pk, ps, pp = pool
    Ho, Wo = P.pool_out(H, pool), P.pool_out(W, pool)
    winner = torch.full((B, H, W), -1, dtype=torch.int32, device="cuda")
    pixel = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    call("lidog_bev_winner", ptr(coords), n, ptr(lx), ptr(ly), lo, lx.shape[0], H, W, ptr(winner), ptr(pixel))
    out = torch.full((B, C, Ho, Wo), NAN, device="cuda")
    arg = torch.full((B, C, Ho, Wo), SENTINEL, dtype=torch.int32, device="cuda")
    words = (Wo + 63) // 64
    bits = torch.full((B * C * Ho * words,), -1, dtype=torch.int64, device="cuda") if rowbits else None
    call("lidog_bev_pool_fwd", ptr(feats), C, ptr(winner), ptr(pixel), n, B, H, W, pk, ps, pp, Ho, Wo, ptr(out),
         ptr(arg), ptr(bits))
    return winner, pixel, out, arg, bits


def _kernel_bwd(winner, pixel, arg, gout, n, C, pool):
    from lidog_amd._lib import call, ptr
    B, _, Ho, Wo = gout.shape
    H, W = winner.shape[1:]
    g = torch.full((n, C), NAN, device="cuda")
    call("lidog_bev_pool_bwd", ptr(gout), ptr(arg), ptr(winner), ptr(pixel), n, C, B, H, W, *pool, Ho, Wo, ptr(g))
    return g


def _bitmap(bits, shape):
    B, C, Ho, Wo = shape
    words = (Wo + 63) // 64
    cols = torch.arange(Wo, device=bits.device)
    return ((bits.view(B, C, Ho, words)[..., cols // 64] >> (cols % 64)) & 1).bool()


def _check(coords, feats, B, bound, pool, rowbits, record_property=None, tag=""):
    """every check of the module docstring on the direct calls; returns the worst precision ratios"""
    n, C = feats.shape
    ref = P.sparse2super64(coords, feats, B, bound, pool=pool)
    winner, pixel, out, arg, bits = _kernel(coords, feats, B, bound, pool, rowbits)
    assert torch.equal(winner.flatten().long(), ref.winner), f"{tag}: winner map"
    assert torch.equal(pixel.long(), ref.pixel), f"{tag}: pixel map"
    P.assert_bits(out, ref.out, f"{tag}: image")
    if bits is None:
        defined = None
        assert torch.equal(arg, ref.src), f"{tag}: argsrc differs at {int((arg != ref.src).sum())} windows"
    else:
        defined = _bitmap(bits, out.shape)
        assert torch.equal(defined, ref.occ), f"{tag}: row bitmasks differ at {int((defined != ref.occ).sum())} windows"
        assert torch.equal(arg[defined], ref.src[defined]), f"{tag}: argsrc"
    del ref.out, ref.occ                        # compared: room for the backward and the second run
    ratios = (0.0, 0.0)
    if n:
        gen = torch.Generator(device="cuda").manual_seed(n + C)
        gout = torch.randint(-8, 9, out.shape, device="cuda", generator=gen).float()
        g64, a64 = ref.backward(gout)
        got = _kernel_bwd(winner, pixel, arg, gout, n, C, pool)
        bev_ref.assert_exact(got, g64, a64, f"{tag}: gradient, integer gout")
        gout = torch.randn(out.shape, device="cuda", generator=gen)
        g64, a64 = ref.backward(gout)
        got = _kernel_bwd(winner, pixel, arg, gout, n, C, pool)
        ratios = bev_ref.assert_precision(got, g64, a64, P.windows_per_cell(pool), f"{tag}: gradient, random gout")
        del g64, a64
    else:
        got = None
    del ref
    # a second run: bit-identical
    w2, p2, out2, arg2, bits2 = _kernel(coords, feats, B, bound, pool, rowbits)
    assert torch.equal(w2, winner) and torch.equal(p2, pixel)
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32))
    if bits is None:
        assert torch.equal(arg2, arg)
    else:
        assert torch.equal(bits2, bits) and torch.equal(arg2[defined], arg[defined])
    if got is not None:
        assert torch.equal(_kernel_bwd(w2, p2, arg2, gout, n, C, pool).view(torch.int32), got.view(torch.int32))
    if record_property is not None:
        record_property(f"{tag}_elem", ratios[0])
        record_property(f"{tag}_fro", ratios[1])
    return ratios


# ------------------------------------------------------------------ production geometry
# (bound, config, B, tensor stride, C, row bitmasks): the BEV levels block8 / block7 (C 96, stride 1 / 2), block6
# (C 128, stride 4) and bottle (C 256, stride 16, no bitmasks: sparse2super keeps them for C <= 128 only)
PROD = [(50.0, "kitti120k", 4, 1, 96, True), (50.0, "kitti120k", 2, 2, 96, True), (50.0, "kitti120k", 2, 4, 128, True),
        (50.0, "kitti120k", 2, 16, 256, False), (30.0, "nusc35k", 4, 1, 96, True), (30.0, "nusc35k", 4, 4, 128, True),
        (30.0, "nusc35k", 4, 16, 256, False)]


@pytest.mark.parametrize("bound,config,B,stride,C,rowbits", PROD)
def test_production_geometry_direct(bound, config, B, stride, C, rowbits, record_property):
    coords = _scans(config, B, stride)
    _check(coords, _features(coords.shape[0], C, C + stride, "relu"), B, bound, (5, 3, 1), rowbits, record_property,
           f"{config}_b{int(bound)}_s{stride}_C{C}")


@pytest.mark.parametrize("bound,config,B,stride,C", [(50.0, "kitti120k", 4, 1, 96), (30.0, "nusc35k", 2, 4, 128),
                                                     (50.0, "kitti120k", 2, 16, 256)])
def test_production_geometry_through_the_module(bound, config, B, stride, C, record_property):
    """bev.sparse2super (autograd, row bitmasks chosen by the module): image bit-exact, feature gradient in the bars"""
    import lidog_amd.me as ME
    from lidog_amd import bev
    coords = _scans(config, B, stride)
    n = coords.shape[0]
    feats = _features(n, C, 5 * C, "relu")
    ref = P.sparse2super64(coords, feats, B, bound)
    fg = feats.clone().requires_grad_(True)
    out = bev.sparse2super(ME.SparseTensor(coordinates=coords, features=fg), bound=bound)
    assert (bev.structural_support(out) is not None) == (C <= 128)
    P.assert_bits(out.detach(), ref.out, "image")
    gen = torch.Generator(device="cuda").manual_seed(1)
    gout = torch.randint(-8, 9, out.shape, device="cuda", generator=gen).float()
    out.backward(gout)
    g64, a64 = ref.backward(gout)
    bev_ref.assert_exact(fg.grad, g64, a64, "gradient, integer gout")
    fg.grad = None
    out = bev.sparse2super(ME.SparseTensor(coordinates=coords, features=fg), bound=bound)
    gout = torch.randn(out.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    out.backward(gout)
    g64, a64 = ref.backward(gout)
    r = bev_ref.assert_precision(fg.grad, g64, a64, P.windows_per_cell((5, 3, 1)), "gradient, random gout")
    record_property("elem", r[0])
    record_property("fro", r[1])


# ------------------------------------------------------------------ edges of the index arithmetic
def test_c512_at_bound_50_top_of_the_index_range(record_property):
    """C H W = 2.048e9 < 2^31: the largest flat index of the viewed image, x C < 2^40 for the magic division"""
    coords = _scans("kitti120k", 1, 1)
    assert 512 * 2000 * 2000 < 2 ** 31
    _check(coords, _features(coords.shape[0], 512, 512, "relu"), 1, 50.0, (5, 3, 1), False, record_property, "C512")


@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("pool,rowbits", [((5, 3, 1), True), ((8, 3, 4), False), ((3, 1, 1), True)])
def test_small_channel_counts_straddle_pixels(C, pool, rowbits, record_property):
    """C < pk: one window row covers several pixels (all pk of them at C = 1), the straddle path of pool_one"""
    coords = _scans("kitti120k", 2, 1)
    _check(coords, _features(coords.shape[0], C, C, "rand"), 2, 10.0, pool, rowbits, record_property, f"C{C}")


@pytest.mark.parametrize("bound,C,B,rowbits", [(50.0, 80, 1, True), (30.0, 97, 2, True), (30.0, 97, 2, False),
                                               (1.0, 100, 2, True), (0.5, 41, 3, False)])
def test_channel_counts_against_the_image_width(bound, C, B, rowbits, record_property):
    """W % C = 0 (80 | 2000), C = 97 (no common factor with W), C > W (bound 1: W = 40; bound 0.5: W = 20)"""
    from oracle.ref_torch import bev_image_size
    H = bev_image_size(bound)
    if bound >= 30:
        coords = _scans("nusc35k" if bound == 30 else "kitti120k", B, 1)
    else:
        coords = _random_coords(B, H, 3000, C, dup=3)
    _check(coords, _features(coords.shape[0], C, C, "rand"), B, bound, (5, 3, 1), rowbits, record_property, f"C{C}")


POOL_GEOMS = [(5, 3, 1), (5, 1, 2), (5, 2, 0), (5, 6, 1), (3, 3, 1), (3, 1, 1), (8, 3, 4), (8, 8, 0), (1, 1, 0),
              (2, 2, 1)]


@pytest.mark.parametrize("pool", POOL_GEOMS)
@pytest.mark.parametrize("C,rowbits", [(5, True), (96, False), (96, True)])
def test_pool_geometries(pool, C, rowbits, record_property):
    """every PK instance (pk <= 3, <= 5, <= 8), stride above the kernel size ((5, 6, 1): cells in no window get 0)"""
    coords = _random_coords(2, 400, 6000, sum(pool) + C, dup=4)
    _check(coords, _features(coords.shape[0], C, C + pool[0], "rand"), 2, 10.0, pool, rowbits, record_property,
           f"pool{pool}")


# ------------------------------------------------------------------ data
def _sweep_bounds(H):
    """every x (then every y) of the lookup range on one row (column): the strict bounds and, at bound 5, the row -1
    that wraps to H - 1"""
    lim = int(H * 0.6)
    c = torch.arange(-lim, lim, dtype=torch.int32)
    z = torch.zeros_like(c)
    a = torch.stack([z, c, torch.full_like(c, 3), z], 1)
    b = torch.stack([z + 1, torch.full_like(c, -2), c, z + 1], 1)
    return torch.cat([a, b, a]).cuda()      # the row sweep twice: the second copy wins its pixels


DATA = ["dup", "empty_scan", "all_oob", "n0", "bounds", "negative", "ties", "inf", "nan"]


def _data_case(kind, C):
    H = 200
    if kind == "dup":
        return _random_coords(2, H, 4000, 1, dup=40, spread=0.3), 2, "rand"
    if kind == "empty_scan":
        return _random_coords(3, H, 3000, 2, dup=2, batch_ids=[0, 2]), 3, "rand"
    if kind == "all_oob":
        c = _random_coords(2, H, 500, 3)
        c[:, 1] = torch.where(c[:, 1] >= 0, c[:, 1] + H, c[:, 1] - H)
        return c, 2, "rand"
    if kind == "n0":
        return torch.empty((0, 4), dtype=torch.int32, device="cuda"), 2, "rand"
    if kind == "bounds":
        return _sweep_bounds(H), 2, "rand"
    return _random_coords(2, H, 4000, 4, dup=3), 2, {"negative": "rand", "ties": "ties", "inf": "inf",
                                                    "nan": "nan"}[kind]


@pytest.mark.parametrize("kind", DATA)
@pytest.mark.parametrize("C,pool,rowbits", [(3, (5, 3, 1), True), (96, (5, 3, 1), False), (16, (3, 1, 1), True)])
def test_data_cases(kind, C, pool, rowbits, record_property):
    """negative features (the empty cells' zeros win windows), exact ties between occupied cells and with empty zeros,
    +-inf, NaN (taken as torch's max_pool2d takes it: the last NaN of a window in scan order)"""
    coords, B, fkind = _data_case(kind, C)
    n = coords.shape[0]
    feats = _features(n, C, C + len(kind), fkind)
    if kind == "nan":
        # the backward of a NaN window is defined; an exact bar on a NaN-free gradient needs no NaN in the gradient
        assert bool(torch.isnan(feats).any())
    _check(coords, feats, B, 5.0, pool, rowbits, record_property, kind)
    if kind == "bounds":
        ref = P.sparse2super64(coords, feats, B, 5.0, pool=pool)
        assert int((ref.pixel < 0).sum()) > 0 and int((ref.pixel % (200 * 200) // 200 == 199).sum()) > 0
    if kind == "all_oob":
        assert int((P.pixels64(coords, B, 5.0, 0.05)[0] >= 0).sum()) == 0


def test_torch_max_pool2d_takes_the_last_nan_of_a_window():
    """the rule the yardstick inherits (and pool_one follows): a NaN is taken whenever it is met"""
    x = torch.tensor([[1.0, 5.0, 2.0], [NAN, 7.0, NAN], [3.0, 9.0, 4.0]], device="cuda").view(1, 1, 3, 3)
    for dt in (torch.float32, torch.float64):
        o, i = torch.nn.functional.max_pool2d(x.to(dt), 3, 1, 0, return_indices=True)
        assert bool(torch.isnan(o).all()) and int(i) == 5
        o, i = torch.nn.functional.max_pool2d(x.to(dt), 2, 1, 1, return_indices=True)
        assert bool(torch.isnan(o[0, 0, 1]).all()) and int(i[0, 0, 1, 0]) == 3 and int(i[0, 0, 1, 2]) == 5
        assert float(o[0, 0, 3, 1]) == 9.0 and float(o[0, 0, 0, 1]) == 5.0
