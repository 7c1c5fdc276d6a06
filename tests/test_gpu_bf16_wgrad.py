"""The bf16-operand weight gradient (lidog_sconv_wgrad_bf16: csrc/sconv_bf16.hip:k_sconv_wgrad_bf16, then
sconv.hip:k_items_sum4) through the C ABI against the float64 yardstick of tests/sparse_ref.py.

Scenes: two small scans, and a flat scene (all z equal: 18 of the 27 offsets of a 3^3 map are empty and must give exactly
0).  Maps: k3, s2 (k2 s2), tr (its exchange) and k1.  Shapes: one per tile family of the kernel -- 32 x 32 (one MFMA tile:
two waves split the two k = 16 steps of a chunk and write two slabs per item), 64 x 64, 96 x 96 (three waves), 128 x 96,
256 x 256 and 384 x 256 (several workgroups per item).  Work-item layouts: what me._wgrad_chunk cuts with _WGRAD_FIT = 0,
1, 2 from the bf16 kernel's OWN slot count, 128-pair items, one item per offset, and `short`: items of 24 pairs, shorter
than one 32-pair chunk and no multiple of the instruction's k = 16.  gW and the partial slots are pre-filled with NaN.

Bars.  Exact: integer operands |v| <= 15, half of them zero -- exact in bf16 (integers up to 256 are), every product and
partial sum exact in fp32 -- so the result must be the float64 result, bit for bit: a lost, doubled or mis-transposed pair
fails it at any size, and so does a tail row that was not zeroed (the NaN pre-fill aside, the clamped loads behind the end
of an item fetch a real, non-zero row).  Precision: randn operands rounded to bf16 FIRST; their products are exact in
fp32, so against wgrad64 of the rounded operands only the fp32 accumulation of P_k terms is left: the elementwise bound
of bev_ref.precision_ratios (1.01 P_k u sum|terms|, per offset) with ratio <= 2 -- the factor 2 is the matrix unit's
adder, which does not round every partial sum to nearest the way the chain of the derivation does (tests/test_gpu_bf16.py
argues the same for the forward kernels).  The Frobenius ratio is recorded, not asserted."""
import numpy as np
import pytest
import torch

import sconv_ref as S
import sparse_ref as R
from helpers import small_batch

pytestmark = pytest.mark.gpu

NAN = float("nan")
SHAPES = [(32, 32), (64, 64), (96, 96), (128, 96), (256, 256), (384, 256)]
KINDS = ["k3", "s2", "tr", "k1"]
_SCENES = {}


def _fill(shape, value, dtype=torch.float32):
    """every output and workspace the tests own; value None: uninitialised (torch.empty)"""
    if value is None:
        return torch.empty(shape, dtype=dtype, device="cuda")
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _dev(t):
    """every float operand the tests own"""
    return t.cuda()


def _manager(coords):
    import lidog_amd.me as ME
    st = ME.SparseTensor(coordinates=coords.cuda(), features=torch.ones((coords.shape[0], 1), device="cuda"))
    return st.coordinate_manager


def _scene(name):
    if name not in _SCENES:
        if name == "small":
            c = small_batch((0, 1), n_points=2500)
        elif name == "flat":
            c = small_batch((2,), n_points=2500).clone()
            c[:, 3] = 0
            c = torch.unique(c, dim=0)
        else:
            c = torch.from_numpy(S.scene(name))
        _SCENES[name] = _manager(c.int())
    return _SCENES[name]


def _pairs(cm, kind):
    """(pair_a, pair_g, k_off_host, n_a, n_g) of gW[k] = sum A[pair_a]^T G[pair_g] for a convolution of that kind"""
    if kind == "k1":
        n = cm.maps[1].n
        r = torch.arange(n, dtype=torch.int32, device="cuda")
        return r, r, [0, n], n, n
    if kind == "k3":
        m = cm.kernel_map(1, 1, 3)
        return m.pair_in, m.pair_out, list(m.k_off_host), m.n_in, m.n_out
    cm.stride(1, 2)
    m = cm.kernel_map(1, 2, 2)
    if kind == "s2":
        return m.pair_in, m.pair_out, list(m.k_off_host), m.n_in, m.n_out
    return m.pair_out, m.pair_in, list(m.k_off_host), m.n_out, m.n_in


def _slabs(Cin, Cout, n_items):
    from lidog_amd import _lib
    return int(_lib.load().lidog_sconv_wgrad_bf16_slabs(Cin, Cout, n_items))


def _short(k_off, Cin, Cout):
    """24 pairs per item, as long as the partial slots stay below 512 MB"""
    P_k = np.diff(np.asarray(k_off, dtype=np.int64))
    short = 24
    while _slabs(Cin, Cout, int(P_k.sum()) // short + len(P_k)) * Cin * Cout * 4 > 512 << 20:
        short *= 2
    return short


def _layouts(k_off, Cin, Cout, monkeypatch):
    import lidog_amd.me as ME
    P_k = np.diff(np.asarray(k_off, dtype=np.int64))
    out, default = {}, ME._WGRAD_FIT
    for fit in (0, 1, 2):
        monkeypatch.setattr(ME, "_WGRAD_FIT", fit)
        out[f"fit{fit}"] = ME._wgrad_chunk(k_off, Cin, Cout, bf16=True)
    monkeypatch.setattr(ME, "_WGRAD_FIT", default)
    out["c128"] = 128
    out["one_per_offset"] = max(128, int(P_k.max()))
    out["short"] = _short(k_off, Cin, Cout)
    return out


def _wgrad(A, pair_a, G, pair_g, k_off, chunk, Cin, Cout):
    import lidog_amd.me as ME
    from lidog_amd._lib import call, ptr
    items, n_items, item_off = ME._wgrad_items_host(k_off, chunk)
    K = len(k_off) - 1
    items = torch.from_numpy(np.ascontiguousarray(items)).cuda()
    item_off = torch.from_numpy(item_off).cuda()
    slabs = _slabs(Cin, Cout, n_items)
    assert slabs >= n_items
    partial = _fill((max(slabs, 1), Cin, Cout), NAN)
    gW = _fill((K, Cin, Cout), NAN)
    call("lidog_sconv_wgrad_bf16", ptr(A), ptr(pair_a), ptr(G), ptr(pair_g), ptr(items), n_items, ptr(item_off), K, Cin,
         Cout, ptr(partial), ptr(gW))
    torch.cuda.synchronize()
    return gW, n_items


def _bf16(t):
    return t.bfloat16().float()


def _operands(n_a, n_g, Cin, Cout, seed, exact):
    g = torch.Generator().manual_seed(seed)
    if exact:
        return (_dev(R.exact_operands((n_a, Cin), g, -15, 15, 0.5, "cuda")),
                _dev(R.exact_operands((n_g, Cout), g, -15, 15, 0.5, "cuda")))
    return _dev(_bf16(torch.randn((n_a, Cin), generator=g))), _dev(_bf16(torch.randn((n_g, Cout), generator=g)))


def _check_all(cm, kind, Cin, Cout, monkeypatch, record_property, tag):
    pair_a, pair_g, k_off, n_a, n_g = _pairs(cm, kind)
    layouts = _layouts(k_off, Cin, Cout, monkeypatch)
    worst = [0.0, 0.0]
    for exact in (True, False):
        A, G = _operands(n_a, n_g, Cin, Cout, Cin * 131 + Cout * 7 + len(kind), exact)
        ref, ab, P_k = R.wgrad64(A.double(), pair_a, G.double(), pair_g, k_off)
        for name, chunk in layouts.items():
            got, n_items = _wgrad(A, pair_a, G, pair_g, k_off, chunk, Cin, Cout)
            what = f"{tag} {Cin}->{Cout} {kind} layout {name} (chunk {chunk}, {n_items} items)"
            if exact:
                R.assert_exact(got, ref, ab, what)
                continue
            for k in range(ref.shape[0]):
                e, f = R.precision_ratios(got[k], ref[k], ab[k], max(int(P_k[k]), 1))
                print(f"{what} offset {k}: elementwise {e:.3g}, Frobenius {f:.3g}")
                assert e <= 2.0, f"{what} offset {k}: {e:.3g} x the fp32 summation bound (NaN: never written)"
                worst = [max(worst[0], e), max(worst[1], f)]
    record_property("worst_elem", worst[0])
    record_property("worst_fro", worst[1])
    return k_off


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Cin,Cout", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_weight_gradient_vs_float64_on_small_scenes(Cin, Cout, kind, monkeypatch, record_property):
    _check_all(_scene("small"), kind, Cin, Cout, monkeypatch, record_property, "small")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Cin,Cout", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_weight_gradient_vs_float64_on_the_flat_scene(Cin, Cout, kind, monkeypatch, record_property):
    """k3: 18 of the 27 offsets are empty; the exact bar holds them to exactly 0 (their reference is 0)"""
    cm = _scene("flat")
    k_off = _check_all(cm, kind, Cin, Cout, monkeypatch, record_property, "flat")
    if kind == "k3":
        assert (np.diff(np.asarray(k_off)) == 0).sum() == 18, "the flat scene should leave the 18 offsets with dz != 0 empty"


@pytest.mark.parametrize("Cin,Cout", [(32, 32), (96, 96), (256, 256)])
def test_empty_offsets_give_exactly_zero(Cin, Cout, monkeypatch):
    cm = _scene("flat")
    pair_a, pair_g, k_off, n_a, n_g = _pairs(cm, "k3")
    empty = np.diff(np.asarray(k_off)) == 0
    assert empty.sum() == 18
    A, G = _operands(n_a, n_g, Cin, Cout, 5, False)
    for name, chunk in _layouts(k_off, Cin, Cout, monkeypatch).items():
        got, _ = _wgrad(A, pair_a, G, pair_g, k_off, chunk, Cin, Cout)
        sub = got[torch.from_numpy(empty).cuda()]
        assert bool((sub == 0).all()), f"{Cin}->{Cout} layout {name}: an empty offset is not exactly zero (NaN: never written)"


@pytest.mark.parametrize("Cin,Cout", [(32, 32), (128, 96), (256, 256)])
def test_two_calls_give_the_same_bits(Cin, Cout, monkeypatch):
    cm = _scene("small")
    pair_a, pair_g, k_off, n_a, n_g = _pairs(cm, "k3")
    g = torch.Generator().manual_seed(9)
    A, G = _dev(torch.randn((n_a, Cin), generator=g)), _dev(torch.randn((n_g, Cout), generator=g))
    lay = _layouts(k_off, Cin, Cout, monkeypatch)
    for name in ("fit1", "short"):
        a, _ = _wgrad(A, pair_a, G, pair_g, k_off, lay[name], Cin, Cout)
        b, _ = _wgrad(A, pair_a, G, pair_g, k_off, lay[name], Cin, Cout)
        assert torch.equal(a, b), f"{Cin}->{Cout} layout {name}: two calls differ"


def _row_of_one_offset(pairs, k_off):
    """(row, offset): a row that the pairs of exactly one offset reference"""
    pairs = pairs.cpu().numpy()
    owner = {}
    for k in range(len(k_off) - 1):
        for r in np.unique(pairs[k_off[k]:k_off[k + 1]]).tolist():
            owner.setdefault(r, set()).add(k)
    for r in sorted(owner):
        if len(owner[r]) == 1:
            return r, next(iter(owner[r]))
    raise AssertionError("no row is referenced by exactly one offset")


@pytest.mark.parametrize("scene,kind", [("isolated", "k3"), ("line_x129", "s2")])
@pytest.mark.parametrize("Cin,Cout", [(32, 32), (128, 96)])
def test_a_nan_and_an_inf_stay_in_their_offset_and_channel(Cin, Cout, scene, kind):
    """`short` items; isolated: every voxel has its centre pair only; line_x129 under k2 s2: every fine voxel has one
    parent, under one offset.  NaN in channel 3 and Inf in channel 17 of ONE feature row: gW[k] of that row's offset is
    non-finite in rows 3 and 17 and nowhere else, and every other element has the bits of the clean run."""
    cm = _scene(scene)
    pair_a, pair_g, k_off, n_a, n_g = _pairs(cm, kind)
    chunk = _short(k_off, Cin, Cout)
    assert chunk == 24
    g = torch.Generator().manual_seed(3)
    A, G = _dev(torch.randn((n_a, Cin), generator=g)), _dev(torch.randn((n_g, Cout), generator=g))
    assert bool((G != 0).all())
    clean, _ = _wgrad(A, pair_a, G, pair_g, k_off, chunk, Cin, Cout)
    assert bool(torch.isfinite(clean).all())
    row, k = _row_of_one_offset(pair_a, k_off)
    A[row, 3], A[row, 17] = NAN, float("inf")
    got, _ = _wgrad(A, pair_a, G, pair_g, k_off, chunk, Cin, Cout)
    bad = ~torch.isfinite(got)
    want = torch.zeros_like(bad)
    want[k, 3, :] = True
    want[k, 17, :] = True
    assert torch.equal(bad, want), f"{scene} {kind} {Cin}->{Cout}: non-finite elements at {(bad != want).nonzero()[:5].tolist()}"
    assert bool(torch.isnan(got[k, 3]).all())
    assert torch.equal(got[~want], clean[~want])
