"""The sparse convolution's weight gradient (lidog_sconv_wgrad: csrc/sconv_mfma.hip:k_sconv_wgrad_mfma on the matrix
core, csrc/sconv.hip:k_sconv_wgrad<RM, CN> / _small / _cin1 / _cout8 on the vector core, then k_items_sum{,4}) and the
bias gradient (lidog_colsum) through the C ABI against the float64 yardstick of tests/sparse_ref.py, on both arithmetic
cores, for every (Cin, Cout, kernel) weight of MinkUNet34 plus two generic shapes.

Work-item layouts: what me._wgrad_chunk cuts with ME._WGRAD_FIT = 0, 1, 2 (the slot-fitted cuts depend on the CU count
of the GPU), the smallest chunk (128 pairs), one item per offset, and items shorter than 32 pairs -- all built by
me._wgrad_items_host (pinned on the host by tests/test_hostprep_cpu.py).  Maps: two small scenes, a flat scene (all z
equal: 18 of the 27 offsets are empty and must give exactly 0), and the bench workload (one kitti120k scan at tensor
strides 1 and 2, four scans at stride 1).

Bars (tests/bev_ref.py): exact (integer operands, every partial sum below 2^24: a lost or doubled pair fails it at any
size), precision (per offset, K = P_k), written (gW and the partial-slot workspace pre-filled with NaN).  The module path
(ME.MinkowskiConvolution / Transpose backward, with the weight-gradient lane on and off) meets the exact bar at bench
size."""
import numpy as np
import pytest
import torch

import sparse_ref as R
from helpers import small_batch

pytestmark = pytest.mark.gpu

NAN = float("nan")

# (Cin, Cout, map): every weight of MinkUNet34 (minkunet.py:PLANES) -- k5 stem, k2 s2 downsampling, k3 blocks, k1
# downsample branches, transposed k2 upsampling -- and the generic fallbacks (k_sconv_wgrad_small, odd Cin * Cout:
# k_items_sum)
SHAPES = [
    (1, 32, "k5"), (32, 32, "s2"), (32, 32, "k3"), (32, 64, "k3"), (32, 64, "k1"),
    (64, 64, "s2"), (64, 64, "k3"), (128, 128, "s2"), (128, 128, "k3"),
    (64, 128, "k3"), (64, 128, "k1"), (128, 256, "k3"), (128, 256, "k1"), (256, 256, "k3"),
    (256, 256, "tr"), (256, 128, "tr"), (384, 256, "k3"), (384, 256, "k1"), (192, 128, "k3"), (192, 128, "k1"),
    (128, 96, "k3"), (128, 96, "k1"), (128, 96, "tr"), (96, 96, "k3"), (96, 96, "tr"), (96, 7, "k1"),
    (20, 12, "k3"), (5, 7, "k3"),
]
_SCENES = {}


@pytest.fixture(params=[1, 0], ids=["mfma_f32", "vector_fma"])
def sparse_core(request, monkeypatch):
    """both arithmetic cores; the slot counts me._wgrad_chunk reads depend on the core, so their cache is private here"""
    import lidog_amd.me as ME
    from lidog_amd import _lib
    L = _lib.load()
    monkeypatch.setattr(ME, "_wgrad_slots_cache", {})
    assert L.lidog_set_sparse_core(request.param) == 0
    yield request.param
    L.lidog_set_sparse_core(1)


def _fill(shape, value, dtype=torch.float32):
    """every output and workspace the tests own; value None: uninitialised (torch.empty)"""
    if value is None:
        return torch.empty(shape, dtype=dtype, device="cuda")
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _dev(t):
    """every float operand the tests own"""
    return t.cuda()


def _scene(name):
    """coordinate manager of a scene, cached per module (the bench maps are built once)"""
    if name not in _SCENES:
        import lidog_amd.me as ME
        from lidog_amd import synth
        if name == "small":
            c = small_batch((0, 1), n_points=2500)
        elif name == "flat":
            c = small_batch((2,), n_points=2500).clone()
            c[:, 3] = 0
            c = torch.unique(c, dim=0)
        elif name == "bench1":
            c = synth.make_batch((0,), "kitti120k", "cpu")["coords_int"]
        else:
            c = synth.make_batch((0, 1, 2, 3), "kitti120k", "cpu")["coords_int"]
        st = ME.SparseTensor(coordinates=c.cuda(), features=torch.ones((c.shape[0], 1), device="cuda"))
        _SCENES[name] = st.coordinate_manager
    return _SCENES[name]


def _pairs(cm, kind, s=1):
    """(pair_a, pair_g, k_off_host, n_a, n_g) of the weight gradient gW[k] = sum A[pair_a]^T G[pair_g] of a convolution
    of kind k5 / k3 / k1 / s2 / tr on the map of tensor stride s (tr: from stride 2 s back to s)"""
    if kind == "k1":
        n = cm.maps[s].n
        r = torch.arange(n, dtype=torch.int32, device="cuda")
        return r, r, [0, n], n, n
    if kind in ("k3", "k5"):
        m = cm.kernel_map(s, s, 3 if kind == "k3" else 5)
        return m.pair_in, m.pair_out, list(m.k_off_host), m.n_in, m.n_out
    cm.stride(s, 2 * s)
    m = cm.kernel_map(s, 2 * s, 2)
    if kind == "s2":
        return m.pair_in, m.pair_out, list(m.k_off_host), m.n_in, m.n_out
    return m.pair_out, m.pair_in, list(m.k_off_host), m.n_out, m.n_in     # transposed: in / out exchanged


def _layouts(k_off, Cin, Cout, monkeypatch, which):
    """{name: chunk} of the work-item cuts to run"""
    import lidog_amd.me as ME
    P_k = np.diff(np.asarray(k_off, dtype=np.int64))
    out = {}
    default = ME._WGRAD_FIT
    for fit in (0, 1, 2):
        monkeypatch.setattr(ME, "_WGRAD_FIT", fit)   # read once at import: the attribute, not the environment
        out[f"fit{fit}"] = ME._wgrad_chunk(k_off, Cin, Cout)
    monkeypatch.setattr(ME, "_WGRAD_FIT", default)
    if which == "all":
        out["c128"] = 128
        out["one_per_offset"] = max(128, int(P_k.max()))
        # items of 24 pairs (every one shorter than 32), as long as the partial slots stay below 512 MB
        short = 24
        while (int(P_k.sum()) // short + len(P_k)) * Cin * Cout * 4 * 4 > 512 << 20:
            short *= 2
        out["short"] = short
    return out


def _wgrad(A, pair_a, G, pair_g, k_off, chunk, Cin, Cout):
    """lidog_sconv_wgrad with the items of me._wgrad_items_host(k_off, chunk); gW and the partial slots pre-filled
    with NaN"""
    import lidog_amd.me as ME
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    items, n_items, item_off = ME._wgrad_items_host(k_off, chunk)
    K = len(k_off) - 1
    items = torch.from_numpy(np.ascontiguousarray(items)).cuda()
    item_off = torch.from_numpy(item_off).cuda()
    slabs = _lib.load().lidog_sconv_wgrad_slabs(Cin, Cout, n_items)
    partial = _fill((max(slabs, 1), Cin, Cout), NAN)
    gW = _fill((K, Cin, Cout), NAN)
    call("lidog_sconv_wgrad", ptr(A), ptr(pair_a), ptr(G), ptr(pair_g), ptr(items), n_items, ptr(item_off), K, Cin, Cout,
         ptr(partial), ptr(gW))
    torch.cuda.synchronize()
    return gW, n_items


def _operands(n_a, n_g, Cin, Cout, seed, exact, P_max):
    g = torch.Generator().manual_seed(seed)
    if exact:
        # |a|, |g| <= 3 with half of them zero: sum |terms| of the largest offset ~ 0.7 P_k, below 2^24 up to the
        # bs-4 centre offset (~2.1 M pairs); small maps get wider operands
        hi = 3 if P_max > 200000 else 15
        return (_dev(R.exact_operands((n_a, Cin), g, -hi, hi, 0.5, "cuda")),
                _dev(R.exact_operands((n_g, Cout), g, -hi, hi, 0.5, "cuda")))
    return _dev(torch.randn((n_a, Cin), generator=g)), _dev(torch.randn((n_g, Cout), generator=g))


def _check_all(cm, kind, Cin, Cout, layouts, record_property, tag, s=1, precision=True):
    pair_a, pair_g, k_off, n_a, n_g = _pairs(cm, kind, s)
    P_max = int(np.diff(np.asarray(k_off)).max())
    worst = [0.0, 0.0]
    for exact in ((True, False) if precision else (True,)):
        A, G = _operands(n_a, n_g, Cin, Cout, Cin * 131 + Cout * 7 + len(kind), exact, P_max)
        ref, ab, P_k = R.wgrad64(A.double(), pair_a, G.double(), pair_g, k_off)
        for name, chunk in layouts.items():
            got, n_items = _wgrad(A, pair_a, G, pair_g, k_off, chunk, Cin, Cout)
            what = f"{tag} {Cin}->{Cout} {kind} layout {name} (chunk {chunk}, {n_items} items)"
            if exact:
                R.assert_exact(got, ref, ab, what)
            else:
                e, f = R.assert_wgrad_precision(got, ref, ab, P_k, what)
                worst = [max(worst[0], e), max(worst[1], f)]
    if precision:
        record_property("worst_elem", worst[0])
        record_property("worst_fro", worst[1])
    return k_off


@pytest.mark.parametrize("Cin,Cout,kind", SHAPES, ids=[f"{a}x{b}_{k}" for a, b, k in SHAPES])
def test_weight_gradient_vs_float64_on_small_scenes(Cin, Cout, kind, sparse_core, monkeypatch, record_property):
    cm = _scene("small")
    k_off = _pairs(cm, kind)[2]
    _check_all(cm, kind, Cin, Cout, _layouts(k_off, Cin, Cout, monkeypatch, "all"), record_property, "small")


@pytest.mark.parametrize("Cin,Cout", [(32, 32), (96, 96), (256, 256), (20, 12), (5, 7)])
def test_empty_offsets_of_a_flat_scene_give_zero(Cin, Cout, sparse_core, monkeypatch, record_property):
    cm = _scene("flat")
    m = cm.kernel_map(1, 1, 3)
    P_k = np.diff(np.asarray(m.k_off_host))
    assert (P_k == 0).sum() == 18, "the flat scene should leave the 18 offsets with dz != 0 empty"
    _check_all(cm, "k3", Cin, Cout, _layouts(list(m.k_off_host), Cin, Cout, monkeypatch, "all"), record_property, "flat")


# bench maps: the layouts the bench runs (fitted to the GPU's slots or not), one item per offset and 128-pair items
BENCH = [(1, 32, 32, "k3"), (1, 96, 96, "k3"), (1, 1, 32, "k5"), (1, 32, 32, "s2"), (2, 64, 64, "k3"),
         (2, 128, 96, "tr")]


def _bench_layouts(k_off, Cin, Cout, monkeypatch):
    lay = _layouts(k_off, Cin, Cout, monkeypatch, "fit")
    lay["one_per_offset"] = int(np.diff(np.asarray(k_off, dtype=np.int64)).max())
    lay["c128"] = 128
    return lay


@pytest.mark.parametrize("s,Cin,Cout,kind", BENCH, ids=[f"s{s}_{b}x{c}_{k}" for s, b, c, k in BENCH])
def test_weight_gradient_vs_float64_on_a_bench_scan(s, Cin, Cout, kind, sparse_core, monkeypatch, record_property):
    cm = _scene("bench1")
    k_off = _pairs(cm, kind, s)[2]
    _check_all(cm, kind, Cin, Cout, _bench_layouts(k_off, Cin, Cout, monkeypatch), record_property, "bench1", s=s)


def test_weight_gradient_exact_on_a_bs4_bench_batch(monkeypatch, record_property):
    """the largest rule book of the bench (four scans, stride 1, 3^3) on the matrix core the bench runs"""
    from lidog_amd import _lib
    assert _lib.load().lidog_get_sparse_core() == 1
    cm = _scene("bench4")
    k_off = _pairs(cm, "k3")[2]
    _check_all(cm, "k3", 96, 96, _bench_layouts(k_off, 96, 96, monkeypatch), record_property, "bench4",
               precision=False)


@pytest.mark.parametrize("scene", ["small", "bench1"])
@pytest.mark.parametrize("C", [7, 16, 32, 96, 256])
def test_bias_gradient_colsum_vs_float64(scene, C, record_property):
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    n = 5003 if scene == "small" else _scene("bench1").maps[1].n
    g = torch.Generator().manual_seed(C + n)
    for exact in (True, False):
        x = _dev(R.exact_operands((n, C), g, -50, 50, 0.3, "cuda") if exact else torch.randn((n, C), generator=g))
        ref, ab = R.colsum64(x.double())
        ws = _fill((_lib.load().lidog_colsum_ws(C),), None, torch.float64)
        out = _fill((C,), NAN)
        call("lidog_colsum", ptr(x), n, C, ptr(out), ptr(ws))
        torch.cuda.synchronize()
        if exact:
            R.assert_exact(out, ref, ab, f"colsum {n}x{C}")
        else:
            # double accumulation, one fp32 rounding at the end: within 1 ulp of the float64 sum (+ gamma_n, negligible)
            err = (out.double() - ref).abs()
            bar = R.ulp32(ref) + R.sums_bar(n, ab)
            r = float((err / bar).max())
            record_property("worst_ulp_ratio", r)
            assert r <= 1.0, f"colsum {n}x{C}: {r:.3g} x (1 ulp + gamma_n) (NaN: never written)"


def test_module_backward_at_bench_size_with_the_lane_on_and_off():
    """ME.MinkowskiConvolution 96 -> 96 k3 and a transposed 256 -> 128 k2 on the bench scan: the weight gradient written
    into the optimiser's flat buffer (on the second stream when the lane is on; the item cuts differ) meets the exact
    bar"""
    import lidog_amd.me as ME
    from lidog_amd.optim import FlatParams
    cm = _scene("bench1")
    cm.stride(1, 2)
    g = torch.Generator().manual_seed(11)
    was = ME._WgradLane.enabled
    try:
        for lane in (True, False):
            ME.set_backward_overlap(lane)
            for Cin, Cout, tr in ((96, 96, False), (256, 128, True)):
                if tr:
                    conv = ME.MinkowskiConvolutionTranspose(Cin, Cout, kernel_size=2, stride=2, dimension=3).cuda()
                else:
                    conv = ME.MinkowskiConvolution(Cin, Cout, kernel_size=3, stride=1, dimension=3).cuda()
                flat = FlatParams(conv)
                flat.zero_grad()
                flat.grad.fill_(NAN)
                s_in = 2 if tr else 1
                n_in = cm.maps[s_in].n
                x = R.exact_operands((n_in, Cin), g, -3, 3, 0.5, "cuda")
                st = ME.SparseTensor(x, coordinate_manager=cm, coordinate_map_key=s_in)
                out = conv(st)
                gy = R.exact_operands((out.F.shape[0], Cout), g, -3, 3, 0.5, "cuda")
                out.F.backward(gy)
                torch.cuda.synchronize()
                pair_a, pair_g, k_off, _, _ = _pairs(cm, "tr" if tr else "k3", 1)
                ref, ab, _ = R.wgrad64(x.double(), pair_a, gy.double(), pair_g, k_off)
                got = conv.kernel.grad.view(ref.shape)
                R.assert_exact(got, ref, ab, f"module {Cin}->{Cout} {'tr' if tr else 'k3'} lane {'on' if lane else 'off'}")
    finally:
        ME.set_backward_overlap(was)
