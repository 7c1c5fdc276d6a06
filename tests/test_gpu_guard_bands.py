"""The hot-path kernels under tests/guard.py: the C-ABI tests of ten modules run again, unchanged, with every output,
product-row buffer, workspace and float operand they own inside a GuardArena -- payloads 16-byte aligned and no more,
NaN / sentinel bands on both sides, the band after a payload as long as one padded 128-row tile of its rows.  Every bar
of the re-run function still applies (the float64 bounds, the exact equalities, the NaN-written checks); on top of it,
no band may have changed when the function returns: a store past the end of an output or a workspace, a `*_ws()`
function that reports too little, fails here with the buffer's name.  A load past the end of a float operand reads a
NaN, which the finiteness checks of the re-run function see.

Each test body runs inside `guarded(...)`, which points the module's allocation hooks (_nan, _fill, _dev) at a fresh
arena and checks it on exit: no test can forget the check.

Cases are the smallest shapes at which a tile tail, a row-block tail or a workspace can go wrong; none is bench size.
The small row operators no re-run reaches (lidog_cat2, lidog_split2, lidog_relu_fwd, lidog_relu_bwd, lidog_add) are
compared bit for bit with their torch expression at the ends of a 256-thread block.

test_the_check_sees_a_stray_store is the one deliberate overrun: one element, read from the input's own band and
stored into the output's own band, both inside the arena's allocations."""
import contextlib

import pytest
import torch

import inorm_ref as IR
import sconv_ref as R
import test_gpu_bev_pool_edge as V
import test_gpu_bf16 as B
import test_gpu_bf16_wgrad as BW
import test_gpu_bn_rows64 as N
import test_gpu_conv2d as C2
import test_gpu_field as F
import test_gpu_inorm64 as I
import test_gpu_pool as P
import test_gpu_sconv_edge64 as E
import test_gpu_sconv_wgrad64 as W
from guard import GuardArena, GuardError

pytestmark = pytest.mark.gpu

NAN = float("nan")


# ------------------------------------------------------------------ the arena under a module's hooks
@contextlib.contextmanager
def guarded(monkeypatch, what, *modules):
    """point _nan / _fill / _dev of `modules` at a fresh arena; check every band when the body returns"""
    arena = GuardArena("cuda")
    for M in modules:
        if hasattr(M, "_nan"):
            monkeypatch.setattr(M, "_nan", arena.nan)
        if hasattr(M, "_fill"):
            monkeypatch.setattr(M, "_fill", lambda shape, value, dtype=torch.float32: arena.full(shape, value, dtype))
        if hasattr(M, "_dev"):     # test_gpu_pool / test_gpu_field pass a column count
            monkeypatch.setattr(M, "_dev", lambda t, C=None: arena.place(t if C is None else t[:, :C]))
    try:
        yield arena
        assert arena.slots, f"{what}: no buffer went through the arena (the hooks are not in use)"
        arena.check(what)
    finally:
        arena.reset()


@pytest.fixture(autouse=True)
def _restore_switches():
    """test_gpu_sconv_edge64's autouse fixture does not follow its functions here"""
    from lidog_amd import _lib
    yield
    L = _lib.load()
    L.lidog_set_sparse_core(1)
    L.lidog_sconv_gemm_units(1, 0)


@pytest.fixture(params=[1, 0], ids=["mfma_f32", "vector_fma"])
def sparse_core(request, monkeypatch):
    """test_gpu_sconv_wgrad64's fixture: both cores, with a private cache of the slot counts me._wgrad_chunk reads"""
    import lidog_amd.me as ME
    from lidog_amd import _lib
    L = _lib.load()
    monkeypatch.setattr(ME, "_wgrad_slots_cache", {})
    assert L.lidog_set_sparse_core(request.param) == 0
    yield request.param
    L.lidog_set_sparse_core(1)


def _ids(cases):
    return ["-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c) for c in cases]


# ------------------------------------------------------------------ sparse convolution: forward, data gradient, epilogues
# one shape per kernel family: MFMA, non-square MFMA, _cout8, _small, _cin8, generic
FAMILIES = [(32, 32), (128, 96), (96, 7), (5, 7), (1, 32), (20, 12)]
TINY = ("tiny_1", "tiny_127", "tiny_128", "tiny_129", "line_x129", "isolated")
FWD = [(s, a, b) for s in TINY for a, b in FAMILIES]


@pytest.mark.parametrize("name,Cin,Cout", FWD, ids=[f"{s}-{a}x{b}" for s, a, b in FWD])
def test_sconv_forward_and_data_gradient(name, Cin, Cout, record_property, monkeypatch):
    with guarded(monkeypatch, f"sconv {name} {Cin}x{Cout}", E):
        E.test_c_abi_forward_and_data_gradient(name, Cin, Cout, record_property)


EPI = [(s, a, b) for s in ("tiny_129", "line_x129") for a, b in ((32, 32), (128, 96))]


@pytest.mark.parametrize("name,Cin,Cout", EPI, ids=[f"{s}-{a}x{b}" for s, a, b in EPI])
def test_sconv_fused_epilogues(name, Cin, Cout, record_property, monkeypatch):
    with guarded(monkeypatch, f"epilogues {name} {Cin}x{Cout}", E):
        E.test_fused_epilogues(name, Cin, Cout, record_property)


@pytest.mark.parametrize("C", [16, 32, 64])
@pytest.mark.parametrize("name", ["tiny_1", "tiny_129", "line_x129"])
def test_sconv_stem(name, C, record_property, monkeypatch):
    with guarded(monkeypatch, f"stem {name} 1x{C}", E):
        E.test_stem_cin1_against_the_two_pass_path(name, C, record_property)


@pytest.mark.parametrize("Cin,Cout", [(32, 32), (20, 12), (5, 7)])
def test_sconv_k2_s2_direct_scatter(Cin, Cout, record_property, monkeypatch):
    with guarded(monkeypatch, f"k2 s2 scatter isolated {Cin}x{Cout}", E):
        E.test_k2_s2_direct_scatter_writes_every_row("isolated", Cin, Cout, record_property)


@pytest.mark.parametrize("name", ["tiny_129", "line_x129"])
def test_sconv_gemm_addend_in_place(name, record_property, monkeypatch):
    with guarded(monkeypatch, f"gemm_addend {name}", E):
        E.test_gemm_addend_in_place(name, record_property)


# ------------------------------------------------------------------ sparse convolution: weight gradient, bias gradient
@pytest.mark.parametrize("Cin,Cout,kind", W.SHAPES, ids=[f"{a}x{b}_{k}" for a, b, k in W.SHAPES])
def test_wgrad_on_small_scenes(Cin, Cout, kind, sparse_core, monkeypatch, record_property):
    with guarded(monkeypatch, f"wgrad small {Cin}x{Cout} {kind} core {sparse_core}", W):
        W.test_weight_gradient_vs_float64_on_small_scenes(Cin, Cout, kind, sparse_core, monkeypatch, record_property)


@pytest.mark.parametrize("Cin,Cout", [(32, 32), (96, 96), (256, 256), (20, 12), (5, 7)])
def test_wgrad_empty_offsets(Cin, Cout, sparse_core, monkeypatch, record_property):
    with guarded(monkeypatch, f"wgrad flat {Cin}x{Cout} core {sparse_core}", W):
        W.test_empty_offsets_of_a_flat_scene_give_zero(Cin, Cout, sparse_core, monkeypatch, record_property)


@pytest.mark.parametrize("C", [7, 16, 32, 96, 256])
def test_bias_gradient_colsum(C, record_property, monkeypatch):
    with guarded(monkeypatch, f"colsum small C{C}", W):
        W.test_bias_gradient_colsum_vs_float64("small", C, record_property)


# ------------------------------------------------------------------ bf16 paths
def test_bf16_pack(monkeypatch):
    with guarded(monkeypatch, "bf16 pack", B):
        B.test_pack_is_bit_equal_to_torch_rounding()


BF_SCENES = ("tiny_1", "tiny_129", "line_x129", "isolated")


@pytest.mark.parametrize("Cin,Cout", B.GEMM_SHAPES, ids=[f"{a}x{b}" for a, b in B.GEMM_SHAPES])
@pytest.mark.parametrize("name", [s for s in BF_SCENES if s in B.GEMM_SCENES])
def test_bf16_gathered_gemm(name, Cin, Cout, record_property, monkeypatch):
    with guarded(monkeypatch, f"bf16 gemm {name} {Cin}x{Cout}", B):
        B.test_gathered_gemm_against_float64_of_the_rounded_operands(name, Cin, Cout, record_property)


@pytest.mark.parametrize("Cin,Cout", B.OS_SHAPES, ids=[f"{a}x{b}" for a, b in B.OS_SHAPES])
@pytest.mark.parametrize("name", [s for s in BF_SCENES if s in B.OS_SCENES])
def test_bf16_output_stationary(name, Cin, Cout, record_property, monkeypatch):
    with guarded(monkeypatch, f"bf16 os {name} {Cin}x{Cout}", B):
        B.test_output_stationary_form_against_float64(name, Cin, Cout, record_property)


@pytest.mark.parametrize("kind", ["k3", "s2"])
@pytest.mark.parametrize("Cin,Cout", BW.SHAPES, ids=[f"{a}x{b}" for a, b in BW.SHAPES])
def test_bf16_wgrad_on_small_scenes(Cin, Cout, kind, monkeypatch, record_property):
    with guarded(monkeypatch, f"bf16 wgrad small {Cin}x{Cout} {kind}", BW):
        BW.test_weight_gradient_vs_float64_on_small_scenes(Cin, Cout, kind, monkeypatch, record_property)


# ------------------------------------------------------------------ BatchNorm over rows, instance norm
BN = [(C, n) for C in (1, 7, 4, 12, 96, 256) for n in (1, 2, N.RB96 - 1, N.RB96, N.RB96 + 1)]


@pytest.mark.parametrize("C,n", BN, ids=[f"C{c}_n{n}" for c, n in BN])
def test_row_batchnorm(C, n, record_property, monkeypatch):
    with guarded(monkeypatch, f"row BatchNorm C{C} n{n}", N):
        N.test_row_batchnorm_vs_float64(C, n, record_property)


@pytest.mark.parametrize("residual", [True, False], ids=["residual", "no_residual"])
@pytest.mark.parametrize("rows", [0, 1, 70])
@pytest.mark.parametrize("C", [8, 96])
def test_row_batchnorm_sync_apply(C, rows, residual, monkeypatch):
    with guarded(monkeypatch, f"bn_apply_sync C{C} rows {rows} residual {residual}", N):
        N.test_sync_apply_equals_finalize_then_apply_bit_for_bit(C, rows, residual)


IN_LAYOUTS = [lay for lay in IR.LAYOUTS if sum(lay["sizes"]) < 10000]


@pytest.mark.parametrize("lay", IN_LAYOUTS, ids=[lay["id"] for lay in IN_LAYOUTS])
def test_instance_norm_and_ibn(lay, record_property, monkeypatch):
    with guarded(monkeypatch, f"instance norm {lay['id']}", I):
        I.test_instance_norm_and_ibn_entries_vs_float64(lay, record_property)


# ------------------------------------------------------------------ pooling
POOL_SCENES = ("tiny_129", "dense_cube_odd", "twin_scans", "one_and_many")


@pytest.mark.parametrize("kind", P.FWD_KINDS)
@pytest.mark.parametrize("name", [s for s in POOL_SCENES if s in P.SCENES])
def test_pool_local_forward(name, kind, record_property, monkeypatch):
    with guarded(monkeypatch, f"pool forward {name} {kind}", P):
        P.test_local_forward_against_float64(name, kind, record_property)


@pytest.mark.parametrize("kind", P.BWD_KINDS)
@pytest.mark.parametrize("name", [s for s in POOL_SCENES if s in P.SCENES])
def test_pool_local_backward(name, kind, record_property, monkeypatch):
    with guarded(monkeypatch, f"pool backward {name} {kind}", P):
        P.test_local_backward_against_float64(name, kind, record_property)


@pytest.mark.parametrize("C", (1, 4, 100))
def test_pool_rows_without_pairs(C, monkeypatch):
    with guarded(monkeypatch, f"pool doctored lists C{C}", P):
        P.test_rows_without_pairs_and_all_minus_inf(C)


@pytest.mark.parametrize("name", [s for s in POOL_SCENES if s in ("twin_scans", "one_and_many", "source8k_x4")])
def test_pool_global(name, record_property, monkeypatch):
    with guarded(monkeypatch, f"global pooling {name}", P):
        P.test_global_pooling_against_float64(name, record_property)


# ------------------------------------------------------------------ field kernels
@pytest.mark.parametrize("s", F.STRIDES)
def test_field_floor(s, monkeypatch):
    with guarded(monkeypatch, f"field floor stride {s}", F):
        F.test_floor_against_the_yardstick(s)


@pytest.mark.parametrize("s", F.STRIDES)
@pytest.mark.parametrize("name", [s for s in F.SCENES if R.scene(s).shape[0] <= 10000])
def test_field_interpolation(name, s, monkeypatch):
    with guarded(monkeypatch, f"interpolation {name} stride {s}", F):
        F.test_interpolation_against_float64(name, s)


@pytest.mark.parametrize("n,hot", [(c, 0) for c in F.COUNTS] + [(257, 300)])
def test_field_lists_reduce_gather(n, hot, monkeypatch):
    with guarded(monkeypatch, f"field lists n {n} hot {hot}", F):
        F.test_field_lists_reduce_gather(n, hot)


# ------------------------------------------------------------------ the BEV head: conv2d and the projection's pooling
K3 = C2.K3_CASES[:5] + [(2, 32, 17, 9, 8, None)]
SPARSE = [c for c in C2.SPARSE_CASES if c[2] * c[3] <= 4096]


@pytest.mark.parametrize("kind", ["exact", "precise"])
@pytest.mark.parametrize("B_,Cin,H,Wd,Cout,ws_slabs", K3, ids=_ids(K3))
def test_conv2d_k3s2(B_, Cin, H, Wd, Cout, ws_slabs, kind, record_property, monkeypatch):
    with guarded(monkeypatch, f"conv2d k3 s2 {B_, Cin, H, Wd, Cout} {kind}", C2):
        C2.test_conv2d_k3s2_kernels_vs_float64(B_, Cin, H, Wd, Cout, ws_slabs, kind, record_property)


@pytest.mark.parametrize("kind", ["exact", "precise"])
@pytest.mark.parametrize("B_,Cin,H,Wd,Cout,bias", C2.PW_CASES[:4], ids=_ids(C2.PW_CASES[:4]))
def test_conv2d_1x1(B_, Cin, H, Wd, Cout, bias, kind, record_property, monkeypatch):
    with guarded(monkeypatch, f"conv2d 1x1 {B_, Cin, H, Wd, Cout} {kind}", C2):
        C2.test_conv2d_1x1_kernels_vs_float64(B_, Cin, H, Wd, Cout, bias, kind, record_property)


@pytest.mark.parametrize("kind", ["exact", "precise"])
@pytest.mark.parametrize("B_,Cin,H,Wd,Cout,pattern", SPARSE, ids=_ids(SPARSE))
def test_conv2d_over_support(B_, Cin, H, Wd, Cout, pattern, kind, record_property, monkeypatch):
    with guarded(monkeypatch, f"conv2d over support {B_, Cin, H, Wd, Cout} {pattern} {kind}", C2):
        C2.test_conv2d_over_support_vs_float64(B_, Cin, H, Wd, Cout, pattern, kind, record_property)


@pytest.mark.parametrize("Cin", [1, 96, 128])
def test_conv2d_over_support_of_an_empty_batch(Cin, monkeypatch):
    with guarded(monkeypatch, f"conv2d over support, empty batch, Cin {Cin}", C2):
        C2.test_conv2d_over_support_of_an_empty_batch(Cin)


@pytest.mark.parametrize("B_", [1, 3])
@pytest.mark.parametrize("pool", V.POOLS, ids=lambda p: "k%ds%dp%d" % p)
@pytest.mark.parametrize("C", [4, 7, 96])
def test_bev_pool(C, pool, B_, monkeypatch):
    with guarded(monkeypatch, f"bev pool C{C} {pool} B{B_}", V):
        V.test_pool_bits_match_reference(C, pool, B_, monkeypatch)


def test_bev_pool_pixel_over_more_than_four_viewed_rows(monkeypatch):
    with guarded(monkeypatch, "bev pool C250", V):
        V.test_pool_pixel_over_more_than_four_viewed_rows(monkeypatch)


@pytest.mark.parametrize("pool", [(5, 3, 1), (3, 2, 1), (8, 3, 4)], ids=lambda p: "k%ds%dp%d" % p)
@pytest.mark.parametrize("C", [7, 96])
def test_bev_pool_inf_nan_ties(C, pool, monkeypatch):
    with guarded(monkeypatch, f"bev pool inf / nan / ties C{C} {pool}", V):
        V.test_pool_inf_nan_ties(C, pool, monkeypatch)


@pytest.mark.parametrize("rowbits", [True, False])
@pytest.mark.parametrize("n", [0, 1, 3])
def test_bev_pool_no_row_one_row_last_pixel(n, rowbits, monkeypatch):
    with guarded(monkeypatch, f"bev pool {n} rows, row bitmasks {rowbits}", V):
        V.test_no_row_one_row_last_pixel(n, rowbits, monkeypatch)


# ------------------------------------------------------------------ the small row operators, directly
ROWS = (1, 255, 256, 257)          # around one 256-thread block


def _randn(arena, *shape, seed):
    """random rows with zeros, negative zeros and a NaN among them (max(NaN, 0) and NaN > 0 take a side)"""
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    flat = x.view(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    if flat.numel() > 5:
        flat[5] = NAN
    return arena.place(x)


def _same_bits(got, want, what):
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32)), what


@pytest.mark.parametrize("Ca,Cb", [(4, 4), (32, 96), (96, 32)])
@pytest.mark.parametrize("n", ROWS)
def test_cat2_and_split2(n, Ca, Cb, monkeypatch):
    from lidog_amd._lib import call, ptr
    with guarded(monkeypatch, f"cat2 / split2 n {n} {Ca}+{Cb}") as arena:
        a, b = _randn(arena, n, Ca, seed=n + Ca), _randn(arena, n, Cb, seed=n + Cb + 1)
        out = arena.nan(n, Ca + Cb, name="cat2 out")
        call("lidog_cat2", ptr(a), Ca, ptr(b), Cb, n, ptr(out))
        torch.cuda.synchronize()
        _same_bits(out, torch.cat([a, b], dim=1), "lidog_cat2")
        g = _randn(arena, n, Ca + Cb, seed=n + 2)
        ga, gb = arena.nan(n, Ca, name="split2 ga"), arena.nan(n, Cb, name="split2 gb")
        call("lidog_split2", ptr(g), Ca, Cb, n, ptr(ga), ptr(gb))
        torch.cuda.synchronize()
        _same_bits(ga, g[:, :Ca], "lidog_split2 ga")
        _same_bits(gb, g[:, Ca:], "lidog_split2 gb")


@pytest.mark.parametrize("C", [1, 4, 7])
@pytest.mark.parametrize("n", ROWS)
def test_relu_and_add(n, C, monkeypatch):
    """ReLU as the kernels define it: y = fmaxf(x, 0) (a NaN gives 0, -0.0 may give either zero: compared as values
    there), dx = y > 0 ? dy : 0; out = a + b"""
    from lidog_amd._lib import call, ptr
    with guarded(monkeypatch, f"relu / add n {n} C {C}") as arena:
        x, dy, b = (_randn(arena, n, C, seed=n * 8 + C + k) for k in range(3))
        y = arena.nan(n, C, name="relu_fwd y")
        call("lidog_relu_fwd", ptr(x), n * C, ptr(y))
        torch.cuda.synchronize()
        want = torch.where(x > 0, x, torch.zeros_like(x))
        assert torch.equal(y, want) and bool(torch.isfinite(y).all()), "lidog_relu_fwd"
        assert torch.equal(y.view(torch.int32)[x > 0], x.view(torch.int32)[x > 0]), "lidog_relu_fwd: bits of the positives"
        dx = arena.nan(n, C, name="relu_bwd dx")
        call("lidog_relu_bwd", ptr(dy), ptr(y), n * C, ptr(dx))
        torch.cuda.synchronize()
        _same_bits(dx, torch.where(y > 0, dy, torch.zeros_like(dy)), "lidog_relu_bwd")
        out = arena.nan(n, C, name="add out")
        call("lidog_add", ptr(x), ptr(b), n * C, ptr(out))
        torch.cuda.synchronize()
        _same_bits(out, x + b, "lidog_add")


# ------------------------------------------------------------------ the check sees a stray store
def test_the_check_sees_a_stray_store():
    """lidog_relu_fwd over n + 1 elements of two n-element arena buffers: the extra element is read from the input's
    NaN band and stored (as 0) into the band after the output -- both inside the arena's own allocations, nothing
    leaves allocated memory.  The check must raise and name the output, the side and offset 0."""
    from lidog_amd._lib import call, ptr
    n = 1000
    arena = GuardArena("cuda")
    x = arena.place(torch.randn(n, generator=torch.Generator().manual_seed(1)), name="relu input")
    y = arena.nan(n, name="relu output")
    arena.check("before the call")
    call("lidog_relu_fwd", ptr(x), n + 1, ptr(y))
    with pytest.raises(GuardError) as e:
        arena.check("one element too many")
    assert e.value.findings == [(arena.slots[1].name, "after", 0, 4)]
    msg = str(e.value)
    assert "relu output" in msg and "band after" in msg and "offset 0 " in msg and "relu input" not in msg
    assert torch.equal(y, x.clamp(min=0))
    arena.reset()
