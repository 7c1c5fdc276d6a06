"""The narrow-input gathered GEMM (csrc/sconv.hip: k_sconv_gemm_cin8 through lidog_sconv_gemm_addend -- the classifier's
data gradient, 7 -> 96, added onto rows that hold the BEV head's gradient) bit for bit against the two-pass form,
lidog_sconv_gemm followed by lidog_add(addend, product): Cin in {1, 7, 8}, Cout in {4, 96}, with and without a gather and
a scatter index, in place (addend == T) and not, and 0, 1, 127, 128 and 129 rows (the last tile empty, one row, one short
of full, full, and a full tile followed by a one-row tile)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _operands(rows, Cin, Cout, indexed):
    g = torch.Generator().manual_seed(100 * rows + 10 * Cin + Cout + int(indexed))
    a_rows = rows + 5 if indexed else rows
    A = torch.randn((a_rows, Cin), generator=g).cuda()
    W = torch.randn((1, Cin, Cout), generator=g).cuda()
    ad = torch.randn((rows, Cout), generator=g).cuda()
    gather = scatter = None
    if indexed:
        gather = torch.randint(0, a_rows, (rows,), generator=g).to(torch.int32).cuda()     # rows read twice, rows never read
        scatter = torch.randperm(rows, generator=g).to(torch.int32).cuda()
    return A, W, ad, gather, scatter


@pytest.mark.parametrize("rows", [0, 1, 127, 128, 129])
@pytest.mark.parametrize("indexed", [False, True], ids=["rows", "gather_scatter"])
@pytest.mark.parametrize("Cout", [4, 96])
@pytest.mark.parametrize("Cin", [1, 7, 8])
def test_gemm_addend_equals_gemm_then_add(Cin, Cout, indexed, rows):
    import lidog_amd.me as ME
    from lidog_amd._lib import call, ptr
    A, W, ad, gather, scatter = _operands(rows, Cin, Cout, indexed)
    m = ME._IdentityMap(rows, "cuda")
    assert m.n_tiles == (rows + 127) // 128
    prod = torch.full((rows, Cout), float("nan"), device="cuda")
    ME._gemm(A, gather, W, None, m, Cin, Cout, prod, scatter)
    want = torch.empty_like(ad)
    call("lidog_add", ptr(ad), ptr(prod), ad.numel(), ptr(want))
    if rows:
        assert bool(torch.isfinite(want).all()) and float(prod.abs().max()) > 0
        # the product itself against float64 (7 products of unit-variance values: a few ulp of the row's magnitude)
        src = gather.long() if indexed else torch.arange(rows, device="cuda")
        dst = scatter.long() if indexed else torch.arange(rows, device="cuda")
        ref = torch.empty((rows, Cout), dtype=torch.float64, device="cuda")
        ref[dst] = A.double()[src] @ W[0].double()
        u = 2.0 ** -24                                   # Cin roundings in the chain: gamma_Cin * sum |a| |w|
        bound = (A.abs().double()[src] @ W[0].abs().double()) * (Cin * u / (1 - Cin * u))
        bound_at = torch.empty_like(ref)
        bound_at[dst] = bound
        assert bool(((prod.double() - ref).abs() <= bound_at).all())
    tiles = (ptr(m.tiles[0]), ptr(m.tiles[1]), ptr(m.tiles[2]), m.n_tiles)
    # out of place: the addend is left alone
    T = torch.full((rows, Cout), float("nan"), device="cuda")
    keep = ad.clone()
    call("lidog_sconv_gemm_addend", ptr(A), ptr(gather), ptr(W), *tiles, Cin, Cout, ptr(ad), ptr(T), ptr(scatter))
    assert torch.equal(T, want) and torch.equal(ad, keep)
    # in place, as the trunk executor calls it
    T = ad.clone()
    call("lidog_sconv_gemm_addend", ptr(A), ptr(gather), ptr(W), *tiles, Cin, Cout, ptr(T), ptr(T), ptr(scatter))
    assert torch.equal(T, want)
