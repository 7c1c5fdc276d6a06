"""tests/sparse_ref.py against independent float64 computations, and its bars against perturbed references:
wgrad64 over the CPU oracle's kernel maps (3^3 s1, 2^3 s2, transposed 2^3, the 5^3 stem) equals autograd of
F.conv3d / F.conv_transpose3d on the densified voxel grid; the row BatchNorm wrappers equal torch's BatchNorm1d in
float64; the precision bar rejects a weight gradient with one pair left out and one from tf32-rounded operands, the
sums bar rejects BatchNorm sums with one row left out."""
import pytest
import torch
import torch.nn.functional as F

import sparse_ref as R

DIMS = (12, 12, 8)     # voxel box (multiples of 4: stride-2 cells do not straddle its edge)


def _coords(seed, density=0.3, batches=2):
    """unique voxels of a random occupancy of the box, coords int32 [n, 4] (batch first), shuffled"""
    g = torch.Generator().manual_seed(seed)
    occ = torch.rand((batches,) + DIMS, generator=g) < density
    c = occ.nonzero().to(torch.int32)
    return c[torch.randperm(c.shape[0], generator=g)].contiguous()


def _dense(rows, coords, stride, dims):
    """[B, C, X, Y, Z] grid at `stride` holding the rows at their voxels (zero elsewhere)"""
    B = int(coords[:, 0].max()) + 1
    d = torch.zeros((B, rows.shape[1]) + tuple(v // stride for v in dims), dtype=rows.dtype)
    c = coords.long()
    d[c[:, 0], :, c[:, 1] // stride, c[:, 2] // stride, c[:, 3] // stride] = rows
    return d


def _cm(coords):
    import oracle.me_cpu as OME
    st = OME.SparseTensor(coordinates=coords, features=torch.ones(coords.shape[0], 1))
    return st.coordinate_manager


def _dense_wgrad(kind, x, c_in, c_out, gy, ks):
    """gW [K, Cin, Cout] from autograd of the dense convolution; offset k = ix + ks iy + ks^2 iz (oracle order)"""
    xd = _dense(x, c_in, 2 if kind == "tr" else 1, DIMS)
    gd = _dense(gy, c_out, 2 if kind == "s2" else 1, DIMS)
    Cin, Cout = x.shape[1], gy.shape[1]
    if kind == "tr":   # weight [Cin, Cout, kx, ky, kz]
        w = torch.zeros((Cin, Cout, ks, ks, ks), dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose3d(xd, w, stride=2)
    else:              # weight [Cout, Cin, kx, ky, kz]
        w = torch.zeros((Cout, Cin, ks, ks, ks), dtype=torch.float64, requires_grad=True)
        y = F.conv3d(xd, w, stride=2 if kind == "s2" else 1, padding=ks // 2 if ks % 2 else 0)
    assert y.shape == gd.shape
    (y * gd).sum().backward()
    gw = w.grad if kind == "tr" else w.grad.transpose(0, 1)        # [Cin, Cout, kx, ky, kz]
    return gw.permute(4, 3, 2, 0, 1).reshape(ks ** 3, Cin, Cout)   # k = ix + ks iy + ks^2 iz


# kind, ks: (3^3 s1), (2^3 s2), (transposed 2^3), (5^3 stem)
MAPS = [("s1", 3), ("s2", 2), ("tr", 2), ("s1", 5)]


@pytest.mark.parametrize("kind,ks", MAPS, ids=["k3s1", "k2s2", "tr_k2", "k5_stem"])
def test_wgrad64_equals_autograd_of_the_dense_convolution(kind, ks):
    coords = _coords(ks * 10 + len(kind))
    cm = _cm(coords)
    c1 = cm.maps[1]
    c2 = cm.stride(1, 2)
    g = torch.Generator().manual_seed(ks)
    Cin, Cout = (1, 5) if ks == 5 else (3, 4)
    if kind == "s1":
        k_off, pin, pout, _ = cm.kernel_map(1, 1, ks)
        c_in, c_out, pair_a, pair_g = c1, c1, pin, pout
    elif kind == "s2":
        k_off, pin, pout, _ = cm.kernel_map(1, 2, ks)
        c_in, c_out, pair_a, pair_g = c1, c2, pin, pout
    else:             # transposed: the stride-2 map used with in / out exchanged
        k_off, pfine, pcoarse, _ = cm.kernel_map(1, 2, ks)
        c_in, c_out, pair_a, pair_g = c2, c1, pcoarse, pfine
    x = torch.randn((c_in.shape[0], Cin), generator=g, dtype=torch.float64)
    gy = torch.randn((c_out.shape[0], Cout), generator=g, dtype=torch.float64)
    gW, ab, P_k = R.wgrad64(x, pair_a, gy, pair_g, k_off, chunk=97)     # several chunks per offset
    assert int(P_k.sum()) == int(k_off[-1]) and (P_k > 0).all()
    want = _dense_wgrad(kind, x, c_in, c_out, gy, ks)
    torch.testing.assert_close(gW, want, rtol=1e-12, atol=1e-12)
    want_abs = _dense_wgrad(kind, x.abs(), c_in, c_out, gy.abs(), ks)
    torch.testing.assert_close(ab, want_abs, rtol=1e-12, atol=1e-12)
    # the fp32 product of the definition passes the precision bar per offset
    got32 = R.wgrad64(x.float(), pair_a, gy.float(), pair_g, k_off)[0]
    R.assert_wgrad_precision(got32, gW, ab, P_k, "fp32 wgrad")


def test_precision_bar_rejects_a_lost_pair_and_tf32_operands():
    coords = _coords(7)
    cm = _cm(coords)
    k_off, pin, pout, _ = cm.kernel_map(1, 1, 3)
    n = coords.shape[0]
    g = torch.Generator().manual_seed(1)
    x = torch.randn((n, 8), generator=g).double()
    gy = torch.randn((n, 8), generator=g).double()
    ref, ab, P_k = R.wgrad64(x, pin, gy, pout, k_off)
    # one pair of the centre offset left out
    k = 13
    lost = torch.cat([pin[:int(k_off[k]) + 5], pin[int(k_off[k]) + 6:]]), torch.cat([pout[:int(k_off[k]) + 5],
                                                                                     pout[int(k_off[k]) + 6:]])
    k_lost = k_off.clone()
    k_lost[k + 1:] -= 1
    got = R.wgrad64(x, lost[0], gy, lost[1], k_lost)[0]
    with pytest.raises(AssertionError):
        R.assert_wgrad_precision(got, ref, ab, P_k, "one pair lost")
    # operands rounded to tf32 (10-bit mantissa), products and sums exact
    got = R.wgrad64(R.round_mantissa(x.float()).double(), pin, R.round_mantissa(gy.float()).double(), pout, k_off)[0]
    with pytest.raises(AssertionError):
        R.assert_wgrad_precision(got, ref, ab, P_k, "tf32")
    # the fp32 result itself passes
    R.assert_wgrad_precision(R.wgrad64(x.float(), pin, gy.float(), pout, k_off)[0], ref, ab, P_k, "fp32")


def test_row_batchnorm_wrappers_equal_torch_batchnorm1d():
    g = torch.Generator().manual_seed(3)
    n, C = 301, 6
    x = (torch.randn((n, C), generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    dy = torch.randn((n, C), generator=g, dtype=torch.float64)
    bn = torch.nn.BatchNorm1d(C).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g))
        bn.bias.copy_(torch.randn(C, generator=g))
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    w, b = bn.weight.detach(), bn.bias.detach()
    y_t = torch.relu(bn(x))
    y_t.backward(dy)
    y, rm, rv, saved = R.bn_rows_train_fwd64(x.detach(), w, b, rm0, rv0, 0.1, bn.eps, True)
    torch.testing.assert_close(y, y_t.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(rm, bn.running_mean, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(rv, bn.running_var, rtol=1e-12, atol=1e-12)
    dx, dw, db = R.bn_rows_bwd64(dy, x.detach(), y, w, saved, True, True)
    torch.testing.assert_close(dx, x.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(dw, bn.weight.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(db, bn.bias.grad, rtol=1e-10, atol=1e-12)
    # the sums, the statistics derived from them and the backward sums
    s1, s2, cnt, s1_abs = R.bn_sums64(x.detach())
    mean, var, invstd, *_ = R.stats_bounds(s1, s2, s1_abs, cnt, bn.eps)
    torch.testing.assert_close(mean, saved[0], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(invstd, saved[1], rtol=1e-10, atol=0)
    xhat = (x.detach() - mean) * invstd
    gs, gxs, _, _ = R.bn_bwd_sums64(dy, xhat, y > 0)
    torch.testing.assert_close(gs, db, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(gxs, dw, rtol=1e-12, atol=1e-12)
    rm2, rv2 = R.running64(rm0, rv0, mean, var, cnt, 0.1)
    torch.testing.assert_close(rm2, rm, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(rv2, rv, rtol=1e-12, atol=1e-12)


def test_sums_bar_rejects_a_lost_row_and_accepts_fp64_order_changes():
    g = torch.Generator().manual_seed(5)
    n, C = 40000, 8
    x = torch.randn((n, C), generator=g).double() * 2 + 0.5
    s1, s2, cnt, s1_abs = R.bn_sums64(x)
    # another double summation order (blocked), as the kernels use
    blocked1 = x.view(400, 100, C).sum(1).sum(0)
    blocked2 = (x * x).view(400, 100, C).sum(1).sum(0)
    assert R.assert_sums(blocked1, s1, s1_abs, cnt, "blocked sum x") <= 1
    assert R.assert_sums(blocked2, s2, s2, cnt, "blocked sum x^2") <= 1
    lost1, lost2 = x[1:].sum(0), (x[1:] * x[1:]).sum(0)
    with pytest.raises(AssertionError):
        R.assert_sums(lost1, s1, s1_abs, cnt, "sum x, one row lost")
    with pytest.raises(AssertionError):
        R.assert_sums(lost2, s2, s2, cnt, "sum x^2, one row lost")
