"""The float64 yardstick of the sparse convolution (tests/sconv_ref.py) against dense float64 F.conv3d /
F.conv_transpose3d and their autograd on every scene and map kind; the CPU oracle (oracle.me_cpu, exact mode) -- maps and
numbers -- against the yardstick; and wrong variants of the conventions, each of which must leave the derived bound.
No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sconv_ref as R

SCENE_NAMES = list(R.SCENES)
KIND_NAMES = list(R.KINDS)


def _operands(n_in, n_out, K, Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_in, Cin, generator=g)
    W = torch.randn(K, Cin, Cout, generator=g) * 0.3
    b = torch.randn(Cout, generator=g)
    gy = torch.randn(n_out, Cout, generator=g)
    ad = torch.randn(n_in, Cin, generator=g)
    return x, W, b, gy, ad


# ------------------------------------------------------------------ 1. the yardstick against dense convolution
def _shift(fine):
    """per-scan translation by an even amount onto a grid that starts at 0 (range_ends would not fit one otherwise);
    returns (batch index 0.., per-row shift [n, 3]) as functions of the batch column"""
    fine = np.asarray(fine, dtype=np.int64)
    batches = np.unique(fine[:, 0])
    lo = {int(b): np.floor_divide(fine[fine[:, 0] == b][:, 1:].min(axis=0), 2) * 2 for b in batches}
    index = {int(b): i for i, b in enumerate(batches)}

    def place(c):
        c = np.asarray(c, dtype=np.int64)
        bi = np.array([index[int(b)] for b in c[:, 0]], dtype=np.int64)
        return bi, c[:, 1:] - np.stack([lo[int(b)] for b in c[:, 0]])
    return place, len(batches)


def _dense_weight(W, ks, transposed):
    K, Cin, Cout = W.shape
    w = W.double().view(ks, ks, ks, Cin, Cout)             # [iz, iy, ix, ci, co]
    w = w.permute(3, 4, 2, 1, 0) if transposed else w.permute(4, 3, 2, 1, 0)
    return w.contiguous()                                  # [.., .., ix, iy, iz]


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_yardstick_equals_dense_float64_convolution(name, kind):
    ks, stride, dil, transposed = R.KINDS[kind]
    cin, cout, nbr = R.scene_map(name, kind)
    Cin, Cout = 3, 2
    x, W, b, gy, ad = _operands(cin.shape[0], cout.shape[0], ks ** 3, Cin, Cout, 17)
    place, B = _shift(R.scene(name))
    bi, pi = place(cin)
    bo, po = place(cout)
    s_in, s_out = (stride, 1) if transposed else (1, stride)
    assert (pi % s_in == 0).all() and (po % s_out == 0).all()
    qi, qo = pi // s_in, po // s_out
    dims = (np.maximum(pi.max(axis=0), po.max(axis=0)) // s_in + 2) // 2 * 2     # even: a k2 s2 window never hangs over
    xd = torch.zeros((B, Cin, *dims.tolist()), dtype=torch.float64)
    xd[bi, :, qi[:, 0], qi[:, 1], qi[:, 2]] = x.double()
    xd.requires_grad_(True)
    w = _dense_weight(W, ks, transposed)
    if transposed:
        yd = F.conv_transpose3d(xd, w, b.double(), stride=stride)
        y = R.tconv64(x, W, b, R.scene_map(name, "k2s2")[2], cout.shape[0])
    else:
        yd = F.conv3d(xd, w, b.double(), stride=stride, padding=dil * (ks // 2) if ks % 2 else 0, dilation=dil)
        y = R.conv64(x, W, b, nbr)
    got = yd[bo, :, qo[:, 0], qo[:, 1], qo[:, 2]]
    mag = R.abs_terms(x, W, b, nbr)
    assert ((got.detach() - y).abs() <= 1e-12 * mag).all(), f"{name} {kind}: forward"
    got.backward(gy.double())
    gd = xd.grad[bi, :, qi[:, 0], qi[:, 1], qi[:, 2]]
    gx = R.dgrad64(gy, W, nbr, ad)
    gmag = R.abs_terms(gy, W.transpose(1, 2), None, R.transpose_map(nbr, cin.shape[0]), ad)
    assert ((gd + ad.double() - gx).abs() <= 1e-12 * gmag).all(), f"{name} {kind}: data gradient"


def test_scenes_are_what_they_claim():
    """the structure the GPU tests rely on: pair counts at the tile edge, empty offsets, full and centre-only rows"""
    def counts(name, kind):
        return (R.scene_map(name, kind)[2] >= 0).sum(axis=1)
    for name in R.SCENES:
        c = R.scene(name)
        assert c.dtype == np.int32 and c.shape[1] == 4 and c.shape[0] <= 4200, name
        assert np.unique(c, axis=0).shape[0] == c.shape[0], name
    per_row = (R.scene_map("dense_cube", "k3s1")[2] >= 0).sum(axis=0)
    assert per_row[0] == 27 and per_row.max() == 27 and counts("dense_cube", "k3s1").sum() == 2 * 28 ** 3
    assert (R.scene_map("dense_cube", "k5s1")[2] >= 0).sum(axis=0).max() == 125
    kids = (R.scene_map("dense_cube_odd", "k2s2")[2] >= 0).sum(axis=0)
    assert set(kids.tolist()) == {1, 2, 4, 8}
    assert R.scene("isolated").shape[0] == 385
    assert counts("isolated", "k3s1").tolist() == [0] * 13 + [385] + [0] * 13
    assert counts("isolated", "k2s2").tolist() == [385] + [0] * 7
    for L in (128, 129, 130):
        c = counts(f"line_x{L}", "k3s1")
        assert (c[12], c[13], c[14]) == (L - 1, L, L - 1) and c.sum() == 3 * L - 2
    c = counts("line_z129", "k3s1")
    assert (c[4], c[13], c[22]) == (128, 129, 128) and c.sum() == 3 * 129 - 2
    c = counts("checkerboard", "k3s1")
    assert all(c[k] == 0 for k in (4, 10, 12, 14, 16, 22)) and c[13] == 864
    t = R.scene("twin_scans")
    assert np.array_equal(np.unique(t[t[:, 0] == 0][:, 1:], axis=0), np.unique(t[t[:, 0] == 1][:, 1:], axis=0))
    assert (R.scene("one_and_many")[:, 0] == 0).sum() == 1
    r = R.scene("range_ends")
    assert r[:, 1:].max() == 65535 and r[:, 1:].min() == -65536 and set(r[:, 0].tolist()) == {0, 4095}
    assert [R.scene(f"tiny_{n}").shape[0] for n in (1, 2, 127, 128, 129)] == [1, 2, 127, 128, 129]


def test_scans_of_any_two_batch_indices_stay_apart():
    """the same block under batch indices of equal parity and at both ends of the range: no neighbour and no strided
    parent is shared"""
    block = R.scene("dense_cube")
    block = block[block[:, 0] == 0]
    for b in (2, 4094, 4095):
        other = block.copy()
        other[:, 0] = b
        c = np.concatenate([block, other])
        n = block.shape[0]
        nbr = R.neighbours(c, c, 3, 1, 1)
        assert (nbr[:, :n] < n).all() and ((nbr[:, n:] >= n) | (nbr[:, n:] < 0)).all()
        assert np.array_equal(nbr[:, n:], np.where(nbr[:, :n] >= 0, nbr[:, :n] + n, -1))
        assert R.strided(c, 2).shape[0] == 2 * R.strided(block, 2).shape[0]


# ------------------------------------------------------------------ 2. the CPU oracle against the yardstick
def _oracle_conv(OME, coords, kind, x, W, b, gy):
    """(output, input gradient, nbr [K, n_out], k_off) of the oracle's exact mode for one map kind"""
    ks, stride, dil, transposed = R.KINDS[kind]
    K, Cin, Cout = W.shape
    st = OME.SparseTensor(coordinates=torch.from_numpy(coords), features=torch.zeros(coords.shape[0], 1))
    cm = st.coordinate_manager
    if transposed:
        cm.stride(1, stride)
        conv = OME.MinkowskiConvolutionTranspose(Cin, Cout, kernel_size=ks, stride=stride, bias=True, dimension=3)
        key = stride
    else:
        conv = OME.MinkowskiConvolution(Cin, Cout, kernel_size=ks, stride=stride, dilation=dil, bias=True, dimension=3)
        key = 1
    with torch.no_grad():
        conv.kernel.copy_(W)
        conv.bias.copy_(b.view(1, -1))
    xin = x.clone().requires_grad_(True)
    out = conv(OME.SparseTensor(features=xin, coordinate_manager=cm, coordinate_map_key=key))
    out.F.backward(gy)
    k_off, _, _, nbr = cm.kernel_map(1, stride, ks, dil)
    return out.F.detach(), xin.grad, nbr.numpy().T, k_off.numpy(), cm


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_oracle_maps_and_numbers_stay_inside_the_yardsticks_bound(name, record_property):
    import oracle.me_cpu as OME
    OME.set_mode("exact")
    coords = R.scene(name)
    worst = 0.0
    for kind in KIND_NAMES:
        ks, stride, dil, transposed = R.KINDS[kind]
        cin, cout, nbr = R.scene_map(name, kind)
        for Cin, Cout in ((5, 7), (32, 32)) if kind == "k3s1" else ((5, 7),):
            x, W, b, gy, ad = _operands(cin.shape[0], cout.shape[0], ks ** 3, Cin, Cout, Cin + len(kind))
            y, gx, o_nbr, o_koff, cm = _oracle_conv(OME, coords, kind, x, W, b, gy)
            fwd = R.scene_map(name, "k2s2" if transposed else kind)[2]       # the table as built: fine -> coarse
            assert np.array_equal(o_nbr, fwd), f"{name} {kind}: neighbour table"
            assert np.array_equal(o_koff, R.pairs(fwd)[0]), f"{name} {kind}: k_off"
            if stride > 1:
                assert np.array_equal(cm.maps[stride].numpy(), R.strided(coords, stride)), f"{name} {kind}: strided"
            r1 = R.worst_ratio(y, R.conv64(x, W, b, nbr), R.bound(x, W, b, nbr))
            nbr_t = R.transpose_map(nbr, cin.shape[0])
            Wt = W.transpose(1, 2)
            r2 = R.worst_ratio(gx, R.dgrad64(gy, W, nbr, n_in=cin.shape[0]), R.bound(gy, Wt, None, nbr_t))
            assert r1 <= 1.0 and r2 <= 1.0, f"{name} {kind} {Cin}->{Cout}: error / bound {r1:.3g} (forward) {r2:.3g} (dgrad)"
            worst = max(worst, r1, r2)
    print(f"oracle worst error / bound on {name}: {worst:.4f}")
    record_property("worst_error_over_bound", worst)


# ------------------------------------------------------------------ 3. wrong variants must leave the bound
def _ref(name, kind, C=4, seed=3):
    cin, cout, nbr = R.scene_map(name, kind)
    ks = R.KINDS[kind][0]
    x, W, b, _, _ = _operands(cin.shape[0], cout.shape[0], ks ** 3, C, C, seed)
    return cin, cout, nbr, x, W, b, R.conv64(x, W, b, nbr), R.bound(x, W, b, nbr)


def _failing(y_wrong, y, bnd):
    """fraction of the reference's elements the wrong result misses, compared row by row as a kernel's output would be
    (rows the wrong result does not have count as missed)"""
    n = min(y.shape[0], y_wrong.shape[0])
    bad = ((y_wrong[:n] - y[:n]).abs() > bnd[:n]).sum().item() + (y.shape[0] - n) * y.shape[1]
    return bad / max(y.numel(), 1)


def _mirrored(name, kind):
    cin, cout, nbr, x, W, b, y, bnd = _ref(name, kind)
    return _failing(R.conv64(x, W.flip(0), b, nbr), y, bnd)


def _y_fastest(name, kind):
    cin, cout, nbr, x, W, b, y, bnd = _ref(name, kind)
    ks, stride, dil, _ = R.KINDS[kind]
    o = R.offsets(ks, 1, dil).reshape(ks, ks, ks, 3)                  # [iz, iy, ix]
    wrong = R.neighbours(cin, cout, ks, 1, stride, dil, offs=o.transpose(0, 2, 1, 3).reshape(-1, 3))
    return _failing(R.conv64(x, W, b, wrong), y, bnd)


def _w_transposed(name, kind):
    cin, cout, nbr, x, W, b, y, bnd = _ref(name, kind)
    return _failing(R.conv64(x, W.transpose(1, 2), b, nbr), y, bnd)


def _last_offset_dropped(name, kind):
    cin, cout, nbr, x, W, b, y, bnd = _ref(name, kind)
    return _failing(R.conv64(x, W[:-1], b, nbr[:-1]), y, bnd)


def _bias_dropped(name, kind):
    cin, cout, nbr, x, W, b, y, bnd = _ref(name, kind)
    return _failing(R.conv64(x, W, None, nbr), y, bnd)


def _truncating_stride(name, kind):
    cin, cout, nbr, x, W, b, y, bnd = _ref(name, kind)
    ks, stride, dil, _ = R.KINDS[kind]
    c = cin.astype(np.int64).copy()
    c[:, 1:] = np.trunc(c[:, 1:] / stride).astype(np.int64) * stride
    _, first = np.unique(c, axis=0, return_index=True)
    wrong_out = c[np.sort(first)]
    return _failing(R.conv64(x, W, b, R.neighbours(cin, wrong_out, ks, 1, stride, dil)), y, bnd)


def _across_batches(name, kind):
    cin, cout, nbr, x, W, b, y, bnd = _ref(name, kind)
    ks, stride, dil, _ = R.KINDS[kind]
    flat_in, flat_out = cin.copy(), cout.copy()
    flat_in[:, 0] = 0
    flat_out[:, 0] = 0
    _, first = np.unique(flat_in, axis=0, return_index=True)
    first = np.sort(first)                                            # a table without the batch keeps the first row
    wrong = R.neighbours(flat_in[first], flat_out, ks, 1, stride, dil)
    wrong = np.where(wrong >= 0, first[np.clip(wrong, 0, None)], -1)
    return _failing(R.conv64(x, W, b, wrong), y, bnd)


def _even_kernel_centred(name, kind):
    cin, cout, nbr, x, W, b, y, bnd = _ref(name, kind)
    ks, stride, dil, _ = R.KINDS[kind]
    wrong = R.neighbours(cin, cout, ks, 1, stride, dil, offs=R.offsets(ks, 1, dil) - (ks // 2))
    return _failing(R.conv64(x, W, b, wrong), y, bnd)


# variant -> (function, the scenes and map kinds where it can differ)
VARIANTS = {
    "mirrored offset order": (_mirrored, [("dense_cube", "k3s1"), ("line_x129", "k3s1"), ("dense_cube", "k2s2")]),
    "y-fastest offsets": (_y_fastest, [("dense_cube", "k3s1"), ("line_x129", "k3s1"), ("checkerboard", "k5s1")]),
    "W[k] transposed": (_w_transposed, [("dense_cube", "k3s1"), ("isolated", "k3s1"), ("tiny_1", "k3s1")]),
    "last offset dropped": (_last_offset_dropped, [("dense_cube", "k3s1"), ("dense_cube", "k2s2"), ("twin_scans", "k3s1")]),
    "bias dropped": (_bias_dropped, [("isolated", "k3s1"), ("dense_cube", "k5s1"), ("range_ends", "k3s1")]),
    "truncating stride": (_truncating_stride, [("dense_cube_odd", "k2s2"), ("dense_cube_odd", "k3s2"),
                                               ("range_ends", "k2s2"), ("dense_cube", "k2s2")]),
    "neighbours across batches": (_across_batches, [("twin_scans", "k3s1"), ("twin_scans", "k5s1"),
                                                    ("dense_cube", "k3s1")]),
    "even-kernel offsets centred": (_even_kernel_centred, [("dense_cube", "k2s2"), ("dense_cube_odd", "k2s2"),
                                                           ("isolated", "k2s2")]),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_wrong_variants_leave_the_bound(variant, record_property):
    fn, where = VARIANTS[variant]
    got = {f"{name} {kind}": fn(name, kind) for name, kind in where}
    caught = [w for w, f in got.items() if f >= 0.5]
    print(f"{variant}: fraction of elements outside the bound {got}; caught on {caught}")
    record_property("caught_on", ", ".join(caught))
    assert caught, f"{variant} stays inside the bound on more than half of the elements everywhere: {got}"
