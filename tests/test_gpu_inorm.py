"""MinkowskiInstanceNorm on the device (csrc/inorm.hip) against a float64 torch restatement of the per-(scan, channel)
formulas (tests/ibn_ref.instance_norm64, run on the device): forward, dx, dweight, dbias over the maps of small_batch at
tensor strides 1 / 2 / 4 / 8, for collated rows, rows shuffled across scans, batch ids {0, 2} only (an empty scan in
between) and a scan of one voxel (variance 0: y = bias); run-to-run bit reproducibility; eval = train; every lidog_in_*
entry of the C ABI called once directly."""
import numpy as np
import pytest
import torch

from helpers import small_batch
from ibn_ref import instance_norm64

pytestmark = pytest.mark.gpu
CHANNELS = (32, 64, 96, 128, 7)
STRIDES = (1, 2, 4, 8)


def _inputs(kind):
    c = small_batch((0, 1), n_points=1500)
    if kind == "shuffled":
        c = c[torch.randperm(c.shape[0], generator=torch.Generator().manual_seed(3))]
    elif kind == "ids02":
        c = c.clone()
        c[c[:, 0] == 1, 0] = 2
    elif kind == "single":
        one = torch.tensor([[2, 7, 7, 7]], dtype=torch.int32)
        c = torch.cat([c, one])
    return c.contiguous()


def _check_one(ME, x_st, C, seed):
    """forward + backward of the module on x_st's map with C channels against the float64 restatement"""
    dev = "cuda"
    n = x_st.C.shape[0]
    g = torch.Generator(device="cpu").manual_seed(seed)
    feats = (torch.randn((n, C), generator=g) * 2 + 0.5).to(dev).requires_grad_(True)
    dy = torch.randn((n, C), generator=g).to(dev)
    m = ME.MinkowskiInstanceNorm(C).to(dev)
    with torch.no_grad():
        m.weight.copy_(torch.randn((1, C), generator=g))
        m.bias.copy_(torch.randn((1, C), generator=g))
    st = ME.SparseTensor(feats, coordinate_manager=x_st.coordinate_manager, coordinate_map_key=x_st.coordinate_map_key)
    outs = []
    for _ in range(3):
        feats.grad = None
        m.weight.grad = m.bias.grad = None
        y = m(st).F
        y.backward(dy)
        outs.append((y.detach().clone(), feats.grad.clone(), m.weight.grad.clone(), m.bias.grad.clone()))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0])), "instance norm is not run-to-run reproducible"
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(st).F, outs[0][0]), "eval-mode output differs from train-mode output"
    m.train()
    batch = st.C[:, 0]
    x64 = feats.detach().double().requires_grad_(True)
    w64 = m.weight.detach().double().requires_grad_(True)
    b64 = m.bias.detach().double().requires_grad_(True)
    ref = instance_norm64(x64, batch, w64, b64)
    ref.backward(dy.double())
    for got, want, what in zip(outs[0], (ref, x64.grad, w64.grad, b64.grad), ("y", "dx", "dweight", "dbias")):
        want = want.detach()
        assert got.shape == want.shape, what
        assert torch.isfinite(got).all(), f"{what}: non-finite values"
        err = (got.double() - want).abs().max().item()
        scale = want.abs().max().item()
        assert err <= 1e-5 * max(scale, 1e-30), f"{what} C={C}: max error {err:.3e} vs max |ref| {scale:.3e}"
    return outs[0][0]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", ["collated", "shuffled", "ids02", "single"])
def test_instance_norm_matches_float64_restatement(kind):
    import lidog_amd.me as ME
    coords = _inputs(kind).cuda()
    x = ME.SparseTensor(torch.ones((coords.shape[0], 1), device="cuda"), coordinates=coords)
    cm = x.coordinate_manager
    for s in STRIDES:
        if s > 1:
            cm.stride(1, s)
        xs = ME.SparseTensor(None, coordinate_manager=cm, coordinate_map_key=s)
        for i, C in enumerate(CHANNELS):
            _check_one(ME, xs, C, seed=100 * s + i)
    if kind == "single":   # the one-voxel scan (batch id 2): variance 0, y = bias
        xs = ME.SparseTensor(None, coordinate_manager=cm, coordinate_map_key=1)
        m = ME.MinkowskiInstanceNorm(32).cuda()
        with torch.no_grad():
            m.bias.copy_(torch.arange(32, dtype=torch.float32)[None] * 0.25)
        f = torch.randn((xs.C.shape[0], 32), device="cuda")
        y = m(ME.SparseTensor(f, coordinate_manager=cm, coordinate_map_key=1)).F
        one = (xs.C[:, 0] == 2).nonzero().flatten()
        assert one.numel() == 1
        assert torch.equal(y[one[0]], m.bias.detach()[0]), "a one-voxel scan must give y = bias"


@pytest.mark.timeout(60)
def test_segments_of_a_shuffled_map():
    """perm is a stable batch order of the map's rows, seg_off the scan boundaries (empty scan 1 included)"""
    import lidog_amd.me as ME
    coords = _inputs("shuffled")
    coords[coords[:, 0] == 1, 0] = 2
    x = ME.SparseTensor(torch.ones((coords.shape[0], 1), device="cuda"), coordinates=coords.cuda())
    perm, seg_off, bid, B = x.coordinate_manager.segments(1)
    c = x.C[:, 0].cpu().numpy()
    assert B == 3
    want = np.argsort(c, kind="stable")
    assert np.array_equal(perm.cpu().numpy(), want)
    assert seg_off.cpu().tolist() == [0, int((c == 0).sum()), int((c == 0).sum()), c.shape[0]]
    assert np.array_equal(bid.cpu().numpy(), c)


@pytest.mark.timeout(60)
def test_every_in_entry_point_called_directly():
    """the C ABI on its own: segments, statistics, apply, backward reduce / apply, the three IBN entries"""
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    L = _lib.load()
    dev = "cuda"
    coords = _inputs("shuffled").to(dev)
    n, C, B = coords.shape[0], 32, 2
    g = torch.Generator().manual_seed(5)
    x = torch.randn((n, C), generator=g).to(dev)
    dy2 = torch.randn((n, 2 * C), generator=g).to(dev)
    w, b = torch.rand(C, generator=g).to(dev) + 0.5, torch.randn(C, generator=g).to(dev)
    perm, bid = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    seg_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    nbytes = L.lidog_in_segments_ws(n)
    ws8 = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call("lidog_in_segments", ptr(coords), n, B, ptr(perm), ptr(seg_off), ptr(bid), ptr(ws8), nbytes)
    ws = torch.empty(L.lidog_in_reduce_ws(B, C), dtype=torch.float64, device=dev)
    mean, invstd = torch.empty(B * C, device=dev), torch.empty(B * C, device=dev)
    call("lidog_in_stats", ptr(x), n, C, B, ptr(perm), ptr(seg_off), 1e-8, ptr(mean), ptr(invstd), ptr(ws))
    y = torch.empty_like(x)
    call("lidog_in_apply", ptr(x), n, C, B, ptr(bid), ptr(mean), ptr(invstd), ptr(w), ptr(b), ptr(y))
    ref = instance_norm64(x.double(), coords[:, 0], w.double(), b.double())
    assert (y.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    dy = dy2[:, C:].contiguous()
    coef = torch.empty(2 * B * C, device=dev)
    dw, db, dx = torch.empty(C, device=dev), torch.empty(C, device=dev), torch.empty_like(x)
    call("lidog_in_bwd_reduce", ptr(dy), ptr(x), n, C, B, ptr(perm), ptr(seg_off), ptr(mean), ptr(invstd), ptr(ws),
         ptr(coef), ptr(dw), ptr(db))
    call("lidog_in_bwd_apply", ptr(dy), ptr(x), n, C, B, ptr(bid), ptr(mean), ptr(invstd), ptr(w), ptr(coef), ptr(dx))
    x64 = x.double().requires_grad_(True)
    instance_norm64(x64, coords[:, 0], w.double(), b.double()).backward(dy.double())
    assert (dx.double() - x64.grad).abs().max().item() <= 1e-5 * x64.grad.abs().max().item()
    assert torch.allclose(db.double(), dy.double().sum(0), rtol=1e-5, atol=1e-4)
    # IBN entries: forward, the two reductions, the fused data gradient
    sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
    bn_mean, bn_invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    bn_ws = torch.empty(L.lidog_bn_reduce_ws(C, 1), dtype=torch.float64, device=dev)
    call("lidog_bn_stats", ptr(x), n, C, 1, ptr(sums), ptr(bn_ws), float(n), 1e-5, 0.0, ptr(bn_mean), ptr(bn_invstd),
         None, None)
    out = torch.empty((n, 2 * C), device=dev)
    bits = torch.empty(L.lidog_relu_bits_words(n, 2 * C), dtype=torch.int32, device=dev)
    call("lidog_ibn_apply", ptr(x), n, C, B, ptr(bn_mean), ptr(bn_invstd), ptr(w), ptr(b), ptr(bid), ptr(mean),
         ptr(invstd), ptr(w), ptr(b), ptr(out), ptr(bits))
    assert torch.equal(out[:, C:], torch.relu(y))
    bn_dw, bn_db, in_dw, in_db = (torch.empty(C, device=dev) for _ in range(4))
    call("lidog_ibn_bwd_reduce", ptr(dy2), ptr(bits), ptr(x), n, C, B, ptr(bn_mean), ptr(bn_invstd), ptr(sums),
         ptr(bn_ws), ptr(bn_dw), ptr(bn_db), ptr(perm), ptr(seg_off), ptr(mean), ptr(invstd), ptr(ws), ptr(coef),
         ptr(in_dw), ptr(in_db))
    call("lidog_ibn_bwd_apply", ptr(dy2), ptr(bits), ptr(x), n, C, B, ptr(bn_mean), ptr(bn_invstd), ptr(w), ptr(sums),
         float(n), ptr(bid), ptr(mean), ptr(invstd), ptr(w), ptr(coef), ptr(dx))
    mask = (out > 0).float()
    assert torch.allclose(in_db.double(), (dy2[:, C:] * mask[:, C:]).double().sum(0), rtol=1e-5, atol=1e-4)
    assert torch.allclose(bn_db.double(), (dy2[:, :C] * mask[:, :C]).double().sum(0), rtol=1e-5, atol=1e-4)
    assert torch.isfinite(dx).all()
