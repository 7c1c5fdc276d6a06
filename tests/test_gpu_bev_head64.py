"""The full-size BEV head against float64: Encoder2D in training mode on sparse2super images of synthetic 120 k-point
scans (tests/bev_ref.encoder2d64 on the same weights): logits, the feature gradient through sparse2super's backward,
every parameter gradient and the running statistics; the routing of the first convolution (support-restricted for
Cin <= 128, dense for the 256-channel bottle level).  Also: the channel lists built from a support map equal the ones
built from the row bitmasks the pooling kernel writes, on a real sparse2super image."""
import functools

import pytest
import torch

import bev_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _scans(seeds):
    from lidog_amd import synth
    return synth.make_batch(list(seeds), "kitti120k", "cuda")["coords_int"]


def _tensor(seeds, feats):
    import lidog_amd.me as ME
    st = ME.SparseTensor(coordinates=_scans(seeds), features=torch.ones((_scans(seeds).shape[0], 1), device="cuda"))
    return ME.SparseTensor(feats, coordinate_manager=st.coordinate_manager, coordinate_map_key=1)


def _features(n, C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    f = torch.rand(n, C, device="cuda", generator=g)
    return torch.where(torch.rand(n, C, device="cuda", generator=g) < 0.3, torch.zeros_like(f), f)


def _pool(coords, feats, bound, rowbits):
    """sparse2super's forward calls: (image, source map, act buffer or None); the act buffer zero-filled beforehand so
    that two of them compare equal in the slots no kernel writes (alignment padding, list entries past the counts)"""
    from lidog_amd import bev
    from lidog_amd._lib import call, load, ptr
    n, C = feats.shape
    lx, ly, lo, H = bev._device_luts(bound, 0.05, "cuda")
    W, B, (pk, ps, pp) = H, 2, (5, 3, 1)
    Ho, Wo = (H + 2 * pp - pk) // ps + 1, (W + 2 * pp - pk) // ps + 1
    winner = torch.full((B, H, W), -1, dtype=torch.int32, device="cuda")
    pixel = torch.empty(n, dtype=torch.int32, device="cuda")
    call("lidog_bev_winner", ptr(coords), n, ptr(lx), ptr(ly), lo, lx.shape[0], H, W, ptr(winner), ptr(pixel))
    act = torch.zeros(load().lidog_conv2d_support_ws(B, C, Ho, Wo), dtype=torch.int32, device="cuda") if rowbits else None
    out = torch.empty((B, C, Ho, Wo), device="cuda")
    arg = torch.empty((B, C, Ho, Wo), dtype=torch.int32, device="cuda")
    call("lidog_bev_pool_fwd", ptr(feats), C, ptr(winner), ptr(pixel), n, B, H, W, pk, ps, pp, Ho, Wo, ptr(out),
         ptr(arg), ptr(act))
    return out, arg, act


def _bits(act, B, C, H, W):
    words = (W + 63) // 64
    b = act[:2 * B * C * H * words].view(torch.int64).view(B, C, H, words)
    cols = torch.arange(W, device=act.device)
    return ((b[..., cols // 64] >> (cols % 64)) & 1).bool()


@pytest.mark.parametrize("zeros", [False, True])
def test_support_lists_from_map_equal_lists_from_pooling_bitmasks(zeros):
    """positive features: every window the pooling kernel computes has a source cell, and the act buffer built from the
    source map (lidog_conv2d_support with a pointer) equals the one built from the pooling kernel's row bitmasks, word
    for word.  Zero-heavy features: a window whose maximum is an empty cell's 0 has no source; the bitmasks are then a
    superset of the source map, and the image is zero outside them."""
    from lidog_amd._lib import call, ptr
    coords = _scans((5, 6))
    n, C, bound = coords.shape[0], 96, 50.0
    feats = _features(n, C, 11) if zeros else torch.rand(n, C, device="cuda",
                                                         generator=torch.Generator(device="cuda").manual_seed(11)) + 0.5
    out_a, _, act_pool = _pool(coords, feats, bound, True)
    out_b, arg_b, _ = _pool(coords, feats, bound, False)     # without bitmasks the source map is -1 on empty windows
    B, _, Ho, Wo = out_a.shape
    assert torch.equal(out_a, out_b)
    sup = arg_b >= 0
    assert 0.02 < float(sup.float().mean()) < 0.10 and bool(sup[1].any())
    call("lidog_conv2d_support", None, B, C, Ho, Wo, ptr(act_pool))
    bits = _bits(act_pool, B, C, Ho, Wo)
    if zeros:
        assert torch.equal(sup & bits, sup) and not torch.equal(sup, bits)
        assert torch.equal(out_a != 0, (out_a != 0) & bits)
        return
    act_map = torch.zeros_like(act_pool)
    call("lidog_conv2d_support", ptr(arg_b), B, C, Ho, Wo, ptr(act_map))
    assert torch.equal(bits, sup), f"{int((bits != sup).sum())} cells differ"
    diff = (act_pool != act_map).nonzero().flatten()
    assert diff.numel() == 0, f"{diff.numel()} of {act_pool.numel()} words differ, first at {diff[:8].tolist()}"


# (bound, Cin, sparse first convolution); B = 2 scans
HEAD_CASES = [(50.0, 96, True), (30.0, 128, True), (50.0, 256, False)]
# bars relative to max |ref| of each tensor; worst measured on the MI355X: logits 1.2e-6, gradients 2.2e-6 (a
# BatchNorm bias), running statistics 1.0e-7
TOL_LOGITS, TOL_GRAD, TOL_STATS = 1e-5, 2e-5, 1e-6
# 3x3 weight gradients relative to max sum |terms| instead (the BatchNorm backward removes the channel mean of the
# gradient, and the input is non-negative: sum x gy cancels far below its terms); worst measured 3.6e-8
TOL_WTERMS = 1e-6


def _rel(got, ref):
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


@pytest.mark.parametrize("bound,Cin,sparse", HEAD_CASES)
def test_full_size_head_vs_float64(bound, Cin, sparse, record_property, monkeypatch):
    """the ReLU decisions of the reference are the kernels' own (the BatchNorm outputs > 0): an output within rounding
    of 0 may fall on either side, and one such flip moves a BatchNorm bias gradient by a whole gradient element"""
    import lidog_amd.me as ME
    from lidog_amd import bev
    from lidog_amd._lib import call, ptr
    seeds = (7, 8)
    n = _scans(seeds).shape[0]
    torch.manual_seed(int(bound) + Cin)
    enc = bev.Encoder2D(Cin, 7).cuda().train()
    with torch.no_grad():                                   # BatchNorm parameters away from (1, 0)
        for i in (1, 4):
            bnm = enc.down1.maxpool_conv[0].double_conv[i]
            bnm.weight.uniform_(0.5, 1.5)
            bnm.bias.uniform_(-0.2, 0.2)
    sd0 = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    feats = _features(n, Cin, Cin).requires_grad_(True)
    bn_out = []
    batch_norm = ME.batch_norm

    def spy(*a, **k):
        y = batch_norm(*a, **k)
        bn_out.append(y.detach() > 0)
        return y

    monkeypatch.setattr(ME, "batch_norm", spy)
    timer = bev.HeadTimer()
    timer.enabled = True
    bev.HEAD_TIMER = timer
    try:
        img = bev.sparse2super(_tensor(seeds, feats), bound=bound)
        assert (bev.structural_support(img) is not None) == sparse
        logits = enc(img)
        # routing of the first convolution's forward: the support path records its work as (act, dims, which)
        assert isinstance(timer.records[0][2], tuple) == sparse
        assert not isinstance(timer.records[1][2], tuple)
        winner, pixel, argsrc, _ = img.grad_fn.saved_tensors
        gl = torch.randn(logits.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        logits.backward(gl)
        torch.cuda.synchronize()
    finally:
        bev.HEAD_TIMER = None

    p64 = {k: (v.double().requires_grad_(True) if "running" not in k and "num_batches" not in k else v.double())
           for k, v in sd0.items()}
    img64 = img.detach().double().requires_grad_(True)
    bn0 = enc.down1.maxpool_conv[0].double_conv[1]
    keep = {}
    assert len(bn_out) == 2
    ref, stats = R.encoder2d64(img64, p64, momentum=bn0.momentum, eps=bn0.eps, keep=keep, relu_masks=bn_out)
    ref.backward(gl.double())

    r, bar = {"logits": _rel(logits.detach(), ref.detach())}, {"logits": TOL_LOGITS}
    sd = enc.state_dict()
    for k, v in stats.items():
        r[k], bar[k] = _rel(sd[k], v), TOL_STATS
    for k, prm in enc.named_parameters():
        if k in keep:                                       # 3x3 weights: (conv input, conv output) of the reference
            xin, yout = keep[k]
            scale = float(R.conv3s2_wgrad64(xin.detach().abs(), yout.grad.abs()).max())
            r[k], bar[k] = float((prm.grad.double() - p64[k].grad).abs().max()) / scale, TOL_WTERMS
        else:
            r[k], bar[k] = _rel(prm.grad, p64[k].grad), TOL_GRAD
    # the feature gradient: sparse2super's backward (pinned elsewhere) applied to the float64 image gradient
    B, C, Ho, Wo = img.shape
    H, W = winner.shape[-2:]
    gref = torch.empty_like(feats)
    call("lidog_bev_pool_bwd", ptr(img64.grad.float().contiguous()), ptr(argsrc), ptr(winner), ptr(pixel), n, C, B, H, W,
         5, 3, 1, Ho, Wo, ptr(gref))
    r["feats"], bar["feats"] = _rel(feats.grad, gref.double()), TOL_GRAD
    for k, v in r.items():
        record_property(k, v)
    assert all(r[k] <= bar[k] for k in r), {k: (f"{r[k]:.3g}", bar[k]) for k in r}
