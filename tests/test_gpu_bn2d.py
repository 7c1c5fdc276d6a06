"""BatchNorm2d on NCHW images (the hw > 1 branch of csrc/bn.hip: k_colreduce_plane, k_bn_apply_plane / k_bn_apply,
k_bn_bwd_apply_plane / k_bn_bwd_apply) through lidog_amd.me.batch_norm(..., hw=H*W) against the float64 yardstick
(tests/bev_ref.py), in training mode (y, running mean / variance, dx, dweight, dbias, with and without the fused ReLU)
and in evaluation mode.  The image sizes reach one and several reduction chunks (16 384 elements, at most 64 of them),
one and several apply chunks (8 192, at most 64; the plane kernels from hw = 1 024) and both caps."""
import pytest
import torch

import bev_ref as R

pytestmark = pytest.mark.gpu

# (B, C, H, W): every hw once; the large ones with a small C
CASES = [
    (4, 256, 1, 2),
    (2, 256, 17, 17),        # 289
    (4, 7, 31, 33),          # 1 023: element-wise kernels
    (2, 7, 32, 32),          # 1 024: plane kernels, one chunk
    (1, 3, 64, 128),         # 8 192
    (1, 7, 3, 2731),         # 8 193: two apply chunks
    (2, 3, 128, 128),        # 16 384: one reduction chunk
    (1, 3, 5, 3277),         # 16 385: two reduction chunks
    (2, 7, 100, 100),        # bound 30, second BN
    (1, 7, 167, 167),        # bound 50, second BN
    (2, 3, 200, 200),        # bound 30, first BN
    (2, 3, 334, 334),
    (1, 3, 1025, 1025),      # hw > 64 * 16 384: both chunk counts capped at 64
]
# bars relative to max |ref| (fp32 arithmetic on fp64 statistics); worst measured on the MI355X: y 1.3e-7, dx 1.7e-7,
# dweight 6.4e-7 (eval), dbias 4.7e-8, running statistics 8.6e-8
TOL_Y, TOL_DX, TOL_PARAM, TOL_STATS = 1e-6, 1e-6, 4e-6, 1e-6


def _poison(*tensors):
    """leave NaN-filled blocks of these sizes in torch's caching allocator: the outputs batch_norm allocates next with
    torch.empty* are pre-filled with NaN, so an element no kernel writes fails the comparison"""
    held = [torch.full_like(t, float("nan")) for t in tensors for _ in range(2)]
    del held
    probe = torch.empty_like(tensors[0])
    assert bool(torch.isnan(probe).all()), "the caching allocator did not hand the NaN block back"
    del probe


def _close(got, ref, tol, what):
    err = float((got.double() - ref).abs().max()) if ref.numel() else 0.0
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    assert err <= tol * scale + 1e-30, f"{what}: max error {err:.3g} > {tol} x max|ref| {scale:.3g}"
    return err / scale if scale else 0.0


@pytest.mark.parametrize("B,C,H,W", CASES)
def test_batchnorm2d_nchw_vs_float64(B, C, H, W, record_property):
    import lidog_amd.me as ME
    g = torch.Generator().manual_seed(B * 100003 + C * 1009 + H * W)
    x = (torch.randn((B, C, H, W), generator=g) * 2 + 0.5).cuda()
    dy = torch.randn((B, C, H, W), generator=g).cuda()
    bn = torch.nn.BatchNorm2d(C).cuda()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g))
        bn.bias.copy_(torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    w64, b64 = bn.weight.detach().double(), bn.bias.detach().double()
    x64, dy64 = x.double(), dy.double()
    relu_train = (H * W) % 2 == 0
    for training, relu in ((True, relu_train), (False, not relu_train)):
        bn.train(training)
        bn.weight.grad = bn.bias.grad = None
        rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
        xg = x.clone().requires_grad_(True)
        _poison(x, bn.weight)
        y = ME.batch_norm(xg, bn, hw=H * W, relu=relu)
        _poison(x, bn.weight)
        y.backward(dy)
        torch.cuda.synchronize()
        tag = "train" if training else "eval"
        if training:
            y64, rm64, rv64, saved = R.bn2d_train_fwd64(x64, w64, b64, rm0.double(), rv0.double(), bn.momentum, bn.eps,
                                                        relu)
            record_property(f"{tag}_rm", _close(bn.running_mean, rm64, TOL_STATS, "running_mean"))
            record_property(f"{tag}_rv", _close(bn.running_var, rv64, TOL_STATS, "running_var"))
        else:
            y64, saved = R.bn2d_eval_fwd64(x64, w64, b64, rm0.double(), rv0.double(), bn.eps, relu)
            assert torch.equal(bn.running_mean, rm0) and torch.equal(bn.running_var, rv0)
        record_property(f"{tag}_y", _close(y.detach(), y64, TOL_Y, f"{tag} y"))
        # the ReLU mask is the kernel's own output decision (an output within rounding of 0 may go either way)
        dx64, dw64, db64 = R.bn2d_bwd64(dy64, x64, y.detach().double(), w64, saved, training, relu)
        record_property(f"{tag}_dx", _close(xg.grad, dx64, TOL_DX, f"{tag} dx"))
        record_property(f"{tag}_dw", _close(bn.weight.grad, dw64, TOL_PARAM, f"{tag} dweight"))
        record_property(f"{tag}_db", _close(bn.bias.grad, db64, TOL_PARAM, f"{tag} dbias"))
