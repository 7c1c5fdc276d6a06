"""RobustNet's instance-whitening loss on the device (csrc/iwloss.hip via lidog_amd.losses) against the float64 literal
IWLoss of tests/robust_ref.py (utils/losses/losses.py:464-485): loss within 1e-5 relative, gradient within 2e-5 relative
per element (a sum of <= 128 non-negative float32 terms), bit-identical repeats, the multi-map launch against per-map
calls, the reference call signature and its mask check, and n < 2."""
import pytest
import torch

from robust_ref import iw_literal

pytestmark = pytest.mark.gpu

CHUNK_ELEMS = 1 << 26   # bmm intermediate elements per chunk of the float64 literal (512 MB)


def _literal64(x):
    """(loss, gradient) of the literal IWLoss in float64, in row chunks (the [n, C, C] intermediates of n = 65 537,
    C = 128 would need 8.6 GB): the loss is a sum over rows, each scaled by 1 / (n (n - 1))"""
    n, C = x.shape
    rows = max(1, CHUNK_ELEMS // (C * C))
    total = torch.zeros((), dtype=torch.float64, device=x.device)
    grad = torch.empty((n, C), dtype=torch.float64, device=x.device)
    mask = torch.ones((C, C), dtype=torch.float64, device=x.device).triu(1)
    eye = torch.eye(C, dtype=torch.float64, device=x.device)
    for s in range(0, n, rows):
        xc = x[s:s + rows].double().requires_grad_(True)
        v = xc.reshape(-1, C, 1)
        f_cor = torch.bmm(v, v.transpose(1, 2)).div(n - 1) + 1e-5 * eye
        part = torch.sum(torch.sum(torch.abs(f_cor * mask), dim=(1, 2), keepdim=True)) / n
        part.backward()
        grad[s:s + rows] = xc.grad
        total += part.detach()
    return total, grad


def _map(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, C), generator=g) * 2.0
    x[torch.rand((n, C), generator=g) < 0.2] = 0.0          # exact zeros
    x[torch.randint(0, n, (max(1, n // 10),), generator=g)] = 0.0   # all-zero rows
    if n >= 3:
        x[1] = torch.rand(C, generator=g) * 1e-3
        x[1, C // 2] = 1e3                                  # one dominant channel
    return x.cuda()


def _check(x, loss, grad):
    ref, rgrad = _literal64(x)
    rel = abs(float(loss) - float(ref)) / max(float(ref), 1e-300)
    assert rel <= 1e-5, (tuple(x.shape), float(loss), float(ref), rel)
    err = (grad.double() - rgrad).abs()
    bad = err > 2e-5 * rgrad.abs()
    assert not bool(bad.any()), (tuple(x.shape), float((err / rgrad.abs().clamp_min(1e-300)).max()))
    assert bool(((x == 0) <= (grad == 0)).all())      # sign(0) = 0


@pytest.mark.timeout(120)
@pytest.mark.parametrize("C", [3, 7, 32, 64, 128])
def test_iw_loss_and_gradient_against_the_float64_literal(C):
    from lidog_amd.losses import iw_loss
    for n in (2, 3, 1000, 65537):
        x = _map(n, C, seed=n * 7 + C).requires_grad_(True)
        loss, per = iw_loss([x], scale=1.0)
        loss.backward()
        assert float(per[0]) == float(loss.detach())
        _check(x.detach(), loss.detach(), x.grad)


@pytest.mark.timeout(60)
def test_iw_loss_is_bit_identical_on_a_repeated_run():
    from lidog_amd.losses import iw_loss
    maps0 = [_map(352 * 50, 32, 1), _map(20000, 64, 2), _map(5000, 128, 3), _map(999, 7, 4)]
    outs = []
    for _ in range(2):
        maps = [m.clone().requires_grad_(True) for m in maps0]
        total, per = iw_loss(maps)
        total.backward()
        outs.append([total.detach(), per] + [m.grad for m in maps])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.timeout(60)
def test_five_map_launch_equals_the_per_map_calls():
    from lidog_amd.losses import iw_loss
    maps0 = [_map(30000, 32, 11), _map(9000, 32, 12), _map(9000, 32, 13), _map(3000, 64, 14), _map(800, 128, 15)]
    maps = [m.clone().requires_grad_(True) for m in maps0]
    total, per = iw_loss(maps, scale=1.0)
    total.backward()
    singles = []
    for m0, m in zip(maps0, maps):
        one = m0.clone().requires_grad_(True)
        t, _ = iw_loss([one], scale=1.0)
        t.backward()
        singles.append(float(t))
        assert torch.equal(one.grad, m.grad)             # elementwise: no dependence on the launch's slicing
    assert torch.allclose(per.cpu().double(), torch.tensor(singles, dtype=torch.float64), rtol=1e-6, atol=0)
    assert abs(float(total) - sum(singles)) <= 1e-6 * sum(singles)
    mean, _ = iw_loss([m.detach() for m in maps])       # default scale: the mean over the maps
    assert abs(float(mean) - sum(singles) / 5) <= 1e-6 * sum(singles)


@pytest.mark.timeout(30)
def test_reference_signature_mask_check_and_small_n():
    from lidog_amd.losses import CovMatrix_IRW, IWLoss, iw_loss
    x = _map(500, 32, 21)
    eye, mask, margin, num = CovMatrix_IRW(relax_denom=2.0)(x)
    assert eye.is_cuda and mask.is_cuda
    got = IWLoss()(x, eye, mask, margin, num)
    ref = iw_literal(x.double())
    assert abs(float(got) - float(ref)) <= 1e-5 * float(ref)
    with pytest.raises(ValueError):
        IWLoss()(x, eye, torch.ones_like(mask), margin, num)
    with pytest.raises(ValueError):
        iw_loss([torch.ones((1, 32), device="cuda")])
    with pytest.raises(ValueError):
        IWLoss()(torch.ones((1, 4), device="cuda"), eye[:4, :4], mask[:4, :4], margin, num)
