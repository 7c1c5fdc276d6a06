"""The DICE losses (csrc/losses.hip) against their float64 yardstick (tests/dice_ref.py): the semantic logits of a
bench-shape batch (4 kitti120k scans, their own labels) and the BEV logits [4, 7, 167, 167] read through .view(-1, 7)
with rasterised labels (mostly ignored pixels), past 2^20 rows where the grid stops growing (every thread then adds more
than 4 rows and the finish walks 1024 partials), every flag, eps, neg_range and an upstream gradient of 0.5, and the
data edges: every row ignored, one row, a class in one row, absent classes, saturated and equal logits.

Direct calls pre-fill the loss, the coefficients and the gradient with NaN.  Checks: loss and gradient within their
bars, ignored rows exactly 0, a repeat bit-identical."""
import functools

import pytest
import torch

import dice_ref as D

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _direct(x, y, ignore, soft, eps, powerize, use_tmask, neg_range, gout):
    from lidog_amd._lib import call, load, ptr
    n, C = x.shape
    ws = torch.full((load().lidog_dice_ws(C),), NAN, dtype=torch.float64, device="cuda")
    loss = torch.full((), NAN, device="cuda")
    coef = torch.full((2 * C,), NAN, device="cuda")
    cfg = (n, C, int(ignore) if ignore is not None else 0, 1 if ignore is not None else 0, float(eps), int(soft),
           int(powerize))
    call("lidog_dice_fwd", ptr(x), ptr(y), *cfg, int(use_tmask), -1.0 if neg_range else 0.0, ptr(ws), ptr(loss),
         ptr(coef))
    g = torch.full_like(x, NAN)
    go = torch.full((), gout, device="cuda")
    call("lidog_dice_bwd", ptr(x), ptr(y), *cfg, ptr(coef), ptr(go), ptr(g))
    return loss, g


def _check(x, y, ignore=-1, soft=True, eps=0.05, powerize=True, use_tmask=True, neg_range=False, gout=1.0,
           record_property=None, tag=""):
    r = D.dice64(x, y, ignore, soft, eps, powerize, use_tmask, neg_range, gout)
    loss, g = _direct(x, y, ignore, soft, eps, powerize, use_tmask, neg_range, gout)
    rl = abs(float(loss) - float(r.loss)) / D.loss_bound(r)
    rg = D.grad_ratio(g, r, D.grad_bound(r, x, y))
    assert rl <= 1, f"{tag}: loss {float(loss)!r} vs {float(r.loss)!r}: {rl:.3g} x the bar"
    assert rg <= 1, f"{tag}: gradient {rg:.3g} x the bar (NaN: never written)"
    if ignore is not None:
        ign = y == ignore
        assert bool((g[ign] == 0).all()) and not bool(torch.signbit(g[ign]).any()), f"{tag}: ignored rows"
    loss2, g2 = _direct(x, y, ignore, soft, eps, powerize, use_tmask, neg_range, gout)
    assert torch.equal(loss2.view(torch.int32), loss.view(torch.int32)) and torch.equal(g2.view(torch.int32),
                                                                                          g.view(torch.int32))
    if record_property is not None:
        record_property(f"{tag}_loss", rl)
        record_property(f"{tag}_grad", rg)
    return r, loss, g


@functools.lru_cache(maxsize=None)
def _bench_batch():
    from lidog_amd import data, synth
    b = synth.make_batch(range(4), "kitti120k", "cuda")
    bev, _ = data.bev_labels(b["coords_int"], b["source_sem_labels0"], bound=50.0, img_size=167, batch_size=4)
    return b["coords_int"], b["source_sem_labels0"], bev


def _logits(n, C, seed, scale=3.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, C, device="cuda", generator=g) * scale


def test_semantic_logits_at_bench_shape(record_property):
    """the module path (SoftDICELoss, as the step calls it) and the direct calls on 4 kitti120k scans"""
    from lidog_amd.losses import SoftDICELoss
    coords, labels, _ = _bench_batch()
    n = coords.shape[0]
    assert n > 300_000
    x = _logits(n, 7, 1)
    r, loss, g = _check(x, labels, record_property=record_property, tag="sem")
    xg = x.clone().requires_grad_(True)
    lm = SoftDICELoss(ignore_label=-1)(xg, labels)
    lm.backward(torch.tensor(0.5, device="cuda"))
    assert torch.equal(lm.detach().view(torch.int32), loss.view(torch.int32))
    assert torch.equal(xg.grad, 0.5 * g)      # the upstream gradient 0.5 scales exactly (a power of two)


def test_bev_logits_through_view(record_property):
    """[4, 7, 167, 167] NCHW logits read through .view(-1, 7), labels from the BEV label raster (mostly ignored)"""
    from lidog_amd.losses import DICELoss
    _, _, bev = _bench_batch()
    x = _logits(4 * 7 * 167 * 167, 1, 2).view(4, 7, 167, 167)
    y = bev.view(-1)
    assert float((y == -1).float().mean()) > 0.5
    r, loss, g = _check(x.view(-1, 7), y, soft=False, powerize=False, use_tmask=False, record_property=record_property,
                        tag="bev")
    xg = x.clone().requires_grad_(True)
    lm = DICELoss(ignore_label=-1)(xg.view(-1, 7), y)
    lm.backward()
    assert torch.equal(lm.detach().view(torch.int32), loss.view(torch.int32)) and torch.equal(xg.grad.view(-1, 7), g)


@pytest.mark.parametrize("n", [(1 << 20) + 1, 5 << 20])
@pytest.mark.parametrize("C", [2, 7, 20])
def test_past_the_grid_cap(n, C, record_property):
    """1024 workgroups: each thread adds ceil(n / 2^18) rows, the finish walks 1024 partials with 8 lanes each"""
    x = _logits(n, C, n + C, 4.0)
    g = torch.Generator(device="cuda").manual_seed(C)
    y = torch.randint(-1, C, (n,), device="cuda", generator=g)
    soft = C != 20
    _check(x, y, soft=soft, powerize=soft, use_tmask=soft, gout=0.5, record_property=record_property,
           tag=f"n{n}_C{C}")


FLAGS = [(s, p, m) for s in (True, False) for p in (True, False) for m in (True, False)]


@pytest.mark.parametrize("soft,powerize,use_tmask", FLAGS)
@pytest.mark.parametrize("eps,neg_range,gout", [(0.05, False, 1.0), (0.25, True, 0.5)])
def test_every_flag(soft, powerize, use_tmask, eps, neg_range, gout, record_property):
    """one class absent (the tmask drops it or keeps it), ignored rows"""
    n, C = 50_000, 7
    x = _logits(n, C, 7 + int(soft) + 2 * int(powerize) + 4 * int(use_tmask))
    y = torch.randint(-1, C - 1, (n,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    _check(x, y, -1, soft, eps, powerize, use_tmask, neg_range, gout, record_property, "flags")


def _case(kind, C=7):
    g = torch.Generator(device="cuda").manual_seed(len(kind))
    n = 20_000
    x = _logits(n, C, len(kind))
    y = torch.randint(0, C, (n,), device="cuda", generator=g)
    ignore = -1
    if kind == "all_ignored":
        y = torch.full_like(y, -1)
    elif kind == "one_row":
        x, y = x[:1], y[:1]
    elif kind == "class_in_one_row":
        y = torch.where(y == 3, torch.zeros_like(y), y)
        y[12345] = 3
    elif kind == "absent":
        y = torch.where(y >= 4, y - 4, y)
    elif kind == "saturated":
        x = torch.where(torch.rand(x.shape, device="cuda", generator=g) < 0.5, x.sign() * 80.0, x * 20).clamp(-80, 80)
    elif kind == "equal":
        x = torch.full_like(x, 0.37)
    elif kind == "ignore255":
        y = torch.where(torch.rand(n, device="cuda", generator=g) < 0.3, torch.full_like(y, 255), y)
        ignore = 255
    return x, y, ignore


CASES = ["all_ignored", "one_row", "class_in_one_row", "absent", "saturated", "equal", "ignore255"]


@pytest.mark.parametrize("kind", CASES)
@pytest.mark.parametrize("soft,use_tmask,neg_range", [(True, True, False), (True, False, True), (False, False, False),
                                                      (False, True, True)])
def test_data_cases(kind, soft, use_tmask, neg_range, record_property):
    x, y, ignore = _case(kind)
    r, loss, g = _check(x, y, ignore, soft, 0.05, soft, use_tmask, neg_range, 1.0, record_property, kind)
    if kind == "all_ignored":
        assert float(loss) == (0.0 if neg_range else 1.0)
        assert bool((g == 0).all())
    if kind == "saturated":
        assert bool((torch.softmax(x, 1) == 0).any())      # p underflows to 0
