"""The cross-entropy family and the KITTI soft-label DICE (csrc/losses.hip) against their float64 yardstick
(tests/ce_ref.py): every row count at which the grid changes (one thread, one wave short of / exactly / past a workgroup,
several workgroups, past 2^20 rows where the grid stops growing), the smallest, the reference's, the 19- and the largest
class count, class weights (absent, random, one class at 0), both ignore labels, the focal parameters, an upstream gradient
of 0.5, and the data edges.

Direct calls pre-fill the loss, the coefficient, the workspace and the gradient with NaN.  Checks: loss and gradient within
their bars (NaN exactly where the yardstick is NaN), the rows that take no part exactly +0, a repeat bit-identical."""
import functools
import math

import numpy as np
import pytest
import torch

import ce_ref as R
import dice_ref as D

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _direct(x, y, ignore, weight, focal, gout):
    from lidog_amd._lib import call, load, ptr
    n, C = x.shape
    ws = torch.full((load().lidog_ce_ws(C),), NAN, dtype=torch.float64, device="cuda")
    loss = torch.full((), NAN, device="cuda")
    coef = torch.full((1,), NAN, device="cuda")
    cfg = (n, C, int(ignore) if ignore is not None else 0, 1 if ignore is not None else 0, ptr(weight))
    alpha, gamma = focal if focal is not None else (1.0, 0.0)
    call("lidog_ce_fwd", ptr(x), ptr(y), *cfg, 0 if focal is None else 1, float(alpha), float(gamma), ptr(ws), ptr(loss),
         ptr(coef))
    g = torch.full_like(x, NAN)
    go = torch.full((), gout, device="cuda")
    call("lidog_ce_bwd", ptr(x), ptr(y), *cfg, ptr(coef), ptr(go), ptr(g))
    return loss, g


def _check(x, y, ignore=-1, weight=None, focal=None, gout=1.0, cpu_yardstick=False, record_property=None, tag=""):
    if cpu_yardstick:
        r = R.degenerate(x, y, weight=weight, ignore=ignore, focal=focal, gout=gout)
        r.grad, r.scored = r.grad.cuda(), r.scored.cuda()
        r.weight = None if r.weight is None else r.weight.cuda()
    else:
        r = R.ce64(x, y, weight=weight, ignore=ignore, focal=focal, gout=gout)
    loss, g = _direct(x, y, ignore, weight, focal, gout)
    if math.isnan(float(r.loss)):
        assert math.isnan(float(loss)), f"{tag}: loss {float(loss)!r}, the yardstick is NaN"
        rl = 0.0
    else:
        bound = R.loss_bound(r)
        print(f"{tag}: loss {float(loss)!r} vs {float(r.loss)!r}, bar {bound:.3g}")
        rl = abs(float(loss) - float(r.loss)) / bound if bound > 0 else (0.0 if float(loss) == float(r.loss) else math.inf)
    rg = R.grad_ratio(g, r, R.grad_bound(r, x, y))
    print(f"{tag}: loss {rl:.3g} x the bar, gradient {rg:.3g} x the bar")
    assert rl <= 1, f"{tag}: loss {float(loss)!r} vs {float(r.loss)!r}: {rl:.3g} x the bar"
    assert rg <= 1, f"{tag}: gradient {rg:.3g} x the bar (inf: a NaN where the yardstick has none, or the reverse)"
    out = ~r.scored
    assert bool((g[out] == 0).all()) and not bool(torch.signbit(g[out]).any()), f"{tag}: rows that take no part"
    loss2, g2 = _direct(x, y, ignore, weight, focal, gout)
    assert torch.equal(_bits(loss2), _bits(loss)) and torch.equal(_bits(g2), _bits(g)), f"{tag}: repeat"
    if record_property is not None:
        record_property(f"{tag}_loss", rl)
        record_property(f"{tag}_grad", rg)
    return r, loss, g


def _logits(n, C, seed, scale=3.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, C, device="cuda", generator=g) * scale


def _labels(n, C, seed, lo=-1):
    return torch.randint(lo, C, (n,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def _weights(kind, C):
    if kind == "none":
        return None
    w = torch.rand(C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(C)) + 0.25
    if kind == "zero_class":
        w[C // 2] = 0.0
    return w


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025, (1 << 20) + 1])
@pytest.mark.parametrize("C", [2, 7, 19, 20])
def test_shapes(n, C, record_property):
    """(1 << 20) + 1 rows: past the grid cap of both kernels (1024 x 1024 rows forward, 4096 x 256 backward): one thread
    of each adds / writes a second round"""
    x = _logits(n, C, n + C, 4.0)
    y = _labels(n, C, C)
    if n == 1:
        y[0] = C - 1
    w = _weights("random" if C % 2 else "none", C)
    focal = (0.25, 2) if C in (7, 20) else None
    _check(x, y, -1, w, focal, 0.5 if n % 2 else 1.0, record_property=record_property, tag=f"n{n}_C{C}")


# ------------------------------------------------------------------ 2. variants
@pytest.mark.parametrize("wkind", ["none", "random", "zero_class"])
@pytest.mark.parametrize("ignore", [-1, 255])
@pytest.mark.parametrize("focal", [None, (0.25, 2), (0.5, 0), (1, 1.5)])
def test_variants(wkind, ignore, focal, record_property):
    n, C = 5000, 7
    x = _logits(n, C, 11)
    y = _labels(n, C, 12, lo=0)
    y = torch.where(torch.rand(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(13)) < 0.3,
                    torch.full_like(y, ignore), y)
    w = _weights(wkind, C)
    r, loss, g = _check(x, y, ignore, w, focal, 1.0, record_property=record_property, tag="variant")
    assert int((~r.scored).sum()) > 1000 and math.isfinite(float(loss))
    # an upstream gradient of 0.5 scales exactly (a power of two), the loss does not move
    loss_h, g_h = _direct(x, y, ignore, w, focal, 0.5)
    assert torch.equal(_bits(loss_h), _bits(loss)) and torch.equal(g_h, 0.5 * g)
    if ignore == 255:       # the other label is an ordinary out-of-range one then: no part, no read of the weights
        y2 = y.clone()
        y2[:100] = -1
        r2, _, g2 = _check(x, y2, ignore, w, focal, 1.0, tag="variant_other_label")
        assert not bool(r2.scored[:100].any())


def test_no_ignore_label():
    """ignore_label=None: every row with a label in [0, C) counts, -1 included in none"""
    n, C = 3000, 7
    x, y = _logits(n, C, 21), _labels(n, C, 22, lo=0)
    r, _, _ = _check(x, y, None, _weights("random", C), None, 1.0, tag="no_ignore")
    assert bool(r.scored.all())


# ------------------------------------------------------------------ 3. data cases
def _case(kind, C=7):
    g = torch.Generator(device="cuda").manual_seed(len(kind))
    n = 20_000
    x = _logits(n, C, len(kind))
    y = torch.randint(0, C, (n,), device="cuda", generator=g)
    if kind == "all_ignored":
        y = torch.full_like(y, -1)
    elif kind == "one_row":
        x, y = x[:1].contiguous(), y[:1].contiguous()
    elif kind == "class_in_one_row":
        y = torch.where(y == 3, torch.zeros_like(y), y)
        y[12345] = 3
    elif kind == "absent":
        y = torch.where(y >= 4, y - 4, y)
    elif kind == "saturated":
        x = torch.where(torch.rand(x.shape, device="cuda", generator=g) < 0.5, x.sign() * 80.0, x * 20).clamp(-80, 80)
    elif kind == "equal":
        x = torch.full_like(x, 0.37)
    elif kind == "out_of_range":
        y[::7] = C + 3
        y[1::11] = -1
    return x, y


CASES = ["all_ignored", "one_row", "class_in_one_row", "absent", "saturated", "equal", "out_of_range"]


@pytest.mark.parametrize("kind", CASES)
@pytest.mark.parametrize("focal", [None, (0.25, 2)])
def test_data_cases(kind, focal, record_property):
    x, y = _case(kind)
    w = _weights("random", 7) if kind in ("class_in_one_row", "out_of_range") else None
    r, loss, g = _check(x, y, -1, w, focal, 1.0, cpu_yardstick=kind == "all_ignored", record_property=record_property,
                        tag=kind)
    if kind == "all_ignored":
        assert math.isnan(float(loss)) and bool((g == 0).all())
    if kind == "saturated":
        assert bool((torch.softmax(x, 1) == 0).any())      # p underflows to 0
    if kind == "equal":
        assert abs(r.ce - math.log(7)) < 1e-12
    if kind == "out_of_range":
        assert bool((g[::7] == 0).all()) and int((~r.scored).sum()) > 4000


def test_zero_total_weight_and_zero_ce():
    """torch's own answers: NaN loss and NaN gradient in the scored rows when every weight is 0; loss 0 and gradient 0
    for the focal loss at ce == 0"""
    x, y = _case("absent")
    y[::5] = -1
    r, loss, g = _check(x, y, -1, torch.zeros(7, device="cuda"), None, 1.0, cpu_yardstick=True, tag="zero_weight")
    assert math.isnan(float(loss)) and bool(torch.isnan(g[y != -1]).all())
    one = torch.zeros(1, 7, device="cuda")
    one[0, 3] = 800.0
    r, loss, g = _check(one, torch.tensor([3], device="cuda"), -1, None, (1, 1.5), 1.0, cpu_yardstick=True, tag="zero_ce")
    assert float(loss) == 0 and bool((g == 0).all())


# ------------------------------------------------------------------ 4. the modules
@pytest.mark.parametrize("C", [7, 19])
def test_module_path_equals_direct_path(C):
    from lidog_amd.losses import CELoss, FocalLoss
    n = 4097
    x, y = _logits(n, C, 31 + C), _labels(n, C, 32)
    w = _weights("random", C)
    half = torch.tensor(0.5, device="cuda")
    for crit, weight, focal in ((CELoss(ignore_label=-1), None, None),
                                (CELoss(ignore_label=-1, weight=w.cpu().numpy()), w, None),
                                (FocalLoss(alpha=0.25, gamma=2), None, (0.25, 2)),
                                (FocalLoss(alpha=1, gamma=1.5, weight=w, ignore_index=-1), w, (1, 1.5))):
        loss, g = _direct(x, y, -1, weight, focal, 0.5)
        xg = x.clone().requires_grad_(True)
        lm = crit(xg, y)
        lm.backward(half)
        assert torch.equal(_bits(lm.detach()), _bits(loss)) and torch.equal(_bits(xg.grad), _bits(g))
        xi = x.clone().requires_grad_(True)                # int32 labels are converted, not reinterpreted
        assert torch.equal(_bits(crit(xi, y.int()).detach()), _bits(loss))


def test_module_checks():
    from lidog_amd.losses import CELoss, FocalLoss, SoftDICELoss
    y = torch.zeros(8, dtype=torch.long, device="cuda")
    for crit in (CELoss(ignore_label=-1), FocalLoss()):
        for bad in (torch.randn(8, 21, device="cuda"), torch.randn(8, 1, device="cuda"),
                    torch.randn(8, 7, device="cuda").double(), torch.randn(2, 4, 7, device="cuda")):
            with pytest.raises(NotImplementedError):
                crit(bad, y)
    with pytest.raises(ValueError):
        CELoss(weight=np.ones(8))(torch.randn(8, 7, device="cuda"), y)
    with pytest.raises(ValueError):
        SoftDICELoss(ignore_label=-1, is_kitti=True)(torch.randn(8, 6, device="cuda"), y)
    with pytest.raises(ValueError):
        SoftDICELoss(ignore_label=-1)(torch.randn(8, 6, device="cuda"), y, is_kitti=True)


@functools.lru_cache(maxsize=None)
def _bev_labels():
    from lidog_amd import data, synth
    b = synth.make_batch(range(4), "kitti120k", "cuda")
    bev, _ = data.bev_labels(b["coords_int"], b["source_sem_labels0"], bound=50.0, img_size=167, batch_size=4)
    return bev


@pytest.mark.parametrize("focal", [None, (0.25, 2)])
def test_bev_logits_through_view(focal, record_property):
    """[4, 7, 167, 167] NCHW logits read through .view(-1, 7), labels from the BEV label raster (mostly ignored)"""
    from lidog_amd.losses import CELoss, FocalLoss
    y = _bev_labels().view(-1)
    x = _logits(4 * 7 * 167 * 167, 1, 2).view(4, 7, 167, 167)
    assert float((y == -1).float().mean()) > 0.5
    r, loss, g = _check(x.view(-1, 7), y, -1, None, focal, 1.0, record_property=record_property, tag="bev")
    xg = x.clone().requires_grad_(True)
    crit = CELoss(ignore_label=-1) if focal is None else FocalLoss(*focal)
    lm = crit(xg.view(-1, 7), y)
    lm.backward()
    assert torch.equal(_bits(lm.detach()), _bits(loss)) and torch.equal(_bits(xg.grad.view(-1, 7)), _bits(g))


# ------------------------------------------------------------------ 5. KITTI soft-label DICE
def _kitti_direct(x, y, ignore, eps, powerize, use_tmask, neg_range, gout):
    from lidog_amd._lib import call, load, ptr
    n, C = x.shape
    ws = torch.full((load().lidog_dice_ws(C),), NAN, dtype=torch.float64, device="cuda")
    loss = torch.full((), NAN, device="cuda")
    coef = torch.full((2 * C,), NAN, device="cuda")
    cfg = (n, C, int(ignore) if ignore is not None else 0, 1 if ignore is not None else 0, float(eps), int(powerize))
    call("lidog_dice_kitti_fwd", ptr(x), ptr(y), *cfg, int(use_tmask), -1.0 if neg_range else 0.0, ptr(ws), ptr(loss),
         ptr(coef))
    g = torch.full_like(x, NAN)
    go = torch.full((), gout, device="cuda")
    call("lidog_dice_kitti_bwd", ptr(x), ptr(y), *cfg, ptr(coef), ptr(go), ptr(g))
    return loss, g


@pytest.mark.parametrize("C", [19, 7])
@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("powerize,use_tmask,neg_range,gout", [(True, True, False, 1.0), (False, False, True, 0.5)])
def test_kitti_soft_dice(C, paired, powerize, use_tmask, neg_range, gout, record_property):
    from lidog_amd.losses import SoftDICELoss
    n = 30_001
    x, y = _logits(n, C, 41 + C), _labels(n, C, 42)
    if not paired:
        y = torch.where((y == 1) | (y == 6), torch.full_like(y, 2), y)
    r = R.kitti_dice64(x, y, -1, 0.05, powerize, use_tmask, neg_range, gout)
    loss, g = _kitti_direct(x, y, -1, 0.05, powerize, use_tmask, neg_range, gout)
    rl = abs(float(loss) - float(r.loss)) / D.loss_bound(r)
    rg = D.grad_ratio(g, r, R.kitti_grad_bound(r, x, y))
    print(f"kitti C{C}: loss {rl:.3g} x the bar, gradient {rg:.3g} x the bar")
    assert rl <= 1 and rg <= 1, (rl, rg)
    ign = y == -1
    assert bool((g[ign] == 0).all()) and not bool(torch.signbit(g[ign]).any())
    loss2, g2 = _kitti_direct(x, y, -1, 0.05, powerize, use_tmask, neg_range, gout)
    assert torch.equal(_bits(loss2), _bits(loss)) and torch.equal(_bits(g2), _bits(g))
    plain = SoftDICELoss(ignore_label=-1, powerize=powerize, use_tmask=use_tmask, neg_range=neg_range)
    if paired:      # the pairing is visible: the plain soft labels give a loss more than two bars away (one bar each)
        assert abs(float(plain(x, y)) - float(loss)) > 2 * D.loss_bound(r)
    else:           # no row labelled 1 or 6: the plain kernel's bits
        assert torch.equal(_bits(plain(x, y)), _bits(loss))
    # is_kitti through the constructor and through forward: the same bits, the direct calls' bits
    go = torch.tensor(gout, device="cuda")
    outs = []
    for crit, kw in ((SoftDICELoss(ignore_label=-1, powerize=powerize, use_tmask=use_tmask, neg_range=neg_range,
                                   is_kitti=True), {}), (plain, {"is_kitti": True})):
        xg = x.clone().requires_grad_(True)
        lm = crit(xg, y, **kw)
        lm.backward(go)
        outs.append((lm.detach(), xg.grad))
    for lm, gm in outs:
        assert torch.equal(_bits(lm), _bits(loss)) and torch.equal(_bits(gm), _bits(g))
    record_property(f"kitti_C{C}_loss", rl)
    record_property(f"kitti_C{C}_grad", rg)


# ------------------------------------------------------------------ 6. the reference's own results
@pytest.mark.parametrize("C", R.GOLDEN_CLASSES)
def test_golden_file_through_the_modules(C):
    """the modules against the reference's fp32 run: inside the kernels' bar plus the reference's own rounding"""
    from lidog_amd.losses import make_criterion
    from lidog_amd.losses import CELoss
    gold = np.load(R.G18)
    x, y, w = (t.cuda() for t in R.golden_case(C))
    assert np.array_equal(gold[f"c{C}/logits"], x.cpu().numpy())
    n = int((y != -1).sum())
    crits = {"ce": (make_criterion("CELoss", -1, C), dict(ignore=-1)),
             "wce": (CELoss(ignore_label=-1, weight=gold[f"c{C}/weights"]), dict(ignore=-1, weight=w)),
             "focal": (make_criterion("FocalLoss", -1, C), dict(ignore=-1, focal=(0.25, 2)))}
    for name, (crit, kw) in crits.items():
        r = R.ce64(x, y, **kw)
        xg = x.clone().requires_grad_(True)
        lm = crit(xg, y)
        lm.backward()
        gl, gg = float(gold[f"c{C}/{name}/loss"]), torch.from_numpy(gold[f"c{C}/{name}/grad"]).cuda().double()
        assert abs(float(lm.detach()) - gl) <= R.loss_bound(r) + R.reference_bound(n, r.M, C, abs(r.dl) * r.ce + abs(gl)), name
        bound = R.grad_bound(r, x, y) + R.reference_bound(n, r.M, C, float(r.grad.abs().max())) * r.scored.unsqueeze(1)
        assert bool(((xg.grad.double() - gg).abs() <= bound).all()), name
    r = R.kitti_dice64(x, y, -1)
    xg = x.clone().requires_grad_(True)
    crit = make_criterion("SoftDICELoss", -1, 19)        # the 19-class rule: is_kitti
    assert crit.is_kitti
    lm = crit(xg, y)
    lm.backward()
    gl, gg = float(gold[f"c{C}/kitti/loss"]), torch.from_numpy(gold[f"c{C}/kitti/grad"]).cuda().double()
    assert abs(float(lm.detach()) - gl) <= D.loss_bound(r) + R.reference_bound(n, r.M, C, 1.0)
    bound = R.kitti_grad_bound(r, x, y) + R.reference_bound(n, r.M, C, float(r.grad.abs().max())) * (y != -1).unsqueeze(1)
    assert bool(((xg.grad.double() - gg).abs() <= bound).all())
