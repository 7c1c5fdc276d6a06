"""The Lovasz-softmax kernels (csrc/lovasz.hip) against the float64 yardstick (tests/lovasz_ref.py), stage by stage, so
that no input has to be left out because two errors tie or lie closer than fp32 resolves:
  (A) err_out against the float64 errors within E_e;
  (B) coef and 1 / P bit for bit against the restatement fed with the kernel's own err_out;
  (C) loss against the float64 dot of those errors with the reference g (the fp64-sum bar), and against the full float64
      loss within max E_e;
  (D) the backward pass against the float64 Jacobian product of the kernel's coef, gout != 1 included;
  (E) end to end against the full float64 gradient on inputs whose sorted errors are separated by more than the sum of
      their bars (asserted from the float64 values: tests/test_lovasz_cpu.py holds it without a GPU);
  (F) two runs give the same bytes, and the module under autograd gives the bytes of the direct calls."""
import numpy as np
import pytest
import torch

import lovasz_ref as R

SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049]      # the wave, the sort chunk and scan block of 1024, two chunks + 1
CLASSES = [2, 7, 19, 20]
# (n, seed, scale) of (E): C = 7, default_rng(seed), logits N(0, scale) as float32, then labels from integers(-1, 7)
SEPARATED_CASES = [(n, seed, s) for n in (33, 65) for seed in range(12) for s in (1.0, 2.0)] + \
                  [(129, seed, 1.0) for seed in (1, 5, 8, 10)] + [(129, seed, 2.0) for seed in (4, 9, 10)]


def separated_case(n, seed, scale):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, 7)) * scale).astype(np.float32)
    return x, rng.integers(-1, 7, size=n)


def _dev(x, y, int32=False):
    return (torch.from_numpy(np.ascontiguousarray(x)).cuda(),
            torch.from_numpy(np.asarray(y)).to(torch.int32 if int32 else torch.int64).cuda())


def forward(x, y, ignore):
    """the direct ABI call on device tensors -> (loss [1], coef [n C + 1], err [C, n]); coef and err start as NaN: every
    entry has to be written"""
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    n, C = x.shape
    ws = torch.empty(_lib.load().lidog_lovasz_ws(n, C), dtype=torch.uint8, device=x.device)
    loss = torch.full((1,), float("nan"), device=x.device)
    coef = torch.full((n * C + 1,), float("nan"), device=x.device)
    err = torch.full((C, n), float("nan"), device=x.device)
    call("lidog_lovasz_fwd", ptr(x), ptr(y), n, C, 0 if ignore is None else ignore, 0 if ignore is None else 1, ptr(ws),
         ptr(loss), ptr(coef), ptr(err))
    return loss, coef, err


def backward(x, y, ignore, coef, gout):
    from lidog_amd._lib import call, ptr
    n, C = x.shape
    g = torch.full((n, C), float("nan"), device=x.device)
    go = torch.tensor([gout], dtype=torch.float32, device=x.device)
    call("lidog_lovasz_bwd", ptr(x), ptr(y), n, C, 0 if ignore is None else ignore, 0 if ignore is None else 1,
         ptr(coef), ptr(coef[n * C:]), ptr(go), ptr(g))
    return g


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ratio(err, bar):
    return err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))


def check_stages(x, y, ignore, gout=-1.75, int32=False):
    """(A) - (D) and (F) on one input; -> (kernel loss, coef [n, C], restatement of the kernel's errors)"""
    from lidog_amd.losses import LovaszSoftmaxLoss
    n, C = x.shape
    xd, yd = _dev(x, y)
    loss, coef, err = forward(xd, yd, ignore)
    loss_h, coef_h, err_h = float(loss), coef.cpu().numpy(), err.cpu().numpy()
    e64, _, ok = R.errors64(x, y, ignore)
    bars = R.error_bars(x, y, ignore)
    full = R.full64(x, y, ignore)
    r = R.from_errors(err_h, y, ignore)
    g = backward(xd, yd, ignore, coef, gout).cpu().numpy()
    want, bound = R.jacobian64(x, y, coef_h[:n * C], coef_h[n * C], ignore, gout)
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"lovasz n={n} C={C}: err {np.nanmax(np.abs(err_h - e64) / bars, initial=0):.3g} x the bar, loss "
              f"{_ratio(abs(loss_h - r['loss']), R.loss_bound_sum(r)):.3g} x the sum bar, "
              f"{_ratio(abs(loss_h - full['loss']), R.loss_bound_errors(x, y, ignore, full['loss'])):.3g} x the error bar, "
              f"backward {np.nanmax(np.abs(g - want) / bound, initial=0):.3g} x the bar")
    # (A)
    assert not np.isnan(err_h).any() and (err_h[:, ~ok] == 0).all() and not np.signbit(err_h[:, ~ok]).any()
    assert (err_h >= 0).all() and (err_h <= 1).all()
    assert (np.abs(err_h.astype(np.float64) - e64) <= bars).all()
    # (B)
    assert np.array_equal(_bits(coef_h[:n * C].reshape(n, C)), _bits(r["coef"]))
    assert _bits(coef_h[n * C:])[0] == _bits(r["inv_p"])
    # (C)
    assert abs(loss_h - r["loss"]) <= R.loss_bound_sum(r)
    assert abs(loss_h - full["loss"]) <= R.loss_bound_errors(x, y, ignore, full["loss"])
    # (D)
    assert not np.isnan(g).any() and (np.abs(g.astype(np.float64) - want) <= bound).all()
    assert (g[~ok] == 0).all() and not np.signbit(g[~ok]).any()
    # (F)
    loss2, coef2, err2 = forward(xd, yd, ignore)
    assert torch.equal(loss2.view(torch.int32), loss.view(torch.int32))
    assert torch.equal(coef2.view(torch.int32), coef.view(torch.int32))
    assert torch.equal(err2.view(torch.int32), err.view(torch.int32))
    xa = xd.clone().requires_grad_(True)
    la = LovaszSoftmaxLoss(ignore_label=ignore)(xa, _dev(x, y, int32)[1] if int32 else yd)
    (la * gout).backward()
    assert la.shape == () and la.view(torch.int32).item() == loss.view(torch.int32).item()
    assert np.array_equal(_bits(xa.grad.cpu().numpy()), _bits(g))
    return loss_h, coef_h[:n * C].reshape(n, C), r


def random_case(n, C, seed, scale):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, C)) * scale).astype(np.float32), rng.integers(-1, C, size=n)


@pytest.mark.gpu
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("n", SIZES)
def test_stages_on_random_rows(n, C):
    x, y = random_case(n, C, 1000 * C + n, 1.0 if n % 2 else 3.0)
    check_stages(x, y, -1)


@pytest.mark.gpu
def test_every_row_ignored():
    x, _ = random_case(65, 7, 1, 1.0)
    loss, coef, _ = check_stages(x, np.full(65, -1), -1)
    assert loss == 0 and (coef == 0).all() and not np.signbit(coef).any()
    xd, yd = _dev(x, np.full(65, -1))
    _, c, _ = forward(xd, yd, -1)
    assert float(c[-1]) == 0
    g = backward(xd, yd, -1, c, 3.0).cpu().numpy()
    assert (g == 0).all() and not np.signbit(g).any()


@pytest.mark.gpu
def test_no_rows():
    xd, yd = _dev(np.zeros((0, 7), dtype=np.float32), np.zeros(0, dtype=np.int64))
    loss, coef, _ = forward(xd, yd, -1)
    assert float(loss) == 0 and float(coef[0]) == 0
    assert backward(xd, yd, -1, coef, 1.0).shape == (0, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 1025])
def test_one_class_present_and_every_row_of_one_class(n):
    x, y = random_case(n, 7, 2, 2.0)
    y = np.where(y >= 0, 3, -1)                             # one class present, next to ignored rows
    _, coef, r = check_stages(x, y, -1)
    assert r["P"] == 1 and (coef[:, [0, 1, 2, 4, 5, 6]] == 0).all()
    _, coef, r = check_stages(x, np.full(n, 5), -1)         # every row of one class
    assert r["P"] == 1 and r["m"] == n and (coef[:, 5] <= 0).all()
    check_stages(x, np.full(n, 5), 5)                       # ... which is the ignore label


@pytest.mark.gpu
def test_labels_outside_the_classes_and_no_ignore_label():
    x, y = random_case(257, 7, 3, 1.0)
    y[:6] = (7, 100, -2, -1, 2 ** 40, -2 ** 40)
    _, coef, _ = check_stages(x, y, None)                   # -1 is outside too when nothing is ignored
    assert (coef[:6] == 0).all()
    check_stages(x, y, 2)                                   # an ignore label inside [0, C)
    check_stages(x, np.abs(y) % 7, None)                    # every row valid


@pytest.mark.gpu
def test_duplicated_rows_tie_by_row_index():
    x, y = random_case(8, 7, 4, 1.0)
    x, y = np.tile(x, (40, 1)), np.tile(y, 40)              # 320 rows, every error 40 times
    y[::3] = (y[::3] + 1) % 7                               # the copies differ in their labels
    loss, coef, r = check_stages(x, y, -1)
    same = np.zeros((64, 7), dtype=np.float32)
    check_stages(same, np.arange(64) % 7, -1)               # every error of a class ties


@pytest.mark.gpu
@pytest.mark.parametrize("spread", [60.0, 200.0])
def test_saturated_rows_use_sign_zero(spread):
    """a spread of 60 makes the largest p exactly 1.0 in fp32, one of 200 the others exactly 0.0: e = 0 there, and the
    coefficient is +0 whatever g is"""
    x, y = random_case(130, 7, 5, 0.01)
    hot = np.arange(130) % 7
    x[np.arange(130), hot] += spread
    y = np.where(np.arange(130) % 2 == 0, hot, y)           # half the rows labelled with their saturated class
    _, coef, r = check_stages(x, y, -1)
    xd, yd = _dev(x, y)
    err = forward(xd, yd, -1)[2].cpu().numpy()
    zero = (err.T == 0) & R.valid_rows(y, 7, -1)[:, None]
    assert zero.sum() >= 65 * (1 if spread < 100 else 6)
    assert (coef[zero] == 0).all() and not np.signbit(coef[zero]).any()


@pytest.mark.gpu
def test_module_refuses_other_shapes_and_dtypes():
    from lidog_amd.losses import LovaszSoftmaxLoss
    crit, y = LovaszSoftmaxLoss(ignore_label=-1), torch.zeros(8, dtype=torch.long, device="cuda")
    for x in (torch.randn(8, 21, device="cuda"), torch.randn(8, 1, device="cuda"), torch.randn(8, 7, 1, device="cuda"),
              torch.randn(8, 7, device="cuda", dtype=torch.float64)):
        with pytest.raises(NotImplementedError):
            crit(x, y)


@pytest.mark.gpu
def test_int32_labels():
    x, y = random_case(1025, 19, 6, 1.0)
    check_stages(x, y, -1, int32=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,scale", SEPARATED_CASES)
def test_end_to_end_gradient_on_separated_errors(n, seed, scale):
    x, y = separated_case(n, seed, scale)
    assert R.separated(x, y, -1, factor=4.0) > 1.0          # the float32 errors sort as the float64 ones do
    full = R.full64(x, y, -1, gout=0.5)
    xd, yd = _dev(x, y)
    loss, coef, _ = forward(xd, yd, -1)
    coef_h = coef.cpu().numpy()
    g = backward(xd, yd, -1, coef, 0.5).cpu().numpy()
    # the same order: the kernel's g is the yardstick's, rounded to float32 once
    want = R.from_errors(full["e"], y, -1)
    assert np.array_equal(_bits(coef_h[:-1].reshape(n, 7)), _bits(want["coef"])) and coef_h[-1] == want["inv_p"]
    # q = float32(g) float32(1 / P): two roundings on top of the backward pass's own bar
    _, bound = R.jacobian64(x, y, coef_h[:-1], coef_h[-1], -1, 0.5)
    q = np.abs(full["g"]) / full["P"]
    extra = R.FACTOR * 0.5 * full["p"] * 2 * R.U * (q + (full["p"] * q).sum(axis=1, keepdims=True))
    assert (np.abs(g.astype(np.float64) - full["grad"]) <= bound + extra).all()
    assert abs(float(loss) - full["loss"]) <= R.loss_bound_errors(x, y, -1, full["loss"])
