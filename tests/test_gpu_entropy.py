"""The entropy criterion (csrc/entropy.hip) through the C ABI against its float64 restatement (tests/entropy_ref.py), every
buffer between guard bands (tests/guard.py) with a band check after every call.

Tolerance: none is fixed in advance.  The same quantities are computed with torch float32 on the CPU (log_softmax ->
exp -> mul -> sum -> mean, gradient by autograd), that composition's max abs error against the float64 restatement is
measured on the same inputs, and the kernel may be at most 4 x that, for loss, row_h and glogits each.  The participating
set, coef[1] and coef[0] == float32(1 / k) are exact."""
import math

import numpy as np
import pytest
import torch

import entropy_ref as R
from guard import GuardArena

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 255, 256, 257, 70001]          # no row, one, around one workgroup, 69 workgroups of the grid-strided sweep
CLASSES = [2, 7, 19, 20]
FACTOR = 4.0
GOUT = -1.75


def make_logits(n, C, seed):
    """N(0, 3^2) float32 logits; from 255 rows on also 16 rows of equal logits, 16 + 8 rows with one logit at +-1e4 and
    8 + 8 rows with one at +-80 (the other logits of those rows stay random)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, C)) * 3.0).astype(np.float32)
    special = {}
    if n >= 255:
        x[0:16] = (rng.standard_normal((16, 1)) * 30.0).astype(np.float32)
        special["equal"] = np.arange(0, 16)
        for name, lo, hi, v in (("hot", 16, 32, 1e4), ("cold", 32, 40, -1e4), ("p80", 40, 48, 80.0), ("m80", 48, 56, -80.0)):
            rows = np.arange(lo, hi)
            x[rows, rng.integers(0, C, size=hi - lo)] = v
            special[name] = rows
    return x, special


def separate_from_margin(x, margin, seed):
    """redraw (N(0, 3^2)) every row whose float64 entropy lies within 1e-3 of the margin until none does"""
    rng = np.random.default_rng([seed, 1])
    for _ in range(100):
        near = np.abs(R.rows64(x)[0] - np.float64(np.float32(margin))) <= 1e-3
        if not near.any():
            return x
        x[near] = (rng.standard_normal((int(near.sum()), x.shape[1])) * 3.0).astype(np.float32)
    raise AssertionError("rows stay near the margin")


def torch_cpu(x, take, gout):
    """(loss, row_h, grad) of the float32 CPU composition over the rows `take`"""
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    logp = torch.log_softmax(xt, dim=1)
    h = -(logp.exp() * logp).sum(dim=1)
    k = int(take.sum())
    if k == 0:
        return 0.0, h.detach().numpy(), np.zeros_like(x)
    loss = h[torch.from_numpy(take)].mean()
    (loss * gout).backward()
    return float(loss.detach()), h.detach().numpy(), xt.grad.numpy()


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).view(np.uint8)


def run_kernels(x, mask, margin, gout, arena):
    """one forward and one backward call on banded buffers -> dict of device tensors"""
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    n, C = x.shape
    xd = arena.place(torch.from_numpy(x), "logits")
    md = arena.place(torch.from_numpy(mask.astype(np.uint8)), "mask") if mask is not None else None
    ws = arena.nan(_lib.load().lidog_entropy_ws(C), dtype=torch.float64, name="ws")
    loss, coef = arena.nan(1, name="loss"), arena.nan(2, name="coef")
    row_h = arena.nan(n, name="row_h")
    call("lidog_entropy_fwd", ptr(xd), ptr(md), n, C, float(margin), ptr(ws), ptr(loss), ptr(coef), ptr(row_h))
    arena.check("lidog_entropy_fwd")
    go = arena.place(torch.tensor([gout], dtype=torch.float32), "gout")
    g = arena.nan(n, C, name="glogits")
    call("lidog_entropy_bwd", ptr(xd), ptr(md), ptr(row_h), n, C, float(margin), ptr(coef), ptr(go), ptr(g))
    arena.check("lidog_entropy_bwd")
    return {"x": xd, "mask": md, "loss": loss, "coef": coef, "row_h": row_h, "g": g, "gout": go}


def check_case(x, mask, margin, special=None):
    n, C = x.shape
    ref = R.entropy64(x, mask, margin, GOUT)
    t_loss, t_h, t_g = torch_cpu(x, ref["take"], GOUT)
    arena = GuardArena()
    out = run_kernels(x, mask, margin, GOUT, arena)
    loss, coef = float(out["loss"]), out["coef"].cpu().numpy()
    h, g = out["row_h"].cpu().numpy(), out["g"].cpu().numpy()
    errs = {}
    for name, got, tor, want in (("loss", loss, t_loss, ref["loss"]), ("row_h", h, t_h, ref["row_h"]),
                                 ("glogits", g, t_g, ref["grad"])):
        got, tor = np.asarray(got, dtype=np.float64), np.asarray(tor, dtype=np.float64)
        errs[name] = (float(np.abs(got - want).max(initial=0.0)), float(np.abs(tor - want).max(initial=0.0)))
    print(f"entropy n={n} C={C} margin={margin:.4g} mask={'yes' if mask is not None else 'no'} k={ref['k']}: " +
          ", ".join(f"{k} kernel {a:.3g} torch-fp32 {b:.3g}" for k, (a, b) in errs.items()))
    assert np.isfinite(h).all() and np.isfinite(g).all() and math.isfinite(loss)
    # exact: the count, 1 / k, the participating set (zero bits elsewhere)
    assert coef[1] == ref["coef"][1] and coef.view(np.uint32)[0] == ref["coef"].view(np.uint32)[0]
    assert (bits(g).reshape(n, 4 * C)[~ref["take"]] == 0).all()
    if margin > 0:
        assert np.array_equal(R.taking(h.astype(np.float64), mask, margin), ref["take"])
    for name, (mine, torchs) in errs.items():
        assert mine <= FACTOR * torchs, (name, mine, torchs)
    if special:
        tol_h, tol_g = FACTOR * errs["row_h"][1], FACTOR * errs["glogits"][1]
        eq = special["equal"]
        assert (np.abs(h[eq].astype(np.float64) - math.log(C)) <= tol_h).all() and (np.abs(g[eq]) <= tol_g).all()
        hot = special["hot"]
        assert (h[hot] == 0).all() and (g[hot] == 0).all()
    # determinism: a second pair of calls gives the same bytes
    again = run_kernels(x, mask, margin, GOUT, arena)
    for k in ("loss", "coef", "row_h", "g"):
        assert np.array_equal(bits(out[k]), bits(again[k])), k
    return out, ref


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("n", SIZES)
def test_against_float64(n, C):
    x, special = make_logits(n, C, 100 * C + n % 97)
    out, ref = check_case(x, None, 0.0, special)
    assert ref["k"] == n
    if n == 0:
        assert float(out["loss"]) == 0 and out["coef"].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("n", [257, 70001])
def test_mask_and_margin(n, C):
    margin = float(np.float32(0.4 * math.log(C)))
    x, _ = make_logits(n, C, 7 * C + n % 89)
    x = separate_from_margin(x, margin, C + n)
    assert R.margin_gap(x, margin) > 1e-3                    # float32 and float64 agree on every row's side
    mask = np.random.default_rng(C).random(n) < 0.6
    for m, mg in ((mask, 0.0), (None, margin), (mask, margin)):
        _, ref = check_case(x, m, mg)
        assert 0 < ref["k"] < n
    # every row masked out
    out, ref = check_case(x, np.zeros(n, dtype=bool), margin)
    assert ref["k"] == 0 and float(out["loss"]) == 0 and out["coef"].tolist() == [0.0, 0.0]
    assert (bits(out["g"]) == 0).all()


@pytest.mark.parametrize("C", [1, 21])
def test_other_class_counts_return_2_before_any_launch(C):
    from lidog_amd import _lib
    from lidog_amd._lib import ptr
    lib, arena, n = _lib.load(), GuardArena(), 33
    x = arena.place(torch.randn(n, C), "logits")
    ws = arena.nan(2048, dtype=torch.float64, name="ws")
    loss, coef, row_h, g = arena.nan(1), arena.nan(2), arena.nan(n), arena.nan(n, C)
    go = arena.place(torch.ones(1), "gout")
    before = [bits(t).copy() for t in (ws, loss, coef, row_h, g)]
    assert lib.lidog_entropy_fwd(ptr(x), None, n, C, 0.0, ptr(ws), ptr(loss), ptr(coef), ptr(row_h), _lib.stream()) == 2
    assert lib.lidog_entropy_bwd(ptr(x), None, ptr(row_h), n, C, 0.0, ptr(coef), ptr(go), ptr(g), _lib.stream()) == 2
    arena.check("refused calls")
    for t, b in zip((ws, loss, coef, row_h, g), before):
        assert np.array_equal(bits(t), b)


@pytest.mark.parametrize("n,C", [(257, 7), (70001, 19)])
def test_entropy_loss_under_autograd(n, C):
    from lidog_amd.losses import EntropyLoss
    margin = float(np.float32(0.4 * math.log(C)))
    x, _ = make_logits(n, C, 5)
    mask = np.random.default_rng(6).random(n) < 0.7
    direct = run_kernels(x, mask, margin, 1.0, GuardArena())
    scaled = run_kernels(x, mask, margin, GOUT, GuardArena())
    crit = EntropyLoss(margin)
    for gout, want in ((1.0, direct), (GOUT, scaled)):
        xa = torch.from_numpy(x).cuda().requires_grad_(True)
        loss = crit(xa, torch.from_numpy(mask).cuda())
        assert loss.shape == () and crit.row_entropy.shape == (n,) and crit.taken.shape == ()
        (loss * gout if gout != 1.0 else loss).backward()
        assert np.array_equal(bits(loss), bits(want["loss"][0]))
        assert np.array_equal(bits(crit.row_entropy), bits(want["row_h"]))
        assert float(crit.taken) == float(want["coef"][1]) > 0
        assert np.array_equal(bits(xa.grad), bits(want["g"]))
    plain = EntropyLoss()                                        # no mask, no margin: every row
    loss = plain(torch.from_numpy(x).cuda())
    every = run_kernels(x, None, 0.0, 1.0, GuardArena())
    assert float(plain.taken) == n and np.array_equal(bits(loss), bits(every["loss"][0]))
    for bad in (torch.randn(8, 21, device="cuda"), torch.randn(8, 7, device="cuda", dtype=torch.float64)):
        with pytest.raises(NotImplementedError):
            plain(bad)
