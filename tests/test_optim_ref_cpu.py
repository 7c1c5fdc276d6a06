"""The float64 yardstick of the optimiser kernels (tests/optim_ref.py) is right, and its bars can fail -- no GPU.

1. adam64 / sgd64 equal torch.optim.Adam(foreach=False) / torch.optim.SGD(nesterov=True) on float64 tensors: 5 steps with
   torch's state carried over, one parameter without a gradient in the first two (its step count lags).  Each step is
   compared on its own from torch's state before it, to 1e-14 relative to the magnitudes that enter each output (the
   bounds' own sensitivities: bound / 2u >= |result|; relative to the result alone no two float64 evaluations of a
   cancelling g s + wd p agree to 1e-14).
2. A correct float32 implementation passes the bars: float32 torch.optim and a numpy float32 chain in torch's order stay
   inside adam_bounds / sgd_bounds on the shared data at steps 1, 7 and 100 000; the unfused chain is within twice
   float32 torch.optim's root-mean-square error / bound (the second bar of the model-layout GPU test).
3. Nine wrong variants of that chain leave the bounds on at least 1 % of the elements."""
import numpy as np
import pytest
import torch

import optim_ref as R

N = 1 << 16
LR, B1, B2, EPS, MU = 1e-2, 0.9, 0.999, 1e-8, 0.98
F = np.float32
ADAM_CONFIGS = [(step, s, wd) for step in (1, 7, 100000) for s in (1.0, 0.25) for wd in (0.0, 1e-4)]
SGD_CONFIGS = [(1, MU, 1e-4, 1.0), (0, MU, 1e-4, 0.25), (0, 0.0, 1e-4, 1.0), (1, MU, 0.0, 0.25)]


# ------------------------------------------------------------------ float32 chains in torch's order (and wrong ones)
def adam32(p, g, m, v, lr, b1, b2, eps, wd, step, s, variant=None, trace=None):
    """torch's _single_tensor_adam in numpy float32, one rounding per operation; `variant`: a wrong implementation"""
    b1f, b2f, eps, wd, s = F(b1), F(b2), F(eps), F(wd), F(1.0 if variant == "grad_scale_dropped" else s)
    st = step - 1 if variant == "beta_pow_step_minus_1" else step
    bc1, bc2 = 1.0 - float(b1f) ** st, 1.0 - float(b2f) ** st
    if variant == "no_bias_correction":
        bc1 = bc2 = 1.0
    lr_bc1, bc2s = F(float(F(lr)) / bc1), F(np.sqrt(bc2))
    t = {} if trace is None else trace
    t["gs"], t["wp"] = g * s, wd * p
    g1 = t["g1"] = t["gs"] if variant == "adamw" else t["gs"] + t["wp"]
    if variant == "adamw":
        p = p - p * (F(lr) * wd)
    t["d"] = g1 - m
    t["t"] = t["d"] * (F(1) - b1f)
    m1 = t["m1"] = m + t["t"]
    t["va"], t["k2g"] = v * b2f, (F(1) - b2f) * g1
    t["vb"] = t["k2g"] * g1
    v1 = t["v1"] = t["va"] + t["vb"]
    if variant == "eps_in_sqrt":
        den = np.sqrt(v1 / (bc2s * bc2s) + eps)
    elif variant == "sqrt_v_over_bc2":
        den = np.sqrt(v1) / F(bc2) + eps
    else:
        t["sq"] = np.sqrt(v1)
        t["q"] = t["sq"] / bc2s
        den = t["q"] + eps
    t["den"] = den
    t["r"] = m1 / den
    t["w"] = lr_bc1 * t["r"]
    p1 = t["p1"] = p - t["w"]
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return p1, m1, v1


def sgd32(p, g, buf, lr, mu, wd, nesterov, s, variant=None, trace=None):
    lr, mu, wd, s = F(lr), F(mu), F(wd), F(s)
    t = {} if trace is None else trace
    t["gs"], t["wp"] = g * s, wd * p
    if variant == "decay_after_momentum":
        b1 = buf * mu + t["gs"]
        step = (t["gs"] + mu * b1 if nesterov else b1) + t["wp"]
    else:
        g1 = t["g1"] = t["gs"] + t["wp"]
        t["bm"] = buf * mu
        b1 = t["bm"] + (g1 * (F(1) - mu) if variant == "dampened" else g1)
        t["mb"] = mu * b1
        step = g1 + t["mb"] if (nesterov and variant != "nesterov_ignored") else b1
    t["b1"], t["st"] = b1, step
    t["w"] = lr * step
    p1 = t["p1"] = p - t["w"]
    assert p1.dtype == b1.dtype == np.float32
    return p1, b1


# ------------------------------------------------------------------ torch.optim, one step from given state
def torch_adam(p, g, m, v, lr, b1, b2, eps, wd, step, s, dtype):
    q = torch.nn.Parameter(torch.from_numpy(p).to(dtype).clone())   # from_numpy shares p's memory
    opt = torch.optim.Adam([q], lr=R.f32(lr), betas=(R.f32(b1), R.f32(b2)), eps=R.f32(eps), weight_decay=R.f32(wd),
                           foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m).to(dtype).clone(),
                    "exp_avg_sq": torch.from_numpy(v).to(dtype).clone()}
    q.grad = torch.from_numpy(g).to(dtype) * torch.tensor(R.f32(s), dtype=dtype)
    opt.step()
    st = opt.state[q]
    return q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def torch_sgd(p, g, buf, lr, mu, wd, nesterov, s, dtype):
    q = torch.nn.Parameter(torch.from_numpy(p).to(dtype).clone())   # from_numpy shares p's memory
    opt = torch.optim.SGD([q], lr=R.f32(lr), momentum=R.f32(mu), weight_decay=R.f32(wd), nesterov=bool(nesterov),
                          foreach=False)
    if mu > 0:
        opt.state[q] = {"momentum_buffer": torch.from_numpy(buf).to(dtype).clone()}
    q.grad = torch.from_numpy(g).to(dtype) * torch.tensor(R.f32(s), dtype=dtype)
    opt.step()
    return q.detach().numpy(), (opt.state[q]["momentum_buffer"].numpy() if mu > 0 else None)


# ------------------------------------------------------------------ 1. the yardstick equals torch in float64
def _rel14(got, ref, bound, what):
    tol = 1e-14 * bound / (2 * R.U)
    bad = ~(np.abs(got - ref) <= tol)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ from torch float64 by more than 1e-14 relative"


@pytest.mark.parametrize("kind", ["Adam", "SGD"])
def test_yardstick_equals_torch_float64_over_five_steps_with_a_lagging_parameter(kind):
    sizes = (300, 257, 64)
    p0, _, _, _ = R.make_data(sum(sizes), 11)
    cuts = np.cumsum((0,) + sizes)
    params = [torch.nn.Parameter(torch.from_numpy(p0[a:b]).double()) for a, b in zip(cuts[:-1], cuts[1:])]
    hp = dict(lr=R.f32(LR), weight_decay=R.f32(1e-4), foreach=False)
    if kind == "Adam":
        opt = torch.optim.Adam(params, betas=(R.f32(B1), R.f32(B2)), eps=R.f32(EPS), **hp)
    else:
        opt = torch.optim.SGD(params, momentum=R.f32(MU), nesterov=True, **hp)
    steps = [0, 0, 0]
    for it in range(5):
        _, g, _, _ = R.make_data(sum(sizes), 100 + it)
        before = []
        for i, q in enumerate(params):
            st = opt.state.get(q, {})
            zero = np.zeros(sizes[i])
            before.append((q.detach().numpy().copy(),
                           st["exp_avg"].numpy().copy() if "exp_avg" in st else zero,
                           st["exp_avg_sq"].numpy().copy() if "exp_avg_sq" in st else zero,
                           st["momentum_buffer"].numpy().copy() if st.get("momentum_buffer") is not None else zero))
            q.grad = None if (i == 1 and it < 2) else torch.from_numpy(g[cuts[i]:cuts[i + 1]]).double()
        opt.step()
        for i, q in enumerate(params):
            pb, mb, vb, bb = before[i]
            if q.grad is None:
                assert np.array_equal(q.detach().numpy(), pb) and q not in opt.state
                continue
            steps[i] += 1
            gi = g[cuts[i]:cuts[i + 1]]
            what = f"{kind} step {it} parameter {i}"
            if kind == "Adam":
                assert float(opt.state[q]["step"]) == steps[i]
                a = (LR, B1, B2, EPS, 1e-4, steps[i], 1.0)
                p1, m1, v1 = R.adam64(pb, gi, mb, vb, *a, abi=False)
                e_p, e_m, e_v = R.adam_bounds(pb, gi, mb, vb, *a)
                _rel14(opt.state[q]["exp_avg"].numpy(), m1, e_m, what + " exp_avg")
                _rel14(opt.state[q]["exp_avg_sq"].numpy(), v1, e_v, what + " exp_avg_sq")
            else:
                a = (LR, MU, 1e-4, 1, 1.0)
                p1, b1 = R.sgd64(pb, gi, bb, *a)
                e_p, e_b = R.sgd_bounds(pb, gi, bb, *a)
                _rel14(opt.state[q]["momentum_buffer"].numpy(), b1, e_b, what + " momentum_buffer")
            _rel14(q.detach().numpy(), p1, e_p, what + " parameter")
    assert steps == [5, 3, 5]


def test_rounding_the_bias_corrections_as_the_entry_point_does_moves_the_step_by_two_roundings_at_most():
    """adam64(abi=True) (what the kernels are compared with) against abi=False (what torch float64 was compared with):
    only lr / bc1 and sqrt(bc2) differ, by one float32 rounding each"""
    p, g, m, v = R.make_data(N, 5)
    for step in (1, 7, 100000):
        a = (LR, B1, B2, EPS, 1e-4, step, 1.0)
        ca, ct = R._adam_chain(p, g, m, v, *a, True), R._adam_chain(p, g, m, v, *a, False)
        assert np.array_equal(ca["m1"], ct["m1"]) and np.array_equal(ca["v1"], ct["v1"])
        assert (np.abs(ca["w"] - ct["w"]) <= 2.02 * R.U * np.abs(ct["w"])).all()      # w: the update, p' = p - w
        lr_bc1, bc2s = R.bias_corrections(*a[:3], step)
        assert lr_bc1 == float(F(lr_bc1)) and bc2s == float(F(bc2s))


# ------------------------------------------------------------------ the shared data is what the issue asks for
def _normal(trace, what):
    for k, x in trace.items():
        ax = np.abs(x.astype(np.float64))
        assert np.isfinite(ax).all() and ((ax == 0) | (ax >= R.TINY)).all(), f"{what}: {k} leaves the normal range"


def test_shared_data_has_its_blocks_and_keeps_every_intermediate_normal():
    for step, s, wd in ADAM_CONFIGS:
        p, g, m, v = R.make_data(N, 3, wd, s)
        b = N // 16
        assert (g[:b] == 0).all() and (m[b:2 * b] == 0).all() and (v[b:2 * b] == 0).all()
        assert (np.abs(p) >= 1e-3 * (1 - 1e-6)).all() and (np.abs(p) <= 10).all() and (v >= 0).all()
        tr = {}
        _, _, v1 = adam32(p, g, m, v, LR, B1, B2, EPS, wd, step, s, trace=tr)
        _normal(tr, f"Adam step {step} scale {s} wd {wd}")
        share = R.small_denominator_share(R.adam64(p, g, m, v, LR, B1, B2, EPS, wd, step, s)[2], B2, step, EPS)
        assert share >= 0.03, f"step {step} scale {s} wd {wd}: eps decides only {share:.3%} of the elements"
        if wd:    # the cancellation block: g' is at most 1 % of either term
            gs, wp = g[2 * b:3 * b].astype(np.float64) * s, R.f32(wd) * p[2 * b:3 * b].astype(np.float64)
            assert (np.abs(gs + wp) <= 1.01e-2 * np.abs(wp)).all()
    for nesterov, mu, wd, s in SGD_CONFIGS:
        p, g, m, _ = R.make_data(N, 3, wd, s)
        tr = {}
        sgd32(p, g, m, LR, mu, wd, nesterov, s, trace=tr)
        _normal(tr, f"SGD nesterov {nesterov} mu {mu}")


# ------------------------------------------------------------------ 2. correct float32 implementations pass
@pytest.mark.parametrize("step,s,wd", ADAM_CONFIGS)
def test_float32_adam_stays_inside_the_bounds(step, s, wd, record_property):
    p, g, m, v = R.make_data(N, 3, wd, s)
    a = (LR, B1, B2, EPS, wd, step, s)
    ref, bounds = R.adam64(p, g, m, v, *a), R.adam_bounds(p, g, m, v, *a)
    for name, got in (("torch", torch_adam(p, g, m, v, *a, torch.float32)), ("chain", adam32(p, g, m, v, *a))):
        for out, x, r64, e in zip(("p", "m", "v"), got, ref, bounds):
            r = R.worst_ratio(x, r64, e)
            record_property(f"{name}_{out}", r)
            assert r <= 1.0, f"float32 {name} {out}: {r:.3g} x its bound"


@pytest.mark.parametrize("nesterov,mu,wd,s", SGD_CONFIGS)
def test_float32_sgd_stays_inside_the_bounds(nesterov, mu, wd, s, record_property):
    p, g, buf, _ = R.make_data(N, 3, wd, s)
    a = (LR, mu, wd, nesterov, s)
    ref, bounds = R.sgd64(p, g, buf, *a), R.sgd_bounds(p, g, buf, *a)
    for name, got in (("torch", torch_sgd(p, g, buf, *a, torch.float32)), ("chain", sgd32(p, g, buf, *a))):
        for out, x, r64, e in zip(("p", "buf"), got, ref, bounds):
            if name == "torch" and mu == 0 and out == "buf":
                continue   # torch keeps no buffer without momentum
            r = R.worst_ratio(x, r64, e)
            record_property(f"{name}_{out}", r)
            assert r <= 1.0, f"float32 {name} {out}: {r:.3g} x its bound"


def test_unfused_chain_is_within_twice_the_rms_distance_of_float32_torch():
    """the bar of the model-layout GPU test, on the host: error / bound in the root mean square, an unfused float32 chain
    (one rounding per operation, as the kernels are built) against float32 torch.optim (whose CPU kernels fuse
    multiply-adds), on a first step (m = v = buf = 0, where the difference is largest) and a later one"""
    wd, s = 1e-4, 1.0
    p, g, m, v = R.make_data(N, 3, wd, s)
    for first in (True, False):
        m0, v0 = (np.zeros_like(m), np.zeros_like(v)) if first else (m, v)
        a = (LR, B1, B2, EPS, wd, 1 if first else 2, s)
        ref, bounds = R.adam64(p, g, m0, v0, *a), R.adam_bounds(p, g, m0, v0, *a)
        for x, y, r64, e in zip(adam32(p, g, m0, v0, *a), torch_adam(p, g, m0, v0, *a, torch.float32), ref, bounds):
            assert R.rms_ratio(x, r64, e) <= 2 * R.rms_ratio(y, r64, e)
        a = (LR, MU, wd, 1, s)
        ref, bounds = R.sgd64(p, g, m0, *a), R.sgd_bounds(p, g, m0, *a)
        for x, y, r64, e in zip(sgd32(p, g, m0, *a), torch_sgd(p, g, m0, *a, torch.float32), ref, bounds):
            assert R.rms_ratio(x, r64, e) <= 2 * R.rms_ratio(y, r64, e)


# ------------------------------------------------------------------ 3. wrong implementations fail
def _outside(got, ref, bounds):
    bad = np.zeros(ref[0].shape, dtype=bool)
    for x, r64, e in zip(got, ref, bounds):
        bad |= ~(np.abs(x.astype(np.float64) - r64) <= e)
    return float(bad.mean())


@pytest.mark.parametrize("variant", ["eps_in_sqrt", "adamw", "no_bias_correction", "beta_pow_step_minus_1",
                                     "grad_scale_dropped", "sqrt_v_over_bc2"])
def test_wrong_adam_leaves_the_bounds(variant, record_property):
    wd, s, step = 1e-4, 0.25, 7
    p, g, m, v = R.make_data(N, 3, wd, s)
    a = (LR, B1, B2, EPS, wd, step, s)
    ref, bounds = R.adam64(p, g, m, v, *a), R.adam_bounds(p, g, m, v, *a)
    assert _outside(adam32(p, g, m, v, *a), ref, bounds) == 0.0
    share = _outside(adam32(p, g, m, v, *a, variant=variant), ref, bounds)
    record_property("outside_share", share)
    assert share >= 0.01, f"{variant} stays inside the bounds on all but {share:.3%} of the elements"


@pytest.mark.parametrize("variant", ["nesterov_ignored", "decay_after_momentum", "dampened"])
def test_wrong_sgd_leaves_the_bounds(variant, record_property):
    wd, s = 1e-4, 0.25
    p, g, buf, _ = R.make_data(N, 3, wd, s)
    a = (LR, MU, wd, 1, s)
    ref, bounds = R.sgd64(p, g, buf, *a), R.sgd_bounds(p, g, buf, *a)
    assert _outside(sgd32(p, g, buf, *a), ref, bounds) == 0.0
    share = _outside(sgd32(p, g, buf, *a, variant=variant), ref, bounds)
    record_property("outside_share", share)
    assert share >= 0.01, f"{variant} stays inside the bounds on all but {share:.3%} of the elements"


def test_transpose64():
    w = np.arange(2 * 3 * 5, dtype=np.float32).reshape(2, 3, 5)
    t = R.transpose64(w)
    assert t.shape == (2, 5, 3) and all(t[k, j, i] == w[k, i, j] for k in range(2) for i in range(3) for j in range(5))
    assert torch.equal(R.transpose64(torch.from_numpy(w)), torch.from_numpy(np.ascontiguousarray(t)))
