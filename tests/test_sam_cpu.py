"""Sharpness-aware minimisation and gradient clipping without a GPU: the numpy restatements (tests/sam_ref.py) against
the usual torch code on the CPU within bounds derived from the arithmetic, the argument checks of optim.SAM, of
build_step and of the command line, the refusal of data-parallel runs, and the three entry points of the library."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import sam_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(27, 8, 16), (16,), (1, 16), (33, 7), (5,), (64, 32)]     # 3 + 1 tensors get a gradient, one gets none


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _tensors(seed, no_grad=(4,)):
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=g) * 0.2 for s in SHAPES]
    grads = [None if i in no_grad else torch.randn(s, generator=g) * 3.0 for i, s in enumerate(SHAPES)]
    return params, grads


def _flat(params, grads):
    """what FlatParams holds: every parameter, and zeros where a parameter has no gradient"""
    w = np.concatenate([p.reshape(-1).numpy() for p in params])
    g = np.concatenate([(torch.zeros_like(p) if q is None else q).reshape(-1).numpy() for p, q in zip(params, grads)])
    return w.copy(), g.copy()


# ------------------------------------------------------------------ 1. the restatements against torch
def test_squared_norm_restatement():
    rng = np.random.default_rng(0)
    g = (rng.standard_normal(4099) * 2).astype(np.float32)
    w = rng.standard_normal(4099).astype(np.float32)
    exact = sum(float(x) ** 2 for x in g.astype(np.float64))      # python doubles, in index order
    assert abs(R.sqnorm64(g) - exact) <= R.sqnorm_bound(g.size) * exact
    t = (np.abs(w) * g).astype(np.float32).astype(np.float64)
    assert abs(R.sqnorm64(g, w) - float(np.sum(t * t))) <= R.sqnorm_bound(g.size) * float(np.sum(t * t))
    assert R.sqnorm64(np.zeros(0, np.float32)) == 0.0
    assert R.sqnorm64(np.float32([3e-20, -4e-20])) == pytest.approx(25e-40, rel=1e-6)   # no float32 underflow
    assert R.sqnorm64(np.float32([3e15, -4e15])) == pytest.approx(25e30, rel=1e-6)      # ... nor overflow


@pytest.mark.parametrize("max_norm", [0.5, 7.0, 1e4])
def test_clip_restatement_against_torch_clip_grad_norm(max_norm):
    """torch takes the norm in float32 and divides in float32; the restatement takes both in float64 and rounds the
    coefficient once.  So the coefficients differ by at most the float32 norm's error (sam_ref.torch_norm_error) plus
    three float32 roundings (torch's + 1e-6, its division, the restatement's cast), and every clipped element by one
    more rounding on each side: |difference| <= |g coef| (e_norm + 5 U32)."""
    params, grads = _tensors(1)
    w, g = _flat(params, grads)
    holders = [torch.nn.Parameter(p.clone()) for p in params]
    for h, q in zip(holders, grads):
        h.grad = None if q is None else q.clone()
    total = torch.nn.utils.clip_grad_norm_(holders, max_norm)
    sq = R.sqnorm64(g)
    e_norm = R.torch_norm_error(g.size)
    assert abs(float(total) - np.sqrt(sq)) <= e_norm * np.sqrt(sq)
    coef = R.clip_coef(sq, max_norm)
    assert (coef < 1) == (max_norm < 1e4)            # both branches of the min are taken over the three cases
    want = R.clip(g, sq, max_norm)
    got = np.concatenate([(torch.zeros_like(h) if h.grad is None else h.grad).reshape(-1).numpy() for h in holders])
    if coef == 1:
        assert np.array_equal(_bits(got), _bits(g)) and np.array_equal(_bits(want), _bits(g))
    else:
        tol = np.abs(want.astype(np.float64)) * (e_norm + 5 * R.U32)
        assert np.all(np.abs(got.astype(np.float64) - want) <= tol)
        assert np.any(got != g)


@pytest.mark.parametrize("adaptive", [False, True])
def test_sam_ascent_restatement_against_the_usual_torch_step(adaptive):
    """sam_ref.torch_sam_ascent is the literal p.add_(e) step.  Its scale carries the float32 norm's error and three
    roundings (+ 1e-12, the division, the restatement's cast); e then takes one rounding per product on each side (one
    plain, three adaptive), so |e - e'| <= |e| (e_norm + 9 U32), and the two sums w + e round once each:
    |difference| <= |e| (e_norm + 9 U32) + 2 U32 |w + e|.  Parameters without a gradient keep their bits."""
    rho = 0.05 if not adaptive else 1.0
    params, grads = _tensors(2)
    w, g = _flat(params, grads)
    moved = [p.clone() for p in params]
    norm = R.torch_sam_ascent(moved, grads, rho, adaptive)
    sq = R.sqnorm64(g, w if adaptive else None)
    e_norm = R.torch_norm_error(g.size)
    assert abs(float(norm) - np.sqrt(sq)) <= e_norm * np.sqrt(sq)
    want = R.perturb(w, g, sq, rho, adaptive)
    got = np.concatenate([p.reshape(-1).numpy() for p in moved])
    e = np.abs(want.astype(np.float64) - w)
    tol = (e + 2 * R.U32 * np.abs(w)) * (e_norm + 9 * R.U32) + 2 * R.U32 * np.abs(want)
    assert np.all(np.abs(got.astype(np.float64) - want) <= tol)
    assert np.any(want != w)
    none = g == 0
    assert none.sum() >= 5 and np.array_equal(_bits(want[none]), _bits(w[none])) and np.array_equal(_bits(got[none]), _bits(w[none]))
    # the length of the step: || e || = rho (plain), to the accuracy of the float32 elements
    if not adaptive:
        assert np.sqrt(np.sum((want.astype(np.float64) - w) ** 2)) == pytest.approx(rho, rel=1e-4)


def test_zero_gradient_elements_keep_a_negative_zero():
    w = np.float32([-0.0, 0.0, 1.5, -2.0])
    g = np.float32([0.0, -0.0, 0.0, 1.0])
    out = R.perturb(w, g, 1.0, 0.05)
    assert np.array_equal(_bits(out[:3]), _bits(w[:3])) and out[3] == np.float32(-2.0) + np.float32(0.05) * np.float32(1.0)
    assert R.sam_coef(0.0, 0.05) == np.float32(np.float64(np.float32(0.05)) / 1e-12)      # a zero gradient: finite


# ------------------------------------------------------------------ 2. argument checks
@pytest.mark.parametrize("rho", [0, 0.0, -0.05, float("nan"), float("inf"), None, "0.05"])
def test_sam_refuses_a_bad_rho(rho):
    from lidog_amd.optim import SAM
    with pytest.raises(ValueError, match="positive and finite"):
        SAM.check_arguments(rho)
    with pytest.raises(ValueError, match="positive and finite"):
        SAM(object(), rho)                              # before the optimiser is looked at


def test_argument_checks_of_the_entry_points():
    from lidog_amd.optim import check_sam_arguments
    check_sam_arguments()
    check_sam_arguments(0.05, True, 1.0)
    check_sam_arguments(None, False, 2)
    with pytest.raises(ValueError, match="sam_adaptive goes with sam_rho"):
        check_sam_arguments(None, True)
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="grad_clip_norm"):
            check_sam_arguments(grad_clip_norm=bad)
    from lidog_amd.train import build_step
    with pytest.raises(ValueError, match="positive and finite"):       # before the model is touched
        build_step(None, "MinkUNet34", sam_rho=0.0)
    with pytest.raises(ValueError, match="grad_clip_norm"):
        build_step(None, "MinkUNet34", grad_clip_norm=0.0)
    with pytest.raises(ValueError, match="sam_adaptive"):
        build_step(None, "MinkUNet34", sam_adaptive=True)


@pytest.mark.parametrize("argv, message", [
    (["--sam-rho", "0"], "positive and finite"), (["--sam-rho", "-0.05"], "positive and finite"),
    (["--sam-rho", "nan"], "positive and finite"), (["--sam-adaptive"], "sam_adaptive goes with sam_rho"),
    (["--grad-clip-norm", "0"], "grad_clip_norm"), (["--sam-rho", "0.05", "--grad-clip-norm", "-1"], "grad_clip_norm")])
def test_train_command_line_errors(argv, message, capsys):
    from lidog_amd.train import parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_train_command_line_values():
    from lidog_amd.train import parse_args, sam_of
    assert sam_of(parse_args([])) == dict(sam_rho=None, sam_adaptive=False, grad_clip_norm=None)
    a = parse_args(["--sam-rho", "0.5", "--sam-adaptive", "--grad-clip-norm", "1.0", "--precision", "bf16"])
    assert sam_of(a) == dict(sam_rho=0.5, sam_adaptive=True, grad_clip_norm=1.0)
    assert sam_of(parse_args(["--grad-clip-norm", "35"])) == dict(sam_rho=None, sam_adaptive=False, grad_clip_norm=35.0)


def test_both_features_refuse_more_than_one_rank(monkeypatch):
    """a faked world size: every way in raises before anything is built or launched"""
    import torch.distributed as dist
    from lidog_amd import optim
    from lidog_amd.train import Fit, build_step
    from lidog_amd.trainer import SourceStep
    model = torch.nn.Linear(3, 2)
    opt = optim.FlatAdam(model, lr=1e-3)                # one rank: built before the world grows
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    for attempt in (lambda: optim.SAM(opt, 0.05), lambda: opt.clip_grad_norm(1.0), opt.grad_norm,
                    lambda: SourceStep(model, opt, grad_clip_norm=1.0),
                    lambda: SourceStep(model, opt, sam=object()),
                    lambda: build_step(model, "MinkUNet34", sam_rho=0.05),
                    lambda: build_step(model, "MinkUNet34", grad_clip_norm=1.0),
                    lambda: Fit("MinkUNet34", sam_rho=0.05), lambda: Fit("MinkUNet34", grad_clip_norm=1.0)):
        with pytest.raises(NotImplementedError, match="2 ranks"):
            attempt()


# ------------------------------------------------------------------ 3. the library
def test_entry_points_are_declared_exported_and_typed():
    from lidog_amd import _lib, optim
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    S, p, i32, i64, f = _lib.SIGNATURES, _lib._p, _lib._i32, _lib._i64, _lib._f
    assert S["lidog_flat_sqnorm"] == [p, p, i64, i32, p, p, p]
    assert S["lidog_flat_sqnorm_ws"] == [i64] and _lib._RESTYPES["lidog_flat_sqnorm_ws"] is i64
    assert S["lidog_sam_perturb"] == [p, p, p, i64, p, f, i32, p]
    assert S["lidog_flat_clip"] == [p, i64, p, f, f, p]
    assert re.search(r"^#define LIDOG_SQNORM_PLAIN 0\b", header, re.M)
    assert re.search(r"^#define LIDOG_SQNORM_ADAPTIVE 1\b", header, re.M)
    assert re.search(rf"^#define LIDOG_FLAT_MAX_BLOCKS {R.MAX_BLOCKS}\b", header, re.M)
    assert (optim.SQNORM_PLAIN, optim.SQNORM_ADAPTIVE, optim.FLAT_MAX_BLOCKS) == (0, 1, R.MAX_BLOCKS)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True)
    names = set(re.findall(r"\bT (lidog_[a-z0-9_]+)", exported.stdout))
    assert {"lidog_flat_sqnorm", "lidog_flat_sqnorm_ws", "lidog_sam_perturb", "lidog_flat_clip"} <= names
    assert "sam.hip" in __import__("lidog_amd.build", fromlist=["SOURCES"]).SOURCES
    assert _lib.ABI_VERSION == 9                                 # additive entries: the version stays


def test_workspace_size_and_checks_before_any_launch():
    import ctypes
    from lidog_amd import _lib
    L = _lib.load()
    for n, blocks in ((0, 1), (1, 1), (1024, 1), (1025, 2), (R.SWEEP, R.MAX_BLOCKS), (R.SWEEP + 1, R.MAX_BLOCKS),
                      (2 ** 33, R.MAX_BLOCKS)):
        assert L.lidog_flat_sqnorm_ws(n) == 8 * blocks, n
    one = ctypes.c_void_p(64)                # never dereferenced: every call below returns from its checks
    assert L.lidog_sam_perturb(one, one, one, 0, one, 0.05, 0, None) == 0
    assert L.lidog_flat_clip(one, 0, one, 1.0, 1.0, None) == 0
    for args in ((one, one, one, -1, one, 0.05, 0), (one, one, one, 4, one, 0.0, 0), (one, one, one, 4, one, float("nan"), 0),
                 (one, one, one, 4, one, float("inf"), 0), (None, one, one, 4, one, 0.05, 0),
                 (one, one, one, 4, None, 0.05, 0), (ctypes.c_void_p(64), ctypes.c_void_p(72), ctypes.c_void_p(4096), 4, one, 0.05, 1)):
        assert L.lidog_sam_perturb(*args, None) == 2, args
        assert b"sam_perturb" in L.lidog_last_error()
    for args in ((one, -1, one, 1.0, 1.0), (one, 4, one, 0.0, 1.0), (one, 4, one, float("nan"), 1.0),
                 (one, 4, one, 1.0, 0.0), (None, 4, one, 1.0, 1.0), (one, 4, None, 1.0, 1.0)):
        assert L.lidog_flat_clip(*args, None) == 2, args
        assert b"flat_clip" in L.lidog_last_error()
    for args in ((one, None, -1, 0, one, one), (one, None, 4, 2, one, one), (one, None, 4, 1, one, one),
                 (None, None, 4, 0, one, one), (one, None, 4, 0, None, one), (one, None, 4, 0, one, None)):
        assert L.lidog_flat_sqnorm(*args, None) == 2, args
        assert b"flat_sqnorm" in L.lidog_last_error()
