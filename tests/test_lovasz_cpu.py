"""The Lovasz-softmax auxiliary criterion without a GPU: the numpy yardstick (tests/lovasz_ref.py) against an independent
float64 torch-autograd restatement of the published algorithm, the bound the GPU tests hold the loss to, the new entry
points of the cross-compiled library and their argument checks, make_aux_criterion, build_step and the command line."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import lovasz_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["lidog_lovasz_ws", "lidog_lovasz_fwd", "lidog_lovasz_bwd"]


def case(n, C, seed, scale=1.0, lo=-1):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, C)) * scale).astype(np.float32)
    y = rng.integers(lo, C, size=n)
    return x, y


# ------------------------------------------------------------------ 1. the yardstick
def published(logits, labels, ignore):
    """lovasz_softmax_flat(classes='present') of Berman et al.'s code on float64 CPU tensors, the ignored rows filtered
    first as flatten_probas does; (loss, d loss / d logits) by autograd"""
    x = torch.from_numpy(np.asarray(logits, dtype=np.float64)).requires_grad_(True)
    t = torch.from_numpy(np.asarray(labels)).long()
    C = x.shape[1]
    keep = (t >= 0) & (t < C)
    if ignore is not None:
        keep &= t != ignore
    probas, lab = torch.softmax(x, 1)[keep], t[keep]
    losses = []
    for c in range(C):
        fg = (lab == c).double()
        if fg.sum() == 0:
            continue
        errors = (fg - probas[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
        gt_sorted = fg[perm]
        gts = gt_sorted.sum()
        intersection = gts - gt_sorted.cumsum(0)
        union = gts + (1 - gt_sorted).cumsum(0)
        jaccard = 1.0 - intersection / union
        if len(gt_sorted) > 1:
            jaccard = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
        losses.append(torch.dot(errors_sorted, jaccard.detach()))
    if not losses:
        return 0.0, np.zeros(x.shape)
    loss = torch.stack(losses).mean()
    return float(loss.detach()), torch.autograd.grad(loss, x)[0].numpy()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_yardstick_equals_the_published_algorithm(n):
    for seed, scale in ((0, 1.0), (1, 3.0)):
        x, y = case(n, 7, seed + 10 * n, scale)
        r = R.full64(x, y, -1, gout=1.0)
        loss, grad = published(x, y, -1)
        assert abs(r["loss"] - loss) <= 1e-12
        assert np.abs(r["grad"] - grad).max() <= 1e-12
        assert (r["grad"][~r["valid"]] == 0).all()


def test_yardstick_special_cases():
    x, y = case(65, 7, 3)
    r = R.full64(x, np.full(65, -1), -1)                    # every row ignored
    assert r["loss"] == 0 and r["P"] == 0 and (r["grad"] == 0).all()
    y2 = y.copy()
    y2[:5] = (9, 7, -3, 100, -1)                            # outside [0, C): as ignored
    y3 = np.where((y2 < 0) | (y2 >= 7), -1, y2)
    a, b = R.full64(x, y2, -1), R.full64(x, y3, -1)
    assert a["loss"] == b["loss"] and np.array_equal(a["grad"], b["grad"]) and (a["grad"][:5] == 0).all()
    one = R.full64(x, np.full(65, 4), None)                 # one class present, no ignore label
    assert one["P"] == 1 and one["present"].tolist() == [c == 4 for c in range(7)]
    loss, grad = published(x, np.full(65, 4), None)
    assert abs(one["loss"] - loss) <= 1e-12 and np.abs(one["grad"] - grad).max() <= 1e-12
    r = R.full64(x, y, 2)                                   # an ignore label inside [0, C)
    loss, grad = published(x, y, 2)
    assert not r["present"][2] and abs(r["loss"] - loss) <= 1e-12 and np.abs(r["grad"] - grad).max() <= 1e-12
    r2 = R.full64(x, y, -1, gout=-2.5)
    assert np.abs(r2["grad"] + 2.5 * R.full64(x, y, -1)["grad"]).max() <= 1e-15


def test_ties_go_by_row_and_saturated_rows_have_no_sign():
    x = np.zeros((6, 3), dtype=np.float32)
    x[:, 0] = -1.0                                          # six identical rows, p = (0.16, 0.42, 0.42)
    y = np.array([0, 1, 0, 2, 1, 0])
    r = R.from_errors(R.errors64(x, y, None)[0], y, None)
    # class 0: fg rows 0, 2, 5 share the larger error and come first in row order, then rows 1, 3, 4
    g0 = R.lovasz_g(np.array([1, 1, 1, 0, 0, 0]))
    assert np.array_equal(r["g"][[0, 2, 5, 1, 3, 4], 0], g0)
    x = np.zeros((4, 3), dtype=np.float32)
    x[:, 1] = 200.0                                         # float32 softmax: exactly (0, 1, 0)
    y = np.array([1, 0, 1, 2])
    e = np.abs((y[None, :] == np.arange(3)[:, None]).astype(np.float32) - np.array([[0], [1], [0]], dtype=np.float32))
    r = R.from_errors(e, y, None)
    assert (r["coef"][e.T == 0] == 0).all() and not np.signbit(r["coef"][e.T == 0]).any()
    assert (r["coef"][1] == [-r["g"][1, 0].astype(np.float32), r["g"][1, 1].astype(np.float32), 0]).all()


@pytest.mark.parametrize("n,scale", [(65, 1.0), (257, 2.0)])
def test_loss_moves_by_at_most_the_largest_error_bar(n, scale):
    """the Lovasz extension is monotone and 1-Lipschitz in the largest perturbation, however the order changes"""
    x, y = case(n, 7, n)
    e, _, ok = R.errors64(x, y, -1)
    base = R.from_errors(e, y, -1)["loss"]
    bars = R.error_bars(x, y, -1)
    assert (bars[:, ~ok] == 0).all() and (bars[:, ok] > 0).all()
    rng = np.random.default_rng(n)
    for k in (1.0, 1e3, 1e5):                               # 1e5 bars reorder thousands of pairs
        for d in (rng.uniform(-1, 1, e.shape), np.ones(e.shape), -np.ones(e.shape)):
            moved = R.from_errors(e + k * bars * d, y, -1)["loss"]
            assert abs(moved - base) <= k * bars.max() * (1 + 1e-9)
    assert R.from_errors(e + bars, y, -1)["loss"] >= base


def test_end_to_end_precondition_holds_for_the_gpu_cases():
    """test_gpu_lovasz.py (E): sorted float64 errors further apart than four times their first-order bars"""
    import test_gpu_lovasz as G
    for n, seed, scale in G.SEPARATED_CASES:
        x, y = G.separated_case(n, seed, scale)
        assert R.separated(x, y, -1, factor=4.0) > 1.0, (n, seed, scale)


# ------------------------------------------------------------------ 2. the library
def test_new_symbols_are_declared_exported_and_typed():
    from lidog_amd import _lib
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (lidog_[a-z0-9_]+)", exported.stdout))
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in exported, name
        decl = re.search(r"^(?:int|int64_t) " + name + r"\(([^;]*?)\)\s*;", header, re.S | re.M).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib.SIGNATURES["lidog_lovasz_ws"] == [ctypes.c_int64, ctypes.c_int32]
    assert _lib._RESTYPES["lidog_lovasz_ws"] is ctypes.c_int64
    assert len(_lib.SIGNATURES["lidog_lovasz_fwd"]) == 11 and len(_lib.SIGNATURES["lidog_lovasz_bwd"]) == 11
    assert _lib.ABI_VERSION == 9 and _lib.load().lidog_abi_version() == 9     # additive entries: the version stays


def test_bad_shapes_return_2_before_any_launch():
    from lidog_amd import _lib
    L = _lib.load()
    one = ctypes.c_void_p(64)        # never dereferenced: every call below returns from its checks
    for n, C in ((5, 1), (5, 21), (-1, 7), (2 ** 31 // 7 + 1, 7), (2 ** 30, 2), (2 ** 40, 7)):
        assert L.lidog_lovasz_ws(n, C) == 0
        assert L.lidog_lovasz_fwd(one, one, n, C, -1, 1, one, one, one, None, None) == 2
        assert b"lovasz" in L.lidog_last_error()
        assert L.lidog_lovasz_bwd(one, one, n, C, -1, 1, one, one, one, one, None) == 2
    assert L.lidog_lovasz_bwd(None, None, 0, 7, -1, 1, None, None, None, None, None) == 0
    a, b = L.lidog_lovasz_ws(1000, 7), L.lidog_lovasz_ws(2000, 7)
    assert 0 < a < b and a % 256 == 0
    assert L.lidog_lovasz_ws(2 ** 31 // 7, 7) > 0 and L.lidog_lovasz_ws(0, 7) > 0


# ------------------------------------------------------------------ 3. the criterion by name, the steps, the command line
def test_make_aux_criterion():
    from lidog_amd import losses as L
    import lidog_amd
    assert L.AUX_CRITERIA == ("LovaszSoftmaxLoss",)
    c = L.make_aux_criterion("LovaszSoftmaxLoss", 255)
    assert type(c) is L.LovaszSoftmaxLoss and c.ignore_label == 255
    assert L.make_aux_criterion("LovaszSoftmaxLoss").ignore_label == -1 and L.LovaszSoftmaxLoss().ignore_label is None
    for name in ("CELoss", "LovaszHingeLoss", "lovaszsoftmaxloss", None):
        with pytest.raises(NotImplementedError):
            L.make_aux_criterion(name, -1)
    for name in ("LovaszSoftmaxLoss", "make_aux_criterion"):
        assert getattr(lidog_amd, name) is getattr(L, name)
    assert "LovaszSoftmaxLoss" not in L.POINT_CRITERIA and "LovaszSoftmaxLoss" not in L.BEV_CRITERIA


def test_module_raises_on_cpu_tensors_and_bad_shapes():
    from lidog_amd.losses import LovaszSoftmaxLoss
    crit = LovaszSoftmaxLoss(ignore_label=-1)
    with pytest.raises(RuntimeError, match="GPU"):
        crit(torch.randn(8, 7), torch.zeros(8, dtype=torch.long))
    with pytest.raises(RuntimeError, match="GPU"):
        crit(torch.randn(8, 7), torch.zeros(8, dtype=torch.int32))


@pytest.mark.parametrize("kind", ["MinkUNet34BEV", "MinkUNet34", "MinkUNet34Robust"])
def test_build_step_with_and_without_the_auxiliary_criterion(kind):
    from lidog_amd import losses as L
    from lidog_amd.train import build_model, build_step
    _, step, _ = build_step(build_model(kind, device="cpu"), kind)
    assert step.sem_aux_criterion is None and type(step.sem_criterion) is L.SoftDICELoss
    _, step, _ = build_step(build_model(kind, device="cpu"), kind, sem_criterion="CELoss", ignore_label=3,
                            sem_aux_criterion="LovaszSoftmaxLoss", sem_aux_weight=0.5, num_sources=2)
    assert type(step.sem_aux_criterion) is L.LovaszSoftmaxLoss and step.sem_aux_criterion.ignore_label == 3
    assert step.sem_aux_weight == 0.5 and type(step.sem_criterion) is L.CELoss and step.num_sources == 2
    _, step, _ = build_step(build_model(kind, device="cpu"), kind, sem_aux_criterion="LovaszSoftmaxLoss")
    assert step.sem_aux_weight == 1.0 and step.sem_aux_criterion.ignore_label == -1
    with pytest.raises(NotImplementedError):
        build_step(build_model(kind, device="cpu"), kind, sem_aux_criterion="CELoss")
    with pytest.raises(ValueError, match="sem_aux_weight"):
        build_step(build_model(kind, device="cpu"), kind, sem_aux_criterion="LovaszSoftmaxLoss", sem_aux_weight=0.0)


def test_step_classes_take_the_arguments_by_keyword_at_the_end():
    import inspect
    from lidog_amd import trainer as T
    from lidog_amd.train import Fit, build_step
    for cls in (T._Step, T.LiDOGStep, T.SourceStep, T.RobustStep):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert [p.name for p in params[-2:]] == ["sem_aux_criterion", "sem_aux_weight"]
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params[-2:])
        assert (params[-2].default, params[-1].default) == (None, 1.0)
    for fn in (Fit.__init__, build_step):
        params = inspect.signature(fn).parameters
        assert params["sem_aux_criterion"].default is None and params["sem_aux_weight"].default == 1.0


def test_cli_parsing_and_its_errors(capsys):
    from lidog_amd.train import parse_args, sem_aux_of
    a = parse_args([])          # the flags leave no attribute unless they are given, like the other late additions
    assert not hasattr(a, "sem_aux_criterion") and not hasattr(a, "sem_aux_weight") and sem_aux_of(a) == (None, 1.0)
    a = parse_args(["--sem-aux-criterion", "LovaszSoftmaxLoss"])
    assert sem_aux_of(a) == ("LovaszSoftmaxLoss", 1.0) and not hasattr(a, "sem_aux_weight")
    for model in ("MinkUNet34BEV", "MinkUNet34", "MinkUNet34IBN", "MinkUNet34Robust"):
        a = parse_args(["--model", model, "--sem-criterion", "CELoss", "--sem-aux-criterion", "LovaszSoftmaxLoss",
                        "--sem-aux-weight", "0.25", "--precision", "bf16"])
        assert sem_aux_of(a) == ("LovaszSoftmaxLoss", 0.25) and a.sem_criterion == "CELoss"
    with pytest.raises(SystemExit):
        parse_args(["--sem-aux-weight", "0.5"])
    assert "--sem-aux-criterion" in capsys.readouterr().err
    for w in ("0", "-1", "nan"):
        with pytest.raises(SystemExit):
            parse_args(["--sem-aux-criterion", "LovaszSoftmaxLoss", "--sem-aux-weight", w])
        assert "--sem-aux-weight" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(["--sem-aux-criterion", "CELoss"])
