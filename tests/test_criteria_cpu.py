"""The training criteria by name, without a GPU: the float64 yardstick (tests/ce_ref.py) against the reference's own
losses (tests/golden/g18_criteria.npz), make_criterion / make_bev_criterion, the command line, the new entry points of
the cross-compiled library and their argument checks, and the defaults of build_step."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ce_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["lidog_ce_ws", "lidog_ce_fwd", "lidog_ce_bwd", "lidog_dice_kitti_fwd", "lidog_dice_kitti_bwd"]


@pytest.fixture(scope="module")
def golden():
    return np.load(R.G18)


# ------------------------------------------------------------------ 1. the yardstick against the reference's own run
@pytest.mark.parametrize("C", R.GOLDEN_CLASSES)
def test_golden_inputs_are_the_shared_cases(golden, C):
    x, y, w = R.golden_case(C)
    assert np.array_equal(golden[f"c{C}/logits"], x.numpy()) and np.array_equal(golden[f"c{C}/labels"], y.numpy())
    assert np.array_equal(golden[f"c{C}/weights"], w.numpy())
    labels = set(y.tolist())
    assert {1, 6, -1} <= labels and set(range(C)) <= labels
    assert os.path.getsize(R.G18) < 100_000


@pytest.mark.parametrize("C", R.GOLDEN_CLASSES)
@pytest.mark.parametrize("name", ["ce", "wce", "focal"])
def test_ce_ref_matches_the_reference(golden, C, name):
    """the reference ran in fp32: it may be off by reference_bound (its own rounding), nothing more"""
    x, y, w = R.golden_case(C)
    r = R.ce64(x, y, weight=w if name == "wce" else None, ignore=-1, focal=(0.25, 2) if name == "focal" else None)
    loss, grad = float(golden[f"c{C}/{name}/loss"]), torch.from_numpy(golden[f"c{C}/{name}/grad"]).double()
    n = int(r.scored.sum())
    assert abs(loss - float(r.loss)) <= R.reference_bound(n, r.M, C, abs(r.dl) * r.ce + abs(float(r.loss)))
    assert float((grad - r.grad).abs().max()) <= R.reference_bound(n, r.M, C, float(r.grad.abs().max()))
    assert bool((grad[y == -1] == 0).all()) and bool((r.grad[y == -1] == 0).all())


@pytest.mark.parametrize("C", R.GOLDEN_CLASSES)
def test_kitti_dice_ref_matches_the_reference(golden, C):
    x, y, _ = R.golden_case(C)
    r = R.kitti_dice64(x, y, ignore=-1)
    loss, grad = float(golden[f"c{C}/kitti/loss"]), torch.from_numpy(golden[f"c{C}/kitti/grad"]).double()
    n = int((y != -1).sum())
    assert abs(loss - float(r.loss)) <= R.reference_bound(n, r.M, C, 1.0)
    assert float((grad - r.grad).abs().max()) <= R.reference_bound(n, r.M, C, float(r.grad.abs().max()))
    plain = R.D.dice64(x, y, -1)          # the pairing changes the result: rows labelled 1 or 6 exist
    assert abs(float(plain.loss) - float(r.loss)) > 1e-4
    nopair = torch.where((y == 1) | (y == 6), torch.full_like(y, 2), y)
    assert float(R.kitti_dice64(x, nopair, ignore=-1).loss) == float(R.D.dice64(x, nopair, -1).loss)


def test_ce_ref_degenerate_inputs_are_what_torch_gives():
    """every row ignored: NaN loss, zero gradient; zero total weight: NaN both; gamma 0 is plain alpha * ce; an
    out-of-range label takes no part"""
    x, y, _ = R.golden_case(7)
    r = R.degenerate(x, torch.full_like(y, -1), ignore=-1)
    assert math.isnan(float(r.loss)) and bool((r.grad == 0).all())
    w = torch.zeros(7)
    r = R.degenerate(x, y, weight=w, ignore=-1)
    assert math.isnan(float(r.loss)) and bool(torch.isnan(r.grad[y != -1]).all()) and bool((r.grad[y == -1] == 0).all())
    a = R.ce64(x, y, ignore=-1)
    f0 = R.ce64(x, y, ignore=-1, focal=(0.5, 0))
    assert float(f0.loss) == 0.5 * float(a.loss) and torch.equal(f0.grad, 0.5 * a.grad) and f0.dl == 0.5 and f0.d2l == 0
    one = torch.zeros(1, 7)
    one[0, 3] = 800.0                       # ce == 0 exactly: (1 - pt) == 0, the focal gradient vanishes
    z = R.degenerate(one, torch.tensor([3]), focal=(1, 1.5))
    assert float(z.loss) == 0 and bool((z.grad == 0).all())
    y2 = y.clone()
    y2[5] = 10
    b = R.ce64(x, y2, ignore=-1)
    y3 = y.clone()
    y3[5] = -1
    assert float(b.loss) == float(R.ce64(x, y3, ignore=-1).loss) and bool((b.grad[5] == 0).all())
    assert not bool(b.scored[5]) and bool((R.grad_bound(b, x, y2)[5] == 0).all())


# ------------------------------------------------------------------ 2. the criteria by name
def test_make_criterion_every_name():
    from lidog_amd import losses as L
    import lidog_amd
    c = L.make_criterion("CELoss", -1, 7)
    assert type(c) is L.CELoss and c.ignore_label == -1 and c.weight is None
    c = L.make_criterion("DICELoss", -1, 7)
    assert type(c) is L.DICELoss and c.ignore_label == -1 and not c.powerize and not c.use_tmask
    c = L.make_criterion("SoftDICELoss", -1, 7)
    assert type(c) is L.SoftDICELoss and c.ignore_label == -1 and not c.is_kitti and c.eps == 0.05
    assert L.make_criterion("SoftDICELoss", -1, 19).is_kitti and not L.make_criterion("SoftDICELoss", -1, 20).is_kitti
    c = L.make_criterion("FocalLoss", 255, 7)
    assert type(c) is L.FocalLoss and (c.alpha, c.gamma) == (0.25, 2) and c.ignore_label == -1     # its own default
    assert (L.FocalLoss().alpha, L.FocalLoss().gamma, L.FocalLoss().ignore_index) == (0.5, 2, -1)
    for name in ("SoftCELoss", "SoftLabelDICELoss", "KLDivLoss", "celoss", None):
        with pytest.raises(NotImplementedError):
            L.make_criterion(name, -1, 7)
    assert type(L.make_bev_criterion("DICELoss", -1)) is L.DICELoss
    b = L.make_bev_criterion("SoftDICELoss", -1)
    assert type(b) is L.SoftDICELoss and not b.is_kitti
    assert type(L.make_bev_criterion("CELoss", -1)) is L.CELoss
    for name in ("FocalLoss", "SoftCELoss", "SoftLabelDICELoss"):
        with pytest.raises(NotImplementedError):
            L.make_bev_criterion(name, -1)
    assert set(L.POINT_CRITERIA) == {"CELoss", "DICELoss", "SoftDICELoss", "FocalLoss"}
    assert set(L.BEV_CRITERIA) == {"DICELoss", "SoftDICELoss", "CELoss"}
    for name in ("CELoss", "FocalLoss", "make_criterion", "make_bev_criterion"):
        assert getattr(lidog_amd, name) is getattr(L, name)


def test_weights_are_taken_from_numpy_or_tensor():
    from lidog_amd.losses import CELoss, FocalLoss
    w = np.linspace(0.5, 2.0, 7)
    a, b = CELoss(ignore_label=-1, weight=w), FocalLoss(weight=torch.from_numpy(w))
    for m in (a, b):
        assert m.weight.dtype == torch.float32 and m.weight.shape == (7,)
        assert np.array_equal(m.weight.cpu().numpy(), w.astype(np.float32))
        assert "weight" not in m.state_dict()
    with pytest.raises(ValueError):
        CELoss(weight=np.ones((2, 7)))


def test_modules_raise_on_cpu_tensors():
    from lidog_amd.losses import CELoss, FocalLoss, SoftDICELoss
    x, y = torch.randn(8, 7), torch.zeros(8, dtype=torch.long)
    for crit in (CELoss(ignore_label=-1), FocalLoss(), SoftDICELoss(ignore_label=-1, is_kitti=True)):
        with pytest.raises(RuntimeError, match="GPU"):
            crit(x, y)
    with pytest.raises(RuntimeError, match="GPU"):
        SoftDICELoss(ignore_label=-1)(x, y, is_kitti=True)


# ------------------------------------------------------------------ 3. the command line and the step's defaults
def test_cli_parsing_and_defaults():
    from lidog_amd.train import parse_args, sem_bev_criterion_of as bev_of, sem_criterion_of as sem_of
    a = parse_args([])          # the flags leave no attribute unless they are given, like the other late additions
    assert a.model == "MinkUNet34BEV" and not hasattr(a, "sem_criterion") and not hasattr(a, "sem_bev_criterion")
    assert sem_of(a) == "SoftDICELoss" and bev_of(a) == "DICELoss"
    a = parse_args(["--sem-criterion", "CELoss", "--sem-bev-criterion", "CELoss"])
    assert sem_of(a) == "CELoss" and bev_of(a) == "CELoss"
    for name in ("CELoss", "DICELoss", "SoftDICELoss", "FocalLoss"):
        a = parse_args(["--model", "MinkUNet34", "--sem-criterion", name])
        assert sem_of(a) == name and bev_of(a) is None
    for name in ("DICELoss", "SoftDICELoss", "CELoss"):
        assert bev_of(parse_args(["--sem-bev-criterion", name])) == name
    for bad in (["--sem-criterion", "KLDivLoss"], ["--sem-bev-criterion", "FocalLoss"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


@pytest.mark.parametrize("kind", ["MinkUNet34", "MinkUNet34IBN", "MinkUNet34Robust"])
def test_bev_criterion_is_refused_without_the_bev_head(kind, capsys):
    from lidog_amd.train import build_step, parse_args
    with pytest.raises(SystemExit):
        parse_args(["--model", kind, "--sem-bev-criterion", "DICELoss"])
    assert "--sem-bev-criterion" in capsys.readouterr().err
    with pytest.raises(ValueError, match="BEV"):
        build_step(torch.nn.Linear(2, 2), kind, sem_bev_criterion="CELoss")


def test_build_step_defaults_and_names():
    from lidog_amd import losses as L
    from lidog_amd.train import build_model, build_step
    _, step, _ = build_step(build_model("MinkUNet34BEV", device="cpu"), "MinkUNet34BEV")
    assert type(step.sem_criterion) is L.SoftDICELoss and not step.sem_criterion.is_kitti
    assert type(step.bev_criterion) is L.DICELoss
    assert step.sem_criterion.ignore_label == -1 and step.bev_criterion.ignore_label == -1
    _, step, _ = build_step(build_model("MinkUNet34BEV", device="cpu"), "MinkUNet34BEV", sem_criterion="FocalLoss",
                            sem_bev_criterion="CELoss")
    assert type(step.sem_criterion) is L.FocalLoss and type(step.bev_criterion) is L.CELoss
    for kind in ("MinkUNet34", "MinkUNet34Robust"):
        _, step, _ = build_step(build_model(kind, device="cpu"), kind)
        assert type(step.sem_criterion) is L.SoftDICELoss and not hasattr(step, "bev_criterion")
        _, step, _ = build_step(build_model(kind, device="cpu"), kind, sem_criterion="CELoss", num_sources=2)
        assert type(step.sem_criterion) is L.CELoss and step.num_sources == 2
    with pytest.raises(NotImplementedError):
        build_step(build_model("MinkUNet34", device="cpu"), "MinkUNet34", sem_criterion="SoftCELoss")


# ------------------------------------------------------------------ 4. the library
def test_new_symbols_are_declared_exported_and_typed():
    from lidog_amd import _lib
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (lidog_[a-z0-9_]+)", exported.stdout))
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in exported, name
        decl = re.search(r"^(?:int|int64_t) " + name + r"\(([^;]*?)\)\s*;", header, re.S | re.M).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    assert "C in {2, 7, 8, 16}" not in header
    assert _lib.ABI_VERSION == 9 and _lib.load().lidog_abi_version() == 9     # additive entries: the version stays


def test_bad_shapes_return_2_before_any_launch():
    from lidog_amd import _lib
    L = _lib.load()
    one = ctypes.c_void_p(64)        # never dereferenced: every call below returns from its checks
    assert L.lidog_ce_ws(7) == L.lidog_ce_ws(20) == 2 * 1024
    for n, C in ((5, 1), (5, 21), (-1, 7)):
        assert L.lidog_ce_fwd(one, one, n, C, -1, 1, None, 0, 1.0, 0.0, one, one, one, None) == 2
        assert b"ce: bad shape" in L.lidog_last_error()
        assert L.lidog_ce_bwd(one, one, n, C, -1, 1, None, one, one, one, None) == 2
    assert L.lidog_ce_bwd(None, None, 0, 7, -1, 1, None, None, None, None, None) == 0
    for n, C in ((5, 6), (5, 1), (5, 21), (-1, 19)):
        assert L.lidog_dice_kitti_fwd(one, one, n, C, -1, 1, 0.05, 1, 1, 0.0, one, one, one, None) == 2
        assert L.lidog_dice_kitti_bwd(one, one, n, C, -1, 1, 0.05, 1, one, one, one, None) == 2
    assert b"dice_kitti" in L.lidog_last_error()
    assert L.lidog_dice_kitti_bwd(None, None, 0, 19, -1, 1, 0.05, 1, None, None, None, None) == 0
