"""Sharpness-aware minimisation and gradient clipping inside the training step, on the GPU, on the small scenes and
models of the existing training tests.

The bar is bit equality with a HAND COMPOSITION of the same step: a twin model from the same bytes is driven through
forward_loss / backward / the optimiser's prepare step, its gradient and weights are read back, w + e (or the clipped
gradient) is computed by tests/sam_ref.py FROM THE NORM WORD THE STEP UNDER TEST EXPOSES, written into the flat buffer,
the caches are refreshed, the second pass runs under ME.frozen_running_stats(), the saved weights are written back, and
the optimiser steps.  State dict, optimiser state and the returned loss must then agree bit for bit, after every one of
three steps, and after three further plain steps (the cache rule: transposed kernels, bf16 packs and the executor's
pointers are those of the live weights again).  Run-to-run bit equality of the plain step is asserted elsewhere
(test_gpu_wavg_fit.test_steps_after_applied_match_a_run_that_never_entered_it), so this is a fair demand."""
import math
import re

import numpy as np
import pytest
import torch

import sam_ref as R
from test_gpu_multi_source import _model, two_source_batch

pytestmark = pytest.mark.gpu

NEW_ENTRY_POINTS = ("lidog_flat_sqnorm", "lidog_sam_perturb", "lidog_flat_clip")
_BATCH = {}


def _batch():
    if not _BATCH:
        _BATCH.update(two_source_batch([0, 1], [2, 3]))
    return _BATCH


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and \
        (torch.equal(_bits(a), _bits(b)) if a.dtype == torch.float32 else torch.equal(a, b))


def _assert_same_state(a, b, what):
    assert list(a) == list(b), what
    bad = [k for k in a if not _same_bits(a[k].cpu(), b[k].cpu())]
    assert not bad, f"{what}: {len(bad)} of {len(a)} tensors differ, first {bad[:3]}"


def _assert_same_run(a, b, what):
    """(model, step) pairs: the whole state dict and the optimiser's state"""
    _assert_same_state(a[0].state_dict(), b[0].state_dict(), f"{what}: state_dict")
    sa, sb = a[1].opt.state_dict(), b[1].opt.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        if torch.is_tensor(sa[k]):
            assert _same_bits(sa[k].cpu(), sb[k].cpu()), f"{what}: optimiser state {k}"
        else:
            assert sa[k] == sb[k], f"{what}: optimiser state {k}: {sa[k]} != {sb[k]}"


@pytest.fixture
def launched(monkeypatch):
    """the names of the entry points lidog_amd.optim calls"""
    from lidog_amd import optim
    names, call = [], optim.call
    monkeypatch.setattr(optim, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    return names


@pytest.fixture
def executor(request):
    from lidog_amd import trunk
    prev = trunk.ENABLED
    trunk.set_enabled(request.param)
    yield request.param
    trunk.set_enabled(prev)


def _build(kind, **kw):
    from lidog_amd.train import build_step
    model, step, _ = build_step(_model(kind), kind, lr=1e-2, **kw)
    return model, step


# ------------------------------------------------------------------ the hand composition
def _total(out):
    return out["loss"] if isinstance(out, dict) else out[0]


def _refresh(step):
    step.opt.transposed.refresh()
    if step.bf16 is not None:
        step.bf16.refresh()


def _check_word(word, g, w=None):
    """the norm word of the step under test against the restatement over THIS twin's gradient"""
    ref = R.sqnorm64(g, w)
    assert np.isfinite(ref) and ref > 0
    assert abs(word - ref) <= R.sqnorm_bound(g.size) * ref, (word, ref)


def _hand_step(step, batch, epoch=0, sam=None, clip=None):
    """one training step from its pieces.  `sam`: (squared-norm word, rho, adaptive); `clip`: (word, max_norm)"""
    import lidog_amd.me as ME
    opt, f = step.opt, step.opt.flat
    with step._scope():
        total = _total(step.forward_loss(batch, epoch))
        opt.zero_grad()
        total.backward()
        if sam is not None:
            word, rho, adaptive = sam
            opt._prepare()
            g, w = f.grad.cpu().numpy(), f.flat.cpu().numpy()
            _check_word(word, g, w if adaptive else None)
            f.flat.copy_(torch.from_numpy(R.perturb(w, g, word, rho, adaptive)))
            _refresh(step)
            with ME.frozen_running_stats():
                second = _total(step.forward_loss(batch, epoch))
            opt.zero_grad()
            second.backward()
            f.flat.copy_(torch.from_numpy(w))
            _refresh(step)
        if clip is not None:
            word, max_norm = clip
            opt._prepare()
            g = f.grad.cpu().numpy()
            _check_word(word, g)
            f.grad.copy_(torch.from_numpy(R.clip(g, word, max_norm)))
        opt.step()
        if step.bf16 is not None:
            step.bf16.refresh()
    return total.detach()


def _compare_steps(a, b, steps, what, rho=None, adaptive=False, max_norm=None, epoch=0):
    """`steps` steps of run a (training_step) against run b (by hand), state and loss compared after each"""
    for s in range(steps):
        out = a[1].training_step(_batch(), epoch=epoch)
        sam = (float(a[1].sam.sqnorm), rho, adaptive) if rho is not None else None
        clip = (float(a[1].opt.sqnorm), max_norm) if max_norm is not None else None
        loss = _hand_step(b[1], _batch(), epoch, sam, clip)
        assert torch.equal(_bits(out["loss"]), _bits(loss)), f"{what}: loss of step {s}"
        _assert_same_run(a, b, f"{what}: after step {s}")


# ------------------------------------------------------------------ 1. the SAM step is its hand composition
@pytest.mark.parametrize("precision", [None, "bf16"])
@pytest.mark.parametrize("executor", [True, False], indirect=True, ids=["executor", "operators"])
@pytest.mark.parametrize("optimizer", ["Adam", "SGD"])
@pytest.mark.parametrize("kind", ["MinkUNet34", "MinkUNet34BEV"])
def test_sam_step_equals_its_hand_composition(kind, optimizer, executor, precision, monkeypatch):
    import lidog_amd.me as ME
    rho = 0.05
    a = _build(kind, optimizer=optimizer, precision=precision, sam_rho=rho)
    b = _build(kind, optimizer=optimizer, precision=precision)
    assert a[1].sam is not None and a[1].sam.backup.data_ptr() != a[1].opt.flat.flat.data_ptr() and b[1].sam is None
    _assert_same_run(a, b, "before the first step")
    backup_at = a[1].sam.backup.data_ptr()
    managers, init = [], ME.CoordinateManager.__init__
    monkeypatch.setattr(ME.CoordinateManager, "__init__", lambda self, *x: (managers.append(self), init(self, *x))[1])
    a[1].training_step(_batch())
    monkeypatch.undo()
    assert len(managers) == 1, "the second pass built coordinate maps of its own"
    assert a[1].last_path == "_TrunkFnBackward" if (executor and precision is None) else a[1].last_path != "_TrunkFnBackward"
    loss = _hand_step(b[1], _batch(), 0, (float(a[1].sam.sqnorm), rho, False))
    assert a[1].last_path == b[1].last_path
    assert len(a[1]._last_manager.trace) == len(b[1]._last_manager.trace)       # one pass's trace: the next batch's prefetch
    _assert_same_run(a, b, "after step 0")
    _compare_steps(a, b, 2, "sam", rho=rho)
    assert a[1].sam.backup.data_ptr() == backup_at and not a[1].sam.perturbed     # allocated once
    assert torch.isfinite(loss)
    if optimizer != "Adam":
        return
    # the cache rule (both models, both paths, both precisions, one optimiser): plain steps on both from here
    a[1].sam = None
    for s in range(3):
        outs = [run[1].training_step(_batch()) for run in (a, b)]
        assert torch.equal(_bits(outs[0]["loss"]), _bits(outs[1]["loss"])), f"loss of plain step {s} after SAM"
    _assert_same_run(a, b, "three plain steps after SAM")


@pytest.mark.parametrize("kind, num_sources, adaptive, max_norm", [
    ("MinkUNet34BEV", 2, False, None), ("MinkUNet34", 2, True, None), ("MinkUNet34Robust", 1, False, None),
    ("MinkUNet34Robust", 2, True, 0.05), ("MinkUNet34BEV", 1, True, 0.05)])
def test_every_step_class_both_source_modes_adaptive_and_clipped(kind, num_sources, adaptive, max_norm):
    """the remaining combinations, two steps each: two sources (every parameter used twice per pass), RobustStep, the
    adaptive form, and SAM with clipping -- the clip is of the second pass's gradient"""
    rho = 1.0 if adaptive else 0.05
    kw = dict(num_sources=num_sources)
    a = _build(kind, sam_rho=rho, sam_adaptive=adaptive, grad_clip_norm=max_norm, **kw)
    b = _build(kind, **kw)
    _compare_steps(a, b, 2, f"{kind} x{num_sources}", rho=rho, adaptive=adaptive, max_norm=max_norm)
    if max_norm is not None:
        assert R.clip_coef(float(a[1].opt.sqnorm), max_norm) < 1, "the bound was not below the norm: nothing was clipped"
        assert float(a[1].opt.sqnorm) != float(a[1].sam.sqnorm)


# ------------------------------------------------------------------ 2. running statistics
def _stats(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}


@pytest.mark.parametrize("executor", [True, False], indirect=True, ids=["executor", "operators"])
def test_running_statistics_are_those_of_the_first_pass(executor):
    import lidog_amd.me as ME
    kind = "MinkUNet34BEV"
    a, c = _build(kind, sam_rho=0.05), _build(kind)
    before = _stats(a[0])
    a[1].training_step(_batch())
    c[1].forward_loss(_batch())                                   # one plain training-mode forward from the same state
    sa, sc = _stats(a[0]), _stats(c[0])
    assert list(sa) == list(sc) and len(sa) > 60
    for k in sa:                                                  # values: (1 - 0) r + 0 x may turn a -0.0 into +0.0
        assert torch.equal(sa[k], sc[k]), k
        if "num_batches" in k:
            assert int(sa[k]) == 1, k
    assert any(not torch.equal(sa[k], before[k]) for k in sa if "running_mean" in k)
    # the context alone: a training-mode forward inside it leaves every statistic and counter where it was
    with ME.frozen_running_stats():
        out = c[1].forward_loss(_batch())
    assert (c[1].last_path == "_TrunkFnBackward") == executor and torch.isfinite(out[0])
    after = _stats(c[0])
    for k in sc:
        assert torch.equal(after[k], sc[k]), k
    c[1].forward_loss(_batch())                                   # and outside it the statistics move again
    assert int(_stats(c[0])[next(k for k in sc if "num_batches" in k)]) == 2


# ------------------------------------------------------------------ 3. warm-up: parameters without a gradient
def test_warmup_leaves_the_segmentation_head_alone(monkeypatch):
    model, step = _build("MinkUNet34BEV", warmup_epochs=1, sam_rho=0.05, grad_clip_norm=1e-3)
    final = {k: p for k, p in model.named_parameters() if k.startswith("final.")}
    assert final
    before = {k: p.detach().clone() for k, p in final.items()}
    seen = []
    first = step.sam.first_step
    monkeypatch.setattr(step.sam, "first_step", lambda: (first(), seen.append({k: p.detach().clone() for k, p in final.items()})))
    other = model.conv0p1s1.kernel.detach().clone()
    moved = []
    second = step.sam.second_step
    monkeypatch.setattr(step.sam, "second_step", lambda: (moved.append(not torch.equal(model.conv0p1s1.kernel, other)), second()))
    step.training_step(_batch(), epoch=0)
    assert len(seen) == 1 and moved == [True]                     # the perturbation was in force, and moved the rest
    for k, p in final.items():
        assert torch.equal(_bits(seen[0][k]), _bits(before[k])), f"{k} moved with the perturbation"
        assert torch.equal(_bits(p), _bits(before[k])), f"{k} changed during a warm-up step"
    index = {id(p): i for i, p in enumerate(step.opt.flat.params)}
    assert all(step.opt.param_steps[index[id(p)]] == 0 for p in final.values())
    assert max(step.opt.param_steps) == 1
    step.training_step(_batch(), epoch=1)                         # warm-up over: the head trains
    assert all(step.opt.param_steps[index[id(p)]] == 1 for p in final.values())
    assert not torch.equal(model.final.kernel, before["final.kernel"])


# ------------------------------------------------------------------ 4. clipping
def test_clipping_equals_its_hand_composition_and_a_large_bound_changes_nothing(launched):
    kind = "MinkUNet34BEV"
    probe = _build(kind)
    total = _total(probe[1].forward_loss(_batch()))
    probe[1].opt.zero_grad()
    total.backward()
    norm = probe[1].opt.grad_norm()
    assert norm.dim() == 0 and norm.dtype == torch.float64 and norm.is_cuda
    g = probe[1].opt.flat.grad.cpu().numpy()
    word = float(probe[1].opt.sqnorm)
    _check_word(word, g)
    assert abs(float(norm) - math.sqrt(word)) <= 4 * R.U64 * math.sqrt(word)
    print(f"gradient norm of the first step: {float(norm):.6g} over {g.size} elements")
    max_norm = 0.25 * float(norm)
    a, b = _build(kind, grad_clip_norm=max_norm), _build(kind)
    del launched[:]
    _compare_steps(a, b, 3, "clip", max_norm=max_norm)
    assert launched.count("lidog_flat_clip") == 3 and launched.count("lidog_flat_sqnorm") == 3
    assert "lidog_sam_perturb" not in launched
    # a bound nothing reaches: an unclipped run, bit for bit
    c, d = _build(kind, grad_clip_norm=1e30), _build(kind)
    for s in range(3):
        outs = [run[1].training_step(_batch()) for run in (c, d)]
        assert torch.equal(_bits(outs[0]["loss"]), _bits(outs[1]["loss"])), s
    _assert_same_run(c, d, "grad_clip_norm=1e30 against no clipping")
    assert not _same_bits(a[0].final.kernel, d[0].final.kernel)   # and the real bound did change the run


# ------------------------------------------------------------------ 5. without the arguments
def test_without_the_arguments_nothing_is_launched_and_nothing_changes(launched):
    from lidog_amd.train import build_step
    kind = "MinkUNet34BEV"
    a = _build(kind)
    # the call as it was written before the arguments existed: positional, without them
    model, step, _ = build_step(_model(kind), kind, "Adam", 1e-2, None, 1e-4, 0.98, 0, (0.5, 0.5), 7, -1, 1, None,
                                "SoftDICELoss", None, None, 1.0)
    b = (model, step)
    assert a[1].sam is None and a[1].grad_clip_norm is None and a[1].opt.sqnorm is None
    for s in range(3):
        outs = [run[1].training_step(_batch()) for run in (a, b)]
        assert torch.equal(_bits(outs[0]["loss"]), _bits(outs[1]["loss"])), s
    _assert_same_run(a, b, "defaults against the earlier call signature")
    assert launched and not set(launched) & set(NEW_ENTRY_POINTS)
    assert a[1].opt.sqnorm is None and a[1].opt._sqnorm_ws is None


# ------------------------------------------------------------------ 6. the command line
def test_train_main_with_both_flags_writes_a_checkpoint_that_resumes(tmp_path, capsys):
    from lidog_amd import train
    run = str(tmp_path / "run")
    argv = ["--config", "source8k", "--scans", "4", "--val-scans", "2", "--batch", "2", "--sam-rho", "0.05",
            "--grad-clip-norm", "1.0", "--check-val-every-n-epoch", "1", "--save-dir", run]
    train.main(argv + ["--epochs", "1"])
    logged = capsys.readouterr().out
    losses = [float(x) for x in re.findall(r"'loss': ([-+0-9.e]+|nan|inf)", logged)]
    assert losses and all(math.isfinite(x) for x in losses), logged[-400:]
    ckpt = train.last_checkpoint(run)
    assert ckpt is not None and ckpt.endswith("epoch=0-step=2.ckpt")
    fit = train._fit_from_args(train.parse_args(argv + ["--epochs", "2", "--resume", ckpt]))
    assert fit.epoch == 1 and fit.step.sam is not None and fit.step.sam.rho == 0.05 and fit.step.grad_clip_norm == 1.0
    hist = fit.run()
    assert [h["epoch"] for h in hist] == [1] and all(math.isfinite(x) for x in hist[0]["losses"])
    assert math.isfinite(hist[0]["validation"]["sem_loss"])
    assert train.last_checkpoint(run).endswith("epoch=1-step=4.ckpt")


def test_train_two_sources_with_both_flags():
    from lidog_amd import train
    a = train.parse_args(["--model", "MinkUNet34", "--sources", "source8k", "nusc35k", "--scans", "4", "--val-scans", "2",
                          "--batch", "2", "--epochs", "1", "--sam-rho", "0.5", "--sam-adaptive", "--grad-clip-norm", "1.0"])
    fit = train._fit_from_args(a)
    assert fit.step.num_sources == 2 and fit.step.sam.adaptive
    hist = fit.run()
    assert len(hist[0]["losses"]) == 2 and all(math.isfinite(x) for x in hist[0]["losses"])
