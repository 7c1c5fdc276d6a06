"""The training steps with the auxiliary point criterion (trainer._Step(sem_aux_criterion=..., sem_aux_weight=...),
train.build_step) on the small two-source batch of test_gpu_multi_source.py: the step's sem loss is the point criterion
plus the weighted Lovasz-softmax loss of the same logits, bit for bit; a training step leaves finite, changed weights;
without the argument nothing new is launched and no bit changes; LiDOGStep's warm-up zeroes the auxiliary term too."""
import pytest
import torch

from test_gpu_multi_source import _model, two_source_batch

pytestmark = pytest.mark.gpu

_BATCH = {}


def _batch():
    if not _BATCH:
        _BATCH.update(two_source_batch([0, 1], [2, 3]))
    return _BATCH


def _bits(t):
    return t.detach().view(torch.int32)


@pytest.fixture
def launched(monkeypatch):
    """the names of the entry points the criteria call"""
    from lidog_amd import losses
    names, call = [], losses.call
    monkeypatch.setattr(losses, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    return names


def _by_hand(logits, labels, w):
    from lidog_amd.losses import LovaszSoftmaxLoss, make_criterion
    main = make_criterion("CELoss", -1, 7)(logits.detach(), labels.long())
    aux = LovaszSoftmaxLoss(ignore_label=-1)(logits.detach(), labels.long())
    assert float(aux) > 0
    return main + w * aux


@pytest.mark.parametrize("num_sources", [1, 2])
def test_sem_loss_is_the_criterion_plus_the_weighted_auxiliary_loss(num_sources, launched):
    from lidog_amd.train import build_step
    batch, w = _batch(), 0.75
    _, step, _ = build_step(_model("MinkUNet34"), "MinkUNet34", num_sources=num_sources, sem_criterion="CELoss",
                            sem_aux_criterion="LovaszSoftmaxLoss", sem_aux_weight=w)
    out = step.forward_loss(batch)
    assert launched.count("lidog_lovasz_fwd") == num_sources
    if num_sources == 1:
        total, logits = out
        assert torch.equal(_bits(total), _bits(_by_hand(logits.F, batch["source_sem_labels0"], w)))
    else:
        for s in (0, 1):
            hand = _by_hand(out["outputs"][s].F, batch[f"source_sem_labels{s}"], w)
            assert torch.equal(_bits(out[f"sem_loss{s}"]), _bits(hand))
        total, sem0, sem1 = (float(out[k].detach()) for k in ("loss", "sem_loss0", "sem_loss1"))
        assert total == pytest.approx(0.5 * sem0 + 0.5 * sem1, rel=1e-6)


@pytest.mark.parametrize("kind,num_sources,precision", [("MinkUNet34", 1, None), ("MinkUNet34BEV", 2, None),
                                                        ("MinkUNet34Robust", 1, None), ("MinkUNet34", 2, "bf16")])
def test_a_training_step_leaves_finite_changed_weights(kind, num_sources, precision, launched):
    from lidog_amd.train import build_step
    model, step, _ = build_step(_model(kind), kind, num_sources=num_sources, lr=1e-3, precision=precision,
                                sem_aux_criterion="LovaszSoftmaxLoss", sem_aux_weight=0.5)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    out = step.training_step(_batch())
    assert all(bool(torch.isfinite(v)) for v in out.values() if torch.is_tensor(v))
    assert launched.count("lidog_lovasz_fwd") == launched.count("lidog_lovasz_bwd") == num_sources
    after = dict(model.named_parameters())
    assert all(bool(torch.isfinite(p).all()) for p in after.values())
    changed = sum(not torch.equal(before[n], p.detach()) for n, p in after.items())
    assert changed >= 0.9 * len(before)


def _loss_and_grads(model, step, batch):
    out = step.forward_loss(batch)
    total = out["loss"] if isinstance(out, dict) else out[0]
    step.opt.zero_grad()
    total.backward()
    torch.cuda.synchronize()
    return total.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("num_sources", [1, 2])
def test_without_the_argument_nothing_changes(num_sources, launched):
    """a step built with the constructor's earlier arguments alone against build_step's default: the same launches of
    the criteria and the same bits in the loss and in every gradient"""
    from lidog_amd.train import build_step
    from lidog_amd.trainer import FlatAdam, SourceStep
    batch = _batch()
    m0 = _model("MinkUNet34")
    old = SourceStep(m0, FlatAdam(m0, lr=1e-3, weight_decay=1e-4), (0.5, 0.5), -1, num_sources, None, "SoftDICELoss", 7)
    l0, g0 = _loss_and_grads(m0, old, batch)
    first = list(launched)
    del launched[:]
    m1, new, _ = build_step(_model("MinkUNet34"), "MinkUNet34", num_sources=num_sources)
    assert new.sem_aux_criterion is None
    l1, g1 = _loss_and_grads(m1, new, batch)
    assert first == list(launched) and not any("lovasz" in name for name in launched) and len(first) == 2 * num_sources
    assert torch.equal(_bits(l0), _bits(l1))
    assert g0.keys() == g1.keys() and all(torch.equal(_bits(g), _bits(g1[n])) for n, g in g0.items())


def test_lidog_warm_up_zeroes_the_auxiliary_term_too(launched):
    from lidog_amd.train import build_step
    _, step, _ = build_step(_model("MinkUNet34BEV"), "MinkUNet34BEV", warmup_epochs=1,
                            sem_aux_criterion="LovaszSoftmaxLoss")
    total, sem, bev, _ = step.forward_loss(_batch(), epoch=0)
    assert float(sem) == 0 and not launched.count("lidog_lovasz_fwd")
    assert torch.equal(_bits(total), _bits(bev))
    total, sem, bev, logits = step.forward_loss(_batch(), epoch=1)
    assert launched.count("lidog_lovasz_fwd") == 1 and float(sem.detach()) > 0
    from lidog_amd.losses import LovaszSoftmaxLoss, make_criterion
    labels = _batch()["source_sem_labels0"].long()
    hand = make_criterion("SoftDICELoss", -1, 7)(logits.F.detach(), labels) + \
        1.0 * LovaszSoftmaxLoss(ignore_label=-1)(logits.F.detach(), labels)
    assert torch.equal(_bits(sem), _bits(hand))
