"""The training steps with their criteria chosen by name (trainer._Step(sem_criterion=...), LiDOGStep(sem_bev_criterion=...),
train.build_step) on two source8k scans: the loss is the module applied by hand to the step's logits, every parameter
gets a finite gradient, the trunk executor still takes the pass, the defaults spelled out change no bit, CELoss steps
lower the loss, and the two-source and bf16 steps run."""
import pytest
import torch

from helpers import seeded_state_dict

pytestmark = pytest.mark.gpu

POINT = ["CELoss", "DICELoss", "SoftDICELoss", "FocalLoss"]
BEV = ["DICELoss", "SoftDICELoss", "CELoss"]


def _model(kind, seed=5):
    from lidog_amd.train import build_model
    m = build_model(kind, bound_2d=50.0, device="cpu")
    m.load_state_dict(seeded_state_dict(m, seed=seed), strict=False)
    return m.cuda().train()


def _step(kind, **kw):
    from lidog_amd.train import build_step
    model, step, _ = build_step(_model(kind), kind, **kw)
    return model, step


_BATCH = {}


def _batch():
    from lidog_amd import synth
    if not _BATCH:
        _BATCH.update(synth.make_batch([3, 4], "source8k", "cuda"))
    return _BATCH


def _backward(model, step, batch):
    out = step.forward_loss(batch)
    step.opt.zero_grad()
    out[0].backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return out, grads


def _finite_everywhere(model, grads):
    """every parameter the pass reaches has a finite gradient, and the pass reaches (nearly) all of them"""
    assert len(grads) >= 0.9 * len(list(model.parameters()))
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert any(float(g.abs().max()) > 0 for g in grads.values())


@pytest.mark.parametrize("name", POINT)
def test_source_step_with_each_criterion(name):
    from lidog_amd.losses import make_criterion
    model, step = _step("MinkUNet34", sem_criterion=name)
    batch = _batch()
    out, grads = _backward(model, step, batch)
    total, sem = out[0], out[-1]
    assert step.last_path == "_TrunkFnBackward"
    by_hand = make_criterion(name, -1, 7)(sem.F.detach(), batch["source_sem_labels0"].long())
    assert torch.equal(total.detach().view(torch.int32), by_hand.view(torch.int32))
    _finite_everywhere(model, grads)


@pytest.mark.parametrize("sem,bev", [(p, BEV[i % 3]) for i, p in enumerate(POINT)] + [("CELoss", "CELoss")])
def test_lidog_step_with_each_criterion(sem, bev):
    from lidog_amd.losses import make_bev_criterion, make_criterion
    model, step = _step("MinkUNet34BEV", sem_criterion=sem, sem_bev_criterion=bev)
    batch = _batch()
    seen, crit = [], step.bev_criterion
    step.bev_criterion = lambda x, y: (seen.append((x.detach(), y)), crit(x, y))[1]    # what the BEV criterion is given
    out, grads = _backward(model, step, batch)
    total, sem_l, bev_l, logits = out
    assert step.last_path == "_TrunkFnBackward"
    hand_sem = make_criterion(sem, -1, 7)(logits.F.detach(), batch["source_sem_labels0"].long())
    assert torch.equal(sem_l.detach().view(torch.int32), hand_sem.view(torch.int32))
    (bx, by), = seen                    # one level; NCHW [2, 7, 167, 167] read through .view(-1, 7)
    assert tuple(bx.shape) == (2 * 167 * 167, 7) and torch.equal(by, batch["source_bev_labels0"]["block8"].view(-1))
    hand_bev = make_bev_criterion(bev, -1)(bx, by)
    assert torch.equal(bev_l.detach().view(torch.int32), hand_bev.view(torch.int32))
    assert float(total.detach()) == pytest.approx(0.5 * float(sem_l.detach()) + 0.5 * float(bev_l.detach()), rel=1e-6)
    _finite_everywhere(model, grads)


@pytest.mark.parametrize("kind", ["MinkUNet34", "MinkUNet34BEV"])
def test_defaults_spelled_out_change_no_bit(kind):
    from lidog_amd import losses as L
    batch = _batch()
    named = dict(sem_criterion="SoftDICELoss")
    if kind == "MinkUNet34BEV":
        named["sem_bev_criterion"] = "DICELoss"
    res = []
    for kw in ({}, named):
        model, step = _step(kind, **kw)
        assert type(step.sem_criterion) is L.SoftDICELoss and not step.sem_criterion.is_kitti
        if kind == "MinkUNet34BEV":
            assert type(step.bev_criterion) is L.DICELoss
        out, grads = _backward(model, step, batch)
        res.append((out[0].detach().clone(), grads))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32))
    assert res[0][1].keys() == res[1][1].keys() and all(torch.equal(g, res[1][1][n]) for n, g in res[0][1].items())


def test_celoss_steps_lower_the_loss():
    model, step = _step("MinkUNet34BEV", lr=1e-3, sem_criterion="CELoss", sem_bev_criterion="CELoss")
    batch = _batch()
    losses = [float(step.training_step(batch)["loss"]) for _ in range(8)]
    assert all(l == l and abs(l) < 1e6 for l in losses), losses
    assert losses[-1] < losses[0], losses


def test_two_source_and_bf16_steps_run():
    from test_gpu_multi_source import _model as ms_model, two_source_batch
    from lidog_amd.train import build_step
    batch = two_source_batch([0, 1], [2, 3])
    _, step, _ = build_step(ms_model("MinkUNet34BEV"), "MinkUNet34BEV", num_sources=2, sem_criterion="CELoss",
                            sem_bev_criterion="CELoss")
    out = step.training_step(batch)
    assert all(bool(torch.isfinite(out[k])) for k in ("loss", "sem_loss0", "sem_loss1", "bev_loss0", "bev_loss1"))
    assert float(out["sem_loss0"]) > 0 and float(out["bev_loss1"]) > 0
    _, bstep = _step("MinkUNet34", precision="bf16", sem_criterion="CELoss")
    out = bstep.training_step(_batch())
    assert bool(torch.isfinite(out["loss"])) and bstep.last_path != "_TrunkFnBackward"
