"""MixStyle in the four models on the device (lidog_amd/minkunet.py: _Trunk.mixstyle_layers): the modules add nothing to
the state dict; in eval mode, and in training mode with p = 0, logits (and every parameter gradient) are those of the plain
model bit for bit; with known draws MinkUNet34's training forward and backward equal the same trunk run operator by
operator with MinkowskiMixStyle(draws=...) at the two places, bit for bit; and a two-step Fit with MixStyle finishes,
logs finite losses and writes a checkpoint with the `mixstyle` key that eval_target loads and scores."""
import os

import numpy as np
import pytest
import torch

from helpers import seeded_state_dict, small_batch

pytestmark = pytest.mark.gpu

KINDS = ("MinkUNet34BEV", "MinkUNet34", "MinkUNet34IBN", "MinkUNet34Robust")
STAGES = ("block1", "block2")


def _pair(kind, **ms):
    """(plain model, model with MixStyle behind block1 / block2), the same seeded weights, on the device"""
    import lidog_amd.train as T
    plain = T.build_model(kind, device="cpu")
    model = T.build_model(kind, device="cpu", mixstyle_layers=STAGES, **ms)
    sd = seeded_state_dict(plain, seed=7)
    plain.load_state_dict(sd)
    model.load_state_dict(sd)                       # strict: the keys are the same
    return plain.cuda(), model.cuda()


def _input(coords):
    import lidog_amd.me as ME
    return ME.SparseTensor(torch.ones((coords.shape[0], 1), device="cuda"), coordinates=coords)


def _logits(kind, model, x):
    out = model(x, is_train=True) if kind == "MinkUNet34BEV" else model(x)
    return (out[0] if isinstance(out, tuple) else out).F


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", KINDS)
def test_keys_eval_logits_and_p0_training_are_the_plain_models(kind):
    coords = small_batch((0, 1), n_points=1500).cuda()
    plain, model = _pair(kind, mixstyle_p=0.0)
    assert list(model.state_dict().keys()) == list(plain.state_dict().keys())
    assert [n for n, _ in model.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert list(model.mixstyle.keys()) == list(STAGES)
    plain.eval(), model.eval()
    with torch.no_grad():
        assert torch.equal(_logits(kind, model, _input(coords)), _logits(kind, plain, _input(coords)))
    plain.train(), model.train()
    g = torch.Generator().manual_seed(3)
    outs = []
    for m in (plain, model):
        y = _logits(kind, m, _input(coords))
        if not outs:
            dy = torch.randn(y.shape, generator=g).cuda()
        y.backward(dy)
        outs.append(y.detach())
    assert torch.equal(outs[0], outs[1]), "training-mode logits with p = 0 differ from the plain model's"
    grads = 0
    for (name, p), (_, q) in zip(plain.named_parameters(), model.named_parameters()):
        assert (p.grad is None) == (q.grad is None), name
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), f"gradient of {name} differs with p = 0"
            grads += 1
    assert grads > 100
    for (name, a), (_, b) in zip(plain.state_dict().items(), model.state_dict().items()):
        assert torch.equal(a, b), f"{name} (running statistics) differs with p = 0"


def _seed_whose_first_draws_swap(alpha):
    """the first model seed with which both stages' first draws pair the two scans with each other (a permutation of
    two scans is the identity half of the time, and an identity partner leaves every scan alone)"""
    from lidog_amd.data import draw_mixstyle
    for seed in range(64):
        draws = [draw_mixstyle(np.random.RandomState([seed, stage]), 2, 1.0, alpha) for stage in (1, 2)]
        if all(d[1].tolist() == [1, 0] and (d[0] != 1).all() for d in draws):
            return seed, draws
    raise AssertionError("no seed found")


def _hand_forward(m, x, mix):
    """_Trunk._trunk_forward's operator path, operator by operator, with `mix[stage]` behind block1 / block2"""
    import lidog_amd.me as ME
    out = m._conv_bn_relu(m.conv0p1s1, m.bn0, x)
    skips = [out]
    for i, s in ((1, 1), (2, 2), (3, 4), (4, 8)):
        out = m._conv_bn_relu(getattr(m, f"conv{i}p{s}s2"), getattr(m, f"bn{i}"), out)
        out = getattr(m, f"block{i}")(out)
        if f"block{i}" in mix:
            out = mix[f"block{i}"](out)
        skips.append(out)
    skips.pop()
    for j, s in ((4, 16), (5, 8), (6, 4), (7, 2)):
        out = m._conv_bn_relu(getattr(m, f"convtr{j}p{s}s2"), getattr(m, f"bntr{j}"), out)
        out = ME.cat(out, skips.pop())
        out = getattr(m, f"block{j + 1}")(out)
    return m.final(out)


@pytest.mark.timeout(120)
def test_minkunet34_with_known_draws_equals_the_hand_composition():
    import lidog_amd.me as ME
    import lidog_amd.train as T
    alpha = 0.4
    seed, draws = _seed_whose_first_draws_swap(alpha)
    coords = small_batch((0, 1), n_points=1500).cuda()
    plain = T.build_model("MinkUNet34", device="cpu")
    model = T.build_model("MinkUNet34", device="cpu", mixstyle_layers=STAGES, mixstyle_p=1.0, mixstyle_alpha=alpha,
                          mixstyle_seed=seed)
    sd = seeded_state_dict(plain, seed=7)
    plain.load_state_dict(sd), model.load_state_dict(sd)
    plain, model = plain.cuda().train(), model.cuda().train()
    y = model(_input(coords)).F
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).cuda()
    y.backward(dy)
    given = {name: (lambda t, mod=ME.MinkowskiMixStyle().cuda(), d=d: mod(t, draws=d)) for name, d in zip(STAGES, draws)}
    ref = _hand_forward(plain, _input(coords), given).F
    ref.backward(dy)
    assert torch.equal(y.detach(), ref.detach()), "training forward differs from the hand composition"
    for (name, p), (_, q) in zip(model.named_parameters(), plain.named_parameters()):
        assert torch.equal(p.grad, q.grad), f"gradient of {name} differs from the hand composition's"
    # and MixStyle did act: the same trunk without it gives other logits
    other = T.build_model("MinkUNet34", device="cpu")
    other.load_state_dict(sd)
    assert not torch.equal(other.cuda().train()(_input(coords)).F.detach(), y.detach())


@pytest.mark.timeout(300)
def test_fit_two_steps_checkpoint_and_eval_target(tmp_path, capsys):
    from lidog_amd import eval_target
    from lidog_amd.train import Fit, SynthScans
    logs = []
    fit = Fit(model_kind="MinkUNet34", batch_size=4, optimizer="Adam", lr=1e-2, epochs=1,
              train_data=SynthScans(8, "source8k"), save_dir=str(tmp_path), check_val_every_n_epoch=5,
              num_sanity_val_steps=0, log=logs.append, mixstyle=STAGES, mixstyle_p=1.0, mixstyle_alpha=0.3)
    assert list(fit.model.mixstyle.keys()) == list(STAGES) and fit.model.mixstyle["block2"].p == 1.0
    hist = fit.run()
    assert len(hist) == 1 and len(hist[0]["losses"]) == 2 and np.isfinite(hist[0]["losses"]).all()
    ck = torch.load(hist[0]["checkpoint"], map_location="cpu", weights_only=False)
    assert ck["mixstyle"] == {"layers": list(STAGES), "p": 1.0, "alpha": 0.3}
    assert not any("mixstyle" in k for k in ck["state_dict"])
    capsys.readouterr()
    res = eval_target.main(["--checkpoint", hist[0]["checkpoint"], "--model", "MinkUNet34", "--sources", "source8k",
                            "--targets", "source8k", "--scans", "2", "--batch", "2"])
    assert res[0]["scans"] == 2 and res[0]["checkpoint_epoch"] == 0 and np.isfinite(res[0]["mean_iou"])
    assert os.path.exists(res[0]["csv"])
