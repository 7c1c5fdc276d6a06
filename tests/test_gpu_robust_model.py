"""MinkUNet34Robust and RobustStep on the device against G10 (the reference class and IWLoss on the CPU oracle,
tests/robust_ref.py) with G9's tolerances: logits, SoftDICE, the five per-map IWLoss values, the epoch-5 total,
gradient norms inside the float64 yardstick, 3 Adam steps; the aux maps' ReLU convention; the epoch switch of the aux
loss; a full-size kitti120k batch-4 step at epoch 5; and the training driver (Fit) -> checkpoint -> fresh model ->
predict."""
import os

import numpy as np
import pytest
import torch

from helpers import seeded_state_dict
from robust_ref import ADAM_LR, ADAM_STEPS, ADAM_WD, G10

pytestmark = pytest.mark.gpu


def _g10_step():
    import lidog_amd
    from lidog_amd.trainer import RobustStep
    g10 = np.load(G10)
    model = lidog_amd.MinkUNet34Robust(1, 7, 3)
    model.load_state_dict(seeded_state_dict(model, seed=7))
    model = model.cuda().train()
    opt = torch.optim.Adam(model.parameters(), lr=ADAM_LR, weight_decay=ADAM_WD)
    coords = torch.from_numpy(g10["coords"]).cuda()
    batch = {"coords_int": coords, "source_features0": torch.ones((coords.shape[0], 1), device="cuda"),
             "source_sem_labels0": torch.from_numpy(g10["labels"]).cuda()}
    return g10, model, RobustStep(model, opt), batch


@pytest.mark.timeout(120)
def test_minkunet34robust_step_matches_g10():
    from lidog_amd.losses import iw_loss
    g10, model, step, batch = _g10_step()
    assert list(model.state_dict().keys()) == list(g10["keys"])
    total, sem_loss, aux_loss, out = step.forward_loss(batch, epoch=5)
    d = (out.F.detach().cpu() - torch.from_numpy(g10["logits"])).abs().max().item()
    assert d <= 1e-4, f"logits differ from G10 by {d}"
    assert abs(float(sem_loss.detach()) - float(g10["sem"])) <= 1e-5
    assert abs(float(aux_loss.detach()) - float(g10["aux"])) <= 1e-5 * max(1.0, float(g10["aux"]))
    assert abs(float(total.detach()) - float(g10["total"])) <= 1e-5
    total.backward()
    params = dict(model.named_parameters())
    bad = []
    for name, g64, e32 in zip(g10["names"], g10["gnorm64"], g10["err32"]):
        got = float(params[str(name)].grad.norm())
        if abs(got - g64) > 5 * e32 * g64 + 1e-7:
            bad.append((str(name), got, float(g64), float(e32)))
    assert not bad, f"gradient norms outside the float64 yardstick: {bad[:5]}"
    # the per-map values, from the aux maps of a fresh forward pass
    with torch.no_grad():
        import lidog_amd.me as ME
        _, maps = model(ME.SparseTensor(batch["source_features0"], coordinates=batch["coords_int"]), is_seg=False)
        _, per = iw_loss([m.F for m in maps])
    assert np.allclose(per.cpu().numpy(), g10["iw"], rtol=1e-4, atol=0), (per.tolist(), g10["iw"].tolist())
    traj = []
    for _ in range(ADAM_STEPS):
        step.opt.step()
        step.opt.zero_grad()
        t, _, _, _ = step.forward_loss(batch, epoch=5)
        t.backward()
        traj.append(float(t.detach()))
    err = np.abs(np.array(traj) - g10["adam_losses"])
    assert err.max() <= 2e-3, (traj, g10["adam_losses"].tolist())


@pytest.mark.timeout(90)
def test_aux_maps_follow_the_reference_relu_convention_and_the_epoch_switch():
    import lidog_amd.me as ME
    g10, model, step, batch = _g10_step()
    x = ME.SparseTensor(batch["source_features0"], coordinates=batch["coords_int"])
    with torch.no_grad():
        _, maps = model(x, is_seg=False)
    assert [m.F.shape[1] for m in maps] == [32, 32, 32, 64, 128]
    # out_in0 and the block1-3 outputs are ReLU'd in place by the reference's later ReLUs; out_in1 is not
    assert [bool(m.F.min() >= 0) for m in maps] == [True, False, True, True, True]
    assert [bool(v >= 0) for v in g10["aux_min"]] == [True, False, True, True, True]
    t4, s4, a4, _ = step.forward_loss(batch, epoch=4)
    assert float(a4) == 0.0 and float(t4) == float(0.5 * s4)
    t5, s5, a5, _ = step.forward_loss(batch, epoch=5)
    assert float(s5) == float(s4) or abs(float(s5) - float(s4)) <= 1e-6   # BN running stats moved, not the batch stats
    assert float(t5) == float(0.5 * s5 + 0.5 * a5) and float(a5) > 0
    res = step.training_step(batch, epoch=5)
    assert set(res) == {"loss", "sem_loss", "aux_loss"} and not any(v.requires_grad for v in res.values())


@pytest.mark.timeout(150)
def test_full_size_kitti_batch4_step_at_epoch_5():
    import lidog_amd
    from lidog_amd import synth
    from lidog_amd.trainer import FlatAdam, RobustStep
    batch = synth.make_batch((0, 1, 2, 3), "kitti120k", device="cuda")
    model = lidog_amd.MinkUNet34Robust(1, 7, 3).cuda().train()
    step = RobustStep(model, FlatAdam(model, lr=1e-2, weight_decay=1e-4))
    res = step.training_step(batch, epoch=5)
    assert all(bool(torch.isfinite(v)) for v in res.values()) and float(res["aux_loss"]) > 0
    assert all(torch.isfinite(p).all() for p in model.parameters())


@pytest.mark.timeout(300)
def test_fit_checkpoint_reload_predict(tmp_path):
    import lidog_amd
    from lidog_amd.evaluate import predict
    from lidog_amd.train import Fit, SynthScans
    fit = Fit(model_kind="MinkUNet34Robust", batch_size=4, optimizer="Adam", lr=1e-2, epochs=1,
              train_data=SynthScans(8), save_dir=str(tmp_path), check_val_every_n_epoch=5, num_sanity_val_steps=0,
              log=lambda *_: None)
    hist = fit.run()
    assert len(hist) == 1 and os.path.exists(hist[0]["checkpoint"]) and np.isfinite(hist[0]["losses"]).all()
    ck = torch.load(hist[0]["checkpoint"], map_location="cpu", weights_only=False)
    fresh = lidog_amd.MinkUNet34Robust(1, 7, 3).cuda()
    fresh.load_state_dict({k[len("model."):]: v for k, v in ck["state_dict"].items()})
    b = SynthScans(2, first=100).batch([0, 1], "cuda")
    p1, l1 = predict(fit.model, b["coords_int"], b["source_features0"])
    p2, l2 = predict(fresh, b["coords_int"], b["source_features0"])
    assert torch.equal(p1, p2) and torch.equal(l1, l2)
