"""MinkUNet34IBN on the device: the fused IBN pass (ME.ibn_relu) equals the literal relu(cat(bn(x), in(x))) bit for bit
in forward and every gradient; the model against G9 (the reference class on the CPU oracle, tests/ibn_ref.py): logits,
SoftDICE loss, gradient norms inside the float64 yardstick, 3 Adam steps; the reference's literal call order
(minkunet_ibn.py:33-50,139-206) restated test-locally gives the product model's logits; a full-size kitti120k step; and
the training driver (Fit) -> checkpoint -> fresh model -> predict."""
import copy
import os

import numpy as np
import pytest
import torch

from helpers import seeded_state_dict, small_batch
from ibn_ref import ADAM_LR, ADAM_STEPS, ADAM_WD, G9, instance_norm64

pytestmark = pytest.mark.gpu


def _fused_equals_literal(coords, C, expect_fused=True):
    """ME.ibn_relu against relu(cat(bn(x), in(x))) through the module's operators on `coords`: torch.equal on the output,
    every gradient and the running statistics"""
    import lidog_amd.me as ME
    g = torch.Generator().manual_seed(C)
    n = coords.shape[0]
    f0 = (torch.randn((n, C), generator=g) * 1.5 + 0.3).cuda()
    dy = torch.randn((n, 2 * C), generator=g).cuda()
    bn, inn = ME.MinkowskiBatchNorm(C).cuda(), ME.MinkowskiInstanceNorm(C).cuda()
    with torch.no_grad():
        for p in (bn.bn.weight, bn.bn.bias, inn.weight, inn.bias):
            p.copy_(torch.randn(p.shape, generator=g) * 0.5 + (1.0 if p is bn.bn.weight or p is inn.weight else 0.0))
    results = []
    for fused in (True, False):
        b, i = copy.deepcopy(bn), copy.deepcopy(inn)
        f = f0.clone().requires_grad_(True)
        x = ME.SparseTensor(f, coordinates=coords)
        if fused:
            out = ME.ibn_relu(b, i, x)
            assert (type(out.F.grad_fn).__name__ == "_IBNReluFnBackward") == expect_fused
        else:
            out = ME.MinkowskiReLU(inplace=True)(ME.cat(b(x), i(x)))
        out.F.backward(dy)
        results.append([out.F.detach(), f.grad, b.bn.weight.grad, b.bn.bias.grad, i.weight.grad, i.bias.grad,
                        b.bn.running_mean, b.bn.running_var])
    names = ["y", "dx", "bn dweight", "bn dbias", "in dweight", "in dbias", "running_mean", "running_var"]
    for a, r, what in zip(results[0], results[1], names):
        assert torch.equal(a, r), f"{what} differs (C={C}): max {((a - r).abs().max().item())}"


@pytest.mark.timeout(90)
@pytest.mark.parametrize("C", [32, 64, 128])
def test_fused_ibn_relu_is_bit_identical_to_the_literal_composition(C):
    coords = small_batch((0, 1), n_points=1500)
    coords = coords[torch.randperm(coords.shape[0], generator=torch.Generator().manual_seed(1))].contiguous().cuda()
    _fused_equals_literal(coords, C)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("name,C,fused", [("tiny16", 32, True), ("b17_literal", 128, False), ("empty_middle", 64, True)])
def test_fused_ibn_relu_is_bit_identical_on_scan_layouts(name, C, fused):
    """the layouts of test_gpu_inorm64.MODULE_LAYOUTS: 16 scans shorter than a row block and one long one, 17 scans at
    C = 128 (2 B C > 4096: ibn_relu itself takes the literal composition), a scan without rows in the middle"""
    import inorm_ref as IR
    sizes = {"tiny16": IR.TINY, "b17_literal": IR._uneven(4000, 17), "empty_middle": [3000, 0, 2003]}[name]
    d = IR.make_case(dict(C=C, sizes=sizes, order="shuffled"))
    i = torch.arange(d["n"], dtype=torch.int32)
    coords = torch.stack([d["batch"], i % 64, (i // 64) % 64, i // 4096], dim=1).contiguous().cuda()
    _fused_equals_literal(coords, C, expect_fused=fused)


def _g9_model():
    import lidog_amd
    g9 = np.load(G9)
    model = lidog_amd.MinkUNet34IBN(1, 7, 3)
    model.load_state_dict(seeded_state_dict(model, seed=7))
    return g9, model.cuda().train()


def _forward_loss(model, coords, labels):
    import lidog_amd.me as ME
    from oracle.ref_torch import soft_dice_loss_ref
    x = ME.SparseTensor(torch.ones((coords.shape[0], 1), device="cuda"), coordinates=coords)
    sem = model(x, is_seg=True)
    return sem, soft_dice_loss_ref(sem.F, labels)


@pytest.mark.timeout(120)
def test_minkunet34ibn_matches_g9():
    g9, model = _g9_model()
    coords, labels = torch.from_numpy(g9["coords"]).cuda(), torch.from_numpy(g9["labels"])
    assert list(model.state_dict().keys()) == list(g9["keys"])
    sem, loss = _forward_loss(model, coords, labels)
    d = (sem.F.detach().cpu() - torch.from_numpy(g9["logits"])).abs().max().item()
    assert d <= 1e-4, f"logits differ from G9 by {d}"
    assert abs(float(loss.detach()) - float(g9["loss"])) <= 1e-5
    loss.backward()
    params = dict(model.named_parameters())
    bad = []
    for name, g64, e32 in zip(g9["names"], g9["gnorm64"], g9["err32"]):
        got = float(params[str(name)].grad.norm())
        if abs(got - g64) > 5 * e32 * g64 + 1e-7:
            bad.append((str(name), got, float(g64), float(e32)))
    assert not bad, f"gradient norms outside the float64 yardstick: {bad[:5]}"
    opt = torch.optim.Adam(model.parameters(), lr=ADAM_LR, weight_decay=ADAM_WD)
    traj = []
    for _ in range(ADAM_STEPS):
        opt.step()
        opt.zero_grad()
        _, lo = _forward_loss(model, coords, labels)
        lo.backward()
        traj.append(float(lo.detach()))
    err = np.abs(np.array(traj) - g9["adam_losses"])
    assert err.max() <= 2e-3, (traj, g9["adam_losses"].tolist())


def _literal_forward(m, x):
    """minkunet_ibn.py:139-206 and :33-50 / resnet_block.py BasicBlock, module by module, as the reference calls them"""
    import lidog_amd.me as ME
    relu = m.relu

    def block(b, x):
        residual = x
        out = b.conv1(x)
        if hasattr(b, "in_norm1"):
            out = relu(ME.cat(b.bn_norm1(out), b.in_norm1(out)))
        else:
            out = relu(b.norm1(out))
        out = b.norm2(b.conv2(out))
        if b.downsample is not None:
            residual = b.downsample(x)
        out += residual
        return relu(out)

    def layer(seq, x):
        for b in seq:
            x = block(b, x)
        return x

    out_p1 = relu(m.bn0(m.conv0p1s1(x)))
    out = relu(m.bn1(m.conv1p1s2(out_p1)))
    out_b1p2 = layer(m.block1, out)
    out = relu(m.bn2(m.conv2p2s2(out_b1p2)))
    out_b2p4 = layer(m.block2, out)
    out = relu(m.bn3(m.conv3p4s2(out_b2p4)))
    out_b3p8 = layer(m.block3, out)
    out = relu(m.bn4(m.conv4p8s2(out_b3p8)))
    out_bottle = layer(m.block4, out)
    out = relu(m.bntr4(m.convtr4p16s2(out_bottle)))
    out = layer(m.block5, ME.cat(out, out_b3p8))
    out = relu(m.bntr5(m.convtr5p8s2(out)))
    out = layer(m.block6, ME.cat(out, out_b2p4))
    out = relu(m.bntr6(m.convtr6p4s2(out)))
    out = layer(m.block7, ME.cat(out, out_b1p2))
    out = relu(m.bntr7(m.convtr7p2s2(out)))
    out = layer(m.block8, ME.cat(out, out_p1))
    return m.final(out), out_bottle


@pytest.mark.timeout(90)
def test_reference_call_order_gives_the_product_logits():
    import lidog_amd.me as ME
    g9, model = _g9_model()
    coords = torch.from_numpy(g9["coords"]).cuda()
    twin = copy.deepcopy(model)
    seg, bottle = model(ME.SparseTensor(torch.ones((coords.shape[0], 1), device="cuda"), coordinates=coords),
                        is_seg=False)
    with torch.no_grad():
        rseg, rbottle = _literal_forward(twin, ME.SparseTensor(torch.ones((coords.shape[0], 1), device="cuda"),
                                                               coordinates=coords))
    assert (seg.F.detach() - rseg.F).abs().max().item() <= 1e-4
    assert (bottle.F.detach() - rbottle.F).abs().max().item() <= 1e-4
    assert bottle.F.shape[1] == 256


@pytest.mark.timeout(150)
def test_full_size_kitti_step_and_instance_norm_outputs():
    import lidog_amd
    import lidog_amd.me as ME
    from lidog_amd.losses import SoftDICELoss
    from lidog_amd import synth
    batch = synth.make_batch((0, 1), "kitti120k", device="cuda")
    model = lidog_amd.MinkUNet34IBN(1, 7, 3).cuda().train()
    seen = {}
    model.block1[0].conv1.register_forward_hook(lambda mod, inp, out: seen.setdefault("x", out))
    x = ME.SparseTensor(batch["source_features0"], coordinates=batch["coords_int"])
    sem = model(x, is_seg=True)
    loss = SoftDICELoss(ignore_label=-1)(sem.F, batch["source_sem_labels0"])
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(sem.F).all()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    h = seen["x"]
    blk = model.block1[0]
    with torch.no_grad():
        out = ME.ibn_relu(blk.bn_norm1, blk.in_norm1, h).F
        C = h.F.shape[1]
        ref = torch.relu(instance_norm64(h.F.double(), h.C[:, 0], blk.in_norm1.weight.double(),
                                         blk.in_norm1.bias.double()))
    err = (out[:, C:].double() - ref).abs().max().item()
    assert err <= 1e-5 * ref.abs().max().item(), err


@pytest.mark.timeout(300)
def test_fit_checkpoint_reload_predict(tmp_path):
    import lidog_amd
    from lidog_amd.checkpoint import load_training_checkpoint  # noqa: F401  (the driver's own loader is used by Fit)
    from lidog_amd.evaluate import predict
    from lidog_amd.train import Fit, SynthScans
    fit = Fit(model_kind="MinkUNet34IBN", batch_size=4, optimizer="Adam", lr=1e-2, epochs=1, train_data=SynthScans(8),
              save_dir=str(tmp_path), check_val_every_n_epoch=5, num_sanity_val_steps=0, log=lambda *_: None)
    hist = fit.run()
    assert len(hist) == 1 and os.path.exists(hist[0]["checkpoint"]) and np.isfinite(hist[0]["losses"]).all()
    ck = torch.load(hist[0]["checkpoint"], map_location="cpu", weights_only=False)
    fresh = lidog_amd.MinkUNet34IBN(1, 7, 3).cuda()
    fresh.load_state_dict({k[len("model."):]: v for k, v in ck["state_dict"].items()})
    b = SynthScans(2, first=100).batch([0, 1], "cuda")
    p1, l1 = predict(fit.model, b["coords_int"], b["source_features0"])
    p2, l2 = predict(fresh, b["coords_int"], b["source_features0"])
    assert torch.equal(p1, p2) and torch.equal(l1, l2)
