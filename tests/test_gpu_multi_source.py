"""Two-source training on the GPU (configs/*/multi/*.yaml): the loss compositions of the reference's two-source
training_steps, the trunk executor's accumulate mode for the second backward pass over one model, BatchNorm statistics
moved twice per step, gradient buckets that wait for both uses of every parameter on two data-parallel ranks, a
full-size step and the CLI / Fit loop with per-source validation."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import REPO, seeded_state_dict, small_batch

pytestmark = pytest.mark.gpu

KINDS = ["MinkUNet34BEV", "MinkUNet34", "MinkUNet34IBN", "MinkUNet34Robust"]
BEV = 17   # bev_image_size(5.0)


def _source(seeds, n_points, device="cuda"):
    coords = small_batch(tuple(seeds), n_points=n_points)
    labels, bev = [], []
    for b, s in enumerate(seeds):
        g = torch.Generator().manual_seed(5000 + s)
        labels.append(torch.randint(-1, 7, (int((coords[:, 0] == b).sum()),), generator=g))
        bev.append(torch.randint(-1, 7, (1, BEV, BEV), generator=g))
    return coords.to(device), torch.cat(labels).to(device), torch.cat(bev).to(device)


def two_source_batch(seeds0, seeds1, n_points=1200, device="cuda"):
    out = {}
    for s, seeds in enumerate((seeds0, seeds1)):
        coords, labels, bev = _source(seeds, n_points + 300 * s, device)
        out.update({f"source_coordinates{s}": coords.float(), f"source_features{s}": torch.ones((coords.shape[0], 1),
                                                                                                device=device),
                    f"source_sem_labels{s}": labels, f"source_bev_labels{s}": {"block8": bev},
                    "coords_int" if s == 0 else "coords_int1": coords})
    return out


def _model(kind, seed=11):
    from lidog_amd.train import build_model
    m = build_model(kind, bound_2d=5.0, device="cpu")
    m.load_state_dict(seeded_state_dict(m, seed=seed), strict=False)
    return m.cuda().train()


def _step(kind, model, **kw):
    from lidog_amd.train import build_step
    return build_step(model, kind, num_sources=2, **kw)[1]


@pytest.fixture
def executor_off():
    from lidog_amd import trunk
    prev = trunk.ENABLED
    trunk.set_enabled(False)
    yield
    trunk.set_enabled(prev)


# ------------------------------------------------------------------ loss compositions
def _literal(kind, model, batch, epoch, w=(0.5, 0.5), warmup=1):
    """the reference's two-source training_step, restated line by line"""
    import lidog_amd.me as ME
    from lidog_amd.losses import DICELoss, SoftDICELoss, iw_loss
    sem_c, bev_c = SoftDICELoss(ignore_label=-1), DICELoss(ignore_label=-1)
    st = [ME.SparseTensor(coordinates=batch["source_coordinates%d" % s].int(), features=batch["source_features%d" % s])
          for s in (0, 1)]
    if kind == "MinkUNet34BEV":      # trainer_lighting_2d_multi.py:166-205
        out0, bev_preds0 = model(st[0], is_train=True)
        out1, bev_preds1 = model(st[1], is_train=True)
        sem_loss_bev0 = sem_loss_bev1 = 0.0
        for key in batch["source_bev_labels0"].keys():
            sem_loss_bev0 = sem_loss_bev0 + bev_c(bev_preds0[key].view(-1, 7), batch["source_bev_labels0"][key].view(-1)) / len(bev_preds0.keys())
            sem_loss_bev1 = sem_loss_bev1 + bev_c(bev_preds1[key].view(-1, 7), batch["source_bev_labels1"][key].view(-1)) / len(bev_preds1.keys())
        if epoch >= warmup:
            sem_loss0 = sem_c(out0.F, batch["source_sem_labels0"])
            sem_loss1 = sem_c(out1.F, batch["source_sem_labels1"])
            total = w[0] * (sem_loss0 + sem_loss_bev0) + w[1] * (sem_loss1 + sem_loss_bev1)
        else:
            sem_loss0 = sem_loss1 = torch.zeros(())
            total = w[0] * sem_loss_bev0 + w[1] * sem_loss_bev1
        return total, {"sem_loss0": sem_loss0, "sem_loss1": sem_loss1, "bev_loss0": sem_loss_bev0,
                       "bev_loss1": sem_loss_bev1}, (out0.F, out1.F)
    if kind == "MinkUNet34Robust":   # trainer_lighting_robustnet.py:104-140
        out0, out_in0 = model(st[0], is_seg=False)
        sem_loss0 = sem_c(out0.F, batch["source_sem_labels0"])
        aux_loss0 = iw_loss([m.F for m in out_in0])[0] if epoch >= 5 else torch.zeros((), device="cuda")
        out1, out_in1 = model(st[1], is_seg=False)
        sem_loss1 = sem_c(out1.F, batch["source_sem_labels1"])
        aux_loss1 = iw_loss([m.F for m in out_in1])[0] if epoch >= 5 else torch.zeros((), device="cuda")
        total = w[0] * sem_loss0 + w[1] * sem_loss1
        total = total + 0.5 * (aux_loss0 + aux_loss1)
        return total, {"sem_loss0": sem_loss0, "sem_loss1": sem_loss1, "aux_loss0": aux_loss0,
                       "aux_loss1": aux_loss1}, (out0.F, out1.F)
    out0 = model(st[0], is_seg=True)     # trainer_lighting.py:100-116
    out1 = model(st[1], is_seg=True)
    sem_loss0 = sem_c(out0.F, batch["source_sem_labels0"])
    sem_loss1 = sem_c(out1.F, batch["source_sem_labels1"])
    return w[0] * sem_loss0 + w[1] * sem_loss1, {"sem_loss0": sem_loss0, "sem_loss1": sem_loss1}, (out0.F, out1.F)


CASES = [("MinkUNet34BEV", 0), ("MinkUNet34BEV", 1), ("MinkUNet34", 0), ("MinkUNet34IBN", 0),
         ("MinkUNet34Robust", 4), ("MinkUNet34Robust", 5)]


@pytest.mark.parametrize("kind,epoch", CASES, ids=[f"{k}-epoch{e}" for k, e in CASES])
def test_two_source_loss_composition_matches_the_reference(kind, epoch, executor_off):
    batch = two_source_batch((1, 2), (3,))
    model, twin = _model(kind), _model(kind)
    step = _step(kind, model, warmup_epochs=1)
    got = step.forward_loss(batch, epoch)
    want, parts, logits = _literal(kind, twin, batch, epoch)
    for s in (0, 1):
        d = (got["outputs"][s].F.detach() - logits[s].detach()).abs().max().item()
        assert d <= 1e-5, (s, d)
    for k, v in parts.items():
        a, b = float(got[k].detach()), float(v.detach() if torch.is_tensor(v) else v)
        assert abs(a - b) <= 1e-6 * max(abs(b), 1e-12), (k, a, b)
    assert abs(float(got["loss"]) - float(want)) <= 1e-6 * abs(float(want))
    if kind == "MinkUNet34BEV" and epoch == 0:
        assert float(got["sem_loss0"]) == 0.0 and float(got["sem_loss1"]) == 0.0
    if kind == "MinkUNet34Robust":
        assert (float(got["aux_loss0"]) > 0) == (epoch >= 5)


# ------------------------------------------------------------------ accumulate mode: bits
def _two_source_grad(model, opt, step, batch, separately=False):
    import lidog_amd.me as ME
    if separately:
        total = 0
        for s in (0, 1):
            opt.zero_grad()
            x = ME.SparseTensor(coordinates=batch["coords_int" if s == 0 else "coords_int1"],
                                features=batch[f"source_features{s}"])
            sem, bev = model(x, is_train=True)
            from lidog_amd.losses import DICELoss, SoftDICELoss
            loss = 0.5 * (SoftDICELoss(ignore_label=-1)(sem.F, batch[f"source_sem_labels{s}"]) +
                          DICELoss(ignore_label=-1)(bev["block8"].view(-1, 7), batch[f"source_bev_labels{s}"]["block8"].view(-1)))
            loss.backward()
            opt.flat.gather_strays()
            total = total + opt.flat.grad.clone()
        return total
    out = step.forward_loss(batch, 0)
    opt.zero_grad()
    out["loss"].backward()
    opt._prepare()
    torch.cuda.synchronize()
    return opt.flat.grad.clone()


def test_accumulate_mode_is_bit_identical_to_autograd_accumulation():
    from lidog_amd import trunk
    batch = two_source_batch((4, 5), (6, 7))
    res = {}
    for name, on, acc in (("executor", True, True), ("autograd", True, False), ("operator", False, True)):
        model = _model("MinkUNet34BEV")
        step = _step("MinkUNet34BEV", model)
        prev_on, prev_acc = trunk.ENABLED, trunk.set_accumulate(acc)
        trunk.set_enabled(on)
        try:
            res[name] = _two_source_grad(model, step.opt, step, batch)
            paths = step.last_paths
            if name == "executor":
                assert paths == ("_TrunkFnBackward", "_TrunkFnBackward"), paths
                # the trunk's gradients are all written in place (the 2-D head, used twice on the operator path, may
                # leave its autograd sums outside the flat buffer: _prepare gathers them)
                head = len(step.opt.flat.params) - len(trunk.program_of(model).params)
                assert step.opt.strays <= head, (step.opt.strays, head)
                base = step.opt.flat.grad.data_ptr()
                assert all(p.grad is not None and p.grad.data_ptr() == base + 4 * off
                           for p, off in zip(step.opt.flat.params, step.opt.flat.offsets))
                sep = _two_source_grad(model, step.opt, step, batch, separately=True)
        finally:
            trunk.set_enabled(prev_on)
            trunk.set_accumulate(prev_acc)
    assert torch.isfinite(res["executor"]).all()
    assert torch.equal(res["executor"], res["operator"])
    assert torch.equal(res["executor"], res["autograd"])
    flat = step.opt.flat
    for p, off in zip(flat.params, flat.offsets):
        a, b = res["executor"][off:off + p.numel()], sep[off:off + p.numel()]
        assert (a - b).norm() <= 1e-5 * b.norm() + 1e-9, (off, float((a - b).norm()), float(b.norm()))


def test_accumulate_kernel_alignment_and_tail():
    from lidog_amd._lib import call
    g = torch.Generator(device="cuda").manual_seed(0)
    buf = torch.randn(10000, device="cuda", generator=g)
    src = torch.randn(10000, device="cuda", generator=g)
    want = buf.clone()
    segs = []
    for lo, n, so in ((0, 7, 0), (9, 1001, 9), (2050, 4099, 2051), (7000, 0, 0), (8001, 3, 8001)):
        want[lo:lo + n] = want[lo:lo + n] + src[so:so + n]
        segs.append((buf[lo:].data_ptr(), src[so:].data_ptr(), n))
    t = np.array(segs * 1, dtype=np.int64)
    call("lidog_grad_accumulate", t.ctypes.data, len(segs))
    torch.cuda.synchronize()
    assert torch.equal(buf, want)


# ------------------------------------------------------------------ BatchNorm statistics move twice
def test_running_statistics_follow_source0_then_source1():
    import lidog_amd.me as ME
    batch = two_source_batch((8,), (9, 10))
    model, twin = _model("MinkUNet34BEV"), _model("MinkUNet34BEV")
    step = _step("MinkUNet34BEV", model)
    step.training_step(batch)
    assert step.last_paths == ("_TrunkFnBackward", "_TrunkFnBackward")
    with torch.no_grad():
        for s in (0, 1):
            twin(ME.SparseTensor(coordinates=batch["coords_int" if s == 0 else "coords_int1"],
                                 features=batch[f"source_features{s}"]), is_train=True)
    a, b = model.state_dict(), twin.state_dict()
    keys = [k for k in a if "running" in k or "num_batches" in k]
    assert len(keys) > 100
    for k in keys:
        torch.testing.assert_close(a[k], b[k], rtol=1e-6, atol=1e-7, msg=k)


# ------------------------------------------------------------------ full size
@pytest.mark.timeout(300)
def test_full_size_two_source_lidog_step():
    from lidog_amd import synth
    from lidog_amd.train import build_model, build_step
    model = build_model("MinkUNet34BEV")
    _, step, _ = build_step(model, "MinkUNet34BEV", num_sources=2)
    batch = synth.make_batch([0, 1, 2, 3], "kitti120k", "cuda", seeds1=[0, 1, 2, 3], config1="nusc35k")
    out = step.training_step(batch)
    torch.cuda.synchronize()
    assert step.last_paths == ("_TrunkFnBackward", "_TrunkFnBackward")
    for k in ("loss", "sem_loss0", "bev_loss0", "sem_loss1", "bev_loss1"):
        assert np.isfinite(float(out[k])), k
    assert torch.isfinite(step.opt.flat.grad).all() and torch.isfinite(step.opt.flat.flat).all()


# ------------------------------------------------------------------ CLI / Fit
@pytest.mark.timeout(300)
def test_cli_two_sources_fit_validate_resume_predict(tmp_path):
    from lidog_amd.evaluate import predict
    from lidog_amd.train import SynthScans, _fit_from_args, build_model, parse_args
    from lidog_amd.trainer import LiDOGStep
    argv = ["--sources", "source8k", "nusc35k", "--source-weights", "0.4", "0.6", "--epochs", "2", "--scans", "4",
            "--batch", "2", "--val-scans", "2", "--check-val-every-n-epoch", "1", "--save-dir", str(tmp_path)]
    fit = _fit_from_args(parse_args(argv))
    fit.log = lambda *_: None
    assert type(fit.step) is LiDOGStep and fit.step.num_sources == 2 and fit.step.w == (0.4, 0.6)
    hist = fit.run()
    assert len(hist) == 2 and all(np.isfinite(h["losses"]).all() for h in hist)
    for h in hist:
        assert set(h["validation"]) == {"source8k", "nusc35k"}
        assert all(np.isfinite(v["sem_loss"]) for v in h["validation"].values())
    assert os.path.exists(hist[1]["checkpoint"])
    again = _fit_from_args(parse_args(argv[:-1] + [str(tmp_path), "--auto-resume"]))
    assert again.epoch == 2 and again.global_step == fit.global_step
    ck = torch.load(hist[1]["checkpoint"], map_location="cpu", weights_only=False)
    fresh = build_model("MinkUNet34BEV")
    fresh.load_state_dict({k[len("model."):]: v for k, v in ck["state_dict"].items()})
    b = SynthScans(2, "nusc35k", first=100).batch([0, 1], "cuda")
    p1, l1 = predict(fit.model, b["coords_int"], b["source_features0"])
    p2, l2 = predict(fresh, b["coords_int"], b["source_features0"])
    assert torch.equal(p1, p2) and torch.equal(l1, l2)


# ------------------------------------------------------------------ two data-parallel ranks
def _dp_worker(rank, world, port, q, executor):
    try:
        _dp_body(rank, world, port, q, executor)
    except Exception as e:
        import traceback
        q.put((rank, False, f"{e!r}\n{traceback.format_exc()}"))
        raise


def _dp_body(rank, world, port, q, executor):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    torch.cuda.set_device(0)
    import lidog_amd
    import lidog_amd.me as ME
    from lidog_amd import bev as BEV
    from lidog_amd import trunk
    from lidog_amd.losses import DICELoss, SoftDICELoss
    from lidog_amd.optim import FlatAdam
    from lidog_amd.trainer import LiDOGStep, setup_data_parallel
    trunk.set_enabled(executor)
    kw = dict(in_channels=1, out_channels=7, D=3, decoder_2d_level=["block8"], mapping_bound_2d=5.0)
    torch.manual_seed(200 + rank)
    model = lidog_amd.MinkUNet34BEV(**kw)
    sd = seeded_state_dict(model, seed=6)
    if rank == 0:
        model.load_state_dict(sd)
    model = setup_data_parallel(model.cuda())
    model.train()
    opt = FlatAdam(model, lr=1e-3, weight_decay=1e-4, bucket_bytes=8 << 20)
    step = LiDOGStep(model, opt, num_sources=2)
    mine = two_source_batch((20 + rank,), (30 + rank,))
    grads = []
    for deferred in (False, True):
        opt.buckets.deferred = deferred
        out = step.forward_loss(mine)
        took = step.last_paths
        opt.zero_grad()
        out["loss"].backward()
        opt._prepare()
        torch.cuda.synchronize()
        grads.append(opt.flat.grad.clone())
        if not deferred:
            early = opt.buckets.issued_early
            strays = opt.strays
            loss = float(out["loss"])
    ok, msg = True, ""
    if (took == ("_TrunkFnBackward",) * 2) != executor or (not executor and "_TrunkFnBackward" in took):
        ok, msg = False, f"paths {took}"
    if executor and strays:
        ok, msg = False, msg + f" {strays} strays"
    if opt.buckets.uses != 2:       # set once by the two-source step's constructor
        ok, msg = False, msg + f" buckets expect {opt.buckets.uses} uses"
    if not torch.equal(grads[0], grads[1]):
        ok, msg = False, msg + " deferred reduction differs"
    g = grads[0].cpu()
    g0 = g.clone()
    dist.broadcast(g0, src=0)
    if not torch.equal(g, g0):
        ok, msg = False, msg + f" ranks differ by {float((g - g0).abs().max())}"
    if early < 1:
        ok, msg = False, msg + " no bucket was reduced during backward"
    losses = torch.tensor([loss], dtype=torch.float64)
    dist.all_reduce(losses)
    if rank == 0:
        ref = lidog_amd.MinkUNet34BEV(**kw)
        ref.load_state_dict(sd)
        ref.cuda().train()
        ropt = FlatAdam(ref, lr=1e-3, weight_decay=1e-4, local=True)
        sem_c, bev_c = SoftDICELoss(ignore_label=-1), DICELoss(ignore_label=-1)
        tot = 0.0
        for s, seeds in ((0, (20, 21)), (1, (30, 31))):     # both ranks' scans of source s in one batch
            joint = two_source_batch(seeds, seeds)
            coords = joint["coords_int" if s == 0 else "coords_int1"]
            labels, bevl = joint[f"source_sem_labels{s}"], joint[f"source_bev_labels{s}"]["block8"]
            x = ME.SparseTensor(coordinates=coords, features=torch.ones((coords.shape[0], 1), device="cuda"))
            o, _, levels, seg = ref._trunk_forward(x)
            logits = (seg if seg is not None else ref.final(o)).F
            lv = levels["block8"]
            for b in range(2):
                rows = (lv.C[:, 0] == b).nonzero().flatten()
                cb = lv.C[rows].clone()
                cb[:, 0] = 0
                img = BEV._Sparse2SuperFn.apply(lv.F[rows], cb.contiguous(), 1, 5.0, 0.05, (5, 3, 1))
                pred = ref.encoders2d["block8"](img)
                l_bev = bev_c(pred.view(-1, 7), bevl[b].view(-1))
                l_sem = sem_c(logits[rows], labels[rows])
                tot = tot + 0.5 * (l_sem + l_bev) / 2
        ropt.zero_grad()
        tot.backward()
        ropt.flat.gather_strays()
        torch.cuda.synchronize()
        g_ref, g_dp = ropt.flat.grad, grads[0] / world
        if abs(float(losses) / world - float(tot)) > 1e-5:
            ok, msg = False, msg + f" loss {float(losses) / world} vs {float(tot)}"
        worst = 1.0
        for (n, p), off in zip(ref.named_parameters(), ropt.flat.offsets):
            a, b = g_dp[off:off + p.numel()].double(), g_ref[off:off + p.numel()].double()
            c = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300))
            if c < worst:
                worst, wn = c, n
        if worst < 1 - 1e-5:
            ok, msg = False, msg + f" gradient cosine {worst} at {wn}"
    q.put((rank, ok, msg))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("executor", [True, False], ids=["trunk_executor", "operator_path"])
def test_two_source_step_two_ranks(executor):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31800 + os.getpid() % 2000 + (0 if executor else 7)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, executor)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=600) for _ in range(2)]
    failed = not all(ok for _, ok, _ in got)
    for p in procs:
        p.join(10 if failed else 120)
        if p.is_alive():
            p.terminate()
            p.join(30)
    assert not failed, got
