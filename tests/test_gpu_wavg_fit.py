"""Weight averaging through the training stack on the GPU (lidog_amd.optim.WeightAverage, Fit(weight_average=...),
checkpoints, eval_target --weights averaged) on the small scenes and models of the existing training tests: the average
after every optimiser step against the numpy restatement bit for bit with one launch per update; a run without the
argument launches nothing and a run with it leaves every live bit where it was; applied() computes what a fresh model
with the averaged state computes and leaves no trace in the steps that follow (the cache rule); update_bn against float64;
the two checkpoint keys and their resume; the -avg results files."""
import os

import numpy as np
import pytest
import torch

import sparse_ref as SR
import wavg_ref as R
from helpers import seeded_state_dict
from test_gpu_multi_source import _model, two_source_batch
from test_gpu_train import _Scenes

pytestmark = pytest.mark.gpu

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


@pytest.fixture
def launched(monkeypatch):
    """the names of the entry points lidog_amd.optim calls"""
    from lidog_amd import optim
    names, call = [], optim.call
    monkeypatch.setattr(optim, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    return names


# ------------------------------------------------------------------ 1. the average after every optimiser step
SCHEDULES = {"ema": dict(mode="ema", decay=0.9, final_decay=0.999, total_steps=6), "swa": dict(mode="swa")}


@pytest.mark.parametrize("kind", ["MinkUNet34", "MinkUNet34BEV"])
def test_average_follows_the_restatement_bit_for_bit(kind, launched):
    """6 steps, an EMA on the cosine schedule and an SWA side by side over one optimiser: after every step the averaged
    parameters and running statistics are the restatement applied to host copies of the live ones.  (A parameter that
    got no gradient is averaged like any other: c0 a + c1 a is not a bit for bit, and nothing here assumes it is.)"""
    from lidog_amd.optim import WeightAverage
    from lidog_amd.train import build_step
    model, step, _ = build_step(_model(kind), kind, lr=1e-2)
    avgs = {name: WeightAverage(step.opt, model, **kw) for name, kw in SCHEDULES.items()}
    flat = step.opt.flat
    buffers = avgs["ema"]._live
    assert len(buffers) >= 60 and all("running_" in k for k, _ in buffers)
    assert avgs["ema"].n_segs == 1 + len(buffers) and avgs["ema"].table.is_cuda
    host = {name: None for name in avgs}
    for s in range(6):
        step.training_step(_batch())
        del launched[:]
        for avg in avgs.values():
            avg.update()
        assert launched == ["lidog_wavg_apply"] * 2               # one launch per update, nothing else
        live = np.concatenate([flat.flat.cpu().numpy()] + [b.detach().reshape(-1).cpu().numpy() for _, b in buffers])
        for name, avg in avgs.items():
            host[name] = R.update(host[name], live, s, **SCHEDULES[name])
            got = np.concatenate([avg.params.cpu().numpy()] + [v.reshape(-1).cpu().numpy() for v in avg._buffer_views])
            bad = np.flatnonzero(got.view(np.int32) != host[name].view(np.int32))
            assert bad.size == 0, f"{kind} {name} step {s}: {bad.size} of {got.size} words differ, first {bad[0]}"
            assert avg.num_updates == s + 1
    # the state dict names what the flat storage holds; integer buffers are the live ones
    sd, live_sd = avgs["swa"].averaged_state_dict(), model.state_dict()
    assert list(sd) == list(live_sd) and all(not v.is_cuda for v in sd.values())
    off = dict(zip((id(p) for p in flat.params), flat.offsets))
    for k, p in model.named_parameters():
        assert torch.equal(_bits(sd[k]), _bits(avgs["swa"].params[off[id(p)]:off[id(p)] + p.numel()].view(p.shape).cpu())), k
    for k, v in live_sd.items():
        if not v.is_floating_point():
            assert int(sd[k]) == int(v) == 6, k                   # flushed by the state-dict hook
    for (k, _), view in zip(buffers, avgs["swa"]._buffer_views):
        assert torch.equal(_bits(sd[k]), _bits(view.cpu())), k


# ------------------------------------------------------------------ 2, 5, 6: Fit, checkpoints, eval_target
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Fit for 2 epochs x 3 steps on one seed: without the argument, with weight_average="ema"; validated every epoch"""
    import lidog_amd
    from lidog_amd import optim
    from lidog_amd.train import Fit
    root = tmp_path_factory.mktemp("wavg")
    sd = seeded_state_dict(lidog_amd.MinkUNet34(in_channels=1, out_channels=7, D=3), seed=11)
    kw = dict(model_kind="MinkUNet34", batch_size=2, optimizer="Adam", lr=1e-2, scheduler="ExponentialLR", epochs=2,
              train_data=_Scenes(6), val_data=_Scenes(4, seed0=80), check_val_every_n_epoch=1, state_dict=sd,
              log_every_n_steps=3, log=lambda *_: None)
    out = {"kw": kw, "root": str(root)}
    names, call = [], optim.call
    optim.call = lambda name, *a: (names.append(name), call(name, *a))[1]
    try:
        for tag, extra in (("plain", {}), ("ema", dict(weight_average="ema", avg_decay=0.5))):
            del names[:]
            fit = Fit(save_dir=str(root / tag), **kw, **extra)
            out[tag] = dict(fit=fit, hist=fit.run(), calls=list(names),
                            state={k: v.detach().cpu().clone() for k, v in fit.model.state_dict().items()})
    finally:
        optim.call = call
    return out


def test_without_the_argument_nothing_changes(runs):
    plain, ema = runs["plain"], runs["ema"]
    assert "lidog_wavg_apply" not in plain["calls"] and plain["fit"].avg is None
    # 6 updates, and a swap into and out of each of the two averaged validations
    assert ema["calls"].count("lidog_wavg_apply") == 6 + 2 * 2 and ema["fit"].avg.num_updates == 6
    for h0, h1 in zip(plain["hist"], ema["hist"]):
        assert h0["losses"] == h1["losses"] and h0["validation"] == h1["validation"] and h0["lr"] == h1["lr"]
        assert "validation_avg" not in h0
        assert set(h1["validation_avg"]) == set(h1["validation"]) and h1["validation_avg"]["steps"] == 2
        assert h1["validation_avg"]["sem_loss"] != h1["validation"]["sem_loss"]
    _assert_same_state(plain["state"], ema["state"], "final live state_dict")


def test_metrics_file_gets_the_averaged_validation_under_its_own_keys(runs):
    import json
    rec = {}
    for tag in ("plain", "ema"):
        with open(os.path.join(runs["root"], tag, "metrics.jsonl")) as f:
            rec[tag] = [json.loads(line) for line in f]
    live = [r for r in rec["ema"] if not any(k.startswith("validation_avg/") for k in r)]
    assert live == rec["plain"]                                   # the live records: same keys, same values
    avg = [r for r in rec["ema"] if any(k.startswith("validation_avg/") for k in r)]
    val = [r for r in rec["plain"] if any(k.startswith("validation/") for k in r)]
    assert len(avg) == len(val) == 2
    for a, v in zip(avg, val):
        assert a["step"] == v["step"] and a["validation_avg/epoch"] == v["validation/epoch"]
        assert {k.replace("validation_avg/", "validation/") for k in a} >= {"validation/epoch", "step"}
        assert all(k == "step" or k.startswith("validation_avg/") for k in a)


def test_checkpoint_holds_the_average_and_resumes_it(runs):
    from lidog_amd.checkpoint import model_state_dict
    from lidog_amd.train import Fit
    ema = runs["ema"]
    last = torch.load(ema["hist"][1]["checkpoint"], map_location="cpu", weights_only=False)
    plain = torch.load(runs["plain"]["hist"][1]["checkpoint"], map_location="cpu", weights_only=False)
    assert set(last) - set(plain) == {"averaged_state_dict", "weight_average"}
    assert last["weight_average"] == dict(mode="ema", decay=0.5, final_decay=None, total_steps=6, num_updates=6)
    _assert_same_state(model_state_dict(last, "averaged"), ema["fit"].avg.averaged_state_dict(), "averaged_state_dict")
    _assert_same_state(last["state_dict"], plain["state_dict"], "live state_dict of the checkpoint")
    first = torch.load(ema["hist"][0]["checkpoint"], map_location="cpu", weights_only=False)
    lines = []
    again = Fit(save_dir=os.path.join(runs["root"], "again"), resume=ema["hist"][0]["checkpoint"],
                weight_average="ema", avg_decay=0.5, **dict(runs["kw"], log=lines.append))
    assert again.epoch == 1 and again.avg.num_updates == 3 == first["weight_average"]["num_updates"]
    _assert_same_state(again.avg.averaged_state_dict(), model_state_dict(first, "averaged"), "resumed average")
    assert any("3 updates restored" in str(l) for l in lines)
    h = again.run()
    assert again.avg.num_updates == 6 and "validation_avg" in h[0]
    # an interrupted run against the uninterrupted one: what test_fit_source_recipe_matches_oracle_and_resumes allows
    np.testing.assert_allclose(h[0]["losses"], ema["hist"][1]["losses"], rtol=0, atol=1e-6)
    # a checkpoint without the keys starts the average afresh, and says so; without the flag the keys are ignored
    lines = []
    fresh = Fit(resume=runs["plain"]["hist"][0]["checkpoint"], weight_average="swa", **dict(runs["kw"], log=lines.append))
    assert fresh.avg.num_updates == 0 and any("starts afresh" in str(l) for l in lines)
    ignoring = Fit(resume=ema["hist"][0]["checkpoint"], **runs["kw"])
    assert ignoring.avg is None and ignoring.epoch == 1


def test_eval_target_averaged_writes_its_own_files(runs, tmp_path):
    from lidog_amd import eval_target
    ckpt = runs["ema"]["hist"][1]["checkpoint"]
    run = os.path.dirname(os.path.dirname(ckpt))
    argv = ["--model", "MinkUNet34", "--sources", "source8k", "--targets", "source8k", "--scans", "2", "--batch", "2"]
    assert not os.path.exists(os.path.join(run, "results"))
    res = eval_target.main(["--checkpoint", ckpt, "--weights", "averaged", "--save-predictions"] + argv)
    avg_csv = os.path.join(run, "results", "source8k-TO-source8k-avg.csv")
    assert res[0]["csv"] == avg_csv and os.listdir(os.path.join(run, "results")) == ["source8k-TO-source8k-avg.csv"]
    assert os.path.isdir(os.path.join(run, "predictions-avg")) and not os.path.exists(os.path.join(run, "predictions"))
    # the same row as --weights live on a copy whose state_dict is the averaged one
    ck = torch.load(ckpt, map_location="cpu", weights_only=False)
    os.makedirs(tmp_path / "swapped" / "checkpoints")
    swapped = str(tmp_path / "swapped" / "checkpoints" / "swapped.ckpt")
    torch.save(dict(ck, state_dict=ck["averaged_state_dict"]), swapped)
    res_live = eval_target.main(["--checkpoint", swapped] + argv)
    assert res_live[0]["csv"].endswith("source8k-TO-source8k.csv")
    assert np.array_equal(res[0]["counts"], res_live[0]["counts"])
    assert open(avg_csv).read() == open(res_live[0]["csv"]).read()
    really_live = eval_target.main(["--checkpoint", ckpt] + argv)
    assert not np.array_equal(really_live[0]["counts"], res[0]["counts"])
    assert sorted(os.listdir(os.path.join(run, "results"))) == ["source8k-TO-source8k-avg.csv", "source8k-TO-source8k.csv"]
    # a checkpoint without the key
    with pytest.raises(SystemExit) as e:
        eval_target.main(["--checkpoint", runs["plain"]["hist"][1]["checkpoint"], "--weights", "averaged"] + argv)
    assert "averaged_state_dict" in str(e.value) and "--weight-average" in str(e.value)


# ------------------------------------------------------------------ 3. applied()
def _trained(kind, precision=None, steps=2):
    """a step object after `steps` training steps, each folded into an EMA of decay 0.5"""
    from lidog_amd.optim import WeightAverage
    from lidog_amd.train import build_step
    model, step, _ = build_step(_model(kind), kind, lr=1e-2, precision=precision)
    avg = WeightAverage(step.opt, model, "ema", decay=0.5)
    for _ in range(steps):
        step.training_step(_batch())
        avg.update()
    return model, step, avg


def _eval_logits(model, precision=None):
    import lidog_amd.me as ME
    from lidog_amd import precision as P
    b = _batch()
    was = model.training
    model.eval()
    with torch.no_grad(), P.scope(model, precision):
        out = model(ME.SparseTensor(coordinates=b["coords_int"], features=b["source_features0"]))
    model.train(was)
    return (out[0] if isinstance(out, tuple) else out).F.detach().clone()


def _train_logits(step):
    out = step.forward_loss(_batch())
    return out[-1].F.detach().clone(), step.last_path


@pytest.mark.parametrize("kind", ["MinkUNet34", "MinkUNet34BEV"])
def test_applied_computes_what_a_model_with_the_averaged_state_computes(kind):
    from lidog_amd import trunk
    from lidog_amd.train import build_step
    model, step, avg = _trained(kind)
    sd = avg.averaged_state_dict()
    assert any(not torch.equal(sd[k], v.cpu()) for k, v in model.state_dict().items())
    twin = _model(kind)
    twin.load_state_dict(sd)
    twin, twin_step, _ = build_step(twin, kind, lr=1e-2)
    live_before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with avg.applied():
        with pytest.raises(RuntimeError, match="nested"):
            with avg.applied():
                pass
        with pytest.raises(RuntimeError, match="applied"):
            avg.update()
        _assert_same_state(avg.averaged_state_dict(), sd, "averaged_state_dict inside applied()")
        for precision in (None, "bf16"):
            assert torch.equal(_bits(_eval_logits(model, precision)), _bits(_eval_logits(twin, precision))), precision
        assert not torch.equal(_eval_logits(model, "bf16"), _eval_logits(model, None))
    _assert_same_state(model.state_dict(), live_before, "live state after applied()")
    _assert_same_state(avg.averaged_state_dict(), sd, "average after applied()")
    # training mode: batch statistics, and the running statistics of the average move as the twin's do
    prev, taken = trunk.ENABLED, []
    try:
        for enabled in (True, False):
            trunk.set_enabled(enabled)
            with avg.applied():
                got, path = _train_logits(step)
            want, twin_path = _train_logits(twin_step)
            assert path == twin_path and (enabled or path != "_TrunkFnBackward")
            taken.append(path)
            assert torch.equal(_bits(got), _bits(want)), f"executor {enabled}"
    finally:
        trunk.set_enabled(prev)
    assert taken[0] == "_TrunkFnBackward"                          # both paths exist for these models
    floats = lambda sd: {k: v.cpu() for k, v in sd.items() if v.is_floating_point()}    # the counters are the live ones
    _assert_same_state(floats(avg.averaged_state_dict()), floats(twin.state_dict()),
                       "the average after two training-mode passes inside applied()")


@pytest.mark.parametrize("precision", [None, "bf16"])
def test_steps_after_applied_match_a_run_that_never_entered_it(precision):
    """the cache rule: transposed kernels, bf16 packs and the executor's pointers are those of the live weights again"""
    a, b = _trained("MinkUNet34", precision), _trained("MinkUNet34", precision)
    _assert_same_state(a[0].state_dict(), b[0].state_dict(), "the two runs before applied()")
    model, step, avg = a
    inside = None
    with avg.applied():
        inside = _eval_logits(model, precision)
    assert not torch.equal(inside, _eval_logits(model, precision))
    _assert_same_state(a[0].state_dict(), b[0].state_dict(), "live state after applied()")
    for s in range(3):
        outs = [run[1].training_step(_batch()) for run in (a, b)]
        assert torch.equal(_bits(outs[0]["loss"]), _bits(outs[1]["loss"])), f"loss of step {s} after applied()"
        assert a[1].last_path == b[1].last_path
        for run in (a, b):
            run[2].update()
    _assert_same_state(a[0].state_dict(), b[0].state_dict(), "live state three steps after applied()")
    _assert_same_state(a[2].averaged_state_dict(), b[2].averaged_state_dict(), "average three steps after applied()")


def test_applied_needs_an_update_first():
    from lidog_amd.optim import FlatAdam, WeightAverage
    import lidog_amd.me as ME
    bn = ME.MinkowskiBatchNorm(8).cuda()
    avg = WeightAverage(FlatAdam(bn, lr=1e-3), bn, "swa")
    with pytest.raises(RuntimeError, match="first update"):
        with avg.applied():
            pass


# ------------------------------------------------------------------ 4. update_bn
def test_update_bn_re_estimates_the_averaged_statistics_only():
    """one MinkowskiBatchNorm, 3 batches: batch k moves the statistics with momentum 1 / k (torch's cumulative average).
    update_bn over the first k batches starts from (0, 1) every time, so the result over k - 1 batches is the float32
    state batch k started from, and each step is held to sparse_ref's bound for ONE running-statistics update."""
    import lidog_amd.me as ME
    from lidog_amd.optim import FlatAdam, WeightAverage
    C, EPS = 24, 1e-5
    g = torch.Generator().manual_seed(7)
    module = ME.MinkowskiBatchNorm(C, eps=EPS, momentum=0.1).cuda().train()
    bn = module.bn
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        bn.num_batches_tracked.fill_(41)
    avg = WeightAverage(FlatAdam(module, lr=1e-3), module, "swa")
    avg.update()
    with torch.no_grad():                                         # the live statistics move on after the copy
        bn.running_mean.add_(0.25)
        bn.running_var.mul_(1.5)
    live = {k: v.detach().clone() for k, v in module.state_dict().items()}
    batches = [(torch.randn(n, C, generator=g) * (1 + k) + 0.3 * k).cuda() for k, n in enumerate((257, 1000, 63))]
    module.eval()
    rm0, rv0 = torch.zeros(C), torch.ones(C)
    for k in range(1, 4):
        avg.update_bn(batches[:k], lambda x: ME.batch_norm(x, bn))
        assert not module.training and not bn.training and bn.momentum == 0.1
        _assert_same_state(module.state_dict(), live, f"live state after update_bn over {k} batches")
        sd = avg.averaged_state_dict()
        rm, rv = sd["bn.running_mean"], sd["bn.running_var"]
        x = batches[k - 1].cpu()
        n = x.shape[0]
        s1, s2, _, s1_abs = SR.bn_sums64(x.double())
        m64, var64, _, d_mean, d_var, _ = SR.stats_bounds(s1, s2, s1_abs, n, EPS)
        rm64, rv64 = SR.running64(rm0.double(), rv0.double(), m64, var64, n, 1.0 / k)
        r = SR.assert_running(rm, rv, rm64, rv64, rm0, rv0, 1.0 / k, d_mean, d_var * n / (n - 1), f"batch {k}")
        print(f"update_bn batch {k}: worst ratios to the bound {r}")
        rm0, rv0 = rm.clone(), rv.clone()
    assert int(avg.averaged_state_dict()["bn.num_batches_tracked"]) == 41
