"""Test-time adaptation on the GPU (lidog_amd.adapt): every mode of TestTimeAdapter against its hand composition from
the library's own pieces, bit for bit where the composition is the definition; AdaBN's running statistics against the
mean of the per-batch statistics within a derived bound; reset(); the refusals; TargetEvaluator(adapter=...); and
eval_target --adapt end to end.  MinkUNet34 and MinkUNet34IBN, randomly initialised, with the BatchNorm running
statistics moved away from (0, 1); SynthScans(4, "source8k") in batches of 2."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = ["MinkUNet34", "MinkUNet34IBN"]


@functools.lru_cache(maxsize=None)
def _batches(n=4, first=0):
    from lidog_amd import evaluate
    from lidog_amd.train import SynthScans
    return tuple(evaluate.dataset_batches(SynthScans(n, "source8k", first=first), 2))


def _model(kind, seed=5):
    from lidog_amd import adapt
    from lidog_amd.train import build_model
    torch.manual_seed(seed)
    model = build_model(kind)
    g = torch.Generator().manual_seed(seed + 1)
    for bn in adapt.batch_norms(model):
        bn.running_mean.copy_(torch.randn(bn.num_features, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(bn.num_features, generator=g) + 0.5)
    return model.eval()


def _twin(model, kind):
    from lidog_amd.train import build_model
    twin = build_model(kind)
    twin.load_state_dict(model.state_dict())
    return twin.eval()


def _bytes(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _same_state(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not torch.equal(_bytes(a[k]), _bytes(b[k]))]


def _train_forward(model, b):
    """the hand-written adapting forward: training mode, batch statistics, running statistics frozen"""
    import lidog_amd.me as ME
    st = ME.SparseTensor(coordinates=b["coords_int"], features=b["source_features0"])
    model.train()
    try:
        with ME.frozen_running_stats():
            return model(st)
    finally:
        model.eval()


def _call(adapter, batches, i):
    b = batches[i][0]
    nxt = batches[i + 1][0]["coords_int"] if i + 1 < len(batches) else None
    return adapter(b["coords_int"], b["source_features0"], nxt)


# ------------------------------------------------------------------ bn
@pytest.mark.parametrize("kind", KINDS)
def test_bn_equals_the_hand_written_forward_and_changes_nothing(kind):
    from lidog_amd import adapt
    model = _model(kind)
    before = _state(model)
    adapter = adapt.TestTimeAdapter(model, "bn")
    batches = _batches()
    for i, (b, _) in enumerate(batches):
        preds, logits = _call(adapter, batches, i)
        with torch.no_grad():
            want = _train_forward(model, b).F
        assert logits.shape == (b["coords_int"].shape[0], 7) and not logits.requires_grad
        assert torch.equal(_bytes(logits), _bytes(want)), i
        assert torch.equal(preds, want.max(dim=1)[1]) and adapter.output.F is logits
        with torch.no_grad():                                    # and they are not the evaluation-mode logits
            assert not torch.equal(logits, model(_sparse(b)).F)
    assert _same_state(before, _state(model)) == [] and not model.training
    assert all(p.requires_grad for p in model.parameters())


def _sparse(b):
    import lidog_amd.me as ME
    return ME.SparseTensor(coordinates=b["coords_int"], features=b["source_features0"])


# ------------------------------------------------------------------ adabn
@pytest.mark.parametrize("kind", KINDS)
def test_adabn_running_statistics_are_the_mean_of_the_batch_statistics(kind):
    from lidog_amd import adapt, evaluate
    model = _model(kind)
    batches = _batches()
    K = len(batches)
    assert K == 2
    bns = adapt.batch_norms(model)
    # each batch alone from a reset with momentum 1.0: running statistics = that batch's mean and unbiased variance
    probe = _twin(model, kind)
    pbns = adapt.batch_norms(probe)
    means, variances = [], []
    for b, _ in batches:
        for bn in pbns:
            bn.running_mean.zero_()
            bn.running_var.fill_(1.0)
            bn.momentum = 1.0
        probe.train()
        with torch.no_grad():
            probe(_sparse(b))
        probe.eval()
        means.append([bn.running_mean.double().cpu() for bn in pbns])
        variances.append([bn.running_var.double().cpu() for bn in pbns])
    momenta = [bn.momentum for bn in bns]
    bns[3].momentum = 0.25                                       # the modules' own momenta, whatever they are, return
    momenta[3] = 0.25
    adapter = adapt.TestTimeAdapter(model, "adabn")
    with pytest.raises(RuntimeError, match="estimate"):
        _call(adapter, batches, 0)
    assert adapter.estimate(batches) == K
    assert [bn.momentum for bn in bns] == momenta and not model.training
    worst = 0.0
    for j, bn in enumerate(bns):
        for got, per_batch in ((bn.running_mean, means), (bn.running_var, variances)):
            stack = torch.stack([per_batch[k][j] for k in range(K)])
            # each of the K updates makes at most three fp32 roundings on values no larger than max_k |.|
            bound = 4 * K * 2.0 ** -24 * stack.abs().max(dim=0)[0]
            err = (got.double().cpu() - stack.mean(dim=0)).abs()
            worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
            assert (err <= bound).all(), j
    print(f"adabn {kind}: worst error {worst:.3g} x the bound")
    assert all(int(v) == K for k, v in model.state_dict().items() if k.endswith("num_batches_tracked"))
    # after estimate a call is the plain evaluation forward
    plain = evaluate.Predictor(_twin(model, kind))
    for i, (b, _) in enumerate(batches):
        preds, logits = _call(adapter, batches, i)
        want_preds, want = _call(plain, batches, i)
        assert torch.equal(_bytes(logits), _bytes(want)) and torch.equal(preds, want_preds)
        assert adapter.output.F is logits


# ------------------------------------------------------------------ tent
def _hand_tent(model, lr=1e-3):
    """(optimiser, criterion) of the hand composition: FlatAdam over norm_parameters only"""
    from lidog_amd import adapt
    from lidog_amd.losses import EntropyLoss
    from lidog_amd.optim import FlatAdam
    keep = {id(p) for p in adapt.norm_parameters(model)}
    for p in model.parameters():
        p.requires_grad_(id(p) in keep)
    return FlatAdam(model, lr=lr, weight_decay=0.0), EntropyLoss()


@pytest.mark.parametrize("kind", KINDS)
def test_tent_step_equals_its_hand_composition(kind):
    from lidog_amd import adapt
    model = _model(kind)
    hand = _twin(model, kind)
    before = _state(model)
    adapter = adapt.TestTimeAdapter(model, "tent")
    opt, crit = _hand_tent(hand)
    batches = _batches()
    for i, (b, _) in enumerate(batches):
        preds, logits = _call(adapter, batches, i)
        opt.zero_grad()
        out = _train_forward(hand, b)
        loss = crit(out.F)
        loss.backward()
        opt.step()
        assert torch.equal(_bytes(logits), _bytes(out.F)), i     # the first forward's: before this batch's update
        assert not logits.requires_grad and torch.equal(preds, out.F.max(dim=1)[1])
        assert torch.equal(_bytes(adapter.criterion.row_entropy), _bytes(crit.row_entropy))
        assert _same_state(_state(model), _state(hand)) == [], i
        assert float(adapter.criterion.taken) == b["coords_int"].shape[0]
    after = _state(model)
    norm = {id(p) for p in adapt.norm_parameters(model)}
    norm_names = {n for n, p in model.named_parameters() if id(p) in norm}
    changed = set(_same_state(before, after))
    assert changed and changed <= norm_names                     # running statistics and counters among the unchanged
    for n, p in model.named_parameters():
        if id(p) not in norm:
            assert p.grad is None and not p.requires_grad, n
    assert not model.training


@pytest.mark.parametrize("kind", KINDS)
def test_tent_with_zero_learning_rate_returns_the_bn_logits(kind):
    from lidog_amd import adapt
    model = _model(kind)
    tent = adapt.TestTimeAdapter(model, "tent", lr=0.0)
    bn = adapt.TestTimeAdapter(_twin(model, kind), "bn")
    batches = _batches()
    for i in range(len(batches)):
        _, a = _call(tent, batches, i)
        _, b = _call(bn, batches, i)
        assert torch.equal(_bytes(a), _bytes(b)), i


@pytest.mark.parametrize("optimizer", ["Adam", "SGD"])
def test_reset_restores_every_byte(optimizer):
    from lidog_amd import adapt
    model = _model("MinkUNet34IBN")
    adapter = adapt.TestTimeAdapter(model, "tent", optimizer=optimizer, steps=2)
    before = _state(model)
    opt_before = {k: getattr(adapter.opt, k).clone() for k in adapter.opt._state}
    batches = _batches()
    _, first = _call(adapter, batches, 0)
    assert _same_state(before, _state(model)) != [] and adapter.opt.steps == 2
    assert any(not torch.equal(_bytes(getattr(adapter.opt, k)), _bytes(v)) for k, v in opt_before.items())
    adapter.reset()
    assert _same_state(before, _state(model)) == [] and adapter.opt.steps == 0
    for k, v in opt_before.items():
        assert torch.equal(_bytes(getattr(adapter.opt, k)), _bytes(v)), k
    _, again = _call(adapter, batches, 0)                        # and the same batch gives the same logits again
    assert torch.equal(_bytes(first), _bytes(again))


@pytest.mark.parametrize("kind", KINDS)
def test_tent_lowers_the_entropy_of_the_batch_it_steps_on(kind):
    from lidog_amd import adapt
    from lidog_amd.losses import EntropyLoss
    model = _model(kind)
    adapter = adapt.TestTimeAdapter(model, "tent")              # the default learning rate
    b = _batches()[0][0]
    crit = EntropyLoss()
    entropies = []
    for _ in range(4):                                           # three steps; the fourth forward sees their effect
        _, logits = adapter(b["coords_int"], b["source_features0"])
        crit(logits)
        entropies.append(float(crit.row_entropy.double().mean()))
    print(f"tent {kind}: mean row entropy per forward {entropies}")
    assert entropies[3] < entropies[0]


def test_refusals():
    from lidog_amd import adapt, evaluate
    model = _model("MinkUNet34")
    for mode in adapt.MODES:
        with pytest.raises(ValueError, match="bf16"):
            evaluate.TargetEvaluator(model, precision="bf16", adapter=adapt.TestTimeAdapter(model, mode))
    adapter = adapt.TestTimeAdapter(model, "tent")
    b = _batches()[0][0]
    with pytest.raises(ValueError, match="rows"):
        adapter(b["coords_int"][:1].contiguous(), b["source_features0"][:1].contiguous())


# ------------------------------------------------------------------ TargetEvaluator
@pytest.mark.parametrize("mode", ["bn", "tent"])
def test_target_evaluator_counts_are_those_of_the_adapters_logits(mode):
    from lidog_amd import adapt, evaluate
    model = _model("MinkUNet34")
    twin = _twin(model, "MinkUNet34")
    batches = _batches(3)
    assert [len(ids) for _, ids in batches] == [2, 1]
    res = evaluate.TargetEvaluator(model, adapter=adapt.TestTimeAdapter(model, mode)).run(batches, 3, rows="scan")
    direct = adapt.TestTimeAdapter(twin, mode)
    counts = torch.zeros((3, 8, 7), dtype=torch.int64, device="cuda")
    done = 0
    for i, (b, ids) in enumerate(batches):
        _, logits = _call(direct, batches, i)
        evaluate.confusion(logits, b["source_sem_labels0"], b["coords_int"], len(ids), out=counts[done:done + len(ids)])
        done += len(ids)
    assert np.array_equal(res["counts"], counts.cpu().numpy()) and res["scans"] == 3
    assert int(res["counts"].sum()) == sum(b["coords_int"].shape[0] for b, _ in batches)


def test_target_evaluator_without_adapter_is_the_existing_path():
    from lidog_amd import evaluate
    model = _model("MinkUNet34")
    batches = _batches(3)
    res = evaluate.TargetEvaluator(model, adapter=None).run(batches, 3, rows="scan")
    old = evaluate.TargetEvaluator(model).run(batches, 3, rows="scan")
    run = evaluate.Predictor(model)
    counts = torch.zeros((3, 8, 7), dtype=torch.int64, device="cuda")
    done = 0
    for i, (b, ids) in enumerate(batches):
        _, logits = _call(run, batches, i)
        evaluate.confusion(logits, b["source_sem_labels0"], b["coords_int"], len(ids), out=counts[done:done + len(ids)])
        done += len(ids)
    assert np.array_equal(res["counts"], old["counts"]) and np.array_equal(res["counts"], counts.cpu().numpy())
    assert np.array_equal(res["rows"], old["rows"]) and res["mean"] == old["mean"]


# ------------------------------------------------------------------ eval_target --adapt
def test_eval_target_adapt_tent_end_to_end(tmp_path, capsys):
    from lidog_amd import adapt, eval_target, evaluate, synth
    from lidog_amd.train import SynthScans
    model = _model("MinkUNet34")
    run = str(tmp_path / "run")
    os.makedirs(os.path.join(run, "checkpoints"))
    ckpt = os.path.join(run, "checkpoints", "weights.ckpt")
    torch.save({"model." + k: v.cpu() for k, v in model.state_dict().items()}, ckpt)
    common = ["--checkpoint", ckpt, "--model", "MinkUNet34", "--sources", "source8k", "--adapt", "tent", "--scans", "2",
              "--batch", "2"]
    capsys.readouterr()
    one = eval_target.main(common + ["--targets", "source8k"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and (lines[0]["adapt"], lines[0]["adapt_lr"], lines[0]["adapt_steps"]) == ("tent", 1e-3, 1)
    assert os.listdir(os.path.join(run, "results")) == ["source8k-TO-source8k-adapt-tent.csv"]
    assert one[0]["csv"].endswith("source8k-TO-source8k-adapt-tent.csv") and one[0]["scans"] == 2
    # two targets: each gets what it gets alone (the adapter is reset per target)
    two = eval_target.main(common + ["--targets", "source8k", "nusc35k"])
    assert sorted(os.listdir(os.path.join(run, "results"))) == ["source8k-TO-source8k-adapt-tent.csv",
                                                               "source8k-TO-source8knusc35k-adapt-tent.csv"]
    assert np.array_equal(two[0]["counts"], one[0]["counts"])
    for t, config in enumerate(("source8k", "nusc35k")):
        alone = _twin(model, "MinkUNet34")
        data = SynthScans(2, config, first=10 ** 6 + t * synth.SOURCE1_SEED)
        res = evaluate.TargetEvaluator(alone, adapter=adapt.TestTimeAdapter(alone, "tent")).run(
            evaluate.dataset_batches(data, 2), 2)
        assert np.array_equal(two[t]["counts"], res["counts"]), config
    # and the adaptation is not a no-op: the plain evaluation counts differ
    plain = evaluate.TargetEvaluator(model).run(
        evaluate.dataset_batches(SynthScans(2, "source8k", first=10 ** 6), 2), 2)
    assert not np.array_equal(plain["counts"], one[0]["counts"])
