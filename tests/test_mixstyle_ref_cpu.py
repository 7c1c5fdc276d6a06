"""MixStyle without a GPU: the float64 restatement of tests/mixstyle_ref.py equals the paper's expressions written per
scan (torch.var(unbiased=True), autograd with detached statistics); lidog_amd.data.draw_mixstyle draws in the stated
order from its own random state; the argument checks and refusals of build_model / build_step / Fit / the parser; and
the bars of mixstyle_ref pass a correct fp32 evaluation and fail five mutants."""
import math
import os

import numpy as np
import pytest
import torch

import inorm_ref as IR
import mixstyle_ref as MR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAY = dict(id="cpu", C=8, sizes=[37, 2, 1, 0, 50, 64, 41], order="shuffled")
LAM = torch.tensor([0.25, 0.0, 0.5, 0.9, 1.0, 0.7, 0.03125], dtype=torch.float32)
PARTNER = torch.tensor([4, 0, 5, 1, 6, 6, 0], dtype=torch.int32)          # not a permutation; 5 and 4 share 6
ROTATION = torch.tensor([4, 0, 1, 2, 5, 6, 3], dtype=torch.int32)         # a permutation that is not its own inverse


# ------------------------------------------------------------------ the restatement against the paper's expressions
def _paper(x, batch, B, lam, partner, eps):
    """MixStyle as the authors' code states it, per scan: mu = x.mean(0), sig = (x.var(0, unbiased) + eps).sqrt(), both
    detached; x_normed = (x - mu) / sig; y = x_normed * sig_mix + mu_mix.  Scans the definition leaves alone stay."""
    y = x.clone()
    stats = {}
    for b in range(B):
        rows = x[batch == b]
        if rows.shape[0] >= 2:
            stats[b] = (rows.mean(0).detach(), (rows.var(0, unbiased=True) + eps).sqrt().detach())
    for b in range(B):
        p, l = int(partner[b]), float(lam[b])
        if b not in stats or p not in stats or p == b or l == 1.0:
            continue
        (mu, sig), (mu_p, sig_p) = stats[b], stats[p]
        mu_mix, sig_mix = l * mu + (1 - l) * mu_p, l * sig + (1 - l) * sig_p
        y[batch == b] = (x[batch == b] - mu) / sig * sig_mix + mu_mix
    return y


@pytest.mark.parametrize("partner", [PARTNER, ROTATION], ids=["shared", "rotation"])
def test_restatement_equals_the_papers_expressions_and_autograd(partner):
    d = IR.make_case(LAY)
    x = d["x"].double().requires_grad_(True)
    y_paper = _paper(x, d["batch"], d["B"], LAM, partner, MR.EPS)
    y_paper.backward(d["dy"].double())
    m = MR.moments64(x.detach(), d["batch"], d["B"])
    sub, scale, add, ident = MR.tables64(m, LAM, partner)
    y, _ = MR.mixstyle_y64(x.detach(), d["batch"], sub, scale, add)
    tol = 1e-12 * (1 + y.abs())
    tol[:, 0] = 1e-9                                          # the channel of mean 1e3: (x - mu) cancels 10 bits more
    assert bool(((y - y_paper.detach()).abs() <= tol).all())
    assert torch.equal(MR.mixstyle64(x.detach(), d["batch"], d["B"], LAM, partner), y)
    dx = d["dy"].double() * scale[d["batch"].long()]          # dx = dy sig_mix / sig: the statistics are constants
    assert bool(((dx - x.grad).abs() <= 1e-12 * (1 + dx.abs())).all())
    rows = ident[d["batch"].long()]
    assert bool(rows.any()) and bool((~rows).any())
    assert torch.equal(y[rows], x.detach()[rows]) and torch.equal(x.grad[rows], d["dy"].double()[rows])
    # the constant channel: var = 0, sig = sqrt(eps) in every scan, scale = 1 exactly
    assert torch.equal(m["sig"][m["cnt"] > 0, 1], torch.full((6,), math.sqrt(MR.EPS), dtype=torch.float64))
    assert torch.equal(scale[:, 1], torch.ones(d["B"], dtype=torch.float64))


def test_unbiased_variance_and_small_scans():
    x = torch.tensor([[1.0, 5.0], [3.0, 5.0], [7.0, 2.0]], dtype=torch.float64)
    batch = torch.tensor([0, 0, 2], dtype=torch.int32)
    m = MR.moments64(x, batch, 3)
    assert m["cnt"].tolist() == [2, 0, 1]
    assert torch.equal(m["mu"], torch.tensor([[2.0, 5.0], [0.0, 0.0], [7.0, 2.0]], dtype=torch.float64))
    assert torch.equal(m["var"], torch.tensor([[2.0, 0.0], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float64))
    lam, partner = torch.tensor([0.5, 0.5, 0.5]), torch.tensor([2, 0, 0], dtype=torch.int32)
    assert MR.identity_scans(m["cnt"], lam, partner).tolist() == [True, True, True]     # every partner or scan < 2 rows


# ------------------------------------------------------------------ the host draws
class _Recorder:
    """a RandomState that notes which draws were asked of it"""

    def __init__(self, seed):
        self.rs, self.calls = np.random.RandomState(seed), []

    def random_sample(self, *a):
        self.calls.append(("random_sample",) + a)
        return self.rs.random_sample(*a)

    def beta(self, *a):
        self.calls.append(("beta",) + a)
        return self.rs.beta(*a)

    def permutation(self, *a):
        self.calls.append(("permutation",) + a)
        return self.rs.permutation(*a)


def test_draw_order_gate_and_reproducibility():
    from lidog_amd.data import draw_mixstyle
    rec = _Recorder(3)
    lam, partner = draw_mixstyle(rec, 5, p=1.0, alpha=0.1)
    assert rec.calls == [("random_sample",), ("beta", 0.1, 0.1, 5), ("permutation", 5)]
    twin = np.random.RandomState(3)
    twin.random_sample()
    assert np.array_equal(lam, twin.beta(0.1, 0.1, 5).astype(np.float32)) and lam.dtype == np.float32
    assert np.array_equal(partner, twin.permutation(5)) and partner.dtype == np.int32
    assert sorted(partner.tolist()) == list(range(5))
    # a failed gate draws nothing more
    rec = _Recorder(3)
    assert draw_mixstyle(rec, 5, p=0.0) is None and rec.calls == [("random_sample",)]
    # the same seed gives the same sequence of draws, gate included
    runs = []
    for _ in range(2):
        rs = np.random.RandomState(11)
        runs.append([draw_mixstyle(rs, 4, p=0.5, alpha=0.1) for _ in range(16)])
    assert any(r is None for r in runs[0]) and any(r is not None for r in runs[0])
    for a, b in zip(*runs):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_modules_own_their_random_state():
    """building a model with MixStyle and drawing from its modules consumes neither numpy's nor torch's global sequence,
    and every module has a sequence of its own"""
    import lidog_amd.train as T
    from lidog_amd.data import draw_mixstyle
    np.random.seed(5)
    torch.manual_seed(5)
    before_np, before_t = np.random.get_state()[1].copy(), torch.get_rng_state().clone()
    torch.manual_seed(5)
    plain = T.build_model("MinkUNet34", device="cpu")
    after_plain = torch.get_rng_state().clone()
    torch.manual_seed(5)
    model = T.build_model("MinkUNet34", device="cpu", mixstyle_layers=("block2", "block1"), mixstyle_seed=1234)
    assert torch.equal(torch.get_rng_state(), after_plain)            # the same draws for the weights
    for (k, v), (k0, v0) in zip(model.state_dict().items(), plain.state_dict().items()):
        assert k == k0 and torch.equal(v, v0)
    mods = model.mixstyle
    assert list(mods.keys()) == ["block1", "block2"] and T.mixstyle_stages_of(model) == ("block1", "block2")
    assert not list(mods.parameters()) and not list(mods.buffers())
    d1 = [draw_mixstyle(mods["block1"].rng, 4, 1.0, 0.1) for _ in range(3)]
    d2 = [draw_mixstyle(mods["block2"].rng, 4, 1.0, 0.1) for _ in range(3)]
    assert not all(np.array_equal(a[0], b[0]) for a, b in zip(d1, d2))
    assert np.array_equal(np.random.get_state()[1], before_np)
    del before_t


# ------------------------------------------------------------------ argument checks and refusals
def test_argument_checks():
    from lidog_amd.data import check_mixstyle_arguments
    assert check_mixstyle_arguments(["block1", "block4"], 0.0, 1e-3) == ("block1", "block4")
    assert check_mixstyle_arguments((), 1.0, 2.0) == ()
    for layers, p, alpha in ((["block5"], 0.5, 0.1), (["block1", "block1"], 0.5, 0.1), (["block1"], -0.1, 0.1),
                             (["block1"], 1.5, 0.1), (["block1"], float("nan"), 0.1), (["block1"], 0.5, 0.0),
                             (["block1"], 0.5, float("inf")), (["block1"], 0.5, float("nan")), (["final"], 0.5, 0.1)):
        with pytest.raises(ValueError):
            check_mixstyle_arguments(layers, p, alpha)


def test_models_take_mixstyle_layers_and_keep_their_keys():
    import lidog_amd.train as T
    for kind in ("MinkUNet34BEV", "MinkUNet34", "MinkUNet34IBN", "MinkUNet34Robust"):
        torch.manual_seed(0)
        plain = T.build_model(kind, device="cpu")
        torch.manual_seed(0)
        model = T.build_model(kind, device="cpu", mixstyle_layers=("block1", "block2"), mixstyle_p=0.3, mixstyle_alpha=0.2)
        assert list(model.state_dict()) == list(plain.state_dict()), kind
        assert [n for n, _ in model.named_parameters()] == [n for n, _ in plain.named_parameters()], kind
        assert T.mixstyle_stages_of(model) == ("block1", "block2") and T.mixstyle_stages_of(plain) == ()
        assert "mixstyle" not in plain._modules
        assert model.mixstyle["block1"].p == 0.3 and model.mixstyle["block2"].alpha == 0.2
        with pytest.raises(ValueError):
            T.build_model(kind, device="cpu", mixstyle_layers=("block8",))


def test_build_step_and_fit_refuse_what_is_not_built():
    import lidog_amd.train as T
    assert T.check_mixstyle(None) == ()
    assert T.check_mixstyle(["block1"], 0.5, 0.1, None, None, 4) == ("block1",)
    with pytest.raises(NotImplementedError, match="bf16"):
        T.check_mixstyle(["block1"], precision="bf16")
    with pytest.raises(NotImplementedError, match="sam_rho"):
        T.check_mixstyle(["block1"], sam_rho=0.05)
    with pytest.raises(ValueError, match="batch of 1"):
        T.check_mixstyle(["block1"], batch_size=1)
    with pytest.raises(ValueError):
        T.check_mixstyle([])
    with pytest.raises(ValueError):
        T.check_mixstyle(["block1"], mixstyle_p=2.0)
    model = T.build_model("MinkUNet34", device="cpu", mixstyle_layers=("block1",))
    with pytest.raises(NotImplementedError, match="bf16"):
        T.build_step(model, "MinkUNet34", precision="bf16")               # the stages come from the model
    with pytest.raises(NotImplementedError, match="sam_rho"):
        T.build_step(model, "MinkUNet34", sam_rho=0.05, mixstyle=["block1"])
    with pytest.raises(ValueError, match="built with"):
        T.build_step(model, "MinkUNet34", mixstyle=["block2"])
    for kw in (dict(precision="bf16"), dict(sam_rho=0.05), dict(batch_size=1), dict(mixstyle_p=-1.0),
               dict(mixstyle_alpha=0.0)):
        with pytest.raises((ValueError, NotImplementedError)):
            T.Fit("MinkUNet34", mixstyle=("block1",), device="cpu", **kw)
    for bad in ((["block7"]), (["block1", "block1"])):
        with pytest.raises(ValueError):
            T.Fit("MinkUNet34", mixstyle=bad, device="cpu")


def test_more_than_one_rank_is_refused(monkeypatch):
    import lidog_amd.train as T
    monkeypatch.setattr(T.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(T.dist, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="2 ranks"):
        T.check_mixstyle(["block1"])
    assert T.check_mixstyle(None) == ()


def test_parser():
    import lidog_amd.train as T
    a = T.parse_args([])
    assert T.mixstyle_of(a) == dict(mixstyle=None, mixstyle_p=0.5, mixstyle_alpha=0.1)
    a = T.parse_args(["--mixstyle"])
    assert T.mixstyle_of(a) == dict(mixstyle=["block1", "block2"], mixstyle_p=0.5, mixstyle_alpha=0.1)
    a = T.parse_args(["--mixstyle", "block3", "block1", "--mixstyle-p", "0.25", "--mixstyle-alpha", "0.3",
                      "--model", "MinkUNet34Robust", "--weight-average", "ema", "--grad-clip-norm", "1.0"])
    assert T.mixstyle_of(a) == dict(mixstyle=["block3", "block1"], mixstyle_p=0.25, mixstyle_alpha=0.3)
    for bad in (["--mixstyle", "block9"], ["--mixstyle", "block1", "block1"], ["--mixstyle", "--batch", "1"],
                ["--mixstyle", "--sam-rho", "0.05"], ["--mixstyle", "--precision", "bf16"], ["--mixstyle-p", "0.2"],
                ["--mixstyle-alpha", "0.2"], ["--mixstyle", "--mixstyle-p", "1.5"],
                ["--mixstyle", "--mixstyle-alpha", "0"], ["--mixstyle", "--mixstyle-alpha", "inf"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)


def test_header_and_sources():
    from lidog_amd import _lib, build
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    for name in ("lidog_mixstyle_ws", "lidog_mixstyle_stats", "lidog_mixstyle_apply", "lidog_mixstyle_bwd"):
        assert name in header
    assert "#define LIDOG_ABI_VERSION 9" in header
    assert "mixstyle.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "mixstyle.hip"))
    argtypes, restypes, _ = _lib.parse_header(header)
    assert len(argtypes["lidog_mixstyle_stats"]) == 16 and "lidog_mixstyle_ws" in restypes


# ------------------------------------------------------------------ the bars: a correct evaluation passes, mutants fail
def _ratios(o, d, lam, partner):
    r = MR.table_ratios(o, d["x"], d["batch"], d["B"], lam, partner)
    ident = MR.identity_scans(torch.bincount(d["batch"].long(), minlength=d["B"]), lam, partner)
    r.update(MR.elem_ratios(o, d["x"], d["dy"], d["batch"], d["B"], ident))
    return r


def test_bars_pass_a_correct_fp32_evaluation():
    for lay in (LAY, dict(id="wide", C=32, sizes=[2500, 2503, 3], order="collated")):
        d = IR.make_case(lay)
        for name, lam, partner in MR.combos(d["B"]) + [("cpu", LAM[:d["B"]], PARTNER[:d["B"]].clamp_max(d["B"] - 1))]:
            o = MR.evaluate32(d["x"], d["dy"], d["batch"], d["B"], lam, partner)
            r = MR.check(o, d, lam, partner, f"{lay['id']} {name}")
            assert max(r.values()) <= 1.0 and r["mean"] > 0


def _fails(o, d, lam, partner, keys):
    r = _ratios(o, d, lam, partner)
    bad = {k for k, v in r.items() if not v <= 1.0}
    assert bad & set(keys), f"the mutant passes the bars of {keys}: {r}"


def test_bars_fail_the_mutants():
    d = IR.make_case(LAY)
    x, dy, batch, B = d["x"], d["dy"], d["batch"], d["B"]
    _fails(MR.evaluate32(x, dy, batch, B, LAM, PARTNER, biased=True), d, LAM, PARTNER, ["sig"])
    _fails(MR.evaluate32(x, dy, batch, B, LAM, PARTNER, swap_lam=True), d, LAM, PARTNER, ["scale", "add"])
    _fails(MR.evaluate32(x, dy, batch, B, LAM, ROTATION, inverse_partner=True), d, LAM, ROTATION, ["scale", "add"])
    # a scan boundary moved by one row: the first row of scan 5 counted to scan 4
    moved = batch.clone()
    moved[(batch == 5).nonzero()[0]] = 4
    o = MR.evaluate32(x, dy, moved, B, LAM, PARTNER)
    _fails(o, d, LAM, PARTNER, ["mean"])
    _fails(o, d, LAM, PARTNER, ["y"])
    # a dropped row: the statistics of scan 0 without its last row (y / dx of every row still written)
    keep = torch.ones(d["n"], dtype=torch.bool)
    keep[(batch == 0).nonzero()[-1]] = False
    part = MR.evaluate32(x[keep], dy[keep], batch[keep], B, LAM, PARTNER)
    o = MR.evaluate32(x, dy, batch, B, LAM, PARTNER)
    o.update({k: part[k] for k in ("mean", "sig", "sub", "scale", "add")})
    _fails(o, d, LAM, PARTNER, ["mean", "sig"])
    # the elementwise bars on their own: one element of y off by 4 ulp, one of dx by 1 ulp, an identity row touched
    good = MR.evaluate32(x, dy, batch, B, LAM, PARTNER)
    row = int((batch == 0).nonzero()[0])
    for key, ulps, fails in (("y", 4, "y"), ("dx", 1, "dx")):
        o = {k: v.clone() for k, v in good.items()}
        v = o[key][row, 3]
        o[key][row, 3] = v + ulps * float(MR.R.ulp32(v.reshape(1))[0]) * (1 if v >= 0 else -1)
        _fails(o, d, LAM, PARTNER, [fails])
    o = {k: v.clone() for k, v in good.items()}
    irow = int((batch == 2).nonzero()[0])                        # scan 2 has one row: an identity scan
    o["y"][irow, 2] = torch.nextafter(o["y"][irow, 2], torch.tensor(math.inf))
    _fails(o, d, LAM, PARTNER, ["identity_rows"])
    o = {k: v.clone() for k, v in good.items()}
    o["scale"].reshape(B, -1)[2, 0] = 1.0 + 2.0 ** -23
    _fails(o, d, LAM, PARTNER, ["identity"])
