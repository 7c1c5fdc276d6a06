"""Weight averaging without a GPU: the numpy float32 restatements (tests/wavg_ref.py) against torch on the CPU bit for bit
and against float64 within a derived bound, the decay schedule, the workgroup layout of the device table, the argument
checks of WeightAverage and of the command lines, the checkpoint keys, and the new entry point of the library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import wavg_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, N = 40, 100003


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _draw(rng, n=N):
    return (rng.standard_normal(n) * 0.3).astype(np.float32)


# ------------------------------------------------------------------ 1. the restatements
def test_ema_restatement_is_torch_bit_for_bit():
    """tau * a + (1 - tau) * p in torch ops on float32 tensors (MomentumUpdater's expression), cosine tau, 40 updates"""
    rng = np.random.default_rng(0)
    a = _draw(rng)
    ta = torch.from_numpy(a.copy())
    for s in range(K):
        p = _draw(rng)
        t = R.tau(s, 0.996, 1.0, K)
        ta = t * ta + (1 - t) * torch.from_numpy(p)
        a = R.ema_step(a, p, t)
        assert np.array_equal(_bits(ta.numpy()), _bits(a)), s


def test_swa_restatement_is_torch_bit_for_bit():
    """a + (p - a) / (n + 1) in torch ops, and torch.optim.swa_utils.AveragedModel itself"""
    from torch.optim.swa_utils import AveragedModel
    rng = np.random.default_rng(1)
    m = torch.nn.Linear(1, 1, bias=False)
    m.weight = torch.nn.Parameter(torch.zeros(N))
    averaged = AveragedModel(m)
    a = ta = None
    for s in range(K):
        p = _draw(rng)
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(p))
        averaged.update_parameters(m)
        tp = torch.from_numpy(p)
        ta = tp.clone() if s == 0 else ta + (tp - ta) / (s + 1)
        a = R.update(a, p, s, "swa")
        assert np.array_equal(_bits(ta.numpy()), _bits(a)), s
        assert np.array_equal(_bits(averaged.module.weight.detach().numpy()), _bits(a)), s


@pytest.mark.parametrize("mode", ["ema", "swa"])
def test_restatement_stays_within_one_rounding_per_operation_of_float64(mode):
    """The same recurrence in float64 (with the float32 coefficients): after K updates the two differ by at most
    K * 2 * 2^-24 * M, M = max(|a|, |p|).  One rounding adds at most 2^-24 times its result.  EMA rounds c0 a and c1 p,
    whose magnitudes sum to at most M, and their sum, at most M: 2 * 2^-24 M per update.  SWA after n updates rounds
    p - a (at most 2 M, divided by n + 1 afterwards), the quotient (at most 2 M / (n + 1)) and the sum (at most M):
    (1 + 4 / (n + 1)) * 2^-24 M, which is 52 * 2^-24 M summed over n = 1 .. 39, below the 80 of the bound.  Earlier error
    is carried with weights that sum to one (both forms are convex combinations), so it is never amplified."""
    rng = np.random.default_rng(2)
    a32 = a64 = None
    M = 0.0
    for s in range(K):
        p = _draw(rng)
        M = max(M, float(np.abs(p).max()))
        a32 = R.update(a32, p, s, mode, 0.9, 0.999, K)
        if s == 0:
            a64 = p.astype(np.float64)
        elif mode == "ema":
            t = R.tau(s, 0.9, 0.999, K)
            a64 = float(np.float32(t)) * a64 + float(np.float32(1.0 - t)) * p.astype(np.float64)
        else:
            a64 = a64 + (p.astype(np.float64) - a64) / (s + 1)
    err = float(np.abs(a32.astype(np.float64) - a64).max())
    bound = K * 2 * 2.0 ** -24 * M
    print(f"{mode}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_tau_sequence():
    S = 10
    assert R.tau(0, 0.99, 1.0, S) == 0.99
    assert R.tau(S // 2, 0.99, 1.0, S) == pytest.approx(0.995, abs=1e-15)
    assert R.tau(S, 0.99, 1.0, S) == 1.0
    assert R.tau(7, 0.99) == 0.99
    from lidog_amd.optim import WeightAverage
    w = WeightAverage.__new__(WeightAverage)
    w.decay, w.final_decay, w.total_steps, w.mode = 0.99, 1.0, S, "ema"
    for s in range(S + 1):
        assert w.tau(s) == R.tau(s, 0.99, 1.0, S)
    assert w.tau(S + 5) == 1.0                                  # the schedule ends at final_decay and stays there
    assert w.coefficients(0) == (0, 0.0, 0.0)
    t = R.tau(3, 0.99, 1.0, S)
    assert w.coefficients(3) == (1, t, 1.0 - t)
    w.mode = "swa"
    assert w.coefficients(3) == (2, 4.0, 0.0)


# ------------------------------------------------------------------ 2. the table
def test_table_layout_and_workgroup_shares():
    from lidog_amd.optim import WAVG_BLOCK_ELEMS, WAVG_MAX_BLOCKS, wavg_table
    base = 1 << 20
    sizes = [7, 0, 38_000_000, 64, 1025, 0]
    triples, at = [], base
    for n in sizes:
        triples.append((at, at + 4 * n, n))
        at += 8 * n + 64
    table, blocks = wavg_table(triples)
    S = len(sizes)
    assert table.dtype == np.int64 and table.shape == (4 * S + 1,)
    assert table[:3 * S].reshape(S, 3).tolist() == [list(t) for t in triples]
    block0 = table[3 * S:]
    assert block0[0] == 0 and block0[-1] == blocks and (np.diff(block0) >= 0).all()
    per = np.diff(block0)
    for n, nb in zip(sizes, per):
        assert (nb == 0) == (n == 0)
        assert nb <= -(-n // WAVG_BLOCK_ELEMS)                   # never a workgroup without a sweep of its own
    assert per[0] == 1 and per[3] == 1 and per[4] == 1 and WAVG_MAX_BLOCKS - 8 <= per[2] <= WAVG_MAX_BLOCKS
    assert blocks <= WAVG_MAX_BLOCKS + S
    assert wavg_table([])[1] == 0 and wavg_table([(0, 0, 0)])[1] == 0


@pytest.mark.parametrize("triples,what", [
    ([(4096, 8192, -1)], "elements"),
    ([(0, 8192, 4)], "addresses"),
    ([(4098, 8192, 4)], "addresses"),
    ([(4096, 4100, 4)], "overlap"),                              # live and average of one segment
    ([(4096, 8192, 4), (4104, 16384, 4)], "overlap"),            # two live ranges
    ([(4096, 8192, 4), (16384, 8200, 4)], "overlap"),            # two averages
])
def test_malformed_tables_are_refused_where_they_are_built(triples, what):
    from lidog_amd.optim import wavg_table
    with pytest.raises(ValueError, match=what):
        wavg_table(triples)


# ------------------------------------------------------------------ 3. arguments
@pytest.mark.parametrize("kw", [dict(mode="mean"), dict(decay=-0.1), dict(decay=1.5), dict(decay=float("nan")),
                                dict(decay=0.99, final_decay=0.9), dict(decay=0.99, final_decay=1.1),
                                dict(decay=0.99, final_decay=1.0), dict(decay=0.99, final_decay=1.0, total_steps=0)])
def test_weight_average_argument_errors(kw):
    from lidog_amd.optim import WeightAverage
    with pytest.raises(ValueError):
        WeightAverage(None, None, **kw)          # refused before the optimiser or the model is looked at


def test_weight_average_accepts_the_edges():
    from lidog_amd.optim import WeightAverage
    for kw in (dict(mode="ema", decay=0.0), dict(mode="ema", decay=1.0), dict(mode="swa"),
               dict(mode="ema", decay=0.5, final_decay=0.5, total_steps=1)):
        WeightAverage.check_arguments(**kw)


@pytest.mark.parametrize("argv", [["--avg-decay", "0.9"], ["--avg-decay-final", "1.0"], ["--avg-start-epoch", "1"],
                                  ["--weight-average", "mean"], ["--weight-average", "ema", "--avg-decay", "1.5"],
                                  ["--weight-average", "ema", "--avg-decay", "-0.5"],
                                  ["--weight-average", "ema", "--avg-decay", "0.99", "--avg-decay-final", "0.9"],
                                  ["--weight-average", "ema", "--avg-decay-final", "1.5"],
                                  ["--weight-average", "swa", "--epochs", "3", "--avg-start-epoch", "3"],
                                  ["--weight-average", "swa", "--avg-start-epoch", "-1"]])
def test_train_command_line_errors(argv, capsys):
    from lidog_amd.train import parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2
    assert "avg" in capsys.readouterr().err or "weight-average" in argv


def test_train_command_line_values():
    from lidog_amd.train import parse_args, weight_average_of
    assert weight_average_of(parse_args([])) == dict(weight_average=None, avg_decay=0.996, avg_decay_final=None,
                                                     avg_start_epoch=0)
    a = parse_args(["--weight-average", "ema", "--avg-decay", "0.99", "--avg-decay-final", "1.0", "--avg-start-epoch", "2",
                    "--model", "MinkUNet34", "--mix", "cosmix", "--precision", "bf16"])
    assert weight_average_of(a) == dict(weight_average="ema", avg_decay=0.99, avg_decay_final=1.0, avg_start_epoch=2)
    assert weight_average_of(parse_args(["--weight-average", "swa"]))["weight_average"] == "swa"


def test_eval_target_command_line():
    from lidog_amd.eval_target import parse_args
    assert parse_args(["--checkpoint", "x.ckpt"]).weights == "live"
    assert parse_args(["--checkpoint", "x.ckpt", "--weights", "averaged"]).weights == "averaged"
    with pytest.raises(SystemExit):
        parse_args(["--checkpoint", "x.ckpt", "--weights", "ema"])


# ------------------------------------------------------------------ 4. checkpoints
def test_model_state_dict_which():
    from lidog_amd.checkpoint import model_state_dict
    live, avg = {"model.w": torch.zeros(2)}, {"model.w": torch.ones(2)}
    ckpt = {"state_dict": live, "averaged_state_dict": avg, "weight_average": {"mode": "ema"}}
    assert torch.equal(model_state_dict(ckpt)["w"], live["model.w"])
    assert torch.equal(model_state_dict(ckpt, which="live")["w"], live["model.w"])
    assert list(model_state_dict(ckpt, which="averaged")) == ["w"]
    assert torch.equal(model_state_dict(ckpt, which="averaged")["w"], avg["model.w"])
    with pytest.raises(KeyError) as e:
        model_state_dict({"state_dict": live}, which="averaged")
    assert "averaged_state_dict" in str(e.value) and "--weight-average" in str(e.value)
    with pytest.raises(ValueError):
        model_state_dict(ckpt, which="both")


class _Average:
    """what save_lightning_checkpoint reads of a WeightAverage"""

    def __init__(self, model, num_updates):
        self.num_updates = num_updates
        self.sd = {k: torch.full_like(v, 0.5) if v.is_floating_point() else v.clone()
                   for k, v in model.state_dict().items()}

    def averaged_state_dict(self):
        return self.sd

    def state_dict(self):
        return {"mode": "ema", "decay": 0.996, "final_decay": None, "total_steps": None,
                "num_updates": self.num_updates}


def test_checkpoint_key_layout(tmp_path):
    from lidog_amd.checkpoint import model_state_dict, save_lightning_checkpoint
    model = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    plain, with_avg, early = (str(tmp_path / n) for n in ("plain.ckpt", "avg.ckpt", "early.ckpt"))
    save_lightning_checkpoint(model, plain, epoch=1, global_step=5)
    save_lightning_checkpoint(model, with_avg, epoch=1, global_step=5, weight_average=_Average(model, 5))
    save_lightning_checkpoint(model, early, epoch=1, global_step=5, weight_average=_Average(model, 0))
    a, b, c = (torch.load(p, weights_only=False) for p in (plain, with_avg, early))
    assert set(b) - set(a) == {"averaged_state_dict", "weight_average"}
    assert set(c) == set(a)                                      # nothing was averaged yet: nothing is stored
    assert list(b["averaged_state_dict"]) == list(b["state_dict"])
    assert all(k.startswith("model.") for k in b["averaged_state_dict"])
    assert b["weight_average"] == _Average(model, 5).state_dict()
    for k, v in a["state_dict"].items():                         # the live part is what it always was
        assert torch.equal(v, b["state_dict"][k])
    avg = model_state_dict(b, which="averaged")
    assert torch.equal(avg["0.weight"], torch.full((2, 3), 0.5))
    assert avg["1.num_batches_tracked"].dtype == torch.int64


# ------------------------------------------------------------------ 5. the library
def test_entry_point_is_declared_exported_and_typed():
    from lidog_amd import _lib
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    assert re.search(r"int lidog_wavg_apply\(const int64_t \*table, int32_t n_segs, int64_t n_blocks, int32_t mode, "
                     r"float c0, float c1,\s+void \*stream\);", header)
    assert _lib.SIGNATURES["lidog_wavg_apply"] == [_lib._p, _lib._i32, _lib._i64, _lib._i32, _lib._f, _lib._f, _lib._p]
    for c, name in enumerate(("COPY", "EMA", "SWA", "SWAP")):
        assert re.search(rf"^#define LIDOG_WAVG_{name} {c}\b", header, re.M)
    from lidog_amd import optim
    assert (optim.WAVG_COPY, optim.WAVG_EMA, optim.WAVG_SWA, optim.WAVG_SWAP) == (0, 1, 2, 3)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True)
    assert "lidog_wavg_apply" in set(re.findall(r"\bT (lidog_[a-z0-9_]+)", exported.stdout))
    assert "wavg.hip" in __import__("lidog_amd.build", fromlist=["SOURCES"]).SOURCES
    assert _lib.ABI_VERSION == 9                                 # an additive entry: the version stays


def test_entry_point_returns_before_any_launch():
    from lidog_amd import _lib
    L = _lib.load()
    one = ctypes.c_void_p(64)                # never dereferenced: every call below returns from its checks
    assert L.lidog_wavg_apply(None, 0, 0, 0, 0.0, 0.0, None) == 0
    assert L.lidog_wavg_apply(one, 0, 5, 1, 0.5, 0.5, None) == 0
    assert L.lidog_wavg_apply(one, 3, 0, 1, 0.5, 0.5, None) == 0
    for args in ((one, -1, 1, 0, 0.0, 0.0), (one, 1, -1, 0, 0.0, 0.0), (one, 1, 1, 4, 0.0, 0.0),
                 (one, 1, 1, -1, 0.0, 0.0), (None, 1, 1, 0, 0.0, 0.0), (one, 1, 2 ** 31, 0, 0.0, 0.0),
                 (one, 1, 1, 2, 0.0, 0.0)):
        assert L.lidog_wavg_apply(*args, None) == 2, args
        assert b"wavg_apply" in L.lidog_last_error()
