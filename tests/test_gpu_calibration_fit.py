"""lidog_calib_fit_step (csrc/calib.hip) through the C ABI: 24 launches queued back to back against the float64
restatement of the same 24 updates and against the root the long-double restatement finds (tests/calibration_ref.py), every
buffer between guard bands with a band check after the launches.

The final beta has no fixed bar: the float64 restatement of the same updates has its own distance from the long-double
root, and the kernel may be at most 4 x that, with a floor of 1e-12 relative."""
import math

import numpy as np
import pytest
import torch

import calibration_ref as R
from guard import GuardArena

pytestmark = pytest.mark.gpu

ITERS = 24
BETA_MIN, BETA_MAX = 0.01, 100.0
FACTOR, FLOOR = 4.0, 1e-12
CASES = [(1, 2, 1.0), (257, 7, 0.4), (257, 20, 3.0), (70001, 2, 3.0), (70001, 7, 1.0), (70001, 20, 0.4)]


def sampled(n, C, k, seed):
    """logits k u with u ~ N(0, 2^2) and labels drawn from softmax(u): the optimum lies near beta = 1 / k.  From 257
    rows on a few rows are unlabelled (-1, C) and do not count."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, C)) * 2.0
    e = np.exp(u - u.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    labels = (rng.random(n)[:, None] > np.cumsum(p, axis=1)).sum(axis=1).clip(0, C - 1).astype(np.int64)
    if n >= 257:
        labels[5:9], labels[9:12] = -1, C
    return (k * u).astype(np.float32), labels


def run_fit(x, labels, iters=ITERS, arena=None):
    """(state [8], trace [iters, 3], err) on the host after lidog_calib_fit_init and `iters` launches"""
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    arena = arena or GuardArena()
    n, C = x.shape
    xd, ld = arena.place(torch.from_numpy(x), "logits"), arena.place(torch.from_numpy(labels), "labels")
    state = arena.nan(8, dtype=torch.float64, name="state")
    trace = arena.nan(iters, 3, dtype=torch.float64, name="trace")
    err = arena.full(1, 0, dtype=torch.int32, name="err")
    ws = arena.full(int(_lib.load().lidog_calib_ws(n)), 0.0, dtype=torch.float64, name="ws")
    call("lidog_calib_fit_init", ptr(state), BETA_MIN, BETA_MAX)
    for i in range(iters):                                        # nothing is read back in between
        call("lidog_calib_fit_step", ptr(xd), ptr(ld), n, C, -1, BETA_MIN, BETA_MAX, ptr(state), trace[i].data_ptr(),
             ptr(err), ptr(ws))
    arena.check("lidog_calib_fit_step")
    assert int(ws[:1].view(torch.int64)) == 0
    return state.cpu().numpy(), trace.cpu().numpy(), int(err)


def check_fit(x, labels, what):
    state, trace, err = run_fit(x, labels)
    s = dict(zip(R.STATE, state))
    ref_state, ref_trace = R.fit(x, labels, ITERS, BETA_MIN, BETA_MAX)
    rows = int(R.taking(x, labels)[0].sum())
    assert err == 0 and np.isfinite(state).all() and np.isfinite(trace).all()
    assert s["rows"] == rows and s["iterations"] == ITERS and trace[0, 0] == 1.0
    assert BETA_MIN <= s["lo"] <= s["beta"] <= s["hi"] <= BETA_MAX
    # the NLL at the last evaluated beta is no larger than at beta = 1, up to the summation error of the two means
    # (N terms below 2 |nll| each, added in double)
    slack = 4 * np.finfo(np.float64).eps * max(1.0, abs(trace[0, 1])) * math.sqrt(max(rows, 1))
    assert trace[-1, 1] <= trace[0, 1] + slack
    assert R.fit_sums(x, labels, s["beta"])[0] <= R.fit_sums(x, labels, 1.0)[0] + slack
    root = R.fit_root(x, labels, ref_state["beta"], BETA_MIN, BETA_MAX)
    mine = abs(float(R.LD(s["beta"]) - root)) / float(root)
    refs = abs(float(R.LD(ref_state["beta"]) - root)) / float(root)
    print(f"fit {what}: beta {s['beta']:.17g} (restatement {ref_state['beta']:.17g}, long-double root {float(root):.17g}) "
          f"relative distance kernel {mine:.3g} restatement {refs:.3g}; nll {trace[0, 1]:.6g} -> {trace[-1, 1]:.6g}, "
          f"last g {s['g']:.3g}")
    assert mine <= max(FACTOR * refs, FLOOR), (mine, refs)
    return s, trace, ref_state


@pytest.mark.parametrize("n,C,k", CASES)
def test_fit_against_the_long_double_root(n, C, k):
    x, labels = sampled(n, C, k, 1000 * C + n % 89)
    s, trace, _ = check_fit(x, labels, f"n={n} C={C} k={k}")
    if n >= 70001:
        assert abs(s["beta"] * k - 1) < 0.05                     # the optimum is near 1 / k: the labels come from u


def test_fit_is_deterministic():
    x, labels = sampled(70001, 7, 3.0, 4)
    a, b = run_fit(x, labels), run_fit(x, labels)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_no_labelled_row_leaves_beta_at_one():
    x, _ = sampled(300, 7, 1.0, 5)
    for xs, ls in ((x, np.full(300, -1, dtype=np.int64)), (x[:0], np.zeros(0, dtype=np.int64))):
        state, trace, err = run_fit(xs, ls)
        s = dict(zip(R.STATE, state))
        assert s["beta"] == 1.0 and s["rows"] == 0 and s["iterations"] == ITERS and err == 0
        assert (s["lo"], s["hi"], s["nll"], s["g"], s["h"]) == (BETA_MIN, BETA_MAX, 0.0, 0.0, 0.0)
        assert (trace[:, 0] == 1.0).all() and not trace[:, 1:].any()


def test_one_sign_of_the_gradient_ends_at_the_bound():
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((257, 7)) * 2.0).astype(np.float32)
    # separable: every arg-max is right, the NLL falls all the way
    s, trace, _ = check_fit(x, x.argmax(axis=1).astype(np.int64), "separable")
    assert s["beta"] == s["lo"] == s["hi"] == BETA_MAX and (trace[:, 2] < 0).all()
    # every label wrong with high confidence: driven to beta_min
    hot = x.copy()
    hot[np.arange(257), rng.integers(0, 7, size=257)] += 40.0
    wrong = ((hot.argmax(axis=1) + 1) % 7).astype(np.int64)
    s, trace, _ = check_fit(hot, wrong, "confidently wrong")
    assert s["beta"] == s["lo"] == s["hi"] == BETA_MIN and (trace[:, 2] > 0).all()


def test_nonfinite_rows_are_left_out_and_reported():
    x, labels = sampled(257, 7, 1.0, 7)
    bad = x.copy()
    bad[20, 3], bad[21, 0] = np.nan, np.inf
    labels[20], labels[21] = 1, 2
    state, trace, err = run_fit(bad, labels)
    assert err == 2 and np.isfinite(state).all() and np.isfinite(trace).all()
    ref_state, _ = R.fit(bad, labels, ITERS, BETA_MIN, BETA_MAX)
    assert state[7] == ref_state["rows"] == R.taking(bad, labels)[0].sum()
    assert abs(state[0] - ref_state["beta"]) <= 1e-9 * ref_state["beta"]


@pytest.mark.parametrize("C", [1, 33])
def test_other_class_counts_return_2_before_any_launch(C):
    from lidog_amd import _lib
    from lidog_amd._lib import ptr
    lib, arena = _lib.load(), GuardArena()
    x = arena.place(torch.randn(9, C), "logits")
    labels = arena.place(torch.zeros(9, dtype=torch.int64), "labels")
    state, trace, ws = (arena.nan(8, dtype=torch.float64), arena.nan(3, dtype=torch.float64),
                        arena.nan(5, dtype=torch.float64))
    err = arena.full(1, 0, dtype=torch.int32)
    assert lib.lidog_calib_fit_step(ptr(x), ptr(labels), 9, C, -1, BETA_MIN, BETA_MAX, ptr(state), ptr(trace), ptr(err),
                                    ptr(ws), _lib.stream()) == 2
    arena.check("refused call")
    assert all(torch.isnan(t).all() for t in (state, trace, ws)) and int(err) == 0


def test_fit_temperature_is_the_kernel():
    from lidog_amd.calibration import CalibrationTable, fit_temperature
    x, labels = sampled(70001, 7, 3.0, 8)
    state, trace, _ = run_fit(x, labels)
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
    fit = fit_temperature(xd, ld)
    assert fit.state.cpu().numpy().tobytes() == state.tobytes() and fit.trace().tobytes() == trace.tobytes()
    assert fit.temperature() == 1.0 / state[0] and fit.summary()["rows"] == state[7]
    assert fit.beta.data_ptr() == fit.state.data_ptr() and fit.beta.shape == (1,)
    raw = CalibrationTable().add(xd, ld).result()
    scaled = CalibrationTable().add(xd, ld, beta=fit.beta).result()          # the device word, where it lies
    also = CalibrationTable().add(xd, ld, beta=fit).result()
    assert scaled["nll"] < raw["nll"] and scaled["accuracy"] == raw["accuracy"] and also["nll"] == scaled["nll"]
    assert scaled["ece"] < raw["ece"]                # k = 3: three times too sharp, far outside the binomial spread
    with pytest.raises(ValueError, match="iters"):
        fit_temperature(xd, ld, iters=0)
