"""lidog_calib_stats (csrc/calib.hip) through the C ABI against its float64 restatement (tests/calibration_ref.py), every
buffer between guard bands (tests/guard.py) with a band check after every call.

What is exact: count and correct per bin, rows, the error word.  The inputs are conditioned for that on the CPU before
any kernel runs: no reference confidence lies within 1e-9 of an interior bin edge k / B (rows that do are redrawn, as
test_gpu_entropy.separate_from_margin does; the rows of equal logits, whose confidence is exactly 1 / C, are only
planted where B is no multiple of C).  conf_q of a bin may differ by its count, brier_q by rows: one unit per llrint.
nll_sum has no fixed bar: the float64 restatement's own distance from the long-double sum of the long-double rows is
measured on the same rows (the restatement adds its rows one after the other), and the kernel may be at most 4 x that,
with a floor of one double ulp of the sum."""
import math

import numpy as np
import pytest
import torch

import calibration_ref as R
from guard import GuardArena

pytestmark = pytest.mark.gpu

# n: no row, one, around one workgroup, 69 workgroups; C: the ends, the project's 7, 20; B: the ends, 10, the default 15
CASES = [(0, 7, 15), (1, 2, 1), (1, 32, 64), (255, 7, 10), (256, 20, 15), (257, 32, 64), (257, 7, 15), (70001, 2, 1),
         (70001, 7, 15), (70001, 20, 10), (70001, 32, 64)]
BETAS = (1.0, 0.4)
EDGE_GAP = 1e-9
FACTOR = 4.0


def make_case(n, C, B, seed):
    """(logits, labels, special): N(0, 3^2) float32 logits and uniform labels; from 255 rows on also, in rows 0..79:
    16 rows of equal logits (where B is no multiple of C), 16 + 8 rows with one logit at +-1e4 (half of the +1e4 rows
    labelled with another class), 8 + 8 rows with one at +-80, 4 rows each with label -1 (ignored), -5 and C, C + 3,
    and 4 + 4 labelled rows holding a NaN / an infinity.  Rows whose confidence at a beta of BETAS lies within EDGE_GAP
    of an interior bin edge are redrawn."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, C)) * 3.0).astype(np.float32)
    labels = rng.integers(0, C, size=n).astype(np.int64)
    special = {}
    if n >= 255:
        if B % C != 0:
            x[0:16] = (rng.standard_normal((16, 1)) * 30.0).astype(np.float32)
            special["equal"] = np.arange(0, 16)
        for name, lo, hi, v in (("hot", 16, 32, 1e4), ("cold", 32, 40, -1e4), ("p80", 40, 48, 80.0), ("m80", 48, 56, -80.0)):
            r = np.arange(lo, hi)
            cols = rng.integers(0, C, size=hi - lo)
            x[r, cols] = v
            special[name] = r
            if name == "hot":
                labels[r] = cols
                labels[r[::2]] = (cols[::2] + 1) % C             # confidently wrong: an NLL of about 1e4 a row
        labels[56:60], labels[60:64], labels[64:66], labels[66:68] = -1, -5, C, C + 3
        special["unlabelled"] = np.arange(56, 68)
        x[np.arange(68, 72), rng.integers(0, C, size=4)] = np.nan
        x[np.arange(72, 76), rng.integers(0, C, size=4)] = (np.inf, -np.inf, np.inf, -np.inf)
        special["nonfinite"] = np.arange(68, 76)
    fixed = np.zeros(n, dtype=bool)
    fixed[:min(n, 80)] = n >= 255
    for _ in range(100):
        near = np.zeros(n, dtype=bool)
        take, _ = R.taking(x, labels)
        for beta in BETAS:
            conf = R.rows(x[take], labels[take], beta)[0]
            t = conf * B
            k = np.rint(t)
            near[np.nonzero(take)[0]] |= (np.abs(t - k) / B <= EDGE_GAP) & (k >= 1) & (k <= B - 1)
        assert not (near & fixed).any(), "a planted row lies on a bin edge"
        if not near.any():
            return x, labels, special
        x[near] = (rng.standard_normal((int(near.sum()), C)) * 3.0).astype(np.float32)
    raise AssertionError("rows stay near a bin edge")


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).view(np.uint8)


class Buffers:
    """fresh zeroed accumulators, error word and workspace for n rows and B bins, in `arena`"""

    def __init__(self, arena, n, B):
        from lidog_amd import _lib
        self.B = B
        self.table = arena.full((B, 3), 0, dtype=torch.int64, name="table")
        self.totals = arena.full(2, 0, dtype=torch.int64, name="totals")
        self.nll = arena.full(1, 0.0, dtype=torch.float64, name="nll_sum")
        self.err = arena.full(1, 0, dtype=torch.int32, name="err")
        self.ws = arena.full(int(_lib.load().lidog_calib_ws(n)), 0.0, dtype=torch.float64, name="ws")

    def outputs(self):
        return self.table, self.totals, self.nll, self.err


def launch(arena, xd, ld, beta, buf, ignore_label=-1, what="lidog_calib_stats"):
    from lidog_amd._lib import call, ptr
    call("lidog_calib_stats", ptr(xd), ptr(ld), xd.shape[0], xd.shape[1], ignore_label, ptr(beta), buf.B,
         ptr(buf.table), ptr(buf.totals), ptr(buf.nll), ptr(buf.err), ptr(buf.ws))
    arena.check(what)
    assert int(buf.ws[:1].view(torch.int64)) == 0                # the ticket is back at zero


def check_against(ref, buf, n, C, B, beta):
    table, totals = buf.table.cpu().numpy(), buf.totals.cpu().numpy()
    nll = float(buf.nll)
    assert np.array_equal(table[:, :2], ref["table"][:, :2]) and totals[0] == ref["totals"][0]
    assert int(buf.err) == ref["err"]
    dq = np.abs(table[:, 2] - ref["table"][:, 2])
    assert (dq <= ref["table"][:, 0]).all(), (dq, ref["table"][:, 0])
    db = abs(int(totals[1]) - int(ref["totals"][1]))
    assert db <= int(ref["totals"][0])
    exact = ref["nll_exact"]
    mine, refs = abs(float(R.LD(nll) - exact)), abs(float(R.LD(ref["nll_sum"]) - exact))
    ulp = math.ulp(float(exact))
    print(f"calib n={n} C={C} B={B} beta={beta}: rows {totals[0]} conf_q off {int(dq.max(initial=0))} brier_q off {db} "
          f"nll_sum {nll:.17g} kernel err {mine:.3g} float64 restatement err {refs:.3g} ulp {ulp:.3g} "
          f"ratio {mine / max(refs, ulp):.3g}")
    assert math.isfinite(nll) and mine <= max(FACTOR * refs, ulp), (mine, refs, ulp)


@pytest.mark.parametrize("n,C,B", CASES)
def test_against_float64(n, C, B):
    x, labels, special = make_case(n, C, B, 100 * C + B + n % 97)
    arena = GuardArena()
    xd, ld = arena.place(torch.from_numpy(x), "logits"), arena.place(torch.from_numpy(labels), "labels")
    one = arena.place(torch.tensor([1.0], dtype=torch.float64), "beta")
    b04 = arena.place(torch.tensor([0.4], dtype=torch.float64), "beta")
    got = {}
    for key, beta, value in (("null", None, 1.0), ("one", one, 1.0), ("b04", b04, 0.4)):
        buf = Buffers(arena, n, B)
        launch(arena, xd, ld, beta, buf)
        ref = R.stats(x, labels, value, B)
        assert R.edge_distance(ref["conf"], B) > EDGE_GAP
        check_against(ref, buf, n, C, B, value if beta is not None else None)
        got[key] = buf
        if n == 0:
            assert all(not bits(t).any() for t in buf.outputs())
        if special:
            take = ref["take"]
            assert not take[special["unlabelled"]].any() and not take[special["nonfinite"]].any() and ref["err"] == 2
            assert ref["table"][:, 0].sum() == n - 20 == ref["totals"][0]
            hot = special["hot"]
            assert (ref["conf"][np.searchsorted(np.nonzero(take)[0], hot)] == 1.0).all()       # exactly 1: the last bin
            assert float(buf.nll) > 8 * 1e4 * value * 0.99
            if "equal" in special:
                assert (ref["conf"][np.searchsorted(np.nonzero(take)[0], special["equal"])] == 1.0 / C).all()
        else:
            assert int(buf.err) == 0
    # a device 1.0 gives NULL's bytes
    for a, b in zip(got["null"].outputs(), got["one"].outputs()):
        assert np.array_equal(bits(a), bits(b))
    # determinism: the same call into fresh accumulators, nll_sum included
    again = Buffers(arena, n, B)
    launch(arena, xd, ld, b04, again)
    for a, b in zip(got["b04"].outputs(), again.outputs()):
        assert np.array_equal(bits(a), bits(b))
    # a pred that is lidog_eval_confusion's: the correct counts add up to the arg-max accuracy at either beta
    if n:
        take = R.taking(x, labels)[0]
        right = int((x[take].argmax(axis=1) == labels[take]).sum())
        assert int(got["null"].table[:, 1].sum()) == right == int(got["b04"].table[:, 1].sum())


def test_no_nonfinite_row_leaves_the_error_word_zero():
    x, labels, _ = make_case(257, 7, 15, 3)
    keep = np.isfinite(x).all(axis=1)
    x, labels = x[keep], labels[keep]
    arena = GuardArena()
    buf = Buffers(arena, x.shape[0], 15)
    launch(arena, arena.place(torch.from_numpy(x)), arena.place(torch.from_numpy(labels)), None, buf)
    assert int(buf.err) == 0 and int(buf.totals[0]) == R.stats(x, labels, 1.0, 15)["totals"][0]


@pytest.mark.parametrize("n,C,B", [(257, 7, 15), (70001, 7, 15), (70001, 32, 64)])
def test_slices_give_the_same_integers(n, C, B):
    x, labels, _ = make_case(n, C, B, 11 + n % 97)
    arena = GuardArena()
    xd, ld = arena.place(torch.from_numpy(x), "logits"), arena.place(torch.from_numpy(labels), "labels")
    beta = arena.place(torch.tensor([0.4], dtype=torch.float64), "beta")
    whole, parts = Buffers(arena, n, B), Buffers(arena, n, B)
    launch(arena, xd, ld, beta, whole)
    cuts = (0, 1, n // 3 + 1, n)
    for a, b in zip(cuts[:-1], cuts[1:]):
        launch(arena, xd[a:b], ld[a:b], beta, parts, what=f"slice {a}:{b}")
    assert np.array_equal(bits(whole.table), bits(parts.table)) and np.array_equal(bits(whole.totals), bits(parts.totals))
    assert int(whole.err) == int(parts.err) == 2
    # nll_sum: another cut, another rounding, the same number up to the summation error of either
    assert abs(float(whole.nll) - float(parts.nll)) <= 1e-12 * abs(float(whole.nll))
    # and the same three calls again: the same bytes, nll_sum included
    again = Buffers(arena, n, B)
    for a, b in zip(cuts[:-1], cuts[1:]):
        launch(arena, xd[a:b], ld[a:b], beta, again)
    assert np.array_equal(bits(again.nll), bits(parts.nll)) and np.array_equal(bits(again.table), bits(parts.table))


def test_an_ignore_label_inside_the_classes():
    x, labels, _ = make_case(257, 7, 15, 5)
    arena = GuardArena()
    buf = Buffers(arena, 257, 15)
    launch(arena, arena.place(torch.from_numpy(x)), arena.place(torch.from_numpy(labels)), None, buf, ignore_label=2)
    ref = R.stats(x, labels, 1.0, 15, ignore_label=2)
    assert ref["totals"][0] < R.stats(x, labels, 1.0, 15)["totals"][0]
    check_against(ref, buf, 257, 7, 15, None)


@pytest.mark.parametrize("C,B", [(1, 15), (33, 15), (7, 0), (7, 65)])
def test_other_shapes_return_2_before_any_launch(C, B):
    from lidog_amd import _lib
    from lidog_amd._lib import ptr
    lib, arena, n = _lib.load(), GuardArena(), 33
    x = arena.place(torch.randn(n, C), "logits")
    labels = arena.place(torch.zeros(n, dtype=torch.int64), "labels")
    buf = Buffers(arena, n, max(1, min(B, 64)))
    buf.table.fill_(-7), buf.totals.fill_(-7), buf.nll.fill_(float("nan")), buf.ws.fill_(float("nan"))
    before = [bits(t).copy() for t in buf.outputs() + (buf.ws,)]
    assert lib.lidog_calib_stats(ptr(x), ptr(labels), n, C, -1, None, B, ptr(buf.table), ptr(buf.totals), ptr(buf.nll),
                                 ptr(buf.err), ptr(buf.ws), _lib.stream()) == 2
    arena.check("refused call")
    for t, b in zip(buf.outputs() + (buf.ws,), before):
        assert np.array_equal(bits(t), b)


def test_calibration_table_is_the_kernel():
    from lidog_amd.calibration import CalibrationTable
    x, labels, _ = make_case(70001, 7, 15, 9)
    keep = np.isfinite(x).all(axis=1)
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
    with pytest.raises(ValueError, match="NaN or infinite"):
        CalibrationTable().add(xd, ld).result()
    xd, ld = xd[torch.from_numpy(keep).cuda()].contiguous(), ld[torch.from_numpy(keep).cuda()].contiguous()
    beta = torch.tensor([0.4], dtype=torch.float64, device="cuda")
    t = CalibrationTable(15).add(xd[:5000], ld[:5000], beta=beta).add(xd[5000:], ld[5000:], beta=beta)
    m = t.result()
    ref = R.stats(x[keep], labels[keep], 0.4, 15)
    assert m["rows"] == ref["totals"][0] and np.array_equal(m["reliability"][:, 1], ref["table"][:, 0])
    assert m["accuracy"] == ref["table"][:, 1].sum() / m["rows"]
    assert abs(m["confidence"] - ref["conf"].mean()) <= 2.0 ** -32 and abs(m["nll"] - ref["nll_sum"] / m["rows"]) <= 1e-9
    assert 0 <= m["ece"] <= m["mce"] <= 1 and 0 <= m["brier"] <= 2
    for bad in (torch.randn(8, 33, device="cuda"), torch.randn(8, 7, device="cuda", dtype=torch.float64)):
        with pytest.raises(ValueError):
            CalibrationTable().add(bad, torch.zeros(8, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="beta"):
        CalibrationTable().add(xd, ld, beta=0.4)
