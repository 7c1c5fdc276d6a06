"""The gradient-norm, SAM-perturbation and clipping kernels (lidog_amd/csrc/sam.hip) against tests/sam_ref.py on the GPU.

Sizes: 0, one element, a float4 tail alone (3), one partial workgroup (1023), exactly one (1024), one and a tail (1025),
and one size past a full sweep of the capped grid -- LIDOG_FLAT_MAX_BLOCKS = 2048 workgroups of 1024 elements -- so that
the grid-stride loop runs.  Every size at a 16-byte-aligned base and at a base one float further (the scalar head), and
1025 also with the buffers aligned differently from each other (the scalar loop).  Two kinds of data: ordinary values,
where the perturbation moves every weight, and the same with values near 1e-20 and 1e+15 mixed in; both with mixed signs
and zeros.

The squared norm is held to 1.01 n 2^-53 relative (sam_ref.sqnorm_bound: non-negative float64 terms, exact products, any
summation order) and to equal bytes on two calls.  Perturbation and clipping are held bit for bit to the restatement FED
WITH THE KERNEL'S OWN NORM WORD: sqrt and division in double are IEEE operations on both sides.  Every buffer lies in a
tests/guard.py arena: no band may change."""
import numpy as np
import pytest
import torch

import sam_ref as R
from guard import GuardArena

pytestmark = pytest.mark.gpu

MAX_BLOCKS = 2048                        # the grid cap: include/lidog_amd.h LIDOG_FLAT_MAX_BLOCKS
PAST_A_SWEEP = MAX_BLOCKS * 1024 + 4 * 1024 + 3
SIZES = [0, 1, 3, 1023, 1024, 1025, PAST_A_SWEEP]
SENTINEL = 123.0                         # the float in front of a payload that starts one float late
_DATA = {}


def _data(n, extreme):
    """(w, g) float32 [n]: mixed signs, a tenth of each zero (a -0.0 among w's), `extreme`: a few 1e-20 / 1e+15 in each,
    never at the same index (|w| g and w^2 g stay finite)"""
    key = (n, extreme)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * n + extreme)
        w = (rng.standard_normal(n) * 0.3).astype(np.float32)
        g = (rng.standard_normal(n) * 2.0).astype(np.float32)
        w[rng.random(n) < 0.1] = 0.0
        g[rng.random(n) < 0.1] = 0.0
        if n > 2:
            w[n // 2] = -0.0
            g[n // 2] = 0.0
        if extreme and n:
            idx = rng.permutation(n)[:min(n, 16)]
            for j, i in enumerate(idx):
                value = np.float32([1e-20, -1e15, 1e15, -1e-20][j % 4] * (1 + j / 16))
                if (j // 4) % 2 == 0:
                    g[i], w[i] = value, np.float32(0.25)
                else:
                    w[i], g[i] = value, np.float32(-0.5)
        _DATA[key] = (w, g)
    return _DATA[key]


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _np_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


class _Buffers:
    """w, g, backup (float32 [n], starting `offs` floats into their payloads), the workspace and the norm word"""

    def __init__(self, n, offs, extreme):
        from lidog_amd import _lib
        self.arena = GuardArena("cuda")
        self.n, self.offs = n, offs
        self.w0, self.g0 = _data(n, extreme)
        self.raw = {}
        for name, off, src in (("w", offs[0], self.w0), ("g", offs[1], self.g0), ("backup", offs[2], None)):
            raw = self.arena.full(n + off, SENTINEL, name=name)
            view = raw[off:]
            if src is not None and n:
                view.copy_(torch.from_numpy(src))
            elif n:
                view.fill_(float("nan"))
            self.raw[name] = raw
            setattr(self, name, view)
        ws_bytes = _lib.load().lidog_flat_sqnorm_ws(n)
        assert ws_bytes == 8 * max(1, min(-(-n // 1024), MAX_BLOCKS))
        self.ws = self.arena.full(ws_bytes // 8, float("nan"), torch.float64, name="ws")
        self.out = self.arena.full(1, float("nan"), torch.float64, name="out")
        for name, off in zip(("w", "g", "backup"), offs):
            assert n == 0 or getattr(self, name).data_ptr() % 16 == 4 * off

    def sqnorm(self, adaptive):
        from lidog_amd._lib import call, ptr
        call("lidog_flat_sqnorm", ptr(self.g), ptr(self.w) if adaptive else None, self.n, 1 if adaptive else 0,
             ptr(self.ws), ptr(self.out))
        return self.out.clone()

    def check(self, what):
        self.arena.check(what)
        for name, off in zip(("w", "g", "backup"), self.offs):
            assert off == 0 or float(self.raw[name][0]) == SENTINEL, f"{what}: the float in front of {name} changed"


CASES = [(n, (o, o, o)) for n in SIZES for o in (0, 1)] + [(1025, (1, 0, 2)), (PAST_A_SWEEP, (0, 3, 0))]


@pytest.mark.parametrize("extreme", [0, 1], ids=["ordinary", "extreme"])
@pytest.mark.parametrize("n, offs", CASES, ids=[f"n{n}-off{''.join(map(str, o))}" for n, o in CASES])
def test_kernels_against_the_restatement(n, offs, extreme):
    from lidog_amd._lib import call, ptr
    b = _Buffers(n, offs, extreme)
    w0, g0 = b.w0, b.g0
    words = {}
    for adaptive in (False, True):
        # ---- the squared norm
        first = b.sqnorm(adaptive)
        b.ws.fill_(float("nan"))                                  # the workspace is written before it is read
        second = b.sqnorm(adaptive)
        assert first.view(torch.int64).item() == second.view(torch.int64).item(), "two calls, two results"
        got = float(first)
        want = R.sqnorm64(g0, w0 if adaptive else None)
        assert np.isfinite(want)
        if n == 0:
            assert got == 0.0 and want == 0.0
        else:
            err = abs(got - want) / want if want else abs(got)
            print(f"n={n} offs={offs} adaptive={adaptive}: sqnorm {got:.17g}, relative error {err:.3g}, "
                  f"bound {R.sqnorm_bound(n):.3g}")
            assert err <= R.sqnorm_bound(n)
        words[adaptive] = got
        assert np.array_equal(_bits(b.w), _np_bits(w0)) and np.array_equal(_bits(b.g), _np_bits(g0))   # inputs only read
        # ---- the ascent step, from the kernel's own word
        rho = 0.05 if not adaptive else 2.0
        call("lidog_sam_perturb", ptr(b.w), ptr(b.g), ptr(b.backup), n, ptr(b.out), rho, 1 if adaptive else 0)
        want_w = R.perturb(w0, g0, got, rho, adaptive)
        got_w = _bits(b.w)
        bad = np.flatnonzero(got_w != _np_bits(want_w))
        assert bad.size == 0, f"adaptive={adaptive}: {bad.size} of {n} weights differ, first {bad[:3]}"
        assert np.array_equal(_bits(b.backup), _np_bits(w0)), "backup is not the old w"
        none = g0 == 0
        assert np.array_equal(got_w[none], _np_bits(w0)[none]), "an element without gradient moved"
        if n >= 1023 and not extreme:
            assert (got_w != _np_bits(w0)).sum() > 0.7 * n        # the step moved what has a gradient
        assert np.array_equal(_bits(b.g), _np_bits(g0))
        b.w.copy_(b.backup)                                       # SAM.second_step's restore
        assert np.array_equal(_bits(b.w), _np_bits(w0)), "restore did not give every byte back"
        if n:
            b.backup.fill_(float("nan"))
        b.check(f"sqnorm + perturb, adaptive={adaptive}")
    # ---- clipping, from the kernel's own word (plain norm)
    b.sqnorm(False)
    sq = float(b.out)
    assert sq == words[False]
    call("lidog_flat_clip", ptr(b.g), n, ptr(b.out), 1e30, 1.0)
    assert np.array_equal(_bits(b.g), _np_bits(g0)), "a large max_norm changed the gradient"
    norm = float(np.sqrt(sq))
    for max_norm, scale in ((0.37 * norm, 1.0), (0.37 * norm, 0.5)):
        if n == 0 or norm == 0:
            continue
        b.g.copy_(torch.from_numpy(g0))
        assert R.clip_coef(sq, max_norm, scale) < 1
        call("lidog_flat_clip", ptr(b.g), n, ptr(b.out), max_norm, scale)
        bad = np.flatnonzero(_bits(b.g) != _np_bits(R.clip(g0, sq, max_norm, scale)))
        assert bad.size == 0, f"clip scale={scale}: {bad.size} of {n} gradients differ, first {bad[:3]}"
        assert float(b.out) == sq                                 # the word is only read
    b.check("clip")


def test_an_all_zero_gradient_moves_nothing():
    """|| g || = 0: coef = rho / 1e-12 is finite, and no element is added to"""
    from lidog_amd._lib import call, ptr
    n = 1025
    b = _Buffers(n, (0, 0, 0), 0)
    b.g.zero_()
    assert float(b.sqnorm(False)) == 0.0
    call("lidog_sam_perturb", ptr(b.w), ptr(b.g), ptr(b.backup), n, ptr(b.out), 0.05, 0)
    assert np.array_equal(_bits(b.w), _np_bits(b.w0)) and np.array_equal(_bits(b.backup), _np_bits(b.w0))
    call("lidog_flat_clip", ptr(b.g), n, ptr(b.out), 1.0, 1.0)
    assert not bool(b.g.any())
    b.check("zero gradient")
