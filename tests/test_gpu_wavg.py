"""lidog_wavg_apply (csrc/wavg.hip) through the C ABI: every mode against the numpy float32 restatement of
tests/wavg_ref.py bit for bit, over segment lengths around the vector width, the wavefront, the workgroup and one
workgroup's sweep, every pair of 4-byte offsets of the two pointers from a 16-byte boundary (the float4 and the scalar
route), 1 to 200 segments in one launch, segments long enough for the grid-stride loop to turn, and with canary words
between and around the segments that no launch may touch."""
import numpy as np
import pytest
import torch

import wavg_ref as R

pytestmark = pytest.mark.gpu

COPY, EMA, SWA, SWAP = range(4)
CANARY = 0x7FC0DEAD                      # as int32 words: the tests compare bits, never values
GAP = 5                                   # canary words between two segments, at least
LENGTHS = [0, 1, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]     # 1024: one workgroup's sweep of float4s
TAUS = [0.0, 0.5, 0.996, 1.0]
DIVISORS = [2, 3, 1000]


def _values(rng, n):
    """normal floats of both signs over six decades"""
    mag = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))
    return (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)


class Arena:
    """segments (n, live offset, average offset) -- the offsets in words from a 16-byte boundary -- laid into one live
    and one average array between canary words; host copies are kept for the expected result"""

    def __init__(self, specs, seed, max_blocks=None):
        from lidog_amd.optim import WAVG_MAX_BLOCKS, wavg_table
        rng = np.random.default_rng(seed)
        self.specs, self.at = specs, []
        cur = [GAP, GAP]
        for n, lo, ao in specs:
            at = []
            for side, off in ((0, lo), (1, ao)):
                start = -(-cur[side] // 4) * 4 + off
                at.append(start)
                cur[side] = start + n + GAP
            self.at.append(tuple(at))
        self.words = [c + GAP for c in cur]
        self.host = []
        for side in (0, 1):
            h = np.full(self.words[side], CANARY, dtype=np.int32).view(np.float32)
            for (n, _, _), at in zip(specs, self.at):
                h[at[side]:at[side] + n] = _values(rng, n)
            self.host.append(h)
        self.dev = [torch.from_numpy(h.copy()).cuda() for h in self.host]
        assert all(d.data_ptr() % 16 == 0 for d in self.dev)
        triples = [(self.dev[0].data_ptr() + 4 * l, self.dev[1].data_ptr() + 4 * a, n)
                   for (n, _, _), (l, a) in zip(specs, self.at)]
        table, self.blocks = wavg_table(triples, WAVG_MAX_BLOCKS if max_blocks is None else max_blocks)
        self.table = torch.from_numpy(table).cuda()

    def reset(self):
        for d, h in zip(self.dev, self.host):
            d.copy_(torch.from_numpy(h))

    def launch(self, mode, c0=0.0, c1=0.0):
        from lidog_amd._lib import call, ptr
        call("lidog_wavg_apply", ptr(self.table), len(self.specs), self.blocks, mode, c0, c1)

    def expected(self, mode, t=None, n_before=None):
        """(live, average) host arrays after one launch on the arena as it was built"""
        live, avg = self.host[0].copy(), self.host[1].copy()
        for (n, _, _), (l, a) in zip(self.specs, self.at):
            p, q = self.host[0][l:l + n], self.host[1][a:a + n]
            if mode == COPY:
                avg[a:a + n] = p
            elif mode == EMA:
                avg[a:a + n] = R.ema_step(q, p, t)
            elif mode == SWA:
                avg[a:a + n] = R.swa_step(q, p, n_before)
            else:
                avg[a:a + n], live[l:l + n] = p, q
        return live, avg

    def check(self, expected, what):
        torch.cuda.synchronize()
        for side, (d, e) in enumerate(zip(self.dev, expected)):
            got = d.cpu().numpy().view(np.int32)
            want = e.view(np.int32)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"{what}: {'live average'.split()[side]} word {bad[0]} of {got.size} " \
                                  f"({bad.size} differ): {got[bad[0]]:#x} != {want[bad[0]]:#x}"

    def every_mode(self, what):
        """COPY, EMA over TAUS, SWA over DIVISORS, SWAP, SWAP twice; canaries are part of every comparison"""
        runs = [(COPY, {}, (0.0, 0.0))]
        runs += [(EMA, dict(t=t), (float(t), float(1.0 - t))) for t in TAUS]
        runs += [(SWA, dict(n_before=d - 1), (float(d), 0.0)) for d in DIVISORS]
        runs += [(SWAP, {}, (0.0, 0.0))]
        for mode, kw, coef in runs:
            self.reset()
            self.launch(mode, *coef)
            self.check(self.expected(mode, **kw), f"{what} mode {mode} {kw}")
        self.launch(SWAP)                                  # the second of two: every byte is back
        self.check(self.host, f"{what} two swaps")


def test_segment_lengths_in_one_launch():
    """aligned pointers: head 0, float4 body, tails of 0..3; an empty segment in the middle of the table"""
    arena = Arena([(n, 0, 0) for n in LENGTHS], seed=1)
    assert arena.blocks == len(LENGTHS) - 1 + 1            # one workgroup each, none for n = 0, two for 1025
    arena.every_mode("lengths")


@pytest.mark.parametrize("n", [2, 5, 64, 1029])
def test_every_pair_of_pointer_offsets(n):
    """equal offsets: a scalar head of (4 - offset) % 4 words, then float4; different ones: the scalar loop"""
    arena = Arena([(n, lo, ao) for lo in range(4) for ao in range(4)], seed=10 + n)
    arena.every_mode(f"offsets n={n}")


@pytest.mark.parametrize("n_segs", [1, 8, 9, 200])
def test_segment_counts(n_segs):
    rng = np.random.default_rng(n_segs)
    specs = [(int(rng.integers(0, 300)), int(rng.integers(0, 4)), int(rng.integers(0, 4))) for _ in range(n_segs)]
    specs[0] = (int(specs[0][0]) + 1,) + specs[0][1:]      # at least one segment has elements
    arena = Arena(specs, seed=100 + n_segs)
    arena.every_mode(f"{n_segs} segments")


def test_no_segments_is_a_no_op():
    from lidog_amd._lib import call, ptr
    arena = Arena([(7, 0, 0)], seed=3)
    block0 = torch.zeros(1, dtype=torch.int64, device="cuda")
    for mode in (COPY, EMA, SWA, SWAP):
        call("lidog_wavg_apply", ptr(block0), 0, 0, mode, 0.5, 0.5)
        call("lidog_wavg_apply", None, 0, 0, mode, 0.5, 0.5)
    arena.check(arena.host, "n_segs = 0")
    empty = Arena([(0, 0, 0), (0, 1, 2)], seed=4)          # segments without elements get no workgroup: no launch
    assert empty.blocks == 0
    empty.launch(SWAP)
    empty.check(empty.host, "empty segments")


@pytest.mark.parametrize("n,lo,ao,max_blocks", [
    (2 ** 20 + 3, 0, 0, 64),        # float4 route, 16 sweeps of 64 workgroups and a tail
    (2 ** 20 + 3, 1, 1, 64),        # the same behind a scalar head of 3
    (2 ** 20 + 3, 0, 2, 64),        # scalar route: 64 sweeps
    (3 * 2 ** 20 + 5, 0, 0, None),  # the default cap: 2048 workgroups, one and a half sweeps
])
def test_grid_stride_loop_turns(n, lo, ao, max_blocks):
    """a long segment next to a short one on either side, the workgroups shared out by size"""
    arena = Arena([(7, 3, 3), (n, lo, ao), (257, 2, 1)], seed=n % 1000 + lo + 4 * ao, max_blocks=max_blocks)
    per = np.diff(arena.table.cpu().numpy()[9:])
    assert per[0] == 1 and per[2] == 1 and per[1] * 1024 < n
    for mode, kw, coef in ((EMA, dict(t=0.996), (0.996, 1.0 - 0.996)), (SWA, dict(n_before=2), (3.0, 0.0)),
                           (COPY, {}, (0.0, 0.0)), (SWAP, {}, (0.0, 0.0))):
        arena.reset()
        arena.launch(mode, *coef)
        arena.check(arena.expected(mode, **kw), f"long segment mode {mode}")
    arena.launch(SWAP)
    arena.check(arena.host, "long segment two swaps")


def test_runs_on_the_stream_it_is_given():
    """queued behind a copy on a side stream, the launch sees that copy's data"""
    arena = Arena([(4099, 0, 0)], seed=5)
    side = torch.cuda.Stream()
    fresh = _values(np.random.default_rng(6), 4099)
    staged = torch.from_numpy(fresh).pin_memory()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        arena.dev[0][arena.at[0][0]:arena.at[0][0] + 4099].copy_(staged, non_blocking=True)
        arena.launch(COPY)
    side.synchronize()
    live, avg = arena.host[0].copy(), arena.host[1].copy()
    live[arena.at[0][0]:arena.at[0][0] + 4099] = fresh
    avg[arena.at[0][1]:arena.at[0][1] + 4099] = fresh
    arena.check((live, avg), "side stream")
