"""tests/maps_ref.py (the numpy restatements the map-building kernels are held to in tests/test_gpu_map_primitives.py)
against two independent statements of the same contracts: the CPU oracle's CoordinateManager (insert, stride,
kernel_map) on every scene of tests/sconv_ref.py and on two helpers.small_batch maps, and brute-force Python loops on
inputs of at most 40 rows.  Plus the workspace contract of lidog_coords_compact / lidog_coords_stride: pure host
code, so the library loads without a GPU."""
import functools

import numpy as np
import pytest
import torch

import maps_ref as M
import sconv_ref as S
from helpers import small_batch

BATCHES = {"batch_01": (0, 1), "batch_34": (3, 4)}


@functools.lru_cache(maxsize=None)
def _coords(name):
    if name in BATCHES:
        return small_batch(BATCHES[name], n_points=2500).numpy()
    return S.scene(name)


MAPS = list(S.SCENES) + list(BATCHES)


# ------------------------------------------------------------------ 1. against the CPU oracle
@pytest.mark.parametrize("name", MAPS)
def test_unique_first_and_insert_info_equal_the_oracle_insert(name):
    import oracle.me_cpu as OME
    c = _coords(name)
    n = c.shape[0]
    rng = np.random.default_rng(n)
    # the map itself (no duplicates) and the map with a third of its rows repeated in shuffled order
    for rows in (c, np.concatenate([c, c[rng.permutation(n)[:n // 3 + 1]]])[rng.permutation(n + n // 3 + 1)]):
        rows = np.ascontiguousarray(rows.astype(np.int32))
        cm = OME.CoordinateManager()
        uniq, inv = cm.insert(torch.from_numpy(rows))
        first, uniq_ref, inv_ref = M.unique_first(rows)
        assert np.array_equal(uniq.numpy(), uniq_ref) and np.array_equal(inv.numpy(), inv_ref)
        assert np.array_equal(first, uniq_ref[inv_ref]) and first.dtype == np.int32
        assert np.array_equal(cm.maps[1].numpy(), rows[uniq_ref])
        info = M.insert_info(rows)
        assert info[0] == uniq_ref.shape[0] and info[1] == 0 and info[2] == rows[:, 0].max()
        assert np.array_equal(info[3:6], rows[:, 1:].min(0)) and np.array_equal(info[6:9], rows[:, 1:].max(0))


@pytest.mark.parametrize("name", MAPS)
def test_stride_equals_the_oracle_stride(name):
    import oracle.me_cpu as OME
    c = _coords(name)
    cm = OME.CoordinateManager()
    cm.insert(torch.from_numpy(c))
    for s in (2, 4, 16):
        out, p2c = M.stride(c, s)
        assert np.array_equal(cm.stride(1, s).numpy(), out)
        assert np.array_equal(out, S.strided(c, s))                                    # the float64 tests' own yardstick
        fl = c.astype(np.int64).copy()
        fl[:, 1:] = fl[:, 1:] // s * s
        assert np.array_equal(out[p2c], fl)


@pytest.mark.parametrize("name", MAPS)
def test_pairs_equal_the_oracle_kernel_map(name):
    import oracle.me_cpu as OME
    c = _coords(name)
    cm = OME.CoordinateManager()
    cm.insert(torch.from_numpy(c))
    for key in ((1, 1, 3), (1, 2, 2), (2, 2, 3)):
        k_off, pin, pout, nbr = (t.numpy() for t in cm.kernel_map(*key))
        n_in = cm.maps[key[0]].shape[0]
        got = M.pairs(nbr.T, n_in)                                                     # the oracle's table is [n_out, K]
        assert np.array_equal(got[0], k_off) and got[0].dtype == np.int64
        assert np.array_equal(got[1], pin) and np.array_equal(got[2], pout)
        _check_positions(nbr.T, n_in, *got)


def _check_positions(nbr, n_in, k_off, pin, pout, pos_out, pos_in):
    """pos_out / pos_in are the inverse of the pair lists"""
    K, n_out = nbr.shape
    assert pos_out.shape == (K, n_out) and pos_in.shape == (K, n_in)
    assert ((pos_out >= 0) == (nbr >= 0)).all() and (pos_out >= 0).sum() == (pos_in >= 0).sum() == pin.shape[0]
    for k in range(K):
        p = np.arange(k_off[k], k_off[k + 1])
        assert np.array_equal(pos_out[k][pout[p]], p) and np.array_equal(pos_in[k][pin[p]], p)


# ------------------------------------------------------------------ 2. against brute-force loops, <= 40 rows
def _tiny_tables(seed, n_out, n_in, K, density):
    """nbr [K, n_out] with entries in [-1, n_in), every row injective on its non-negative entries"""
    rng = np.random.default_rng(seed)
    nbr = np.full((K, n_out), -1, np.int64)
    for k in range(K):
        take = np.nonzero(rng.random(n_out) < density)[0][:n_in]
        nbr[k, take] = rng.permutation(n_in)[:take.shape[0]]
    return nbr


def test_unique_first_stride_and_info_equal_loops():
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 7, 40):
        rows = np.concatenate([rng.integers(0, 3, (n, 1)), rng.integers(-3, 3, (n, 3))], axis=1).astype(np.int32)
        if n == 40:
            rows[[0, 17, 39], 2] = (65536, -65537, 70000)                   # three rows out of range, two of them equal-ish
            rows[5] = rows[0]                                               # ... and a copy of one: still its own coordinate
        first, uniq, inv = M.unique_first(rows)
        seen, f_ref, u_ref, i_ref = {}, [], [], []
        for i, r in enumerate(rows.tolist()):
            ok = 0 <= r[0] <= 4095 and all(-65536 <= v <= 65535 for v in r[1:])
            key = tuple(r) if ok else ("out of range", i)
            if key not in seen:
                seen[key] = (i, len(u_ref))
                u_ref.append(i)
            f_ref.append(seen[key][0])
            i_ref.append(seen[key][1])
        assert first.tolist() == f_ref and uniq.tolist() == u_ref and inv.tolist() == i_ref
        info = M.insert_info(rows)
        if n:
            assert info.tolist() == [len(u_ref), int(n == 40), max(r[0] for r in rows.tolist())] + \
                [min(r[j] for r in rows.tolist()) for j in (1, 2, 3)] + [max(r[j] for r in rows.tolist()) for j in (1, 2, 3)]
        else:
            assert info.tolist() == [0, 0, -2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40, -2 ** 40, -2 ** 40, -2 ** 40]
        if n == 40:
            continue
        for s in (2, 3, 16):
            out, p2c = M.stride(rows, s)
            seen, o_ref, p_ref = {}, [], []
            for r in rows.tolist():
                q = (r[0],) + tuple((v // s) * s for v in r[1:])            # python's // floors toward -infinity
                if q not in seen:
                    seen[q] = len(o_ref)
                    o_ref.append(list(q))
                p_ref.append(seen[q])
            assert out.tolist() == o_ref and p2c.tolist() == p_ref and out.dtype == np.int32


@pytest.mark.parametrize("K,n_out,n_in,density", [(1, 1, 1, 1.0), (3, 40, 33, 0.3), (27, 17, 40, 0.16), (8, 40, 40, 0.0),
                                                  (5, 33, 40, 1.0)])
def test_pairs_rows_and_subset_equal_loops(K, n_out, n_in, density):
    nbr = _tiny_tables(K * 100 + n_out, n_out, n_in, K, density)
    k_off, pin, pout, pos_out, pos_in = M.pairs(nbr, n_in)
    ko, pi, po = [0], [], []
    po_ref = [[-1] * n_out for _ in range(K)]
    pi_ref = [[-1] * n_in for _ in range(K)]
    for k in range(K):
        for o in range(n_out):
            if nbr[k][o] >= 0:
                po_ref[k][o] = pi_ref[k][nbr[k][o]] = len(pi)
                pi.append(nbr[k][o])
                po.append(o)
        ko.append(len(pi))
    assert k_off.tolist() == ko and pin.tolist() == pi and pout.tolist() == po
    assert pos_out.tolist() == po_ref and pos_in.tolist() == pi_ref
    assert (pin.dtype, pout.dtype, pos_out.dtype, pos_in.dtype) == (np.int32,) * 4
    for mark_k in (-1, 0, K - 1):
        row_ptr, row_list = M.rows(pos_out, mark_k)
        rp, rl = [0], []
        for o in range(n_out):
            for k in range(K):
                if pos_out[k][o] >= 0:
                    rl.append(-1 if k == mark_k else pos_out[k][o])
            rp.append(len(rl))
        assert row_ptr.tolist() == rp and row_list.tolist() == rl
    sel = list(range(K))[::-1][:27]
    assert M.subset(nbr, sel).tolist() == [nbr[k].tolist() for k in sel]
    assert np.array_equal(S.pairs(nbr)[0], k_off) and np.array_equal(S.pairs(nbr)[1], pin)


@pytest.mark.parametrize("K,n", [(1, 1), (3, 40), (10, 33), (27, 40)])
def test_sorted_tables_equal_loops(K, n):
    for density in (0.0, 0.3, 1.0):
        nbr = _tiny_tables(K + n, n, n, K, density)
        if K == 3:
            nbr[1] = nbr[0]                                                  # equal counts: the lower offset ranks first
        k_off = M.pairs(nbr, n)[0]
        perm, wave, order = M.sorted_tables(nbr, k_off)
        cnt = [(nbr[k] >= 0).sum() for k in range(K)]
        by_count = sorted(range(K), key=lambda k: (-cnt[k], k))             # most frequent first = bit 0
        keys = [sum(1 << by_count.index(k) for k in range(K) if nbr[k][r] >= 0) for r in range(n)]
        want = sorted(range(n), key=lambda r: (keys[r], r))
        assert perm.shape == (128,) and perm[:n].tolist() == want and (perm[n:] == -1).all()
        masks = [sum(1 << k for k in range(K) if nbr[k][r] >= 0) for r in want] + [0] * (128 - n)
        w_ref = []
        for w in range(4):
            v = 0
            for m in masks[32 * w:32 * w + 32]:
                v |= m
            w_ref.append(v)
        assert wave.tolist() == w_ref and wave.dtype == np.uint32 and order.tolist() == [0]
    # the tile order on its own: stable ascending 127 - blocks over several tiles
    n = 5 * 128
    nbr = np.full((3, n), -1)
    nbr[0, 128:256] = 1                      # sorted: the 512 rows without a neighbour first, then the 128 with offset 0
    perm, wave, order = M.sorted_tables(nbr, M.pairs(nbr, n)[0])
    assert order.tolist() == [4, 0, 1, 2, 3] and wave.tolist() == [0] * 16 + [1] * 4


def test_segments_and_field_lists_equal_loops():
    rng = np.random.default_rng(3)
    for n, B in ((0, 1), (1, 1), (40, 2), (40, 9), (33, 4096)):
        batch = rng.integers(0, B, n)
        if n:
            batch[batch == 1] = 0                                            # an absent index in the middle
        perm, seg_off = M.segments(batch, B)
        want = sorted(range(n), key=lambda r: (batch[r], r))
        assert perm.tolist() == want and seg_off.shape == (B + 1,)
        assert seg_off.tolist() == [sum(1 for v in batch if v < b) for b in range(B + 1)]
    for n, m in ((0, 3), (1, 1), (40, 7), (40, 1), (37, 600)):
        inv = rng.integers(-1, m + 1, n)                                     # -1 and m name no row
        row_ptr, row_list = M.field_lists(inv, m)
        rp, rl = [0], []
        for v in range(m):
            rl += [j for j in range(n) if inv[j] == v]
            rp.append(len(rl))
        assert row_ptr.tolist() == rp and row_list.tolist() == rl and row_ptr.dtype == row_list.dtype == np.int32


# ------------------------------------------------------------------ 3. the workspace contract
@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2096128, 2096129, 2 ** 30])
def test_scan_workspaces_hold_the_block_sums(n):
    """device_exclusive_scan writes ceil(n / 1024) + 1 block sums behind the n (compact) or 2 n (stride) words in front
    of them; the 2048 words past n that the header used to state are one word short from n = 2 096 129 on"""
    from lidog_amd import _lib
    L = _lib.load()
    blocks = (n + 1023) // 1024
    assert L.lidog_coords_compact_ws(n) >= n + blocks + 1
    assert L.lidog_coords_stride_ws(n) >= 2 * n + blocks + 1
    assert L.lidog_coords_compact_ws(-n - 1) >= 0 and L.lidog_coords_stride_ws(-n - 1) >= 0
    assert (2048 >= blocks + 1) == (n <= 2096128)
