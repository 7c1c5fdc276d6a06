"""The integer kernels that build a batch's coordinate maps, each through the C ABI on synthetic tables at its block edges,
against the numpy restatements of tests/maps_ref.py: hash insert (+ the 9-word record), first-occurrence compaction,
strided maps, the ballot / prefix-sum rule book, per-row lists, the subset copy, the radix sort behind the sorted-row
tables, lidog_in_segments and lidog_field_lists.

Every input is an integer table made with numpy from a fixed seed (no scan generator).  Every output and every
workspace is allocated GUARD words longer than the header asks for and filled with a sentinel; results are compared
with array_equal (no tolerance anywhere), the words behind every buffer must be unchanged, and a second call must give
the same bytes.  Row counts: multiples of a wavefront, of a 256-thread workgroup and of a 1024-row scan block / radix
chunk, 65 536 rows (k_rs_scan's second trip), 262 144 rows (scan_block_offsets' and k_pairs_scan's second trip),
2 100 000 rows (where a scan workspace of 2048 words past n is too small) and 2 097 153 rows (16 385 tiles: the tile order
without the keys in LDS)."""
import numpy as np
import pytest
import torch

import maps_ref as M

pytestmark = pytest.mark.gpu

GUARD = 4096
SENT = -7
SMALL = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
BIG = [65535, 65536, 65537, 262143, 262144, 262145]
HUGE = 2100000


class Bufs:
    """sentinel-filled device buffers with GUARD words behind each; check() looks at all the guards"""

    def __init__(self):
        self.all = []

    def new(self, words, dtype=torch.int32):
        full = torch.full((int(words) + GUARD,), SENT, dtype=dtype, device="cuda")
        self.all.append((full, int(words)))
        return full[:int(words)]

    def check(self):
        for full, words in self.all:
            assert bool((full[words:] == SENT).all()), f"words behind a buffer of {words} were written"


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _np(t):
    return t.cpu().numpy()


def _same(want, got):
    got = _np(got) if isinstance(got, torch.Tensor) else got
    return want.shape == got.shape and np.array_equal(want, got)


def _twice(run):
    """run() -> dict of numpy results; called twice on fresh buffers, the second call must repeat the first's bytes"""
    a, b = run(), run()
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), f"second call changed {k}"
    return a


def _lib():
    from lidog_amd import _lib
    return _lib


# ------------------------------------------------------------------ synthetic coordinate rows
def _codes(d, bits, seed):
    """d distinct integers below 2^bits (an odd multiplier is a bijection modulo a power of two)"""
    assert d <= 1 << bits
    return (np.arange(d, dtype=np.int64) * 0x9E3779B1 + seed * 0x85EBCA6B) & ((1 << bits) - 1)


def _mixed_rows(d, seed):
    """d distinct rows: batch 0..7, x, y, z in [-512, 512)"""
    c = _codes(d, 33, seed)
    return np.stack([c >> 30, (c & 1023) - 512, ((c >> 10) & 1023) - 512, ((c >> 20) & 1023) - 512], axis=1).astype(np.int32)


def _extreme_rows(d, seed):
    """d distinct rows within 128 cells of the ends of the key's range on every axis (batch within 4 of 0 / 4095); the 16
    corners themselves (-65536 / 65535 on each axis, batch 0 / 4095) come first"""
    c = _codes(d, 27, seed)
    corners = np.array([(b << 24) | (x << 16) | (y << 8) | z for b in (0, 4) for x in (0, 128) for y in (0, 128)
                        for z in (0, 128)], dtype=np.int64)[:d]
    missing = corners[~np.isin(corners, c)]
    free = np.nonzero(~np.isin(c, corners))[0][:missing.shape[0]]
    c[free] = missing

    def axis(v):       # bit 7: which end, bits 0..6: distance from it
        return np.where(v & 128, M.HI - (v & 127), M.LO + (v & 127))

    b = c >> 24
    rows = np.stack([np.where(b & 4, M.BATCH_HI - (b & 3), b & 3), axis((c >> 16) & 255), axis((c >> 8) & 255),
                     axis(c & 255)], axis=1)
    return rows.astype(np.int32)


def _with_duplicates(make, n, dup, seed):
    rng = np.random.default_rng(seed)
    d = {"none": n, "twice": (n + 1) // 2, "equal": 1, "percent": max(1, n // 100)}[dup]
    base = make(d, seed)
    if dup == "none":
        idx = np.arange(n)
    elif dup == "twice":
        idx = np.concatenate([np.arange(d), np.arange(n - d)])
    elif dup == "equal":
        idx = np.zeros(n, np.int64)
    else:
        idx = np.concatenate([np.arange(d), rng.integers(0, d, n - d)])
    return np.ascontiguousarray(base[idx[rng.permutation(n)]])


INSERT_CASES = {
    "mixed_none": (_mixed_rows, "none"), "mixed_twice": (_mixed_rows, "twice"), "mixed_equal": (_mixed_rows, "equal"),
    "mixed_percent": (_mixed_rows, "percent"), "extreme_none": (_extreme_rows, "none"),
    "extreme_percent": (_extreme_rows, "percent"), "out_of_range": (_mixed_rows, "twice"),
}


def _insert_rows(n, case):
    make, dup = INSERT_CASES[case]
    rows = _with_duplicates(make, n, dup, n % 1000 + len(case))
    if case == "out_of_range":          # first, middle and last row outside the key's range, on three different columns
        rows[0, 1] = M.HI + 1
        rows[n // 2, 0] = M.BATCH_HI + 1
        rows[n - 1, 3] = M.LO - 1
    return rows


def _zero_offset_map(coords, n, keys, vals, cap):
    """lidog_kernel_map with the single offset (0, 0, 0): every row of `coords` looked up in the table"""
    L = _lib()
    bufs = Bufs()
    nbr = bufs.new(n)
    off = np.zeros((1, 3), np.int32)
    L.call("lidog_kernel_map", L.ptr(coords), n, L.ptr(keys), L.ptr(vals), cap, off.ctypes.data, 1, L.ptr(nbr))
    out = _np(nbr)
    bufs.check()
    return out


# ------------------------------------------------------------------ insert, insert_info, compact
@pytest.mark.parametrize("case", list(INSERT_CASES))
@pytest.mark.parametrize("n", SMALL + BIG + [HUGE])
def test_insert_info_and_compact(n, case):
    L = _lib()
    rows = _insert_rows(n, case)
    bad = case == "out_of_range"
    first_ref, uniq_ref, inv_ref = M.unique_first(rows)
    m = uniq_ref.shape[0]
    d_rows = _cuda(rows)
    cap = L.load().lidog_hash_capacity(n)
    assert cap >= 2 * n

    def run():
        bufs = Bufs()
        keys, vals = bufs.new(cap, torch.int64), bufs.new(cap)
        keys2, vals2 = bufs.new(cap, torch.int64), bufs.new(cap)
        first, first2 = bufs.new(n), bufs.new(n)
        n_unique, info = bufs.new(1, torch.int64), bufs.new(9, torch.int64)
        err, err2 = bufs.new(1), bufs.new(1)
        err.zero_()
        err2.zero_()
        L.call("lidog_coords_insert", L.ptr(d_rows), n, L.ptr(keys), L.ptr(vals), cap, L.ptr(first), L.ptr(n_unique),
               L.ptr(err))
        L.call("lidog_coords_insert_info", L.ptr(d_rows), n, L.ptr(keys2), L.ptr(vals2), cap, L.ptr(first2), L.ptr(info),
               L.ptr(err2))
        uniq, inv = bufs.new(n), bufs.new(n)
        ws = bufs.new(L.load().lidog_coords_compact_ws(n))
        L.call("lidog_coords_compact", L.ptr(first2), n, L.ptr(keys2), L.ptr(vals2), cap, L.ptr(d_rows), L.ptr(uniq),
               L.ptr(inv), L.ptr(ws))
        out = dict(first=_np(first), first2=_np(first2), n_unique=_np(n_unique), info=_np(info), err=_np(err),
                   err2=_np(err2), uniq=_np(uniq), inv=_np(inv))
        # the rewritten table: the unique rows looked up with the offset (0, 0, 0) are their own output rows
        coords_u = _cuda(rows[uniq_ref])
        out["self"] = _zero_offset_map(coords_u, m, keys2, vals2, cap)
        out["self_first"] = _zero_offset_map(coords_u, m, keys, vals, cap)         # not compacted: first rows
        bufs.check()
        return out

    o = _twice(run)
    assert _same(first_ref, o["first"]) and _same(first_ref, o["first2"])
    assert o["n_unique"][0] == m and o["err"][0] == int(bad) and o["err2"][0] == int(bad)
    assert _same(M.insert_info(rows), o["info"])
    assert _same(uniq_ref, o["uniq"][:m]) and (o["uniq"][m:] == SENT).all() and _same(inv_ref, o["inv"])
    ok = M.in_range(rows[uniq_ref])
    assert ok.all() != bad
    assert _same(np.where(ok, np.arange(m), -1).astype(np.int32), o["self"])
    assert _same(np.where(ok, uniq_ref, -1).astype(np.int32), o["self_first"])


def test_no_rows_on_every_entry_point():
    L = _lib()
    bufs = Bufs()
    cap = L.load().lidog_hash_capacity(0)
    keys, vals = bufs.new(cap, torch.int64), bufs.new(cap)
    one = bufs.new(16)
    n_unique, info, n_out = bufs.new(1, torch.int64), bufs.new(9, torch.int64), bufs.new(1, torch.int64)
    err = bufs.new(1)
    err.zero_()
    empty = np.zeros((0, 4), np.int32)
    L.call("lidog_coords_insert", L.ptr(one), 0, L.ptr(keys), L.ptr(vals), cap, L.ptr(one), L.ptr(n_unique), L.ptr(err))
    assert n_unique.item() == 0
    L.call("lidog_coords_insert_info", L.ptr(one), 0, L.ptr(keys), L.ptr(vals), cap, L.ptr(one), L.ptr(info), L.ptr(err))
    assert _same(M.insert_info(empty), info)
    ws = bufs.new(max(L.load().lidog_coords_compact_ws(0), L.load().lidog_coords_stride_ws(0)))
    L.call("lidog_coords_compact", L.ptr(one), 0, L.ptr(keys), L.ptr(vals), cap, L.ptr(one), L.ptr(one), L.ptr(one),
           L.ptr(ws))
    L.call("lidog_coords_stride", L.ptr(one), 0, 2, L.ptr(keys), L.ptr(vals), cap, L.ptr(one), L.ptr(one), L.ptr(n_out),
           L.ptr(ws), L.ptr(err))
    assert n_out.item() == 0
    off = np.zeros((1, 3), np.int32)
    L.call("lidog_kernel_map", L.ptr(one), 0, L.ptr(keys), L.ptr(vals), cap, off.ctypes.data, 1, L.ptr(one))
    # the table of no rows holds no key
    probe = _cuda(_mixed_rows(5, 1))
    assert (_zero_offset_map(probe, 5, keys, vals, cap) == -1).all()
    k_off = bufs.new(4, torch.int64)
    L.call("lidog_kernel_map_pairs", L.ptr(one), 0, 5, 3, L.ptr(k_off), L.ptr(one), L.ptr(one), None, None, L.ptr(ws))
    assert (k_off == 0).all()
    L.call("lidog_kernel_map_subset", L.ptr(one), 0, 125, off.ctypes.data, 1, L.ptr(one))
    L.call("lidog_kernel_map_sorted", L.ptr(one), 0, 3, L.ptr(k_off), L.ptr(one), L.ptr(one), L.ptr(one), L.ptr(ws), 0)
    seg_off = bufs.new(3)
    L.call("lidog_in_segments", L.ptr(one), 0, 2, L.ptr(one), L.ptr(seg_off), L.ptr(one), L.ptr(ws), 0)
    assert (seg_off == 0).all()
    row_ptr = bufs.new(6)
    L.call("lidog_field_lists", L.ptr(one), 0, 5, L.ptr(row_ptr), L.ptr(one), L.ptr(ws), 0)
    assert (row_ptr == 0).all()
    assert err.item() == 0 and (one == SENT).all()
    bufs.check()


# ------------------------------------------------------------------ strided maps
@pytest.mark.parametrize("s", [2, 3, 16])
@pytest.mark.parametrize("n", SMALL + BIG + [HUGE])
def test_strided_map(n, s):
    L = _lib()
    rows = _mixed_rows(n, n % 1000 + s)
    rows = np.ascontiguousarray(rows[np.random.default_rng(n + s).permutation(n)])
    out_ref, p2c_ref = M.stride(rows, s)
    m = out_ref.shape[0]
    d_rows = _cuda(rows)
    cap = L.load().lidog_hash_capacity(n)

    def run():
        bufs = Bufs()
        keys, vals = bufs.new(cap, torch.int64), bufs.new(cap)
        p2c, out = bufs.new(n), bufs.new(4 * n)
        n_out, err = bufs.new(1, torch.int64), bufs.new(1)
        err.zero_()
        ws = bufs.new(L.load().lidog_coords_stride_ws(n))
        L.call("lidog_coords_stride", L.ptr(d_rows), n, s, L.ptr(keys), L.ptr(vals), cap, L.ptr(p2c), L.ptr(out),
               L.ptr(n_out), L.ptr(ws), L.ptr(err))
        res = dict(p2c=_np(p2c), out=_np(out).reshape(n, 4), n_out=_np(n_out), err=_np(err))
        # the child table: its own rows looked up with the offset (0, 0, 0)
        res["self"] = _zero_offset_map(_cuda(out_ref), m, keys, vals, cap)
        bufs.check()
        return res

    o = _twice(run)
    assert o["n_out"][0] == m and o["err"][0] == 0
    assert _same(out_ref, o["out"][:m]) and _same(p2c_ref, o["p2c"])
    assert _same(np.arange(m, dtype=np.int32), o["self"])


# ------------------------------------------------------------------ rule book
DENSITIES = ["empty", "sparse", "full", "first_empty_last_full"]


def _nbr_table(K, n_out, n_in, density, seed):
    """nbr [K, n_out], entries in [-1, n_in); every row injective on its non-negative entries, as a real map's is"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n_in)
    nbr = np.full((K, n_out), -1, np.int32)
    for k in range(K):
        p = {"empty": 0.0, "sparse": 0.16, "full": 1.0}.get(density, 0.0 if k == 0 else 1.0 if k == K - 1 else 0.16)
        if density == "first_empty_last_full" and K == 1:
            p = 1.0
        if p == 0.0:
            continue
        rows_k = np.nonzero(rng.random(n_out) < p)[0][:n_in] if p < 1.0 else np.arange(min(n_out, n_in))
        nbr[k, rows_k] = np.roll(perm, 7919 * k)[:rows_k.shape[0]]
    return nbr


def _pairs_call(d_nbr, n_out, n_in, K, P, with_pos):
    L = _lib()
    bufs = Bufs()
    k_off = bufs.new(K + 1, torch.int64)
    pair_in, pair_out = bufs.new(P), bufs.new(P)            # a caller that knows P: not one entry more
    pos_out = bufs.new(K * n_out) if with_pos else None
    pos_in = bufs.new(K * n_in) if with_pos else None
    ws = bufs.new(((n_out + 1023) // 1024 + 1) * K + K + 2)
    L.call("lidog_kernel_map_pairs", L.ptr(d_nbr), n_out, n_in, K, L.ptr(k_off), L.ptr(pair_in), L.ptr(pair_out),
           L.ptr(pos_out), L.ptr(pos_in), L.ptr(ws))
    res = dict(k_off=_np(k_off), pair_in=_np(pair_in), pair_out=_np(pair_out))
    if with_pos:
        res.update(pos_out=_np(pos_out).reshape(K, n_out), pos_in=_np(pos_in).reshape(K, n_in))
    bufs.check()
    return res


@pytest.mark.parametrize("K,n_out", [(K, n) for K in (1, 8, 27) for n in SMALL + BIG] + [(125, n) for n in SMALL])
def test_kernel_map_pairs(K, n_out):
    for j, density in enumerate(DENSITIES):
        n_in = n_out + 37 if j >= 2 else max(1, n_out - n_out // 3)        # full offsets: a pair in EVERY row
        nbr = _nbr_table(K, n_out, n_in, density, 1000 * K + n_out % 997 + j)
        k_off, pin, pout, pos_out, pos_in = M.pairs(nbr, n_in)
        P = int(k_off[-1])
        if density == "empty":
            assert P == 0
        if density == "first_empty_last_full" and K > 1:
            assert k_off[1] == 0 and k_off[K] - k_off[K - 1] == n_out
        d_nbr = _cuda(nbr)
        o = _twice(lambda: _pairs_call(d_nbr, n_out, n_in, K, P, True))
        assert _same(k_off, o["k_off"]) and _same(pin, o["pair_in"]) and _same(pout, o["pair_out"]), density
        assert _same(pos_out, o["pos_out"]) and _same(pos_in, o["pos_in"]), density
        o = _twice(lambda: _pairs_call(d_nbr, n_out, n_in, K, P, False))
        assert _same(k_off, o["k_off"]) and _same(pin, o["pair_in"]) and _same(pout, o["pair_out"]), density


@pytest.mark.parametrize("K", [1, 27])
@pytest.mark.parametrize("n", [0, 1, 1022, 1023, 1024, 262143, 262144])
def test_kernel_map_rows(n, K):
    """the scan runs over n + 1 entries: 1023 rows fill one block, 1024 start a second, 262 143 fill 256 blocks"""
    L = _lib()
    for density in ("sparse", "full", "empty"):
        pos = M.pairs(_nbr_table(K, n, n + 5, density, 77 * K + n % 991), n + 5)[3]
        d_pos = _cuda(pos)
        for mark_k in (-1, 0, K - 1):
            row_ptr_ref, row_list_ref = M.rows(pos, mark_k)

            def run():
                bufs = Bufs()
                row_ptr, row_list = bufs.new(n + 1), bufs.new(row_list_ref.shape[0])
                ws = bufs.new((n + 1 + 1023) // 1024 + 1)
                L.call("lidog_kernel_map_rows", L.ptr(d_pos), n, K, mark_k, L.ptr(row_ptr), L.ptr(row_list), L.ptr(ws))
                res = dict(row_ptr=_np(row_ptr), row_list=_np(row_list))
                bufs.check()
                return res

            o = _twice(run)
            assert _same(row_ptr_ref, o["row_ptr"]) and _same(row_list_ref, o["row_list"]), (density, mark_k)


# ------------------------------------------------------------------ subset of a larger table
def _subset_call(d_big, n, K_big, sel, shift):
    """shift = 1: the destination starts 4 bytes into its allocation, which rules the int4 copy out"""
    L = _lib()
    bufs = Bufs()
    K = len(sel)
    full = bufs.new(K * n + shift)
    dst = full[shift:]
    assert dst.data_ptr() % 16 == 4 * shift
    sel = np.ascontiguousarray(sel, dtype=np.int32)
    try:
        L.call("lidog_kernel_map_subset", L.ptr(d_big), n, K_big, sel.ctypes.data, K, L.ptr(dst))
    finally:
        bufs.check()
        assert (full[:shift] == SENT).all()
    return dict(nbr=_np(dst).reshape(K, n))


@pytest.mark.parametrize("n", [1, 3, 4, 1023, 1024, 1028])
def test_kernel_map_subset(n):
    from lidog_amd import me
    rng = np.random.default_rng(n)
    big125 = rng.integers(-1, n, (125, n)).astype(np.int32)
    big27 = rng.integers(-1, n, (27, n)).astype(np.int32)
    for big, sel in ((big125, me._SUBSET_3_OF_5), (big125, [124]), (big27, list(range(27))[::-1]), (big27, [0])):
        d_big = _cuda(big)
        assert d_big.data_ptr() % 16 == 0
        for shift in (0, 1):       # n % 4 == 0 and both tables 16-byte aligned: int4 copy; anything else: scalar copy
            o = _twice(lambda: _subset_call(d_big, n, big.shape[0], sel, shift))
            assert _same(M.subset(big, sel), o["nbr"])
    # the two refusals leave the destination alone
    d_big = _cuda(big125)
    for K_big, sel in ((125, [0, 125]), (125, [-1]), (125, list(range(28))), (27, list(range(28)))):
        with pytest.raises(RuntimeError, match="kernel_map_subset"):
            _subset_call(d_big, n, K_big, sel, 0)


# ------------------------------------------------------------------ sorted rows (the radix sort, wave masks, tile order)
def _has_patterns(K, n, seed):
    """name -> has [K, n] bool: which offsets every row has a neighbour at"""
    rng = np.random.default_rng(seed)
    out = {"random": rng.random((K, n)) < 0.16}
    m0 = int(rng.integers(1, 1 << K))
    out["one_mask"] = np.repeat(np.array([[(m0 >> k) & 1] for k in range(K)], dtype=bool), n, axis=1)
    if K <= 10:
        r = np.arange(n) % (1 << K)
        out["cycled"] = np.stack([(r >> k) & 1 for k in range(K)]).astype(bool)
    third = rng.random((K, n)) < 0.3
    third[:, ::3] = False
    out["third_without_neighbour"] = third
    if K >= 2:
        tie = rng.random((K, n)) < 0.3
        tie[K - 1] = np.roll(tie[0], 1)                     # equal counts on other rows: the lower offset ranks first
        out["equal_counts"] = tie
    hole = rng.random((K, n)) < 0.3
    hole[K // 2] = False
    out["empty_offset"] = hole
    return out


def _sorted_check(has, seed):
    L = _lib()
    K, n = has.shape
    rng = np.random.default_rng(seed)
    nbr = np.where(has, rng.integers(0, n, (1, n)), -1).astype(np.int32)          # only the sign matters
    k_off = np.concatenate([[0], np.cumsum(has.sum(axis=1))]).astype(np.int64)
    perm_ref, wave_ref, order_ref = M.sorted_tables(nbr, k_off)
    d_nbr, d_k_off = _cuda(nbr), _cuda(k_off)
    pad = (n + 127) // 128 * 128
    nbytes = L.load().lidog_kernel_map_sorted_ws(n)

    def run():
        bufs = Bufs()
        perm, wave, order = bufs.new(pad), bufs.new(pad // 32), bufs.new(pad // 128)
        ws = bufs.new((nbytes + 3) // 4)
        L.call("lidog_kernel_map_sorted", L.ptr(d_nbr), n, K, L.ptr(d_k_off), L.ptr(perm), L.ptr(wave), L.ptr(order),
               L.ptr(ws), nbytes)
        res = dict(perm=_np(perm), wave=_np(wave).view(np.uint32), order=_np(order))
        bufs.check()
        return res

    o = _twice(run)
    assert _same(perm_ref, o["perm"]) and (perm_ref[n:] == -1).all()
    assert _same(wave_ref, o["wave"]) and _same(order_ref, o["order"])


@pytest.mark.parametrize("K", [1, 9, 10, 18, 19, 27])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 129, 1023, 1024, 1025, 65535, 65536, 65537])
def test_kernel_map_sorted(n, K):
    """K <= 9, <= 18, <= 27: one, two and three 9-bit radix passes, the row ids ending in `perm` from either side"""
    for name, has in _has_patterns(K, n, 31 * K + n % 983).items():
        _sorted_check(has, K + n)


def test_kernel_map_sorted_past_16384_tiles():
    """2 097 153 rows = 16 385 tiles: k_os_tile_order reads the tiles' keys from global memory, no longer from LDS"""
    n = 2097153
    assert (n + 127) // 128 == 16385
    _sorted_check(np.random.default_rng(5).random((3, n)) < 0.16, 5)


# ------------------------------------------------------------------ segments of a map by batch index
@pytest.mark.parametrize("n", SMALL + BIG)
def test_in_segments(n):
    L = _lib()
    rng = np.random.default_rng(n)
    for B in (1, 2, 512, 513, 4096):
        ids = np.arange(B) if B < 4096 else np.unique(np.concatenate([[0, 4095], rng.integers(0, 4096, 35)]))
        batch = ids[rng.integers(0, ids.shape[0], n)]
        if n >= 2 and B >= 2:
            batch[[0, n - 1]] = (B - 1, 0)                  # the last index first, the first one last
        coords = np.concatenate([batch[:, None], rng.integers(-100, 100, (n, 3))], axis=1).astype(np.int32)
        perm_ref, seg_ref = M.segments(batch, B)
        d_coords = _cuda(coords)
        nbytes = L.load().lidog_in_segments_ws(n)

        def run():
            bufs = Bufs()
            perm, seg_off, bid = bufs.new(n), bufs.new(B + 1), bufs.new(n)
            ws = bufs.new((nbytes + 3) // 4)
            L.call("lidog_in_segments", L.ptr(d_coords), n, B, L.ptr(perm), L.ptr(seg_off), L.ptr(bid), L.ptr(ws), nbytes)
            res = dict(perm=_np(perm), seg_off=_np(seg_off), bid=_np(bid))
            bufs.check()
            return res

        o = _twice(run)
        assert _same(perm_ref, o["perm"]) and _same(seg_ref, o["seg_off"]), B
        assert _same(batch.astype(np.int32), o["bid"]), B


# ------------------------------------------------------------------ per-row lists of an index table
@pytest.mark.parametrize("n", SMALL + BIG)
def test_field_lists(n):
    """m = 511 / 512 and 262 143 / 262 144: the keys 0 .. m take one, two and three 9-bit passes"""
    L = _lib()
    rng = np.random.default_rng(n)
    for m in (1, 511, 512, 262143, 262144):
        inv = rng.integers(0, m, n)
        inv[rng.random(n) < 0.5] = m // 2                   # one hot row holds half the entries
        nobody = rng.random(n) < 0.05
        inv[nobody] = np.where(rng.random(int(nobody.sum())) < 0.5, -1, m)
        inv = inv.astype(np.int32)
        row_ptr_ref, row_list_ref = M.field_lists(inv, m)
        d_inv = _cuda(inv)
        nbytes = L.load().lidog_field_lists_ws(n, m)

        def run():
            bufs = Bufs()
            row_ptr, row_list = bufs.new(m + 1), bufs.new(n)
            ws = bufs.new((nbytes + 3) // 4)
            L.call("lidog_field_lists", L.ptr(d_inv), n, m, L.ptr(row_ptr), L.ptr(row_list), L.ptr(ws), nbytes)
            listed = int(row_ptr[m].item())
            res = dict(row_ptr=_np(row_ptr), row_list=_np(row_list)[:listed])
            bufs.check()
            return res

        o = _twice(run)
        assert _same(row_ptr_ref, o["row_ptr"]) and _same(row_list_ref, o["row_list"]), m
