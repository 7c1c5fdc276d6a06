"""Numpy restatements of the integer kernels that build a batch's coordinate maps (csrc/coords.hip, the sorted-row tables
of csrc/sconv_os.hip, lidog_in_segments, lidog_field_lists), one function per contract and written as
include/lidog_amd.h states it: no torch, no GPU, nothing imported from the package under test or from the CPU oracle.
tests/test_maps_ref_cpu.py pins them to oracle.me_cpu.CoordinateManager and to brute-force Python loops;
tests/test_gpu_map_primitives.py holds the kernels to them with array_equal.

Conventions: coordinates are int32 rows (batch, x, y, z); a neighbour table is [K, n_out] (k-major) with -1 for "no
neighbour"; position tables likewise; every index table is int32 and k_off is int64, as the C ABI has them."""
import numpy as np

LO, HI, BATCH_HI = -65536, 65535, 4095          # the range of the 63-bit hash key


def in_range(rows):
    """rows the hash key can hold: -65536 <= x, y, z <= 65535 and 0 <= batch <= 4095"""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    return (r[:, 0] >= 0) & (r[:, 0] <= BATCH_HI) & ((r[:, 1:] >= LO) & (r[:, 1:] <= HI)).all(axis=1)


def _keys(rows):
    """one int64 per row: equal for equal in-range rows; a row out of range enters no key and is a coordinate of its own
    (key -1 - i)"""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    ok = in_range(r)
    key = (((r[:, 0] << 17 | (r[:, 1] - LO)) << 17 | (r[:, 2] - LO)) << 17) | (r[:, 3] - LO)
    return np.where(ok, key, -1 - np.arange(r.shape[0], dtype=np.int64))


def unique_first(rows):
    """(first_row [n], unique_rows [m], inverse [n]): first_row[i] = the first row with row i's coordinate, unique_rows =
    the rows that are their own first occurrence, ascending, inverse[i] = position of first_row[i] in unique_rows"""
    key = _keys(rows)
    n = key.shape[0]
    if n == 0:
        z = np.zeros(0, np.int32)
        return z, z.copy(), z.copy()
    _, first_of_key, which = np.unique(key, return_index=True, return_inverse=True)      # return_index: first occurrence
    first_row = first_of_key[which.reshape(-1)]
    own = first_row == np.arange(n)
    rank = np.cumsum(own) - own                       # exclusive count of first occurrences
    return first_row.astype(np.int32), np.nonzero(own)[0].astype(np.int32), rank[first_row].astype(np.int32)


def stride(rows, s):
    """(coords_out [m, 4], parent2child [n]): floor(c / s) * s toward -infinity per spatial column, duplicates collapsed,
    rows in first-occurrence order of the parent"""
    c = np.asarray(rows, dtype=np.int64).reshape(-1, 4).copy()
    c[:, 1:] = np.floor_divide(c[:, 1:], s) * s       # numpy floors (-7 // 2 == -4), C truncates
    _, uniq, inv = unique_first(c)
    return c[uniq].astype(np.int32), inv


def insert_info(rows):
    """the 9-word record of lidog_coords_insert_info: (unique rows, error flag, largest batch index, lowest x, y, z,
    highest x, y, z) over ALL rows; without rows the extrema are the placeholders -2^40 (largest) and 2^40 (lowest)"""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    if r.shape[0] == 0:
        return np.array([0, 0, -(1 << 40)] + [1 << 40] * 3 + [-(1 << 40)] * 3, dtype=np.int64)
    m = unique_first(r)[1].shape[0]
    return np.array([m, int(not in_range(r).all()), r[:, 0].max(), *r[:, 1:].min(axis=0), *r[:, 1:].max(axis=0)],
                    dtype=np.int64)


def pairs(nbr, n_in):
    """(k_off [K + 1] int64, pair_in [P], pair_out [P], pos_out [K, n_out], pos_in [K, n_in]): per offset k the pairs
    (nbr[k][o], o) with nbr[k][o] >= 0 in ascending o; pos_out[k][o] / pos_in[k][i] = the position of that pair in the
    lists, -1 elsewhere"""
    nbr = np.asarray(nbr)
    K, n_out = nbr.shape
    valid = nbr >= 0
    k_off = np.concatenate([[0], np.cumsum(valid.sum(axis=1))]).astype(np.int64)
    kk, oo = np.nonzero(valid)                        # row-major: ascending k, then ascending o
    pair_in = nbr[kk, oo].astype(np.int32)
    pair_out = oo.astype(np.int32)
    p = np.arange(kk.shape[0], dtype=np.int32)
    pos_out = np.full((K, n_out), -1, np.int32)
    pos_out[kk, oo] = p
    pos_in = np.full((K, n_in), -1, np.int32)
    pos_in[kk, pair_in] = p
    return k_off, pair_in, pair_out, pos_out, pos_in


def rows(pos, mark_k=-1):
    """(row_ptr [n + 1], row_list [row_ptr[n]]) of a position table pos [K, n]: the entries >= 0 of column o in ascending
    offset order; the entry of offset mark_k (>= 0) is stored as -1"""
    pos = np.asarray(pos)
    K, n = pos.shape
    valid = (pos >= 0).T                              # [n, K]: row-major selection = per row, ascending k
    row_ptr = np.concatenate([[0], np.cumsum(valid.sum(axis=1))]).astype(np.int32)
    vals = pos.T.copy()
    if mark_k >= 0:
        vals[:, mark_k] = -1
    return row_ptr, vals[valid].astype(np.int32)


def subset(big, sel):
    """row k of the small table = row sel[k] of the large one"""
    return np.asarray(big)[np.asarray(sel, dtype=np.int64)]


def _popcount(v):
    v = np.asarray(v, dtype=np.uint64)
    c = np.zeros(v.shape, np.int64)
    for b in range(32):
        c += ((v >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return c


def sorted_tables(nbr, k_off):
    """(perm [pad128(n)], wave_masks [pad128(n) / 32] uint32, tile_order [pad128(n) / 128]) of lidog_kernel_map_sorted.
    Only the sign of nbr matters.  The sort key of a row has one bit per offset it has a neighbour at; the bit position of
    offset k is the number of offsets with MORE pairs (k_off; ties: lower k first), so the rarest offset is the most
    significant bit.  perm = the rows in stable ascending key order, -1 behind row n; wave_masks = the OR of the
    neighbour masks (bit k = offset k) of every 32 sorted rows; tile_order = the 128-row tiles in stable ascending
    order of 127 - blocks, blocks = the set bits of the tile's four wave masks."""
    nbr = np.asarray(nbr)
    K, n = nbr.shape
    counts = np.diff(np.asarray(k_off, dtype=np.int64))
    pos = [sum(1 for j in range(K) if counts[j] > counts[k] or (counts[j] == counts[k] and j < k)) for k in range(K)]
    mask = np.zeros(n, np.int64)
    key = np.zeros(n, np.int64)
    for k in range(K):
        has = (nbr[k] >= 0).astype(np.int64)
        mask |= has << k
        key |= has << pos[k]
    order = np.argsort(key, kind="stable")
    pad = (n + 127) // 128 * 128
    perm = np.concatenate([order, np.full(pad - n, -1)]).astype(np.int32)
    wave = np.bitwise_or.reduce(np.concatenate([mask[order], np.zeros(pad - n, np.int64)]).reshape(-1, 32), axis=1)
    blocks = _popcount(wave).reshape(-1, 4).sum(axis=1)
    tile_order = np.argsort(127 - blocks, kind="stable").astype(np.int32)
    return perm, wave.astype(np.uint32), tile_order


def segments(batch, B):
    """(perm [n], seg_off [B + 1]) of lidog_in_segments: the rows in stable batch order, and where each batch index starts
    in it (an absent index: an empty range)"""
    batch = np.asarray(batch, dtype=np.int64)
    perm = np.argsort(batch, kind="stable")
    seg_off = np.searchsorted(batch[perm], np.arange(B + 1), side="left")
    return perm.astype(np.int32), seg_off.astype(np.int32)


def field_lists(inv, m):
    """(row_ptr [m + 1], row_list [row_ptr[m]]) of lidog_field_lists: the entries j with inv[j] == v are
    row_list[row_ptr[v] .. row_ptr[v + 1]) in ascending j; an entry outside [0, m) is in no list"""
    inv = np.asarray(inv, dtype=np.int64)
    key = np.where((inv >= 0) & (inv < m), inv, m)
    order = np.argsort(key, kind="stable")
    row_ptr = np.searchsorted(key[order], np.arange(m + 1), side="left").astype(np.int32)
    return row_ptr, order[:row_ptr[m]].astype(np.int32)
