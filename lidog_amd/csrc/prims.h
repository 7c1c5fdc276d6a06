// Integer prefix sums, the stable radix sort, "rows grouped by key" and the ordered compaction, stated once for every
// feature file.  Device-side pieces are inline here; the kernels and their host loops are in prims.hip (C++ linkage:
// not part of the C ABI).  Wave64 throughout.  Not named scan*: in this tree a scan is a LiDAR sweep (scan_ops.h).
#pragma once
#include "common.h"

// ------------------------------------------------------------------ device side
// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(v, d);
        if (lane >= d) v += y;
    }
    return v;
}

// exclusive prefix sum over the THREADS threads of a workgroup; *total = the sum of all of them, in every thread
template <int THREADS>
__device__ __forceinline__ int block_excl_scan(int v, int *total) {
    static_assert(THREADS % 64 == 0, "whole waves");
    __shared__ int wsum[THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int x = wave_incl_scan(v);
    __syncthreads();  // protect wsum reuse across calls
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < THREADS / 64; ++i) {
        if (i < w) off += wsum[i];
        tot += wsum[i];
    }
    *total = tot;
    return off + x - v;
}

// One workgroup of THREADS threads walks n items in chunks of THREADS * IPT (IPT consecutive items per thread) and
// carries the running total: store(i, sum of load(0 .. i)) for every i < n; returns the sum of all n, in every thread.
// load and store may name the same array: a thread stores only items it has loaded.  Called by the whole workgroup.
template <int THREADS, int IPT, class Load, class Store>
__device__ __forceinline__ int block_scan_chunks(int64_t n, Load load, Store store) {
    int carry = 0;   // every thread gets every chunk's total, so the carry needs no LDS of its own
    for (int64_t c0 = 0; c0 < n; c0 += (int64_t)THREADS * IPT) {
        const int64_t b = c0 + (int64_t)IPT * threadIdx.x;
        int v[IPT], t = 0;
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            v[j] = (b + j < n) ? load(b + j) : 0;
            t += v[j];
        }
        int tot;
        int e = carry + block_excl_scan<THREADS>(t, &tot);
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            if (b + j < n) store(b + j, e);
            e += v[j];
        }
        carry += tot;
    }
    return carry;
}

// number of lanes below this one whose bit is set in a ballot
__device__ __forceinline__ int wave_rank_below(uint64_t ballot) {
    return __popcll(ballot & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// the live lanes of the wave whose BITS-bit digit equals this lane's (the radix scatter's match: BITS ballots)
template <int BITS>
__device__ __forceinline__ uint64_t wave_digit_peers(uint32_t d, bool live) {
    uint64_t peers = __ballot(live);
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        peers &= bit ? bal : ~bal;
    }
    return peers;
}

// first position of the sorted keys[n] whose key is >= k
__device__ __forceinline__ int64_t key_lower_bound(const uint32_t *__restrict__ keys, int64_t n, uint64_t k) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((uint64_t)keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------ host side (prims.hip)
// workspace pieces start on 256-byte boundaries
static inline int64_t lidog_align256(int64_t bytes) { return (bytes + 255) / 256 * 256; }

// Exclusive scan of int32 data[n] in place (scan_block_sums, scan_block_offsets, scan_apply).  sums:
// lidog_scan_sums_ints(n) int32 of scratch; the total is left in sums[ceil(n / 1024)].
int64_t lidog_scan_sums_ints(int64_t n);
int lidog_exclusive_scan(int32_t *data, int64_t n, int32_t *sums, hipStream_t st);

// Stable LSD radix sort of n (key, val) pairs, one digit per pass (k_rs_hist, k_rs_scan, k_rs_scatter); keys
// 0 .. max_key take lidog_radix_passes(max_key) passes.  The pairs end in (ka, va) after an even number of passes and
// in (kb, vb) after an odd one.  hist: lidog_radix_sort_hist_ints(n, passes) int32.
int lidog_radix_passes(int64_t max_key);
int64_t lidog_radix_sort_hist_ints(int64_t n, int passes);
int lidog_radix_sort_pairs(uint32_t *ka, int32_t *va, uint32_t *kb, int32_t *vb, int64_t n, int passes, int32_t *hist,
                           hipStream_t st);

// Rows grouped by key: the caller's key kernel writes n (key, id) pairs to (ka, va) of lidog_group_bufs; then
// lidog_group_by_key sorts them, which leaves the ids in `ids_out` (ascending inside a key), and writes lower[v] =
// first sorted position whose key is >= v for v = 0 .. m.  ws: lidog_group_ws(n, passes) bytes.
struct LidogGroupBufs {
    uint32_t *ka, *kb;
    int32_t *va, *vb, *hist;
};
int64_t lidog_group_ws(int64_t n, int passes);
LidogGroupBufs lidog_group_bufs(void *ws, int64_t n, int passes, int32_t *ids_out);
int lidog_group_by_key(const LidogGroupBufs &b, int64_t n, int passes, int64_t m, int32_t *lower, hipStream_t st);

// Stable multi-way split: the body of the ABI entry lidog_mix_split, whose contract include/lidog_amd.h states
#define LIDOG_SPLIT_MAX_SLOTS 256
int64_t lidog_split_ws_ints(int64_t n, int32_t n_slots);
int lidog_split_rows(const int32_t *keys, int64_t n, const int32_t *slot_of_key, int32_t n_keys, int32_t n_slots,
                     int32_t *rows_out, int32_t *slot_start, int32_t *ws, hipStream_t st);

// Ordered compaction (the split's kernels with one slot and flags for keys): rows_out = the rows i < n with
// flags[i] != 0, ascending; *count = a device word in ws that holds their number.  ws: lidog_compact_ws_ints(n) int32.
int64_t lidog_compact_ws_ints(int64_t n);
int lidog_compact_rows(const int32_t *flags, int64_t n, int32_t *rows_out, int32_t *ws, const int32_t **count,
                       hipStream_t st);
