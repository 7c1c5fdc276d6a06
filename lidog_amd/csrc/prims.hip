// Kernels and host loops of the integer primitives declared in prims.h.  Everything is integer work whose result does
// not depend on the order of arrival: the same bytes on every run.
#include "prims.h"

// ------------------------------------------------------------------ exclusive scan of int32 data[n] in place
// sums[nb + 1] scratch (nb = ceil(n / 1024)); sums[nb] = total
__global__ __launch_bounds__(256) void scan_block_sums(const int32_t *__restrict__ data, int64_t n,
                                                       int32_t *__restrict__ sums) {
    int64_t base = (int64_t)blockIdx.x * 1024 + threadIdx.x * 4;
    int v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (base + j < n) v += data[base + j];
    int tot;
    block_excl_scan<256>(v, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void scan_block_offsets(int32_t *__restrict__ sums, int64_t nb) {
    const int tot = block_scan_chunks<256, 1>(nb, [&](int64_t i) { return sums[i]; },
                                              [&](int64_t i, int e) { sums[i] = e; });
    if (threadIdx.x == 0) sums[nb] = tot;
}

__global__ __launch_bounds__(256) void scan_apply(int32_t *__restrict__ data, int64_t n,
                                                  const int32_t *__restrict__ sums) {
    int64_t base = (int64_t)blockIdx.x * 1024 + threadIdx.x * 4;
    int v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = (base + j < n) ? data[base + j] : 0;
        s += v[j];
    }
    int tot;
    int ex = block_excl_scan<256>(s, &tot) + sums[blockIdx.x];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (base + j < n) data[base + j] = ex;
        ex += v[j];
    }
}

// one int per 1024-entry block and the total behind them
int64_t lidog_scan_sums_ints(int64_t n) { return cdiv64(n, 1024) + 1; }

int lidog_exclusive_scan(int32_t *data, int64_t n, int32_t *sums, hipStream_t st) {
    int64_t nb = cdiv64(n, 1024);
    if (nb == 0) return 0;
    scan_block_sums<<<dim3((unsigned)nb), 256, 0, st>>>(data, n, sums);
    scan_block_offsets<<<1, 256, 0, st>>>(sums, nb);
    scan_apply<<<dim3((unsigned)nb), 256, 0, st>>>(data, n, sums);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ stable LSD radix sort of (key, val) pairs
// Hand-written for wave64: RS_BITS bits per pass.  A workgroup is ONE wavefront that owns RS_CHUNK consecutive
// elements: (1) per-chunk digit histogram (+ per-digit totals), (2) exclusive scan of the digit-major [RS_BINS][chunks]
// table, one wavefront per digit, (3) scatter -- the chunk is walked 64 elements at a time in order; the lanes holding
// the same digit find each other with RS_BITS ballots, rank = popcount of the lower peers, the lowest peer advances the
// digit's cursor: equal keys keep their input order (what the numpy restatement in tests/maps_ref.py calls a stable
// argsort).  Replaces the CUB-compatibility wrapper of round 4 (~10 launches of rocPRIM's merge-sort fallback per sort;
// here 3 per pass).
#define RS_BITS 9
#define RS_BINS (1 << RS_BITS)
#define RS_CHUNK 1024

// hist [RS_BINS][chunks] (digit-major) + totals [RS_BINS] (zeroed by the caller; integer atomics: order-independent)
__global__ __launch_bounds__(64) void k_rs_hist(const uint32_t *__restrict__ keys, int64_t n, int shift, int chunks,
                                                int32_t *__restrict__ hist, int32_t *__restrict__ totals) {
    __shared__ int32_t cnt[RS_BINS];
    const int lane = threadIdx.x;
    for (int i = lane; i < RS_BINS; i += 64) cnt[i] = 0;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * RS_CHUNK, hi = lo + RS_CHUNK < n ? lo + RS_CHUNK : n;
    uint32_t kreg[RS_CHUNK / 64];      // every load of the chunk in flight before the first use
#pragma unroll
    for (int r = 0; r < RS_CHUNK / 64; ++r) {
        const int64_t i = lo + 64 * r + lane;
        kreg[r] = keys[i < hi ? i : hi - 1];
    }
#pragma unroll
    for (int r = 0; r < RS_CHUNK / 64; ++r)
        if (lo + 64 * r + lane < hi) atomicAdd(&cnt[(kreg[r] >> shift) & (RS_BINS - 1)], 1);
    __syncthreads();
    for (int i = lane; i < RS_BINS; i += 64) {
        const int32_t c = cnt[i];
        hist[(int64_t)i * chunks + blockIdx.x] = c;
        if (c) atomicAdd(&totals[i], c);
    }
}

// one wavefront per digit d: hist[d][*] becomes the exclusive scan of the digit's chunk counts, offset by the number of
// keys with a smaller digit (the sum of totals[0 .. d)) -- the global position of the first key of (digit, chunk)
__global__ __launch_bounds__(64) void k_rs_scan(int32_t *__restrict__ hist, const int32_t *__restrict__ totals, int chunks) {
    const int d = blockIdx.x, lane = threadIdx.x;
    int32_t before = 0;
    for (int i = lane; i < d; i += 64) before += totals[i];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) before += __shfl_xor(before, s);
    int32_t *row = hist + (int64_t)d * chunks;
    int32_t run = before;
    for (int c0 = 0; c0 < chunks; c0 += 64) {
        const int c = c0 + lane;
        const int32_t v = c < chunks ? row[c] : 0;
        const int32_t inc = wave_incl_scan(v);
        if (c < chunks) row[c] = run + inc - v;
        run += __shfl(inc, 63);
    }
}

__global__ __launch_bounds__(64) void k_rs_scatter(const uint32_t *__restrict__ keys, const int32_t *__restrict__ vals,
                                                   int64_t n, int shift, int chunks, const int32_t *__restrict__ hist,
                                                   uint32_t *__restrict__ keys_out, int32_t *__restrict__ vals_out) {
    __shared__ int32_t cur[RS_BINS];
    const int lane = threadIdx.x;
    for (int i = lane; i < RS_BINS; i += 64) cur[i] = hist[(int64_t)i * chunks + blockIdx.x];
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * RS_CHUNK, hi = lo + RS_CHUNK < n ? lo + RS_CHUNK : n;
    uint32_t kreg[RS_CHUNK / 64];
    int32_t vreg[RS_CHUNK / 64];
#pragma unroll
    for (int r = 0; r < RS_CHUNK / 64; ++r) {
        const int64_t i = lo + 64 * r + lane;
        kreg[r] = keys[i < hi ? i : hi - 1];
        vreg[r] = vals[i < hi ? i : hi - 1];
    }
#pragma unroll
    for (int r = 0; r < RS_CHUNK / 64; ++r) {
        const int64_t i = lo + 64 * r + lane;
        const bool live = i < hi;
        const uint32_t key = kreg[r];
        const int32_t val = vreg[r];
        const uint32_t d = (key >> shift) & (RS_BINS - 1);
        const uint64_t peers = wave_digit_peers<RS_BITS>(d, live);
        const int rank = wave_rank_below(peers);
        const int32_t at = cur[d];
        __syncthreads();   // every lane has read its cursor before the leaders move them (one wave: costs nothing)
        if (live && rank == 0) cur[d] = at + __popcll(peers);
        __syncthreads();
        if (live) {
            keys_out[at + rank] = key;
            vals_out[at + rank] = val;
        }
    }
}

static int64_t rs_chunks(int64_t n) { return cdiv64(n, RS_CHUNK); }

int lidog_radix_passes(int64_t max_key) {
    int bits = 1;
    while (bits < 63 && ((int64_t)1 << bits) <= max_key) ++bits;
    return (bits + RS_BITS - 1) / RS_BITS;
}

int64_t lidog_radix_sort_hist_ints(int64_t n, int passes) { return (int64_t)RS_BINS * (rs_chunks(n) + passes); }

int lidog_radix_sort_pairs(uint32_t *ka, int32_t *va, uint32_t *kb, int32_t *vb, int64_t n, int passes, int32_t *hist,
                           hipStream_t st) {
    const int chunks = (int)rs_chunks(n);
    int32_t *totals = hist + (int64_t)RS_BINS * chunks;      // [passes][RS_BINS], one row per pass (zeroed once)
    LIDOG_CHECK_HIP(hipMemsetAsync(totals, 0, sizeof(int32_t) * RS_BINS * passes, st));
    for (int pass = 0; pass < passes; ++pass) {
        const int shift = pass * RS_BITS;
        int32_t *tot = totals + pass * RS_BINS;
        k_rs_hist<<<chunks, 64, 0, st>>>(ka, n, shift, chunks, hist, tot);
        k_rs_scan<<<RS_BINS, 64, 0, st>>>(hist, tot, chunks);
        k_rs_scatter<<<chunks, 64, 0, st>>>(ka, va, n, shift, chunks, hist, kb, vb);
        uint32_t *tk = ka; ka = kb; kb = tk;
        int32_t *tv = va; va = vb; vb = tv;
    }
    return 0;
}

// ------------------------------------------------------------------ rows grouped by key
// lower[v] = first sorted position whose key is >= v (v = 0 .. m)
__global__ __launch_bounds__(256) void k_key_lower_bound(const uint32_t *__restrict__ sorted, int64_t n, int64_t m,
                                                         int32_t *__restrict__ lower) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v <= m) lower[v] = (int32_t)key_lower_bound(sorted, n, (uint64_t)v);
}

int64_t lidog_group_ws(int64_t n, int passes) {
    return 3 * lidog_align256(4 * n) + lidog_align256(4 * lidog_radix_sort_hist_ints(n, passes));
}

LidogGroupBufs lidog_group_bufs(void *ws, int64_t n, int passes, int32_t *ids_out) {
    char *p = (char *)ws;
    LidogGroupBufs b;
    b.ka = (uint32_t *)p;         p += lidog_align256(4 * n);
    b.kb = (uint32_t *)p;         p += lidog_align256(4 * n);
    int32_t *tmp = (int32_t *)p;  p += lidog_align256(4 * n);
    b.hist = (int32_t *)p;
    b.va = (passes & 1) ? tmp : ids_out;   // the ids start where this many passes leave them in ids_out
    b.vb = (passes & 1) ? ids_out : tmp;
    return b;
}

int lidog_group_by_key(const LidogGroupBufs &b, int64_t n, int passes, int64_t m, int32_t *lower, hipStream_t st) {
    if (lidog_radix_sort_pairs(b.ka, b.va, b.kb, b.vb, n, passes, b.hist, st)) return 1;
    k_key_lower_bound<<<(unsigned)cdiv64(m + 1, 256), 256, 0, st>>>((passes & 1) ? b.kb : b.ka, n, m, lower);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ stable multi-way split, ordered compaction
#define SPLIT_THREADS 256
#define SPLIT_WAVES (SPLIT_THREADS / 64)
#define SPLIT_ITERS 4       // rows per split block: SPLIT_THREADS * SPLIT_ITERS
#define SPLIT_TILE (SPLIT_THREADS * SPLIT_ITERS)

__device__ __forceinline__ int mix_slot(const int32_t *__restrict__ keys, int64_t i, int64_t n,
                                        const int32_t *__restrict__ slot_of_key, int32_t n_keys, int32_t S) {
    if (i >= n) return -1;
    const int32_t k = keys[i];
    if (!slot_of_key) return k ? 0 : -1;   // the compaction: a flag, one slot
    if (k < 0 || k >= n_keys) return -1;
    const int32_t s = slot_of_key[k];
    return (s >= 0 && s < S) ? s : -1;
}

// taken rows per (slot, block): cnt[s * nblocks + b]
__global__ __launch_bounds__(SPLIT_THREADS) void k_mix_split_count(const int32_t *__restrict__ keys, int64_t n,
                                                                   const int32_t *__restrict__ slot_of_key,
                                                                   int32_t n_keys, int32_t S, int64_t nblocks,
                                                                   int32_t *__restrict__ cnt) {
    __shared__ int32_t c[LIDOG_SPLIT_MAX_SLOTS];
    for (int s = threadIdx.x; s < S; s += SPLIT_THREADS) c[s] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * SPLIT_TILE;
#pragma unroll
    for (int it = 0; it < SPLIT_ITERS; ++it) {
        const int s = mix_slot(keys, base + it * SPLIT_THREADS + threadIdx.x, n, slot_of_key, n_keys, S);
        if (s >= 0) atomicAdd(&c[s], 1);   // a count: the order of the adds does not matter
    }
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += SPLIT_THREADS) cnt[(int64_t)s * nblocks + blockIdx.x] = c[s];
}

// exclusive scan of cnt[len] in place (one block, chunks of 1024 with a carry); slot_start[s] = cnt[s * nblocks] after
// the scan, slot_start[S] = the total
__global__ __launch_bounds__(SPLIT_THREADS) void k_mix_split_scan(int32_t *cnt, int64_t len, int64_t nblocks, int32_t S,
                                                                  int32_t *__restrict__ slot_start) {
    const int tot = block_scan_chunks<SPLIT_THREADS, 4>(len, [&](int64_t i) { return cnt[i]; },
                                                        [&](int64_t i, int e) { cnt[i] = e; });
    __syncthreads();   // the starts below were stored by other threads
    for (int s = threadIdx.x; s < S; s += SPLIT_THREADS) slot_start[s] = cnt[(int64_t)s * nblocks];
    if (threadIdx.x == 0) slot_start[S] = tot;
}

// position of a taken row = start of its (slot, block) + taken rows of its slot in earlier chunks of the block + in
// earlier waves of the chunk + its rank among the lanes of its wave holding the same slot (ballot, popcount of the lower
// lanes).  Each pass of the loop below resolves the lanes of one slot, so a wave runs (distinct slots in it) passes.
__global__ __launch_bounds__(SPLIT_THREADS) void k_mix_split_scatter(const int32_t *__restrict__ keys, int64_t n,
                                                                     const int32_t *__restrict__ slot_of_key,
                                                                     int32_t n_keys, int32_t S, int64_t nblocks,
                                                                     const int32_t *__restrict__ start,
                                                                     int32_t *__restrict__ rows_out) {
    __shared__ int32_t run[LIDOG_SPLIT_MAX_SLOTS];
    __shared__ int32_t wcnt[SPLIT_WAVES][LIDOG_SPLIT_MAX_SLOTS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int s = threadIdx.x; s < S; s += SPLIT_THREADS) {
        run[s] = start[(int64_t)s * nblocks + blockIdx.x];
#pragma unroll
        for (int i = 0; i < SPLIT_WAVES; ++i) wcnt[i][s] = 0;
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * SPLIT_TILE;
    for (int it = 0; it < SPLIT_ITERS; ++it) {
        const int64_t row = base + it * SPLIT_THREADS + threadIdx.x;
        const int slot = mix_slot(keys, row, n, slot_of_key, n_keys, S);
        int rank = 0;
        uint64_t pending = __ballot(slot >= 0);
        while (pending) {   // wave-uniform
            const int leader = __builtin_ctzll(pending);
            const int s = __shfl(slot, leader);
            const uint64_t same = __ballot(slot == s);
            if (slot == s) rank = wave_rank_below(same);
            if (lane == leader) wcnt[w][s] = __popcll(same);
            pending &= ~same;
        }
        __syncthreads();
        if (slot >= 0) {
            int pos = run[slot] + rank;
            for (int i = 0; i < w; ++i) pos += wcnt[i][slot];
            rows_out[pos] = (int32_t)row;
        }
        __syncthreads();
        for (int s = threadIdx.x; s < S; s += SPLIT_THREADS) {
            int add = 0;
#pragma unroll
            for (int i = 0; i < SPLIT_WAVES; ++i) {
                add += wcnt[i][s];
                wcnt[i][s] = 0;
            }
            run[s] += add;
        }
        __syncthreads();
    }
}

int64_t lidog_split_ws_ints(int64_t n, int32_t n_slots) {
    return (int64_t)(n_slots > 0 ? n_slots : 0) * cdiv64(n > 0 ? n : 0, SPLIT_TILE) + 1;
}

// slot_of_key == NULL: keys are flags, n_slots = 1 (mix_slot)
static int split_launch(const int32_t *keys, int64_t n, const int32_t *slot_of_key, int32_t n_keys, int32_t n_slots,
                        int32_t *rows_out, int32_t *slot_start, int32_t *ws, hipStream_t st) {
    const int64_t nblocks = cdiv64(n, SPLIT_TILE);
    if (nblocks == 0 || n_slots == 0) {
        LIDOG_CHECK_HIP(hipMemsetAsync(slot_start, 0, sizeof(int32_t) * (size_t)(n_slots + 1), st));
        return 0;
    }
    LIDOG_REQUIRE(nblocks < (int64_t)UINT32_MAX, "lidog_mix_split: grid too large");
    k_mix_split_count<<<(unsigned)nblocks, SPLIT_THREADS, 0, st>>>(keys, n, slot_of_key, n_keys, n_slots, nblocks, ws);
    k_mix_split_scan<<<1, SPLIT_THREADS, 0, st>>>(ws, (int64_t)n_slots * nblocks, nblocks, n_slots, slot_start);
    k_mix_split_scatter<<<(unsigned)nblocks, SPLIT_THREADS, 0, st>>>(keys, n, slot_of_key, n_keys, n_slots, nblocks,
                                                                     ws, rows_out);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

int lidog_split_rows(const int32_t *keys, int64_t n, const int32_t *slot_of_key, int32_t n_keys, int32_t n_slots,
                     int32_t *rows_out, int32_t *slot_start, int32_t *ws, hipStream_t st) {
    LIDOG_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX, "lidog_mix_split: n = %lld out of range", (long long)n);
    LIDOG_REQUIRE(n_slots >= 0 && n_slots <= LIDOG_SPLIT_MAX_SLOTS, "lidog_mix_split: %d slots (at most %d)", n_slots,
                  LIDOG_SPLIT_MAX_SLOTS);
    LIDOG_REQUIRE(n_keys >= 0, "lidog_mix_split: n_keys = %d", n_keys);
    LIDOG_REQUIRE(slot_of_key || n_keys == 0, "lidog_mix_split: %d keys without their table", n_keys);
    // an empty table is never read (every key is outside it), and a NULL one would select the flag form: any address
    return split_launch(keys, n, slot_of_key ? slot_of_key : keys, n_keys, n_slots, rows_out, slot_start, ws, st);
}

// ws: the slot's (start, end) pair, then the split's own workspace
int64_t lidog_compact_ws_ints(int64_t n) { return 2 + lidog_split_ws_ints(n, 1); }

int lidog_compact_rows(const int32_t *flags, int64_t n, int32_t *rows_out, int32_t *ws, const int32_t **count,
                       hipStream_t st) {
    LIDOG_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX, "lidog_compact_rows: n = %lld out of range", (long long)n);
    *count = ws + 1;
    return split_launch(flags, n, nullptr, 0, 1, rows_out, ws, ws + 2, st);
}
