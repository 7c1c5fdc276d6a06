// Scan-mixing kernels of the augmentation-based baselines: PointCutMixSourceDataset.merge_data
// (utils/datasets/pointcutmix.py:43-135) and CoSMixSourceDataset.merge_data (utils/datasets/cosmix.py:50-171).
// The host makes the reference's random draws; the device counts (cells of the 10 m quantisation, classes), splits the
// source rows into the drawn cells / classes in the reference's concatenation order and writes the merged point set in
// one gather.  The two quantisations reuse lidog_voxel_floor / lidog_coords_insert / lidog_coords_compact (data.py).
// No position comes from an atomic: the result is the same on every run.
#include "aug_ops.h"
#include "prims.h"

#define MIX_THREADS 256
#define MIX_HIST_BINS 4096      // LDS bins per pass of the histogram; more bins take more passes over the keys
#define MIX_MAX_SLOTS LIDOG_SPLIT_MAX_SLOTS
#define MIX_MAX_COLS 6

// ------------------------------------------------------------------ histogram
// per-block LDS counts (one pass per MIX_HIST_BINS bins), then one global atomic per block per non-empty bin
__global__ __launch_bounds__(MIX_THREADS) void k_mix_hist(const int32_t *__restrict__ keys, int64_t n, int32_t nbins,
                                                          int32_t *counts) {
    __shared__ int32_t h[MIX_HIST_BINS];
    const int64_t stride = (int64_t)gridDim.x * MIX_THREADS;
    for (int32_t b0 = 0; b0 < nbins; b0 += MIX_HIST_BINS) {
        const int32_t nb = min(MIX_HIST_BINS, nbins - b0);
        for (int j = threadIdx.x; j < nb; j += MIX_THREADS) h[j] = 0;
        __syncthreads();
        for (int64_t i = (int64_t)blockIdx.x * MIX_THREADS + threadIdx.x; i < n; i += stride) {
            const int64_t k = (int64_t)keys[i] - b0;
            if (k >= 0 && k < nb) atomicAdd(&h[k], 1);
        }
        __syncthreads();
        for (int j = threadIdx.x; j < nb; j += MIX_THREADS)
            if (h[j]) atomicAdd(&counts[b0 + j], h[j]);
        __syncthreads();
    }
}

extern "C" int lidog_mix_histogram(const int32_t *keys, int64_t n, int32_t nbins, int32_t *counts, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0 && nbins >= 0, "lidog_mix_histogram: n = %lld, nbins = %d", (long long)n, nbins);
    if (nbins == 0) return 0;
    LIDOG_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)nbins, st));
    if (n == 0) return 0;
    const int64_t blocks = cdiv64(n, MIX_THREADS);
    const unsigned grid = (unsigned)(blocks < 1024 ? blocks : 1024);
    k_mix_hist<<<grid, MIX_THREADS, 0, st>>>(keys, n, nbins, counts);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ stable multi-way split
// the kernels are the tree's shared split (prims.hip), which the ordered compactions of the other files use with one slot
extern "C" int64_t lidog_mix_split_ws(int64_t n, int32_t n_slots) { return lidog_split_ws_ints(n, n_slots); }

extern "C" int lidog_mix_split(const int32_t *keys, int64_t n, const int32_t *slot_of_key, int32_t n_keys,
                               int32_t n_slots, int32_t *rows_out, int32_t *slot_start, int32_t *ws, void *stream) {
    return lidog_split_rows(keys, n, slot_of_key, n_keys, n_slots, rows_out, slot_start, ws, (hipStream_t)stream);
}

// ------------------------------------------------------------------ fused concatenating gather
struct MixCols {
    const uint32_t *t[MIX_MAX_COLS];   // target rows
    const uint32_t *s[MIX_MAX_COLS];   // source rows
    uint32_t *o[MIX_MAX_COLS];         // merged rows
    int32_t words[MIX_MAX_COLS];       // 32-bit words per row
    int32_t n;
};

// merged row r < n_target: target row r; r = n_target + j: source row rows[j] (perm == NULL), or
// rows[slot_start[s] + perm[j]] with take_start[s] <= j < take_start[s + 1].  Coordinates: float(c) * voxel, the float32
// product torch computes for `int_tensor * voxel_size`.
__global__ __launch_bounds__(MIX_THREADS) void k_mix_gather(const int32_t *__restrict__ coords_t, int64_t n_target,
                                                            const int32_t *__restrict__ coords_s,
                                                            const int32_t *__restrict__ rows,
                                                            const int32_t *__restrict__ slot_start,
                                                            const int32_t *__restrict__ perm,
                                                            const int32_t *__restrict__ take_start, int32_t S,
                                                            int64_t n_take, float voxel, float *__restrict__ coords_out,
                                                            MixCols cols) {
    __shared__ int32_t ts[MIX_MAX_SLOTS + 1];
    if (perm) {
        for (int s = threadIdx.x; s <= S; s += MIX_THREADS) ts[s] = take_start[s];
        __syncthreads();
    }
    const int64_t r = (int64_t)blockIdx.x * MIX_THREADS + threadIdx.x;
    if (r >= n_target + n_take) return;
    const bool tgt = r < n_target;
    int64_t src;
    if (tgt) {
        src = r;
    } else {
        const int64_t j = r - n_target;
        if (perm) {
            int lo = 0, hi = S;   // the last slot whose take_start <= j (empty slots share their start)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (ts[mid] <= j) lo = mid;
                else hi = mid;
            }
            src = rows[slot_start[lo] + perm[j]];
        } else {
            src = rows[j];
        }
    }
    const int32_t *c = (tgt ? coords_t : coords_s) + 3 * src;
#pragma unroll
    for (int d = 0; d < 3; ++d) coords_out[3 * r + d] = (float)c[d] * voxel;
    for (int k = 0; k < cols.n; ++k) {
        const int wd = cols.words[k];
        const uint32_t *in = (tgt ? cols.t[k] : cols.s[k]) + src * wd;
        uint32_t *out = cols.o[k] + r * wd;
        for (int q = 0; q < wd; ++q) out[q] = in[q];
    }
}

extern "C" int lidog_mix_gather(const int32_t *coords_t, int64_t n_target, const int32_t *coords_s,
                                const int32_t *rows, const int32_t *slot_start, const int32_t *perm,
                                const int32_t *take_start, int32_t n_slots, int64_t n_take, float voxel_size,
                                float *coords_out, int32_t n_cols, void *const *cols_host,
                                const int32_t *col_words_host, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n_target >= 0 && n_take >= 0, "lidog_mix_gather: negative row count");
    LIDOG_REQUIRE(n_cols >= 0 && n_cols <= MIX_MAX_COLS, "lidog_mix_gather: %d columns (at most %d)", n_cols,
                  MIX_MAX_COLS);
    LIDOG_REQUIRE(n_take == 0 || rows, "lidog_mix_gather: source rows missing");
    LIDOG_REQUIRE(!perm || (n_slots >= 1 && n_slots <= MIX_MAX_SLOTS && slot_start && take_start),
                  "lidog_mix_gather: a permutation needs 1..%d slots, slot_start and take_start", MIX_MAX_SLOTS);
    MixCols cols = {};
    cols.n = n_cols;
    for (int k = 0; k < n_cols; ++k) {
        cols.t[k] = (const uint32_t *)cols_host[3 * k];
        cols.s[k] = (const uint32_t *)cols_host[3 * k + 1];
        cols.o[k] = (uint32_t *)cols_host[3 * k + 2];
        cols.words[k] = col_words_host[k];
        LIDOG_REQUIRE(cols.words[k] >= 0, "lidog_mix_gather: column %d has %d words", k, cols.words[k]);
    }
    const int64_t total = n_target + n_take;
    if (total == 0) return 0;
    k_mix_gather<<<(unsigned)cdiv64(total, MIX_THREADS), MIX_THREADS, 0, st>>>(
        coords_t, n_target, coords_s, rows, slot_start, perm, take_start, n_slots, n_take, voxel_size, coords_out,
        cols);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ the same gather with CoSMix's per-class transforms
struct MixAugKinds {
    int32_t n;
    int32_t kind[AUG_MAX_OPS];
};

// Merged row r as k_mix_gather (take_start is always read: every class row needs its slot).  A class row of slot s is
// float(c) * voxel transformed by the slot's operations (slot_params[(s * kinds.n + o) * 9 ..], kinds shared by the
// slots); a target row stays float(c) * voxel.  f64: torch.cat promoted the concatenation to float64 (a rotation in the
// list and a class drawn), so every row, the target's included, is floored as float64; otherwise as float32.
__global__ __launch_bounds__(MIX_THREADS) void k_mix_gather_aug(
    const int32_t *__restrict__ coords_t, int64_t n_target, const int32_t *__restrict__ coords_s, int64_t n_source,
    const int32_t *__restrict__ rows, const int32_t *__restrict__ slot_start, const int32_t *__restrict__ perm,
    const int32_t *__restrict__ take_start, int32_t S, int64_t n_take, float voxel, MixAugKinds kinds,
    const double *__restrict__ slot_params, int32_t f64, double qx, double qy, double qz, int4 *__restrict__ rows_out,
    MixCols cols) {
    __shared__ int32_t ts[MIX_MAX_SLOTS + 1];
    if (S > 0) {   // block-uniform; no class drawn: take_start may be NULL
        for (int s = threadIdx.x; s <= S; s += MIX_THREADS) ts[s] = take_start[s];
        __syncthreads();
    }
    const int64_t r = (int64_t)blockIdx.x * MIX_THREADS + threadIdx.x;
    if (r >= n_target + n_take) return;
    const bool tgt = r < n_target;   // S == 0 only with n_take == 0 (checked by the entry): every row is a target row
    int64_t src = r;
    int slot = 0;
    if (!tgt) {
        const int64_t j = r - n_target;
        int lo = 0, hi = S;   // the last slot whose take_start <= j (empty slots share their start)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (ts[mid] <= j) lo = mid;
            else hi = mid;
        }
        slot = lo;
        // perm == NULL: every row of every slot in order, rows[j].  Never read outside rows or the source scan.
        int64_t k = perm ? (int64_t)slot_start[lo] + perm[j] : j;
        k = k < 0 ? 0 : (k >= n_source ? n_source - 1 : k);
        src = rows[k];
        src = src < 0 ? 0 : (src >= n_source ? n_source - 1 : src);
    }
    const int32_t *c = (tgt ? coords_t : coords_s) + 3 * src;
    const float x0 = (float)c[0] * voxel, x1 = (float)c[1] * voxel, x2 = (float)c[2] * voxel;
    AugPoint a = aug_transform_point(x0, x1, x2, tgt ? 0 : kinds.n, kinds.kind,
                                     slot_params + (int64_t)slot * kinds.n * 9);
    if (f64 && !a.is64) {   // float32 rows of a float64 concatenation widen exactly
#pragma unroll
        for (int k = 0; k < 3; ++k) a.d[k] = (double)a.f[k];
        a.is64 = true;
    }
    rows_out[r] = aug_voxel_row(a, 0, qx, qy, qz);
    for (int k = 0; k < cols.n; ++k) {
        const int wd = cols.words[k];
        const uint32_t *in = (tgt ? cols.t[k] : cols.s[k]) + src * wd;
        uint32_t *out = cols.o[k] + r * wd;
        for (int q = 0; q < wd; ++q) out[q] = in[q];
    }
}

extern "C" int lidog_mix_gather_aug(const int32_t *coords_t, int64_t n_target, const int32_t *coords_s,
                                    int64_t n_source, const int32_t *rows, const int32_t *slot_start,
                                    const int32_t *perm, const int32_t *take_start, int32_t n_slots, int64_t n_take,
                                    float voxel_size, const int32_t *op_kinds_host, int32_t n_ops,
                                    const double *slot_params, int32_t f64, double qx, double qy, double qz,
                                    int32_t *rows_out, int32_t n_cols, void *const *cols_host,
                                    const int32_t *col_words_host, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n_target >= 0 && n_take >= 0 && n_source >= 0, "lidog_mix_gather_aug: negative row count");
    LIDOG_REQUIRE(n_target + n_take < (int64_t)INT32_MAX, "lidog_mix_gather_aug: %lld rows out of range",
                  (long long)(n_target + n_take));
    LIDOG_REQUIRE(n_cols >= 0 && n_cols <= MIX_MAX_COLS, "lidog_mix_gather_aug: %d columns (at most %d)", n_cols,
                  MIX_MAX_COLS);
    LIDOG_REQUIRE(n_slots >= 0 && n_slots <= MIX_MAX_SLOTS, "lidog_mix_gather_aug: %d slots (at most %d)", n_slots,
                  MIX_MAX_SLOTS);
    LIDOG_REQUIRE(n_take == 0 || (n_slots >= 1 && n_source >= 1 && rows && slot_start && take_start),
                  "lidog_mix_gather_aug: class rows need 1..%d slots, rows, slot_start and take_start", MIX_MAX_SLOTS);
    LIDOG_REQUIRE(n_ops >= 0 && n_ops <= AUG_MAX_OPS, "lidog_mix_gather_aug: %d operations (at most %d)", n_ops,
                  AUG_MAX_OPS);
    LIDOG_REQUIRE(n_ops == 0 || n_take == 0 || (op_kinds_host && slot_params),
                  "lidog_mix_gather_aug: operations missing");
    LIDOG_REQUIRE(qx > 0 && qy > 0 && qz > 0, "lidog_mix_gather_aug: voxel size must be positive");
    MixAugKinds kinds = {};
    kinds.n = n_take ? n_ops : 0;
    for (int o = 0; o < kinds.n; ++o) {
        LIDOG_REQUIRE(op_kinds_host[o] == AUG_ROTATION || op_kinds_host[o] == AUG_SCALE,
                      "lidog_mix_gather_aug: operation %d of kind %d (0 rotation, 1 scale)", o, op_kinds_host[o]);
        kinds.kind[o] = op_kinds_host[o];
    }
    MixCols cols = {};
    cols.n = n_cols;
    for (int k = 0; k < n_cols; ++k) {
        cols.t[k] = (const uint32_t *)cols_host[3 * k];
        cols.s[k] = (const uint32_t *)cols_host[3 * k + 1];
        cols.o[k] = (uint32_t *)cols_host[3 * k + 2];
        cols.words[k] = col_words_host[k];
        LIDOG_REQUIRE(cols.words[k] >= 0, "lidog_mix_gather_aug: column %d has %d words", k, cols.words[k]);
    }
    const int64_t total = n_target + n_take;
    if (total == 0) return 0;
    LIDOG_REQUIRE(rows_out && (n_target == 0 || coords_t), "lidog_mix_gather_aug: an input or output array is missing");
    k_mix_gather_aug<<<(unsigned)cdiv64(total, MIX_THREADS), MIX_THREADS, 0, st>>>(
        coords_t, n_target, coords_s, n_source, rows, slot_start, perm, take_start, n_take ? n_slots : 0, n_take,
        voxel_size, kinds, slot_params, f64, qx, qy, qz, (int4 *)rows_out, cols);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
