// Sensor-aware scan mixing: PolarMix (Xiao et al., NeurIPS 2022: an azimuth sector swapped between two scans, rotated
// copies of the instance classes pasted) and LaserMix (Kong et al., CVPR 2023: the two scans interleaved by inclination
// band).  Neither is in the reference; include/lidog_amd.h states both operations in exact arithmetic.  Three steps:
//   k_sensormix_keys     one int32 key per row of both scans (sector bit, band, instance bit), from the voxel centre in
//                        doubled integer units; no atan2 / sqrt / sin / cos on the device
//   lidog_sensormix_select   the kept base rows, the taken donor rows and the pasted donor rows, each ascending: three
//                        ordered selections of prims.hip over a 32-entry key table
//   k_sensormix_gather   the merged voxel rows and columns in one launch, pasted copies rotated about z
// No position comes from an atomic: the same bytes on every run.
#include "prims.h"

#define SMIX_THREADS 256
#define SMIX_MAX_BOUNDS 7
#define SMIX_MAX_COPIES 8
#define SMIX_MAX_COLS 6
#define SMIX_KEYS 32            // distinct key values: 1 + 3 + 1 bits
#define SMIX_LIMIT (1 << 24)    // |c| < 2^24: X*X + Y*Y and Z*Z are exact in int64 and in float64

struct SmixBounds {
    double t2[SMIX_MAX_BOUNDS];
    int32_t neg[SMIX_MAX_BOUNDS];
    int32_t n;
};

// ------------------------------------------------------------------ keys
// Every product and difference below is rounded on its own (__dmul_rn / __dsub_rn are never contracted): a fused
// multiply-add decides rows on a boundary differently.
__device__ __forceinline__ int smix_key(int32_t x, int32_t y, int32_t z, int32_t label, double ax, double ay, double bx,
                                        double by, int32_t wide, const SmixBounds &bd, uint32_t instance_mask) {
    const int64_t X = 2 * (int64_t)x + 1, Y = 2 * (int64_t)y + 1, Z = 2 * (int64_t)z + 1;
    const double Xd = (double)X, Yd = (double)Y;
    const double sa = __dsub_rn(__dmul_rn(ax, Yd), __dmul_rn(ay, Xd));
    const double sb = __dsub_rn(__dmul_rn(bx, Yd), __dmul_rn(by, Xd));
    const bool in = wide ? (sa >= 0.0 || sb < 0.0) : (sa >= 0.0 && sb < 0.0);
    const double zz = (double)(Z * Z), rr = (double)(X * X + Y * Y);
    int band = 0;
#pragma unroll
    for (int j = 0; j < SMIX_MAX_BOUNDS; ++j) {
        if (j < bd.n) {
            const double lim = __dmul_rn(bd.t2[j], rr);
            band += bd.neg[j] ? (Z > 0 || zz <= lim) : (Z > 0 && zz >= lim);
        }
    }
    const bool inst = label >= 0 && label < 32 && ((instance_mask >> label) & 1u);
    return (in ? 1 : 0) | (band << 1) | (inst ? 16 : 0);
}

// row r < n0: row r of scan 0; else row r - n0 of scan 1.  A coordinate outside the range: info[0] = 1 (every such
// thread stores the same word) and the row's key is left alone.
__global__ __launch_bounds__(SMIX_THREADS) void k_sensormix_keys(
    const int32_t *__restrict__ coords0, const int32_t *__restrict__ labels0, int64_t n0,
    const int32_t *__restrict__ coords1, const int32_t *__restrict__ labels1, int64_t n1, double ax, double ay,
    double bx, double by, int32_t wide, SmixBounds bd, uint32_t instance_mask, int32_t *__restrict__ keys,
    int32_t *__restrict__ info) {
    const int64_t r = (int64_t)blockIdx.x * SMIX_THREADS + threadIdx.x;
    if (r >= n0 + n1) return;
    const bool first = r < n0;
    const int64_t i = first ? r : r - n0;
    const int32_t *c = (first ? coords0 : coords1) + 3 * i;
    const int32_t x = c[0], y = c[1], z = c[2];
    if (x <= -SMIX_LIMIT || x >= SMIX_LIMIT || y <= -SMIX_LIMIT || y >= SMIX_LIMIT || z <= -SMIX_LIMIT ||
        z >= SMIX_LIMIT) {
        info[0] = 1;
        return;
    }
    const int32_t *lab = first ? labels0 : labels1;
    keys[r] = smix_key(x, y, z, lab ? lab[i] : -1, ax, ay, bx, by, wide, bd, instance_mask);
}

extern "C" int lidog_sensormix_keys(const int32_t *coords0, const int32_t *labels0, int64_t n0,
                                    const int32_t *coords1, const int32_t *labels1, int64_t n1, double ax, double ay,
                                    double bx, double by, int32_t wide, const double *t2_host, const int32_t *neg_host,
                                    int32_t n_bounds, uint32_t instance_mask, int32_t *keys, int32_t *info,
                                    void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n0 >= 0 && n1 >= 0 && n0 + n1 < (int64_t)INT32_MAX, "lidog_sensormix_keys: n0 = %lld, n1 = %lld",
                  (long long)n0, (long long)n1);
    LIDOG_REQUIRE(n_bounds >= 0 && n_bounds <= SMIX_MAX_BOUNDS, "lidog_sensormix_keys: %d boundaries (at most %d)",
                  n_bounds, SMIX_MAX_BOUNDS);
    LIDOG_REQUIRE(n_bounds == 0 || (t2_host && neg_host), "lidog_sensormix_keys: the boundary tables are missing");
    LIDOG_REQUIRE(info, "lidog_sensormix_keys: info is missing");
    LIDOG_REQUIRE((n0 == 0 || coords0) && (n1 == 0 || coords1) && (n0 + n1 == 0 || keys),
                  "lidog_sensormix_keys: an input or output array is missing");
    LIDOG_REQUIRE(ax == ax && ay == ay && bx == bx && by == by, "lidog_sensormix_keys: a direction is NaN");
    SmixBounds bd = {};
    bd.n = n_bounds;
    for (int j = 0; j < n_bounds; ++j) {
        LIDOG_REQUIRE(t2_host[j] >= 0.0, "lidog_sensormix_keys: t2[%d] = %g is no square", j, t2_host[j]);
        bd.t2[j] = t2_host[j];
        bd.neg[j] = neg_host[j] != 0;
    }
    LIDOG_CHECK_HIP(hipMemsetAsync(info, 0, sizeof(int32_t), st));
    const int64_t n = n0 + n1;
    if (n == 0) return 0;
    k_sensormix_keys<<<(unsigned)cdiv64(n, SMIX_THREADS), SMIX_THREADS, 0, st>>>(
        coords0, labels0, n0, coords1, labels1, n1, ax, ay, bx, by, wide, bd, instance_mask, keys, info);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ the three ordered selections
// table[t * 32 + k] = slot 0 when key k is in set t, else -1 (not taken): the slot_of_key tables of lidog_split_rows
__global__ void k_sensormix_tables(uint32_t keep, uint32_t take, uint32_t paste, int32_t *__restrict__ table) {
    const int t = threadIdx.x / SMIX_KEYS, k = threadIdx.x % SMIX_KEYS;
    const uint32_t m = t == 0 ? keep : (t == 1 ? take : paste);
    table[threadIdx.x] = ((m >> k) & 1u) ? 0 : -1;
}

#define SMIX_TABLE_INTS 128   // 3 * 32 entries, the split's workspace after them

extern "C" int64_t lidog_sensormix_select_ws(int64_t n_base, int64_t n_donor) {
    const int64_t a = lidog_split_ws_ints(n_base, 1), b = lidog_split_ws_ints(n_donor, 1);
    return SMIX_TABLE_INTS + (a > b ? a : b);
}

extern "C" int lidog_sensormix_select(const int32_t *keys_base, int64_t n_base, const int32_t *keys_donor,
                                      int64_t n_donor, uint32_t keep_keys, uint32_t take_keys, uint32_t paste_keys,
                                      int32_t *rows_keep, int32_t *rows_take, int32_t *rows_paste, int32_t *sizes,
                                      int32_t *ws, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n_base >= 0 && n_donor >= 0 && n_base < (int64_t)INT32_MAX && n_donor < (int64_t)INT32_MAX,
                  "lidog_sensormix_select: n_base = %lld, n_donor = %lld", (long long)n_base, (long long)n_donor);
    LIDOG_REQUIRE(sizes && ws, "lidog_sensormix_select: sizes or the workspace is missing");
    LIDOG_REQUIRE((n_base == 0 || (keys_base && rows_keep)) && (n_donor == 0 || (keys_donor && rows_take && rows_paste)),
                  "lidog_sensormix_select: an input or output array is missing");
    k_sensormix_tables<<<1, 3 * SMIX_KEYS, 0, st>>>(keep_keys, take_keys, paste_keys, ws);
    LIDOG_LAUNCH_CHECK();
    int32_t *split_ws = ws + SMIX_TABLE_INTS;
    // an empty set launches nothing: its (start, size) pair is zeroed by the split itself
    if (lidog_split_rows(keys_base, n_base, ws, SMIX_KEYS, keep_keys ? 1 : 0, rows_keep, sizes, split_ws, st)) return 1;
    if (!keep_keys) LIDOG_CHECK_HIP(hipMemsetAsync(sizes, 0, 2 * sizeof(int32_t), st));
    if (lidog_split_rows(keys_donor, n_donor, ws + SMIX_KEYS, SMIX_KEYS, take_keys ? 1 : 0, rows_take, sizes + 2,
                         split_ws, st))
        return 1;
    if (!take_keys) LIDOG_CHECK_HIP(hipMemsetAsync(sizes + 2, 0, 2 * sizeof(int32_t), st));
    if (lidog_split_rows(keys_donor, n_donor, ws + 2 * SMIX_KEYS, SMIX_KEYS, paste_keys ? 1 : 0, rows_paste, sizes + 4,
                         split_ws, st))
        return 1;
    if (!paste_keys) LIDOG_CHECK_HIP(hipMemsetAsync(sizes + 4, 0, 2 * sizeof(int32_t), st));
    return 0;
}

// ------------------------------------------------------------------ the merged rows
struct SmixCols {
    const uint32_t *b[SMIX_MAX_COLS];   // base rows
    const uint32_t *d[SMIX_MAX_COLS];   // donor rows
    uint32_t *o[SMIX_MAX_COLS];         // merged rows
    int32_t words[SMIX_MAX_COLS];       // 32-bit words per row
    int32_t n;
};

struct SmixCopies {
    double c[SMIX_MAX_COPIES], s[SMIX_MAX_COPIES];
    int32_t ident[SMIX_MAX_COPIES];     // (c, s) == (1, 0): the integer voxel is copied
    int32_t n;
};

// merged row r: base row rows_keep[r] for r < n_keep; donor row rows_take[r - n_keep] for the next n_take; then copy k
// of donor row rows_paste[j] at n_keep + n_take + k * n_paste + j.  A list entry outside its scan is clamped: nothing
// outside the two scans is read.
__global__ __launch_bounds__(SMIX_THREADS) void k_sensormix_gather(
    const int32_t *__restrict__ coords_base, int64_t n_base, const int32_t *__restrict__ coords_donor, int64_t n_donor,
    const int32_t *__restrict__ rows_keep, int64_t n_keep, const int32_t *__restrict__ rows_take, int64_t n_take,
    const int32_t *__restrict__ rows_paste, int64_t n_paste, SmixCopies cp, int4 *__restrict__ rows_out, SmixCols cols) {
    const int64_t r = (int64_t)blockIdx.x * SMIX_THREADS + threadIdx.x;
    if (r >= n_keep + n_take + (int64_t)cp.n * n_paste) return;
    const bool base = r < n_keep;
    int copy = -1;
    int64_t src;
    if (base) {
        src = rows_keep[r];
    } else if (r < n_keep + n_take) {
        src = rows_take[r - n_keep];
    } else {
        const int64_t j = r - n_keep - n_take;
        copy = (int)(j / n_paste);
        src = rows_paste[j - (int64_t)copy * n_paste];
    }
    const int64_t n_src = base ? n_base : n_donor;
    src = src < 0 ? 0 : (src >= n_src ? n_src - 1 : src);
    const int32_t *c = (base ? coords_base : coords_donor) + 3 * src;
    int32_t x = c[0], y = c[1];
    const int32_t z = c[2];
    if (copy >= 0 && !cp.ident[copy]) {
        double cc = 1.0, ss = 0.0;
#pragma unroll
        for (int k = 0; k < SMIX_MAX_COPIES; ++k)   // no dynamic index into the argument struct
            if (k == copy) {
                cc = cp.c[k];
                ss = cp.s[k];
            }
        const double U = (double)x + 0.5, V = (double)y + 0.5;
        const double xr = __dsub_rn(__dmul_rn(cc, U), __dmul_rn(ss, V));
        const double yr = __dadd_rn(__dmul_rn(ss, U), __dmul_rn(cc, V));
        x = lidog_voxel_coord(floor(xr));
        y = lidog_voxel_coord(floor(yr));
    }
    rows_out[r] = make_int4(0, x, y, z);
    for (int k = 0; k < cols.n; ++k) {
        const int wd = cols.words[k];
        const uint32_t *in = (base ? cols.b[k] : cols.d[k]) + src * wd;
        uint32_t *out = cols.o[k] + r * wd;
        for (int q = 0; q < wd; ++q) out[q] = in[q];
    }
}

extern "C" int lidog_sensormix_gather(const int32_t *coords_base, int64_t n_base, const int32_t *coords_donor,
                                      int64_t n_donor, const int32_t *rows_keep, int64_t n_keep,
                                      const int32_t *rows_take, int64_t n_take, const int32_t *rows_paste,
                                      int64_t n_paste, const double *cs_host, int32_t n_copies, int32_t *rows_out,
                                      int32_t n_cols, void *const *cols_host, const int32_t *col_words_host,
                                      void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n_base >= 0 && n_donor >= 0 && n_keep >= 0 && n_take >= 0 && n_paste >= 0,
                  "lidog_sensormix_gather: negative row count");
    LIDOG_REQUIRE(n_keep <= n_base && n_take <= n_donor && n_paste <= n_donor,
                  "lidog_sensormix_gather: %lld / %lld / %lld rows listed of scans with %lld and %lld rows",
                  (long long)n_keep, (long long)n_take, (long long)n_paste, (long long)n_base, (long long)n_donor);
    LIDOG_REQUIRE(n_copies >= 0 && n_copies <= SMIX_MAX_COPIES, "lidog_sensormix_gather: %d copies (at most %d)",
                  n_copies, SMIX_MAX_COPIES);
    LIDOG_REQUIRE(n_copies == 0 || cs_host, "lidog_sensormix_gather: the (c, s) table is missing");
    LIDOG_REQUIRE(n_cols >= 0 && n_cols <= SMIX_MAX_COLS, "lidog_sensormix_gather: %d columns (at most %d)", n_cols,
                  SMIX_MAX_COLS);
    SmixCopies cp = {};
    cp.n = n_paste ? n_copies : 0;
    for (int k = 0; k < cp.n; ++k) {
        cp.c[k] = cs_host[2 * k];
        cp.s[k] = cs_host[2 * k + 1];
        LIDOG_REQUIRE(cp.c[k] == cp.c[k] && cp.s[k] == cp.s[k], "lidog_sensormix_gather: copy %d has a NaN", k);
        cp.ident[k] = cp.c[k] == 1.0 && cp.s[k] == 0.0;
    }
    SmixCols cols = {};
    cols.n = n_cols;
    for (int k = 0; k < n_cols; ++k) {
        cols.b[k] = (const uint32_t *)cols_host[3 * k];
        cols.d[k] = (const uint32_t *)cols_host[3 * k + 1];
        cols.o[k] = (uint32_t *)cols_host[3 * k + 2];
        cols.words[k] = col_words_host[k];
        LIDOG_REQUIRE(cols.words[k] >= 0, "lidog_sensormix_gather: column %d has %d words", k, cols.words[k]);
    }
    const int64_t total = n_keep + n_take + (int64_t)cp.n * n_paste;
    LIDOG_REQUIRE(total < (int64_t)INT32_MAX, "lidog_sensormix_gather: %lld rows out of range", (long long)total);
    if (total == 0) return 0;
    LIDOG_REQUIRE(rows_out && (n_keep == 0 || (coords_base && rows_keep)) && (n_take == 0 || (coords_donor && rows_take)) &&
                      (cp.n * n_paste == 0 || (coords_donor && rows_paste)),
                  "lidog_sensormix_gather: an input or output array is missing");
    k_sensormix_gather<<<(unsigned)cdiv64(total, SMIX_THREADS), SMIX_THREADS, 0, st>>>(
        coords_base, n_base, coords_donor, n_donor, rows_keep, n_keep, rows_take, n_take, rows_paste, n_paste, cp,
        (int4 *)rows_out, cols);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
