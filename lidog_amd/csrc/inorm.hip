// Instance normalisation of sparse feature matrices (MinkowskiInstanceNorm, ME 0.5.4) and the IBN block's fused
// BatchNorm | InstanceNorm + ReLU pass.  Reference call sites: utils/models/minkunet_ibn.py:26 (in_norm1) and :38-40
// (bn_out = bn_norm1(out); in_out = in_norm1(out); ME.cat(bn_out, in_out) -> ReLU).
//
// Instance norm normalises every channel PER SCAN: for batch index b and channel c,
//   mean[b, c] = sum_{rows of b} x / n_b,  var[b, c] = sum (x - mean)^2 / n_b (biased),
//   y = (x - mean[b, c]) * (var + eps)^-1/2 * w[c] + bias[c].
// The statistics are segmented sums keyed on the batch column of the coordinate map:
//   segments   a stable ordering of the map's rows by batch id (lidog_group_by_key of prims.hip) + seg_off[B + 1];
//              built once per coordinate map by the caller and kept with it
//   reduce     per-(b, c) sums in double over each segment; workgroup w owns a contiguous range of SORTED rows and
//              writes one partial row of 2 B C columns (zeros for the scans it does not touch); the two-level
//              last-workgroup tail of stats_tail.h adds the rows in a fixed order and finalises per (b, c): no float
//              atomics, the same bits on every run
//   apply      y = (x - mean[b]) * invstd[b] * w + bias, b read from the per-row batch ids
// The backward pass is the standard normalisation gradient per (b, c): a reduce pass (sum dy, sum dy * xhat) that also
// writes dweight / dbias [C] (sums over b in ascending order) and per-(b, c) coefficients m0 = sum dy / n_b,
// m1 = sum dy xhat / n_b; then dx = (dy - m0 - xhat * m1) * (invstd * w).
//
// [rows, C] with C % 4 == 0 streams float4 rows as bn.hip does; any other C takes plain scalar kernels (the module is
// public; no performance target there).
#include "bn_math.h"
#include "common.h"
#include "mixstyle.h"
#include "prims.h"
#include "stats_tail.h"

#define IN_MAX_BLOCKS 256       // workgroups (= partial rows) of a segmented reduction
#define IN_LDS_DOUBLES 4096     // LDS of a reduction workgroup: the row reduction, then the final per-(b, c) sums

// the float4 path: C4 <= 256 lanes per row, and the final 2 B C sums of the backward reduction fit in LDS
static bool in_vector_path(int C, int B) { return C % 4 == 0 && C / 4 <= 256 && 2 * (int64_t)B * C <= IN_LDS_DOUBLES; }

// ------------------------------------------------------------------ segments
__global__ __launch_bounds__(256) void k_in_keys(const int32_t *__restrict__ coords, int64_t n, int32_t *__restrict__ bid,
                                                 uint32_t *__restrict__ keys, int32_t *__restrict__ rows) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int32_t b = coords[r * 4];
    bid[r] = b;
    keys[r] = (uint32_t)b;
    rows[r] = (int32_t)r;
}

// batch ids are below 4096: at most the passes of a 12-bit key, which size the workspace
extern "C" int64_t lidog_in_segments_ws(int64_t n) {
    if (n <= 0) return 256;
    return lidog_group_ws(n, lidog_radix_passes(4095));
}

extern "C" int lidog_in_segments(const int32_t *coords, int64_t n, int32_t B, int32_t *perm, int32_t *seg_off,
                                 int32_t *bid, void *ws, int64_t ws_bytes, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(B >= 0 && B <= 4096 && n >= 0 && n < ((int64_t)1 << 31), "in_segments: 0 <= B <= 4096, n < 2^31");
    LIDOG_REQUIRE(seg_off != nullptr, "in_segments: seg_off [B + 1] required");
    if (n == 0) {
        LIDOG_CHECK_HIP(hipMemsetAsync(seg_off, 0, sizeof(int32_t) * (B + 1), st));
        return 0;
    }
    LIDOG_REQUIRE(coords && perm && bid && ws, "in_segments: coords, perm, bid and the workspace are required");
    LIDOG_REQUIRE(ws_bytes >= lidog_in_segments_ws(n), "in_segments: workspace too small");
    // seg_off[b] = first sorted position whose batch id is >= b (b = 0 .. B): empty scans get empty ranges
    const int passes = lidog_radix_passes(B - 1);   // the ids of B scans
    const LidogGroupBufs g = lidog_group_bufs(ws, n, passes, perm);
    k_in_keys<<<(unsigned)cdiv64(n, 256), 256, 0, st>>>(coords, n, bid, g.ka, g.va);
    return lidog_group_by_key(g, n, passes, B, seg_off, st);
}

// ------------------------------------------------------------------ segmented reductions
// What the last workgroup does with the per-(b, c) sums.  MODE 0 (x, x^2): mean / invstd.  MODE 1 (dy, dy * xhat):
// coef [2][B][C] = (sum dy / n_b, sum dy xhat / n_b) and dw / db [C] = sums over b, ascending.  MODE 2 (x, x^2, the
// terms of MODE 0): MixStyle's mean / sig and, behind a barrier, its three mixed tables (mixstyle.h).
struct InFinish {
    const int32_t *seg_off;
    int B, C;
    float eps;
    float *mean, *invstd;    // MODE 0
    float *coef, *dw, *db;   // MODE 1
    MsMix mix;               // MODE 2 (with mean)
};

__device__ __forceinline__ void in_finalize(int mode, const InFinish &f, int j, double s0, double s1) {
    const int b = j / f.C;
    const double cnt = (double)(f.seg_off[b + 1] - f.seg_off[b]);
    if (mode == 0) {
        double m = 0.0, var = 0.0;
        if (cnt > 0) {   // a scan with no rows in this map: finite placeholders, no row reads them
            m = s0 / cnt;
            var = s1 / cnt - m * m;
            if (var < 0) var = 0;
        }
        f.mean[j] = (float)m;
        f.invstd[j] = (float)(1.0 / sqrt(var + (double)f.eps));
    } else {
        const int BC = f.B * f.C;
        f.coef[j] = cnt > 0 ? (float)(s0 / cnt) : 0.f;
        f.coef[BC + j] = cnt > 0 ? (float)(s1 / cnt) : 0.f;
    }
}

// MODE 2, phase one: the moments of (b, c) = j in double into mom [2][B C], rounded once into mean / sig
__device__ __forceinline__ void in_finalize_ms(const InFinish &f, int j, double s0, double s1, double *mom) {
    const int b = j / f.C;
    double mu, sig;
    ms_moments(s0, s1, (double)(f.seg_off[b + 1] - f.seg_off[b]), (double)f.eps, mu, sig);
    mom[j] = mu;
    mom[f.B * f.C + j] = sig;
    f.mean[j] = (float)mu;
    f.mix.sig[j] = (float)sig;
}

// largest b in [0, B) with seg_off[b] <= v (the scan that holds sorted row v)
__device__ __forceinline__ int in_seg_of(const int32_t *__restrict__ seg_off, int B, int64_t v) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_off[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// MODE 0: (x, x * x).  MODE 1: (g, g * xhat), g = dy masked by the ReLU bits when given.  dy is read at row * dy_s4 + c4
// (float4 units) and the mask bit at float4 number row * bits_s4 + bits_o4 + c4 of the bit layout of lidog_bn_apply_bits:
// the same kernel serves the stand-alone instance norm (dy [n, C]) and the IN half of the IBN block (dy [n, 2C]).
template <int MODE>
__global__ __launch_bounds__(256) void k_in_reduce4(const float4 *__restrict__ x, const float4 *__restrict__ dy, int dy_s4,
                                                    const uint32_t *__restrict__ bits, int bits_s4, int bits_o4,
                                                    int64_t n, int C4, const int32_t *__restrict__ perm,
                                                    const float *__restrict__ mean, const float *__restrict__ invstd,
                                                    int64_t per_wg, StatsTail tail, InFinish fin) {
    __shared__ double red[IN_LDS_DOUBLES];
    const int C = C4 * 4, B = fin.B, BC = B * C;
    const int RB = 256 / C4;
    const int tid = threadIdx.x;
    const int r = tid / C4, c4 = tid % C4;
    const bool active = r < RB;
    const int32_t *seg_off = fin.seg_off;
    const int64_t lo = (int64_t)blockIdx.x * per_wg, hi = lo + per_wg < n ? lo + per_wg : n;
    const int b0 = in_seg_of(seg_off, B, lo), b1 = in_seg_of(seg_off, B, hi - 1);
    double *prow = tail.partial + (size_t)blockIdx.x * 2 * BC;
    for (int j = tid; j < 2 * BC; j += 256) {   // the scans this workgroup has no rows of
        const int bj = (j < BC ? j : j - BC) / C;
        if (bj < b0 || bj > b1) lidog_store_sc1(prow + j, 0.0);
    }
    for (int b = b0; b <= b1; ++b) {
        const int64_t s = seg_off[b] > lo ? seg_off[b] : lo, e = seg_off[b + 1] < hi ? seg_off[b + 1] : hi;
        double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        float m[4] = {0, 0, 0, 0}, is[4] = {1, 1, 1, 1};
        if (MODE == 1 && active) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { m[j] = mean[b * C + c4 * 4 + j]; is[j] = invstd[b * C + c4 * 4 + j]; }
        }
        if (active) {
            // 4 rows in flight per lane; the last row of the range stands in for rows past it (masked afterwards)
            for (int64_t row0 = s + r; row0 < e; row0 += 4 * RB) {
                float4 v[4], g[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    int64_t row = row0 + u * RB;
                    row = row < e ? row : e - 1;
                    const int64_t pr = perm[row];
                    v[u] = x[pr * C4 + c4];
                    g[u] = MODE == 1 ? dy[pr * dy_s4 + c4] : make_float4(0, 0, 0, 0);
                    if (MODE == 1 && bits)
                        g[u] = bn_relu_mask4(g[u], lidog_relu_bits_as_float4(bits, pr * bits_s4 + bits_o4 + c4));
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (row0 + u * RB >= e) continue;
                    bn_red_terms4<MODE == 1>(v[u], g[u], g[u], false, bn_f4(m), bn_f4(is), a);   // g is masked already
                }
            }
        }
        lidog_stats_wg_reduce(red, tid, RB, C4, c4, active && r == 0, a);
        if (active && r == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lidog_store_sc1(prow + b * C + c4 * 4 + j, a[j]);
                lidog_store_sc1(prow + BC + b * C + c4 * 4 + j, a[4 + j]);
            }
        }
        __syncthreads();   // red is rewritten by the next scan
    }
    lidog_stats_tail_rows_with(tail, (int)blockIdx.x, (int)gridDim.x, 1, [&](const double *grows, int ng) {
        for (int j = tid; j < BC; j += 256) {
            const double s0 = lidog_rows_sum_sc1(grows, 0, ng, 2 * BC, j);
            const double s1 = lidog_rows_sum_sc1(grows, 0, ng, 2 * BC, BC + j);
            if (MODE == 2) in_finalize_ms(fin, j, s0, s1, red);
            else in_finalize(MODE, fin, j, s0, s1);
            if (MODE == 1) { red[j] = s0; red[BC + j] = s1; }
        }
        if (MODE == 2) {   // every scan's moments are in LDS before any scan reads its partner's
            __syncthreads();
            for (int j = tid; j < BC; j += 256) ms_tables(fin.mix, seg_off, red, B, C, j);
        }
        if (MODE == 1) {
            __syncthreads();
            for (int c = tid; c < C; c += 256) {
                double s0 = 0.0, s1 = 0.0;
                for (int b = 0; b < B; ++b) { s0 += red[b * C + c]; s1 += red[BC + b * C + c]; }
                fin.db[c] = (float)s0;
                fin.dw[c] = (float)s1;
            }
        }
    });
}

// C % 4 != 0 (or sums that do not fit the LDS of the float4 path): one workgroup per (b, c), strided rows
template <int MODE>
__global__ __launch_bounds__(256) void k_in_reduce_scalar(const float *__restrict__ x, const float *__restrict__ dy,
                                                          int C, const int32_t *__restrict__ perm,
                                                          const float *__restrict__ mean,
                                                          const float *__restrict__ invstd, double *__restrict__ sums,
                                                          InFinish fin) {
    __shared__ double s_red[2][4];
    const int j = blockIdx.x, b = j / C, c = j % C;
    const int64_t s = fin.seg_off[b], e = fin.seg_off[b + 1];
    const float m = MODE == 1 ? mean[j] : 0.f, is = MODE == 1 ? invstd[j] : 1.f;
    double t0 = 0, t1 = 0;
    for (int64_t i = s + threadIdx.x; i < e; i += 256) {
        const int64_t pr = perm[i];
        bn_red_terms<MODE == 1>(x[pr * C + c], MODE == 1 ? dy[pr * C + c] : 0.f, 1.f, false, m, is, t0, t1);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        t0 += __shfl_down(t0, d);
        t1 += __shfl_down(t1, d);
    }
    if ((threadIdx.x & 63) == 0) { s_red[0][threadIdx.x >> 6] = t0; s_red[1][threadIdx.x >> 6] = t1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s0 = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
        const double s1 = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
        if (MODE == 2) in_finalize_ms(fin, j, s0, s1, sums);
        else in_finalize(MODE, fin, j, s0, s1);
        if (MODE == 1) { sums[j] = s0; sums[(int64_t)fin.B * C + j] = s1; }
    }
}

// MODE 2 on the scalar path, phase two: the moments of every (b, c) are in `mom` (the launch in front of this one)
__global__ __launch_bounds__(256) void k_in_ms_tables(const double *__restrict__ mom, InFinish fin) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < fin.B * fin.C) ms_tables(fin.mix, fin.seg_off, mom, fin.B, fin.C, j);
}

__global__ void k_in_param_grads(const double *__restrict__ sums, int B, int C, float *__restrict__ dw,
                                 float *__restrict__ db) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0, s1 = 0.0;
    for (int b = 0; b < B; ++b) { s0 += sums[b * C + c]; s1 += sums[(int64_t)B * C + b * C + c]; }
    db[c] = (float)s0;
    dw[c] = (float)s1;
}

static int64_t in_per_wg(int64_t n, int C4) {
    const int64_t RB = 256 / C4;
    int64_t per = cdiv64(n, IN_MAX_BLOCKS);
    return per < 4 * RB ? 4 * RB : per;
}

extern "C" int64_t lidog_in_reduce_ws(int32_t B, int32_t C) {
    const int64_t wide = (int64_t)2 * B * C;
    if (in_vector_path(C, B)) return (IN_MAX_BLOCKS + cdiv64(IN_MAX_BLOCKS, STATS_GROUP)) * wide;
    return wide;
}

template <int MODE>
static int in_reduce(const float *x, const float *dy, int dy_s4, const uint32_t *bits, int bits_s4, int bits_o4,
                     int64_t n, int C, int B, const int32_t *perm, const float *mean, const float *invstd, double *ws,
                     const InFinish &fin, hipStream_t st) {
    if (B == 0 || C == 0) return 0;
    LIDOG_REQUIRE(ws != nullptr && fin.seg_off != nullptr && (n == 0 || perm != nullptr),
                  "instance norm reduce: seg_off, perm and a workspace of lidog_in_reduce_ws(B, C) doubles required");
    if (n > 0 && in_vector_path(C, B)) {
        const int C4 = C / 4;
        const int64_t per = in_per_wg(n, C4);
        const int nb = (int)cdiv64(n, per);
        unsigned *tickets = lidog_stats_tickets(st);
        if (!tickets) return 1;
        StatsTail tail{ws, tickets, nullptr, 0.0, B * C, BnFinish{}};
        k_in_reduce4<MODE><<<(unsigned)nb, 256, 0, st>>>((const float4 *)x, (const float4 *)dy, dy_s4, bits, bits_s4,
                                                          bits_o4, n, C4, perm, mean, invstd, per, tail, fin);
        if (hipPeekAtLastError() != hipSuccess) lidog_stats_tickets_reset(st);
    } else {
        LIDOG_REQUIRE(bits == nullptr && (MODE != 1 || dy_s4 == C / 4 || C % 4 != 0),
                      "instance norm reduce: strided / masked dy only on the float4 path");
        k_in_reduce_scalar<MODE><<<(unsigned)(B * C), 256, 0, st>>>(x, dy, C, perm, mean, invstd, ws, fin);
        if (MODE == 1) k_in_param_grads<<<(C + 127) / 128, 128, 0, st>>>(ws, B, C, fin.dw, fin.db);
        if (MODE == 2) k_in_ms_tables<<<(unsigned)cdiv64((int64_t)B * C, 256), 256, 0, st>>>(ws, fin);
    }
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_in_stats(const float *x, int64_t n, int32_t C, int32_t B, const int32_t *perm,
                              const int32_t *seg_off, float eps, float *mean, float *invstd, double *ws, void *stream) {
    LIDOG_REQUIRE(mean && invstd, "in_stats: mean / invstd [B, C] required");
    InFinish fin{seg_off, B, C, eps, mean, invstd, nullptr, nullptr, nullptr};
    return in_reduce<0>(x, nullptr, 0, nullptr, 0, 0, n, C, B, perm, nullptr, nullptr, ws, fin, (hipStream_t)stream);
}

extern "C" int lidog_in_bwd_reduce(const float *dy, const float *x, int64_t n, int32_t C, int32_t B,
                                   const int32_t *perm, const int32_t *seg_off, const float *mean, const float *invstd,
                                   double *ws, float *coef, float *dw, float *db, void *stream) {
    LIDOG_REQUIRE(coef && dw && db, "in_bwd_reduce: coef [2, B, C], dw [C] and db [C] required");
    InFinish fin{seg_off, B, C, 0.f, nullptr, nullptr, coef, dw, db};
    return in_reduce<1>(x, dy, C / 4, nullptr, 0, 0, n, C, B, perm, mean, invstd, ws, fin, (hipStream_t)stream);
}

int lidog_in_reduce_mixstyle(const float *x, int64_t n, int C, int B, const int32_t *perm, const int32_t *seg_off,
                             float eps, float *mean, const MsMix &mix, double *ws, hipStream_t st) {
    InFinish fin{seg_off, B, C, eps, mean, nullptr, nullptr, nullptr, nullptr, mix};
    return in_reduce<2>(x, nullptr, 0, nullptr, 0, 0, n, C, B, perm, nullptr, nullptr, ws, fin, st);
}

// ------------------------------------------------------------------ elementwise passes
static unsigned in_grid(int64_t n) {
    const int64_t g = cdiv64(n, 256);
    return (unsigned)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

__global__ __launch_bounds__(256) void k_in_apply4(const float4 *__restrict__ x, int64_t total4, int C4,
                                                   const int32_t *__restrict__ bid, const float4 *__restrict__ mean,
                                                   const float4 *__restrict__ invstd, const float4 *__restrict__ w,
                                                   const float4 *__restrict__ b, float4 *__restrict__ y) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / C4;
        const int c4 = (int)(i - row * C4);
        const int64_t k = (int64_t)bid[row] * C4 + c4;
        y[i] = bn_affine4(x[i], mean[k], invstd[k], w[c4], b[c4]);
    }
}

__global__ __launch_bounds__(256) void k_in_apply(const float *__restrict__ x, int64_t total, int C,
                                                  const int32_t *__restrict__ bid, const float *__restrict__ mean,
                                                  const float *__restrict__ invstd, const float *__restrict__ w,
                                                  const float *__restrict__ b, float *__restrict__ y) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / C;
        const int c = (int)(i - row * C);
        const int64_t k = (int64_t)bid[row] * C + c;
        y[i] = bn_affine(x[i], mean[k], invstd[k], w[c], b[c]);
    }
}

__global__ __launch_bounds__(256) void k_in_bwd_apply4(const float4 *__restrict__ dy, const float4 *__restrict__ x,
                                                       int64_t total4, int C4, int B, const int32_t *__restrict__ bid,
                                                       const float4 *__restrict__ mean, const float4 *__restrict__ invstd,
                                                       const float4 *__restrict__ w, const float4 *__restrict__ coef,
                                                       float4 *__restrict__ dx) {
    const int64_t BC4 = (int64_t)B * C4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / C4;
        const int c4 = (int)(i - row * C4);
        const int64_t k = (int64_t)bid[row] * C4 + c4;
        const float4 g = dy[i], xv = x[i], mu = mean[k], is = invstd[k], ww = w[c4], m0 = coef[k], m1 = coef[BC4 + k];
        dx[i] = bn_dx_scaled4(g, xv, mu, is, bn_scale4(is, ww), m0, m1);
    }
}

__global__ __launch_bounds__(256) void k_in_bwd_apply(const float *__restrict__ dy, const float *__restrict__ x,
                                                      int64_t total, int C, int B, const int32_t *__restrict__ bid,
                                                      const float *__restrict__ mean, const float *__restrict__ invstd,
                                                      const float *__restrict__ w, const float *__restrict__ coef,
                                                      float *__restrict__ dx) {
    const int64_t BC = (int64_t)B * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / C;
        const int c = (int)(i - row * C);
        const int64_t k = (int64_t)bid[row] * C + c;
        dx[i] = bn_dx_scaled(dy[i], x[i], mean[k], invstd[k], bn_scale(invstd[k], w[c]), coef[k], coef[BC + k]);
    }
}

extern "C" int lidog_in_apply(const float *x, int64_t n, int32_t C, int32_t B, const int32_t *bid, const float *mean,
                              const float *invstd, const float *w, const float *b, float *y, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    (void)B;
    const int64_t total = n * C;
    if (total == 0) return 0;
    if (C % 4 == 0)
        k_in_apply4<<<in_grid(total / 4), 256, 0, st>>>((const float4 *)x, total / 4, C / 4, bid, (const float4 *)mean,
                                                        (const float4 *)invstd, (const float4 *)w, (const float4 *)b,
                                                        (float4 *)y);
    else
        k_in_apply<<<in_grid(total), 256, 0, st>>>(x, total, C, bid, mean, invstd, w, b, y);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_in_bwd_apply(const float *dy, const float *x, int64_t n, int32_t C, int32_t B, const int32_t *bid,
                                  const float *mean, const float *invstd, const float *w, const float *coef, float *dx,
                                  void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = n * C;
    if (total == 0) return 0;
    if (C % 4 == 0)
        k_in_bwd_apply4<<<in_grid(total / 4), 256, 0, st>>>((const float4 *)dy, (const float4 *)x, total / 4, C / 4, B,
                                                            bid, (const float4 *)mean, (const float4 *)invstd,
                                                            (const float4 *)w, (const float4 *)coef, (float4 *)dx);
    else
        k_in_bwd_apply<<<in_grid(total), 256, 0, st>>>(dy, x, total, C, B, bid, mean, invstd, w, coef, dx);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ the IBN block: ReLU(BN(x)) | ReLU(IN(x))
// y [n, 2C]: float4 q = row * 2 C4 + c of y is BatchNorm (c < C4) or instance norm (c >= C4) of x's float4 row * C4 +
// c mod C4, then max(., 0); bits: lidog_bn_apply_bits' layout over y.  The result equals lidog_bn_apply +
// lidog_in_apply + lidog_cat2 + lidog_relu_fwd bit for bit.  The two halves of a row are read by neighbouring lanes: x
// comes from HBM once.
__global__ __launch_bounds__(256) void k_ibn_apply4(const float4 *__restrict__ x, int64_t total4, int C4,
                                                    const float4 *__restrict__ bn_mean,
                                                    const float4 *__restrict__ bn_invstd, const float4 *__restrict__ bn_w,
                                                    const float4 *__restrict__ bn_b, const int32_t *__restrict__ bid,
                                                    const float4 *__restrict__ in_mean,
                                                    const float4 *__restrict__ in_invstd,
                                                    const float4 *__restrict__ in_w, const float4 *__restrict__ in_b,
                                                    float4 *__restrict__ y, uint32_t *__restrict__ bits) {
    const int C8 = 2 * C4;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < total4; base += (int64_t)gridDim.x * 256) {
        const int64_t i = base + threadIdx.x;
        const bool ok = i < total4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) {
            const int64_t row = i / C8;
            const int c = (int)(i - row * C8);
            if (c < C4) {
                v = bn_affine4(x[row * C4 + c], bn_mean[c], bn_invstd[c], bn_w[c], bn_b[c]);
            } else {
                const int c4 = c - C4;
                const int64_t k = (int64_t)bid[row] * C4 + c4;
                v = bn_affine4(x[row * C4 + c4], in_mean[k], in_invstd[k], in_w[c4], in_b[c4]);
            }
            v = bn_res_relu4(v, nullptr, i, 1);
            y[i] = v;
        }
        lidog_relu_bits_store(bits, i, ok, v);
    }
}

// The BatchNorm half's backward reduction, k_colreduce_nc4<1> of bn.hip (no ReLU operand) over the masked BN half of
// dy [n, 2C]: the same grid (lidog_bn_bwd_reduce_blocks), the same rows per lane in the same order, the same LDS
// reduction and tail -- the sums lidog_bn_bwd_reduce computes from ReLU-backward + split2 output, bit for bit.
__global__ __launch_bounds__(256) void k_ibn_bn_reduce4(const float4 *__restrict__ x, const float4 *__restrict__ dy,
                                                        const uint32_t *__restrict__ bits, int64_t n, int C4,
                                                        const float *__restrict__ mean, const float *__restrict__ invstd,
                                                        StatsTail tail) {
    __shared__ double red[256 * 8];
    const int RB = 256 / C4;
    const int tid = threadIdx.x;
    const int r = tid / C4, c4 = tid % C4;
    const bool active = r < RB;
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float m[4] = {0, 0, 0, 0}, is[4] = {1, 1, 1, 1};
    if (active) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { m[j] = mean[c4 * 4 + j]; is[j] = invstd[c4 * 4 + j]; }
        const int64_t step = (int64_t)gridDim.x * RB;
        for (int64_t row0 = (int64_t)blockIdx.x * RB + r; row0 < n; row0 += 4 * step) {
            float4 v[4], g[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                int64_t row = row0 + u * step;
                row = row < n ? row : n - 1;
                v[u] = x[row * C4 + c4];
                g[u] = bn_relu_mask4(dy[row * 2 * C4 + c4], lidog_relu_bits_as_float4(bits, row * 2 * C4 + c4));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool ok = row0 + u * step < n;
                const float4 gg = ok ? g[u] : make_float4(0, 0, 0, 0);
                bn_red_terms4<1>(v[u], gg, gg, false, bn_f4(m), bn_f4(is), a);   // g is masked already
            }
        }
    }
    lidog_stats_wg_reduce(red, tid, RB, C4, c4, active && r == 0, a);
    lidog_stats_tail(tail, active && r == 0, c4, a);
}

// dx = dx_BN + dx_IN from dy [n, 2C] and the mask bits of the forward pass: the sum autograd adds for the two readers
// of x
__global__ __launch_bounds__(256) void k_ibn_bwd_apply4(const float4 *__restrict__ dy, const uint32_t *__restrict__ bits,
                                                        const float4 *__restrict__ x, int64_t total4, int C4, int B,
                                                        const float *__restrict__ bn_mean,
                                                        const float *__restrict__ bn_invstd,
                                                        const float *__restrict__ bn_w, const double *__restrict__ bn_sums,
                                                        double bn_ic, const int32_t *__restrict__ bid,
                                                        const float4 *__restrict__ in_mean,
                                                        const float4 *__restrict__ in_invstd,
                                                        const float4 *__restrict__ in_w, const float4 *__restrict__ coef,
                                                        float4 *__restrict__ dx) {
    __shared__ float4 s_bn[5][256];   // per channel quad: mean, invstd, invstd * w, m0, m1 of the BatchNorm half
    const int C = 4 * C4;
    for (int q = threadIdx.x; q < C4; q += 256) {
        float t[5][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * q + j;
            t[0][j] = bn_mean[c];
            t[1][j] = bn_invstd[c];
            t[2][j] = bn_scale(bn_invstd[c], bn_w[c]);
            t[3][j] = (float)(bn_sums[c] * bn_ic);
            t[4][j] = (float)(bn_sums[C + c] * bn_ic);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) s_bn[k][q] = make_float4(t[k][0], t[k][1], t[k][2], t[k][3]);
    }
    __syncthreads();
    const int64_t BC4 = (int64_t)B * C4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / C4;
        const int c4 = (int)(i - row * C4);
        const int64_t qb = row * 2 * C4 + c4, qi = qb + C4;
        float4 gb = dy[qb], gi = dy[qi];
        const float4 xv = x[i];
        gb = bn_relu_mask4(gb, lidog_relu_bits_as_float4(bits, qb));
        gi = bn_relu_mask4(gi, lidog_relu_bits_as_float4(bits, qi));
        const float4 mu = s_bn[0][c4], is = s_bn[1][c4], sc = s_bn[2][c4], m0 = s_bn[3][c4], m1 = s_bn[4][c4];
        const int64_t k = (int64_t)bid[row] * C4 + c4;
        const float4 imu = in_mean[k], iis = in_invstd[k], iw = in_w[c4], im0 = coef[k], im1 = coef[BC4 + k];
        const float4 ob = bn_dx_scaled4(gb, xv, mu, is, sc, m0, m1);
        const float4 oi = bn_dx_scaled4(gi, xv, imu, iis, bn_scale4(iis, iw), im0, im1);
        dx[i] = make_float4(ob.x + oi.x, ob.y + oi.y, ob.z + oi.z, ob.w + oi.w);
    }
}

static bool ibn_shape_ok(int64_t n, int C, int B) { return n > 0 && in_vector_path(C, B) && C >= 4; }

extern "C" int lidog_ibn_apply(const float *x, int64_t n, int32_t C, int32_t B, const float *bn_mean,
                               const float *bn_invstd, const float *bn_w, const float *bn_b, const int32_t *bid,
                               const float *in_mean, const float *in_invstd, const float *in_w, const float *in_b,
                               float *y, uint32_t *relu_bits, void *stream) {
    LIDOG_REQUIRE(ibn_shape_ok(n, C, B), "ibn_apply: n > 0, C %% 4 == 0, C <= 1024, 2 B C <= %d", IN_LDS_DOUBLES);
    LIDOG_REQUIRE(relu_bits != nullptr, "ibn_apply: relu_bits [lidog_relu_bits_words(n, 2 C)] required");
    const int64_t total4 = n * (2 * C / 4);
    k_ibn_apply4<<<in_grid(total4), 256, 0, (hipStream_t)stream>>>(
        (const float4 *)x, total4, C / 4, (const float4 *)bn_mean, (const float4 *)bn_invstd, (const float4 *)bn_w,
        (const float4 *)bn_b, bid, (const float4 *)in_mean, (const float4 *)in_invstd, (const float4 *)in_w,
        (const float4 *)in_b, (float4 *)y, relu_bits);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_ibn_bwd_reduce(const float *dy, const uint32_t *relu_bits, const float *x, int64_t n, int32_t C,
                                    int32_t B, const float *bn_mean, const float *bn_invstd, double *bn_sums,
                                    double *bn_ws, float *bn_dw, float *bn_db, const int32_t *perm,
                                    const int32_t *seg_off, const float *in_mean, const float *in_invstd, double *in_ws,
                                    float *in_coef, float *in_dw, float *in_db, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(ibn_shape_ok(n, C, B), "ibn_bwd_reduce: n > 0, C %% 4 == 0, C <= 1024, 2 B C <= %d", IN_LDS_DOUBLES);
    LIDOG_REQUIRE(dy && relu_bits && x && bn_sums && bn_ws && bn_dw && bn_db && in_coef && in_dw && in_db,
                  "ibn_bwd_reduce: missing argument");
    // BatchNorm half: lidog_bn_bwd_reduce's launch (grid, workspace, tail, row count behind the sums)
    const int64_t nb = lidog_bn_bwd_reduce_blocks(n, C);
    BnFinish bfin = {0.f, 0.f, nullptr, nullptr, nullptr, nullptr, bn_dw, bn_db};
    StatsTail tail;
    if (lidog_stats_tail_make(&tail, bn_ws, bn_sums, (double)n, C, bfin, st)) return 1;
    k_ibn_bn_reduce4<<<(unsigned)nb, 256, 0, st>>>((const float4 *)x, (const float4 *)dy, relu_bits, n, C / 4, bn_mean,
                                                    bn_invstd, tail);
    lidog_stats_tail_finish(tail, (int)nb, st);
    LIDOG_LAUNCH_CHECK();
    // instance-norm half: the stand-alone reduction, reading dy's second half through the mask
    InFinish fin{seg_off, B, C, 0.f, nullptr, nullptr, in_coef, in_dw, in_db};
    return in_reduce<1>(x, dy + C, 2 * C / 4, relu_bits, 2 * C / 4, C / 4, n, C, B, perm, in_mean, in_invstd, in_ws,
                        fin, st);
}

extern "C" int lidog_ibn_bwd_apply(const float *dy, const uint32_t *relu_bits, const float *x, int64_t n, int32_t C,
                                   int32_t B, const float *bn_mean, const float *bn_invstd, const float *bn_w,
                                   const double *bn_sums, double bn_count, const int32_t *bid, const float *in_mean,
                                   const float *in_invstd, const float *in_w, const float *in_coef, float *dx,
                                   void *stream) {
    LIDOG_REQUIRE(ibn_shape_ok(n, C, B) && bn_count > 0, "ibn_bwd_apply: n > 0, bn_count > 0, C %% 4 == 0, C <= 1024");
    const int64_t total4 = n * (C / 4);
    k_ibn_bwd_apply4<<<in_grid(total4), 256, 0, (hipStream_t)stream>>>(
        (const float4 *)dy, relu_bits, (const float4 *)x, total4, C / 4, B, bn_mean, bn_invstd, bn_w, bn_sums,
        1.0 / bn_count, bid, (const float4 *)in_mean, (const float4 *)in_invstd, (const float4 *)in_w,
        (const float4 *)in_coef, (float4 *)dx);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
