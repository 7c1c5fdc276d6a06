// Instance-whitening loss of RobustNet (IWLoss, utils/losses/losses.py:464-485), applied by
// PLTRobustNet.training_step (utils/pipelines/trainer_lighting_robustnet.py) to five feature maps of MinkUNet34Robust.
//
// The reference views a map X [n, C] as [n, C, 1], so its "covariance" is one C x C outer product PER ROW:
//   f_cor_i = x_i x_i^T / (n - 1) + eps I,  masked by ones(C, C).triu(1) (which removes eps I),
//   L(X) = sum_i sum_{j<k} |f_cor_i[j, k]| / n = 1 / (n (n - 1)) * sum_i sum_k |x_ik| P_ik,  P_ik = sum_{j<k} |x_ij|
//   dL/dx_im = sign(x_im) (P_im + Q_im) / (n (n - 1)),  Q_im = sum_{j>m} |x_ij|,  sign(0) = 0 (abs backward)
// Every term is >= 0.  Q is an exclusive reverse scan, never S - P - |x|: that difference cancels when one channel
// dominates a row.  Materialised the reference's way the map costs three [n, C, C] intermediates each way; here each
// pass reads every map once (and the backward pass writes the gradient once).
//
// One launch covers up to IW_MAX_MAPS maps of their own (x, n, C) and weight w (passed by value in IwMaps):
//   forward   workgroup b owns the b-th slice of the rows of EVERY map and writes one partial row of IW_COLS doubles
//             (the per-map sums of its slice); the two-level last-workgroup tail of stats_tail.h adds the rows in a fixed
//             order and writes per_map[m] = w_m S_m and total = scale * sum_m per_map[m] (ascending m): no float
//             atomics, the same bits on every run
//   backward  dx_m = sign(x) (P + Q) * (gout[0] * scale * w_m), gout read on the device (no host synchronisation)
// C % 4 == 0 and C <= 128: a row is C / 4 lanes reading float4, rows packed 64 / (C / 4) to a wave (never straddling
// one); the per-lane exclusive prefix / suffix of |x| comes from a segmented shuffle scan across the row's lanes.  Any
// other C: one thread per row, plain loops (no performance target).
#include "common.h"
#include "stats_tail.h"

#define IW_MAX_MAPS 8
#define IW_COLS 8               // columns of a partial row (2 * StatsTail::C): one per map
#define IW_MAX_BLOCKS 1024      // workgroups (= partial rows) of a launch
#define IW_THREADS 256

struct IwMaps {
    const float *x[IW_MAX_MAPS];
    float *g[IW_MAX_MAPS];      // backward: the gradients [n_m, C_m]
    int64_t n[IW_MAX_MAPS];
    int64_t per_wg[IW_MAX_MAPS];   // rows of map m in one workgroup's slice
    double w[IW_MAX_MAPS];
    int C[IW_MAX_MAPS];
    int M;
    double scale;
};

__device__ __forceinline__ bool iw_vector(int C) { return (C & 3) == 0 && C <= 128; }

// Segmented exclusive scans of v over the L lanes of a row (q = lane index within the row; the row's lanes are
// consecutive and never straddle a wave): pre = sum over q' < q, suf = sum over q' > q.
__device__ __forceinline__ void iw_row_scans(float v, int q, int L, float &pre, float &suf) {
    float inc = v, rinc = v;
    for (int d = 1; d < L; d <<= 1) {   // L is uniform across the workgroup: every lane shuffles
        const float up = __shfl_up(inc, d, 64);
        const float dn = __shfl_down(rinc, d, 64);
        if (q >= d) inc += up;
        if (q + d < L) rinc += dn;
    }
    // exclusive forms without subtraction: the neighbour's inclusive value (0 at the row's ends)
    const float lpre = __shfl_up(inc, 1, 64);
    const float lsuf = __shfl_down(rinc, 1, 64);
    pre = q > 0 ? lpre : 0.f;
    suf = q + 1 < L ? lsuf : 0.f;
}

// ------------------------------------------------------------------ forward
__global__ __launch_bounds__(IW_THREADS) void k_iw_fwd(IwMaps maps, StatsTail tail, float *__restrict__ total_out,
                                                          float *__restrict__ per_map) {
    __shared__ double s_red[IW_MAX_MAPS][IW_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *prow = tail.partial + (size_t)blockIdx.x * IW_COLS;
    for (int m = 0; m < maps.M; ++m) {
        const int C = maps.C[m];
        const int64_t n = maps.n[m];
        const int64_t lo = (int64_t)blockIdx.x * maps.per_wg[m];
        const int64_t hi = lo + maps.per_wg[m] < n ? lo + maps.per_wg[m] : n;
        double acc = 0.0;
        if (iw_vector(C)) {
            const int L = C >> 2, RW = 64 / L;       // lanes per row, rows per wave
            const int r = lane / L, q = lane - r * L;
            const bool active = r < RW;
            const float4 *x4 = (const float4 *)maps.x[m];
            const int64_t step = (int64_t)RW * (IW_THREADS / 64);
            // 4 row groups in flight; every lane of a wave takes part in the shuffles (inactive ones carry zeros)
            for (int64_t row0 = lo + (int64_t)wave * RW + r; row0 - r < hi; row0 += 4 * step) {
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t row = row0 + u * step;
                    v[u] = (active && row < hi) ? x4[row * L + q] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float a0 = fabsf(v[u].x), a1 = fabsf(v[u].y), a2 = fabsf(v[u].z), a3 = fabsf(v[u].w);
                    float pre, suf;
                    iw_row_scans(((a0 + a1) + a2) + a3, q, L, pre, suf);
                    (void)suf;
                    const float p1 = pre + a0, p2 = p1 + a1, p3 = p2 + a2;
                    acc += (double)a0 * (double)pre + (double)a1 * (double)p1 + (double)a2 * (double)p2 +
                           (double)a3 * (double)p3;
                }
            }
        } else {
            const float *x = maps.x[m];
            for (int64_t row = lo + tid; row < hi; row += IW_THREADS) {
                const float *xr = x + row * C;
                float p = 0.f;
                for (int k = 0; k < C; ++k) {
                    const float a = fabsf(xr[k]);
                    acc += (double)a * (double)p;
                    p += a;
                }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d, 64);
        if (lane == 0) s_red[m][wave] = acc;
    }
    __syncthreads();
    if (tid < IW_COLS) {
        double s = 0.0;
        if (tid < maps.M) s = ((s_red[tid][0] + s_red[tid][1]) + s_red[tid][2]) + s_red[tid][3];
        lidog_store_sc1(prow + tid, s);
    }
    lidog_stats_tail_rows_with(tail, (int)blockIdx.x, (int)gridDim.x, 1, [&](const double *grows, int ng) {
        if (tid == 0) {
            double total = 0.0;
            for (int m = 0; m < maps.M; ++m) {
                const double lm = lidog_rows_sum_sc1(grows, 0, ng, IW_COLS, m) * maps.w[m];
                per_map[m] = (float)lm;
                total += lm;
            }
            total_out[0] = (float)(total * maps.scale);
        }
    });
}

// ------------------------------------------------------------------ backward
__device__ __forceinline__ float iw_sign_mul(float x, float s, float c) {
    return x > 0.f ? s * c : (x < 0.f ? -(s * c) : 0.f);
}

__global__ __launch_bounds__(IW_THREADS) void k_iw_bwd(IwMaps maps, const float *__restrict__ gout) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double go = (double)gout[0];
    for (int m = 0; m < maps.M; ++m) {
        const int C = maps.C[m];
        const int64_t n = maps.n[m];
        const int64_t lo = (int64_t)blockIdx.x * maps.per_wg[m];
        const int64_t hi = lo + maps.per_wg[m] < n ? lo + maps.per_wg[m] : n;
        const float c = (float)(go * maps.scale * maps.w[m]);
        if (iw_vector(C)) {
            const int L = C >> 2, RW = 64 / L;
            const int r = lane / L, q = lane - r * L;
            const bool active = r < RW;
            const float4 *x4 = (const float4 *)maps.x[m];
            float4 *g4 = (float4 *)maps.g[m];
            const int64_t step = (int64_t)RW * (IW_THREADS / 64);
            for (int64_t row0 = lo + (int64_t)wave * RW + r; row0 - r < hi; row0 += 4 * step) {
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t row = row0 + u * step;
                    v[u] = (active && row < hi) ? x4[row * L + q] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float a0 = fabsf(v[u].x), a1 = fabsf(v[u].y), a2 = fabsf(v[u].z), a3 = fabsf(v[u].w);
                    float pre, suf;
                    iw_row_scans(((a0 + a1) + a2) + a3, q, L, pre, suf);
                    const float p1 = pre + a0, p2 = p1 + a1, p3 = p2 + a2;   // exclusive prefixes of x, y, z, w
                    const float s2 = suf + a3, s1 = s2 + a2, s0 = s1 + a1;   // exclusive suffixes (reverse scan)
                    const int64_t row = row0 + u * step;
                    if (active && row < hi) {
                        float4 o;
                        o.x = iw_sign_mul(v[u].x, pre + s0, c);
                        o.y = iw_sign_mul(v[u].y, p1 + s1, c);
                        o.z = iw_sign_mul(v[u].z, p2 + s2, c);
                        o.w = iw_sign_mul(v[u].w, p3 + suf, c);
                        g4[row * L + q] = o;
                    }
                }
            }
        } else {
            const float *x = maps.x[m];
            float *g = maps.g[m];
            for (int64_t row = lo + tid; row < hi; row += IW_THREADS) {
                const float *xr = x + row * C;
                float *gr = g + row * C;
                float p = 0.f;
                for (int k = 0; k < C; ++k) {   // exclusive prefixes first, parked in the gradient row
                    gr[k] = p;
                    p += fabsf(xr[k]);
                }
                float s = 0.f;
                for (int k = C - 1; k >= 0; --k) {   // then the exclusive suffixes, added
                    const float xv = xr[k];
                    gr[k] = iw_sign_mul(xv, gr[k] + s, c);
                    s += fabsf(xv);
                }
            }
        }
    }
}

// ------------------------------------------------------------------ host
extern "C" int64_t lidog_iw_ws(void) {
    return (int64_t)(IW_MAX_BLOCKS + cdiv64(IW_MAX_BLOCKS, STATS_GROUP)) * IW_COLS;
}

static int iw_pack(IwMaps *p, const float *const *x, float *const *g, const int64_t *n, const int32_t *C,
                   const double *w, int32_t M, double scale, int *nb) {
    LIDOG_REQUIRE(M >= 1 && M <= IW_MAX_MAPS, "iw: 1 <= M <= %d maps per launch", IW_MAX_MAPS);
    LIDOG_REQUIRE(x && n && C && w, "iw: x, n, C and w [M] required");
    *p = IwMaps{};
    p->M = M;
    p->scale = scale;
    // workgroups: enough that the largest map gives each one >= 64 rows, at most IW_MAX_BLOCKS
    int64_t most = 0;
    for (int m = 0; m < M; ++m) {
        LIDOG_REQUIRE(x[m] != nullptr && n[m] >= 2 && n[m] < ((int64_t)1 << 40) && C[m] >= 1,
                      "iw: map %d needs x, n >= 2 (the loss divides by n (n - 1)) and C >= 1", m);
        LIDOG_REQUIRE(!g || g[m] != nullptr, "iw: gradient %d required", m);
        LIDOG_REQUIRE(C[m] % 4 != 0 || C[m] > 128 || ((uintptr_t)x[m] % 16 == 0 && (!g || (uintptr_t)g[m] % 16 == 0)),
                      "iw: map %d (C %% 4 == 0) must be 16-byte aligned", m);
        most = n[m] > most ? n[m] : most;
    }
    int64_t blocks = cdiv64(most, 64);
    blocks = blocks < 1 ? 1 : (blocks > IW_MAX_BLOCKS ? IW_MAX_BLOCKS : blocks);
    for (int m = 0; m < M; ++m) {
        p->x[m] = x[m];
        p->g[m] = g ? g[m] : nullptr;
        p->n[m] = n[m];
        p->per_wg[m] = cdiv64(n[m], blocks);
        p->w[m] = w[m];
        p->C[m] = C[m];
    }
    *nb = (int)blocks;
    return 0;
}

extern "C" int lidog_iw_fwd(const float *const *x, const int64_t *n, const int32_t *C, const double *w, int32_t M,
                            double scale, double *ws, float *total, float *per_map, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    IwMaps maps;
    int nb = 0;
    if (int rc = iw_pack(&maps, x, nullptr, n, C, w, M, scale, &nb)) return rc;
    LIDOG_REQUIRE(ws && total && per_map, "iw_fwd: workspace (lidog_iw_ws() doubles), total [1] and per_map [M] required");
    unsigned *tickets = lidog_stats_tickets(st);
    if (!tickets) return 1;
    StatsTail tail{ws, tickets, nullptr, 0.0, IW_COLS / 2, BnFinish{}};
    k_iw_fwd<<<(unsigned)nb, IW_THREADS, 0, st>>>(maps, tail, total, per_map);
    if (hipPeekAtLastError() != hipSuccess) lidog_stats_tickets_reset(st);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_iw_bwd(const float *const *x, const int64_t *n, const int32_t *C, const double *w, int32_t M,
                            double scale, const float *gout, float *const *gx, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    IwMaps maps;
    int nb = 0;
    LIDOG_REQUIRE(gx && gout, "iw_bwd: gout [1] and the gradients gx [M] required");
    if (int rc = iw_pack(&maps, x, gx, n, C, w, M, scale, &nb)) return rc;
    k_iw_bwd<<<(unsigned)nb, IW_THREADS, 0, st>>>(maps, gout);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
