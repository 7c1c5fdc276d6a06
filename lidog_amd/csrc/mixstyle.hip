// MixStyle (Zhou et al., ICLR 2021) on the rows of a sparse tensor: every scan's per-channel feature mean and standard
// deviation are interpolated with those of a partner scan of the batch.  Not in the reference repository; the
// definition is the one stated in include/lidog_amd.h.
//
//   stats   the instance norm's segmented reduction (inorm.hip: k_in_reduce4 and the two-level last-workgroup tail of
//           stats_tail.h) with MixStyle's finishing step (mixstyle.h): unbiased per-(b, c) moments in double, then,
//           behind a workgroup barrier, the three fp32 tables sub = mu_b, scale = sig_mix / sig_b, add = mu_mix.
//           lam / partner are host arrays: partner is checked before anything is queued, both are copied into the tail
//           of the workspace in stream order.
//   apply   y = fmaf(x - sub[b], scale[b], add[b]), one streaming pass, b from the per-row batch ids
//   bwd     dx = dy * scale[b]: the statistics are constants to autograd
// An identity scan has the table row (0, 1, 0): fmaf(x - 0, 1, 0) == x and dy * 1 == dy bit for bit.
#include "common.h"
#include "mixstyle.h"

extern "C" int64_t lidog_in_reduce_ws(int32_t B, int32_t C);

// doubles: the reduction's workspace, then lam [B] float and partner [B] int32 (B doubles hold both)
extern "C" int64_t lidog_mixstyle_ws(int32_t B, int32_t C) { return lidog_in_reduce_ws(B, C) + (B > 0 ? B : 0); }

extern "C" int lidog_mixstyle_stats(const float *x, int64_t n, int32_t C, int32_t B, const int32_t *perm,
                                    const int32_t *seg_off, const float *lam, const int32_t *partner, float eps,
                                    float *mean, float *sig, float *sub, float *scale, float *add, double *ws,
                                    void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && B >= 0 && B <= 4096 && C >= 0,
                  "mixstyle_stats: 0 <= n < 2^31, 0 <= B <= 4096, C >= 0");
    if (B == 0 || C == 0) return 0;
    LIDOG_REQUIRE(lam && partner && mean && sig && sub && scale && add && ws && seg_off,
                  "mixstyle_stats: lam, partner (host), mean, sig, sub, scale, add [B, C], seg_off and the workspace "
                  "of lidog_mixstyle_ws(B, C) doubles are required");
    for (int b = 0; b < B; ++b)
        LIDOG_REQUIRE(partner[b] >= 0 && partner[b] < B, "mixstyle_stats: partner[%d] = %d is outside [0, %d)", b,
                      partner[b], B);
    double *tail = ws + lidog_in_reduce_ws(B, C);
    float *d_lam = (float *)tail;
    int32_t *d_partner = (int32_t *)(d_lam + B);
    LIDOG_CHECK_HIP(hipMemcpyAsync(d_lam, lam, sizeof(float) * B, hipMemcpyHostToDevice, st));
    LIDOG_CHECK_HIP(hipMemcpyAsync(d_partner, partner, sizeof(int32_t) * B, hipMemcpyHostToDevice, st));
    const MsMix mix{d_lam, d_partner, sig, sub, scale, add};
    return lidog_in_reduce_mixstyle(x, n, C, B, perm, seg_off, eps, mean, mix, ws, st);
}

// ------------------------------------------------------------------ elementwise passes
static unsigned ms_grid(int64_t n) {
    const int64_t g = cdiv64(n, 256);
    return (unsigned)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

__device__ __forceinline__ float ms_y(float x, float sub, float scale, float add) { return fmaf(x - sub, scale, add); }

__global__ __launch_bounds__(256) void k_ms_apply4(const float4 *__restrict__ x, int64_t total4, int C4,
                                                   const int32_t *__restrict__ bid, const float4 *__restrict__ sub,
                                                   const float4 *__restrict__ scale, const float4 *__restrict__ add,
                                                   float4 *__restrict__ y) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / C4;
        const int c4 = (int)(i - row * C4);
        const int64_t k = (int64_t)bid[row] * C4 + c4;
        const float4 v = x[i], s = sub[k], m = scale[k], a = add[k];
        y[i] = make_float4(ms_y(v.x, s.x, m.x, a.x), ms_y(v.y, s.y, m.y, a.y), ms_y(v.z, s.z, m.z, a.z),
                           ms_y(v.w, s.w, m.w, a.w));
    }
}

__global__ __launch_bounds__(256) void k_ms_apply(const float *__restrict__ x, int64_t total, int C,
                                                  const int32_t *__restrict__ bid, const float *__restrict__ sub,
                                                  const float *__restrict__ scale, const float *__restrict__ add,
                                                  float *__restrict__ y) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / C;
        const int64_t k = (int64_t)bid[row] * C + (i - row * C);
        y[i] = ms_y(x[i], sub[k], scale[k], add[k]);
    }
}

__global__ __launch_bounds__(256) void k_ms_bwd4(const float4 *__restrict__ dy, int64_t total4, int C4,
                                                 const int32_t *__restrict__ bid, const float4 *__restrict__ scale,
                                                 float4 *__restrict__ dx) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / C4;
        const int c4 = (int)(i - row * C4);
        const float4 g = dy[i], m = scale[(int64_t)bid[row] * C4 + c4];
        dx[i] = make_float4(g.x * m.x, g.y * m.y, g.z * m.z, g.w * m.w);
    }
}

__global__ __launch_bounds__(256) void k_ms_bwd(const float *__restrict__ dy, int64_t total, int C,
                                                const int32_t *__restrict__ bid, const float *__restrict__ scale,
                                                float *__restrict__ dx) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / C;
        dx[i] = dy[i] * scale[(int64_t)bid[row] * C + (i - row * C)];
    }
}

// bid is the map's own batch column (lidog_in_segments), every entry in [0, B)
extern "C" int lidog_mixstyle_apply(const float *x, int64_t n, int32_t C, int32_t B, const int32_t *bid,
                                    const float *sub, const float *scale, const float *add, float *y, void *stream) {
    LIDOG_REQUIRE(n >= 0 && C >= 0 && B >= 0, "mixstyle_apply: n, C, B >= 0");
    const int64_t total = n * C;
    if (total == 0) return 0;
    LIDOG_REQUIRE(x && bid && sub && scale && add && y, "mixstyle_apply: missing argument");
    if (C % 4 == 0)
        k_ms_apply4<<<ms_grid(total / 4), 256, 0, (hipStream_t)stream>>>(
            (const float4 *)x, total / 4, C / 4, bid, (const float4 *)sub, (const float4 *)scale, (const float4 *)add,
            (float4 *)y);
    else
        k_ms_apply<<<ms_grid(total), 256, 0, (hipStream_t)stream>>>(x, total, C, bid, sub, scale, add, y);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_mixstyle_bwd(const float *dy, int64_t n, int32_t C, int32_t B, const int32_t *bid,
                                  const float *scale, float *dx, void *stream) {
    LIDOG_REQUIRE(n >= 0 && C >= 0 && B >= 0, "mixstyle_bwd: n, C, B >= 0");
    const int64_t total = n * C;
    if (total == 0) return 0;
    LIDOG_REQUIRE(dy && bid && scale && dx, "mixstyle_bwd: missing argument");
    if (C % 4 == 0)
        k_ms_bwd4<<<ms_grid(total / 4), 256, 0, (hipStream_t)stream>>>((const float4 *)dy, total / 4, C / 4, bid,
                                                                        (const float4 *)scale, (float4 *)dx);
    else
        k_ms_bwd<<<ms_grid(total), 256, 0, (hipStream_t)stream>>>(dy, total, C, bid, scale, dx);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
