// The entropy criterion of test-time adaptation (lidog_amd.adapt; TENT, Wang et al., ICLR 2021): the mean Shannon entropy
// of the row softmax over the rows that take part, and its gradient.  Not in the reference; include/lidog_amd.h states
// the arithmetic.  The shape of k_ce_sums / k_ce_finish / k_ce_bwd (losses.hip): one thread per row, the row in
// registers (one instantiation per class count), 256-thread workgroups, per-workgroup double partials added in a fixed
// order, no floating-point atomics, nothing read back.
// Per row the arithmetic runs in double on the shifted logits z_c = x_c - m (exact: the difference of two floats):
//   s = sum exp(z_c),  lse - x_c = log s - z_c,  H = lse - sum p_c x_c = log s - (sum exp(z_c) z_c) / s
// so a row is rounded to float once, at the store: H = lse - sum p x on the unshifted logits in float would lose
// |m| 2^-24 to cancellation.  20 double exp per row is nothing next to the row's own load: the pass stays memory-bound.
#include "criteria.h"

#define EN_MAX_BLOCKS 1024

// (log s, H) of a row; e[c] = exp(z_c), z[c] = z_c.  A logit far below the maximum gives e = 0 and e z = 0: no NaN.
template <int C>
__device__ __forceinline__ void entropy_row(const float *__restrict__ x, double (&e)[C], double (&z)[C], double &logs,
                                            double &s, double &H) {
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = x[c];
    float m = v[0];
#pragma unroll
    for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
    s = 0.0;
    double ez = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        z[c] = (double)v[c] - (double)m;
        e[c] = exp(z[c]);
        s += e[c];
        ez += e[c] * z[c];
    }
    logs = log(s);
    H = logs - ez / s;
}

__device__ __forceinline__ bool entropy_takes_part(const uint8_t *__restrict__ mask, int64_t r, float h, float margin) {
    return (mask == nullptr || mask[r] != 0) && (margin <= 0.f || h < margin);
}

// row_h[r] for every row; partial[block][2] = (sum of H over the rows that take part, their number)
template <int C>
__global__ __launch_bounds__(256) void k_entropy_sums(const float *__restrict__ logits, const uint8_t *__restrict__ mask,
                                                      int64_t n, float margin, float *__restrict__ row_h,
                                                      double *__restrict__ partial) {
    __shared__ double red[4][2];
    double acc_h = 0.0, acc_k = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        double e[C], z[C], logs, s, H;
        entropy_row<C>(logits + r * C, e, z, logs, s, H);
        const float h = (float)H;
        row_h[r] = h;
        if (entropy_takes_part(mask, r, h, margin)) {
            acc_h += H;
            acc_k += 1.0;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        acc_h += __shfl_down(acc_h, d);
        acc_k += __shfl_down(acc_k, d);
    }
    if (lane == 0) {
        red[wave][0] = acc_h;
        red[wave][1] = acc_k;
    }
    __syncthreads();
    if (threadIdx.x < 2)
        partial[(size_t)blockIdx.x * 2 + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// one block: (S, k) over the partials in a fixed tree; loss = S / k, coef = (1 / k, k); all 0 when no row takes part
__global__ __launch_bounds__(256) void k_entropy_finish(const double *__restrict__ partial, int nb,
                                                        float *__restrict__ loss, float *__restrict__ coef) {
    __shared__ double part[256][2];
    double s = 0, k = 0;
    for (int b = threadIdx.x; b < nb; b += 256) {
        s += partial[(size_t)b * 2];
        k += partial[(size_t)b * 2 + 1];
    }
    part[threadIdx.x][0] = s;
    part[threadIdx.x][1] = k;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {      // a fixed tree: bit-reproducible
        if ((int)threadIdx.x < d) {
            part[threadIdx.x][0] += part[threadIdx.x + d][0];
            part[threadIdx.x][1] += part[threadIdx.x + d][1];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double S = part[0][0], K = part[0][1];      // K: a sum of ones, exact up to 2^53 rows
        loss[0] = K > 0 ? (float)(S / K) : 0.f;
        coef[0] = K > 0 ? (float)(1.0 / K) : 0.f;
        coef[1] = (float)K;
    }
}

template <int C>
__global__ __launch_bounds__(256) void k_entropy_bwd(const float *__restrict__ logits, const uint8_t *__restrict__ mask,
                                                     const float *__restrict__ row_h, int64_t n, float margin,
                                                     const float *__restrict__ coef, const float *__restrict__ gout,
                                                     float *__restrict__ glogits) {
    const double gk = (double)gout[0] * (double)coef[0];
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        float *g = glogits + r * C;
        if (!entropy_takes_part(mask, r, row_h[r], margin)) {
#pragma unroll
            for (int c = 0; c < C; ++c) g[c] = 0.f;
            continue;
        }
        double e[C], z[C], logs, s, H;
        entropy_row<C>(logits + r * C, e, z, logs, s, H);
        const double gs = gk / s;
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = (float)(gs * e[c] * ((logs - z[c]) - H));
    }
}

extern "C" int64_t lidog_entropy_ws(int32_t C) { return (int64_t)EN_MAX_BLOCKS * 2; }

extern "C" int lidog_entropy_fwd(const float *logits, const uint8_t *mask, int64_t n, int32_t C, float margin, double *ws,
                                 float *loss, float *coef, float *row_h, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0 && C >= 2 && C <= DL_MAXC, "entropy: bad shape");
    int64_t nb = cdiv64(n, 256 * 4);
    nb = nb < 1 ? 1 : (nb > EN_MAX_BLOCKS ? EN_MAX_BLOCKS : nb);
#define CALL(C_) k_entropy_sums<C_><<<(unsigned)nb, 256, 0, st>>>(logits, mask, n, margin, row_h, ws)
    DICE_DISPATCH(CALL)
#undef CALL
    k_entropy_finish<<<1, 256, 0, st>>>(ws, (int)nb, loss, coef);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_entropy_bwd(const float *logits, const uint8_t *mask, const float *row_h, int64_t n, int32_t C,
                                 float margin, const float *coef, const float *gout, float *glogits, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0 && C >= 2 && C <= DL_MAXC, "entropy: bad shape");
    if (n == 0) return 0;
    int64_t nb = cdiv64(n, 256);
    if (nb > 4096) nb = 4096;
#define CALL(C_) \
    k_entropy_bwd<C_><<<(unsigned)nb, 256, 0, st>>>(logits, mask, row_h, n, margin, coef, gout, glogits)
    DICE_DISPATCH(CALL)
#undef CALL
    LIDOG_LAUNCH_CHECK();
    return 0;
}
