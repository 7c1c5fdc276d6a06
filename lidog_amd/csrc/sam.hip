// The global gradient norm over the optimiser's flat gradient buffer and its two users (lidog_amd/optim.py): gradient
// clipping (torch's clip_grad_norm_) and the ascent step of sharpness-aware minimisation (SAM / ASAM).  The arithmetic
// is stated in include/lidog_amd.h and restated in numpy by tests/sam_ref.py; the build sets -ffp-contract=off, so every
// fp32 operation is rounded on its own.
//
// All three are streaming passes in the style of k_wavg (wavg.hip): at most LIDOG_FLAT_MAX_BLOCKS workgroups of 256
// threads, one float4 per thread and sweep, a grid-stride loop beyond; a scalar head up to the first 16-byte boundary,
// a float4 body, a scalar tail; buffers aligned differently mod 16 take the scalar loop throughout.
//
// The norm is summed in fp64 without atomics and in an order that no timing can change: lanes -> thread -> wave
// (shuffles) -> workgroup (LDS) -> one partial sum per workgroup in the workspace; a second launch of ONE workgroup adds
// the partial sums the same way.  Its users read the double where it lies: nothing crosses to the host.
#include "common.h"

namespace {
constexpr int FLAT_BLOCK = 256;
constexpr int64_t FLAT_SWEEP = 4 * FLAT_BLOCK;      // elements one workgroup covers per sweep

inline int64_t flat_blocks(int64_t n) {
    const int64_t nb = cdiv64(n, FLAT_SWEEP);
    return nb > LIDOG_FLAT_MAX_BLOCKS ? LIDOG_FLAT_MAX_BLOCKS : nb;
}

// how a workgroup walks n elements from `base`: [0, head) scalar, `body` float4s from base + head, then a scalar tail
struct FlatWalk {
    int64_t head, body, tail0;
};
__device__ __forceinline__ FlatWalk flat_walk(const void *base, int64_t n) {
    FlatWalk k;
    k.head = (int64_t)(((16 - ((uintptr_t)base & 15)) & 15) >> 2);
    if (k.head > n) k.head = n;
    k.body = (n - k.head) >> 2;
    k.tail0 = k.head + 4 * k.body;
    return k;
}

// the sum of `v` over the 256 threads of the workgroup in a fixed tree; valid in thread 0
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double waves[FLAT_BLOCK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = v;
    __syncthreads();
    return (waves[0] + waves[1]) + (waves[2] + waves[3]);
}

template <int MODE>
__device__ __forceinline__ double sq_term(float g, float w) {
    const float t = MODE == LIDOG_SQNORM_ADAPTIVE ? fabsf(w) * g : g;
    return (double)t * (double)t;
}
}  // namespace

template <int MODE>
__global__ __launch_bounds__(256) void k_sqnorm_partial(const float *__restrict__ g, const float *__restrict__ w,
                                                        int64_t n, double *__restrict__ partial) {
    const int64_t t = (int64_t)blockIdx.x * FLAT_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * FLAT_BLOCK;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (MODE == LIDOG_SQNORM_ADAPTIVE && (((uintptr_t)g ^ (uintptr_t)w) & 15) != 0) {
        for (int64_t i = t; i < n; i += stride) a0 = a0 + sq_term<MODE>(g[i], w[i]);
    } else {
        const FlatWalk k = flat_walk(g, n);
        if (t < k.head) a0 = a0 + sq_term<MODE>(g[t], MODE ? w[t] : 0.f);
        const float4 *__restrict__ g4 = (const float4 *)(g + k.head);
        const float4 *__restrict__ w4 = MODE ? (const float4 *)(w + k.head) : g4;    // plain mode: w is NULL, not read
        for (int64_t i = t; i < k.body; i += stride) {
            const float4 x = g4[i];
            float4 y = x;
            if (MODE == LIDOG_SQNORM_ADAPTIVE) y = w4[i];
            a0 = a0 + sq_term<MODE>(x.x, y.x);
            a1 = a1 + sq_term<MODE>(x.y, y.y);
            a2 = a2 + sq_term<MODE>(x.z, y.z);
            a3 = a3 + sq_term<MODE>(x.w, y.w);
        }
        if (t < n - k.tail0) a0 = a0 + sq_term<MODE>(g[k.tail0 + t], MODE ? w[k.tail0 + t] : 0.f);
    }
    const double s = block_sum((a0 + a1) + (a2 + a3));
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one workgroup: thread t adds partial[t], partial[t + 256], ... in that order
__global__ __launch_bounds__(256) void k_sqnorm_finish(const double *__restrict__ partial, int nb,
                                                       double *__restrict__ out) {
    double a = 0.0;
    for (int i = threadIdx.x; i < nb; i += FLAT_BLOCK) a = a + partial[i];
    const double s = block_sum(a);
    if (threadIdx.x == 0) out[0] = s;
}

extern "C" int64_t lidog_flat_sqnorm_ws(int64_t n) {
    const int64_t nb = n > 0 ? flat_blocks(n) : 0;
    return 8 * (nb > 0 ? nb : 1);
}

extern "C" int lidog_flat_sqnorm(const float *g, const float *w, int64_t n, int32_t mode, void *ws, double *out,
                                 void *stream) {
    LIDOG_REQUIRE(n >= 0, "flat_sqnorm: %lld elements", (long long)n);
    LIDOG_REQUIRE(mode == LIDOG_SQNORM_PLAIN || mode == LIDOG_SQNORM_ADAPTIVE, "flat_sqnorm: unknown mode %d", mode);
    LIDOG_REQUIRE(out != nullptr && ((uintptr_t)out & 7) == 0, "flat_sqnorm: out must be an 8-byte aligned device word");
    hipStream_t st = (hipStream_t)stream;
    int nb = 0;
    if (n > 0) {
        LIDOG_REQUIRE(g != nullptr && ((uintptr_t)g & 3) == 0, "flat_sqnorm: g is not a float32 array");
        LIDOG_REQUIRE(mode == LIDOG_SQNORM_PLAIN || (w != nullptr && ((uintptr_t)w & 3) == 0),
                      "flat_sqnorm: the adaptive norm needs w");
        LIDOG_REQUIRE(ws != nullptr && ((uintptr_t)ws & 7) == 0, "flat_sqnorm: ws must be 8-byte aligned");
        nb = (int)flat_blocks(n);
        if (mode == LIDOG_SQNORM_ADAPTIVE)
            k_sqnorm_partial<LIDOG_SQNORM_ADAPTIVE><<<nb, FLAT_BLOCK, 0, st>>>(g, w, n, (double *)ws);
        else
            k_sqnorm_partial<LIDOG_SQNORM_PLAIN><<<nb, FLAT_BLOCK, 0, st>>>(g, nullptr, n, (double *)ws);
        LIDOG_LAUNCH_CHECK();
    }
    k_sqnorm_finish<<<1, FLAT_BLOCK, 0, st>>>((const double *)ws, nb, out);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ SAM's ascent step
namespace {
template <int ADAPTIVE>
__device__ __forceinline__ float sam_new_w(float w, float g, float coef) {
    if (g == 0.f) return w;      // no gradient: not even w + 0 (a -0.0 would lose its sign)
    const float e = ADAPTIVE ? ((w * w) * g) * coef : coef * g;
    return w + e;
}
}  // namespace

template <int ADAPTIVE>
__global__ __launch_bounds__(256) void k_sam_perturb(float *__restrict__ w, const float *__restrict__ g,
                                                     float *__restrict__ backup, int64_t n,
                                                     const double *__restrict__ sqnorm, float rho) {
    const float coef = (float)((double)rho / (sqrt(sqnorm[0]) + 1e-12));
    const int64_t t = (int64_t)blockIdx.x * FLAT_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * FLAT_BLOCK;
    if (((((uintptr_t)w ^ (uintptr_t)g) | ((uintptr_t)w ^ (uintptr_t)backup)) & 15) != 0) {
        for (int64_t i = t; i < n; i += stride) {
            const float x = w[i];
            backup[i] = x;
            w[i] = sam_new_w<ADAPTIVE>(x, g[i], coef);
        }
        return;
    }
    const FlatWalk k = flat_walk(w, n);
    if (t < k.head) {
        const float x = w[t];
        backup[t] = x;
        w[t] = sam_new_w<ADAPTIVE>(x, g[t], coef);
    }
    float4 *__restrict__ w4 = (float4 *)(w + k.head);
    float4 *__restrict__ b4 = (float4 *)(backup + k.head);
    const float4 *__restrict__ g4 = (const float4 *)(g + k.head);
    for (int64_t i = t; i < k.body; i += stride) {
        float4 x = w4[i];
        const float4 y = g4[i];
        b4[i] = x;
        x.x = sam_new_w<ADAPTIVE>(x.x, y.x, coef);
        x.y = sam_new_w<ADAPTIVE>(x.y, y.y, coef);
        x.z = sam_new_w<ADAPTIVE>(x.z, y.z, coef);
        x.w = sam_new_w<ADAPTIVE>(x.w, y.w, coef);
        w4[i] = x;
    }
    if (t < n - k.tail0) {
        const int64_t i = k.tail0 + t;
        const float x = w[i];
        backup[i] = x;
        w[i] = sam_new_w<ADAPTIVE>(x, g[i], coef);
    }
}

extern "C" int lidog_sam_perturb(float *w, const float *g, float *backup, int64_t n, const double *sqnorm, float rho,
                                 int32_t adaptive, void *stream) {
    LIDOG_REQUIRE(n >= 0, "sam_perturb: %lld elements", (long long)n);
    LIDOG_REQUIRE(rho > 0.f && rho <= 3.0e38f, "sam_perturb: rho = %g must be positive and finite", (double)rho);
    if (n == 0) return 0;
    LIDOG_REQUIRE(w != nullptr && g != nullptr && backup != nullptr && (((uintptr_t)w | (uintptr_t)g | (uintptr_t)backup) & 3) == 0,
                  "sam_perturb: w, g and backup are float32 arrays");
    LIDOG_REQUIRE(sqnorm != nullptr && ((uintptr_t)sqnorm & 7) == 0, "sam_perturb: sqnorm is an 8-byte aligned device word");
    const uintptr_t a[3] = {(uintptr_t)w, (uintptr_t)g, (uintptr_t)backup};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            LIDOG_REQUIRE(a[i] + 4 * (uintptr_t)n <= a[j] || a[j] + 4 * (uintptr_t)n <= a[i],
                          "sam_perturb: w, g and backup overlap");
    const unsigned nb = (unsigned)flat_blocks(n);
    hipStream_t st = (hipStream_t)stream;
    if (adaptive)
        k_sam_perturb<1><<<nb, FLAT_BLOCK, 0, st>>>(w, g, backup, n, sqnorm, rho);
    else
        k_sam_perturb<0><<<nb, FLAT_BLOCK, 0, st>>>(w, g, backup, n, sqnorm, rho);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ clip_grad_norm_
__global__ __launch_bounds__(256) void k_flat_clip(float *__restrict__ g, int64_t n, const double *__restrict__ sqnorm,
                                                   float max_norm, float grad_scale) {
    const double norm = (double)grad_scale * sqrt(sqnorm[0]);
    const float coef = fminf(1.0f, (float)((double)max_norm / (norm + 1e-6)));
    const int64_t t = (int64_t)blockIdx.x * FLAT_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * FLAT_BLOCK;
    const FlatWalk k = flat_walk(g, n);
    if (t < k.head) g[t] = g[t] * coef;
    float4 *__restrict__ g4 = (float4 *)(g + k.head);
    for (int64_t i = t; i < k.body; i += stride) {
        float4 x = g4[i];
        x.x = x.x * coef;
        x.y = x.y * coef;
        x.z = x.z * coef;
        x.w = x.w * coef;
        g4[i] = x;
    }
    if (t < n - k.tail0) g[k.tail0 + t] = g[k.tail0 + t] * coef;
}

extern "C" int lidog_flat_clip(float *g, int64_t n, const double *sqnorm, float max_norm, float grad_scale,
                               void *stream) {
    LIDOG_REQUIRE(n >= 0, "flat_clip: %lld elements", (long long)n);
    LIDOG_REQUIRE(max_norm > 0.f, "flat_clip: max_norm = %g must be positive", (double)max_norm);
    LIDOG_REQUIRE(grad_scale > 0.f, "flat_clip: grad_scale = %g must be positive", (double)grad_scale);
    if (n == 0) return 0;
    LIDOG_REQUIRE(g != nullptr && ((uintptr_t)g & 3) == 0, "flat_clip: g is not a float32 array");
    LIDOG_REQUIRE(sqnorm != nullptr && ((uintptr_t)sqnorm & 7) == 0, "flat_clip: sqnorm is an 8-byte aligned device word");
    k_flat_clip<<<(unsigned)flat_blocks(n), FLAT_BLOCK, 0, (hipStream_t)stream>>>(g, n, sqnorm, max_norm, grad_scale);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
