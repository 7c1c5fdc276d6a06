// Fused optimiser steps on slices of the flat parameter / gradient buffers (lidog_amd/optim.py).
// SGD: torch.optim.SGD(lr, momentum, weight_decay, nesterov=True, dampening=0) as configured at
// utils/pipelines/trainer_lighting_2d.py:351-355 (momentum 0.98, :26).  Adam: torch.optim.Adam (k_adam).
#include "common.h"

// g' = g * grad_scale + wd * p;  buf = mu * buf + g'  (buf starts at 0: the first step gives buf = g' like
// torch's clone);  p -= lr * (g' + mu * buf)  [nesterov]  or  p -= lr * buf
__global__ __launch_bounds__(256) void k_sgd(float *__restrict__ p, const float *__restrict__ g,
                                             float *__restrict__ buf, int64_t n, float lr, float mu, float wd,
                                             int nesterov, float grad_scale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float pi = p[i];
        const float gi = g[i] * grad_scale + wd * pi;
        const float bi = buf[i] * mu + gi;
        const float step = nesterov ? gi + mu * bi : bi;
        p[i] = pi - lr * step;
        buf[i] = bi;
    }
}

extern "C" int lidog_sgd_step(float *param, const float *grad, float *momentum_buf, int64_t n, float lr,
                              float momentum, float weight_decay, int32_t nesterov, float grad_scale,
                              void *stream) {
    if (n == 0) return 0;
    LIDOG_REQUIRE(momentum >= 0.f && lr >= 0.f, "sgd_step: lr and momentum must be non-negative");
    int64_t g = cdiv64(n, 256);
    if (g > 8192) g = 8192;
    k_sgd<<<(unsigned)g, 256, 0, (hipStream_t)stream>>>(param, grad, momentum_buf, n, lr, momentum, weight_decay,
                                                        nesterov, grad_scale);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// Adam on a flat buffer: torch.optim.Adam semantics (L2 weight decay folded into the gradient; bias-corrected step)
__global__ __launch_bounds__(256) void k_adam(float *__restrict__ p, const float *__restrict__ g,
                                              float *__restrict__ m, float *__restrict__ v, int64_t n, float lr_bc1,
                                              float beta1, float beta2, float eps, float wd, float bc2_sqrt,
                                              float grad_scale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float pi = p[i];
        float gi = g[i] * grad_scale + wd * pi;
        float mi = m[i];
        mi = mi + (gi - mi) * (1.f - beta1);
        float vi = v[i] * beta2 + (1.f - beta2) * gi * gi;
        float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = pi - lr_bc1 * (mi / denom);
        m[i] = mi;
        v[i] = vi;
    }
}

extern "C" int lidog_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                               float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                               float grad_scale, void *stream) {
    if (n == 0) return 0;
    double bc1 = 1.0 - pow((double)beta1, (double)step);
    double bc2 = 1.0 - pow((double)beta2, (double)step);
    int64_t g = cdiv64(n, 256);
    if (g > 8192) g = 8192;
    k_adam<<<(unsigned)g, 256, 0, (hipStream_t)stream>>>(param, grad, exp_avg, exp_avg_sq, n, (float)((double)lr / bc1),
                                                         beta1, beta2, eps, weight_decay, (float)sqrt(bc2), grad_scale);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// Gradient accumulation of the trunk executor's second pass over one model in one step (lidog_amd/trunk.py, csrc/
// trunk.hip accumulate mode): dst[i] = dst[i] + src[i] over up to ACC_SEGS (dst, src, n) segments per launch.  Plain fp32
// adds, so the result has the bits of autograd's `grad += new` whichever of the two passes wrote dst.  A segment is
// walked as a scalar head up to dst's first 16-byte boundary, float4 body, scalar tail (a bias of 7); a src whose
// alignment differs from dst's takes the scalar loop throughout.
namespace {
constexpr int ACC_SEGS = 8;
struct AccSegs {
    float *dst[ACC_SEGS];
    const float *src[ACC_SEGS];
    int64_t n[ACC_SEGS];
    int64_t block0[ACC_SEGS + 1];   // first workgroup of every segment; block0[nseg] = grid size
    int32_t nseg;
};
}  // namespace

__global__ __launch_bounds__(256) void k_grad_accumulate(AccSegs a) {
    int s = 0;
    while (s + 1 < a.nseg && (int64_t)blockIdx.x >= a.block0[s + 1]) ++s;
    float *__restrict__ dst = a.dst[s];
    const float *__restrict__ src = a.src[s];
    const int64_t n = a.n[s];
    const int64_t t = ((int64_t)blockIdx.x - a.block0[s]) * 256 + threadIdx.x;
    const int64_t stride = (a.block0[s + 1] - a.block0[s]) * 256;
    if ((((uintptr_t)dst ^ (uintptr_t)src) & 15) != 0) {
        for (int64_t i = t; i < n; i += stride) dst[i] = dst[i] + src[i];
        return;
    }
    int64_t head = (int64_t)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2);
    if (head > n) head = n;
    const int64_t body = (n - head) >> 2, tail0 = head + 4 * body;
    if (t < head) dst[t] = dst[t] + src[t];
    float4 *__restrict__ d4 = (float4 *)(dst + head);
    const float4 *__restrict__ s4 = (const float4 *)(src + head);
    for (int64_t i = t; i < body; i += stride) {
        float4 x = d4[i];
        const float4 y = s4[i];
        x.x = x.x + y.x;
        x.y = x.y + y.y;
        x.z = x.z + y.z;
        x.w = x.w + y.w;
        d4[i] = x;
    }
    if (t < n - tail0) dst[tail0 + t] = dst[tail0 + t] + src[tail0 + t];
}

extern "C" int lidog_grad_accumulate(const int64_t *segs, int32_t n_segs, void *stream) {
    LIDOG_REQUIRE(n_segs >= 0 && (segs || n_segs == 0), "grad_accumulate: bad segment table");
    for (int32_t s0 = 0; s0 < n_segs; s0 += ACC_SEGS) {
        AccSegs a;
        a.nseg = 0;
        int64_t blocks = 0;
        for (int32_t s = s0; s < n_segs && s < s0 + ACC_SEGS; ++s) {
            const int64_t *g = segs + 3 * (int64_t)s;
            LIDOG_REQUIRE(g[2] >= 0 && ((g[0] && g[1]) || g[2] == 0), "grad_accumulate: segment %d is malformed", s);
            if (g[2] == 0) continue;
            int64_t nb = cdiv64(g[2], 1024);     // one float4 per thread
            if (nb > 4096) nb = 4096;
            a.dst[a.nseg] = (float *)(uintptr_t)g[0];
            a.src[a.nseg] = (const float *)(uintptr_t)g[1];
            a.n[a.nseg] = g[2];
            a.block0[a.nseg] = blocks;
            blocks += nb;
            ++a.nseg;
        }
        if (a.nseg == 0) continue;
        a.block0[a.nseg] = blocks;
        k_grad_accumulate<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(a);
        LIDOG_LAUNCH_CHECK();
    }
    return 0;
}
