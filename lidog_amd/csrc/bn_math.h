// The BatchNorm arithmetic, stated once (device functions only: no state, no launchers).
//
// The library promises that a fused path produces the bits of the separate kernels: the _in_bn staging forms, the
// _bwdstats reduction, the evaluation-mode epilogues, the IBN pass and the SyncBatchNorm apply against their two-pass
// forms.  Every such promise holds because both sides evaluate the float expressions below in the same operation
// order (-ffp-contract=off in build.py keeps the compiler from fusing them).  A kernel that normalises, reduces or
// differentiates a BatchNorm / InstanceNorm calls these functions instead of writing the expression out.
#pragma once
#include "common.h"

__device__ __forceinline__ float4 bn_f4(const float (&a)[4]) { return make_float4(a[0], a[1], a[2], a[3]); }

// ---- forward: y = (x - mean) * invstd * w + b, left to right
__device__ __forceinline__ float bn_xhat(float x, float mean, float invstd) { return (x - mean) * invstd; }
__device__ __forceinline__ float bn_affine(float x, float mean, float invstd, float w, float b) {
    return bn_xhat(x, mean, invstd) * w + b;
}
__device__ __forceinline__ float4 bn_affine4(float4 v, float4 m, float4 s, float4 w, float4 b) {
    v.x = bn_affine(v.x, m.x, s.x, w.x, b.x);
    v.y = bn_affine(v.y, m.y, s.y, w.y, b.y);
    v.z = bn_affine(v.z, m.z, s.z, w.z, b.z);
    v.w = bn_affine(v.w, m.w, s.w, w.w, b.w);
    return v;
}

// + residual, then ReLU.  SELECT: the ReLU as `v > 0 ? v : 0` (bn.hip: k_bn_apply, k_bn_apply_plane) instead of one
// fmaxf (every float4 kernel and the convolution epilogues); each kernel keeps the form it was written with.
// r: the residual, loaded by the caller ahead of its use (unconditional batched loads)
template <bool SELECT = false>
__device__ __forceinline__ float bn_res_relu(float v, bool has_res, float r, int relu) {
    if (has_res) v += r;
    if (relu) v = SELECT ? (v > 0.f ? v : 0.f) : fmaxf(v, 0.f);
    return v;
}
// res: the residual tensor or NULL; its element / float4 number i is loaded only when there is one
template <bool SELECT = false>
__device__ __forceinline__ float bn_res_relu(float v, const float *res, int64_t i, int relu) {
    if (res) v += res[i];
    if (relu) v = SELECT ? (v > 0.f ? v : 0.f) : fmaxf(v, 0.f);
    return v;
}
__device__ __forceinline__ float4 bn_res_relu4(float4 v, const float4 *res, int64_t i, int relu) {
    if (res) { float4 r = res[i]; v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w; }
    if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    return v;
}

// ---- ReLU bit mask of a [rows, C] matrix (C % 4 == 0): bit 4 * (q % 8) + j of word q / 8 is (element j of float4
// number q) > 0.  Written by lidog_bn_apply_bits / lidog_bn_apply_sync / lidog_ibn_apply.
// Store: called by all 256 threads of a workgroup for float4 numbers base + threadIdx.x (base a multiple of 8); a lane
// with !ok passes zeros.  The word is assembled from 8 neighbouring lanes with shuffles.
__device__ __forceinline__ void lidog_relu_bits_store(uint32_t *bits, int64_t q, bool ok, float4 v) {
    uint32_t nib = (v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u) | (v.z > 0.f ? 4u : 0u) | (v.w > 0.f ? 8u : 0u);
    uint32_t wv = nib << (4 * (threadIdx.x & 7));
    wv |= __shfl_xor(wv, 1);
    wv |= __shfl_xor(wv, 2);
    wv |= __shfl_xor(wv, 4);
    if (ok && (threadIdx.x & 7) == 0) bits[q >> 3] = wv;
}
// Read back as a float4 of 1 / 0 so that the consumers keep their `y > 0` tests.
__device__ __forceinline__ float4 lidog_relu_bits_as_float4(const uint32_t *__restrict__ bits, int64_t q) {
    const uint32_t nib = bits[q >> 3] >> (4 * (int)(q & 7));
    return make_float4((float)(nib & 1u), (float)((nib >> 1) & 1u), (float)((nib >> 2) & 1u), (float)((nib >> 3) & 1u));
}
// dy where the forward output (or its mask bit) is > 0, else 0
__device__ __forceinline__ float4 bn_relu_mask4(float4 g, float4 y) {
    g.x = y.x > 0.f ? g.x : 0.f; g.y = y.y > 0.f ? g.y : 0.f;
    g.z = y.z > 0.f ? g.z : 0.f; g.w = y.w > 0.f ? g.w : 0.f;
    return g;
}

// ---- reductions, accumulated in double
// MODE 0: (x, x*x)            -> statistics
// MODE 1: (dy', dy' * xhat)   -> backward reductions, dy' = dy * (ry > 0) when has_relu
template <int MODE>
__device__ __forceinline__ void bn_red_terms(float x, float dy, float ry, bool has_relu, float mean, float invstd,
                                             double &t0, double &t1) {
    if (MODE == 0) {
        t0 += (double)x;
        t1 += (double)x * (double)x;
    } else {
        float g = (has_relu && !(ry > 0.f)) ? 0.f : dy;
        float xh = bn_xhat(x, mean, invstd);
        t0 += (double)g;
        t1 += (double)g * (double)xh;
    }
}
// a channel quad: a[0..3] first sums, a[4..7] second sums (the layout lidog_stats_tail takes)
template <int MODE>
__device__ __forceinline__ void bn_red_terms4(float4 x, float4 dy, float4 ry, bool has_relu,
                                              float4 mean, float4 invstd, double (&a)[8]) {
    bn_red_terms<MODE>(x.x, dy.x, ry.x, has_relu, mean.x, invstd.x, a[0], a[4]);
    bn_red_terms<MODE>(x.y, dy.y, ry.y, has_relu, mean.y, invstd.y, a[1], a[5]);
    bn_red_terms<MODE>(x.z, dy.z, ry.z, has_relu, mean.z, invstd.z, a[2], a[6]);
    bn_red_terms<MODE>(x.w, dy.w, ry.w, has_relu, mean.w, invstd.w, a[3], a[7]);
}

// ---- input gradient dx = (g - m0 - xhat * m1) * invstd * w, m0 / m1 the means of the two backward sums.
// Two forms that ROUND DIFFERENTLY -- do not merge them, each kernel's dx bits depend on its form:
//   bn_dx         * invstd, then * w            bn.hip: k_bn_bwd_apply, k_bn_bwd_apply_plane (scalar / NCHW layouts)
//   bn_dx_scaled  * sc, sc = bn_scale(invstd, w) rounded once beforehand
//                                               bn.hip: k_bn_bwd_apply4; inorm.hip: k_in_bwd_apply{,4}, k_ibn_bwd_apply4
__device__ __forceinline__ float bn_dx(float g, float x, float mean, float invstd, float w, float m0, float m1) {
    return (g - m0 - bn_xhat(x, mean, invstd) * m1) * invstd * w;
}
__device__ __forceinline__ float bn_scale(float invstd, float w) { return invstd * w; }
__device__ __forceinline__ float4 bn_scale4(float4 s, float4 w) {
    return make_float4(bn_scale(s.x, w.x), bn_scale(s.y, w.y), bn_scale(s.z, w.z), bn_scale(s.w, w.w));
}
__device__ __forceinline__ float bn_dx_scaled(float g, float x, float mean, float invstd, float sc, float m0, float m1) {
    return (g - m0 - bn_xhat(x, mean, invstd) * m1) * sc;
}
__device__ __forceinline__ float4 bn_dx_scaled4(float4 g, float4 x, float4 mean, float4 invstd,
                                                float4 sc, float4 m0, float4 m1) {
    return make_float4(bn_dx_scaled(g.x, x.x, mean.x, invstd.x, sc.x, m0.x, m1.x),
                       bn_dx_scaled(g.y, x.y, mean.y, invstd.y, sc.y, m0.y, m1.y),
                       bn_dx_scaled(g.z, x.z, mean.z, invstd.z, sc.z, m0.z, m1.z),
                       bn_dx_scaled(g.w, x.w, mean.w, invstd.w, sc.w, m0.w, m1.w));
}

// ---- finalise: (sum x, sum x^2, count) -> mean, invstd (biased variance) and the running statistics (unbiased)
struct BnMoments {
    double mean, var;   // var: biased, clamped at 0
};
__device__ __forceinline__ BnMoments bn_moments(double sx, double sxx, double count) {
    BnMoments o;
    o.mean = sx / count;
    o.var = sxx / count - o.mean * o.mean;
    if (o.var < 0) o.var = 0;
    return o;
}
__device__ __forceinline__ float bn_invstd(double var, float eps) { return (float)(1.0 / sqrt(var + (double)eps)); }
__device__ __forceinline__ void bn_running_update(const BnMoments &o, double count, int c, const BnFinish &fin) {
    if (fin.running_mean) {
        double unb = (count > 1) ? o.var * count / (count - 1) : o.var;
        fin.running_mean[c] = (1.f - fin.momentum) * fin.running_mean[c] + fin.momentum * (float)o.mean;
        fin.running_var[c] = (1.f - fin.momentum) * fin.running_var[c] + fin.momentum * (float)unb;
    }
}
__device__ __forceinline__ void lidog_bn_finalize_channel(double sx, double sxx, double count, int c,
                                                          const BnFinish &fin) {
    const BnMoments o = bn_moments(sx, sxx, count);
    fin.mean[c] = (float)o.mean;
    fin.invstd[c] = bn_invstd(o.var, fin.eps);
    bn_running_update(o, count, c, fin);
}
