// MixStyle's finishing step of the per-(scan, channel) reduction of inorm.hip (k_in_reduce4 / k_in_reduce_scalar, MODE 2):
// what follows the double sums (sum x, sum x^2) of every (b, c).  The definition is stated in include/lidog_amd.h
// (lidog_mixstyle_stats); tests/mixstyle_ref.py restates it in float64.
//
// Two phases with a workgroup barrier between them, because a scan's tables need its partner's statistics:
//   ms_moments   mu, sig of one (b, c) in double (unbiased variance); kept in double for phase two and rounded once
//                into the float outputs mean / sig
//   ms_tables    (sub, scale, add) of one (b, c) from its own and its partner's (mu, sig), rounded once from double
// The float4 path runs both in the last workgroup of the reduction's tail (moments kept in its LDS); the scalar path
// keeps the moments in the workspace and runs phase two as a launch of B C threads behind the reduction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct MsMix {
    const float *lam;         // [B] device
    const int32_t *partner;   // [B] device, every entry in [0, B) (checked on the host by lidog_mixstyle_stats)
    float *sig, *sub, *scale, *add;   // [B, C] each
};

// cnt rows: mu = s0 / cnt, var = max(0, (s1 - s0^2 / cnt) / (cnt - 1)), sig = sqrt(var + eps); var = 0 for cnt < 2 and
// mu = 0 for a scan without rows
__device__ __forceinline__ void ms_moments(double s0, double s1, double cnt, double eps, double &mu, double &sig) {
    mu = 0.0;
    double var = 0.0;
    if (cnt > 0) mu = s0 / cnt;
    if (cnt > 1) {
        var = (s1 - s0 * s0 / cnt) / (cnt - 1.0);
        if (var < 0) var = 0;
    }
    sig = sqrt(var + eps);
}

// mom: [2][B C] doubles (mu, then sig) of every (b, c), complete and visible to this thread
__device__ __forceinline__ void ms_tables(const MsMix &m, const int32_t *__restrict__ seg_off, const double *mom, int B,
                                          int C, int j) {
    const int b = j / C, c = j - b * C, BC = B * C;
    const int p = m.partner[b];
    const float lam = m.lam[b];
    const int nb = seg_off[b + 1] - seg_off[b], np = seg_off[p + 1] - seg_off[p];
    // an identity scan: y == x and dx == dy bit for bit.  add is the zero with the sign bit set (it compares equal to
    // 0): fmaf(x, 1, -0) keeps the sign of a zero x, fmaf(-0, 1, +0) would give +0
    float sub = 0.f, scale = 1.f, add = -0.f;
    if (nb >= 2 && np >= 2 && p != b && lam != 1.f) {
        const double l = (double)lam;
        const double mu_b = mom[j], sig_b = mom[BC + j], mu_p = mom[p * C + c], sig_p = mom[BC + p * C + c];
        const double mu_mix = l * mu_b + (1.0 - l) * mu_p;
        const double sig_mix = l * sig_b + (1.0 - l) * sig_p;
        sub = (float)mu_b;
        scale = (float)(sig_mix / sig_b);
        add = (float)mu_mix;
    }
    m.sub[j] = sub;
    m.scale[j] = scale;
    m.add[j] = add;
}

// inorm.hip: the MODE 2 launch of the instance norm's reduction.  mean / mix.sig / mix.sub / mix.scale / mix.add
// [B, C] float; ws: lidog_in_reduce_ws(B, C) doubles.  One launch on the float4 path, two on the scalar one.
int lidog_in_reduce_mixstyle(const float *x, int64_t n, int C, int B, const int32_t *perm, const int32_t *seg_off,
                             float eps, float *mean, const MsMix &mix, double *ws, hipStream_t st);
