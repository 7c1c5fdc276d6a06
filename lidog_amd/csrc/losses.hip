// DICE losses of the LiDOG step, one pass forward and one pass backward over the logits.
// Reference: utils/losses/losses.py:56-97 (DICELoss), :100-187 (SoftDICELoss), called from
// utils/pipelines/trainer_lighting_2d.py:172-190 on the semantic logits [N,7] and on the BEV logits
// (NCHW read through .view(-1, 7)).  The torch formulation costs ~30 elementwise/reduction launches per loss,
// several of them column reductions of a 7-column matrix; here: softmax + the four per-class sums in one kernel
// (per-workgroup fp64 partials added in a fixed order: reproducible), a one-block finalize that also emits the
// per-class coefficients of the gradient, and one kernel for d loss / d logits.
//   loss = 1 - sum_c present_c * 2 I_c / U_c / (sum_c present_c + 1e-12),
//   I_c = sum_r p_rc t_rc,  U_c = sum_r (p_rc^2 or p_rc) + sum_r t_rc + 1e-12,
//   t = one-hot (DICE) or label-smoothed one-hot (soft: 1-eps / eps/(C-1)); rows with the ignore label are skipped.
//   KITTI soft labels (get_kitti_soft, losses.py:112-126; `kitti` != 0): a row labelled 1 or 6 carries (1-eps)/2 on
//   classes 1 and 6 both; the present-class count still takes the hard label.
// Weighted cross-entropy and the focal loss on top of it (CELoss losses.py:8-25, FocalLoss :423-436), further down:
//   ce = sum_r w[t_r] (lse(x_r) - x_r[t_r]) / sum_r w[t_r] over the rows whose label is neither the ignore label nor
//   outside [0, C);  focal = alpha (1 - exp(-ce))^gamma ce, a scalar function of ce: one pass each way for both.
#include "criteria.h"

#define DL_MAX_BLOCKS 1024

// partial[block][4][C] = (I, sum p^2 or p, sum t, count of rows of the class)
template <int C>
__global__ __launch_bounds__(256) void k_dice_sums(const float *__restrict__ logits, const int64_t *__restrict__ target,
                                                   int64_t n, int64_t ignore, int has_ignore, float t_on, float t_off,
                                                   int powerize, int kitti, double *__restrict__ partial) {
    __shared__ double red[4][4 * C];
    float acc[4 * C];
#pragma unroll
    for (int i = 0; i < 4 * C; ++i) acc[i] = 0.f;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        const int64_t t = target[r];
        if (has_ignore && t == ignore) continue;
        float p[C];
        softmax_row<C>(logits + r * C, p);
        const bool pair = kitti && (t == 1 || t == 6);   // classes 1 and 6 share the row's mass
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const bool on = (t == c);
            const float tw = (pair && (c == 1 || c == 6)) ? 0.5f * t_on : (on ? t_on : t_off);
            acc[c] += p[c] * tw;
            acc[C + c] += powerize ? p[c] * p[c] : p[c];
            acc[2 * C + c] += tw;
            acc[3 * C + c] += on ? 1.f : 0.f;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 4 * C; ++i) {
        double v = (double)acc[i];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4 * C)
        partial[(size_t)blockIdx.x * 4 * C + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// one block: sums[4C] over the partials in block order; loss; coef[2C] = (a_c, b_c) with
// d loss / d p_rc = a_c * t_rc + b_c * (2 p_rc or 1)
__global__ __launch_bounds__(1024) void k_dice_finish(const double *__restrict__ partial, int nb, int C, int use_tmask,
                                                     float offset, float *__restrict__ loss, float *__restrict__ coef) {
    // 8 lanes per column: lane l adds the partials b = l, l + 8, ...; the 8 lane sums are combined in lane order
    // (fixed order: bit-reproducible).  One thread per column took 56 us on the step's forward -> backward seam.
    __shared__ double s[4 * DL_MAXC];
    __shared__ double part[8][4 * DL_MAXC];
    const int i = threadIdx.x >> 3, l = threadIdx.x & 7;
    if (i < 4 * C) {
        double v = 0;
        for (int b = l; b < nb; b += 8) v += partial[(size_t)b * 4 * C + i];
        part[l][i] = v;
    }
    __syncthreads();
    if (l == 0 && i < 4 * C) {
        double v = part[0][i];
#pragma unroll
        for (int q = 1; q < 8; ++q) v += part[q][i];
        s[i] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double np = 0, acc = 0;
        for (int c = 0; c < C; ++c) {
            const double pres = use_tmask ? (s[3 * C + c] > 0 ? 1.0 : 0.0) : 1.0;
            const double uni = s[C + c] + s[2 * C + c] + 1e-12;
            np += pres;
            acc += pres * 2.0 * s[c] / uni;
        }
        const double den = np + 1e-12;
        loss[0] = (float)(1.0 - acc / den) + offset;
        for (int c = 0; c < C; ++c) {
            const double pres = use_tmask ? (s[3 * C + c] > 0 ? 1.0 : 0.0) : 1.0;
            const double uni = s[C + c] + s[2 * C + c] + 1e-12;
            coef[c] = (float)(-2.0 * pres / den / uni);
            coef[C + c] = (float)(2.0 * pres / den * s[c] / (uni * uni));
        }
    }
}

template <int C>
__global__ __launch_bounds__(256) void k_dice_bwd(const float *__restrict__ logits, const int64_t *__restrict__ target,
                                                  int64_t n, int64_t ignore, int has_ignore, float t_on, float t_off,
                                                  int powerize, int kitti, const float *__restrict__ coef,
                                                  const float *__restrict__ gout, float *__restrict__ glogits) {
    float a[C], b[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        a[c] = coef[c];
        b[c] = coef[C + c];
    }
    const float go = gout[0];
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        const int64_t t = target[r];
        float *g = glogits + r * C;
        if (has_ignore && t == ignore) {
#pragma unroll
            for (int c = 0; c < C; ++c) g[c] = 0.f;
            continue;
        }
        float p[C], gp[C];
        softmax_row<C>(logits + r * C, p);
        float dot = 0.f;
        const bool pair = kitti && (t == 1 || t == 6);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float tw = (pair && (c == 1 || c == 6)) ? 0.5f * t_on : ((t == c) ? t_on : t_off);
            gp[c] = a[c] * tw + b[c] * (powerize ? 2.f * p[c] : 1.f);
            dot += p[c] * gp[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = go * p[c] * (gp[c] - dot);
    }
}

static int dice_blocks(int64_t n) {
    int64_t nb = cdiv64(n, 256 * 4);
    if (nb < 1) nb = 1;
    return (int)(nb > DL_MAX_BLOCKS ? DL_MAX_BLOCKS : nb);
}

extern "C" int64_t lidog_dice_ws(int32_t C) { return (int64_t)DL_MAX_BLOCKS * 4 * C; }

static int dice_fwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                    int32_t has_ignore, float eps, int32_t soft, int32_t powerize, int32_t use_tmask, float offset,
                    int32_t kitti, double *ws, float *loss, float *coef, hipStream_t st) {
    LIDOG_REQUIRE(n >= 0 && C >= 2 && C <= DL_MAXC, "dice: bad shape");
    const float t_on = soft ? 1.f - eps : 1.f, t_off = soft ? eps / (float)(C - 1) : 0.f;
    const int nb = dice_blocks(n);
#define CALL(C_) \
    k_dice_sums<C_><<<nb, 256, 0, st>>>(logits, target, n, ignore_label, has_ignore, t_on, t_off, powerize, kitti, ws)
    DICE_DISPATCH(CALL)
#undef CALL
    k_dice_finish<<<1, 1024, 0, st>>>(ws, nb, C, use_tmask, offset, loss, coef);   // 8 lanes x 4C <= 80 columns
    LIDOG_LAUNCH_CHECK();
    return 0;
}

static int dice_bwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                    int32_t has_ignore, float eps, int32_t soft, int32_t powerize, int32_t kitti, const float *coef,
                    const float *gout, float *glogits, hipStream_t st) {
    if (n == 0) return 0;
    const float t_on = soft ? 1.f - eps : 1.f, t_off = soft ? eps / (float)(C - 1) : 0.f;
    int64_t nb = cdiv64(n, 256);
    if (nb > 4096) nb = 4096;
#define CALL(C_)                                                                                                \
    k_dice_bwd<C_><<<(unsigned)nb, 256, 0, st>>>(logits, target, n, ignore_label, has_ignore, t_on, t_off, powerize, \
                                                 kitti, coef, gout, glogits)
    DICE_DISPATCH(CALL)
#undef CALL
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_dice_fwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                              int32_t has_ignore, float eps, int32_t soft, int32_t powerize, int32_t use_tmask,
                              float offset, double *ws, float *loss, float *coef, void *stream) {
    return dice_fwd(logits, target, n, C, ignore_label, has_ignore, eps, soft, powerize, use_tmask, offset, 0, ws, loss,
                    coef, (hipStream_t)stream);
}

extern "C" int lidog_dice_bwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                              int32_t has_ignore, float eps, int32_t soft, int32_t powerize, const float *coef,
                              const float *gout, float *glogits, void *stream) {
    return dice_bwd(logits, target, n, C, ignore_label, has_ignore, eps, soft, powerize, 0, coef, gout, glogits,
                    (hipStream_t)stream);
}

// SoftDICELoss(is_kitti=True): always the label-smoothed targets; classes 1 and 6 must exist
extern "C" int lidog_dice_kitti_fwd(const float *logits, const int64_t *target, int64_t n, int32_t C,
                                    int64_t ignore_label, int32_t has_ignore, float eps, int32_t powerize,
                                    int32_t use_tmask, float offset, double *ws, float *loss, float *coef,
                                    void *stream) {
    LIDOG_REQUIRE(C >= 7, "dice_kitti: the soft labels pair classes 1 and 6: C must be in [7, 20]");
    return dice_fwd(logits, target, n, C, ignore_label, has_ignore, eps, 1, powerize, use_tmask, offset, 1, ws, loss,
                    coef, (hipStream_t)stream);
}

extern "C" int lidog_dice_kitti_bwd(const float *logits, const int64_t *target, int64_t n, int32_t C,
                                    int64_t ignore_label, int32_t has_ignore, float eps, int32_t powerize,
                                    const float *coef, const float *gout, float *glogits, void *stream) {
    LIDOG_REQUIRE(n >= 0 && C >= 7 && C <= DL_MAXC, "dice_kitti: bad shape (C must be in [7, 20])");
    return dice_bwd(logits, target, n, C, ignore_label, has_ignore, eps, 1, powerize, 1, coef, gout, glogits,
                    (hipStream_t)stream);
}

// ------------------------------------------------------------------ weighted cross-entropy, focal loss
// A row takes part when its label is not the ignore label and lies in [0, C) (torch asserts on the device for any other
// label; a kernel cannot raise without a synchronisation, so such a row gets zero weight and a zero gradient, and the
// weight table is never read for it).
// partial[block][2] = (sum w[t] nll, sum w[t])
template <int C>
__global__ __launch_bounds__(256) void k_ce_sums(const float *__restrict__ logits, const int64_t *__restrict__ target,
                                                 int64_t n, int64_t ignore, int has_ignore,
                                                 const float *__restrict__ weight, double *__restrict__ partial) {
    __shared__ double red[4][2];
    float acc_s = 0.f, acc_w = 0.f;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        const int64_t t = target[r];
        if ((has_ignore && t == ignore) || t < 0 || t >= C) continue;
        const float *x = logits + r * C;
        float v[C];
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = x[c];
        float m = v[0], xt = v[0];
#pragma unroll
        for (int c = 1; c < C; ++c) {
            m = fmaxf(m, v[c]);
            xt = (t == c) ? v[c] : xt;
        }
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) s += expf(v[c] - m);
        const float nll = logf(s) - (xt - m);
        const float w = weight ? weight[t] : 1.f;
        acc_s += w * nll;
        acc_w += w;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double vs = (double)acc_s, vw = (double)acc_w;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        vs += __shfl_down(vs, d);
        vw += __shfl_down(vw, d);
    }
    if (lane == 0) {
        red[wave][0] = vs;
        red[wave][1] = vw;
    }
    __syncthreads();
    if (threadIdx.x < 2)
        partial[(size_t)blockIdx.x * 2 + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// one block: (S, W) over the partials in a fixed order; ce = S / W; loss = ce or alpha (1 - exp(-ce))^gamma ce;
// coef[0] = (d loss / d ce) / W, the one coefficient the backward pass needs
__global__ __launch_bounds__(256) void k_ce_finish(const double *__restrict__ partial, int nb, int focal, double alpha,
                                                   double gamma, float *__restrict__ loss, float *__restrict__ coef) {
    __shared__ double part[256][2];
    double s = 0, w = 0;
    for (int b = threadIdx.x; b < nb; b += 256) {
        s += partial[(size_t)b * 2];
        w += partial[(size_t)b * 2 + 1];
    }
    part[threadIdx.x][0] = s;
    part[threadIdx.x][1] = w;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {      // a fixed tree: bit-reproducible
        if ((int)threadIdx.x < d) {
            part[threadIdx.x][0] += part[threadIdx.x + d][0];
            part[threadIdx.x][1] += part[threadIdx.x + d][1];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double S = part[0][0], W = part[0][1];
        const double ce = S / W;
        double l = ce, dl = 1.0;
        if (focal) {
            const double pt = exp(-ce), q = 1.0 - pt;
            const double qg = pow(q, gamma);
            l = alpha * qg * ce;
            // d/dce: gamma q^(gamma-1) pt ce + q^gamma; a zero exponent has a zero derivative whatever q is
            dl = alpha * ((gamma == 0.0 ? 0.0 : gamma * pow(q, gamma - 1.0) * pt * ce) + qg);
        }
        loss[0] = (float)l;
        coef[0] = (float)(dl / W);
    }
}

template <int C>
__global__ __launch_bounds__(256) void k_ce_bwd(const float *__restrict__ logits, const int64_t *__restrict__ target,
                                                int64_t n, int64_t ignore, int has_ignore,
                                                const float *__restrict__ weight, const float *__restrict__ coef,
                                                const float *__restrict__ gout, float *__restrict__ glogits) {
    const float gk = gout[0] * coef[0];
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        const int64_t t = target[r];
        float *g = glogits + r * C;
        if ((has_ignore && t == ignore) || t < 0 || t >= C) {
#pragma unroll
            for (int c = 0; c < C; ++c) g[c] = 0.f;
            continue;
        }
        float p[C];
        softmax_row<C>(logits + r * C, p);
        const float s = gk * (weight ? weight[t] : 1.f);
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = s * (p[c] - ((t == c) ? 1.f : 0.f));
    }
}

extern "C" int64_t lidog_ce_ws(int32_t C) { return (int64_t)DL_MAX_BLOCKS * 2; }

extern "C" int lidog_ce_fwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                            int32_t has_ignore, const float *weight, int32_t focal, double alpha, double gamma,
                            double *ws, float *loss, float *coef, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0 && C >= 2 && C <= DL_MAXC, "ce: bad shape");
    const int nb = dice_blocks(n);
#define CALL(C_) k_ce_sums<C_><<<nb, 256, 0, st>>>(logits, target, n, ignore_label, has_ignore, weight, ws)
    DICE_DISPATCH(CALL)
#undef CALL
    k_ce_finish<<<1, 256, 0, st>>>(ws, nb, focal, alpha, gamma, loss, coef);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_ce_bwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                            int32_t has_ignore, const float *weight, const float *coef, const float *gout,
                            float *glogits, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0 && C >= 2 && C <= DL_MAXC, "ce: bad shape");
    if (n == 0) return 0;
    int64_t nb = cdiv64(n, 256);
    if (nb > 4096) nb = 4096;
#define CALL(C_) \
    k_ce_bwd<C_><<<(unsigned)nb, 256, 0, st>>>(logits, target, n, ignore_label, has_ignore, weight, coef, gout, glogits)
    DICE_DISPATCH(CALL)
#undef CALL
    LIDOG_LAUNCH_CHECK();
    return 0;
}
