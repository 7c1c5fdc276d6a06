// Calibration of the row softmax (lidog_amd.calibration): the reliability table and the proper scores of a batch of
// labelled logits, and one iteration of the temperature fit (Guo et al., ICML 2017).  Not in the reference, whose metrics
// are IoU only; include/lidog_amd.h states the arithmetic and tests/calibration_ref.py restates it in numpy.
//
// Both kernels are streaming passes in the shape of k_entropy_sums (entropy.hip): one thread per row, the row in
// registers, 256-thread workgroups in a grid-strided sweep of at most CAL_MAX_BLOCKS workgroups, the row arithmetic in
// double on the shifted logits.  The class count is a run-time value up to 32; a kernel is instantiated for 8, 16 and 32
// register slots and the unrolled class loops skip the slots past C (C is uniform: a scalar branch).
//
// What is bounded is summed as integers: the bins in LDS (k_eval_confusion's scheme), then one global integer atomic per
// non-empty bin and workgroup, so the table does not depend on the order of rows, the grid or the cut into batches.
// What is not (NLL, the fit's three sums) goes lanes -> wave (shuffles) -> workgroup (LDS) -> one double per workgroup
// in the workspace, and the LAST workgroup to arrive (an integer ticket) adds those in a fixed order: no floating-point
// atomic, one launch, the same bytes every time.
#include <math.h>

#include "common.h"

#define CAL_THREADS 256
#define CAL_MAX_BLOCKS 1024
#define CAL_MAX_CLASSES 32
#define CAL_MAX_BINS 64
#define CAL_Q 4294967296.0                  // 2^32: the unit of conf_q and brier_q
#define CAL_ERR_NONFINITE 2                 // bit 1 of the error word

namespace {
inline int64_t cal_blocks(int64_t n) {
    const int64_t nb = cdiv64(n, CAL_THREADS * 4);
    return nb < 1 ? 1 : (nb > CAL_MAX_BLOCKS ? CAL_MAX_BLOCKS : nb);
}

__device__ __forceinline__ bool cal_labelled(int64_t l, int C, int64_t ignore_label) {
    return l >= 0 && l < C && l != ignore_label;                // lidog_eval_confusion's rule
}

// the row into registers; m = its maximum, pred = the first maximal class (row_argmax.h's rule on a row without NaN).
// false: a logit is NaN or infinite.
template <int CP>
__device__ __forceinline__ bool cal_row(const float *__restrict__ x, int C, float (&v)[CP], float &m, int &pred) {
    bool finite = true;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        v[c] = 0.f;
        if (c < C) {
            v[c] = x[c];
            finite = finite && (fabsf(v[c]) <= 3.402823466e38f);
        }
    }
    m = v[0];
    pred = 0;
#pragma unroll
    for (int c = 1; c < CP; ++c)
        if (c < C && v[c] > m) {
            m = v[c];
            pred = c;
        }
    return finite;
}

// sums of K doubles over the workgroup in a fixed tree; valid in thread 0.  red: LDS [4][K]
template <int K>
__device__ __forceinline__ void cal_block_sum(double (&v)[K], double (*red)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[k] = v[k] + __shfl_down(v[k], d, 64);
    __syncthreads();                                    // red may still be read from an earlier use
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// s + x with its rounding error (Knuth's two-sum; the build keeps every operation on its own: -ffp-contract=off)
__device__ __forceinline__ void cal_two_sum(double &s, double &c, double x) {
    const double t = s + x, bb = t - s;
    c += (s - (t - bb)) + (x - bb);
    s = t;
}

// a compensated sum (s, c) over the workgroup in a fixed tree; valid in thread 0.  red: LDS [4][2]
__device__ __forceinline__ void cal_block_sum2(double &s, double &c, double (*red)[2]) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double s2 = __shfl_down(s, d, 64), c2 = __shfl_down(c, d, 64);
        cal_two_sum(s, c, s2);
        c += c2;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = s;
        red[threadIdx.x >> 6][1] = c;
    }
    __syncthreads();
    s = red[0][0];
    c = red[0][1];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        cal_two_sum(s, c, red[w][0]);
        c += red[w][1];
    }
}

// partial[b][K] of this workgroup is written; true in every thread of the last workgroup to get here, which then sees
// every workgroup's partials.  The ticket returns to 0 for the next launch.
template <int K>
__device__ __forceinline__ bool cal_arrive(const double (&v)[K], double *__restrict__ partial, unsigned *ticket) {
    __shared__ int s_last;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) partial[(size_t)blockIdx.x * K + k] = v[k];
        __threadfence();
        s_last = atomicAdd(ticket, 1u) == gridDim.x - 1;            // an integer ticket
    }
    __syncthreads();
    if (!s_last) return false;
    __threadfence();
    return true;
}

// the last workgroup: thread t adds partial[t], partial[t + 256], ... in that order, then the tree
template <int K>
__device__ __forceinline__ void cal_total(const double *partial, double (&v)[K], double (*red)[K]) {
    const volatile double *p = partial;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += CAL_THREADS)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = v[k] + p[(size_t)b * K + k];
    cal_block_sum<K>(v, red);
}
}  // namespace

// ------------------------------------------------------------------ the reliability table and the proper scores
template <int CP>
__global__ __launch_bounds__(CAL_THREADS) void k_calib_stats(const float *__restrict__ logits,
                                                             const int64_t *__restrict__ labels, int64_t n, int C,
                                                             int64_t ignore_label, const double *__restrict__ beta_p,
                                                             int B, unsigned long long *__restrict__ table,
                                                             unsigned long long *__restrict__ totals,
                                                             double *__restrict__ nll_sum, int32_t *__restrict__ err,
                                                             double *__restrict__ ws) {
    __shared__ unsigned long long bins[CAL_MAX_BINS * 3];
    __shared__ double red[4][2];
    __shared__ long long redi[4][2];
    for (int j = threadIdx.x; j < 3 * B; j += CAL_THREADS) bins[j] = 0;
    __syncthreads();
    const double beta = beta_p != nullptr ? beta_p[0] : 1.0;
    double nll = 0.0, nll_c = 0.0;                // a compensated sum: the terms span 1e-16 .. 1e4 and beyond
    long long rows = 0, brier_q = 0;
    int bad = 0;
    for (int64_t r = (int64_t)blockIdx.x * CAL_THREADS + threadIdx.x; r < n; r += (int64_t)gridDim.x * CAL_THREADS) {
        const int64_t l = labels[r];
        if (!cal_labelled(l, C, ignore_label)) continue;
        float v[CP], m;
        int pred;
        if (!cal_row<CP>(logits + r * C, C, v, m, pred)) {
            bad = 1;
            continue;
        }
        double e[CP], s = 0.0, zl = 0.0;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) {
                const double z = beta * ((double)v[c] - (double)m);
                e[c] = exp(z);
                s += e[c];
                if (c == (int)l) zl = z;
            }
        double brier = 0.0;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) {
                const double d = e[c] / s - (c == (int)l ? 1.0 : 0.0);
                brier += d * d;
            }
        const double conf = 1.0 / s;
        if (!(conf > 0.0)) {                        // a beta that is no positive finite number: reported, never binned
            bad = 1;
            continue;
        }
        int bin = (int)floor(conf * (double)B);
        bin = bin > B - 1 ? B - 1 : (bin < 0 ? 0 : bin);
        atomicAdd(&bins[3 * bin], 1ull);
        if (pred == (int)l) atomicAdd(&bins[3 * bin + 1], 1ull);
        atomicAdd(&bins[3 * bin + 2], (unsigned long long)llrint(conf * CAL_Q));
        cal_two_sum(nll, nll_c, log(s) - zl);
        brier_q += llrint(brier * CAL_Q);
        rows += 1;
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(err, CAL_ERR_NONFINITE);
    for (int j = threadIdx.x; j < 3 * B; j += CAL_THREADS)
        if (bins[j]) atomicAdd(&table[j], bins[j]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {              // integers: any order gives the same sum
        rows += __shfl_down(rows, d, 64);
        brier_q += __shfl_down(brier_q, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        redi[threadIdx.x >> 6][0] = rows;
        redi[threadIdx.x >> 6][1] = brier_q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long k = (redi[0][0] + redi[1][0]) + (redi[2][0] + redi[3][0]);
        if (k != 0) {
            atomicAdd(&totals[0], (unsigned long long)k);
            atomicAdd(&totals[1], (unsigned long long)((redi[0][1] + redi[1][1]) + (redi[2][1] + redi[3][1])));
        }
    }
    cal_block_sum2(nll, nll_c, red);
    double part[2] = {nll, nll_c};
    if (!cal_arrive<2>(part, ws + 1, (unsigned *)ws)) return;
    // the last workgroup: thread t adds the partials t, t + 256, ... in that order, then the tree
    const volatile double *p = ws + 1;
    nll = nll_c = 0.0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += CAL_THREADS) {
        cal_two_sum(nll, nll_c, p[2 * (size_t)b]);
        nll_c += p[2 * (size_t)b + 1];
    }
    cal_block_sum2(nll, nll_c, red);
    if (threadIdx.x == 0) {
        nll_sum[0] = nll_sum[0] + (nll + nll_c);
        *(unsigned *)ws = 0u;
    }
}

extern "C" int64_t lidog_calib_ws(int64_t n) { return 1 + 4 * cal_blocks(n > 0 ? n : 0); }

static int cal_check(const char *who, int64_t n, int32_t C) {
    LIDOG_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
    LIDOG_REQUIRE(C >= 2 && C <= CAL_MAX_CLASSES, "%s: %d classes (2..%d)", who, C, CAL_MAX_CLASSES);
    LIDOG_REQUIRE(n * (int64_t)C < ((int64_t)1 << 31), "%s: n * C = %lld reaches 2^31", who, (long long)(n * C));
    return 0;
}

extern "C" int lidog_calib_stats(const float *logits, const int64_t *labels, int64_t n, int32_t C, int64_t ignore_label,
                                 const double *beta, int32_t n_bins, int64_t *table, int64_t *totals, double *nll_sum,
                                 int32_t *err, double *ws, void *stream) {
    if (int rc = cal_check("lidog_calib_stats", n, C)) return rc;
    LIDOG_REQUIRE(n_bins >= 1 && n_bins <= CAL_MAX_BINS, "lidog_calib_stats: %d bins (1..%d)", n_bins, CAL_MAX_BINS);
    if (n == 0) return 0;
    LIDOG_REQUIRE(logits && labels && table && totals && nll_sum && err && ws, "lidog_calib_stats: null argument");
    LIDOG_REQUIRE((((uintptr_t)table | (uintptr_t)totals | (uintptr_t)nll_sum | (uintptr_t)ws |
                    (uintptr_t)beta) & 7) == 0, "lidog_calib_stats: table, totals, nll_sum, beta and ws are 8-byte aligned");
    const unsigned nb = (unsigned)cal_blocks(n);
    hipStream_t st = (hipStream_t)stream;
#define CALL(CP_)                                                                                                      \
    k_calib_stats<CP_><<<nb, CAL_THREADS, 0, st>>>(logits, labels, n, C, ignore_label, beta, n_bins,                  \
                                                   (unsigned long long *)table, (unsigned long long *)totals, nll_sum, \
                                                   err, ws)
    if (C <= 8) CALL(8);
    else if (C <= 16) CALL(16);
    else CALL(32);
#undef CALL
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ one iteration of the temperature fit
__global__ void k_calib_fit_init(double *__restrict__ state, double beta_min, double beta_max) {
    if (threadIdx.x < LIDOG_CALIB_STATE) {
        const double b = fmin(fmax(1.0, beta_min), beta_max);
        state[threadIdx.x] = threadIdx.x == LIDOG_CALIB_BETA ? b : threadIdx.x == LIDOG_CALIB_LO ? beta_min
                             : threadIdx.x == LIDOG_CALIB_HI ? beta_max : 0.0;
    }
}

extern "C" int lidog_calib_fit_init(double *state, double beta_min, double beta_max, void *stream) {
    LIDOG_REQUIRE(state != nullptr && ((uintptr_t)state & 7) == 0, "lidog_calib_fit_init: state is an 8-byte aligned array");
    LIDOG_REQUIRE(beta_min > 0 && beta_min <= beta_max && beta_max <= 1.79e308,
                  "lidog_calib_fit_init: 0 < beta_min <= beta_max, finite (got %g, %g)", beta_min, beta_max);
    k_calib_fit_init<<<1, 64, 0, (hipStream_t)stream>>>(state, beta_min, beta_max);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// the bracketed Newton update of the header, by one thread
__device__ __forceinline__ void cal_fit_update(double *__restrict__ state, double *__restrict__ trace, double L,
                                               double G, double H, double K, double beta_min, double beta_max) {
    const double beta = state[LIDOG_CALIB_BETA];
    double lo = state[LIDOG_CALIB_LO], hi = state[LIDOG_CALIB_HI];
    double nll = 0.0, g = 0.0, h = 0.0, next = beta;
    if (K > 0.0) {
        nll = L / K;
        g = G / K;
        h = H / K;
        if (g > 0.0) hi = beta;                       // g is non-decreasing: the minimum lies at or below beta
        else if (g < 0.0) lo = beta;
        else lo = hi = beta;
        const double cand = h > 0.0 ? beta - g / h : (g > 0.0 ? -INFINITY : g < 0.0 ? INFINITY : beta);
        if (cand == beta)
            next = beta;                              // the step is below beta's spacing: converged, stay
        else if (cand > lo && cand < hi)
            next = cand;                              // false for a NaN step as well
        else if (g < 0.0 && cand >= hi && hi == beta_max && beta != beta_max)
            next = beta_max;                          // the step leaves through the interval's own bound: look there
        else if (g > 0.0 && cand <= lo && lo == beta_min && beta != beta_min)
            next = beta_min;
        else
            next = lo + (hi - lo) * 0.5;
        next = fmin(fmax(next, beta_min), beta_max);
    }
    trace[0] = beta;
    trace[1] = nll;
    trace[2] = g;
    state[LIDOG_CALIB_BETA] = next;
    state[LIDOG_CALIB_LO] = lo;
    state[LIDOG_CALIB_HI] = hi;
    state[LIDOG_CALIB_NLL] = nll;
    state[LIDOG_CALIB_G] = g;
    state[LIDOG_CALIB_H] = h;
    state[LIDOG_CALIB_ITER] = state[LIDOG_CALIB_ITER] + 1.0;
    state[LIDOG_CALIB_ROWS] = K;
}

template <int CP>
__global__ __launch_bounds__(CAL_THREADS) void k_calib_fit_step(const float *__restrict__ logits,
                                                                const int64_t *__restrict__ labels, int64_t n, int C,
                                                                int64_t ignore_label, double beta_min, double beta_max,
                                                                double *__restrict__ state, double *__restrict__ trace,
                                                                int32_t *__restrict__ err, double *__restrict__ ws) {
    __shared__ double red[4][4];
    const double beta = state[LIDOG_CALIB_BETA];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};           // sum of log s - beta z_label, of E_p[z] - z_label, of Var_p[z]; rows
    int bad = 0;
    for (int64_t r = (int64_t)blockIdx.x * CAL_THREADS + threadIdx.x; r < n; r += (int64_t)gridDim.x * CAL_THREADS) {
        const int64_t l = labels[r];
        if (!cal_labelled(l, C, ignore_label)) continue;
        float v[CP], m;
        int pred;
        if (!cal_row<CP>(logits + r * C, C, v, m, pred)) {
            bad = 1;
            continue;
        }
        double e[CP], s = 0.0, ez = 0.0, zl = 0.0;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) {
                const double z = (double)v[c] - (double)m;
                e[c] = exp(beta * z);
                s += e[c];
                ez += e[c] * z;
                if (c == (int)l) zl = z;
            }
        const double mean = ez / s;
        double var = 0.0;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) {
                const double d = ((double)v[c] - (double)m) - mean;
                var += e[c] * (d * d);
            }
        acc[0] += log(s) - beta * zl;
        acc[1] += mean - zl;
        acc[2] += var / s;
        acc[3] += 1.0;
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(err, CAL_ERR_NONFINITE);
    cal_block_sum<4>(acc, red);
    if (!cal_arrive<4>(acc, ws + 1, (unsigned *)ws)) return;
    cal_total<4>(ws + 1, acc, red);
    if (threadIdx.x == 0) {
        cal_fit_update(state, trace, acc[0], acc[1], acc[2], acc[3], beta_min, beta_max);
        *(unsigned *)ws = 0u;
    }
}

extern "C" int lidog_calib_fit_step(const float *logits, const int64_t *labels, int64_t n, int32_t C,
                                    int64_t ignore_label, double beta_min, double beta_max, double *state, double *trace,
                                    int32_t *err, double *ws, void *stream) {
    if (int rc = cal_check("lidog_calib_fit_step", n, C)) return rc;
    LIDOG_REQUIRE(beta_min > 0 && beta_min <= beta_max && beta_max <= 1.79e308,
                  "lidog_calib_fit_step: 0 < beta_min <= beta_max, finite (got %g, %g)", beta_min, beta_max);
    LIDOG_REQUIRE(state && trace && err && ws && (n == 0 || (logits && labels)), "lidog_calib_fit_step: null argument");
    LIDOG_REQUIRE((((uintptr_t)state | (uintptr_t)trace | (uintptr_t)ws) & 7) == 0,
                  "lidog_calib_fit_step: state, trace and ws are 8-byte aligned");
    const unsigned nb = (unsigned)cal_blocks(n);        // one workgroup even for n == 0: the state still moves on
    hipStream_t st = (hipStream_t)stream;
#define CALL(CP_)                                                                                                     \
    k_calib_fit_step<CP_><<<nb, CAL_THREADS, 0, st>>>(logits, labels, n, C, ignore_label, beta_min, beta_max, state, \
                                                      trace, err, ws)
    if (C <= 8) CALL(8);
    else if (C <= 16) CALL(16);
    else CALL(32);
#undef CALL
    LIDOG_LAUNCH_CHECK();
    return 0;
}
