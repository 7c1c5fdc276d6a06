// Lovasz-softmax (Berman et al., CVPR 2018; lovasz_softmax_flat with classes='present') on logits [n, C]: the auxiliary
// point criterion of the training steps.  A row is valid when its label is not the ignore label and lies in [0, C) (the
// rule of lidog_ce_fwd); m = the valid rows, p = the fp32 row softmax.  For a class c carried by a valid row:
//   fg_i = [t_i == c],  e_i = |fg_i - p_ic|;  pi = the valid rows by descending e (fp32 values), ties by ascending row;
//   G = sum fg,  cf_j = sum_{k <= j} fg_pi(k)                                        (integers)
//   J(0, .) = 0,  J(j, cf) = 1.0 - (double)(G - cf) / (double)(G + j - cf)           (j = 1 .. m)
//   g_j = J(j, cf_j) - J(j - 1, cf_j - fg_pi(j)),   loss_c = sum_j e_pi(j) g_j,   loss = mean of loss_c over those classes.
// g_j depends on integers and on one double division and two double subtractions alone, so after one integer prefix sum
// every position is independent of its neighbours, and a float64 restatement has the same bits.
// Forward, 26 launches and memsets whatever n is:
//   (a) k_lv_keys: softmax, and per (class, row) the key 0x3F800000 - bits(e) (ascending-sortable: 0 <= e <= 1 in fp32,
//       every exp term is <= their sum and that sum is >= 1), 0xFFFFFFFF for an invalid row, the payload c n + row, e;
//   (b) ONE stable radix sort of the C n pairs on the key (prims.h: 4 passes of 9 bits cover the 32 key bits), then one
//       stable pass on the class c = payload / n: segment c of the result is class c in the order pi, invalid rows last;
//   (c) k_lv_flags + the integer exclusive scan of prims.h over fg in sorted order (and over the rows' validity behind
//       it: cf, G and m are differences of that one scan), then k_lv_grad: g_j in double, coef scattered by row, and
//       e g added into per-workgroup fp64 partials in a fixed order;
//   (d) k_lv_finish: the partials in a fixed order, loss and 1 / P.
// No floating-point atomics, no device -> host read: launch sizes come from n and C.  Backward: one pass per row.
#include "criteria.h"
#include "prims.h"

#define LV_KEY_ONE 0x3F800000u          // bits(1.0f)
#define LV_KEY_INVALID 0xFFFFFFFFu      // above every valid key, whatever the logits hold
#define LV_KEY_PASSES 4                 // 4 x 9 bits >= the 32 bits of a key
#define LV_MAX_XBLOCKS 1024             // workgroups per class of k_lv_grad = fp64 partials per class

__device__ __forceinline__ bool lv_valid(int64_t t, int C, int64_t ignore, int has_ignore) {
    return !(has_ignore && t == ignore) && t >= 0 && t < C;
}

// (a) class-major: position c n + r holds (key, payload c n + r, e) of row r in class c; valid[r] behind the C n flags
template <int C>
__global__ __launch_bounds__(256) void k_lv_keys(const float *__restrict__ logits, const int64_t *__restrict__ target,
                                                 int64_t n, int64_t ignore, int has_ignore, uint32_t *__restrict__ keys,
                                                 int32_t *__restrict__ vals, float *__restrict__ err,
                                                 int32_t *__restrict__ valid) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int64_t t = target[r];
    const bool ok = lv_valid(t, C, ignore, has_ignore);
    float p[C];
    if (ok) softmax_row<C>(logits + r * C, p);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int64_t s = (int64_t)c * n + r;
        float e = 0.f;
        uint32_t key = LV_KEY_INVALID;
        if (ok) {
            e = fabsf((t == c ? 1.f : 0.f) - p[c]);
            key = LV_KEY_ONE - __float_as_uint(e);
        }
        keys[s] = key;
        vals[s] = (int32_t)s;
        err[s] = e;
    }
    valid[r] = ok ? 1 : 0;
}

// (b) the key of the last pass: the class of the payload
__global__ __launch_bounds__(256) void k_lv_class_keys(const int32_t *__restrict__ vals, int64_t total, uint32_t n,
                                                       uint32_t *__restrict__ keys) {
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < total; s += (int64_t)gridDim.x * 256)
        keys[s] = (uint32_t)vals[s] / n;
}

// (c) flag[c n + j] = fg of the row at sorted position j of class c; flag[(C + 1) n] = 0 closes the scanned array, so
// that every count is a difference of two entries of the exclusive scan
__global__ __launch_bounds__(256) void k_lv_flags(const int32_t *__restrict__ vals, const int64_t *__restrict__ target,
                                                  int64_t n, int C, int64_t ignore, int has_ignore,
                                                  int32_t *__restrict__ flag) {
    const int c = blockIdx.y;
    if (blockIdx.x == 0 && c == 0 && threadIdx.x == 0) flag[(int64_t)(C + 1) * n] = 0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        const int64_t s = (int64_t)c * n + j, row = (int64_t)vals[s] - (int64_t)c * n;
        int fg = 0;
        if (row >= 0 && row < n) {     // a sorted payload of class c is c n + row: never false, and no address without it
            const int64_t t = target[row];
            fg = (t == c && !(has_ignore && t == ignore)) ? 1 : 0;
        }
        flag[s] = fg;
    }
}

// ex = the exclusive scan of flag [(C + 1) n + 1].  Sorted position j (1-based) of class c: cf = ex[c n + j] - ex[c n],
// fg = ex[c n + j] - ex[c n + j - 1], G = ex[(c + 1) n] - ex[c n], m = ex[(C + 1) n] - ex[C n].  coef[row][c] = g sign(p -
// fg) with sign(0) = 0; +0 for the invalid rows (positions j > m) and the absent classes (G = 0).
// partial[c gridDim.x + block] = sum of e g over the block's positions: per thread in position order, then the 64 lanes
// and the 4 waves in a fixed order.
__global__ __launch_bounds__(256) void k_lv_grad(const int32_t *__restrict__ vals, const int32_t *__restrict__ ex,
                                                 const float *__restrict__ err, int64_t n, int C,
                                                 float *__restrict__ coef, double *__restrict__ partial) {
    __shared__ double red[4];
    const int c = blockIdx.y;
    const int64_t seg = (int64_t)c * n;
    const int base = ex[seg], G = ex[seg + n] - base;
    const int64_t m = ex[(int64_t)(C + 1) * n] - ex[(int64_t)C * n];
    double acc = 0.0;
    for (int64_t j0 = (int64_t)blockIdx.x * 256 + threadIdx.x; j0 < n; j0 += (int64_t)gridDim.x * 256) {
        const int64_t s = seg + j0, j = j0 + 1, row = (int64_t)vals[s] - seg;
        if (row < 0 || row >= n) continue;      // as in k_lv_flags
        float cv = 0.f;
        if (G > 0 && j <= m) {
            const int x0 = ex[s], x1 = ex[s + 1];
            const int fg = x1 - x0;
            const int64_t cf = x1 - base, cf0 = cf - fg;
            const float e = err[seg + row];
            const double j1 = 1.0 - (double)(G - cf) / (double)(G + j - cf);
            const double jp = j == 1 ? 0.0 : 1.0 - (double)(G - cf0) / (double)(G + (j - 1) - cf0);
            const double g = j1 - jp;
            acc += (double)e * g;
            const float gf = (float)g;
            cv = e == 0.f ? 0.f : (fg ? -gf : gf);
        }
        coef[row * C + c] = cv;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)c * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// (d) one block: the np partials in a fixed order; P = the classes with G > 0; loss = sum / P; inv_p = 1 / P (0: P = 0)
__global__ __launch_bounds__(256) void k_lv_finish(const double *__restrict__ partial, int np,
                                                   const int32_t *__restrict__ ex, int64_t n, int C,
                                                   float *__restrict__ loss, float *__restrict__ inv_p) {
    __shared__ double part[256];
    double s = 0.0;
    for (int b = threadIdx.x; b < np; b += 256) s += partial[b];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {      // a fixed tree: bit-reproducible
        if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int P = 0;
        for (int c = 0; c < C; ++c) P += ex[(int64_t)(c + 1) * n] - ex[(int64_t)c * n] > 0 ? 1 : 0;
        loss[0] = P ? (float)(part[0] / (double)P) : 0.f;
        inv_p[0] = P ? (float)(1.0 / (double)P) : 0.f;
    }
}

// glogits_i = gout p_i (q_i - <q_i, p_i>) with q = coef / P; +0 in the invalid rows
template <int C>
__global__ __launch_bounds__(256) void k_lv_bwd(const float *__restrict__ logits, const int64_t *__restrict__ target,
                                                int64_t n, int64_t ignore, int has_ignore,
                                                const float *__restrict__ coef, const float *__restrict__ inv_p,
                                                const float *__restrict__ gout, float *__restrict__ glogits) {
    const float go = gout[0], ip = inv_p[0];
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        float *g = glogits + r * C;
        if (!lv_valid(target[r], C, ignore, has_ignore)) {
#pragma unroll
            for (int c = 0; c < C; ++c) g[c] = 0.f;
            continue;
        }
        float p[C], q[C];
        softmax_row<C>(logits + r * C, p);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            q[c] = coef[r * C + c] * ip;
            dot += p[c] * q[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = go * p[c] * (q[c] - dot);
    }
}

// ------------------------------------------------------------------ host side
// the pieces of the workspace, each on a 256-byte boundary; N = C n pairs
struct LvWs {
    uint32_t *ka, *kb;
    int32_t *va, *vb, *hist, *flag, *sums;
    float *err;
    double *partial;
    int64_t bytes;
};

static LvWs lv_ws(void *ws, int64_t n, int32_t C) {
    const int64_t N = n * C, L = N + n + 1;
    char *p = (char *)ws;
    LvWs w;
    auto take = [&](int64_t bytes) { char *q = p; p += lidog_align256(bytes); return q; };
    w.ka = (uint32_t *)take(4 * N);
    w.kb = (uint32_t *)take(4 * N);
    w.va = (int32_t *)take(4 * N);
    w.vb = (int32_t *)take(4 * N);
    w.hist = (int32_t *)take(4 * lidog_radix_sort_hist_ints(N, LV_KEY_PASSES));
    w.flag = (int32_t *)take(4 * L);
    w.sums = (int32_t *)take(4 * lidog_scan_sums_ints(L));
    w.err = (float *)take(4 * N);
    w.partial = (double *)take(8 * (int64_t)C * LV_MAX_XBLOCKS);
    w.bytes = p - (char *)ws;
    return w;
}

static bool lv_shape_ok(int64_t n, int32_t C) {
    return C >= 2 && C <= DL_MAXC && n >= 0 && n < ((int64_t)1 << 31) / C + 1 && n * C < ((int64_t)1 << 31);
}

extern "C" int64_t lidog_lovasz_ws(int64_t n, int32_t C) { return lv_shape_ok(n, C) ? lv_ws(nullptr, n, C).bytes : 0; }

extern "C" int lidog_lovasz_fwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                                int32_t has_ignore, void *ws, float *loss, float *coef, float *err_out, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(lv_shape_ok(n, C), "lovasz: n >= 0, C in [2, 20] and n C < 2^31, got n = %lld, C = %d", (long long)n, C);
    if (n == 0) {       // loss 0 and 1 / P = 0: coef is its tail word alone
        LIDOG_CHECK_HIP(hipMemsetAsync(loss, 0, sizeof(float), st));
        LIDOG_CHECK_HIP(hipMemsetAsync(coef, 0, sizeof(float), st));
        return 0;
    }
    const LvWs w = lv_ws(ws, n, C);
    const int64_t N = n * C, L = N + n + 1;
    float *err = err_out ? err_out : w.err;
    const unsigned rows_blocks = (unsigned)cdiv64(n, 256);
#define CALL(C_) \
    k_lv_keys<C_><<<rows_blocks, 256, 0, st>>>(logits, target, n, ignore_label, has_ignore, w.ka, w.va, err, w.flag + N)
    DICE_DISPATCH(CALL)
#undef CALL
    // an even number of passes leaves the pairs in (ka, va); the class pass moves them to (kb, vb)
    if (lidog_radix_sort_pairs(w.ka, w.va, w.kb, w.vb, N, LV_KEY_PASSES, w.hist, st)) return 1;
    int64_t nb = cdiv64(N, 1024);
    k_lv_class_keys<<<(unsigned)(nb > 4096 ? 4096 : nb), 256, 0, st>>>(w.va, N, (uint32_t)n, w.ka);
    if (lidog_radix_sort_pairs(w.ka, w.va, w.kb, w.vb, N, 1, w.hist, st)) return 1;
    int64_t xb = cdiv64(n, 1024);
    if (xb > LV_MAX_XBLOCKS) xb = LV_MAX_XBLOCKS;
    const dim3 grid((unsigned)xb, (unsigned)C);
    k_lv_flags<<<grid, 256, 0, st>>>(w.vb, target, n, C, ignore_label, has_ignore, w.flag);
    if (lidog_exclusive_scan(w.flag, L, w.sums, st)) return 1;
    k_lv_grad<<<grid, 256, 0, st>>>(w.vb, w.flag, err, n, C, coef, w.partial);
    k_lv_finish<<<1, 256, 0, st>>>(w.partial, (int)xb * C, w.flag, n, C, loss, coef + N);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_lovasz_bwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                                int32_t has_ignore, const float *coef, const float *invP, const float *gout,
                                float *glogits, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(lv_shape_ok(n, C), "lovasz: n >= 0, C in [2, 20] and n C < 2^31, got n = %lld, C = %d", (long long)n, C);
    if (n == 0) return 0;
    int64_t nb = cdiv64(n, 256);
    if (nb > 4096) nb = 4096;
#define CALL(C_) \
    k_lv_bwd<C_><<<(unsigned)nb, 256, 0, st>>>(logits, target, n, ignore_label, has_ignore, coef, invP, gout, glogits)
    DICE_DISPATCH(CALL)
#undef CALL
    LIDOG_LAUNCH_CHECK();
    return 0;
}
