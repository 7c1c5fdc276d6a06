// Test-time augmentation at the point level: the scores of one view of a loader batch, gathered per kept point and
// accumulated into acc [k, C].
//   lidog_tta_vote   acc[p] (=|+=) s(logits[inverse[p]]), s = softmax (mode 0), the logits themselves (mode 1) or the
//                    one-hot of the row's ev_argmax (mode 2)
// One block owns TTA_ROWS consecutive rows of acc and one thread computes one row's scores: no atomics on acc, and the
// views arrive as separate launches in view order, so the fp32 sum of a row has one fixed order.  inverse[p] is checked
// before any address is formed from it; a point whose entry lies outside [0, m) sets bit 0 of the error word and its acc
// row is neither read nor written.
//
// Rows are C floats (28 bytes at C = 7).  A thread that walks its own row makes every wave instruction touch 64 rows;
// measured that way the kernel ran at half the speed of the torch composition.  So global memory is
// walked by ELEMENT: the block's acc rows are one contiguous range, read and written with consecutive lanes on
// consecutive floats, and the gathered logits rows are fetched with C consecutive lanes on one row.  The rows meet their
// owning threads in LDS, at an odd row stride (no bank conflicts in the per-row walks).
#include "common.h"
#include "row_argmax.h"

#define TTA_THREADS 256
#define TTA_ROWS TTA_THREADS                // acc rows of a block
#define TTA_MAX_CLASSES 32                  // lidog_point_labels' limit: its logits are this kernel's acc
#define TTA_MODE_PROB 0
#define TTA_MODE_LOGIT 1
#define TTA_MODE_VOTE 2
#define TTA_ERR_INVERSE 1

// prob: the row maximum is torch's (a NaN wins), x - max in fp32, accurate expf, the sum in class order, one IEEE
// division per class.  A NaN or +inf logit makes the whole row NaN, as torch.softmax does.
__device__ __forceinline__ void tta_softmax_row(float *x, int C) {
    float mx = x[0];
    for (int c = 1; c < C; ++c) {
        const float v = x[c];
        if (v > mx || v != v) mx = v;
    }
    float sum = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float e = expf(x[c] - mx);
        x[c] = e;
        sum = c == 0 ? e : sum + e;
    }
    for (int c = 0; c < C; ++c) x[c] = x[c] / sum;
}

// dynamic LDS: TTA_ROWS rows of (C | 1) floats (not used by mode 1)
__global__ __launch_bounds__(TTA_THREADS) void k_tta_vote(const float *__restrict__ logits, int64_t m, int32_t C,
                                                          const int64_t *__restrict__ inverse, int64_t k, int32_t mode,
                                                          int32_t first, float *__restrict__ acc,
                                                          int32_t *__restrict__ err) {
    extern __shared__ __align__(16) float s_x[];
    __shared__ int64_t s_r[TTA_ROWS];                   // the logits row of every acc row of the block, -1: none
    const int CS = C | 1;
    const int64_t p0 = (int64_t)blockIdx.x * TTA_ROWS;
    const int rows = (int)(k - p0 < (int64_t)TTA_ROWS ? k - p0 : (int64_t)TTA_ROWS);
    const int tid = threadIdx.x;
    int bad = 0;
    if (tid < rows) {
        int64_t r = inverse[p0 + tid];
        if (r < 0 || r >= m) {
            bad = 1;
            r = -1;
        }
        s_r[tid] = r;
    }
    if (__syncthreads_or(bad) && tid == 0) atomicOr(err, TTA_ERR_INVERSE);
    const unsigned n_el = (unsigned)(rows * C);          // <= 8192
    float *__restrict__ a = acc + p0 * C;
    if (mode == TTA_MODE_LOGIT) {
        for (unsigned e = tid; e < n_el; e += TTA_THREADS) {
            const unsigned p = e / (unsigned)C, c = e - p * (unsigned)C;
            const int64_t r = s_r[p];
            if (r >= 0) {
                const float x = logits[r * C + c];
                a[e] = first ? x : a[e] + x;
            }
        }
        return;
    }
    for (unsigned e = tid; e < n_el; e += TTA_THREADS) {
        const unsigned p = e / (unsigned)C, c = e - p * (unsigned)C;
        const int64_t r = s_r[p];
        if (r >= 0) s_x[p * CS + c] = logits[r * C + c];
    }
    __syncthreads();
    if (tid < rows && s_r[tid] >= 0) {
        float *x = s_x + tid * CS;
        if (mode == TTA_MODE_PROB) {
            tta_softmax_row(x, C);
        } else {
            const int top = ev_argmax(x, C);
            for (int c = 0; c < C; ++c) x[c] = c == top ? 1.0f : 0.0f;
        }
    }
    __syncthreads();
    for (unsigned e = tid; e < n_el; e += TTA_THREADS) {
        const unsigned p = e / (unsigned)C, c = e - p * (unsigned)C;
        if (s_r[p] >= 0) {
            const float s = s_x[p * CS + c];
            a[e] = first ? s : a[e] + s;
        }
    }
}

extern "C" int lidog_tta_vote(const float *logits, int64_t m, int32_t n_classes, const int64_t *inverse, int64_t k,
                              int32_t mode, int32_t first, float *acc, int32_t *err, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(k >= 0 && m >= 0, "lidog_tta_vote: %lld points, %lld rows", (long long)k, (long long)m);
    LIDOG_REQUIRE(n_classes >= 1 && n_classes <= TTA_MAX_CLASSES, "lidog_tta_vote: %d classes (1..%d)", n_classes,
                  TTA_MAX_CLASSES);
    LIDOG_REQUIRE(mode == TTA_MODE_PROB || mode == TTA_MODE_LOGIT || mode == TTA_MODE_VOTE,
                  "lidog_tta_vote: mode = %d (0 prob, 1 logit, 2 vote)", mode);
    if (k == 0) return 0;
    LIDOG_REQUIRE(inverse && acc && err && (m == 0 || logits), "lidog_tta_vote: null argument");
    const int64_t blocks = cdiv64(k, TTA_ROWS);
    LIDOG_REQUIRE(blocks < (int64_t)INT32_MAX, "lidog_tta_vote: grid too large");
    const size_t lds = mode == TTA_MODE_LOGIT ? 0 : sizeof(float) * TTA_ROWS * (size_t)(n_classes | 1);   // <= 33 KiB
    k_tta_vote<<<(unsigned)blocks, TTA_THREADS, lds, st>>>(logits, m, n_classes, inverse, k, mode, first, acc, err);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
