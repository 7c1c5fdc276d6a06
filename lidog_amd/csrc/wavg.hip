// Weight averaging along the training trajectory (lidog_amd/optim.py:WeightAverage): ONE streaming launch over every
// (live, average, n) segment of a model -- the optimiser's flat parameter buffer plus each floating-point buffer (the
// BatchNorm running statistics).  With p the live element and a the average:
//   COPY  a = p                      the first update of either mode
//   EMA   a = c0 * a + c1 * p        MomentumUpdater of the reference (utils/common/momentum.py), c0 = tau, c1 = 1 - tau
//   SWA   a = a + (p - a) / c0       torch.optim.swa_utils.AveragedModel's default, c0 = updates so far + 1
//   SWAP  exchange a and p           WeightAverage.applied(): the model computes with the average, in place
// Every operation is rounded on its own (the build sets -ffp-contract=off) and the division is IEEE-correct (hipcc's
// default for HIP), so a numpy float32 restatement of the same expression gives the same bits (tests/wavg_ref.py).
//
// The table lives in DEVICE memory and is laid out once by the host: table[3 s .. 3 s + 2] = segment s, then
// block0[0 .. n_segs] = first workgroup of every segment, block0[n_segs] = grid.  A workgroup finds its segment by a
// binary search of block0 (the index is uniform: scalar loads) and walks it as k_grad_accumulate walks one (optim.hip):
// a scalar head up to the first 16-byte boundary, a float4 body, a scalar tail; a segment whose two pointers are aligned
// differently takes the scalar loop throughout.  No atomics, nothing read back.
#include "common.h"

namespace {
template <int MODE>
__device__ __forceinline__ void wavg_one(float &p, float &a, float c0, float c1) {
    if (MODE == LIDOG_WAVG_COPY) {
        a = p;
    } else if (MODE == LIDOG_WAVG_EMA) {
        a = c0 * a + c1 * p;
    } else if (MODE == LIDOG_WAVG_SWA) {
        a = a + (p - a) / c0;
    } else {
        const float t = a;
        a = p;
        p = t;
    }
}

// one element at index i: only what the mode needs is read and written
template <int MODE>
__device__ __forceinline__ void wavg_scalar(float *__restrict__ live, float *__restrict__ avg, int64_t i, float c0,
                                            float c1) {
    float p = live[i], a = MODE == LIDOG_WAVG_COPY ? 0.f : avg[i];
    wavg_one<MODE>(p, a, c0, c1);
    avg[i] = a;
    if (MODE == LIDOG_WAVG_SWAP) live[i] = p;
}
}  // namespace

template <int MODE>
__global__ __launch_bounds__(256) void k_wavg(const int64_t *__restrict__ table, int n_segs, float c0, float c1) {
    const int64_t *__restrict__ block0 = table + 3 * (int64_t)n_segs;
    const int64_t b = blockIdx.x;
    if (b >= block0[n_segs]) return;
    int lo = 0, hi = n_segs;                 // the last s with block0[s] <= b (segments of no workgroups are skipped)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (block0[mid] <= b) lo = mid; else hi = mid;
    }
    const int s = lo;
    float *__restrict__ live = (float *)(uintptr_t)table[3 * s];
    float *__restrict__ avg = (float *)(uintptr_t)table[3 * s + 1];
    const int64_t n = table[3 * s + 2];
    const int64_t t = (b - block0[s]) * 256 + threadIdx.x;
    const int64_t stride = (block0[s + 1] - block0[s]) * 256;
    if ((((uintptr_t)live ^ (uintptr_t)avg) & 15) != 0) {
        for (int64_t i = t; i < n; i += stride) wavg_scalar<MODE>(live, avg, i, c0, c1);
        return;
    }
    int64_t head = (int64_t)(((16 - ((uintptr_t)avg & 15)) & 15) >> 2);
    if (head > n) head = n;
    const int64_t body = (n - head) >> 2, tail0 = head + 4 * body;
    if (t < head) wavg_scalar<MODE>(live, avg, t, c0, c1);
    float4 *__restrict__ p4 = (float4 *)(live + head);
    float4 *__restrict__ a4 = (float4 *)(avg + head);
    for (int64_t i = t; i < body; i += stride) {
        float4 p = p4[i], a;
        if (MODE == LIDOG_WAVG_COPY) a = p; else a = a4[i];
        wavg_one<MODE>(p.x, a.x, c0, c1);
        wavg_one<MODE>(p.y, a.y, c0, c1);
        wavg_one<MODE>(p.z, a.z, c0, c1);
        wavg_one<MODE>(p.w, a.w, c0, c1);
        a4[i] = a;
        if (MODE == LIDOG_WAVG_SWAP) p4[i] = p;
    }
    if (t < n - tail0) wavg_scalar<MODE>(live, avg, tail0 + t, c0, c1);
}

extern "C" int lidog_wavg_apply(const int64_t *table, int32_t n_segs, int64_t n_blocks, int32_t mode, float c0,
                                float c1, void *stream) {
    LIDOG_REQUIRE(n_segs >= 0 && n_blocks >= 0, "wavg_apply: negative segment or workgroup count");
    LIDOG_REQUIRE(mode >= LIDOG_WAVG_COPY && mode <= LIDOG_WAVG_SWAP, "wavg_apply: unknown mode %d", mode);
    if (n_segs == 0 || n_blocks == 0) return 0;
    LIDOG_REQUIRE(table != nullptr, "wavg_apply: no table");
    LIDOG_REQUIRE(n_blocks <= 0x7fffffff, "wavg_apply: %lld workgroups", (long long)n_blocks);
    LIDOG_REQUIRE(mode != LIDOG_WAVG_SWA || c0 != 0.f, "wavg_apply: the SWA divisor is 0");
    const dim3 grid((unsigned)n_blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (mode) {
    case LIDOG_WAVG_COPY: k_wavg<LIDOG_WAVG_COPY><<<grid, block, 0, st>>>(table, n_segs, c0, c1); break;
    case LIDOG_WAVG_EMA: k_wavg<LIDOG_WAVG_EMA><<<grid, block, 0, st>>>(table, n_segs, c0, c1); break;
    case LIDOG_WAVG_SWA: k_wavg<LIDOG_WAVG_SWA><<<grid, block, 0, st>>>(table, n_segs, c0, c1); break;
    default: k_wavg<LIDOG_WAVG_SWAP><<<grid, block, 0, st>>>(table, n_segs, c0, c1); break;
    }
    LIDOG_LAUNCH_CHECK();
    return 0;
}
