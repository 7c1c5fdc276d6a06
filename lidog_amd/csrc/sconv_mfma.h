// launchers of csrc/sconv_mfma.hip (internal to the library)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bn_math.h"

// BatchNorm (+ ReLU) of the layer that produced the gathered rows, applied while they are staged: the consumer reads the
// producer's raw convolution output and never needs the normalised copy (the staged values are the bits lidog_bn_apply
// would have written).  mean == NULL: rows taken as they are.
struct InBn {
    const float *mean, *invstd, *w, *b;
    int relu;
};

__device__ __forceinline__ float4 in_bn_apply(float4 v, const float4 &m, const float4 &s, const float4 &w, const float4 &b,
                                              int relu) {
    v = bn_affine4(v, m, s, w, b);
    const float lo = relu ? 0.f : -__builtin_inff();   // one max either way: no branch in the staging loop
    v.x = fmaxf(v.x, lo); v.y = fmaxf(v.y, lo); v.z = fmaxf(v.z, lo); v.w = fmaxf(v.w, lo);
    return v;
}

int lidog_launch_gemm_mfma(const float *A, const int32_t *gather, const float *B, const float *bias,
                           const int32_t *tile_k, const int32_t *tile_row0, const int32_t *tile_rows, int n_tiles,
                           int Cin, int Cout, float *T, const int32_t *scatter, InBn in_bn, int64_t a_rows, hipStream_t st);
void lidog_gemm_multi_suspend(int delta);
int lidog_launch_wgrad_mfma(const float *A, const int32_t *pa, const float *G, const int32_t *pg,
                            const int32_t *items, int n_items, int Cin, int Cout, float *partial, InBn in_bn,
                            hipStream_t st);
int lidog_wgrad_mfma_slabs(int Cin, int Cout, int n_items);
int lidog_wgrad_mfma_wg_per_cu(int Cin, int Cout, int fold);
// csrc/sconv.hip: the fixed-order sum of a weight gradient's partial slots (`per` per work item) into gW [K][n]
void lidog_launch_items_sum(const float *partial, const int32_t *item_off, int per, int K, int64_t n, float *gW,
                            hipStream_t st);
