// RandomRotation / RandomScale (utils/common/augmentation.py:7-44) on one point under numpy's dtype rules, and the voxel
// floor of ME.utils.sparse_quantize in the point's own dtype.  Shared by augment.hip (the items of a training dataset)
// and mix.hip (CoSMix's transform of every pasted class, cosmix.py:135-136).
#pragma once
#include "common.h"

#define AUG_MAX_OPS 4
#define AUG_ROTATION 0
#define AUG_SCALE 1

struct AugOps {
    int32_t n;
    int32_t kind[AUG_MAX_OPS];
    double p[AUG_MAX_OPS][9];   // rotation: R row-major (out_j = sum_k p_k R[k][j]); scale: s_x, s_y, s_z
};

struct AugPoint {
    double d[3];   // the point once it is float64
    float f[3];    // the point while it is float32
    bool is64;
};

// numpy's arithmetic on one row (x, y, z float32; op o has kind[o] and the parameters params[9 o ..]).  `coords @ R` with
// a float64 R: the float32 row is widened (exactly) and every output is (p0 R0j + p1 R1j) + p2 R2j in float64.
// `coords[:, k] = coords[:, k] * s_k` with a float64 s_k: one float64 product, which the in-place assignment rounds back
// to float32 while the array still is float32.
__device__ __forceinline__ AugPoint aug_transform_point(float x0, float x1, float x2, int32_t n_ops,
                                                        const int32_t *__restrict__ kind,
                                                        const double *__restrict__ params) {
    AugPoint a;
    a.is64 = false;
    a.f[0] = x0; a.f[1] = x1; a.f[2] = x2;
#pragma unroll
    for (int k = 0; k < 3; ++k) a.d[k] = 0.0;
    for (int o = 0; o < n_ops; ++o) {
        const double *p = params + 9 * o;
        if (kind[o] == AUG_ROTATION) {
            double x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = a.is64 ? a.d[k] : (double)a.f[k];
#pragma unroll
            for (int j = 0; j < 3; ++j) a.d[j] = (x[0] * p[j] + x[1] * p[3 + j]) + x[2] * p[6 + j];
            a.is64 = true;
        } else if (a.is64) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a.d[k] = a.d[k] * p[k];
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) a.f[k] = (float)((double)a.f[k] * p[k]);
        }
    }
    return a;
}

__device__ __forceinline__ AugPoint aug_transform(const float *__restrict__ pts, int64_t i, const AugOps &ops) {
    return aug_transform_point(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], ops.n, ops.kind, &ops.p[0][0]);
}

// (batch, floor(p / q)): np.floor(c / q) on a float64 array with q = float64(quantization_size); on a float32 array with
// q = float32(quantization_size), as k_voxel_floor
__device__ __forceinline__ int4 aug_voxel_row(const AugPoint &a, int32_t batch, double qx, double qy, double qz) {
    if (a.is64)
        return make_int4(batch, lidog_voxel_coord(floor(a.d[0] / qx)), lidog_voxel_coord(floor(a.d[1] / qy)),
                         lidog_voxel_coord(floor(a.d[2] / qz)));
    return make_int4(batch, lidog_voxel_coord(floorf(a.f[0] / (float)qx)), lidog_voxel_coord(floorf(a.f[1] / (float)qy)),
                     lidog_voxel_coord(floorf(a.f[2] / (float)qz)));
}
