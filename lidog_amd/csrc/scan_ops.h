// The per-row operations of a scan file shared by the loader (scanload.hip) and the point-label path (pointlabels.hip):
// the raw label's look-up, the radius test and the record's coordinates.  One definition, so that a row kept by one is a
// row kept by the other, bit for bit.
#pragma once
#include <stdint.h>

#define SCAN_LABELS_NONE 0
#define SCAN_LABELS_I32 1
#define SCAN_LABELS_U8 2

// numpy's `lut[idx]`: 0 <= idx < L as is, -L <= idx < 0 wraps, anything else is an IndexError (*bad)
__device__ __forceinline__ int32_t scan_map_label(const void *__restrict__ labels_raw, int32_t kind, int32_t mask,
                                                  int64_t i, const int32_t *__restrict__ lut, int32_t L, bool *bad) {
    if (kind == SCAN_LABELS_NONE) return 0;      // a scan without a label file: zeros, unmapped (synth4d.py:115-116)
    int64_t idx = kind == SCAN_LABELS_I32 ? (int64_t)(((const int32_t *)labels_raw)[i] & mask)
                                          : (int64_t)((const uint8_t *)labels_raw)[i];
    if (idx < 0) idx += L;
    if (idx < 0 || idx >= L) {
        *bad = true;
        return -1;
    }
    return lut[idx];
}

// `np.sum(np.square(points), axis=1) < in_R ** 2` on a float32 [n, 3] view: every product and every sum rounded to
// float32 on its own, (x x + y y) + z z, a strict comparison; a NaN fails it.  The operations are written out under
// `fp contract(off)`, so no product is fused into a sum whatever -ffp-contract the file is built with (the library's
// build passes `off` as well).  HIP's __fmul_rn / __fadd_rn would not do: they are plain `*` and `+` inside header
// functions, outside the reach of a pragma here, and fuse under the compiler's default.
__device__ __forceinline__ bool scan_in_radius(float x, float y, float z, float r2) {
#pragma clang fp contract(off)
    const float xx = x * x, yy = y * y, zz = z * z;
    const float xy = xx + yy;
    return xy + zz < r2;
}

__device__ __forceinline__ void scan_xyz(const float *__restrict__ pts, int32_t stride, bool vec4, int64_t i, float *x,
                                         float *y, float *z) {
    if (vec4) {      // stride 4 on a 16-byte aligned buffer: one 16-byte load per lane
        const float4 p = ((const float4 *)pts)[i];
        *x = p.x; *y = p.y; *z = p.z;
    } else {
        const float *p = pts + (int64_t)stride * i;
        *x = p[0]; *y = p[1]; *z = p[2];
    }
}
