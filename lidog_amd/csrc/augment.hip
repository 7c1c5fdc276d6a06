// The per-point part of one augmented training item (sub_p / augmentation_list of the reference's training datasets):
// the sub-sample gather (random_sample, utils/datasets/dataset.py:58-72), RandomRotation / RandomScale
// (utils/common/augmentation.py:7-44) with numpy's dtype rules, the bounds filter with the ego box
// (utils/datasets/semantickitti_bev.py:155-172), the voxel floor of ME.utils.sparse_quantize in the point's own dtype,
// and the stable compaction of the kept rows.  The host makes the draws; the rotation matrix and the scales travel by
// value in the launch arguments.  The kept rows take their positions from lidog_compact_rows (prims.hip: per-block counts,
// one scan, in-wave ballot ranks), never from an atomic: the same rows in the same order on every run.
#include "aug_ops.h"
#include "prims.h"

#define AUG_THREADS 256

// filter_bounds: strict comparisons on the value in its own dtype (a float32 widens exactly)
__device__ __forceinline__ bool aug_in_bounds(const AugPoint &a) {
    const double x = a.is64 ? a.d[0] : (double)a.f[0];
    const double y = a.is64 ? a.d[1] : (double)a.f[1];
    const double z = a.is64 ? a.d[2] : (double)a.f[2];
    const bool in = (-60.0 < x) & (x < 60.0) & (-60.0 < y) & (y < 60.0) & (-10.0 < z) & (z < 8.0);
    const bool ego = (-3.0 < x) & (x < 3.0) & (-2.0 < y) & (y < 2.0);
    return in & !ego;
}

__device__ __forceinline__ int64_t aug_source_row(const int32_t *__restrict__ sampled_idx, int64_t j, int64_t n,
                                                  int32_t *info) {
    int64_t i = sampled_idx ? (int64_t)sampled_idx[j] : j;
    if (i < 0 || i >= n) {   // never read outside the scan: the row is clamped and the caller told
        info[1] = 1;
        i = i < 0 ? 0 : n - 1;
    }
    return i;
}

// keep[j] = 1 for a sampled row inside the bounds, 0 otherwise: the flags of lidog_compact_rows
__global__ __launch_bounds__(AUG_THREADS) void k_aug_flag(const float *__restrict__ pts, int64_t n,
                                                          const int32_t *__restrict__ sampled_idx, int64_t k, AugOps ops,
                                                          int32_t *__restrict__ keep, int32_t *info) {
    const int64_t j = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x;
    if (j >= k) return;
    const int64_t i = aug_source_row(sampled_idx, j, n, info);
    keep[j] = aug_in_bounds(aug_transform(pts, i, ops)) ? 1 : 0;
}

// output row r: sampled row kept[r] (kept == NULL: r itself), r < count (count_dev == NULL: k).  The transform is
// computed again rather than stored: 30 flops against 24 bytes of traffic each way.
__global__ __launch_bounds__(AUG_THREADS) void k_aug_emit(const float *__restrict__ pts, int64_t n,
                                                          const int32_t *__restrict__ sampled_idx, int64_t k, AugOps ops,
                                                          const int32_t *__restrict__ kept,
                                                          const int32_t *__restrict__ count_dev, double qx, double qy,
                                                          double qz, int32_t batch, const int32_t *__restrict__ labels,
                                                          int4 *__restrict__ rows, void *__restrict__ xyz,
                                                          int32_t *__restrict__ src, int32_t *__restrict__ labels_out,
                                                          int32_t *info) {
    const int64_t r = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x;
    const int64_t count = count_dev ? (int64_t)*count_dev : k;
    if (r == 0) info[0] = (int32_t)count;
    if (r >= count || r >= k) return;
    const int64_t j = kept ? (int64_t)kept[r] : r;
    if (j < 0 || j >= k) {
        info[1] = 1;
        return;
    }
    const int64_t i = aug_source_row(sampled_idx, j, n, info);
    const AugPoint a = aug_transform(pts, i, ops);
    rows[r] = aug_voxel_row(a, batch, qx, qy, qz);   // the floor in the point's own dtype
    if (a.is64) {
        double *o = (double *)xyz + 3 * r;
        o[0] = a.d[0]; o[1] = a.d[1]; o[2] = a.d[2];
    } else {
        float *o = (float *)xyz + 3 * r;
        o[0] = a.f[0]; o[1] = a.f[1]; o[2] = a.f[2];
    }
    src[r] = (int32_t)i;
    if (labels) labels_out[r] = labels[i];
}

extern "C" int32_t lidog_augment_is_f64(const int32_t *op_kinds_host, int32_t n_ops) {
    for (int o = 0; o < n_ops; ++o)
        if (op_kinds_host[o] == AUG_ROTATION) return 1;
    return 0;
}

extern "C" int64_t lidog_augment_ws(int64_t k) {
    const int64_t kk = k > 0 ? k : 0;   // keep [k], kept [k], a spare word (ABI 9 fixes the size), the compaction's own
    return 2 * kk + 1 + lidog_compact_ws_ints(kk);
}

extern "C" int lidog_augment_points(const float *points, int64_t n, const int32_t *sampled_idx, int64_t k,
                                    const int32_t *op_kinds_host, const double *op_params_host, int32_t n_ops,
                                    int32_t use_bounds, double qx, double qy, double qz, int32_t batch,
                                    const int32_t *labels, int32_t *rows, void *xyz, int32_t *src, int32_t *labels_out,
                                    int32_t *info, int32_t *ws, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0 && k >= 0 && k < (int64_t)INT32_MAX && n < (int64_t)INT32_MAX,
                  "lidog_augment_points: n = %lld, k = %lld out of range", (long long)n, (long long)k);
    LIDOG_REQUIRE(sampled_idx || k == n || k == 0,
                  "lidog_augment_points: without sampled_idx every row is taken (k = n)");
    LIDOG_REQUIRE(n_ops >= 0 && n_ops <= AUG_MAX_OPS, "lidog_augment_points: %d operations (at most %d)", n_ops,
                  AUG_MAX_OPS);
    LIDOG_REQUIRE(n_ops == 0 || (op_kinds_host && op_params_host), "lidog_augment_points: operations missing");
    LIDOG_REQUIRE(qx > 0 && qy > 0 && qz > 0, "lidog_augment_points: voxel size must be positive");
    LIDOG_REQUIRE(info, "lidog_augment_points: info is required");
    LIDOG_REQUIRE(k == 0 || (n > 0 && points && rows && xyz && src && (!labels || labels_out)),
                  "lidog_augment_points: an input or output array is missing");
    LIDOG_REQUIRE(!use_bounds || k == 0 || ws, "lidog_augment_points: the bounds filter needs the workspace");
    AugOps ops = {};
    ops.n = n_ops;
    for (int o = 0; o < n_ops; ++o) {
        LIDOG_REQUIRE(op_kinds_host[o] == AUG_ROTATION || op_kinds_host[o] == AUG_SCALE,
                      "lidog_augment_points: operation %d of kind %d (0 rotation, 1 scale)", o, op_kinds_host[o]);
        ops.kind[o] = op_kinds_host[o];
        for (int q = 0; q < 9; ++q) ops.p[o][q] = op_params_host[9 * o + q];
    }
    LIDOG_CHECK_HIP(hipMemsetAsync(info, 0, 2 * sizeof(int32_t), st));
    if (k == 0) return 0;
    const unsigned grid = (unsigned)cdiv64(k, AUG_THREADS);
    const int32_t *kept = nullptr, *count = nullptr;
    if (use_bounds) {
        int32_t *keep = ws, *kept_w = ws + k, *compact_ws = ws + 2 * k + 1;
        k_aug_flag<<<grid, AUG_THREADS, 0, st>>>(points, n, sampled_idx, k, ops, keep, info);
        LIDOG_LAUNCH_CHECK();
        if (lidog_compact_rows(keep, k, kept_w, compact_ws, &count, st)) return 1;
        kept = kept_w;
    }
    k_aug_emit<<<grid, AUG_THREADS, 0, st>>>(points, n, sampled_idx, k, ops, kept, count, qx, qy, qz, batch, labels,
                                             (int4 *)rows, xyz, src, labels_out, info);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
