// The first mile of a scan read from a file (utils/datasets/semantickitti.py:100-131,190-213, nuscenes.py:144-178,
// 238-266, synth4d.py:106-137,203-220), which the reference runs with numpy in DataLoader workers: unpack the point
// records, mask the raw labels and map them through the learning-map LUT, apply the radius mask, compact the kept rows
// in order, and count the per-class label statistics.  The host uploads the files' bytes unmodified.  The kept rows take
// their positions from lidog_compact_rows (prims.hip: per-block counts, one scan, in-wave ballot ranks), never from an
// atomic; the statistics are integer counts (LDS bins, one global integer add per non-empty bin and block): the same
// bytes on every run.
#include "common.h"
#include "prims.h"
#include "scan_ops.h"

#define SCAN_THREADS 256
#define SCAN_MAX_BLOCKS 1024
#define SCAN_MAX_CLASSES 256

// mapped[i] = the mapped label of row i; keep[i] = 1 for a kept row, 0 otherwise (use_radius: the flags of
// lidog_compact_rows); counts[c] += rows of the file with mapped label c; info[1] += label errors
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_flag(const float *__restrict__ pts, int32_t stride, int32_t vec4,
                                                            const void *__restrict__ labels_raw, int32_t kind,
                                                            int32_t mask, int64_t n, const int32_t *__restrict__ lut,
                                                            int32_t L, int32_t use_radius, float r2,
                                                            int32_t *__restrict__ mapped, int32_t *__restrict__ keep,
                                                            unsigned long long *__restrict__ counts, int32_t C,
                                                            int32_t *info) {
    __shared__ int32_t bins[SCAN_MAX_CLASSES];
    __shared__ int32_t s_bad;
    for (int c = threadIdx.x; c < C; c += SCAN_THREADS) bins[c] = 0;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x * SCAN_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * SCAN_THREADS + threadIdx.x; i < n; i += step) {
        bool bad = false;
        const int32_t l = scan_map_label(labels_raw, kind, mask, i, lut, L, &bad);
        if (bad) atomicAdd(&s_bad, 1);                       // a count
        if (counts && !bad && l >= 0 && l < C) atomicAdd(&bins[l], 1);
        if (mapped) mapped[i] = l;
        if (keep) {
            float x, y, z;
            scan_xyz(pts, stride, vec4 != 0, i, &x, &y, &z);
            keep[i] = scan_in_radius(x, y, z, r2) ? 1 : 0;
        }
    }
    __syncthreads();
    if (counts)
        for (int c = threadIdx.x; c < C; c += SCAN_THREADS)
            if (bins[c]) atomicAdd(&counts[c], (unsigned long long)bins[c]);
    if (threadIdx.x == 0 && s_bad) atomicAdd(&info[1], s_bad);
}

// output row r: file row kept[r] (kept == NULL: r itself), r < count (count_dev == NULL: n).  info[0] = kept rows,
// info[2] += kept rows with a non-finite coordinate (possible only without a radius mask)
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_emit(const float *__restrict__ pts, int32_t stride, int32_t vec4,
                                                            int64_t n, const int32_t *__restrict__ mapped,
                                                            const int32_t *__restrict__ kept,
                                                            const int32_t *__restrict__ count_dev,
                                                            float *__restrict__ points_out,
                                                            int32_t *__restrict__ labels_out, int32_t *info) {
    const int64_t count = count_dev ? (int64_t)*count_dev : n;
    if (blockIdx.x == 0 && threadIdx.x == 0) info[0] = (int32_t)count;
    const int64_t step = (int64_t)gridDim.x * SCAN_THREADS;
    int32_t odd = 0;
    for (int64_t r = (int64_t)blockIdx.x * SCAN_THREADS + threadIdx.x; r < count && r < n; r += step) {
        const int64_t i = kept ? (int64_t)kept[r] : r;
        if (i < 0 || i >= n) continue;                       // never read outside the file
        float x, y, z;
        scan_xyz(pts, stride, vec4 != 0, i, &x, &y, &z);
        float *o = points_out + 3 * r;
        o[0] = x; o[1] = y; o[2] = z;
        labels_out[r] = mapped[i];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) ++odd;
    }
    if (odd) atomicAdd(&info[2], odd);                       // a count
}

extern "C" int64_t lidog_scan_load_ws(int64_t n) {
    const int64_t nn = n > 0 ? n : 0;   // mapped, keep, kept [n], a spare word (ABI 9 fixes the size), the compaction's
    return 3 * nn + 1 + lidog_compact_ws_ints(nn);
}

extern "C" int lidog_scan_load(const float *points_raw, int32_t point_stride, const void *labels_raw, int32_t label_kind,
                               int32_t label_mask, int64_t n, const int32_t *lut, int32_t lut_len, int32_t use_radius,
                               float radius_sq, float *points_out, int32_t *labels_out, int64_t *counts,
                               int32_t num_classes, int32_t *info, int32_t *ws, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX, "lidog_scan_load: n = %lld out of range", (long long)n);
    LIDOG_REQUIRE(label_kind == SCAN_LABELS_NONE || label_kind == SCAN_LABELS_I32 || label_kind == SCAN_LABELS_U8,
                  "lidog_scan_load: label_kind = %d (0 none, 1 int32, 2 uint8)", label_kind);
    LIDOG_REQUIRE(label_kind == SCAN_LABELS_NONE || n == 0 || (labels_raw && lut && lut_len > 0),
                  "lidog_scan_load: labels without their array or their look-up table");
    LIDOG_REQUIRE(!points_raw || point_stride >= 3, "lidog_scan_load: point_stride = %d (at least 3)", point_stride);
    LIDOG_REQUIRE(!counts || (num_classes >= 1 && num_classes <= SCAN_MAX_CLASSES),
                  "lidog_scan_load: %d classes (1..%d)", num_classes, SCAN_MAX_CLASSES);
    LIDOG_REQUIRE(info, "lidog_scan_load: info is required");
    LIDOG_REQUIRE(!points_raw || n == 0 || (points_out && labels_out && ws),
                  "lidog_scan_load: an output array or the workspace is missing");
    LIDOG_REQUIRE(points_raw || !use_radius || n == 0, "lidog_scan_load: a radius mask without points");
    LIDOG_CHECK_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int32_t), st));
    if (n == 0) return 0;
    const int64_t blocks = cdiv64(n, SCAN_THREADS);
    const unsigned grid = (unsigned)(blocks < SCAN_MAX_BLOCKS ? blocks : SCAN_MAX_BLOCKS);
    const int32_t vec4 = (points_raw && point_stride == 4 && ((uintptr_t)points_raw & 15) == 0) ? 1 : 0;
    if (!points_raw) {                  // the labels alone: get_dataset_stats
        if (!counts && label_kind == SCAN_LABELS_NONE) return 0;
        k_scan_flag<<<grid, SCAN_THREADS, 0, st>>>(nullptr, 0, 0, labels_raw, label_kind, label_mask, n, lut, lut_len,
                                                   0, 0.0f, nullptr, nullptr, (unsigned long long *)counts,
                                                   counts ? num_classes : 0, info);
        LIDOG_LAUNCH_CHECK();
        return 0;
    }
    int32_t *mapped = ws, *keep = ws + n, *kept_w = ws + 2 * n, *compact_ws = ws + 3 * n + 1;
    k_scan_flag<<<grid, SCAN_THREADS, 0, st>>>(points_raw, point_stride, vec4, labels_raw, label_kind, label_mask, n,
                                               lut, lut_len, use_radius, radius_sq, mapped,
                                               use_radius ? keep : nullptr,
                                               (unsigned long long *)counts, counts ? num_classes : 0, info);
    LIDOG_LAUNCH_CHECK();
    const int32_t *kept = nullptr, *count = nullptr;
    if (use_radius) {
        if (lidog_compact_rows(keep, n, kept_w, compact_ws, &count, st)) return 1;
        kept = kept_w;
    }
    k_scan_emit<<<grid, SCAN_THREADS, 0, st>>>(points_raw, point_stride, vec4, n, mapped, kept, count, points_out,
                                               labels_out, info);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
