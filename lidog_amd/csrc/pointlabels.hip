// One label per point of a scan file, in file order (what the SemanticKITTI and nuScenes-lidarseg benchmarks score):
//   lidog_scan_keep_rows   the row every record of a file has in lidog_scan_load's compacted output, -1 for a record the
//                          radius mask dropped: the same scan_in_radius, the same lidog_compact_rows, the list inverted
//   lidog_point_labels     a loader batch: the arg-max once per voxel row (ev_argmax, the voxel-level evaluator's rule),
//                          then a walk over the file rows: keep_row -> inverse_map -> voxel prediction -> out_lut; with
//                          the files' raw labels also the per-scan confusion counts over the kept, labelled points
// Counts are integers in LDS bins, added with one 64-bit integer atomic per non-empty bin and block; positions come from
// lidog_compact_rows, never from an atomic: two runs give the same bytes.  Every value read from an input array is
// checked before it is used as an index; what fails sets a bit of the error word and leaves the record at `fill`, uncounted.
#include "common.h"
#include "prims.h"
#include "row_argmax.h"
#include "scan_ops.h"

#define PL_THREADS 256
#define PL_ITERS 4                          // file rows per thread of the label kernel, kept in registers
#define PL_TILE (PL_THREADS * PL_ITERS)
#define PL_MAX_BLOCKS 1024                  // of the keep-index kernels (grid-stride)
#define PL_MAX_CLASSES 32
#define PL_MAX_SCANS 64                     // of a batch: their offsets travel as a kernel argument (1.5 KiB)
#define PL_LDS_BINS 8192                    // int32 bins of a block (32 KiB): C * C per scan of a pass; a block adds at
                                            // most PL_TILE to a bin between two flushes, so 32 bits never overflow
#define PL_ERR_SCAN 1                       // a row outside every scan's range of file rows (the host checks the offsets)
#define PL_ERR_LABEL 2                      // a raw label outside the learning table
#define PL_ERR_INVERSE 4                    // an inverse_map entry outside its scan's voxel rows
#define PL_ERR_KEEP 8                       // a keep_row entry outside its scan's kept rows

// ------------------------------------------------------------------ keep index of a file
// keep[i] = 1 for a kept row, 0 otherwise (the flags of lidog_compact_rows); keep_row[i] = -1
__global__ __launch_bounds__(PL_THREADS) void k_keep_flag(const float *__restrict__ pts, int32_t stride, int32_t vec4,
                                                          int64_t n, float r2, int32_t *__restrict__ keep,
                                                          int32_t *__restrict__ keep_row) {
    const int64_t step = (int64_t)gridDim.x * PL_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; i < n; i += step) {
        float x, y, z;
        scan_xyz(pts, stride, vec4 != 0, i, &x, &y, &z);
        keep[i] = scan_in_radius(x, y, z, r2) ? 1 : 0;
        keep_row[i] = -1;
    }
}

// keep_row[kept[r]] = r for r < count (kept == NULL: every row keeps its own number, count = n); info[0] = count
__global__ __launch_bounds__(PL_THREADS) void k_keep_invert(const int32_t *__restrict__ kept,
                                                            const int32_t *__restrict__ count_dev, int64_t n,
                                                            int32_t *__restrict__ keep_row, int32_t *info) {
    const int64_t count = count_dev ? (int64_t)*count_dev : n;
    if (blockIdx.x == 0 && threadIdx.x == 0) info[0] = (int32_t)count;
    const int64_t step = (int64_t)gridDim.x * PL_THREADS;
    for (int64_t r = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; r < count && r < n; r += step) {
        const int64_t i = kept ? (int64_t)kept[r] : r;
        if (i >= 0 && i < n) keep_row[i] = (int32_t)r;       // never written outside the file
    }
}

extern "C" int64_t lidog_scan_keep_rows_ws(int64_t n) {
    const int64_t nn = n > 0 ? n : 0;   // keep [n], kept [n], a spare word (ABI 9 fixes the size), the compaction's own
    return 2 * nn + 1 + lidog_compact_ws_ints(nn);
}

extern "C" int lidog_scan_keep_rows(const float *points_raw, int32_t point_stride, int64_t n, int32_t use_radius,
                                    float radius_sq, int32_t *keep_row, int32_t *info, int32_t *ws, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX, "lidog_scan_keep_rows: n = %lld out of range", (long long)n);
    LIDOG_REQUIRE(point_stride >= 3, "lidog_scan_keep_rows: point_stride = %d (at least 3)", point_stride);
    LIDOG_REQUIRE(info, "lidog_scan_keep_rows: info is required");
    LIDOG_CHECK_HIP(hipMemsetAsync(info, 0, sizeof(int32_t), st));
    if (n == 0) return 0;
    LIDOG_REQUIRE(keep_row && (!use_radius || (points_raw && ws)),
                  "lidog_scan_keep_rows: the points, the output array or the workspace is missing");
    const int64_t blocks = cdiv64(n, PL_THREADS);
    const unsigned grid = (unsigned)(blocks < PL_MAX_BLOCKS ? blocks : PL_MAX_BLOCKS);
    const int32_t *kept = nullptr, *count = nullptr;
    if (use_radius) {
        const int32_t vec4 = (point_stride == 4 && ((uintptr_t)points_raw & 15) == 0) ? 1 : 0;
        int32_t *keep = ws, *kept_w = ws + n, *compact_ws = ws + 2 * n + 1;
        k_keep_flag<<<grid, PL_THREADS, 0, st>>>(points_raw, point_stride, vec4, n, radius_sq, keep, keep_row);
        LIDOG_LAUNCH_CHECK();
        if (lidog_compact_rows(keep, n, kept_w, compact_ws, &count, st)) return 1;
        kept = kept_w;
    }
    k_keep_invert<<<grid, PL_THREADS, 0, st>>>(kept, count, n, keep_row, info);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ point labels and point confusion of a batch
__global__ __launch_bounds__(PL_THREADS) void k_point_argmax(const float *__restrict__ logits, int64_t n_voxels,
                                                             int32_t C, int32_t *__restrict__ pred) {
    const int64_t r = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x;
    if (r < n_voxels) pred[r] = ev_argmax(logits + r * C, C);
}

struct PointLabelsArgs {
    int64_t row_off[PL_MAX_SCANS + 1], kept_off[PL_MAX_SCANS + 1], vox_off[PL_MAX_SCANS + 1];   // [n_scans + 1] used
    const int32_t *keep_row;                          // [n_rows]: row among its scan's kept rows, -1 dropped
    const int64_t *inverse_map;                       // [n_kept]: voxel row within its scan
    const int32_t *pred;                              // [n_voxels]
    const int32_t *out_lut;                           // [C]
    const void *labels_raw;                           // [n_rows] or NULL
    const int32_t *lut;
    int64_t n_rows, n_kept, n_voxels, ignore_label;
    int32_t n_scans, C, kind, mask, L, slots;
    uint32_t fill;
};

// A block takes PL_TILE consecutive file rows.  The offsets are host values: they arrive with the launch and are staged
// in LDS for the search, so no copy is queued in front of the kernel.  The scan of a row is the last one whose first row
// is not past it (empty scans share their start with the next one and are never chosen).  The bins of the scans [smin, smax] of the
// block's counted rows are covered in passes of `slots` scans, as in k_eval_confusion: bin = (scan - base) * C * C +
// label * C + prediction.
__global__ __launch_bounds__(PL_THREADS) void k_point_labels(PointLabelsArgs a, uint32_t *__restrict__ labels_out,
                                                             unsigned long long *__restrict__ counts,
                                                             int32_t *__restrict__ err) {
    __shared__ int32_t bins[PL_LDS_BINS];
    __shared__ int64_t s_row[PL_MAX_SCANS + 1], s_kept[PL_MAX_SCANS + 1], s_vox[PL_MAX_SCANS + 1];
    __shared__ int32_t s_lo, s_hi, s_err;
    const int B = a.n_scans, C = a.C;
    for (int s = threadIdx.x; s <= B; s += PL_THREADS) {
        s_row[s] = a.row_off[s];
        s_kept[s] = a.kept_off[s];
        s_vox[s] = a.vox_off[s];
    }
    if (threadIdx.x == 0) {
        s_lo = INT32_MAX;
        s_hi = -1;
        s_err = 0;
    }
    __syncthreads();
    const int64_t base_row = (int64_t)blockIdx.x * PL_TILE;
    int32_t scan[PL_ITERS], bin[PL_ITERS];
    int lo = INT32_MAX, hi = -1, e = 0;
#pragma unroll
    for (int it = 0; it < PL_ITERS; ++it) {
        const int64_t r = base_row + it * PL_THREADS + threadIdx.x;
        scan[it] = -1;
        bin[it] = 0;
        if (r < a.n_rows) {
            int s = 0, top = B;
            while (top - s > 1) {
                const int mid = (s + top) >> 1;
                if (s_row[mid] <= r) s = mid;
                else top = mid;
            }
            uint32_t out = a.fill;
            bool bad = false;
            const int32_t l = a.labels_raw ? scan_map_label(a.labels_raw, a.kind, a.mask, r, a.lut, a.L, &bad) : 0;
            if (bad) e |= PL_ERR_LABEL;
            if (r < s_row[s] || r >= s_row[s + 1]) {
                e |= PL_ERR_SCAN;
            } else {
                const int64_t kr = a.keep_row[r];
                if (kr != -1) {
                    const int64_t gk = s_kept[s] + kr;
                    if (kr < 0 || gk >= s_kept[s + 1] || gk < 0 || gk >= a.n_kept) {
                        e |= PL_ERR_KEEP;
                    } else {
                        const int64_t v = a.inverse_map[gk];
                        const int64_t gv = s_vox[s] + v;
                        if (v < 0 || gv >= s_vox[s + 1] || gv < 0 || gv >= a.n_voxels) {
                            e |= PL_ERR_INVERSE;
                        } else if (!bad) {
                            const int32_t p = a.pred[gv];                   // 0 <= p < C: ev_argmax's range
                            out = (uint32_t)a.out_lut[p];
                            if (counts && (int64_t)l != a.ignore_label && l >= 0 && l < C) {
                                scan[it] = s;
                                bin[it] = l * C + p;
                                lo = min(lo, s);
                                hi = max(hi, s);
                            }
                        }
                    }
                }
            }
            labels_out[r] = out;
        }
    }
    if (e) atomicOr(&s_err, e);
    if (hi >= 0) {
        atomicMin(&s_lo, lo);
        atomicMax(&s_hi, hi);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_err) atomicOr(err, s_err);
    const int smin = s_lo, smax = s_hi;      // block-uniform
    const int per_scan = C * C;
    for (int base = smin; base <= smax; base += a.slots) {
        const int ns = min(a.slots, smax - base + 1);
        const int nb = ns * per_scan;
        for (int j = threadIdx.x; j < nb; j += PL_THREADS) bins[j] = 0;
        __syncthreads();
#pragma unroll
        for (int it = 0; it < PL_ITERS; ++it) {
            const int d = scan[it] - base;
            if (scan[it] >= 0 && d >= 0 && d < ns) atomicAdd(&bins[d * per_scan + bin[it]], 1);   // a count
        }
        __syncthreads();
        for (int j = threadIdx.x; j < nb; j += PL_THREADS)
            if (bins[j]) atomicAdd(&counts[(int64_t)base * per_scan + j], (unsigned long long)bins[j]);
        __syncthreads();
    }
}

extern "C" int64_t lidog_point_labels_ws(int64_t n_voxels) { return n_voxels > 0 ? n_voxels : 0; }

extern "C" int lidog_point_labels(const float *logits, int64_t n_voxels, int32_t n_classes, int32_t n_scans,
                                  const int64_t *row_off, const int64_t *kept_off, const int64_t *vox_off,
                                  int64_t n_rows, int64_t n_kept, const int32_t *keep_row, const int64_t *inverse_map,
                                  const int32_t *out_lut, uint32_t fill, const void *labels_raw, int32_t label_kind,
                                  int32_t label_mask, const int32_t *lut, int32_t lut_len, int64_t ignore_label,
                                  uint32_t *labels_out, int64_t *counts, int32_t *err, int32_t *ws, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n_rows >= 0 && n_kept >= 0 && n_voxels >= 0, "lidog_point_labels: rows %lld, kept %lld, voxels %lld",
                  (long long)n_rows, (long long)n_kept, (long long)n_voxels);
    LIDOG_REQUIRE(n_classes >= 1 && n_classes <= PL_MAX_CLASSES, "lidog_point_labels: %d classes (1..%d)", n_classes,
                  PL_MAX_CLASSES);
    LIDOG_REQUIRE(n_scans >= 1 && n_scans <= PL_MAX_SCANS, "lidog_point_labels: %d scans (1..%d)", n_scans,
                  PL_MAX_SCANS);
    LIDOG_REQUIRE(label_kind == SCAN_LABELS_NONE || label_kind == SCAN_LABELS_I32 || label_kind == SCAN_LABELS_U8,
                  "lidog_point_labels: label_kind = %d (0 none, 1 int32, 2 uint8)", label_kind);
    LIDOG_REQUIRE(label_kind == SCAN_LABELS_NONE || n_rows == 0 || (labels_raw && lut && lut_len > 0 && counts),
                  "lidog_point_labels: labels without their array, their look-up table or the counts");
    if (n_rows == 0) return 0;
    LIDOG_REQUIRE(row_off && kept_off && vox_off && keep_row && out_lut && labels_out && err,
                  "lidog_point_labels: null argument");
    LIDOG_REQUIRE((n_kept == 0 || inverse_map) && (n_voxels == 0 || (logits && ws)),
                  "lidog_point_labels: the inverse map, the logits or the workspace is missing");
    PointLabelsArgs a = {};
    for (int s = 0; s <= n_scans; ++s) {
        a.row_off[s] = row_off[s];
        a.kept_off[s] = kept_off[s];
        a.vox_off[s] = vox_off[s];
        LIDOG_REQUIRE(s == 0 ? (row_off[0] == 0 && kept_off[0] == 0 && vox_off[0] == 0)
                             : (row_off[s] >= row_off[s - 1] && kept_off[s] >= kept_off[s - 1] &&
                                vox_off[s] >= vox_off[s - 1]),
                      "lidog_point_labels: the offsets of scan %d do not start at 0 or decrease", s);
    }
    LIDOG_REQUIRE(row_off[n_scans] == n_rows && kept_off[n_scans] == n_kept && vox_off[n_scans] == n_voxels,
                  "lidog_point_labels: the offsets end at %lld rows, %lld kept rows, %lld voxels, not at the sizes given",
                  (long long)row_off[n_scans], (long long)kept_off[n_scans], (long long)vox_off[n_scans]);
    const int64_t blocks = cdiv64(n_rows, PL_TILE), vblocks = cdiv64(n_voxels, PL_THREADS);
    LIDOG_REQUIRE(blocks < (int64_t)INT32_MAX && vblocks < (int64_t)INT32_MAX, "lidog_point_labels: grid too large");
    if (n_voxels > 0) {
        k_point_argmax<<<(unsigned)vblocks, PL_THREADS, 0, st>>>(logits, n_voxels, n_classes, ws);
        LIDOG_LAUNCH_CHECK();
    }
    const bool with_labels = label_kind != SCAN_LABELS_NONE;
    a.keep_row = keep_row; a.inverse_map = inverse_map; a.pred = ws; a.out_lut = out_lut;
    a.labels_raw = with_labels ? labels_raw : nullptr;
    a.lut = lut;
    a.n_rows = n_rows; a.n_kept = n_kept; a.n_voxels = n_voxels; a.ignore_label = ignore_label;
    a.n_scans = n_scans; a.C = n_classes; a.kind = label_kind; a.mask = label_mask; a.L = lut_len;
    a.slots = PL_LDS_BINS / (n_classes * n_classes);                       // >= 8 at 32 classes
    a.fill = fill;
    k_point_labels<<<(unsigned)blocks, PL_THREADS, 0, st>>>(a, labels_out,
                                                            with_labels ? (unsigned long long *)counts : nullptr, err);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
