// Evaluation statistics of test_step (utils/pipelines/trainer_lighting.py:186-253, trainer_lighting_bev.py:265-323):
// the row arg-max of the logits and the per-scan confusion counts that sklearn's jaccard_score is made of, and the
// packed per-scan records of the prediction dump.  Counts are integers accumulated in LDS bins and added with one
// global integer atomic per non-empty bin and block; the dump takes its positions from lidog_mix_split (mix.hip:
// per-block counts, one scan, in-wave ballot ranks).  No float atomic, no position from an atomic: two runs give the
// same bytes.
#include "common.h"
#include "row_argmax.h"

#define EV_THREADS 256
#define EV_ITERS 4                          // rows per thread of the confusion kernel, kept in registers
#define EV_TILE (EV_THREADS * EV_ITERS)
#define EV_MAX_CLASSES 32
#define EV_LDS_BINS 8192                    // int32 bins of a block (32 KiB): (C + 1) * C per scan of a pass
#define EV_MAX_SCANS 256                    // of the dump: lidog_mix_split's slots

// A block takes EV_TILE consecutive rows.  Its LDS holds the bins of `slots` consecutive scans; the scans of its rows
// [smin, smax] are covered in passes of `slots` scans (one pass when the rows of a scan are contiguous and the batch is
// small, as in a collated batch; any order of rows stays correct, it only takes more passes).  bin = (scan - base) *
// (C + 1) * C + (label + 1 or 0) * C + pred.
__global__ __launch_bounds__(EV_THREADS) void k_eval_confusion(const float *__restrict__ logits,
                                                               const int64_t *__restrict__ labels,
                                                               const int32_t *__restrict__ coords, int64_t n, int32_t C,
                                                               int32_t n_scans, int64_t ignore_label, int32_t slots,
                                                               int64_t *__restrict__ preds,
                                                               unsigned long long *__restrict__ counts,
                                                               int32_t *__restrict__ err) {
    __shared__ int32_t bins[EV_LDS_BINS];
    __shared__ int32_t s_lo, s_hi;
    if (threadIdx.x == 0) {
        s_lo = INT32_MAX;
        s_hi = -1;
    }
    __syncthreads();
    const int per_scan = (C + 1) * C;
    const int64_t base_row = (int64_t)blockIdx.x * EV_TILE;
    int32_t scan[EV_ITERS], bin[EV_ITERS];
    int lo = INT32_MAX, hi = -1;
#pragma unroll
    for (int it = 0; it < EV_ITERS; ++it) {
        const int64_t r = base_row + it * EV_THREADS + threadIdx.x;
        scan[it] = -1;
        bin[it] = 0;
        if (r < n) {
            const int p = ev_argmax(logits + r * C, C);
            preds[r] = p;
            const int64_t l = labels[r];
            const int row = (l == ignore_label || l < 0 || l >= C) ? 0 : (int)l + 1;
            const int32_t s = coords[4 * r];
            if (s >= 0 && s < n_scans) {
                scan[it] = s;
                bin[it] = row * C + p;
                lo = min(lo, s);
                hi = max(hi, s);
            } else {
                *err = 1;            // reported, never counted: no write outside counts
            }
        }
    }
    if (hi >= 0) {
        atomicMin(&s_lo, lo);
        atomicMax(&s_hi, hi);
    }
    __syncthreads();
    const int smin = s_lo, smax = s_hi;      // block-uniform
    for (int base = smin; base <= smax; base += slots) {
        const int ns = min(slots, smax - base + 1);
        const int nb = ns * per_scan;
        for (int j = threadIdx.x; j < nb; j += EV_THREADS) bins[j] = 0;
        __syncthreads();
#pragma unroll
        for (int it = 0; it < EV_ITERS; ++it) {
            const int d = scan[it] - base;
            if (scan[it] >= 0 && d >= 0 && d < ns) atomicAdd(&bins[d * per_scan + bin[it]], 1);   // a count
        }
        __syncthreads();
        for (int j = threadIdx.x; j < nb; j += EV_THREADS)
            if (bins[j]) atomicAdd(&counts[(int64_t)base * per_scan + j], (unsigned long long)bins[j]);
        __syncthreads();
    }
}

extern "C" int lidog_eval_confusion(const float *logits, const int64_t *labels, const int32_t *coords, int64_t n,
                                    int32_t n_classes, int32_t n_scans, int64_t ignore_label, int64_t *preds,
                                    int64_t *counts, int32_t *err, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0, "lidog_eval_confusion: n = %lld", (long long)n);
    LIDOG_REQUIRE(n_classes >= 1 && n_classes <= EV_MAX_CLASSES, "lidog_eval_confusion: %d classes (1..%d)", n_classes,
                  EV_MAX_CLASSES);
    LIDOG_REQUIRE(n_scans >= 0, "lidog_eval_confusion: n_scans = %d", n_scans);
    if (n == 0) return 0;
    LIDOG_REQUIRE(logits && labels && coords && preds && counts && err, "lidog_eval_confusion: null argument");
    const int64_t blocks = cdiv64(n, EV_TILE);
    LIDOG_REQUIRE(blocks < (int64_t)INT32_MAX, "lidog_eval_confusion: grid too large");
    const int32_t slots = EV_LDS_BINS / ((n_classes + 1) * n_classes);     // >= 7 at 32 classes
    k_eval_confusion<<<(unsigned)blocks, EV_THREADS, 0, st>>>(logits, labels, coords, n, n_classes, n_scans,
                                                              ignore_label, slots, preds,
                                                              (unsigned long long *)counts, err);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ prediction dump
// keys[i] = scan of a labelled row, -1 otherwise; table = the identity (slot = scan)
__global__ __launch_bounds__(EV_THREADS) void k_eval_keys(const int32_t *__restrict__ coords,
                                                          const int64_t *__restrict__ labels, int64_t n,
                                                          int32_t n_scans, int64_t ignore_label,
                                                          int32_t *__restrict__ keys, int32_t *__restrict__ table,
                                                          int32_t *__restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x;
    if (i < n_scans) table[i] = (int32_t)i;
    if (i >= n) return;
    const int32_t s = coords[4 * i];
    const bool in = s >= 0 && s < n_scans;
    if (!in) *err = 1;
    keys[i] = (in && labels[i] != ignore_label) ? s : -1;
}

// record j = (x, y, z, prediction, label) of kept row rows[j]; header = start of every scan, then the total
__global__ __launch_bounds__(EV_THREADS) void k_eval_records(const int32_t *__restrict__ coords,
                                                             const int64_t *__restrict__ preds,
                                                             const int64_t *__restrict__ labels,
                                                             const int32_t *__restrict__ rows,
                                                             const int32_t *__restrict__ slot_start, int32_t n_scans,
                                                             int64_t n, int32_t *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x;
    if (j <= n_scans) out[j] = slot_start[j];
    if (j >= n || j >= slot_start[n_scans]) return;
    const int64_t r = rows[j];
    int32_t *o = out + (n_scans + 1) + 5 * j;
    o[0] = coords[4 * r + 1];
    o[1] = coords[4 * r + 2];
    o[2] = coords[4 * r + 3];
    o[3] = (int32_t)preds[r];
    o[4] = (int32_t)labels[r];
}

extern "C" int64_t lidog_eval_pack_ws(int64_t n, int32_t n_scans) {
    const int64_t nn = n > 0 ? n : 0, s = n_scans > 0 ? n_scans : 0;   // keys [n], rows [n], table [s], slot_start [s + 1]
    return 2 * nn + 2 * s + 1 + lidog_mix_split_ws(nn, (int32_t)s);
}

extern "C" int lidog_eval_pack(const int32_t *coords, const int64_t *preds, const int64_t *labels, int64_t n,
                               int32_t n_scans, int64_t ignore_label, int32_t *out, int32_t *err, int32_t *ws,
                               void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX, "lidog_eval_pack: n = %lld out of range", (long long)n);
    LIDOG_REQUIRE(n_scans >= 1 && n_scans <= EV_MAX_SCANS, "lidog_eval_pack: %d scans (1..%d)", n_scans, EV_MAX_SCANS);
    LIDOG_REQUIRE(out && err && ws, "lidog_eval_pack: null argument");
    int32_t *keys = ws, *rows = ws + n, *table = ws + 2 * n, *slot_start = table + n_scans,
            *split_ws = slot_start + n_scans + 1;
    const int64_t span = n > n_scans + 1 ? n : n_scans + 1;
    const unsigned grid = (unsigned)cdiv64(span, EV_THREADS);
    k_eval_keys<<<grid, EV_THREADS, 0, st>>>(coords, labels, n, n_scans, ignore_label, keys, table, err);
    LIDOG_LAUNCH_CHECK();
    if (lidog_mix_split(keys, n, table, n_scans, n_scans, rows, slot_start, split_ws, stream)) return 1;
    k_eval_records<<<grid, EV_THREADS, 0, st>>>(coords, preds, labels, rows, slot_start, n_scans, n, out);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
