// Training-step statistics (log_losses of utils/pipelines/trainer_lighting_2d.py:203-291, trainer_lighting.py:118-153):
// the batch-wide confusion counts that the per-class IoU and the class occurrences of every logged tensor are made
// of: the point logits of each source and every BEV level, all in ONE launch.  The method is evalstats.hip's: row
// arg-max, integer LDS bins, one global integer atomic per non-empty bin and block; no float atomic, so two runs give
// the same bytes.  What differs: no per-scan split, no predictions written, several tensors ("segments") per launch.
#include "common.h"
#include "row_argmax.h"

#define TS_THREADS 256                      // one row per thread and chunk
#define TS_CHUNKS 4
#define TS_ROWS (TS_THREADS * TS_CHUNKS)    // rows of a block, all of one segment
#define TS_MAX_CLASSES 32
#define TS_MAX_SEGMENTS 8
#define TS_STAGE (TS_THREADS * (TS_MAX_CLASSES + 1))
#define TS_BINS ((TS_MAX_CLASSES + 1) * TS_MAX_CLASSES)

// the segment table, a kernel argument by value: block b belongs to the segment s with first[s] <= b < first[s + 1]
struct TsTable {
    const float *logits[TS_MAX_SEGMENTS];
    const int64_t *labels[TS_MAX_SEGMENTS];
    int64_t n[TS_MAX_SEGMENTS];
    int32_t first[TS_MAX_SEGMENTS + 1];
};

// A row is C consecutive floats (28 bytes at 7 classes): a thread that walked its own row in global memory would
// make every wave load touch 64 rows.  Instead the block copies the C * 256 floats of a chunk, which are contiguous, to
// LDS with consecutive lanes on consecutive addresses (16 bytes per lane where the chunk starts on a 16-byte boundary),
// and every thread reads its row from there.  The LDS row stride is C | 1: an odd number of dwords, so the 32 lanes of
// a bank group fall on 32 different banks whatever C is.
__global__ __launch_bounds__(TS_THREADS) void k_train_confusion(TsTable t, int32_t n_segments, int32_t C,
                                                                int64_t ignore_label,
                                                                unsigned long long *__restrict__ counts,
                                                                int32_t *__restrict__ err) {
    __shared__ __align__(16) float stage[TS_STAGE];
    __shared__ int32_t bins[TS_BINS];
    __shared__ int32_t bad;
    int s = 0;
    while (s + 1 < n_segments && (int32_t)blockIdx.x >= t.first[s + 1]) ++s;      // block-uniform, at most 7 steps
    const float *__restrict__ logits = t.logits[s];
    const int64_t *__restrict__ labels = t.labels[s];
    const int64_t n = t.n[s];
    const int64_t row0 = (int64_t)(blockIdx.x - t.first[s]) * TS_ROWS;
    const int per_seg = (C + 1) * C;
    const int stride = C | 1;
    for (int j = threadIdx.x; j < per_seg; j += TS_THREADS) bins[j] = 0;
    if (threadIdx.x == 0) bad = 0;
    for (int ch = 0; ch < TS_CHUNKS; ++ch) {
        const int64_t base = row0 + (int64_t)ch * TS_THREADS;
        if (base >= n) break;                                                      // block-uniform
        const int rows = (int)min((int64_t)TS_THREADS, n - base);
        const int len = rows * C;
        const float *__restrict__ g = logits + base * C;
        __syncthreads();                    // the previous chunk's rows are read (first chunk: bins and bad are cleared)
        if (stride == C) {
            int done = 0;
            if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
                const int len4 = len >> 2;
                const float4 *__restrict__ g4 = reinterpret_cast<const float4 *>(g);
                float4 *s4 = reinterpret_cast<float4 *>(stage);
                for (int j = threadIdx.x; j < len4; j += TS_THREADS) s4[j] = g4[j];
                done = len4 << 2;
            }
            for (int j = done + threadIdx.x; j < len; j += TS_THREADS) stage[j] = g[j];
        } else {
            for (int j = threadIdx.x; j < len; j += TS_THREADS) {
                const int r = j / C;
                stage[r * stride + (j - r * C)] = g[j];
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            const int p = ev_argmax(stage + threadIdx.x * stride, C);
            const int64_t l = labels[base + threadIdx.x];
            int row = 0;
            if (l >= 0 && l < C && l != ignore_label)
                row = (int)l + 1;
            else if (l != ignore_label)
                bad = 1;                    // every writer stores the same value
            atomicAdd(&bins[row * C + p], 1);                                      // a count
        }
    }
    __syncthreads();
    unsigned long long *__restrict__ out = counts + (int64_t)s * per_seg;
    for (int j = threadIdx.x; j < per_seg; j += TS_THREADS)
        if (bins[j]) atomicAdd(&out[j], (unsigned long long)bins[j]);
    if (threadIdx.x == 0 && bad) atomicOr(err, 1 << s);
}

extern "C" int lidog_train_confusion(const float *const *logits, const int64_t *const *labels, const int64_t *n,
                                     int32_t n_segments, int32_t n_classes, int64_t ignore_label, int64_t *counts,
                                     int32_t *err, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n_segments >= 1 && n_segments <= TS_MAX_SEGMENTS, "lidog_train_confusion: %d segments (1..%d)",
                  n_segments, TS_MAX_SEGMENTS);
    LIDOG_REQUIRE(n_classes >= 1 && n_classes <= TS_MAX_CLASSES, "lidog_train_confusion: %d classes (1..%d)", n_classes,
                  TS_MAX_CLASSES);
    LIDOG_REQUIRE(logits && labels && n, "lidog_train_confusion: null segment table");
    TsTable t;
    int64_t blocks = 0;
    for (int s = 0; s < TS_MAX_SEGMENTS; ++s) {
        const bool in = s < n_segments;
        if (in) {
            LIDOG_REQUIRE(n[s] >= 0, "lidog_train_confusion: segment %d: n = %lld", s, (long long)n[s]);
            LIDOG_REQUIRE(n[s] == 0 || (logits[s] && labels[s]), "lidog_train_confusion: segment %d: null pointer", s);
        }
        t.logits[s] = in ? logits[s] : nullptr;
        t.labels[s] = in ? labels[s] : nullptr;
        t.n[s] = in ? n[s] : 0;
        LIDOG_REQUIRE(blocks < (int64_t)INT32_MAX, "lidog_train_confusion: grid too large");
        t.first[s] = (int32_t)blocks;
        blocks += cdiv64(t.n[s], TS_ROWS);
    }
    LIDOG_REQUIRE(blocks < (int64_t)INT32_MAX, "lidog_train_confusion: grid too large");
    t.first[TS_MAX_SEGMENTS] = (int32_t)blocks;
    if (blocks == 0) return 0;
    LIDOG_REQUIRE(counts && err, "lidog_train_confusion: null counts or err");
    k_train_confusion<<<(unsigned)blocks, TS_THREADS, 0, st>>>(t, n_segments, n_classes, ignore_label,
                                                               (unsigned long long *)counts, err);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
