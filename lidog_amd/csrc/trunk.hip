// Trunk executor: the MinkUNet encoder-decoder (utils/models/minkunet_bev.py:302-399, utils/models/minkunet.py:97-158)
// forward and backward as ONE host call each.
//
// The python operator path (lidog_amd/me.py) issues ~1 000 launches per training step through ~550 autograd nodes; the
// launch sequence itself is static (63 convolutions, 62 BatchNorms, 4 concatenations) -- only row counts and map
// pointers change per batch.  This file walks a table-driven program and calls the SAME entry points of this library
// in the same order with the same arguments as me._SparseConvFn / me._BatchNormFn / me._Cat2Fn do, so every result is
// bit-identical to the operator path (tests/test_gpu_trunk.py); what changes is the host cost of a step.
//
// No state is kept between calls except a pool of timing-less events for the second backward stream.  All memory comes
// from the caller: `arena` (activations that live until backward), `garena` (gradients; never reused inside one
// backward pass, so the weight gradients running on the lane stream may read them at any time), `scratch` (product
// rows, reduction workspaces: main stream only), `lane_scratch` (weight-gradient partial slabs: lane stream only).
#include <stdlib.h>

#include <mutex>
#include <vector>

#include "common.h"

void lidog_gemm_multi_suspend(int delta);   // sconv_mfma.hip

namespace {

// ---- table layouts (int64 rows; python fills them as numpy arrays, lidog_amd/trunk.py)
enum { TC_KIND, TC_MAP, TC_CIN, TC_COUT, TC_K, TC_W, TC_WT, TC_GW, TC_BIAS, TC_GBIAS, TC_BNW, TC_BNB, TC_BNRM, TC_BNRV,
       TC_GBNW, TC_GBNB, TC_ITEMS, TC_NITEMS, TC_ITEMOFF, TC_ACC, TC_COLS = 20 };
enum { TM_K, TM_NIN, TM_NOUT, TM_P, TM_PAIR_IN, TM_PAIR_OUT, TM_RP_OUT, TM_RL_OUT, TM_RP_IN, TM_RL_IN, TM_TILES,
       TM_NTILES, TM_NBR, TM_IDENT, TM_PERM, TM_WMASK, TM_ORDER, TM_COLS = 20 };
enum { TO_TYPE, TO_CONV, TO_IN, TO_OUT, TO_RELU, TO_RES, TO_FOLD, TO_B, TO_COLS = 8 };
enum { TB_LEVEL, TB_CH, TB_EXT, TB_COLS = 4 };
enum { REC_PRE, REC_MEAN, REC_INVSTD, REC_BITS, REC_COLS = 4 };   // REC_BITS: arena offset + 1 of the ReLU bit mask, 0 = none

enum { KIND_K3 = 0, KIND_DOWN = 1, KIND_UP = 2, KIND_1X1 = 3, KIND_STEM = 4 };
enum { OP_CONVBN = 0, OP_CAT = 1, OP_CONV = 2 };

struct Bump {
    char *base;
    int64_t off, cap, peak;
    bool dry;
    void reset() { off = 0; }
    void *take(int64_t bytes) {
        int64_t a = (bytes + 255) / 256 * 256;
        void *p = dry ? (void *)(uintptr_t)(4096 + off) : (void *)(base + off);
        off += a;
        if (off > peak) peak = off;
        return p;
    }
    bool ok() const { return dry || peak <= cap; }
};

// where a step launches: the stream, and the allocator its per-launch scratch comes from
struct Where {
    void *stream;
    Bump *scratch;
};

struct Ctx {
    const int64_t *convs;
    const double *conv_f;
    int n_convs;
    const int64_t *maps;
    int n_maps;
    const int64_t *ops;
    int n_ops;
    const int64_t *bufs;
    int n_bufs;
    const int64_t *level_rows;
    const int64_t *ext;
    bool dry;
    int64_t rows(int b) const { return level_rows[bufs[b * TB_COLS + TB_LEVEL]]; }
    int ch(int b) const { return (int)bufs[b * TB_COLS + TB_CH]; }
    int64_t bytes(int b) const { return rows(b) * ch(b) * 4; }
    int64_t ext_of(int64_t b) const { return bufs[b * TB_COLS + TB_EXT]; }
    const int64_t *op(int o) const { return ops + (int64_t)o * TO_COLS; }
    const int64_t *conv(const int64_t *op) const { return convs + op[TO_CONV] * TC_COLS; }
    const int64_t *map(const int64_t *c) const { return maps + c[TC_MAP] * TM_COLS; }
};

template <typename T>
inline T *P(int64_t v) { return reinterpret_cast<T *>(static_cast<uintptr_t>(v)); }

// ---- data parallelism inside the executor (train_lidog.py:227-231: DDP + MinkowskiSyncBatchNorm).
// dp [DP_COLS] int64, NULL = single process.  Two transports: native RCCL communicators of this library
// (csrc/comm.hip; the statistics all-reduce is queued on the launch stream itself, between the reduction and the apply
// kernel, the gradient buckets on a stream of their own) or a host callback `int cb(int what, int64 a, int64 b)` that
// performs the collective with whatever the caller has (torch.distributed over gloo in the two-rank tests):
// what 0 = all-reduce (sum) of b doubles at device address a, in order on the launch stream; 1 = gradient bucket a has
// all its gradients queued.
enum { DP_SYNC_BN, DP_COMM_BN, DP_CALLBACK, DP_COMM_GRAD, DP_COMM_STREAM, DP_GRAD_BASE, DP_N_BUCKETS, DP_BUCKETS,
       DP_PENDING, DP_PARAM_BUCKET, DP_PEER, DP_COLS = 12 };
typedef int (*dp_callback_t)(int32_t what, int64_t a, int64_t b);

struct Dp {
    const int64_t *d;
    bool sync_bn() const { return d && d[DP_SYNC_BN] != 0; }
    bool buckets() const { return d && d[DP_N_BUCKETS] > 0 && d[DP_PENDING] && d[DP_PARAM_BUCKET]; }
    // the peer communicator's calls are bound to one stream (csrc/comm.hip): follow this pass's launch stream
    int bind(void *st) const {
        if (d && d[DP_PEER]) return lidog_peer_rebind_stream(P<void>(d[DP_PEER]), st);
        return 0;
    }
    int check() const {
        if (!d) return 0;
        LIDOG_REQUIRE(!d[DP_SYNC_BN] || d[DP_COMM_BN] || d[DP_CALLBACK] || d[DP_PEER],
                      "trunk: SyncBatchNorm statistics need a communicator or a callback");
        if (d[DP_N_BUCKETS] > 0) {
            LIDOG_REQUIRE(d[DP_BUCKETS] && d[DP_PENDING] && d[DP_PARAM_BUCKET], "trunk: gradient bucket tables missing");
            LIDOG_REQUIRE(d[DP_CALLBACK] || (d[DP_COMM_GRAD] && d[DP_COMM_STREAM] && d[DP_GRAD_BASE]),
                          "trunk: gradient buckets need a communicator with its stream, or a callback");
        }
        return 0;
    }
    // sum over the ranks of n doubles, in order on `st`
    int allreduce_f64(double *buf, int64_t n, void *st) const {
        // statistics messages: the one-shot peer all-reduce where it is set up (lidog_amd.comm), else the communicator
        if (d[DP_PEER] && n <= lidog_peer_max_doubles(P<void>(d[DP_PEER])))
            return lidog_peer_allreduce_f64(P<void>(d[DP_PEER]), buf, n, st);
        if (d[DP_COMM_BN]) return lidog_allreduce_f64(buf, n, P<void>(d[DP_COMM_BN]), st);
        LIDOG_REQUIRE(d[DP_CALLBACK], "trunk: no transport for the statistics all-reduce");
        int rc = reinterpret_cast<dp_callback_t>(static_cast<uintptr_t>(d[DP_CALLBACK]))(0, (int64_t)(uintptr_t)buf, n);
        LIDOG_REQUIRE(rc == 0, "trunk: the statistics all-reduce callback failed (%d)", rc);
        return 0;
    }
};

// a step that can fail: RUN hands its error code on; TRY is RUN for launches, which dry mode leaves out
#define RUN(expr)                            \
    do {                                     \
        if (int _rc = (expr)) return _rc;    \
    } while (0)
#define TRY(expr)                  \
    do {                           \
        if (!ctx.dry) RUN(expr);   \
    } while (0)

// events for forking the lane stream behind the main stream (one per convolution) and joining it again; one pool per
// process (one process drives one GPU), grown under a lock: backward passes run on autograd's device threads
hipEvent_t *event_pool(int n) {
    static std::vector<hipEvent_t> pool;
    static std::mutex lock;
    std::lock_guard<std::mutex> guard(lock);
    if ((int)pool.capacity() < 4096) pool.reserve(4096);   // the returned pointer stays valid while the pool grows
    while ((int)pool.size() < n) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
        pool.push_back(e);
    }
    return pool.data();
}

// order between streams; nothing happens in dry mode (no events exist there)
int ev_record(const Ctx &ctx, hipEvent_t ev, void *st) {
    if (!ctx.dry) LIDOG_CHECK_HIP(hipEventRecord(ev, (hipStream_t)st));
    return 0;
}
int ev_wait(const Ctx &ctx, void *st, hipEvent_t ev) {
    if (!ctx.dry) LIDOG_CHECK_HIP(hipStreamWaitEvent((hipStream_t)st, ev, 0));
    return 0;
}
// whatever `behind` is handed from now on runs after what `ahead` holds at this moment
int ev_order(const Ctx &ctx, void *ahead, hipEvent_t ev, void *behind) {
    RUN(ev_record(ctx, ev, ahead));
    return ev_wait(ctx, behind, ev);
}

// sorted rows of a sparse symmetric 3^3 map `m` and channel counts its kernel takes: the convolution (and its data
// gradient, over the mirrored offsets) runs on the output-stationary kernel (csrc/sconv_os.hip), no product rows
bool takes_os(const int64_t *m, int64_t Cin, int64_t Cout) {
    return m[TM_PERM] && m[TM_WMASK] && m[TM_ORDER] && m[TM_NBR] && m[TM_NIN] == m[TM_NOUT] && Cin % 32 == 0 &&
           Cout % 32 == 0 && lidog_get_sparse_core() == 1;
}

// op o is conv1 of a layer's first block and op o + 1 the block's 1x1 downsample convolution + BatchNorm on the same
// input (resnet_block.py:8-56; minkunet_bev.py:414-420).  The structural part only: what a pass asks of the branch
// beyond that (no residual, no ReLU, not external, side branches left, ...) stands where it is asked.
bool branch_follows(const Ctx &ctx, int o) {
    if (o < 0 || o + 1 >= ctx.n_ops) return false;
    const int64_t *op = ctx.op(o), *nx = ctx.op(o + 1);
    return op[TO_TYPE] == OP_CONVBN && op[TO_FOLD] && nx[TO_TYPE] == OP_CONVBN && nx[TO_IN] == op[TO_IN] &&
           ctx.conv(nx)[TC_KIND] == KIND_1X1;
}

int check_tables(const Ctx &ctx, bool grads) {
    LIDOG_REQUIRE(ctx.n_convs > 0 && ctx.n_ops > 0 && ctx.n_bufs > 0 && ctx.n_maps > 0, "trunk: empty tables");
    for (int b = 0; b < ctx.n_bufs; ++b)
        LIDOG_REQUIRE(ctx.rows(b) > 0 && ctx.ch(b) > 0, "trunk: buffer %d has no rows or channels", b);
    for (int o = 0; o < ctx.n_ops; ++o) {
        const int64_t *op = ctx.op(o);
        auto buf_ok = [&](int64_t b) { return b >= 0 && b < ctx.n_bufs; };
        LIDOG_REQUIRE(buf_ok(op[TO_IN]) && buf_ok(op[TO_OUT]), "trunk: op %d names a missing buffer", o);
        if (op[TO_TYPE] == OP_CAT) {
            LIDOG_REQUIRE(buf_ok(op[TO_B]), "trunk: op %d names a missing buffer", o);
            int a = (int)op[TO_IN], b = (int)op[TO_B], out = (int)op[TO_OUT];
            LIDOG_REQUIRE(ctx.rows(a) == ctx.rows(b) && ctx.rows(a) == ctx.rows(out) &&
                              ctx.ch(a) + ctx.ch(b) == ctx.ch(out) && ctx.ch(a) % 4 == 0 && ctx.ch(b) % 4 == 0,
                          "trunk: op %d concatenates mismatching buffers", o);
            continue;
        }
        LIDOG_REQUIRE(op[TO_CONV] >= 0 && op[TO_CONV] < ctx.n_convs, "trunk: op %d names a missing convolution", o);
        const int64_t *c = ctx.conv(op);
        LIDOG_REQUIRE(c[TC_MAP] >= 0 && c[TC_MAP] < ctx.n_maps, "trunk: op %d names a missing map", o);
        const int64_t *m = ctx.map(c);
        const int kind = (int)c[TC_KIND];
        const int64_t n_in = kind == KIND_UP ? m[TM_NOUT] : m[TM_NIN], n_out = kind == KIND_UP ? m[TM_NIN] : m[TM_NOUT];
        LIDOG_REQUIRE(ctx.rows((int)op[TO_IN]) == n_in && ctx.rows((int)op[TO_OUT]) == n_out,
                      "trunk: op %d: buffers of %lld -> %lld rows on a map of %lld -> %lld rows", o,
                      (long long)ctx.rows((int)op[TO_IN]), (long long)ctx.rows((int)op[TO_OUT]), (long long)n_in,
                      (long long)n_out);
        LIDOG_REQUIRE(ctx.ch((int)op[TO_IN]) == c[TC_CIN] && ctx.ch((int)op[TO_OUT]) == c[TC_COUT],
                      "trunk: op %d: channel counts do not match its convolution", o);
        LIDOG_REQUIRE(m[TM_K] == c[TC_K] && m[TM_NTILES] > 0 && m[TM_TILES], "trunk: op %d: map / kernel mismatch", o);
        LIDOG_REQUIRE(c[TC_W] && (c[TC_GW] || !grads), "trunk: op %d: missing weights", o);
        if (op[TO_TYPE] == OP_CONVBN) {
            LIDOG_REQUIRE(c[TC_COUT] % 4 == 0, "trunk: op %d: BatchNorm width must be a multiple of 4", o);
            LIDOG_REQUIRE(c[TC_BNW] && c[TC_BNB] && c[TC_BNRM] && c[TC_BNRV] && ((c[TC_GBNW] && c[TC_GBNB]) || !grads),
                          "trunk: op %d: missing BatchNorm tensors", o);
            if (op[TO_RES] >= 0)
                LIDOG_REQUIRE(buf_ok(op[TO_RES]) && ctx.bytes((int)op[TO_RES]) == ctx.bytes((int)op[TO_OUT]),
                              "trunk: op %d: residual of another shape", o);
        }
        switch (kind) {
            case KIND_K3:
                // sorted rows (output-stationary kernel) stand in for the per-row lists of the reduction pass
                LIDOG_REQUIRE(m[TM_PAIR_IN] && m[TM_PAIR_OUT] && c[TC_CIN] % 4 == 0 &&
                                  (takes_os(m, c[TC_CIN], c[TC_COUT]) ||
                                   (m[TM_RP_OUT] && m[TM_RL_OUT] && m[TM_RP_IN] && m[TM_RL_IN])),
                              "trunk: op %d: 3^3 map without pair or row lists", o);
                break;
            case KIND_DOWN:
            case KIND_UP:
                LIDOG_REQUIRE(m[TM_PAIR_IN] && m[TM_PAIR_OUT] && m[TM_RP_OUT] && m[TM_RL_OUT] && c[TC_CIN] % 4 == 0,
                              "trunk: op %d: 2^3 map without pair or row lists", o);
                break;
            case KIND_1X1:
                LIDOG_REQUIRE(m[TM_IDENT] && m[TM_K] == 1, "trunk: op %d: 1x1 convolution without identity rows", o);
                break;
            case KIND_STEM:
                LIDOG_REQUIRE(m[TM_NBR] && m[TM_PAIR_IN] && m[TM_PAIR_OUT] && c[TC_CIN] == 1,
                              "trunk: op %d: stem without neighbour table", o);
                break;
            default:
                LIDOG_REQUIRE(false, "trunk: op %d: unknown convolution kind %d", o, kind);
        }
    }
    return 0;
}

inline const int32_t *tile_row(const int64_t *m, int r) { return P<const int32_t>(m[TM_TILES]) + r * m[TM_NTILES]; }

// Fusions the executor applies on top of the operator path's launch sequence (results stay bit-identical):
//   1 = BatchNorm-backward statistics in the epilogue of the data-gradient reduction that produces the gradient
//   2 = ReLU masks of the BatchNorm + residual + ReLU layers kept as bits (backward reads 1/32 of the saved output)
//   4 = BatchNorm + ReLU between the two convolutions of a block applied in the second one's staging (in_bn_reader below)
int g_fusions = 7;
// the downsample branch of a layer's first block on the second stream in the forward pass (A/B: LIDOG_SIDE_FORWARD=0)
int g_side_forward = [] {
    const char *e = getenv("LIDOG_SIDE_FORWARD");
    return (e && e[0] == '0') ? 0 : 1;
}();
enum { SIDE_EVENT0 = 3000 };   // events of the forward pass's lane forks / joins, behind everything the backward pass uses
// ... and in the backward pass the same branch (BatchNorm backward + 1x1 data gradient of the downsample convolution) runs
// on a third stream of this library's, between the residual add's gradient and the block input's (A/B: LIDOG_SIDE_BACKWARD=0)
int g_side_backward = [] {
    const char *e = getenv("LIDOG_SIDE_BACKWARD");
    return (e && e[0] == '0') ? 0 : 1;
}();
enum { SIDE_BWD_EVENT0 = SIDE_EVENT0 + 64, MAX_SIDE = 16 };   // four events per side branch, at most MAX_SIDE per pass

hipStream_t side_stream() {
    static std::mutex lock;
    static std::vector<std::pair<int, hipStream_t>> streams;     // one per device this process drives
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> guard(lock);
    for (auto &p : streams)
        if (p.first == dev) return p.second;
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return nullptr;
    streams.emplace_back(dev, st);
    return st;
}

// The BatchNorm + ReLU of op o needs no pass of its own when its output has exactly one reader and that reader is a 3^3
// convolution + BatchNorm on the matrix-core kernels (conv1 -> BN -> ReLU -> conv2 of a BasicBlock): the reader takes
// the raw convolution output and the BatchNorm vectors instead (lidog_sconv_*_in_bn), forward and weight gradient; the
// BatchNorm's own backward pass already works from the raw output (mask recomputed from it).  Returns the reader's op
// index, or -1.  Pure function of the tables: the forward and the backward pass decide alike.
int in_bn_reader(const Ctx &ctx, int o) {
    if (!(g_fusions & 4) || lidog_get_sparse_core() != 1) return -1;
    const int64_t *op = ctx.op(o);
    if (op[TO_TYPE] != OP_CONVBN || !op[TO_RELU] || op[TO_RES] >= 0) return -1;
    const int64_t out = op[TO_OUT];
    if (ctx.ext_of(out) >= 0) return -1;
    int reader = -1, users = 0;
    for (int q = 0; q < ctx.n_ops; ++q) {
        const int64_t *u = ctx.op(q);
        if (u[TO_TYPE] == OP_CAT) {
            if (u[TO_IN] == out || u[TO_B] == out) ++users;
            continue;
        }
        if (u[TO_TYPE] == OP_CONVBN && u[TO_RES] == out) ++users;
        if (u[TO_IN] == out) {
            ++users;
            reader = q;
        }
    }
    if (users != 1 || reader < o) return -1;
    const int64_t *u = ctx.op(reader);
    const int64_t *c = ctx.conv(u);
    if (u[TO_TYPE] != OP_CONVBN || c[TC_KIND] != KIND_K3 || c[TC_CIN] % 32 || c[TC_COUT] % 32) return -1;
    return reader;
}

// what the reader of a folded BatchNorm is handed instead of the normalised rows
struct InBnArgs {
    const float *pre, *mean, *invstd, *w, *b;
};

// Optional timing of the gathered GEMM's launches (bench.py's roofline figure): HIP events on the launch stream around
// every lidog_sconv_gemm call of the executor, with the launch's algorithmic FLOPs and bytes (every distinct input row
// and weight read once, every product row written once, the gather index read once: SURVEY.md 8(d)).
struct GemmRec {
    hipEvent_t e0, e1;
    double flops, bytes;
};
bool g_timing = false;
// algorithmic bytes of the two other HBM-heavy families while timing is on (DESIGN.md section 3 formulas; bench.py sets
// them against the PMC traffic of the same families): [0] MFMA weight-gradient launches, [1] their bytes
// 4 P (Cin + Cout) + 4 K Cin Cout (1 + 2 slabs / K), [2] per-row reduction launches, [3] their bytes
// 4 (P + N) C + 4 (P + N) (+ 8 N C for the saved input and mask / addend the backward-statistics form also reads)
double g_work[6] = {0, 0, 0, 0, 0, 0};   // [4] output-stationary launches, [5] their bytes 4 n (Cin + Cout) + 4 K Cin Cout + 4 K n
inline bool counting(const Ctx &ctx) { return g_timing && !ctx.dry; }
void work_wgrad(const Ctx &ctx, const int64_t *m, int Cin, int Cout, int K, int slabs) {
    if (!counting(ctx) || Cin % 32 || Cout % 32) return;     // the MFMA kernels only
    g_work[0] += 1;
    g_work[1] += 4.0 * (double)m[TM_P] * (Cin + Cout) + 4.0 * (double)Cin * Cout * (K + 2.0 * (slabs > 1 ? slabs : 1));
}
// bwdstats: the backward-statistics form of the reduction
void work_reduce(const Ctx &ctx, const int64_t *m, int64_t n, int C, bool bwdstats) {
    if (!counting(ctx)) return;
    g_work[2] += 1;
    g_work[3] += 4.0 * ((double)m[TM_P] + n) * C + 4.0 * ((double)m[TM_P] + n) + (bwdstats ? 8.0 * (double)n * C : 0.0);
}
// addend: channels of the rows added in the epilogue (data gradient of a block's conv1), else 0
void work_os(const Ctx &ctx, int64_t n, int Cin, int Cout, int K, int addend) {
    if (!counting(ctx)) return;
    g_work[4] += 1;
    g_work[5] += 4.0 * n * (Cin + Cout + addend) + 4.0 * K * Cin * Cout + 4.0 * K * n;
}
std::vector<GemmRec> g_recs;
std::vector<hipEvent_t> g_spare;

hipEvent_t timing_event() {
    hipEvent_t e = nullptr;
    if (!g_spare.empty()) {
        e = g_spare.back();
        g_spare.pop_back();
    } else if (hipEventCreate(&e) != hipSuccess) {
        e = nullptr;
    }
    return e;
}

// n_src: rows of A (the gathered matrix)
int gemm(const Ctx &ctx, const int64_t *m, const float *A, int64_t n_src, const int32_t *gather, const float *B,
         const float *bias, int Cin, int Cout, float *out, const int32_t *scatter, void *st,
         const InBnArgs *in_bn = nullptr) {
    if (ctx.dry) return 0;
    GemmRec rec{nullptr, nullptr, 0, 0};
    if (g_timing) {
        rec.e0 = timing_event();
        rec.e1 = timing_event();
        LIDOG_REQUIRE(rec.e0 && rec.e1, "trunk: cannot create timing events");
        const double rows = (double)m[TM_P], src = (double)(n_src < m[TM_P] ? n_src : m[TM_P]);
        rec.flops = 2.0 * rows * Cin * Cout;
        rec.bytes = 4.0 * (src * Cin + rows * Cout + (double)m[TM_K] * Cin * Cout) + 4.0 * rows;
        LIDOG_CHECK_HIP(hipEventRecord(rec.e0, (hipStream_t)st));
    }
    int rc = in_bn ? lidog_sconv_gemm_in_bn(in_bn->pre, gather, B, bias, tile_row(m, 0), tile_row(m, 1), tile_row(m, 2),
                                            (int32_t)m[TM_NTILES], Cin, Cout, out, scatter, in_bn->mean, in_bn->invstd,
                                            in_bn->w, in_bn->b, 1, n_src, st)
                   : lidog_sconv_gemm(A, gather, B, bias, tile_row(m, 0), tile_row(m, 1), tile_row(m, 2),
                                      (int32_t)m[TM_NTILES], Cin, Cout, out, scatter, n_src, st);
    if (rc) return rc;
    if (g_timing) {
        LIDOG_CHECK_HIP(hipEventRecord(rec.e1, (hipStream_t)st));
        g_recs.push_back(rec);
    }
    return 0;
}

// ---- the forward pass, step by step
struct Forward {
    const Ctx &ctx;
    const Dp &dp;
    int64_t *rec;
    Bump ar, sc;
    void *stream, *lane;
    const bool sync;
    std::vector<float *> bp;                // activation buffers
    std::vector<hipEvent_t> join_of;        // buffer -> event after which its lane-made contents are complete
    // buffers whose BatchNorm + ReLU is applied by their reader (fusion 4): filled when the producer has run
    std::vector<InBnArgs> lazy;
    hipEvent_t *side_ev = nullptr;
    int n_side = 0;

    // One convolution (+ the statistics of its BatchNorm) and, separately, the BatchNorm's finalise + apply: under
    // SyncBatchNorm an all-reduce of the statistics sits between the two, and the first block of a layer sends the
    // statistics of conv1 and of its 1x1 downsample convolution (both read the block input) in ONE message
    // (me.BasicBlock._forward_joint_sync).
    struct Pending {
        int o;
        const int64_t *op, *c;
        float *pre, *mean, *invstd, *y;
        uint32_t *bits;
        double *sums;
        int64_t n;
        int Cout;
        float eps, mom;
    };

    Forward(const Ctx &c, const Dp &d, int64_t *rec_, Bump arena, Bump scratch, void *stream_, void *lane_)
        : ctx(c), dp(d), rec(rec_), ar(arena), sc(scratch), stream(stream_), lane(lane_), sync(d.sync_bn()),
          bp(c.n_bufs, nullptr), join_of(c.n_bufs, nullptr),
          lazy(c.n_bufs, InBnArgs{nullptr, nullptr, nullptr, nullptr, nullptr}) {}

    // the launch stream with the per-op scratch; a side branch runs on Where{lane, &ar}: the lane and the ARENA (the
    // per-op scratch is recycled by the launch stream's next op while the lane may still be reading)
    Where on_stream() { return Where{stream, &sc}; }

    // activation buffers: external ones are the caller's tensors, the others live in the arena
    int place_buffers() {
        int64_t *buf_off = rec + (int64_t)ctx.n_ops * REC_COLS;
        for (int b = 0; b < ctx.n_bufs; ++b) {
            int64_t e = ctx.ext_of(b);
            if (e >= 0) {
                bp[b] = P<float>(ctx.ext[e]);
                buf_off[b] = -1;
                LIDOG_REQUIRE(ctx.dry || bp[b], "trunk: external buffer %d missing", b);
            } else {
                buf_off[b] = ar.off;
                bp[b] = (float *)ar.take(ctx.bytes(b));
            }
        }
        return 0;
    }

    // the four events of the next side branch (fork, branch statistics ready, all-reduce done, branch output ready),
    // the pool's range created on first use; dry mode: none
    int side_events(hipEvent_t ev[4]) {
        for (int i = 0; i < 4; ++i) ev[i] = nullptr;
        if (ctx.dry) return 0;
        if (!side_ev) {
            side_ev = event_pool(SIDE_EVENT0 + 4 * MAX_SIDE);
            LIDOG_REQUIRE(side_ev, "trunk: cannot create events");
            side_ev += SIDE_EVENT0;
        }
        for (int i = 0; i < 4; ++i) ev[i] = side_ev[4 * n_side + i];
        return 0;
    }

    // the launch stream is about to read buffer b: wait for the side branch that made it on the lane, if one did
    int join(int64_t b, Where w) {
        if (!join_of[b]) return 0;
        RUN(ev_wait(ctx, w.stream, join_of[b]));
        join_of[b] = nullptr;
        return 0;
    }

    // sums_at: where this layer's (sum x, sum x^2, rows) go when they are part of a joint message, else NULL
    int conv(int o, double *sums_at, Where w, Pending &pd) {
        const int64_t *op = ctx.op(o);
        int64_t *r = rec + (int64_t)o * REC_COLS;
        const int64_t *c = ctx.conv(op);
        const int64_t *m = ctx.map(c);
        const int kind = (int)c[TC_KIND], Cin = (int)c[TC_CIN], Cout = (int)c[TC_COUT], K = (int)c[TC_K];
        const bool bn = op[TO_TYPE] == OP_CONVBN;
        const float *x = bp[op[TO_IN]];
        // an input made by a side branch on the lane (in MinkUNet34 such a buffer is only ever read as a residual, below;
        // a program that feeds it to a convolution is ordered here)
        if (w.stream == stream) RUN(join(op[TO_IN], w));
        const InBnArgs *in_bn = lazy[op[TO_IN]].pre ? &lazy[op[TO_IN]] : nullptr;   // 3^3 convolution + BatchNorm only
        const int64_t n = ctx.rows((int)op[TO_OUT]), n_in = ctx.rows((int)op[TO_IN]);
        const float *W = P<const float>(c[TC_W]), *bias = P<const float>(c[TC_BIAS]);
        float *y = bp[op[TO_OUT]];
        float *pre = y, *mean = nullptr, *invstd = nullptr;
        const float eps = (float)ctx.conv_f[op[TO_CONV] * 2], mom = (float)ctx.conv_f[op[TO_CONV] * 2 + 1];
        if (bn) {
            r[REC_PRE] = ar.off;
            pre = (float *)ar.take(n * Cout * 4);
            r[REC_MEAN] = ar.off;
            mean = (float *)ar.take(Cout * 4);
            r[REC_INVSTD] = ar.off;
            invstd = (float *)ar.take(Cout * 4);
        }
        // ReLU after a residual add: the mask cannot be recomputed from the BatchNorm input alone; kept as bits
        uint32_t *bits = nullptr;
        r[REC_BITS] = 0;
        if (bn && (g_fusions & 2) && op[TO_RELU] && op[TO_RES] >= 0) {
            r[REC_BITS] = ar.off + 1;
            bits = (uint32_t *)ar.take(lidog_relu_bits_words(n, Cout) * 4);
        }
        float *rm = P<float>(c[TC_BNRM]), *rv = P<float>(c[TC_BNRV]);
        double *sums = nullptr;
        if (bn) sums = sums_at ? sums_at : (double *)w.scratch->take((2 * Cout + 1) * 8);
        // local BatchNorm: the reduction's last kernel finalises mean / invstd / running statistics; SyncBatchNorm:
        // sums and row count only, finalised after the all-reduce
        float *f_mean = sync ? nullptr : mean, *f_invstd = sync ? nullptr : invstd;
        float *f_rm = sync ? nullptr : rm, *f_rv = sync ? nullptr : rv;
        const float f_eps = sync ? 0.f : eps, f_mom = sync ? 0.f : mom;
        bool stats_done = false;
        const int32_t *nbr = P<const int32_t>(m[TM_NBR]), *perm = P<const int32_t>(m[TM_PERM]);
        const uint32_t *wmask = P<const uint32_t>(m[TM_WMASK]);
        const int32_t *order = P<const int32_t>(m[TM_ORDER]);
        const bool os = kind == KIND_K3 && takes_os(m, Cin, Cout);
        if (os && bn) {
            double *ws = (double *)w.scratch->take(lidog_sconv_os_stats_ws(n, Cout) * 8);
            if (in_bn)
                TRY(lidog_sconv_os_stats_in_bn(in_bn->pre, nbr, n, K, perm, wmask, order, W, bias, Cin, Cout, pre, sums, ws,
                                               (double)n, f_eps, f_mom, f_mean, f_invstd, f_rm, f_rv, in_bn->mean,
                                               in_bn->invstd, in_bn->w, in_bn->b, 1, w.stream));
            else
                TRY(lidog_sconv_os_stats(x, nbr, n, K, perm, wmask, order, W, bias, Cin, Cout, pre, sums, ws, (double)n,
                                         f_eps, f_mom, f_mean, f_invstd, f_rm, f_rv, w.stream));
            stats_done = true;
            work_os(ctx, n, Cin, Cout, K, 0);
        } else if (os) {
            TRY(lidog_sconv_os(x, nbr, n, K, perm, wmask, order, W, 0, bias, nullptr, Cin, Cout, pre, w.stream));
        } else if (kind == KIND_K3 || kind == KIND_DOWN) {
            // gathered GEMM into product rows, per-row reduction (+ BatchNorm statistics in its epilogue)
            float *T = (float *)w.scratch->take(m[TM_P] * Cout * 4);
            if (int rc = gemm(ctx, m, x, n_in, P<const int32_t>(m[TM_PAIR_IN]), W, nullptr, Cin, Cout, T, nullptr,
                              w.stream, kind == KIND_K3 ? in_bn : nullptr))
                return rc;
            const int32_t *rp = P<const int32_t>(m[TM_RP_OUT]), *rl = P<const int32_t>(m[TM_RL_OUT]);
            if (bn) {
                double *ws = (double *)w.scratch->take(lidog_sconv_reduce_stats_ws(n, Cout) * 8);
                TRY(lidog_sconv_reduce_rows_stats(T, rp, rl, n, Cout, bias, pre, sums, ws, (double)n, f_eps, f_mom, f_mean,
                                                  f_invstd, f_rm, f_rv, w.stream));
                stats_done = true;
            } else {
                TRY(lidog_sconv_reduce_rows(T, rp, rl, n, Cout, bias, nullptr, pre, w.stream));
            }
            work_reduce(ctx, m, n, Cout, false);
        } else if (kind == KIND_UP) {
            // transposed 2^3 stride 2: every fine row has exactly one pair, the GEMM scatters straight into the output
            if (int rc = gemm(ctx, m, x, n_in, P<const int32_t>(m[TM_PAIR_OUT]), W, bias, Cin, Cout, pre,
                              P<const int32_t>(m[TM_PAIR_IN]), w.stream))
                return rc;
        } else if (kind == KIND_1X1) {
            RUN(gemm(ctx, m, x, n_in, nullptr, W, bias, Cin, Cout, pre, nullptr, w.stream));
        } else {
            TRY(lidog_sconv_cin1(x, nbr, W, bias, n, K, Cout, pre, w.stream));
        }
        if (bn && !stats_done) {
            int64_t wsn = lidog_bn_reduce_ws(Cout, 1);
            double *ws = wsn ? (double *)w.scratch->take(wsn * 8) : nullptr;
            TRY(lidog_bn_stats(pre, n, Cout, 1, sums, ws, (double)n, f_eps, f_mom, f_mean, f_invstd, f_rm, f_rv, w.stream));
        }
        pd = Pending{o, op, c, pre, mean, invstd, y, bits, sums, n, Cout, eps, mom};
        return 0;
    }

    int bn(const Pending &pd, Where w) {
        const int64_t *op = pd.op, *c = pd.c;
        const float *res = op[TO_RES] >= 0 ? bp[op[TO_RES]] : nullptr;
        if (res)                                         // the residual branch was made on the lane
            RUN(join(op[TO_RES], w));
        const float *bnw = P<const float>(c[TC_BNW]), *bnb = P<const float>(c[TC_BNB]);
        float *rm = P<float>(c[TC_BNRM]), *rv = P<float>(c[TC_BNRV]);
        if (in_bn_reader(ctx, pd.o) >= 0) {
            // no apply pass: the one reader of this output normalises the raw rows as it gathers them.  SyncBatchNorm:
            // mean / invstd / running statistics from the all-reduced sums (the apply pass would have derived them)
            if (sync) TRY(lidog_bn_finalize(pd.sums, -1.0, pd.Cout, pd.eps, pd.mom, pd.mean, pd.invstd, rm, rv, w.stream));
            lazy[op[TO_OUT]] = InBnArgs{pd.pre, pd.mean, pd.invstd, bnw, bnb};
            return 0;
        }
        if (sync) {   // mean / invstd / running statistics from the all-reduced sums (global count behind them) + the apply
                      // pass, one launch
            TRY(lidog_bn_apply_sync(pd.pre, pd.n, pd.Cout, pd.sums, pd.eps, pd.mom, pd.mean, pd.invstd, rm, rv, bnw, bnb,
                                    res, (int32_t)op[TO_RELU], pd.y, pd.bits, w.stream));
            return 0;
        }
        TRY(lidog_bn_apply_bits(pd.pre, pd.n, pd.Cout, 1, pd.mean, pd.invstd, bnw, bnb, res, (int32_t)op[TO_RELU], pd.y,
                                pd.bits, w.stream));
        return 0;
    }

    // conv1 of a layer's first block (op o) together with the block's downsample branch (op o + 1, branch_follows).
    // The 1x1 downsample convolution + BatchNorm reads the block input and is read again only by the residual add behind
    // conv2.  on_lane: it runs on the second stream (idle in the forward pass), next to conv1 / conv2 of its block, and
    // is issued before conv1; else it follows conv1 on the launch stream.  sync: the statistics of both travel in one
    // message.  Both: the branch's convolution + statistics on the lane next to conv1's, the joint message all-reduced ON
    // THE LAUNCH STREAM as before (the order of the collectives does not change), its apply pass back on the lane behind
    // the all-reduce.  The message then lives in the arena (the lane still reads its half after the launch stream's next
    // op has recycled the per-op scratch).  With neither, the two are plain ops of run().
    int conv1_and_branch(int o, bool on_lane) {
        const int64_t *op = ctx.op(o), *nx = ctx.op(o + 1);
        const int Ca = (int)ctx.conv(op)[TC_COUT], Cd = (int)ctx.conv(nx)[TC_COUT];
        const Where here = on_stream(), br = on_lane ? Where{lane, &ar} : here;
        double *msg = sync ? (double *)br.scratch->take((int64_t)(2 * Ca + 1 + 2 * Cd + 1) * 8) : nullptr;
        double *msg2 = sync ? msg + 2 * Ca + 1 : nullptr;
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        Pending pd, pd2;
        auto branch_bn = [&]() -> int {      // the branch's apply pass; its output is complete behind ev[3] on the lane
            RUN(bn(pd2, br));
            if (!on_lane) return 0;
            RUN(ev_record(ctx, ev[3], lane));
            join_of[nx[TO_OUT]] = ev[3];
            return 0;
        };
        if (on_lane) {
            RUN(side_events(ev));
            RUN(ev_order(ctx, stream, ev[0], lane));
            ++n_side;
            RUN(conv(o + 1, msg2, br, pd2));
            RUN(sync ? ev_record(ctx, ev[1], lane) : branch_bn());
        }
        RUN(conv(o, msg, here, pd));
        if (!on_lane) RUN(conv(o + 1, msg2, here, pd2));
        if (sync) {
            if (on_lane) RUN(ev_wait(ctx, stream, ev[1]));
            TRY(dp.allreduce_f64(msg, 2 * Ca + 1 + 2 * Cd + 1, stream));
            if (on_lane) RUN(ev_order(ctx, stream, ev[2], lane));
        }
        RUN(bn(pd, here));
        return sync ? branch_bn() : 0;
    }

    int run() {
        for (int o = 0; o < ctx.n_ops; ++o) {
            const int64_t *op = ctx.op(o);
            sc.reset();
            if (op[TO_TYPE] == OP_CAT) {
                int a = (int)op[TO_IN], b = (int)op[TO_B];
                TRY(lidog_cat2(bp[a], ctx.ch(a), bp[b], ctx.ch(b), ctx.rows(a), bp[op[TO_OUT]], stream));
                continue;
            }
            if (branch_follows(ctx, o)) {
                // under SyncBatchNorm the branch's statistics travel in conv1's message, on the lane or not; with local
                // BatchNorm the pair is special only when the branch goes to the lane
                const bool on_lane = lane && g_side_forward && ctx.op(o + 1)[TO_RES] < 0 && n_side < MAX_SIDE;
                if (sync || on_lane) {
                    RUN(conv1_and_branch(o, on_lane));
                    ++o;     // the downsample op has been done
                    continue;
                }
            }
            Pending pd;
            RUN(conv(o, nullptr, on_stream(), pd));
            if (op[TO_TYPE] != OP_CONVBN) continue;
            if (sync) TRY(dp.allreduce_f64(pd.sums, 2 * pd.Cout + 1, stream));
            RUN(bn(pd, on_stream()));
        }
        // nothing made on the lane is left unjoined (every downsample output is a residual above; belt and braces)
        for (int b = 0; b < ctx.n_bufs; ++b)
            if (join_of[b]) RUN(ev_wait(ctx, stream, join_of[b]));
        return 0;
    }
};

}  // namespace

// Forward pass.  rec [n_ops * 4 + n_bufs]: arena offsets of what backward needs (filled here, opaque to the caller).
// need [2]: bytes of arena / scratch this batch takes (always filled; with dry != 0 nothing is launched).
extern "C" int lidog_trunk_forward(const int64_t *convs, const double *conv_f, int32_t n_convs, const int64_t *maps,
                                   int32_t n_maps, const int64_t *ops, int32_t n_ops, const int64_t *bufs,
                                   int32_t n_bufs, const int64_t *level_rows, const int64_t *ext, void *arena,
                                   int64_t arena_bytes, void *scratch, int64_t scratch_bytes, int64_t *rec,
                                   int64_t *need, int32_t dry, const int64_t *dp_desc, void *stream, void *lane) {
    Ctx ctx{convs, conv_f, n_convs, maps, n_maps, ops, n_ops, bufs, n_bufs, level_rows, ext, dry != 0};
    Dp dp{dp_desc};
    RUN(check_tables(ctx, false));
    RUN(dp.check());
    if (!ctx.dry) {
        // sizes first: nothing is launched into an arena that is too small
        int64_t want[2];
        if (int rc = lidog_trunk_forward(convs, conv_f, n_convs, maps, n_maps, ops, n_ops, bufs, n_bufs, level_rows,
                                         ext, nullptr, 0, nullptr, 0, rec, want, 1, dp_desc, stream, lane))
            return rc;
        LIDOG_REQUIRE(arena && scratch && want[0] <= arena_bytes && want[1] <= scratch_bytes,
                      "trunk: forward needs %lld B of arena and %lld B of scratch, got %lld / %lld", (long long)want[0],
                      (long long)want[1], (long long)arena_bytes, (long long)scratch_bytes);
    }
    Forward fw(ctx, dp, rec, Bump{(char *)arena, 0, arena_bytes, 0, ctx.dry},
               Bump{(char *)scratch, 0, scratch_bytes, 0, ctx.dry}, stream, lane);
    if (!ctx.dry && dp.sync_bn()) RUN(dp.bind(stream));
    RUN(fw.place_buffers());
    RUN(fw.run());
    need[0] = fw.ar.peak;
    need[1] = fw.sc.peak;
    return 0;
}

namespace {

// the data gradients' gathered GEMMs run next to the lane's weight gradients: one unit per workgroup there
// (sconv_mfma.hip:lidog_gemm_multi_suspend)
struct MultiUnitGuard {
    bool on;
    explicit MultiUnitGuard(bool o) : on(o) { if (on) lidog_gemm_multi_suspend(1); }
    ~MultiUnitGuard() { if (on) lidog_gemm_multi_suspend(-1); }
};

// what the forward pass kept of a BatchNorm (rec, arena, convolution table)
struct SavedBn {
    const float *pre, *mean, *invstd;   // the raw convolution output and its statistics
    const uint32_t *bits;               // the ReLU mask as bits (fusion 2), or NULL
    const float *ymask;                 // else the saved output, where the mask cannot be recomputed from `pre`
    bool from_x;                        // ReLU without residual: mask recomputed from `pre`, weight and bias
    const float *w, *b;
    const float *fx_w() const { return from_x ? w : nullptr; }
    const float *fx_b() const { return from_x ? b : nullptr; }
};

// ---- the backward pass, step by step
struct Backward {
    const Ctx &ctx;
    const Dp &dp;
    const int64_t *ext_grad, *rec;
    void *arena;
    Bump ga, sc, ls;
    void *stream, *lane;
    int32_t *conv_done;
    const bool wgrad_first, sync, buckets;
    const int n_buckets;
    hipEvent_t *events = nullptr;
    int lane_used = 0;
    std::vector<float *> bp;
    // gradient slot of every buffer: 0 = nothing yet, 1 = the caller's tensor (read only), 2 = ours (garena)
    std::vector<float *> gp;
    std::vector<int> gs;
    // producer of every buffer and its first consumer in forward order = the LAST one to add to its gradient here
    std::vector<int> producer, first_consumer;
    // BatchNorm-backward sums of op o already produced by the reduction that completed its output gradient
    std::vector<double *> bwd_sums;
    // Accumulate mode (TC_ACC, the second backward pass over a model called twice before one backward: the optimiser's
    // slices already hold the first pass's gradients): this pass's parameter gradients go to garena and one
    // lidog_grad_accumulate per convolution and stream adds them into the slices -- the kernel gradient behind its
    // weight-gradient kernel on the lane (which, in stream order, also holds whatever the first pass still writes there),
    // bias and BatchNorm gradients on the launch stream -- before param_done counts the convolution down.  No side
    // branch then: its BatchNorm gradients would be added on a third stream the buckets do not watch.
    bool accumulate = false;
    std::vector<float *> acc_src;
    std::vector<int64_t> acc_segs;
    // Side branch: the downsample convolution of a layer's first block (1x1 + BatchNorm, no ReLU; its output is only the
    // residual of conv2's BatchNorm) has its backward -- BatchNorm reduce + apply, 1x1 data gradient -- on a third stream,
    // from the moment conv2's BatchNorm backward has written the residual's gradient until conv1's data gradient adds the
    // branch's contribution to the block input's gradient.  Under SyncBatchNorm the branch's statistics message is still
    // all-reduced ON THE LAUNCH STREAM, at the op's place in the order: the launch stream waits for the branch's reduction
    // (long finished: conv2's data gradient was queued in between), the branch's apply pass waits for the all-reduce.
    // Gradient buckets watch the launch stream and the lane only; that covers a side op's parameter gradients when the
    // launch stream has waited for its reduction (SyncBatchNorm), not otherwise (local BatchNorm + buckets: in line).
    // Same kernels, same arguments: same bits.
    bool side_on = false;
    hipStream_t side_st = nullptr;
    hipEvent_t *side_ev = nullptr;
    int n_side = 0;
    std::vector<int> is_side;
    std::vector<hipEvent_t> res_ready, join_evt;
    std::vector<char> res_ok;     // the buffer's gradient is one residual gradient (decided alike in dry runs)
    hipEvent_t side_last = nullptr;

    // one convolution (+ BatchNorm) op on its way through the steps below
    struct Op {
        int o;
        const int64_t *op, *c, *m;
        int kind, Cin, Cout, K, in_b, out_b;
        int64_t n, n_in;
        bool side;                      // runs on the side stream
        Where w;                        // the launch stream and the per-op scratch, or the side stream and garena
        const float *gout;              // gradient of the convolution's output
        bool has_in_bn;                 // input normalised on the fly in the forward pass (fusion 4) ...
        SavedBn in_bn;                  // ... from this record of its producer
        const int32_t *g_in, *g_out;    // pair lists of the input / output side
        bool wgrad_done;
        void *wgrad_st;
        // data gradient between its matrix kernel and its reduction / commit
        enum { DIRECT, OS, TWO_PASS } route;
        float *gx, *T;
        bool folds;
    };

    Backward(const Ctx &c, const Dp &d, const int64_t *ext_grad_, void *arena_, const int64_t *rec_, Bump garena,
             Bump scratch, Bump lane_scratch, int32_t *conv_done_, bool wgrad_first_, void *stream_, void *lane_)
        : ctx(c), dp(d), ext_grad(ext_grad_), rec(rec_), arena(arena_), ga(garena), sc(scratch), ls(lane_scratch),
          stream(stream_), lane(lane_), conv_done(conv_done_), wgrad_first(wgrad_first_), sync(d.sync_bn()),
          buckets(d.buckets() && !c.dry), n_buckets(buckets ? (int)d.d[DP_N_BUCKETS] : 0), bp(c.n_bufs, nullptr),
          gp(c.n_bufs, nullptr), gs(c.n_bufs, 0), producer(c.n_bufs, -1), first_consumer(c.n_bufs, c.n_ops),
          bwd_sums(c.n_ops, nullptr), acc_src((size_t)c.n_convs * 4, nullptr), is_side(c.n_ops, 0),
          res_ready(c.n_bufs, nullptr), join_evt(c.n_bufs, nullptr), res_ok(c.n_bufs, 0) {}

    int setup() {
        const int n_convs = ctx.n_convs, n_ops = ctx.n_ops;
        if ((lane || buckets) && !ctx.dry) {
            // [0, n_convs): lane forks; n_convs: the final join; then two per gradient bucket (main / lane -> bucket stream)
            LIDOG_REQUIRE(n_convs + 1 + 2 * n_buckets < SIDE_EVENT0,
                          "trunk: %d convolutions + %d gradient buckets need more events than the %d in front of the side streams' range",
                          n_convs, n_buckets, (int)SIDE_EVENT0);
            events = event_pool(n_convs + 1 + 2 * n_buckets);
            LIDOG_REQUIRE(events, "trunk: cannot create events");
        }
        const int64_t *buf_off = rec + (int64_t)n_ops * REC_COLS;
        for (int b = 0; b < ctx.n_bufs; ++b) {
            int64_t e = ctx.ext_of(b);
            if (e >= 0) {
                bp[b] = P<float>(ctx.ext[e]);
                if (ext_grad[e]) {
                    gp[b] = P<float>(ext_grad[e]);
                    gs[b] = 1;
                }
            } else {
                bp[b] = ctx.dry ? (float *)(uintptr_t)4096 : (float *)((char *)arena + buf_off[b]);
            }
        }
        for (int i = 0; i < n_convs; ++i) conv_done[i] = 0;
        for (int o = n_ops - 1; o >= 0; --o) {
            const int64_t *op = ctx.op(o);
            producer[op[TO_OUT]] = o;
            first_consumer[op[TO_IN]] = o;
            if (op[TO_TYPE] == OP_CAT) first_consumer[op[TO_B]] = o;
            if (op[TO_TYPE] == OP_CONVBN && op[TO_RES] >= 0) first_consumer[op[TO_RES]] = o;
        }
        for (int i = 0; i < n_convs; ++i) accumulate = accumulate || ctx.convs[(int64_t)i * TC_COLS + TC_ACC] != 0;
        side_on = g_side_backward && lane && (sync || !dp.buckets()) && !accumulate;
        if (side_on)
            for (int o = 1; o < n_ops; ++o) {
                const int64_t *op = ctx.op(o);
                if (branch_follows(ctx, o - 1) && op[TO_RES] < 0 && !op[TO_RELU] && ctx.ext_of(op[TO_OUT]) < 0 &&
                    ctx.ext_of(op[TO_IN]) != 0)
                    is_side[o] = 1;
            }
        return 0;
    }

    // A gradient bucket (a contiguous slice of the flat gradient buffer, lidog_amd.optim.GradientBuckets) is reduced as
    // soon as the last gradient of its parameters has been QUEUED: the bucket stream waits for what the launch stream
    // and the lane stream hold at that moment, nothing ever waits for the bucket stream here (the caller joins it
    // before the optimiser step).  pending[b] is shared with the caller, whose own parameters (the 2-D head) count
    // down in the same array from their gradient hooks.
    int param_done(int64_t conv, int slot) {
        if (!buckets) return 0;
        const int b = P<const int32_t>(dp.d[DP_PARAM_BUCKET])[conv * 4 + slot];
        if (b < 0) return 0;
        LIDOG_REQUIRE(b < n_buckets, "trunk: parameter of convolution %lld in bucket %d of %d", (long long)conv, b, n_buckets);
        int32_t *pending = P<int32_t>(dp.d[DP_PENDING]);
        if (--pending[b] != 0) return 0;
        if (!dp.d[DP_COMM_GRAD]) {
            int rc = reinterpret_cast<dp_callback_t>(static_cast<uintptr_t>(dp.d[DP_CALLBACK]))(1, b, 0);
            LIDOG_REQUIRE(rc == 0, "trunk: the gradient bucket callback failed (%d)", rc);
            return 0;
        }
        void *cst = P<void>(dp.d[DP_COMM_STREAM]);
        RUN(ev_order(ctx, stream, events[ctx.n_convs + 1 + 2 * b], cst));
        if (lane)   // every bucket waits for the lane as it stands: stream order then covers all earlier weight gradients
            RUN(ev_order(ctx, lane, events[ctx.n_convs + 2 + 2 * b], cst));
        const int64_t *sl = P<const int64_t>(dp.d[DP_BUCKETS]) + 2 * b;
        return lidog_allreduce_f32(P<float>(dp.d[DP_GRAD_BASE]) + sl[0], sl[1] - sl[0], P<void>(dp.d[DP_COMM_GRAD]), cst);
    }

    // where a producer writes its contribution to buffer b's gradient, and what happens once it is queued
    float *target(int b) { return (float *)ga.take(ctx.bytes(b)); }
    int commit(int b, float *p) {
        if (gs[b] != 0) {
            float *dst = gs[b] == 2 ? gp[b] : (float *)ga.take(ctx.bytes(b));
            TRY(lidog_add(gp[b], p, ctx.rows(b) * ctx.ch(b), dst, stream));
            p = dst;
        }
        replace(b, p);
        return 0;
    }
    void replace(int b, float *p) {      // p holds the whole gradient of buffer b (what was there entered as an addend)
        gp[b] = p;
        gs[b] = 2;
    }

    // where parameter gradient `slot` (table column `col`) of a convolution is written: its slice, or in accumulate
    // mode a garena copy that add_seg / flush_segs add into the slice
    float *grad_out(int64_t conv, int slot, int col, int64_t count) {
        const int64_t *cc = ctx.convs + conv * TC_COLS;
        if (!cc[TC_ACC]) return P<float>(cc[col]);
        float *&p = acc_src[conv * 4 + slot];
        if (!p) {   // the same alignment mod 16 as the destination: the float4 path of the add applies to both
            char *b = (char *)ga.take(count * 4 + 16);
            p = (float *)(b + (((uintptr_t)cc[col] - (uintptr_t)b) & 15));
        }
        return p;
    }
    void add_seg(int64_t conv, int slot, int col, int64_t count) {
        const float *src = acc_src[conv * 4 + slot];
        if (!src) return;
        acc_segs.push_back(ctx.convs[conv * TC_COLS + col]);
        acc_segs.push_back((int64_t)(uintptr_t)src);
        acc_segs.push_back(count);
    }
    int flush_segs(void *st) {
        if (acc_segs.empty() || ctx.dry) { acc_segs.clear(); return 0; }
        const int rc = lidog_grad_accumulate(acc_segs.data(), (int32_t)(acc_segs.size() / 3), st);
        acc_segs.clear();
        return rc;
    }

    // the side stream and the pool's range of side events, created on first use; dry mode: neither
    int side_open() {
        if (ctx.dry || side_ev) return 0;
        side_st = side_stream();
        side_ev = event_pool(SIDE_BWD_EVENT0 + 4 * MAX_SIDE);
        LIDOG_REQUIRE(side_st && side_ev, "trunk: cannot create the side stream");
        side_ev += SIDE_BWD_EVENT0;
        return 0;
    }
    // event k of the current side branch: 0 residual gradient ready, 1 branch done, 2 statistics ready, 3 all-reduce done
    hipEvent_t side_event(int k) const { return side_ev ? side_ev[4 * n_side + k] : nullptr; }
    int join_side(int b) {      // the launch stream is about to read what the side branch wrote for buffer b
        if (join_evt[b]) RUN(ev_wait(ctx, stream, join_evt[b]));
        join_evt[b] = nullptr;
        return 0;
    }

    SavedBn saved_bn(int o) const {
        const int64_t *op = ctx.op(o), *c = ctx.conv(op), *r = rec + (int64_t)o * REC_COLS;
        auto kept = [&](int64_t off) {      // dry runs: a placeholder that is never read
            return ctx.dry ? (const char *)(uintptr_t)4096 : (const char *)arena + off;
        };
        const bool relu = op[TO_RELU] != 0, from_x = relu && op[TO_RES] < 0;   // Cout % 4 == 0: check_tables
        return SavedBn{(const float *)kept(r[REC_PRE]), (const float *)kept(r[REC_MEAN]), (const float *)kept(r[REC_INVSTD]),
                       (!ctx.dry && r[REC_BITS]) ? (const uint32_t *)kept(r[REC_BITS] - 1) : nullptr,
                       (relu && !from_x && !r[REC_BITS]) ? bp[op[TO_OUT]] : nullptr, from_x,
                       P<const float>(c[TC_BNW]), P<const float>(c[TC_BNB])};
    }

    int cat_split(const int64_t *op) {
        const int a = (int)op[TO_IN], b = (int)op[TO_B];
        float *ga_ = target(a), *gb_ = target(b);
        TRY(lidog_split2(gp[op[TO_OUT]], ctx.ch(a), ctx.ch(b), ctx.rows(a), ga_, gb_, stream));
        RUN(commit(a, ga_));
        return commit(b, gb_);
    }

    // BatchNorm backward (me._BatchNormFn.backward): reduce (unless the sums came with the output gradient), the
    // SyncBatchNorm all-reduce, apply; q.gout becomes the gradient of the convolution output
    int bn_backward(Op &q) {
        const int64_t *op = q.op;
        const SavedBn s = saved_bn(q.o);
        const int Cout = q.Cout;
        const int64_t n = q.n;
        const bool has_res = op[TO_RES] >= 0;
        double *sums = bwd_sums[q.o];
        if (!sums) {
            sums = (double *)q.w.scratch->take((2 * Cout + 1) * 8);
            int64_t wsn = lidog_bn_reduce_ws(Cout, 1);
            double *ws = wsn ? (double *)q.w.scratch->take(wsn * 8) : nullptr;
            float *g_w = grad_out(op[TO_CONV], 2, TC_GBNW, Cout), *g_b = grad_out(op[TO_CONV], 3, TC_GBNB, Cout);
            TRY(lidog_bn_bwd_reduce_bits(q.gout, s.pre, s.ymask, s.bits, n, Cout, 1, s.mean, s.invstd, sums, ws, (double)n,
                                         g_w, g_b, s.fx_w(), s.fx_b(), q.w.stream));
        }
        float *dx = (float *)ga.take(n * Cout * 4);
        float *dres = has_res ? target((int)op[TO_RES]) : nullptr;
        // SyncBatchNorm: (sum dy', sum dy' xhat, rows) summed over the ranks; the apply kernel reads the global count.
        // A side op's message: the launch stream waits for the reduction, the side stream for the all-reduce
        if (sync) {
            if (q.side) RUN(ev_order(ctx, side_st, side_event(2), stream));
            TRY(dp.allreduce_f64(sums, 2 * Cout + 1, stream));
            if (q.side) RUN(ev_order(ctx, stream, side_event(3), side_st));
        }
        TRY(lidog_bn_bwd_apply_bits(q.gout, s.pre, s.ymask, s.bits, n, Cout, 1, s.mean, s.invstd, s.w, sums,
                                    sync ? -1.0 : (double)n, dx, dres, nullptr, nullptr, s.fx_b(), q.w.stream));
        if (has_res) {
            const int rb = (int)op[TO_RES];
            const bool first = gs[rb] == 0;
            RUN(commit(rb, dres));
            // the residual branch may start now (if it is a side branch and this was its whole gradient)
            if (side_on && first && producer[rb] >= 0 && is_side[producer[rb]] && n_side < MAX_SIDE) res_ok[rb] = 1;
            if (res_ok[rb]) {
                RUN(side_open());
                res_ready[rb] = side_event(0);
                RUN(ev_record(ctx, res_ready[rb], stream));
            }
        }
        q.gout = dx;
        return 0;
    }

    // weight gradient: on the lane behind an event of the op's stream, or in line
    int wgrad(Op &q) {
        const int64_t *c = q.c;
        const int Cin = q.Cin, Cout = q.Cout, K = q.K;
        q.wgrad_done = true;
        const int n_items = (int)c[TC_NITEMS];
        int slabs = lidog_sconv_wgrad_slabs(Cin, Cout, n_items);
        int64_t pbytes = (int64_t)(slabs > 1 ? slabs : 1) * Cin * Cout * 4;
        float *partial;
        void *st = q.w.stream;
        if (lane) {
            ls.reset();
            partial = (float *)ls.take(pbytes);
            RUN(ev_order(ctx, q.w.stream, events ? events[q.op[TO_CONV]] : nullptr, lane));
            st = lane;
            lane_used = 1;
        } else {
            partial = (float *)q.w.scratch->take(pbytes);
        }
        float *gw_out = grad_out(q.op[TO_CONV], 0, TC_GW, (int64_t)K * Cin * Cout);
        q.wgrad_st = st;
        const int32_t *items = P<const int32_t>(c[TC_ITEMS]), *item_off = P<const int32_t>(c[TC_ITEMOFF]);
        if (q.has_in_bn)
            TRY(lidog_sconv_wgrad_in_bn(q.in_bn.pre, q.g_in, q.gout, q.g_out, items, n_items, item_off, K, Cin, Cout, partial,
                                        gw_out, q.in_bn.mean, q.in_bn.invstd, q.in_bn.w, q.in_bn.b, 1, st));
        else
            TRY(lidog_sconv_wgrad(bp[q.in_b], q.g_in, q.gout, q.g_out, items, n_items, item_off, K, Cin, Cout, partial,
                                  gw_out, st));
        work_wgrad(ctx, q.m, Cin, Cout, K, slabs);
        return 0;
    }

    // the classifier's data gradient on rows that already hold a gradient (the BEV head's): product and sum
    // in one pass, the bits of the product pass followed by commit()'s lidog_add
    int dgrad_1x1_addend(Op &q, const float *Wt) {
        const int64_t *m = q.m;
        float *dst = gs[q.in_b] == 2 ? gp[q.in_b] : (float *)ga.take(ctx.bytes(q.in_b));
        TRY(lidog_sconv_gemm_addend(q.gout, nullptr, Wt, tile_row(m, 0), tile_row(m, 1), tile_row(m, 2),
                                    (int32_t)m[TM_NTILES], q.Cout, q.Cin, gp[q.in_b], dst, nullptr, q.w.stream));
        replace(q.in_b, dst);
        return 0;
    }
    int dgrad_1x1(Op &q, const float *Wt) {
        float *gx = target(q.in_b);
        RUN(gemm(ctx, q.m, q.gout, q.n, nullptr, Wt, nullptr, q.Cout, q.Cin, gx, nullptr, q.w.stream));
        RUN(commit(q.in_b, gx));
        if (q.side && !ctx.dry) {
            join_evt[q.in_b] = side_last = side_event(1);
            RUN(ev_record(ctx, side_last, side_st));
        }
        return 0;
    }
    // every fine (input) row has exactly one pair: the GEMM scatters straight into the gradient
    int dgrad_down(Op &q, const float *Wt) {
        float *gx = target(q.in_b);
        RUN(gemm(ctx, q.m, q.gout, q.n, q.g_out, Wt, nullptr, q.Cout, q.Cin, gx, q.g_in, stream));
        return commit(q.in_b, gx);
    }
    // output-stationary data gradient over the mirrored offsets of the map's sorted rows; what reached the
    // input buffer earlier (the residual branch of a block) is added in its epilogue, as the reduction pass
    // does.  The BatchNorm-backward sums of the producing layer then come from the stand-alone reduction
    // (the operator path's kernel: the same bits).
    int dgrad_os(Op &q, const float *Wt) {
        const int64_t *m = q.m;
        q.gx = target(q.in_b);
        TRY(lidog_sconv_os(q.gout, P<const int32_t>(m[TM_NBR]), q.n_in, q.K, P<const int32_t>(m[TM_PERM]),
                           P<const uint32_t>(m[TM_WMASK]), P<const int32_t>(m[TM_ORDER]), Wt, 1, nullptr,
                           q.folds ? gp[q.in_b] : nullptr, q.Cout, q.Cin, q.gx, stream));
        work_os(ctx, q.n_in, q.Cin, q.Cout, q.K, q.folds ? q.Cin : 0);
        return 0;
    }

    // First half of the data gradient: up to its matrix kernel.  For the direct kinds (1x1, 2^3 stride 2: the GEMM writes
    // the gradient rows themselves) that is all of it; the other two leave q.route / q.gx / q.T for dgrad_finish.
    int dgrad_matrix(Op &q, const float *Wt) {
        q.route = Op::DIRECT;
        if (q.kind == KIND_1X1 && q.Cout <= 8 && q.Cin % 4 == 0 && gs[q.in_b] != 0) return dgrad_1x1_addend(q, Wt);
        if (q.kind == KIND_1X1) return dgrad_1x1(q, Wt);
        if (q.kind == KIND_DOWN) return dgrad_down(q, Wt);
        q.folds = q.op[TO_FOLD] && gs[q.in_b] != 0;
        if (q.kind == KIND_K3 && takes_os(q.m, q.Cin, q.Cout)) {
            q.route = Op::OS;
            return dgrad_os(q, Wt);
        }
        q.route = Op::TWO_PASS;
        q.T = (float *)sc.take(q.m[TM_P] * q.Cin * 4);
        return gemm(ctx, q.m, q.gout, q.n, q.g_out, Wt, nullptr, q.Cout, q.Cin, q.T, nullptr, stream);
    }

    // Second half: the per-row reduction of the product rows, with one of three epilogues
    int dgrad_reduce(Op &q) {
        const int64_t *m = q.m;
        const int in_b = q.in_b, Cin = q.Cin;
        const int64_t n_in = q.n_in;
        // K3: rows of the input side; UP: the coarse rows are the map's OUTPUT side
        const int32_t *rp = P<const int32_t>(q.kind == KIND_UP ? m[TM_RP_OUT] : m[TM_RP_IN]);
        const int32_t *rl = P<const int32_t>(q.kind == KIND_UP ? m[TM_RL_OUT] : m[TM_RL_IN]);
        float *gx = target(in_b);
        // This reduction completes the gradient of in_b when nothing reaches that buffer after it: it is the
        // buffer's first consumer in forward order, and whatever arrived before is either absent or enters
        // as the addend.  If a BatchNorm produced the buffer, its backward sums ride in the epilogue.
        const int po = producer[in_b];
        const bool bwdstats = (g_fusions & 1) && po >= 0 && ctx.op(po)[TO_TYPE] == OP_CONVBN && first_consumer[in_b] == q.o &&
                              (q.folds || gs[in_b] == 0) && Cin % 4 == 0 && Cin / 4 <= 256;
        if (bwdstats) {
            const int64_t pconv = ctx.op(po)[TO_CONV];
            const SavedBn p = saved_bn(po);
            double *sums = (double *)ga.take((2 * Cin + 1) * 8);   // lives until the producer's turn
            double *ws = (double *)sc.take(lidog_bn_reduce_ws(Cin, 1) * 8);
            float *pg_w = grad_out(pconv, 2, TC_GBNW, Cin), *pg_b = grad_out(pconv, 3, TC_GBNB, Cin);
            TRY(lidog_sconv_reduce_rows_bwdstats(q.T, rp, rl, n_in, Cin, q.folds ? gp[in_b] : nullptr, gx, p.pre, p.ymask,
                                                 p.bits, p.mean, p.invstd, p.fx_w(), p.fx_b(), sums, ws, (double)n_in, pg_w,
                                                 pg_b, stream));
            bwd_sums[po] = sums;
            replace(in_b, gx);
        } else if (q.folds) {
            // the residual branch's gradient of the block input enters the sum in the reduction's epilogue
            TRY(lidog_sconv_reduce_rows(q.T, rp, rl, n_in, Cin, nullptr, gp[in_b], gx, stream));
            replace(in_b, gx);
        } else {
            TRY(lidog_sconv_reduce_rows(q.T, rp, rl, n_in, Cin, nullptr, nullptr, gx, stream));
            RUN(commit(in_b, gx));
        }
        work_reduce(ctx, m, n_in, Cin, bwdstats);
        return 0;
    }
    int dgrad_finish(Op &q) {
        if (q.route == Op::TWO_PASS) return dgrad_reduce(q);
        if (q.route == Op::OS) {
            if (!q.folds) return commit(q.in_b, q.gx);
            replace(q.in_b, q.gx);
        }
        return 0;
    }

    // convolution backward (me._SparseConvFn.backward): weight gradient and data gradient
    int conv_backward(Op &q) {
        const int64_t *c = q.c, *m = q.m;
        // input normalised on the fly in the forward pass (fusion 4): the weight gradient does the same from the
        // producer's raw output
        const int po = producer[q.in_b];
        q.has_in_bn = po >= 0 && in_bn_reader(ctx, po) == q.o;
        if (q.has_in_bn) q.in_bn = saved_bn(po);
        if (q.kind == KIND_1X1) {
            q.g_in = q.g_out = P<const int32_t>(m[TM_IDENT]);
        } else {
            q.g_in = P<const int32_t>(m[q.kind == KIND_UP ? TM_PAIR_OUT : TM_PAIR_IN]);
            q.g_out = P<const int32_t>(m[q.kind == KIND_UP ? TM_PAIR_IN : TM_PAIR_OUT]);
        }
        q.wgrad_done = false;
        q.wgrad_st = q.w.stream;
        // with a lane, the weight gradient is queued behind the data gradient's matrix kernel (the lane forks there),
        // unless the caller wants it first; without a data gradient or a matrix kernel of its own, behind everything
        const bool behind = lane && !wgrad_first;
        if (!behind) RUN(wgrad(q));
        const bool need_dgrad = ctx.ext_of(q.in_b) != 0 && q.kind != KIND_STEM;  // ext slot 0 = input features
        if (need_dgrad) {
            RUN(join_side(q.in_b));    // what a side branch has written to this buffer's gradient
            const float *Wt = P<const float>(c[TC_WT]);
            if (!Wt) {
                float *w = (float *)ga.take((int64_t)q.K * q.Cin * q.Cout * 4);
                TRY(lidog_transpose_kernel(P<const float>(c[TC_W]), q.K, q.Cin, q.Cout, w, q.w.stream));
                Wt = w;
            }
            RUN(dgrad_matrix(q, Wt));
            if (!q.wgrad_done && q.route != Op::DIRECT) RUN(wgrad(q));
            RUN(dgrad_finish(q));
        }
        if (!q.wgrad_done) RUN(wgrad(q));
        return 0;
    }

    int bias_grad(Op &q) {
        if (!(q.c[TC_BIAS] && q.c[TC_GBIAS])) return 0;
        double *ws = (double *)q.w.scratch->take(lidog_colsum_ws(q.Cout) * 8);
        float *g_bias = grad_out(q.op[TO_CONV], 1, TC_GBIAS, q.Cout);
        TRY(lidog_colsum(q.gout, q.n, q.Cout, g_bias, ws, q.w.stream));
        return 0;
    }

    // parameter bookkeeping once every gradient of the convolution is queued
    int params_done(Op &q) {
        const int64_t *c = q.c, conv = q.op[TO_CONV];
        const bool bias = c[TC_BIAS] && c[TC_GBIAS], bn = q.op[TO_TYPE] == OP_CONVBN;
        if (c[TC_ACC]) {   // accumulate mode: add this convolution's gradients into the optimiser's slices
            add_seg(conv, 0, TC_GW, (int64_t)q.K * q.Cin * q.Cout);
            if (q.wgrad_st != q.w.stream) RUN(flush_segs(q.wgrad_st));
            if (bias) add_seg(conv, 1, TC_GBIAS, q.Cout);
            if (bn) {
                add_seg(conv, 2, TC_GBNW, q.Cout);
                add_seg(conv, 3, TC_GBNB, q.Cout);
            }
            RUN(flush_segs(q.w.stream));
        }
        // every parameter gradient of this convolution is queued now (kernel: lane or launch stream; bias and BatchNorm
        // gains / biases: launch stream)
        if (ctx.dry) return 0;
        RUN(param_done(conv, 0));
        if (bias) RUN(param_done(conv, 1));
        if (bn) {
            RUN(param_done(conv, 2));
            RUN(param_done(conv, 3));
        }
        return 0;
    }

    int step(int o) {
        const int64_t *op = ctx.op(o);
        sc.reset();
        const int out_b = (int)op[TO_OUT], in_b = (int)op[TO_IN];
        if (gs[out_b] == 0) return 0;  // nothing reached this output: no gradients below it on this branch
        RUN(join_side(out_b));
        if (op[TO_TYPE] == OP_CAT) return cat_split(op);
        Op q;
        q.o = o;
        q.op = op;
        q.c = ctx.conv(op);
        q.m = ctx.map(q.c);
        q.kind = (int)q.c[TC_KIND], q.Cin = (int)q.c[TC_CIN], q.Cout = (int)q.c[TC_COUT], q.K = (int)q.c[TC_K];
        q.in_b = in_b, q.out_b = out_b;
        q.n = ctx.rows(out_b), q.n_in = ctx.rows(in_b);
        // this op on the side stream?  (its output gradient is exactly one BatchNorm's residual gradient, and nothing has
        // reached the block input yet: the branch is the first contributor there, no add kernel)
        q.side = is_side[o] && res_ok[out_b] && gs[in_b] == 0 && n_side < MAX_SIDE;
        q.w = Where{stream, &sc};
        if (q.side) {
            RUN(side_open());
            RUN(ev_wait(ctx, side_st, res_ready[out_b]));
            // per-op scratch is recycled by the launch stream's next op
            q.w = Where{ctx.dry ? stream : (void *)side_st, &ga};
        }
        conv_done[op[TO_CONV]] = 1;
        q.gout = gp[out_b];
        if (op[TO_TYPE] == OP_CONVBN) RUN(bn_backward(q));
        RUN(conv_backward(q));
        RUN(bias_grad(q));
        if (q.side) {
            if (!ctx.dry && !join_evt[in_b]) {   // no data gradient was asked for: still order the parameter gradients
                side_last = side_event(1);
                RUN(ev_record(ctx, side_last, side_st));
            }
            ++n_side;
        }
        return params_done(q);
    }

    // on return the launch stream has waited for the side stream and the lane
    int join_streams() {
        if (side_last) RUN(ev_wait(ctx, stream, side_last));   // BatchNorm gradients of the side ops
        if (lane_used && !ctx.dry) return ev_order(ctx, lane, events[ctx.n_convs], stream);
        return 0;
    }
};

}  // namespace

// Backward pass.  ext_grad [n_ext]: incoming gradients of the external buffers (0 = none; read only).  Parameter
// gradients are written to the gW / g_bias / g_bn_* pointers of the convolution table.  lane: second stream for the
// weight gradients (NULL = in line); wgrad_first: queue a weight gradient before its data gradient's GEMM instead of
// behind it (me._WgradLane modes 1 / 2).  On return the main stream has been made to wait for the lane.
// need [3]: bytes of garena / scratch / lane_scratch.  conv_done [n_convs] (host): 1 for every convolution whose
// parameter gradients were written (a gradient reached its output), else 0.
extern "C" int lidog_trunk_backward(const int64_t *convs, const double *conv_f, int32_t n_convs, const int64_t *maps,
                                    int32_t n_maps, const int64_t *ops, int32_t n_ops, const int64_t *bufs,
                                    int32_t n_bufs, const int64_t *level_rows, const int64_t *ext,
                                    const int64_t *ext_grad, void *arena, const int64_t *rec, void *garena,
                                    int64_t garena_bytes, void *scratch, int64_t scratch_bytes, void *lane_scratch,
                                    int64_t lane_bytes, int64_t *need, int32_t *conv_done, int32_t dry,
                                    int32_t wgrad_first, const int64_t *dp_desc, void *stream, void *lane) {
    Ctx ctx{convs, conv_f, n_convs, maps, n_maps, ops, n_ops, bufs, n_bufs, level_rows, ext, dry != 0};
    Dp dp{dp_desc};
    RUN(check_tables(ctx, true));
    RUN(dp.check());
    if (!ctx.dry) {
        int64_t want[3];
        if (int rc = lidog_trunk_backward(convs, conv_f, n_convs, maps, n_maps, ops, n_ops, bufs, n_bufs, level_rows,
                                          ext, ext_grad, arena, rec, nullptr, 0, nullptr, 0, nullptr, 0, want,
                                          conv_done, 1, wgrad_first, dp_desc, stream, lane))
            return rc;
        LIDOG_REQUIRE(arena && garena && scratch && (lane_scratch || !lane) && want[0] <= garena_bytes &&
                          want[1] <= scratch_bytes && want[2] <= lane_bytes,
                      "trunk: backward needs %lld / %lld / %lld B (gradients / scratch / lane), got %lld / %lld / %lld",
                      (long long)want[0], (long long)want[1], (long long)want[2], (long long)garena_bytes,
                      (long long)scratch_bytes, (long long)lane_bytes);
    }
    Backward bw(ctx, dp, ext_grad, arena, rec, Bump{(char *)garena, 0, garena_bytes, 0, ctx.dry},
                Bump{(char *)scratch, 0, scratch_bytes, 0, ctx.dry}, Bump{(char *)lane_scratch, 0, lane_bytes, 0, ctx.dry},
                conv_done, wgrad_first != 0, stream, lane);
    MultiUnitGuard multi_unit_guard(lane != nullptr && !ctx.dry);
    if (!ctx.dry && dp.sync_bn()) RUN(dp.bind(stream));
    RUN(bw.setup());
    for (int o = n_ops - 1; o >= 0; --o)
        RUN(bw.step(o));
    RUN(bw.join_streams());
    need[0] = bw.ga.peak;
    need[1] = bw.sc.peak;
    need[2] = bw.ls.peak;
    return 0;
}

// readers [n_ops]: for every op the op index of the convolution that normalises its output while staging it (fusion 4,
// in_bn_reader above), -1 where the BatchNorm keeps its own apply pass.  Host only; what the two passes will decide.
extern "C" int lidog_trunk_in_bn_readers(const int64_t *convs, int32_t n_convs, const int64_t *maps, int32_t n_maps,
                                         const int64_t *ops, int32_t n_ops, const int64_t *bufs, int32_t n_bufs,
                                         int32_t *readers) {
    LIDOG_REQUIRE(convs && maps && ops && bufs && readers, "trunk_in_bn_readers: null argument");
    Ctx ctx{convs, nullptr, n_convs, maps, n_maps, ops, n_ops, bufs, n_bufs, nullptr, nullptr, true};
    for (int o = 0; o < n_ops; ++o) readers[o] = in_bn_reader(ctx, o);
    return 0;
}

// Which fusions the executor applies (bit mask, see g_fusions; default: all).  Returns the previous mask; < 0 only reads.
extern "C" int32_t lidog_trunk_fusions(int32_t mask) {
    int32_t old = g_fusions;
    if (mask >= 0) g_fusions = mask;
    return old;
}

// Timing of the executor's gathered-GEMM launches (see GemmRec above).  on != 0: every launch from now on is bracketed
// by events; lidog_trunk_gemm_timing_read waits for the recorded launches and returns (launches, total ms, algorithmic
// FLOPs, algorithmic bytes) in out[0..3], then forgets them.  Not thread-safe: one timing client per process.
extern "C" int lidog_trunk_gemm_timing(int32_t on) {
    g_timing = on != 0;
    return 0;
}

// [0] MFMA weight-gradient launches, [1] their algorithmic bytes, [2] per-row reduction launches, [3] their algorithmic
// bytes, [4] output-stationary convolution launches, [5] theirs, accumulated by the executor while
// lidog_trunk_gemm_timing is on; reading resets them
extern "C" int lidog_trunk_work_read(double *out) {
    for (int i = 0; i < 6; ++i) {
        out[i] = g_work[i];
        g_work[i] = 0;
    }
    return 0;
}

extern "C" int lidog_trunk_gemm_timing_read(double *out) {
    out[0] = out[1] = out[2] = out[3] = 0;
    for (GemmRec &r : g_recs) {
        float ms = 0;
        LIDOG_CHECK_HIP(hipEventSynchronize(r.e1));
        LIDOG_CHECK_HIP(hipEventElapsedTime(&ms, r.e0, r.e1));
        out[0] += 1;
        out[1] += ms;
        out[2] += r.flops;
        out[3] += r.bytes;
        g_spare.push_back(r.e0);
        g_spare.push_back(r.e1);
    }
    g_recs.clear();
    return 0;
}
