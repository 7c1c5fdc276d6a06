// BEV projection of sparse voxel features, fused: winner map (last row wins) + the reference's
// [H,W,C] -> view(1,C,H,W) memory reinterpretation + MaxPool2d, without the dense [H,W,C] tensor.
// Reference: MinkUNetBaseBEV.filter_bounds / sparse2super, utils/models/minkunet_bev.py:158-230.
// CPU restatement: oracle/ref_torch.py:sparse2super_ref.
#include "common.h"

__global__ __launch_bounds__(256) void k_bev_winner(const int4 *__restrict__ coords, int64_t n,
                                                    const int32_t *__restrict__ lut_x,
                                                    const int32_t *__restrict__ lut_y, int lut_lo, int lut_n, int H,
                                                    int W, int32_t *winner, int32_t *__restrict__ pixel) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int4 c = coords[i];
    int ix = c.y - lut_lo, iy = c.z - lut_lo;
    int pix = -1;
    if (ix >= 0 && ix < lut_n && iy >= 0 && iy < lut_n) {
        int px = lut_x[ix], py = lut_y[iy];
        if (px >= 0 && py >= 0 && px < W && py < H) {
            pix = (c.x * H + py) * W + px;
            atomicMax(&winner[pix], (int32_t)i);  // sequential index_put_: the LAST row wins
        }
    }
    pixel[i] = pix;
}

extern "C" int lidog_bev_winner(const int32_t *coords, int64_t n, const int32_t *lut_x, const int32_t *lut_y,
                                int32_t lut_lo, int32_t lut_n, int32_t H, int32_t W, int32_t *winner, int32_t *pixel,
                                void *stream) {
    if (n == 0) return 0;
    k_bev_winner<<<(unsigned)cdiv64(n, 256), 256, 0, (hipStream_t)stream>>>((const int4 *)coords, n, lut_x, lut_y,
                                                                          lut_lo, lut_n, H, W, winner, pixel);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// out[b][c'][yo][xo] = max over the pool window of V[c'][yy][xx], V = the [H,W,C] image of sample b
// read through view(C,H,W): flat f = c'*H*W + yy*W + xx  ->  pixel f / C, feature channel f % C.
// Ties keep the first cell in window scan order, and a NaN is taken whenever it is met, so the last NaN of a window
// wins (torch max_pool2d's rule: `v > best || isnan(v)`).  PK >= pool kernel size.
struct PoolGeom {
    int C, H, W, pk, ps, pp, Ho, Wo, w_div_c, w_mod_c;
    uint64_t c_magic;  // ceil(2^40 / C): x / C = (x * c_magic) >> 40, exact while x * C < 2^40
};

template <int PK>
__device__ __forceinline__ void pool_one(const float *__restrict__ feats, const int32_t *__restrict__ win,
                                         const PoolGeom &g, int cp, int yo, int xo, float &best, int32_t &src) {
    const int C = g.C, H = g.H, W = g.W, pk = g.pk;
    const unsigned HW = (unsigned)H * (unsigned)W;
    best = -INFINITY;
    src = -1;
    // The window's cells of one view row are consecutive flat indices: they fall on one pixel (or two at a
    // multiple of C), so the pixel's winner is looked up once per row, not once per cell.  All rows' lookups are
    // issued first, unconditionally (index clamped): a load behind a data-dependent branch costs one memory
    // latency per window row.  One division per output (by multiplication); the rows below advance (pixel,
    // channel) by (W / C, W % C) with adds only -- 32-bit integer multiplies are quarter rate.
    int x_lo = xo * g.ps - g.pp, x_hi = x_lo + pk;
    if (x_lo < 0) x_lo = 0;
    if (x_hi > W) x_hi = W;
    const int seg = x_hi - x_lo;
    const int y0 = yo * g.ps - g.pp;
    const int dy_lo = y0 < 0 ? -y0 : 0;  // first window row inside the image
    const int n_rows = (pk < H - y0 ? pk : H - y0) - dy_lo;
    const unsigned f0 = (unsigned)cp * HW + __umul24((unsigned)(y0 + dy_lo), (unsigned)W) + (unsigned)x_lo;
    unsigned pix = (unsigned)(((uint64_t)f0 * g.c_magic) >> 40);
    int ch = (int)(f0 - __umul24(pix, (unsigned)C));
    int rows[PK], rows_b[PK], chs[PK];
    unsigned pixs[PK];
    // a row segment of pk cells runs over at most two pixels while C >= pk - 1: then the second pixel's winner is
    // looked up with the first one's, and no load waits for another
    const bool two = C >= pk - 1;  // uniform
#pragma unroll
    for (int j = 0; j < PK; ++j) {
        pixs[j] = pix;
        chs[j] = ch;
        rows[j] = rows_b[j] = -1;
        if (j < pk) rows[j] = win[pix < HW ? pix : HW - 1u];  // uniform predicate
        if (j < pk && two) rows_b[j] = win[pix + 1u < HW ? pix + 1u : HW - 1u];
        pix += (unsigned)g.w_div_c;
        ch += g.w_mod_c;
        if (ch >= C) {
            ch -= C;
            ++pix;
        }
    }
    if (two) {
        // Cell i of row j belongs to the row's first pixel while its channel stays below C and to the next pixel after
        // that; an empty pixel's cell is (0, -1); a cell outside the segment or the image is skipped.  A row on which
        // no lane of the wave meets an occupied pixel -- most rows: the image is 98 % empty -- is all zeros and takes
        // one compare.  The loads of the other rows (index 0 where there is nothing to read) depend on the winner
        // lookups alone and are all issued before the first compare, so a window costs two memory round trips; the
        // compares keep the scan order.
        const int NONE = -(1 << 30);
        int sa[PK], sb[PK];  // index of cell 0 of the segment in the first / the second pixel's feature row
        bool any[PK];
        float v[PK][PK];
#pragma unroll
        for (int j = 0; j < PK; ++j) {
            sa[j] = rows[j] >= 0 ? rows[j] * C + chs[j] : NONE;
            sb[j] = rows_b[j] >= 0 ? rows_b[j] * C + chs[j] - C : NONE;
            any[j] = __any(j < n_rows && seg > 0 && (rows[j] >= 0 || (chs[j] + seg > C && rows_b[j] >= 0)));
            if (any[j]) {
#pragma unroll
                for (int i = 0; i < PK; ++i) {
                    const int32_t s = (chs[j] + i >= C ? sb[j] : sa[j]) + i;
                    v[j][i] = feats[j < n_rows && i < seg && s >= 0 ? s : 0];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < PK; ++j) {
            if (any[j]) {
#pragma unroll
                for (int i = 0; i < PK; ++i) {
                    const int32_t s = (chs[j] + i >= C ? sb[j] : sa[j]) + i;
                    const float x = s >= 0 ? v[j][i] : 0.f;
                    if (j < n_rows && i < seg && (x > best || isnan(x))) {
                        best = x;
                        src = s >= 0 ? s : -1;
                    }
                }
            } else if (j < n_rows && seg > 0 && 0.f > best) {
                best = 0.f;
                src = -1;
            }
        }
        return;
    }
    // C < pk - 1 (a segment can run over three pixels or more): cell by cell
#pragma unroll
    for (int j = 0; j < PK; ++j) {
        if (j >= n_rows || seg <= 0) continue;
        int row = rows[j];
        ch = chs[j];
        pix = pixs[j];
        for (int xx = x_lo; xx < x_hi; ++xx) {
            float v = 0.f;
            int32_t s = -1;
            if (row >= 0) {
                s = row * C + ch;
                v = feats[(int64_t)s];
            }
            if (v > best || isnan(v)) {
                best = v;
                src = s;
            }
            if (++ch == C) {
                ch = 0;
                ++pix;
                if (xx + 1 < x_hi) row = win[pix];
            }
        }
    }
}

// Sparse formulation: 98 % of the BEV pixels are empty, and a window without an occupied pixel pools to
// (0, -1).  The output is therefore filled with (0, -1) by two memsets and only the windows that contain a
// cell of an occupied pixel are computed: one wave per voxel row; the row that owns its pixel (the winner)
// enumerates the windows covering its C cells -- one or two runs along x in the viewed image -- and computes
// each of them completely (several winners may compute the same window: they write the same value).
// (Since round 11 only for images so narrow that a pixel's cells touch more than BEV_MAXRUN viewed rows; every
// other shape takes k_bev_pool_fwd_flat below.)
template <int PK>
__global__ __launch_bounds__(256) void k_bev_pool_fwd_sparse(const float *__restrict__ feats,
                                                             const int32_t *__restrict__ winner,
                                                             const int32_t *__restrict__ pixel, int64_t n,
                                                             PoolGeom g, float *__restrict__ out,
                                                             int32_t *__restrict__ argsrc,
                                                             unsigned long long *__restrict__ rowbits, int words) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const int pixi = pixel[i];
    if (pixi < 0 || winner[pixi] != (int32_t)i) return;
    const unsigned HW = (unsigned)g.H * (unsigned)g.W;
    const unsigned b = (unsigned)pixi / HW;
    const unsigned q = (unsigned)pixi - b * HW;
    const int32_t *win = winner + (size_t)b * HW;
    unsigned f = q * (unsigned)g.C;  // first cell of the pixel in the viewed image (C*H*W < 2^31)
    int left = g.C;
    while (left > 0) {
        const unsigned cp = f / HW;
        const unsigned r = f - cp * HW;
        const int yy = (int)(r / (unsigned)g.W);
        const int xx0 = (int)(r - (unsigned)yy * (unsigned)g.W);
        const int len = left < g.W - xx0 ? left : g.W - xx0;
        const int xx1 = xx0 + len - 1;
        // windows (yo, xo) with yo*ps-pp <= yy <= yo*ps-pp+pk-1, likewise in x
        int t0 = yy + g.pp - g.pk + 1, t1 = xx0 + g.pp - g.pk + 1;
        const int yo_lo = t0 > 0 ? (t0 + g.ps - 1) / g.ps : 0;
        const int xo_lo = t1 > 0 ? (t1 + g.ps - 1) / g.ps : 0;
        int yo_hi = (yy + g.pp) / g.ps, xo_hi = (xx1 + g.pp) / g.ps;
        if (yo_hi > g.Ho - 1) yo_hi = g.Ho - 1;
        if (xo_hi > g.Wo - 1) xo_hi = g.Wo - 1;
        const int nx = xo_hi - xo_lo + 1, ny = yo_hi - yo_lo + 1;
        if (nx > 0 && ny > 0) {
            if (rowbits && lane < ny) {
                // structural support of the image for the convolution that reads it (conv2d_sparse.hip): one bit per
                // computed window, row (b, cp, yo) = words of 64 columns; lane l marks row yo_lo + l
                unsigned long long *rw = rowbits + (((size_t)b * g.C + cp) * g.Ho + (yo_lo + lane)) * words;
                for (int w = xo_lo >> 6; w <= (xo_hi >> 6); ++w) {
                    unsigned long long m = ~0ull;
                    if (w == (xo_lo >> 6)) m &= ~0ull << (xo_lo & 63);
                    if (w == (xo_hi >> 6)) m &= ~0ull >> (63 - (xo_hi & 63));
                    atomicOr(&rw[w], m);
                }
            }
            float *o = out + ((size_t)b * g.C + cp) * ((size_t)g.Ho * g.Wo);
            int32_t *a = argsrc + ((size_t)b * g.C + cp) * ((size_t)g.Ho * g.Wo);
            for (int yo = yo_lo; yo <= yo_hi; ++yo)
                for (int xo = xo_lo + lane; xo <= xo_hi; xo += 64) {
                    float best;
                    int32_t src;
                    pool_one<PK>(feats, win, g, (int)cp, yo, xo, best, src);
                    o[(size_t)yo * g.Wo + xo] = best;
                    a[(size_t)yo * g.Wo + xo] = src;
                }
        }
        f += (unsigned)len;
        left -= len;
    }
}

// The same windows, with the work laid out over the lanes instead of one wave per voxel row.  A wave takes BEV_RPW
// consecutive voxel rows: lane l tests row l (pixel[] and winner[] of all rows in one round trip), a ballot compacts the
// winners, and each winner's lane writes its runs -- (plane, first window row and column, windows per row), at most
// BEV_MAXRUN of them -- and its window count to LDS and marks the row bitmasks.  The wave's windows are then numbered
// consecutively across its winners (a scan of the counts) and dealt to the lanes 64 at a time: a lane finds its
// winner by a search of the counts, its run and (yo, xo) from the run's record, and computes the window with
// pool_one.  So no wave is launched for a row that owns no pixel, every window row of a winner is computed in the
// same pass, a pass holds windows of several winners, and the lanes are full whatever the run lengths are.
// Which lane computes a window changes nothing in its value (pool_one is a function of the window alone).
#define BEV_RPW 16    // voxel rows per wave
#define BEV_MAXRUN 4  // viewed-image rows the C cells of one pixel can touch

struct __align__(16) PoolRun {
    int plane, yo_lo, xo_lo, nx;  // plane = b * C + c'
};

template <int PK>
__global__ __launch_bounds__(256) void k_bev_pool_fwd_flat(const float *__restrict__ feats,
                                                           const int32_t *__restrict__ winner,
                                                           const int32_t *__restrict__ pixel, int64_t n, PoolGeom g,
                                                           float *__restrict__ out, int32_t *__restrict__ argsrc,
                                                           unsigned long long *__restrict__ rowbits, int words) {
    static_assert(BEV_RPW == 16 && BEV_MAXRUN == 4, "the searches below are written out for 16 rows and 4 runs");
    __shared__ PoolRun s_run[4][BEV_RPW][BEV_MAXRUN];
    __shared__ int4 s_rc[4][BEV_RPW];  // windows of the winner up to and including run r
    __shared__ int s_end[4][BEV_RPW];  // windows of the wave up to and including winner s
    __shared__ int s_b[4][BEV_RPW];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = ((int64_t)blockIdx.x * 4 + wv) * BEV_RPW + lane;
    const unsigned HW = (unsigned)g.H * (unsigned)g.W;
    int pixi = -1;
    if (lane < BEV_RPW && i < n) pixi = pixel[i];
    bool isw = false;
    if (pixi >= 0) isw = winner[pixi] == (int32_t)i;
    const unsigned long long wmask = __ballot(isw);
    const int slot = __popcll(wmask & ((1ull << lane) - 1ull));
    const int nw = __popcll(wmask);
    if (lane < BEV_RPW) s_end[wv][lane] = 0x7fffffff;
    int cnt = 0;
    if (isw) {
        const unsigned b = (unsigned)pixi / HW;
        const unsigned q = (unsigned)pixi - b * HW;
        unsigned f = q * (unsigned)g.C;  // first cell of the pixel in the viewed image (C*H*W < 2^31)
        int left = g.C, nr = 0;
        int rc[BEV_MAXRUN] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
        while (left > 0) {
            const unsigned cp = f / HW;
            const unsigned r = f - cp * HW;
            const int yy = (int)(r / (unsigned)g.W);
            const int xx0 = (int)(r - (unsigned)yy * (unsigned)g.W);
            const int len = left < g.W - xx0 ? left : g.W - xx0;
            const int xx1 = xx0 + len - 1;
            // windows (yo, xo) with yo*ps-pp <= yy <= yo*ps-pp+pk-1, likewise in x
            int t0 = yy + g.pp - g.pk + 1, t1 = xx0 + g.pp - g.pk + 1;
            const int yo_lo = t0 > 0 ? (t0 + g.ps - 1) / g.ps : 0;
            const int xo_lo = t1 > 0 ? (t1 + g.ps - 1) / g.ps : 0;
            int yo_hi = (yy + g.pp) / g.ps, xo_hi = (xx1 + g.pp) / g.ps;
            if (yo_hi > g.Ho - 1) yo_hi = g.Ho - 1;
            if (xo_hi > g.Wo - 1) xo_hi = g.Wo - 1;
            const int nx = xo_hi - xo_lo + 1, ny = yo_hi - yo_lo + 1;
            if (nx > 0 && ny > 0 && nr < BEV_MAXRUN) {
                const int plane = (int)(b * (unsigned)g.C + cp);
                if (rowbits) {
                    // structural support of the image for the convolution that reads it (conv2d_sparse.hip): one bit per
                    // computed window, row (b, cp, yo) = words of 64 columns
                    for (int yo = yo_lo; yo <= yo_hi; ++yo) {
                        unsigned long long *rw = rowbits + ((size_t)plane * g.Ho + yo) * words;
                        for (int w = xo_lo >> 6; w <= (xo_hi >> 6); ++w) {
                            unsigned long long m = ~0ull;
                            if (w == (xo_lo >> 6)) m &= ~0ull << (xo_lo & 63);
                            if (w == (xo_hi >> 6)) m &= ~0ull >> (63 - (xo_hi & 63));
                            atomicOr(&rw[w], m);
                        }
                    }
                }
                PoolRun pr;
                pr.plane = plane; pr.yo_lo = yo_lo; pr.xo_lo = xo_lo; pr.nx = nx;
                s_run[wv][slot][nr] = pr;
                cnt += nx * ny;
                rc[nr] = cnt;
                ++nr;
            }
            f += (unsigned)len;
            left -= len;
        }
        s_rc[wv][slot] = make_int4(rc[0], rc[1], rc[2], rc[3]);
        s_b[wv][slot] = (int)b;
    }
    int inc = cnt;  // inclusive scan over the wave's rows (winners keep their lane order in the slots)
#pragma unroll
    for (int d = 1; d < BEV_RPW; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (isw) s_end[wv][slot] = inc;
    __syncthreads();
    const int total = nw ? s_end[wv][nw - 1] : 0;
    const int *e = s_end[wv];
    const size_t HoWo = (size_t)g.Ho * g.Wo;
    for (int it = lane; it < total; it += 64) {
        // s = number of winners whose windows end at or before `it` (unused slots hold 0x7fffffff)
        int s = e[7] <= it ? 8 : 0;
        if (e[s + 3] <= it) s += 4;
        if (e[s + 1] <= it) s += 2;
        if (e[s] <= it) s += 1;
        int t = it - (s ? e[s - 1] : 0);
        const int4 rc = s_rc[wv][s];
        const int r = (t >= rc.x) + (t >= rc.y) + (t >= rc.z);
        t -= r == 0 ? 0 : r == 1 ? rc.x : r == 2 ? rc.y : rc.z;
        const PoolRun pr = s_run[wv][s][r];
        const int dy = t / pr.nx;
        const int yo = pr.yo_lo + dy, xo = pr.xo_lo + (t - dy * pr.nx);
        const int b = s_b[wv][s];
        float best;
        int32_t src;
        pool_one<PK>(feats, winner + (size_t)b * HW, g, pr.plane - b * g.C, yo, xo, best, src);
        const size_t o = (size_t)pr.plane * HoWo + (size_t)yo * g.Wo + xo;
        out[o] = best;
        argsrc[o] = src;
    }
}

extern "C" int lidog_bev_pool_fwd(const float *feats, int32_t C, const int32_t *winner, const int32_t *pixel,
                                  int64_t n, int32_t B, int32_t H, int32_t W, int32_t pk, int32_t ps, int32_t pp,
                                  int32_t Ho, int32_t Wo, float *out, int32_t *argsrc, uint64_t *rowbits,
                                  void *stream) {
    int64_t total = (int64_t)B * C * Ho * Wo;
    if (total == 0) return 0;
    LIDOG_REQUIRE((int64_t)H * W * C < ((int64_t)1 << 31), "bev_pool_fwd: C*H*W must stay below 2^31");
    LIDOG_REQUIRE((int64_t)B * H * W < ((int64_t)1 << 31), "bev_pool_fwd: B*H*W must stay below 2^31");
    LIDOG_REQUIRE(C >= 1 && C <= 512, "bev_pool_fwd: 1 <= C <= 512");
    LIDOG_REQUIRE(pk >= 1 && pk <= 8 && ps >= 1, "bev_pool_fwd: pool kernel size must be 1..8");
    LIDOG_REQUIRE(2 * pp <= pk, "bev_pool_fwd: padding must be at most half the kernel size (as torch requires)");
    LIDOG_REQUIRE((int64_t)H * W < ((int64_t)1 << 24), "bev_pool_fwd: H*W must stay below 2^24");
    LIDOG_REQUIRE(n * C < ((int64_t)1 << 31), "bev_pool_fwd: n*C must stay below 2^31 (int32 cell indices)");
    hipStream_t st = (hipStream_t)stream;
    // windows without an occupied pixel: max over zeros = 0, no source cell
    if (hipMemsetAsync(out, 0, sizeof(float) * (size_t)total, st) != hipSuccess) return 1;
    // with row bitmasks argsrc is only ever read where a bit is set (lidog_bev_pool_bwd), i.e. where it was written
    if (!rowbits && hipMemsetAsync(argsrc, 0xff, sizeof(int32_t) * (size_t)total, st) != hipSuccess) return 1;
    const int words = (Wo + 63) / 64;
    if (rowbits && hipMemsetAsync(rowbits, 0, sizeof(uint64_t) * (size_t)B * C * Ho * words, st) != hipSuccess) return 1;
    if (n == 0) return 0;
    LIDOG_REQUIRE(rowbits == nullptr || pk + ps <= 64, "bev_pool_fwd: row bitmasks need pool kernel + stride <= 64");
    PoolGeom g;
    g.C = C; g.H = H; g.W = W; g.pk = pk; g.ps = ps; g.pp = pp; g.Ho = Ho; g.Wo = Wo;
    g.w_div_c = W / C; g.w_mod_c = W % C;
    g.c_magic = (((uint64_t)1 << 40) + (uint64_t)C - 1) / (uint64_t)C;
    // viewed-image rows that C consecutive cells can touch; a pixel with more of them than the run records hold
    // (an image narrower than a third of C) takes the one-wave-per-row kernel
    const int max_runs = C >= 2 ? (C - 2) / W + 2 : 1;
    const bool flat = max_runs <= BEV_MAXRUN;
    const unsigned grid = flat ? (unsigned)cdiv64(n, 4 * BEV_RPW) : (unsigned)cdiv64(n, 4);
#define BEV_POOL_LAUNCH(PK)                                                                                     \
    do {                                                                                                        \
        if (flat)                                                                                               \
            k_bev_pool_fwd_flat<PK><<<grid, 256, 0, st>>>(feats, winner, pixel, n, g, out, argsrc,              \
                                                          reinterpret_cast<unsigned long long *>(rowbits), words); \
        else                                                                                                    \
            k_bev_pool_fwd_sparse<PK><<<grid, 256, 0, st>>>(feats, winner, pixel, n, g, out, argsrc,            \
                                                            reinterpret_cast<unsigned long long *>(rowbits), words); \
    } while (0)
    if (pk <= 3) BEV_POOL_LAUNCH(3);
    else if (pk <= 5) BEV_POOL_LAUNCH(5);
    else BEV_POOL_LAUNCH(8);
#undef BEV_POOL_LAUNCH
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// Backward of the fused scatter + view + max-pool, as a GATHER (no atomics: bit-reproducible).  One thread per
// (voxel row i, channel c): the row's pixel belongs to the winner row w (index_put's backward is a gather: EVERY row that
// targets a pixel receives that pixel's gradient); cell (w, c) sits at flat index f = q*C + c of the viewed image
// -> (c', yy, xx); it can be the arg-max of the at most ceil(pk/ps)^2 windows that cover it, whose gradients are
// added in ascending (yo, xo) order when argsrc says this cell was their maximum.  Every window covering a cell of an
// occupied pixel was computed by the forward pass, so argsrc is defined wherever it is read here.
__global__ __launch_bounds__(256) void k_bev_pool_bwd_gather(const float *__restrict__ gout,
                                                             const int32_t *__restrict__ argsrc,
                                                             const int32_t *__restrict__ winner,
                                                             const int32_t *__restrict__ pixel, int64_t n, PoolGeom g,
                                                             float *__restrict__ gfeats) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * g.C) return;
    const int64_t i = idx / g.C;
    const int c = (int)(idx - i * g.C);
    const int pixi = pixel[i];
    float acc = 0.f;
    if (pixi >= 0) {
        const unsigned HW = (unsigned)g.H * (unsigned)g.W;
        const unsigned b = (unsigned)pixi / HW;
        const unsigned q = (unsigned)pixi - b * HW;
        const int32_t cell = winner[pixi] * g.C + c;
        const unsigned f = q * (unsigned)g.C + (unsigned)c;
        const unsigned cp = f / HW;
        const unsigned r = f - cp * HW;
        const int yy = (int)(r / (unsigned)g.W);
        const int xx = (int)(r - (unsigned)yy * (unsigned)g.W);
        const int t0 = yy + g.pp - g.pk + 1, t1 = xx + g.pp - g.pk + 1;
        const int yo_lo = t0 > 0 ? (t0 + g.ps - 1) / g.ps : 0;
        const int xo_lo = t1 > 0 ? (t1 + g.ps - 1) / g.ps : 0;
        int yo_hi = (yy + g.pp) / g.ps, xo_hi = (xx + g.pp) / g.ps;
        if (yo_hi > g.Ho - 1) yo_hi = g.Ho - 1;
        if (xo_hi > g.Wo - 1) xo_hi = g.Wo - 1;
        const size_t plane = ((size_t)b * g.C + cp) * ((size_t)g.Ho * g.Wo);
        for (int yo = yo_lo; yo <= yo_hi; ++yo)
            for (int xo = xo_lo; xo <= xo_hi; ++xo) {
                const size_t e = plane + (size_t)yo * g.Wo + xo;
                if (argsrc[e] == cell) acc += gout[e];
            }
    }
    gfeats[idx] = acc;
}

// The same gather with the index arithmetic of a voxel row done once per row and the loads of a cell issued together.
// A wave takes BEV_RPW consecutive rows: lane l resolves row l (pixel -> winner cell, plane and position of the
// pixel's first cell in the viewed image) into LDS; the wave's rows x C cells are then dealt to the lanes 64 at a time.
// A cell advances its row's position by c with carries (no division), finds its window range with multiplications by
// ceil(2^40 / ps), loads the NW x NW (argsrc, gout) pairs of the windows that can cover it UNCONDITIONALLY (indices
// clamped into the plane) and only then selects and adds, in ascending (yo, xo) order.  NW = ceil(pk / ps).
struct __align__(16) PoolRow {
    int cell0, plane0, yy0, xx0;  // winner * C, b * C + c' (-1: row outside the image), position of the first cell
};

template <int NW>
__global__ __launch_bounds__(256) void k_bev_pool_bwd_rows(const float *__restrict__ gout,
                                                           const int32_t *__restrict__ argsrc,
                                                           const int32_t *__restrict__ winner,
                                                           const int32_t *__restrict__ pixel, int64_t n, PoolGeom g,
                                                           uint64_t ps_magic, float *__restrict__ gfeats) {
    __shared__ PoolRow s_row[4][BEV_RPW];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wv) * BEV_RPW;
    if (lane < BEV_RPW) {
        PoolRow pr;
        pr.cell0 = 0; pr.plane0 = -1; pr.yy0 = 0; pr.xx0 = 0;
        const int64_t i = row0 + lane;
        const int pixi = i < n ? pixel[i] : -1;
        if (pixi >= 0) {
            const unsigned HW = (unsigned)g.H * (unsigned)g.W;
            const unsigned b = (unsigned)pixi / HW;
            const unsigned q = (unsigned)pixi - b * HW;
            const unsigned f = q * (unsigned)g.C;
            const unsigned cp = f / HW;
            const unsigned r = f - cp * HW;
            pr.yy0 = (int)(r / (unsigned)g.W);
            pr.xx0 = (int)(r - (unsigned)pr.yy0 * (unsigned)g.W);
            pr.plane0 = (int)(b * (unsigned)g.C + cp);
            pr.cell0 = winner[pixi] * g.C;
        }
        s_row[wv][lane] = pr;
    }
    __syncthreads();
    const int64_t rows_left = n - row0;
    const int rows = rows_left < BEV_RPW ? (rows_left > 0 ? (int)rows_left : 0) : BEV_RPW;
    const int items = rows * g.C;
    const size_t HoWo = (size_t)g.Ho * g.Wo;
    float *gf = gfeats + row0 * g.C;
    for (int k = lane; k < items; k += 64) {
        const int rl = (int)(((uint64_t)(unsigned)k * g.c_magic) >> 40);  // k / C
        const int c = k - rl * g.C;
        const PoolRow pr = s_row[wv][rl];
        float acc = 0.f;
        if (pr.plane0 >= 0) {
            int xx = pr.xx0 + c, yy = pr.yy0, plane = pr.plane0;
            while (xx >= g.W) {
                xx -= g.W;
                if (++yy == g.H) {
                    yy = 0;
                    ++plane;
                }
            }
            const int32_t cell = pr.cell0 + c;
            const int t0 = yy + g.pp - g.pk + 1, t1 = xx + g.pp - g.pk + 1;
            const int yo_lo = t0 > 0 ? (int)(((uint64_t)(unsigned)(t0 + g.ps - 1) * ps_magic) >> 40) : 0;
            const int xo_lo = t1 > 0 ? (int)(((uint64_t)(unsigned)(t1 + g.ps - 1) * ps_magic) >> 40) : 0;
            int yo_hi = (int)(((uint64_t)(unsigned)(yy + g.pp) * ps_magic) >> 40);
            int xo_hi = (int)(((uint64_t)(unsigned)(xx + g.pp) * ps_magic) >> 40);
            if (yo_hi > g.Ho - 1) yo_hi = g.Ho - 1;
            if (xo_hi > g.Wo - 1) xo_hi = g.Wo - 1;
            const size_t base = (size_t)plane * HoWo;
            int32_t a[NW * NW];
            float v[NW * NW];
#pragma unroll
            for (int jy = 0; jy < NW; ++jy)
#pragma unroll
                for (int jx = 0; jx < NW; ++jx) {
                    const int yo = yo_lo + jy, xo = xo_lo + jx;
                    const size_t e = base + (size_t)(yo < g.Ho ? yo : g.Ho - 1) * g.Wo + (xo < g.Wo ? xo : g.Wo - 1);
                    a[jy * NW + jx] = argsrc[e];
                    v[jy * NW + jx] = gout[e];
                }
#pragma unroll
            for (int jy = 0; jy < NW; ++jy)
#pragma unroll
                for (int jx = 0; jx < NW; ++jx)
                    if (yo_lo + jy <= yo_hi && xo_lo + jx <= xo_hi && a[jy * NW + jx] == cell) acc += v[jy * NW + jx];
        }
        gf[k] = acc;
    }
}

extern "C" int lidog_bev_pool_bwd(const float *gout, const int32_t *argsrc, const int32_t *winner,
                                  const int32_t *pixel, int64_t n, int32_t C, int32_t B, int32_t H, int32_t W,
                                  int32_t pk, int32_t ps, int32_t pp, int32_t Ho, int32_t Wo, float *gfeats,
                                  void *stream) {
    hipStream_t st = (hipStream_t)stream;
    (void)B;
    if (n == 0) return 0;
    LIDOG_REQUIRE((int64_t)H * W * C < ((int64_t)1 << 31), "bev_pool_bwd: C*H*W must stay below 2^31");
    LIDOG_REQUIRE(pk >= 1 && pk <= 8 && ps >= 1 && 2 * pp <= pk, "bev_pool_bwd: bad pooling geometry");
    LIDOG_REQUIRE(n * C < ((int64_t)1 << 31), "bev_pool_bwd: n*C must stay below 2^31 (int32 cell indices)");
    PoolGeom g;
    g.C = C; g.H = H; g.W = W; g.pk = pk; g.ps = ps; g.pp = pp; g.Ho = Ho; g.Wo = Wo;
    g.w_div_c = W / C; g.w_mod_c = W % C;
    g.c_magic = (((uint64_t)1 << 40) + (uint64_t)C - 1) / (uint64_t)C;
    // windows along one axis that can cover a cell; the unrolled kernel is built for up to 4, and its multiplications
    // by ceil(2^40 / ps) and ceil(2^40 / C) are exact for the sizes below
    const int nw = (pk + ps - 1) / ps;
    const bool by_rows = nw <= 4 && ps < (1 << 15) && C <= 4096 && H < (1 << 24) && W < (1 << 24) && Ho >= 1 && Wo >= 1;
    if (by_rows) {
        const uint64_t ps_magic = (((uint64_t)1 << 40) + (uint64_t)ps - 1) / (uint64_t)ps;
        const unsigned grid = (unsigned)cdiv64(n, 4 * BEV_RPW);
        switch (nw) {
            case 1: k_bev_pool_bwd_rows<1><<<grid, 256, 0, st>>>(gout, argsrc, winner, pixel, n, g, ps_magic, gfeats); break;
            case 2: k_bev_pool_bwd_rows<2><<<grid, 256, 0, st>>>(gout, argsrc, winner, pixel, n, g, ps_magic, gfeats); break;
            case 3: k_bev_pool_bwd_rows<3><<<grid, 256, 0, st>>>(gout, argsrc, winner, pixel, n, g, ps_magic, gfeats); break;
            default: k_bev_pool_bwd_rows<4><<<grid, 256, 0, st>>>(gout, argsrc, winner, pixel, n, g, ps_magic, gfeats);
        }
    } else {
        k_bev_pool_bwd_gather<<<(unsigned)cdiv64(n * C, 256), 256, 0, st>>>(gout, argsrc, winner, pixel, n, g, gfeats);
    }
    LIDOG_LAUNCH_CHECK();
    return 0;
}
