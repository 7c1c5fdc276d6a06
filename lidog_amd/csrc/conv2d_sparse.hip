// Conv2d(k3, s2, p1) over a STRUCTURALLY SPARSE input: the first convolution of Encoder2D reads the image made by
// sparse2super (utils/models/minkunet_bev.py:158-230), in which 95 % of the cells are empty (no voxel under the
// pooling window: exact zeros, and no gradient is needed there).  Seen through the implicit-GEMM tiles of
// conv2d.hip, only ~21 % of the (128-pixel tile, input channel) pairs contain a non-empty cell (seed-0 synthetic
// scan; scripts/bev_sparsity.py), so each tile works on the compacted list of its active channels:
//   FWD    reduction index k = (ci, tap) runs over the active channels only (a skipped term is 0 * w: the fmaf
//          chain of the remaining terms is unchanged, so the result is bit-identical to the dense kernel);
//   DGRAD  rows i = ci of the output tile are the active channels only (the gradient of an empty cell is never
//          read: sparse2super's backward routes gradients to arg-max cells); rows of inactive channels are NOT
//          written.
// The activity comes from a `support` tensor [B,Cin,H,W] int32 (>= 0 where the cell is non-empty: the arg-max
// source map of the pooling): one pass turns it into a bit per cell, a second one into per-tile channel lists.
#include <vector>

#include "conv2d.h"

// ------------------------------------------------------------------ support -> row bitmasks -> tile lists
// one wave per image row (b, c, y): bit x of word x / 64 = support[b][c][y][x] >= 0
__global__ __launch_bounds__(256) void k_support_rowbits(const int32_t *__restrict__ sup, int64_t rows, int W,
                                                         int words, uint64_t *__restrict__ bits) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int32_t *s = sup + row * W;
    for (int w = 0; w < words; ++w) {
        const int x = w * 64 + lane;
        const bool v = x < W && s[x] >= 0;
        const uint64_t bal = __ballot(v);
        if (lane == 0) bits[row * words + w] = bal;
    }
}

// Tile = 128 consecutive pixels j = (b, yc, xc) of a pixel grid Hc x Wc per image.  Pixel (yc, xc) touches the
// input rows 2*yc + ya + [0, ny) and columns 2*xc + xlo .. 2*xc + xhi; `mask` selects the column parity.
//   forward / weight gradient: the output pixels, ya = -1, ny = 3, xlo = -1, xhi = +1, every column
//   data gradient, class (py, px): the input pixels of the class, ya = py, ny = 1, xlo = xhi = px, parity px
struct ListGeom {
    int C, H, W, Hc, Wc, Nj;
    int ya, ny, xlo, xhi;
    uint64_t mask;
};

// lists[tile][0] = number of active channels, lists[tile][1..] = their ids, ascending
__device__ __forceinline__ void tile_list(const uint64_t *__restrict__ bits, int words, const ListGeom &g,
                                          int32_t *__restrict__ lists, uint64_t *__restrict__ tbits, int tile) {
    __shared__ int s_cnt[2];
    const int c = threadIdx.x;
    int j = tile * IG_T;
    const int j1 = (j + IG_T - 1 < g.Nj - 1) ? j + IG_T - 1 : g.Nj - 1;
    const int hw = g.Hc * g.Wc;
    bool act = false;
    if (c < g.C) {
        while (j <= j1) {
            const int b = j / hw, r = j - b * hw;
            const int yc = r / g.Wc, xa = r - yc * g.Wc;
            int xb = xa + (j1 - j);
            if (xb > g.Wc - 1) xb = g.Wc - 1;
            int x_lo = 2 * xa + g.xlo, x_hi = 2 * xb + g.xhi;
            if (x_lo < 0) x_lo = 0;
            if (x_hi > g.W - 1) x_hi = g.W - 1;
            for (int dy = 0; dy < g.ny; ++dy) {
                const int y = 2 * yc + g.ya + dy;
                if (y < 0 || y >= g.H) continue;
                const uint64_t *row = bits + ((size_t)(b * g.C + c) * g.H + y) * words;
                for (int w = x_lo >> 6; w <= (x_hi >> 6); ++w) {
                    uint64_t m = g.mask;
                    if (w == (x_lo >> 6)) m &= ~0ull << (x_lo & 63);
                    if (w == (x_hi >> 6)) m &= ~0ull >> (63 - (x_hi & 63));
                    if (row[w] & m) act = true;
                }
            }
            j += xb - xa + 1;
        }
    }
    const uint64_t bal = __ballot(act);
    const int lane = c & 63, wv = c >> 6;
    const int pre = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[wv] = __popcll(bal);
    __syncthreads();
    int32_t *lst = lists + (size_t)tile * (g.C + 1);
    if (act) lst[1 + (wv ? s_cnt[0] : 0) + pre] = c;
    if (c == 0) lst[0] = s_cnt[0] + s_cnt[1];
    if (tbits && lane == 0) tbits[(size_t)tile * 2 + wv] = bal;  // bit c of the tile's 128-bit channel mask
}

__global__ __launch_bounds__(128) void k_tile_lists(const uint64_t *__restrict__ bits, int words, ListGeom g,
                                                    int32_t *__restrict__ lists, uint64_t *__restrict__ tbits) {
    tile_list(bits, words, g, lists, tbits, (int)blockIdx.x);
}

// the four data-gradient classes in one launch (they feed the backward pass only, but are built on the forward pass's
// stream: four launches of ~870 workgroups each cost four launch latencies there): workgroup x belongs to the class
// whose tile range [first[cls], first[cls + 1]) holds it
struct ListGeom4 {
    ListGeom g[4];
    int first[5];
    int64_t off[4];
};
__global__ __launch_bounds__(128) void k_tile_lists4(const uint64_t *__restrict__ bits, int words, ListGeom4 q,
                                                     int32_t *__restrict__ act) {
    const int x = blockIdx.x;
    const int cls = x < q.first[1] ? 0 : x < q.first[2] ? 1 : x < q.first[3] ? 2 : 3;
    tile_list(bits, words, q.g[cls], act + q.off[cls], nullptr, x - q.first[cls]);
}

// Weight gradient: the columns (ci, tap) of gW are cut into groups of WA_GC channels; group g works on the pixel
// tiles in which one of its channels is active.  glists[g][0] = number of such tiles, glists[g][1..] = their ids,
// ascending (ordered compaction: ballot + prefix over the four waves, 256 tiles per round).
#ifndef WA_GC
#define WA_GC 7   // 63 of 64 MFMA columns carry data; 57 % of the (group, tile) pairs are active on a LiDAR sweep
#endif
#define WA_NT ((9 * WA_GC + 31) / 32)  // 32-column MFMA tiles per group
__global__ __launch_bounds__(256) void k_group_lists(const uint64_t *__restrict__ tbits, int n_tiles, int C,
                                                     int32_t *__restrict__ glists) {
    __shared__ int s_cnt[4];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint64_t m0 = 0, m1 = 0;
    for (int c = g * WA_GC; c < g * WA_GC + WA_GC && c < C; ++c) {
        if (c < 64) m0 |= 1ull << c;
        else m1 |= 1ull << (c - 64);
    }
    int32_t *gl = glists + (size_t)g * (n_tiles + 1);
    int base = 0;
    for (int t0 = 0; t0 < n_tiles; t0 += 256) {
        const int t = t0 + tid;
        const bool f = t < n_tiles && ((tbits[(size_t)t * 2] & m0) | (tbits[(size_t)t * 2 + 1] & m1)) != 0;
        const uint64_t bal = __ballot(f);
        if (lane == 0) s_cnt[wv] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wv; ++w) off += s_cnt[w];
        if (f) gl[1 + off + __popcll(bal & ((1ull << lane) - 1ull))] = t;
        base += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        __syncthreads();
    }
    if (tid == 0) gl[0] = base;
}

struct ActLayout {
    int words;
    int64_t bits_off, fwd_off, tbits_off, glists_off, dgrad_off[4], total;  // in int32 elements
    int fwd_tiles, dgrad_tiles[4], groups;
};

static ActLayout act_layout(int B, int C, int H, int W) {
    ActLayout L;
    L.words = (W + 63) / 64;
    L.bits_off = 0;
    int64_t off = 2 * (int64_t)B * C * H * L.words;  // uint64 words as int32 pairs (offset stays even)
    L.fwd_tiles = (int)cdiv64((int64_t)B * c2_out_dim(H) * c2_out_dim(W), IG_T);
    L.fwd_off = off;
    off += (int64_t)L.fwd_tiles * (C + 1);
    off += off & 1;
    L.tbits_off = off;                       // uint64 [fwd_tiles][2]
    off += 4 * (int64_t)L.fwd_tiles;
    L.groups = (C + WA_GC - 1) / WA_GC;
    L.glists_off = off;
    off += (int64_t)L.groups * (L.fwd_tiles + 1);
    for (int cls = 0; cls < 4; ++cls) {
        int py = cls >> 1, px = cls & 1;
        int Hc = (H - py + 1) / 2, Wc = (W - px + 1) / 2;
        L.dgrad_tiles[cls] = (int)cdiv64((int64_t)B * Hc * Wc, IG_T);
        L.dgrad_off[cls] = off;
        off += (int64_t)L.dgrad_tiles[cls] * (C + 1);
    }
    L.total = off;
    return L;
}

extern "C" int64_t lidog_conv2d_support_ws(int32_t B, int32_t Cin, int32_t H, int32_t W) {
    return act_layout(B, Cin, H, W).total;
}

extern "C" int lidog_conv2d_support(const int32_t *support, int32_t B, int32_t Cin, int32_t H, int32_t W,
                                    int32_t *act, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(Cin >= 1 && Cin <= 128, "conv2d_support: 1 <= Cin <= 128");
    LIDOG_REQUIRE((int64_t)B * Cin * H * W < ((int64_t)1 << 31), "conv2d_support: tensor too large");
    if ((int64_t)B * H * W == 0) return 0;
    ActLayout L = act_layout(B, Cin, H, W);
    uint64_t *bits = reinterpret_cast<uint64_t *>(act + L.bits_off);
    int64_t rows = (int64_t)B * Cin * H;
    if (support)  // NULL: lidog_bev_pool_fwd has already written the row bitmasks
        k_support_rowbits<<<(unsigned)cdiv64(rows, 4), 256, 0, st>>>(support, rows, W, L.words, bits);
    ListGeom g;
    g.C = Cin; g.H = H; g.W = W;
    g.Hc = c2_out_dim(H); g.Wc = c2_out_dim(W); g.Nj = B * g.Hc * g.Wc;
    g.ya = -1; g.ny = 3; g.xlo = -1; g.xhi = 1; g.mask = ~0ull;
    uint64_t *tbits = reinterpret_cast<uint64_t *>(act + L.tbits_off);
    k_tile_lists<<<(unsigned)L.fwd_tiles, 128, 0, st>>>(bits, L.words, g, act + L.fwd_off, tbits);
    k_group_lists<<<(unsigned)L.groups, 256, 0, st>>>(tbits, L.fwd_tiles, Cin, act + L.glists_off);
    ListGeom4 q;
    q.first[0] = 0;
    for (int cls = 0; cls < 4; ++cls) {
        int py = cls >> 1, px = cls & 1;
        g.Hc = (H - py + 1) / 2; g.Wc = (W - px + 1) / 2; g.Nj = B * g.Hc * g.Wc;
        g.ya = py; g.ny = 1; g.xlo = px; g.xhi = px;
        g.mask = px ? 0xAAAAAAAAAAAAAAAAull : 0x5555555555555555ull;
        q.g[cls] = g;
        q.off[cls] = L.dgrad_off[cls];
        q.first[cls + 1] = q.first[cls] + L.dgrad_tiles[cls];
    }
    if (q.first[4] > 0) k_tile_lists4<<<(unsigned)q.first[4], 128, 0, st>>>(bits, L.words, q, act);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ FWD over the active channels of each pixel tile
// Same tile and MFMA schedule as k_conv_s2<IG_FWD, 2, 2, 2>: D[co][pixel] = sum_k W[co][k] * im2col(X)[k][pixel],
// 128 x 128, 32-deep stages.  The reduction table of the workgroup lists (offset, tap, weight row) of the ACTIVE
// channels' 9 taps, padded to a multiple of 32 with entries whose tap never validates; the weights are read from
// the transposed copy Wt[k][co], so that a stage row is contiguous whatever k it is.
__global__ __launch_bounds__(256) void k_conv_fwd_act(IgParams p, const int32_t *__restrict__ lists,
                                                      const float *__restrict__ Wt) {
    __shared__ __attribute__((aligned(16))) float As[C2_KB * IG_LD];
    __shared__ float Bs[C2_KB * IG_LD];
    extern __shared__ int2 s_tab[];  // [max(Kp, C2_KB)] (x offset, tap | weight row << 5)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.y * IG_T, j0 = blockIdx.x * IG_T;
    const int HW = p.H * p.W, HoWo = p.Ho * p.Wo;
    const int kw = __builtin_amdgcn_readfirstlane(tid >> 7);
    const int32_t *lst = lists + (size_t)blockIdx.x * (p.Cin + 1);
    const int n_act = lst[0];
    const int Kd = n_act * 9, Kp = (Kd + C2_KB - 1) / C2_KB * C2_KB;

    // padded to a whole stage with entries whose tap never validates, and to one stage at least: load(0) of a tile
    // without active channels reads weight row 0 and the lane's own pixel
    for (int kk = tid; kk < (Kp > 0 ? Kp : C2_KB); kk += 256) {
        int koff = 0, t = 15, row = 0;
        if (kk < Kd) {
            int a = kk / 9;
            t = kk - a * 9;
            int ci = lst[1 + a];
            int ty = t / 3, tx = t - ty * 3;
            koff = ci * HW + (ty - 1) * p.W + (tx - 1);
            row = ci * 9 + t;
        }
        s_tab[kk] = make_int2(koff, t | (row << 5));
    }
    const PixelTaps px = fwd_pixel(p, j0 + (tid & 127));
    __syncthreads();  // table complete

    float4 ra[4];
    GatherB gb;
    const int a_kr = tid >> 5, a_c4 = (tid & 31) * 4;  // stage row / column quad of float4 v: row a_kr + 8 v
    auto load = [&](int s) {
        const int k0 = s * C2_KB;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int row = s_tab[k0 + a_kr + 8 * v].y >> 5;
            ra[v] = *reinterpret_cast<const float4 *>(Wt + (size_t)row * p.Cout + i0 + a_c4);
        }
        gb.load(p.Bm, &s_tab[k0 + kw], px);
    };
    auto store = [&]() {
#pragma unroll
        for (int v = 0; v < 4; ++v) *reinterpret_cast<float4 *>(&As[(a_kr + 8 * v) * IG_LD + a_c4]) = ra[v];
        gb.store(&Bs[kw * IG_LD + (tid & 127)]);
    };

    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    const int li = lane & 31, kh = lane >> 5;
    f32x16 acc[2][2];
    mfma_stages<2, 2, IG_LD, IG_LD>(acc, &As[kh * IG_LD + wi + li], &Bs[kh * IG_LD + wj + li], Kp / C2_KB, load, store);

#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        int jo = j0 + wj + 32 * tj + li;
        if (jo >= p.Nj) continue;
        int b = jo / HoWo;
        size_t col_off = (size_t)b * p.Cout * HoWo + (jo - b * HoWo);
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                int i = i0 + wi + 32 * ti + mfma_row(e, kh);
                if (i < p.Mi) p.D[col_off + (size_t)i * HoWo] = acc[ti][tj][e];
            }
        }
    }
}

extern "C" int lidog_conv2d_fwd_sparse(const float *x, const float *w, const int32_t *act, int32_t B, int32_t Cin,
                                       int32_t H, int32_t W, int32_t Cout, float *y, float *ws, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(Cin >= 1 && Cin <= 128 && Cout % IG_T == 0, "conv2d_fwd_sparse: Cin <= 128, Cout a multiple of 128");
    LIDOG_REQUIRE(ws != nullptr, "conv2d_fwd_sparse: needs a Cin*9*Cout float workspace (transposed weights)");
    IgParams p = {};
    p.Bm = x; p.D = y;
    p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout;
    p.Ho = c2_out_dim(H); p.Wo = c2_out_dim(W);
    p.Mi = Cout; p.Nj = B * p.Ho * p.Wo; p.Kd = Cin * 9;
    if (p.Nj == 0) return 0;
    LIDOG_REQUIRE((int64_t)B * Cin * H * W < ((int64_t)1 << 31) && (int64_t)(p.Kd + C2_KB) * 8 <= 24576,
                  "conv2d_fwd_sparse: tensor too large for 32-bit offsets / reduction table");
    ActLayout L = act_layout(B, Cin, H, W);
    // Wt[k][co] = W[co][k]
    int rc = lidog_transpose_kernel(w, 1, Cout, p.Kd, ws, stream);
    if (rc) return rc;
    dim3 grid((unsigned)L.fwd_tiles, (unsigned)(Cout / IG_T), 1);
    k_conv_fwd_act<<<grid, 256, (size_t)(p.Kd + C2_KB) * sizeof(int2), st>>>(p, act + L.fwd_off, ws);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ DGRAD for the active channels of each pixel tile
// Same schedule as k_conv_s2<IG_DGRAD, 1, 3, 1> (rows i = ci, 128 class pixels per tile, k = (co, tap)), with the
// rows of the tile = the active channels of the tile: TIA = ceil(n_act / 32) row blocks instead of Cin / 32.
template <int TIA>
__device__ __forceinline__ void conv_dgrad_act_body(const IgParams &p, const int tile, const int *s_ch, int n_act,
                                                    float *As, float *Bs, const int2 *s_tab) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = tile * IG_T;
    const int kw = __builtin_amdgcn_readfirstlane(tid >> 7);
    const PixelTaps px = dgrad_pixel(p, j0 + (tid & 127));

    // A rows this thread stages: float4 v covers rows 32 v + (tid >> 3)
    const float *a_ptr[TIA];
    bool a_ok[TIA];
#pragma unroll
    for (int v = 0; v < TIA; ++v) {
        int il = 32 * v + (tid >> 3);
        a_ok[v] = il < n_act;
        a_ptr[v] = p.A + (size_t)(a_ok[v] ? s_ch[il] : 0) * p.Kd + (tid & 7) * 4;
    }

    float4 ra[TIA];
    GatherB gb;
    auto load = [&](int s) {
        const int k0 = s * C2_KB;
#pragma unroll
        for (int v = 0; v < TIA; ++v) ra[v] = *reinterpret_cast<const float4 *>(a_ptr[v] + k0);
        gb.load(p.Bm, &s_tab[k0 + kw], px);
    };
    auto store = [&]() {
        store_a_rows(As, ra, a_ok, tid);
        gb.store(&Bs[kw * IG_LD + (tid & 127)]);
    };

    const int wj = wave * 32;
    const int li = lane & 31, kh = lane >> 5;
    f32x16 acc[TIA][1];
    mfma_stages<TIA, 1, IG_LD, IG_LD>(acc, &As[kh * IG_LD + li], &Bs[kh * IG_LD + wj + li], p.Kd / C2_KB, load, store);

    const int jo = j0 + wj + li;
    if (jo < p.Nj) {
        const size_t col_off = dgrad_pixel_offset(p, jo);
        const int HW = p.H * p.W;
#pragma unroll
        for (int ti = 0; ti < TIA; ++ti) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                int il = 32 * ti + mfma_row(e, kh);
                if (il < n_act) p.D[col_off + (size_t)s_ch[il] * HW] = acc[ti][0][e];
            }
        }
    }
}

// the four parity classes in one launch, the four-tap class first (conv2d.hip:k_conv_s2 has the reasoning)
__global__ __launch_bounds__(256) void k_conv_dgrad_act(IgClasses pc, const int32_t *__restrict__ act) {
    __shared__ float As[C2_KB * IG_LD];
    __shared__ float Bs[C2_KB * IG_LD];
    __shared__ int s_ch[128];
    extern __shared__ int2 s_tab[];  // [Kd] (offset, tap)
    const int tid = threadIdx.x;
    int cls = 0;
    while (cls + 1 < pc.n && (int)blockIdx.x >= pc.first[cls + 1]) ++cls;
    const IgParams p = pc.c[cls];
    const int tile = (int)blockIdx.x - pc.first[cls];
    const int32_t *lst = act + pc.list_off[cls] + (size_t)tile * (p.Cin + 1);
    const int n_act = lst[0];
    if (n_act == 0) return;  // workgroup-uniform: nothing of this tile is needed
    if (tid < n_act) s_ch[tid] = lst[1 + tid];
    for (int kk = tid; kk < p.Kd; kk += 256) s_tab[kk] = dgrad_tab(p, kk);
    __syncthreads();
    if (n_act <= 32) conv_dgrad_act_body<1>(p, tile, s_ch, n_act, As, Bs, s_tab);
    else if (n_act <= 64) conv_dgrad_act_body<2>(p, tile, s_ch, n_act, As, Bs, s_tab);
    else if (n_act <= 96) conv_dgrad_act_body<3>(p, tile, s_ch, n_act, As, Bs, s_tab);
    else conv_dgrad_act_body<4>(p, tile, s_ch, n_act, As, Bs, s_tab);
}

extern "C" int lidog_conv2d_dgrad_sparse(const float *gy, const float *w, const int32_t *act, int32_t B, int32_t Cin,
                                         int32_t H, int32_t W, int32_t Cout, float *gx, float *ws, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(Cin >= 1 && Cin <= 128 && Cout % C2_KB == 0, "conv2d_dgrad_sparse: Cin <= 128, Cout % 32 == 0");
    LIDOG_REQUIRE(ws != nullptr, "conv2d_dgrad_sparse: needs a 9*Cin*Cout float workspace for the repacked weights");
    LIDOG_REQUIRE((int64_t)B * Cout * c2_out_dim(H) * c2_out_dim(W) < ((int64_t)1 << 31) &&
                      (int64_t)Cout * 4 * 8 <= 24576 && (int64_t)B * Cin * H * W < ((int64_t)1 << 31),
                  "conv2d_dgrad_sparse: tensor too large for 32-bit offsets / reduction table");
    ActLayout L = act_layout(B, Cin, H, W);
    lidog_launch_repack_dgrad_all(w, Cin, Cout, ws, st);   // conv2d.hip: the four classes' weight slabs, one launch
    IgParams cls_p[4];
    lidog_dgrad_classes(gy, ws, B, Cin, H, W, Cout, gx, cls_p);
    IgClasses pc = {};
    size_t tab = 0;
    for (int cls : {3, 1, 2, 0}) {
        const IgParams &p = cls_p[cls];
        if (p.Nj <= 0 || L.dgrad_tiles[cls] <= 0) continue;
        pc.c[pc.n] = p;
        pc.list_off[pc.n] = (long long)L.dgrad_off[cls];
        pc.first[pc.n + 1] = pc.first[pc.n] + (int)L.dgrad_tiles[cls];
        ++pc.n;
        if ((size_t)p.Kd * sizeof(int2) > tab) tab = (size_t)p.Kd * sizeof(int2);
    }
    if (pc.n > 0) k_conv_dgrad_act<<<(unsigned)pc.first[pc.n], 256, tab, st>>>(pc, act);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ WGRAD over the active pixel tiles of each channel group
// gW[co][(ci,tap)] = sum over pixels of gY[co][pixel] * X[ci][window(pixel) + tap].  Workgroup (g, co tile, split):
// the 9 * WA_GC columns of channel group g (padded to WA_NT MFMA tiles of 32) x 128 rows, accumulated over the
// pixel tiles of glists[g] that fall to this split, 32 pixels per LDS stage; splits are summed in order afterwards
// (no atomics).  A pixel tile in which none of the group's channels is active contributes exact zeros and is
// never visited.  Narrow groups skip more tiles but re-read gY once per group (WA_GC = 3: 41 % of the tiles, twice
// the gY traffic of the dense kernel, no faster; 7: 57 %, 1.2 x the traffic; 14: 69 %, 0.7 x).
#define WA_TPI 16  // pixel tiles per work item
#define WA_LDA 129
#define WA_LDB (32 * WA_NT + 1)
__global__ __launch_bounds__(256) void k_conv_wgrad_act(IgParams p, const int32_t *__restrict__ glists, int n_tiles,
                                                        int splits) {
    __shared__ float As[C2_KB * WA_LDA];
    __shared__ float Bs[C2_KB * WA_LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x, i0 = blockIdx.y * IG_T, sp = blockIdx.z;
    const int HoWo = p.Ho * p.Wo;
    const int32_t *gl = glists + (size_t)g * (n_tiles + 1);
    const int n_g = gl[0];
    // work item = WA_TPI consecutive entries of the group's tile list: equal work per workgroup whatever the
    // number of active tiles of the group (equal splits per group left the busiest groups 1.75 x the average)
    const int t_begin = sp * WA_TPI;
    if (sp > 0 && t_begin >= n_g) return;  // slab sp of this group is not summed (k_sum_group_splits)
    const int t_end = t_begin + WA_TPI < n_g ? t_begin + WA_TPI : n_g;
    const int nq = t_end > t_begin ? 4 * (t_end - t_begin) : 0;  // stages of 32 pixels
    const int kk = tid & 31, rg = tid >> 5;

    int cpk[4 * WA_NT];  // -1 = idle column
#pragma unroll
    for (int r = 0; r < 4 * WA_NT; ++r) {
        int j = rg + 8 * r;
        int ci = g * WA_GC + j / 9;
        cpk[r] = -1;
        if (j < 9 * WA_GC && ci < p.Cin) cpk[r] = wgrad_col(p, ci, j % 9);
    }
    unsigned a_mask = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) a_mask |= (unsigned)(i0 + rg + 8 * r < p.Mi) << r;

    WgradStage<4 * WA_NT> st;
    // tile ids are fetched one tile (four stages) ahead: the address chain list -> gY / X of a stage would
    // otherwise be two dependent memory latencies long, more than the MFMA phase it hides behind
    const int n_my = t_end - t_begin;
    int tile_cur = n_my > 0 ? gl[1 + t_begin] : 0;
    int tile_nxt = n_my > 1 ? gl[2 + t_begin] : tile_cur;
    auto load = [&](int q) {
        if ((q & 3) == 0 && q > 0) {
            tile_cur = tile_nxt;
            const int ahead = (q >> 2) + 1;
            tile_nxt = gl[1 + t_begin + (ahead < n_my ? ahead : n_my - 1)];
        }
        const int m = tile_cur * IG_T + (q & 3) * C2_KB + kk;
        const bool mv = m < p.Kd;
        const int mc = mv ? m : p.Kd - 1;
        const int pb = mc / HoWo, r_ = mc - pb * HoWo;
        const int yo = r_ / p.Wo, xo = r_ - yo * p.Wo;
        st.load(p, i0, a_mask, cpk, mv, pb, yo, xo, rg);
    };
    auto store = [&]() { st.store(&As[kk * WA_LDA + rg], &Bs[kk * WA_LDB + rg], a_mask); };

    const int li = lane & 31, kh = lane >> 5;
    f32x16 acc[1][WA_NT];
    mfma_stages<1, WA_NT, WA_LDA, WA_LDB>(acc, &As[kh * WA_LDA + 32 * wave + li], &Bs[kh * WA_LDB + li], nq, load,
                                          store);

#pragma unroll
    for (int t = 0; t < WA_NT; ++t) {
        const int j = 32 * t + li;
        const int ci = g * WA_GC + j / 9;
        if (j < 9 * WA_GC && ci < p.Cin) {
            float *d = p.D + (size_t)sp * p.Mi * p.Nj + (size_t)ci * 9 + j % 9;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                int i = i0 + 32 * wave + mfma_row(e, kh);
                if (i < p.Mi) d[(size_t)i * p.Nj] = acc[0][t][e];
            }
        }
    }
}

// gw[co][col] = sum of the slabs of the column's channel group, in order: ceil(n_g / WA_TPI) of them (at least one)
__global__ __launch_bounds__(256) void k_sum_group_splits(const float *__restrict__ partial, int64_t n, int Nj,
                                                          const int32_t *__restrict__ glists, int n_tiles,
                                                          float *__restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int col = (int)(i % Nj);
    const int g = col / (9 * WA_GC);
    int ns = (glists[(size_t)g * (n_tiles + 1)] + WA_TPI - 1) / WA_TPI;
    if (ns < 1) ns = 1;
    float acc = partial[i];
    for (int s = 1; s < ns; ++s) acc += partial[(size_t)s * n + i];
    out[i] = acc;
}

extern "C" int64_t lidog_conv2d_wgrad_sparse_ws(int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout) {
    ActLayout L = act_layout(B, Cin, H, W);
    int64_t splits = cdiv64(L.fwd_tiles, WA_TPI);
    return (splits < 1 ? 1 : splits) * (int64_t)Cout * Cin * 9;
}

extern "C" int lidog_conv2d_wgrad_sparse(const float *x, const float *gy, const int32_t *act, int32_t B, int32_t Cin,
                                         int32_t H, int32_t W, int32_t Cout, float *gw, float *ws, int64_t ws_floats,
                                         void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(Cin >= 1 && Cin <= 128 && Cout % 8 == 0, "conv2d_wgrad_sparse: Cin <= 128, Cout % 8 == 0");
    IgParams p = {};
    p.A = gy; p.Bm = x;
    p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout;
    p.Ho = c2_out_dim(H); p.Wo = c2_out_dim(W);
    p.Mi = Cout; p.Nj = Cin * 9; p.Kd = B * p.Ho * p.Wo;
    LIDOG_REQUIRE((int64_t)Cin * H * W < ((int64_t)1 << 27) && (int64_t)B * Cin * H * W < ((int64_t)1 << 31) &&
                      (int64_t)B * Cout * p.Ho * p.Wo < ((int64_t)1 << 31),
                  "conv2d_wgrad_sparse: tensor too large for the packed 32-bit offsets");
    const int64_t slab = (int64_t)p.Mi * p.Nj;
    if (p.Kd == 0) return hipMemsetAsync(gw, 0, sizeof(float) * slab, st) == hipSuccess ? 0 : 1;
    ActLayout L = act_layout(B, Cin, H, W);
    const int itiles = (int)cdiv64(p.Mi, IG_T);
    int splits = (int)cdiv64(L.fwd_tiles, WA_TPI);
    if (splits < 1) splits = 1;
    LIDOG_REQUIRE(ws != nullptr && (int64_t)splits * slab <= ws_floats,
                  "conv2d_wgrad_sparse: workspace too small (lidog_conv2d_wgrad_sparse_ws floats needed)");
    p.D = ws;
    dim3 grid((unsigned)L.groups, (unsigned)itiles, (unsigned)splits);
    k_conv_wgrad_act<<<grid, 256, 0, st>>>(p, act + L.glists_off, L.fwd_tiles, splits);
    k_sum_group_splits<<<(unsigned)cdiv64(slab, 256), 256, 0, st>>>(ws, slab, p.Nj, act + L.glists_off, L.fwd_tiles,
                                                                    gw);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// Matrix work the three support-restricted kernels EXECUTE for the lists in `act` (bench.py's `bev_mfma_frac`: executed
// FLOPs, not the dense-equivalent figure): out[0] forward, out[1] data gradient, out[2] weight gradient, in FLOPs.
//   forward: per pixel tile 2 * 128 pixels * Cout * (9 * active channels, padded to the 32-deep stage);
//   data gradient: per class tile 2 * 128 pixels * (active channels padded to a 32-row block) * Cout * taps of the class;
//   weight gradient: per (channel group, active pixel tile) 2 * 128 pixels * Cout * (WA_NT * 32 columns).
// Reads the list headers back (synchronises with `stream`): measurement only, never on the training path.
extern "C" int lidog_conv2d_support_work(const int32_t *act, int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout,
                                         double *out, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(act && out && Cin >= 1 && Cin <= 128, "conv2d_support_work: bad arguments");
    ActLayout L = act_layout(B, Cin, H, W);
    out[0] = out[1] = out[2] = 0.0;
    std::vector<int32_t> head;
    auto heads = [&](int64_t off, int tiles, int pitch) -> int {
        head.assign((size_t)(tiles > 0 ? tiles : 1), 0);
        if (tiles <= 0) return 0;
        LIDOG_CHECK_HIP(hipMemcpy2DAsync(head.data(), sizeof(int32_t), act + off, (size_t)pitch * sizeof(int32_t),
                                         sizeof(int32_t), (size_t)tiles, hipMemcpyDeviceToHost, st));
        LIDOG_CHECK_HIP(hipStreamSynchronize(st));
        return 0;
    };
    if (int rc = heads(L.fwd_off, L.fwd_tiles, Cin + 1)) return rc;
    for (int t = 0; t < L.fwd_tiles; ++t) {
        const int Kp = (head[t] * 9 + C2_KB - 1) / C2_KB * C2_KB;
        out[0] += 2.0 * IG_T * Cout * Kp;
    }
    for (int cls = 0; cls < 4; ++cls) {
        const int nt = ((cls >> 1) ? 2 : 1) * ((cls & 1) ? 2 : 1);
        if (int rc = heads(L.dgrad_off[cls], L.dgrad_tiles[cls], Cin + 1)) return rc;
        for (int t = 0; t < L.dgrad_tiles[cls]; ++t)
            out[1] += 2.0 * IG_T * ((head[t] + 31) / 32 * 32) * (double)Cout * nt;
    }
    if (int rc = heads(L.glists_off, L.groups, L.fwd_tiles + 1)) return rc;
    for (int g = 0; g < L.groups; ++g) out[2] += 2.0 * IG_T * (double)head[g] * Cout * (WA_NT * 32);
    return 0;
}
