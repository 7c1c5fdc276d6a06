// Dense 2-D BEV head on the matrix cores: implicit-GEMM convolution forward / data gradient /
// weight gradient with exact-f32 MFMA (v_mfma_f32_32x32x2_f32: bit-for-bit an fmaf chain).
// Reference: Encoder2D = Conv2d(k3,s2,p1,bias=False) x2 + Conv2d(k1) (utils/models/conv2d.py:16-22,
// 116,184-185), NCHW float32.  CPU checker: oracle/ref_torch.py:Encoder2DRef (torch CPU conv).
//
// Every kernel computes D[i][j] = sum_k A(i,k) * B(k,j) on 128x128 (or 96x128) tiles, 32-deep LDS stages,
// 4 waves x MFMA 32x32 tiles.  j always runs over pixels so that the D columns (MFMA lane
// dimension) are contiguous in NCHW memory:
//   FWD    i = co, k = (ci,ky,kx), j = (b,yo,xo)   A = W[co][k]            B = im2col(X)
//   DGRAD  i = ci, k = (co,tap),   j = class pixel  A = Wd[class][ci][k]   B = gathered gY   (4 stride-2
//          parity classes, each with only its 1/2/2/4 contributing taps -> no wasted FLOPs)
//   WGRAD  i = co, k = (b,yo,xo),  j = (ci,ky,kx)   A = gY[co][k]          B = im2col(X)^T, split over k
#include "common.h"
#include "clock_stamp.h"

#include "conv2d.h"

// ------------------------------------------------------------------ WGRAD
// D[co][(ci,ky,kx)] = sum over pixels k = (b,yo,xo) of gY[co][k] * X[ci][2yo-1+ky][2xo-1+kx], split over k.
// 128 x 128 tile, 32 pixels per stage.  Thread (kk = tid & 31, rg = tid >> 5) stages pixel kk of 16 gY rows
// and 16 im2col columns; its (ci,ky,kx) columns are fixed for the whole kernel (packed offset + tap), its pixel
// advances by 32 per stage with adds only.  Loads are unconditional (invalid taps read element 0) and zeroed
// when the stage is written to LDS; LDS row pitch 129 makes the transposing stores conflict-free.
#define WG_LD 129
__global__ __launch_bounds__(256) void k_conv_wgrad(IgParams p) {
    __shared__ float As[C2_KB * WG_LD];
    __shared__ float Bs[C2_KB * WG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.y * IG_T, j0 = blockIdx.x * IG_T;
    const int HoWo = p.Ho * p.Wo;
    const int k_begin = blockIdx.z * p.k_chunk;
    const int k_end = k_begin + p.k_chunk < p.Kd ? k_begin + p.k_chunk : p.Kd;
    const int kk = tid & 31, rg = tid >> 5;

    int cpk[16];  // -1 past Nj
    unsigned a_mask = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        int j = j0 + rg + 8 * r;
        cpk[r] = -1;
        int ci = j / 9;
        if (j < p.Nj) cpk[r] = wgrad_col(p, ci, j - ci * 9);
        a_mask |= (unsigned)(i0 + rg + 8 * r < p.Mi) << r;
    }
    // pixel of this thread in the current stage (clamped to the last pixel once past the end)
    int m = k_begin + kk;
    int pb, yo, xo;
    {
        int mc = m < p.Kd ? m : p.Kd - 1;
        pb = mc / HoWo;
        int r_ = mc - pb * HoWo;
        yo = r_ / p.Wo;
        xo = r_ - yo * p.Wo;
    }

    WgradStage<16> st;
    // stage s > 0: step the pixel 32 on first (past the end: the last prefetch stages pixels with mv false)
    auto load = [&](int s) {
        if (s > 0) {
            m += C2_KB;
            if (m < p.Kd) {
                xo += C2_KB;
                while (xo >= p.Wo) {
                    xo -= p.Wo;
                    ++yo;
                }
                while (yo >= p.Ho) {
                    yo -= p.Ho;
                    ++pb;
                }
            }
        }
        st.load(p, i0, a_mask, cpk, m < k_end, pb, yo, xo, rg);
    };
    auto store = [&]() { st.store(&As[kk * WG_LD + rg], &Bs[kk * WG_LD + rg], a_mask); };

    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    const int li = lane & 31, kh = lane >> 5;
    f32x16 acc[2][2];
    mfma_stages<2, 2, WG_LD, WG_LD>(acc, &As[kh * WG_LD + wi + li], &Bs[kh * WG_LD + wj + li],
                                    (k_end - k_begin + C2_KB - 1) / C2_KB, load, store);

#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        int j = j0 + wj + 32 * tj + li;
        if (j >= p.Nj) continue;
        float *d = p.D + (size_t)blockIdx.z * p.Mi * p.Nj + j;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                int i = i0 + wi + 32 * ti + mfma_row(e, kh);
                if (i < p.Mi) d[(size_t)i * p.Nj] = acc[ti][tj][e];
            }
        }
    }
}

// ------------------------------------------------------------------ FWD / DGRAD, table-driven
// Same 128-pixel-wide tiles as k_igemm with 32-deep stages, built so that a stage costs ~150 instructions per
// wave besides its MFMAs (the first version spent ~530 on reduction-index arithmetic, as long as the MFMA phase):
//  - the reduction index kk -> (address offset, tap) map is computed once per workgroup into an LDS table;
//    per staged element only a table read, a tap-validity bit test (per-lane 9-bit / 4-bit mask), one add
//    and one select remain; all offsets are 32-bit;
//  - invalid taps load a known-good address; they (and rows past Mi) are zeroed when the stage is written to
//    LDS, not after the load;
//  - the LDS operand reads of MFMA step k2+1 are issued before the MFMAs of step k2 (mfma_stages).
// WM x (4/WM) waves, each TI x TJ MFMA tiles: 128 x 128 (WM=2,TI=2,TJ=2) or 96 x 128 (WM=1,TI=3,TJ=1; the
// data gradient of a 96-channel input would waste a quarter of a 128-row tile).
template <int MODE, int WM, int TI, int TJ>
__device__ __forceinline__ void conv_s2_tile(const IgParams &p, const int bx, const int by, float *__restrict__ As,
                                             float *__restrict__ Bs) {
    constexpr int TMR = WM * TI * 32;              // tile rows (i)
    constexpr int AV = (TMR * C2_KB / 4) / 256;    // float4 of A per thread per stage
    static_assert((4 / WM) * TJ * 32 == IG_T, "tile is 128 pixels wide");
    static_assert((TMR * C2_KB / 4) % 256 == 0, "A stage must divide over the threads");
    extern __shared__ int2 s_tab[];  // [Kd] (offset, tap)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = by * TMR, j0 = bx * IG_T;
    const int HoWo = p.Ho * p.Wo, HW = p.H * p.W;
    const int kw = __builtin_amdgcn_readfirstlane(tid >> 7);

    for (int kk = tid; kk < p.Kd; kk += 256) {
        if (MODE == IG_FWD) {
            int ci = kk / 9, t = kk - ci * 9;
            int ty = t / 3, tx = t - ty * 3;
            s_tab[kk] = make_int2(ci * HW + (ty - 1) * p.W + (tx - 1), t);
        } else {
            s_tab[kk] = dgrad_tab(p, kk);
        }
    }

    const int j = j0 + (tid & 127);
    const PixelTaps px = MODE == IG_FWD ? fwd_pixel(p, j) : dgrad_pixel(p, j);

    // ---- the A rows this thread stages
    const float *a_ptr[AV];
    bool a_ok[AV];
#pragma unroll
    for (int v = 0; v < AV; ++v) {
        int i = i0 + 32 * v + (tid >> 3);
        a_ok[v] = i < p.Mi;
        a_ptr[v] = p.A + (size_t)(a_ok[v] ? i : p.Mi - 1) * p.Kd + (tid & 7) * 4;
    }
    __syncthreads();  // table complete

    float4 ra[AV];
    GatherB gb;
    auto load = [&](int s) {
        const int k0 = s * C2_KB;
#pragma unroll
        for (int v = 0; v < AV; ++v) ra[v] = *reinterpret_cast<const float4 *>(a_ptr[v] + k0);
        gb.load(p.Bm, &s_tab[k0 + kw], px);
    };
    auto store = [&]() {
        store_a_rows(As, ra, a_ok, tid);
        gb.store(&Bs[kw * IG_LD + (tid & 127)]);
    };

    const int wi = (WM == 1 ? 0 : (wave >> 1)) * (TI * 32), wj = (WM == 1 ? wave : (wave & 1)) * (TJ * 32);
    const int li = lane & 31, kh = lane >> 5;
    f32x16 acc[TI][TJ];
    mfma_stages<TI, TJ, IG_LD, IG_LD>(acc, &As[kh * IG_LD + wi + li], &Bs[kh * IG_LD + wj + li], p.Kd / C2_KB, load,
                                      store);

#pragma unroll
    for (int tj = 0; tj < TJ; ++tj) {
        int jo = j0 + wj + 32 * tj + li;
        if (jo >= p.Nj) continue;
        size_t col_off, i_stride;
        if (MODE == IG_FWD) {
            int b = jo / HoWo;
            col_off = (size_t)b * p.Cout * HoWo + (jo - b * HoWo);
            i_stride = HoWo;
        } else {
            col_off = dgrad_pixel_offset(p, jo);
            i_stride = HW;
        }
#pragma unroll
        for (int ti = 0; ti < TI; ++ti) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                int i = i0 + wi + 32 * ti + mfma_row(e, kh);
                if (i < p.Mi) p.D[col_off + (size_t)i * i_stride] = acc[ti][tj][e];
            }
        }
    }
}

// One launch over up to four problems (the stride-2 parity classes of a data gradient, longest reduction first) or one
// (forward): workgroup x -> (class, pixel tile, row tile) with the row tiles of a pixel tile next to each other (the
// second one finds the gathered pixels in L2).  Four launches of 1 744 / 1 734 / 1 734 / 1 724 equal workgroups on 512
// slots were 3.4 rounds each, i.e. four with the last one 40 % full; one launch with the 4-tap class first lets the short
// classes fill the long one's tail.
// (Tried and dropped, round 5: the forward pass's pixel tiles behind the last full round of 128-row workgroups as 64-row
// workgroups in the same launch -- 1 536 + 416 half-sized instead of 1 744 equal ones on 512 slots: 46.79 vs 46.80 ms.)
template <int MODE, int WM, int TI, int TJ>
__global__ __launch_bounds__(256) void k_conv_s2(IgClasses pc) {
    __shared__ float As[C2_KB * IG_LD];
    __shared__ float Bs[C2_KB * IG_LD];
    const int x = blockIdx.x;
    int cls = 0;
    while (cls + 1 < pc.n && x >= pc.first[cls + 1]) ++cls;
    const IgParams p = pc.c[cls];
    const int r = x - pc.first[cls];
    const int rt = pc.row_tiles[cls];
    LIDOG_STAMP_BEGIN()
    conv_s2_tile<MODE, WM, TI, TJ>(p, r / rt, r % rt, As, Bs);
    LIDOG_STAMP_END()
}

// ------------------------------------------------------------------ weight repack for DGRAD
// Wd[ci][co*nt + tap] = W[co][ci][ky(tap)][kx(tap)] per parity class;
// all four parity classes (py, px) in one launch: class cls = 2 py + px owns nt = (py ? 2 : 1) (px ? 2 : 1) taps and the
// slab behind the classes before it (Cin * Cout * {0, 1, 3, 5} floats) -- four launches of a few microseconds each sat
// between the data-gradient kernels of every 3x3 convolution
__global__ __launch_bounds__(256) void k_repack_dgrad_all(const float *__restrict__ W, int Cin, int Cout,
                                                          float *__restrict__ Wd) {
    const int64_t cc = (int64_t)Cin * Cout;
    int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 9 * cc) return;
    const int cls = e < cc ? 0 : e < 3 * cc ? 1 : e < 5 * cc ? 2 : 3;
    const int64_t base = cls == 0 ? 0 : cls == 1 ? cc : cls == 2 ? 3 * cc : 5 * cc;
    const int py = cls >> 1, px = cls & 1;
    const int nky = py ? 2 : 1, nkx = px ? 2 : 1, ky0 = py ? 0 : 1, kx0 = px ? 0 : 1, nt = nky * nkx;
    const int64_t l = e - base;
    int kd = (int)(l % ((int64_t)Cout * nt));
    int ci = (int)(l / ((int64_t)Cout * nt));
    int co = kd / nt, tap = kd % nt;
    int ky = ky0 + (tap / nkx) * 2, kx = kx0 + (tap % nkx) * 2;
    Wd[e] = W[(((size_t)co * Cin + ci) * 3 + ky) * 3 + kx];
}

void lidog_launch_repack_dgrad_all(const float *W, int Cin, int Cout, float *Wd, hipStream_t st) {
    const int64_t total = 9 * (int64_t)Cin * Cout;
    k_repack_dgrad_all<<<(unsigned)cdiv64(total, 256), 256, 0, st>>>(W, Cin, Cout, Wd);
}

__global__ __launch_bounds__(256) void k_sum_splits(const float *__restrict__ partial, int64_t n, int splits,
                                                    int64_t stride, float *__restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float acc = partial[i];
    for (int s = 1; s < splits; ++s) acc += partial[(size_t)s * stride + i];
    out[i] = acc;
}

// ------------------------------------------------------------------ 1x1 convolution with few outputs (OutConv 256 -> 7)
#define PW_MAXCO 8
__global__ __launch_bounds__(256) void k_pw_fwd(const float *__restrict__ X, const float *__restrict__ W,
                                                const float *__restrict__ bias, int Cin, int Cout, int64_t HW,
                                                int64_t total, float *__restrict__ Y) {
    int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (b, pixel)
    if (e >= total) return;
    int64_t b = e / HW, pix = e - b * HW;
    float acc[PW_MAXCO];
#pragma unroll
    for (int co = 0; co < PW_MAXCO; ++co) acc[co] = 0.f;
    const float *x = X + (size_t)b * Cin * HW + pix;
    for (int ci = 0; ci < Cin; ++ci) {
        float v = x[(size_t)ci * HW];
#pragma unroll
        for (int co = 0; co < PW_MAXCO; ++co)
            if (co < Cout) acc[co] = __builtin_fmaf(v, W[co * Cin + ci], acc[co]);
    }
#pragma unroll
    for (int co = 0; co < PW_MAXCO; ++co)
        if (co < Cout) Y[((size_t)b * Cout + co) * HW + pix] = acc[co] + (bias ? bias[co] : 0.f);
}

__global__ __launch_bounds__(256) void k_pw_dgrad(const float *__restrict__ gY, const float *__restrict__ W, int Cin,
                                                  int Cout, int64_t HW, int64_t total, float *__restrict__ gX) {
    int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    int64_t b = e / HW, pix = e - b * HW;
    float g[PW_MAXCO];
#pragma unroll
    for (int co = 0; co < PW_MAXCO; ++co) g[co] = (co < Cout) ? gY[((size_t)b * Cout + co) * HW + pix] : 0.f;
    for (int ci = 0; ci < Cin; ++ci) {
        float acc = 0.f;
#pragma unroll
        for (int co = 0; co < PW_MAXCO; ++co)
            if (co < Cout) acc = __builtin_fmaf(g[co], W[co * Cin + ci], acc);
        gX[((size_t)b * Cin + ci) * HW + pix] = acc;
    }
}

// gW[co][ci] = sum_{b,pix} gY[b][co][pix] * X[b][ci][pix], gbias[co] = sum gY[b][co][pix].
// Block (ci, s): slice s = (image b, quarter of its pixels); partial[s][co*Cin + ci] (and partial[s][Cout*Cin + co]
// from the ci == 0 blocks) in double per block, summed over s in order by k_sum_splits: no atomics.
#define PW_QUARTERS 4
__global__ __launch_bounds__(256) void k_pw_wgrad(const float *__restrict__ X, const float *__restrict__ gY, int Cin,
                                                  int Cout, int HW, float *__restrict__ partial) {
    __shared__ double red[2 * PW_MAXCO][4];
    const int ci = blockIdx.x, s = blockIdx.y;
    const int b = s / PW_QUARTERS, q = s % PW_QUARTERS;
    const int chunk = (HW + PW_QUARTERS - 1) / PW_QUARTERS;
    const int e0 = q * chunk, e1 = e0 + chunk < HW ? e0 + chunk : HW;
    const float *x = X + ((size_t)b * Cin + ci) * HW;
    const float *g = gY + (size_t)b * Cout * HW;
    double acc[PW_MAXCO], accb[PW_MAXCO];
#pragma unroll
    for (int co = 0; co < PW_MAXCO; ++co) { acc[co] = 0; accb[co] = 0; }
    for (int e = e0 + threadIdx.x; e < e1; e += 256) {
        float xv = x[e];
#pragma unroll
        for (int co = 0; co < PW_MAXCO; ++co)
            if (co < Cout) {
                float gv = g[(size_t)co * HW + e];
                acc[co] += (double)gv * (double)xv;
                accb[co] += (double)gv;
            }
    }
#pragma unroll
    for (int co = 0; co < PW_MAXCO; ++co) {
        double a = acc[co], bsum = accb[co];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { a += __shfl_down(a, d); bsum += __shfl_down(bsum, d); }
        if ((threadIdx.x & 63) == 0) { red[co][threadIdx.x >> 6] = a; red[PW_MAXCO + co][threadIdx.x >> 6] = bsum; }
    }
    __syncthreads();
    if (threadIdx.x < Cout) {
        int co = threadIdx.x;
        float *dst = partial + (size_t)s * (Cout * Cin + Cout);
        dst[co * Cin + ci] = (float)(red[co][0] + red[co][1] + red[co][2] + red[co][3]);
        if (ci == 0)
            dst[Cout * Cin + co] = (float)(red[PW_MAXCO + co][0] + red[PW_MAXCO + co][1] + red[PW_MAXCO + co][2] +
                                           red[PW_MAXCO + co][3]);
    }
}

// ------------------------------------------------------------------ C ABI
void lidog_dgrad_classes(const float *gy, const float *Wd, int B, int Cin, int H, int W, int Cout, float *gx,
                         IgParams cls[4]) {
    const float *slab = Wd;
    for (int c = 0; c < 4; ++c) {
        IgParams &p = cls[c];
        p = IgParams{};
        p.Bm = gy; p.D = gx;
        p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout; p.Ho = c2_out_dim(H); p.Wo = c2_out_dim(W);
        p.py = c >> 1; p.px = c & 1;
        // y + 1 - ky even: y even -> ky = 1; y odd -> ky in {0, 2}
        p.nky = p.py ? 2 : 1; p.ky0 = p.py ? 0 : 1;
        p.nkx = p.px ? 2 : 1; p.kx0 = p.px ? 0 : 1;
        p.Hc = (H - p.py + 1) / 2; p.Wc = (W - p.px + 1) / 2;
        const int nt = p.nky * p.nkx;
        p.Mi = Cin; p.Nj = B * p.Hc * p.Wc; p.Kd = Cout * nt;
        p.A = slab;
        slab += (int64_t)Cin * Cout * nt;
    }
}

extern "C" int lidog_conv2d_fwd(const float *x, const float *w, const float *bias, int32_t B, int32_t Cin, int32_t H,
                                int32_t W, int32_t Cout, int32_t ksize, int32_t stride, int32_t pad, float *y,
                                void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (ksize == 1) {
        LIDOG_REQUIRE(stride == 1 && pad == 0 && Cout <= PW_MAXCO, "conv2d_fwd: 1x1 path needs stride 1, Cout <= 8");
        int64_t HW = (int64_t)H * W, total = (int64_t)B * HW;
        if (total) k_pw_fwd<<<(unsigned)cdiv64(total, 256), 256, 0, st>>>(x, w, bias, Cin, Cout, HW, total, y);
        LIDOG_LAUNCH_CHECK();
        return 0;
    }
    LIDOG_REQUIRE(ksize == 3 && stride == 2 && pad == 1 && bias == nullptr,
                  "conv2d_fwd: MFMA path implements k3 s2 p1 without bias (Encoder2D)");
    LIDOG_REQUIRE((Cin * 9) % C2_KB == 0, "conv2d_fwd: Cin*9 must be a multiple of 32");
    IgParams p = {};
    p.A = w; p.Bm = x; p.D = y;
    p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout;
    p.Ho = c2_out_dim(H); p.Wo = c2_out_dim(W);
    p.Mi = Cout; p.Nj = B * p.Ho * p.Wo; p.Kd = Cin * 9;
    if (p.Nj == 0) return 0;
    LIDOG_REQUIRE((int64_t)B * Cin * H * W < ((int64_t)1 << 31) && (int64_t)p.Kd * 8 <= 24576,
                  "conv2d_fwd: tensor too large for 32-bit offsets / reduction table");
    IgClasses pc = {};
    pc.c[0] = p;
    pc.n = 1;
    pc.row_tiles[0] = (int)cdiv64(p.Mi, IG_T);
    pc.first[1] = (int)cdiv64(p.Nj, IG_T) * pc.row_tiles[0];
    k_conv_s2<IG_FWD, 2, 2, 2><<<(unsigned)pc.first[pc.n], 256, (size_t)p.Kd * sizeof(int2), st>>>(pc);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_conv2d_dgrad(const float *gy, const float *w, int32_t B, int32_t Cin, int32_t H, int32_t W,
                                  int32_t Cout, int32_t ksize, int32_t stride, int32_t pad, float *gx, float *ws,
                                  void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (ksize == 1) {
        LIDOG_REQUIRE(stride == 1 && pad == 0 && Cout <= PW_MAXCO, "conv2d_dgrad: 1x1 path needs stride 1, Cout <= 8");
        int64_t HW = (int64_t)H * W, total = (int64_t)B * HW;
        if (total) k_pw_dgrad<<<(unsigned)cdiv64(total, 256), 256, 0, st>>>(gy, w, Cin, Cout, HW, total, gx);
        LIDOG_LAUNCH_CHECK();
        return 0;
    }
    LIDOG_REQUIRE(ksize == 3 && stride == 2 && pad == 1, "conv2d_dgrad: MFMA path implements k3 s2 p1");
    LIDOG_REQUIRE(ws != nullptr, "conv2d_dgrad: needs a 9*Cin*Cout float workspace for the repacked weights");
    LIDOG_REQUIRE(Cout % C2_KB == 0, "conv2d_dgrad: Cout must be a multiple of 32");
    LIDOG_REQUIRE((int64_t)B * Cout * c2_out_dim(H) * c2_out_dim(W) < ((int64_t)1 << 31) &&
                      (int64_t)Cout * 4 * 8 <= 24576,
                  "conv2d_dgrad: tensor too large for 32-bit offsets / reduction table");
    lidog_launch_repack_dgrad_all(w, Cin, Cout, ws, st);
    const bool rows96 = Cin % 128 != 0 && Cin % 96 == 0;   // 96-row tiles: no idle quarter of a 128-row tile
    IgClasses pc = {};
    IgParams cls_p[4];
    lidog_dgrad_classes(gy, ws, B, Cin, H, W, Cout, gx, cls_p);
    // longest reduction first: (py, px) = (1, 1) has four taps, (0, 1) and (1, 0) two, (0, 0) one
    const int rt = rows96 ? Cin / 96 : (int)cdiv64(Cin, IG_T);
    size_t tab = 0;
    for (int cls : {3, 1, 2, 0}) {
        const IgParams &p = cls_p[cls];
        if (p.Nj <= 0) continue;
        pc.c[pc.n] = p;
        pc.row_tiles[pc.n] = rt;
        pc.first[pc.n + 1] = pc.first[pc.n] + (int)cdiv64(p.Nj, IG_T) * rt;
        ++pc.n;
        if ((size_t)p.Kd * sizeof(int2) > tab) tab = (size_t)p.Kd * sizeof(int2);
    }
    if (pc.n > 0) {
        if (rows96) k_conv_s2<IG_DGRAD, 1, 3, 1><<<(unsigned)pc.first[pc.n], 256, tab, st>>>(pc);
        else k_conv_s2<IG_DGRAD, 2, 2, 2><<<(unsigned)pc.first[pc.n], 256, tab, st>>>(pc);
    }
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_conv2d_wgrad(const float *x, const float *gy, int32_t B, int32_t Cin, int32_t H, int32_t W,
                                  int32_t Cout, int32_t ksize, int32_t stride, int32_t pad, float *gw, float *gbias,
                                  float *ws, int64_t ws_floats, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (ksize == 1) {
        LIDOG_REQUIRE(stride == 1 && pad == 0 && Cout <= PW_MAXCO, "conv2d_wgrad: 1x1 path needs stride 1, Cout <= 8");
        const int splits = B * PW_QUARTERS;
        const int64_t slab = (int64_t)Cout * Cin + Cout;
        LIDOG_REQUIRE(ws != nullptr && ws_floats >= splits * slab,
                      "conv2d_wgrad: 1x1 path needs a workspace of %lld floats", (long long)(splits * slab));
        LIDOG_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "conv2d_wgrad: image too large");
        if (B == 0 || H * W == 0) return 0;
        k_pw_wgrad<<<dim3((unsigned)Cin, (unsigned)splits), 256, 0, st>>>(x, gy, Cin, Cout, H * W, ws);
        k_sum_splits<<<(unsigned)cdiv64((int64_t)Cout * Cin, 256), 256, 0, st>>>(ws, (int64_t)Cout * Cin, splits, slab, gw);
        if (gbias) k_sum_splits<<<1, 256, 0, st>>>(ws + (int64_t)Cout * Cin, Cout, splits, slab, gbias);
        LIDOG_LAUNCH_CHECK();
        return 0;
    }
    LIDOG_REQUIRE(ksize == 3 && stride == 2 && pad == 1 && gbias == nullptr, "conv2d_wgrad: MFMA path implements k3 s2 p1");
    IgParams p = {};
    p.A = gy; p.Bm = x;
    p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout;
    p.Ho = c2_out_dim(H); p.Wo = c2_out_dim(W);
    p.Mi = Cout; p.Nj = Cin * 9; p.Kd = B * p.Ho * p.Wo;
    int64_t slab = (int64_t)p.Mi * p.Nj;
    int tiles = (int)(cdiv64(p.Nj, IG_T) * cdiv64(p.Mi, IG_T));
    // two full rounds of the chip's slots (211 registers: two workgroups per CU, 512 slots on 256 CUs), never a few
    // workgroups more: 36 tiles x 29 splits = 1 044 workgroups ran a third round for the last 20 (round 5)
    int splits = 1024 / tiles;
    if (splits < 1) splits = 1;
    LIDOG_REQUIRE(Cout % 8 == 0, "conv2d_wgrad: Cout must be a multiple of 8");
    LIDOG_REQUIRE((int64_t)Cin * H * W < ((int64_t)1 << 27) && (int64_t)B * Cin * H * W < ((int64_t)1 << 31) &&
                      (int64_t)B * Cout * p.Ho * p.Wo < ((int64_t)1 << 31),
                  "conv2d_wgrad: tensor too large for the packed 32-bit offsets");
    int64_t max_by_k = cdiv64(p.Kd, 4 * C2_KB);
    if (splits > max_by_k) splits = (int)(max_by_k < 1 ? 1 : max_by_k);
    if ((int64_t)splits * slab > ws_floats) splits = (int)(ws_floats / slab);
    LIDOG_REQUIRE(splits >= 1, "conv2d_wgrad: workspace too small (%lld floats needed per split)", (long long)slab);
    p.k_chunk = (int)(cdiv64(cdiv64(p.Kd, splits), C2_KB) * C2_KB);
    splits = (int)cdiv64(p.Kd, p.k_chunk);
    p.D = (splits == 1) ? gw : ws;
    dim3 grid((unsigned)cdiv64(p.Nj, IG_T), (unsigned)cdiv64(p.Mi, IG_T), (unsigned)splits);
    k_conv_wgrad<<<grid, 256, 0, st>>>(p);
    if (splits > 1) k_sum_splits<<<(unsigned)cdiv64(slab, 256), 256, 0, st>>>(ws, slab, splits, slab, gw);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
