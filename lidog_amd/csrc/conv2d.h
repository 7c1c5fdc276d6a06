// Shared by conv2d.hip (dense implicit-GEMM kernels) and conv2d_sparse.hip (structurally sparse input): the parameter
// blocks, the exact-f32 MFMA stage pipeline and the pixel / gather pieces every Conv2d(k3, s2, p1) kernel uses.
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define IG_T 128
#define IG_LD 132
#define C2_KB 32  // reduction depth of one LDS stage

struct IgParams {
    const float *A;   // FWD: W [Cout][Cin*9]; DGRAD: Wd class slab [Cin][Cout*nt]; WGRAD: gY
    const float *Bm;  // FWD/WGRAD: X; DGRAD: gY
    float *D;         // FWD: Y; DGRAD: gX; WGRAD: partial slab [split][Cout][Cin*9]
    int Cin, H, W, Cout, Ho, Wo;
    int Mi, Nj, Kd;   // GEMM extents
    // DGRAD class description
    int py, px, nky, nkx, Hc, Wc;
    int ky0, kx0;
    // WGRAD split
    int k_chunk;
};

enum { IG_FWD = 0, IG_DGRAD = 1, IG_WGRAD = 2 };

// up to four problems in one launch (the stride-2 parity classes of a data gradient, longest reduction first)
struct IgClasses {
    IgParams c[4];
    int first[5];            // first workgroup of every class; first[n] = grid size
    int n;
    int row_tiles[4];        // row tiles of a pixel tile (next to each other in the grid)
    long long list_off[4];   // sparse data gradient: the class's tile lists inside the activity buffer (int32 units)
};

// output extent of a 3x3 stride-2 pad-1 convolution over n input pixels
static inline int c2_out_dim(int n) { return (n + 2 - 3) / 2 + 1; }

// Wd = the data-gradient weight slabs of the four stride-2 parity classes of a 3x3 kernel W [Cout][Cin][3][3], in class
// order (9 Cin Cout floats), one launch (conv2d.hip)
void lidog_launch_repack_dgrad_all(const float *W, int Cin, int Cout, float *Wd, hipStream_t st);

// cls[c] = the data-gradient problem of parity class c = 2 py + px (input pixels (2 yc + py, 2 xc + px)), reading its
// weights from its slab of Wd as lidog_launch_repack_dgrad_all lays them out (conv2d.hip)
void lidog_dgrad_classes(const float *gy, const float *Wd, int B, int Cin, int H, int W, int Cout, float *gx,
                         IgParams cls[4]);

// ------------------------------------------------------------------ the stage pipeline
// acc[TI][TJ] = sum over n_stages LDS stages of C2_KB reduction rows of A^T B, in k order (bit-for-bit an fmaf chain).
// Per stage: store() writes the registers staged by the previous load() to LDS, load(s) fetches the next stage
// (the last stage re-loads itself), then C2_KB / 2 steps of TI x TJ v_mfma_f32_32x32x2_f32 with the LDS operand reads
// of step k2 + 1 issued before the MFMAs of step k2.  load(0) is issued even when n_stages is 0 (ahead of the branch,
// the prefetch loads need one wait before the first store instead of one per value): like the last stage's prefetch
// it is never stored, but every load() must stay inside the buffers.
// a_rd / b_rd: this lane's column of the wave's first A / B tile at reduction row lane >> 5; tile a / b lies 32 a /
// 32 b columns further; LDA / LDB are the LDS row pitches.
template <int TI, int TJ, int LDA, int LDB, typename Load, typename Store>
__device__ __forceinline__ void mfma_stages(f32x16 (&acc)[TI][TJ], const float *a_rd, const float *b_rd, int n_stages,
                                            Load &&load, Store &&store) {
#pragma unroll
    for (int a = 0; a < TI; ++a)
#pragma unroll
        for (int b = 0; b < TJ; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
    load(0);
    for (int s = 0; s < n_stages; ++s) {
        __syncthreads();
        store();
        __syncthreads();
        load(s + 1 < n_stages ? s + 1 : s);
        float af[TI], bf[TJ], an[TI], bn[TJ];
#pragma unroll
        for (int a = 0; a < TI; ++a) af[a] = a_rd[32 * a];
#pragma unroll
        for (int b = 0; b < TJ; ++b) bf[b] = b_rd[32 * b];
#pragma unroll
        for (int k2 = 0; k2 < C2_KB / 2; ++k2) {
            if (k2 + 1 < C2_KB / 2) {
#pragma unroll
                for (int a = 0; a < TI; ++a) an[a] = a_rd[(2 * k2 + 2) * LDA + 32 * a];
#pragma unroll
                for (int b = 0; b < TJ; ++b) bn[b] = b_rd[(2 * k2 + 2) * LDB + 32 * b];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int a = 0; a < TI; ++a)
#pragma unroll
                for (int b = 0; b < TJ; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a], bf[b], acc[a][b], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (k2 + 1 < C2_KB / 2) {
#pragma unroll
                for (int a = 0; a < TI; ++a) af[a] = an[a];
#pragma unroll
                for (int b = 0; b < TJ; ++b) bf[b] = bn[b];
            }
        }
    }
}

// D layout of the 32x32 MFMA: element e of lane (li, kh = lane >> 5) is row mfma_row(e, kh), column li of the tile
__device__ __forceinline__ int mfma_row(int e, int kh) { return (e & 3) + 8 * (e >> 2) + 4 * kh; }

// S[STEP r] = v[r] where bit r of ok is set, else 0: staged registers go to LDS, invalid taps and rows zeroed here
// rather than after the load (a select right behind a load makes the wave wait for it before its MFMA phase)
template <int STEP, int N>
__device__ __forceinline__ void store_masked(float *S, const float (&v)[N], unsigned ok) {
#pragma unroll
    for (int r = 0; r < N; ++r) S[STEP * r] = ((ok >> r) & 1u) ? v[r] : 0.f;
}

// ------------------------------------------------------------------ FWD / DGRAD: one pixel per lane
// The lane's pixel j (fixed for the whole kernel): 32-bit element offsets of its first tap (`base`) and of a
// known-good address (`safe`), and its tap-validity mask (0 past Nj)
struct PixelTaps {
    int base, safe;
    unsigned mask;
};

// forward: output pixel j = (b, yo, xo); base = safe = the centre tap (always inside the image); 9-bit mask (ty, tx)
__device__ __forceinline__ PixelTaps fwd_pixel(const IgParams &p, int j) {
    const bool jvalid = j < p.Nj;
    const int jj = jvalid ? j : 0;
    const int HoWo = p.Ho * p.Wo;
    const int pb = jj / HoWo, r = jj - pb * HoWo;
    const int yo = r / p.Wo, xo = r - yo * p.Wo;
    PixelTaps t;
    t.base = pb * p.Cin * p.H * p.W + (2 * yo) * p.W + 2 * xo;
    t.safe = t.base;
    t.mask = 0;
#pragma unroll
    for (int ty = 0; ty < 3; ++ty)
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
            int y = 2 * yo - 1 + ty, x = 2 * xo - 1 + tx;
            t.mask |= (unsigned)(y >= 0 && y < p.H && x >= 0 && x < p.W) << (ty * 3 + tx);
        }
    if (!jvalid) t.mask = 0;
    return t;
}

// data gradient: pixel j = (b, yc, xc) of the class; base = the gY pixel of the class's first tap (y0 - ty, x0 - tx for
// the later ones), safe = gY[b][0][0][0]; 4-bit mask over (ty, tx)
__device__ __forceinline__ PixelTaps dgrad_pixel(const IgParams &p, int j) {
    const bool jvalid = j < p.Nj;
    const int jj = jvalid ? j : 0;
    const int hw = p.Hc * p.Wc;
    const int pb = jj / hw, r = jj - pb * hw;
    const int pyy = (r / p.Wc) * 2 + p.py, pxx = (r % p.Wc) * 2 + p.px;
    const int y0 = (pyy + 1 - p.ky0) >> 1, x0 = (pxx + 1 - p.kx0) >> 1;  // output pixel of the class's first tap
    PixelTaps t;
    t.safe = pb * p.Cout * p.Ho * p.Wo;
    t.base = t.safe + y0 * p.Wo + x0;
    t.mask = 0;
#pragma unroll
    for (int ty = 0; ty < 2; ++ty)
#pragma unroll
        for (int tx = 0; tx < 2; ++tx)
            t.mask |= (unsigned)(y0 - ty >= 0 && y0 - ty < p.Ho && x0 - tx >= 0 && x0 - tx < p.Wo) << (ty * 2 + tx);
    if (!jvalid) t.mask = 0;
    return t;
}

// data gradient: element offset of class pixel j in gX (channel 0)
__device__ __forceinline__ size_t dgrad_pixel_offset(const IgParams &p, int j) {
    const int hw = p.Hc * p.Wc;
    const int b = j / hw, r = j - b * hw;
    const int y = (r / p.Wc) * 2 + p.py, x = (r % p.Wc) * 2 + p.px;
    return (size_t)b * p.Cin * p.H * p.W + (size_t)y * p.W + x;
}

// data-gradient reduction table entry of k = (co, tap): (gY offset relative to the first tap, tap bit)
__device__ __forceinline__ int2 dgrad_tab(const IgParams &p, int kk) {
    const int nt = p.nky * p.nkx;
    const int co = kk / nt, tap = kk - co * nt;
    const int ty = tap / p.nkx, tx = tap - ty * p.nkx;
    return make_int2(co * p.Ho * p.Wo - ty * p.Wo - tx, ty * 2 + tx);
}

// The B half of a FWD / DGRAD stage: rows kw + 2 r (r < 16) of the lane's pixel column.  tab[k] = (offset, tap in the
// low 5 bits); a tap outside the pixel's mask reads px.safe and is zeroed at the store.
struct GatherB {
    float v[16];
    unsigned ok;
    __device__ __forceinline__ void load(const float *Bm, const int2 *tab, const PixelTaps &px) {
        ok = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int2 e = tab[2 * r];  // wave-uniform address: a broadcast read
            const unsigned o = (px.mask >> (e.y & 31)) & 1u;
            ok |= o << r;
            v[r] = Bm[o ? px.base + e.x : px.safe];
        }
    }
    // Bs: the lane's column at row kw
    __device__ __forceinline__ void store(float *Bs) const { store_masked<2 * IG_LD>(Bs, v, ok); }
};

// A stage read from a row-major [rows][Kd] matrix: float4 v of the thread covers row 32 v + (tid >> 3), columns
// 4 (tid & 7) .. + 3 of the stage, stored transposed (As[k][row]); rows with ok[v] false are zeroed
template <int AV>
__device__ __forceinline__ void store_a_rows(float *As, const float4 (&ra)[AV], const bool (&ok)[AV], int tid) {
#pragma unroll
    for (int v = 0; v < AV; ++v) {
        const int il = 32 * v + (tid >> 3), q = tid & 7;
        As[(q * 4 + 0) * IG_LD + il] = ok[v] ? ra[v].x : 0.f;
        As[(q * 4 + 1) * IG_LD + il] = ok[v] ? ra[v].y : 0.f;
        As[(q * 4 + 2) * IG_LD + il] = ok[v] ? ra[v].z : 0.f;
        As[(q * 4 + 3) * IG_LD + il] = ok[v] ? ra[v].w : 0.f;
    }
}

// ------------------------------------------------------------------ WGRAD: one pixel per thread and stage
// column (ci, t) of gW as the thread packs it: ((X offset of the tap relative to the window corner) << 4) | t
__device__ __forceinline__ int wgrad_col(const IgParams &p, int ci, int t) {
    const int ty = t / 3, tx = t - ty * 3;
    return ((ci * p.H * p.W + ty * p.W + tx) << 4) | t;
}

// Stage pixel (pb, yo, xo) of one thread: gY rows i0 + rg + 8 r (rows past Mi, a_mask bit clear, re-read row i0 + rg)
// and the im2col columns cpk[r] (-1: idle) of the pixel's window; an invalid tap reads X[0].  mv false (pixel past
// the end of the range): everything is zeroed at the store.
template <int NB>
struct WgradStage {
    float ra[16], rb[NB];
    unsigned okb;
    bool mv;
    __device__ __forceinline__ void load(const IgParams &p, int i0, unsigned a_mask, const int (&cpk)[NB], bool valid,
                                         int pb, int yo, int xo, int rg) {
        mv = valid;
        const int HoWo = p.Ho * p.Wo;
        const int a_base = (pb * p.Cout + i0 + rg) * HoWo + yo * p.Wo + xo;
#pragma unroll
        for (int r = 0; r < 16; ++r) ra[r] = p.A[a_base + (((a_mask >> r) & 1u) ? r * 8 * HoWo : 0)];
        const int b_base = pb * p.Cin * p.H * p.W + (2 * yo - 1) * p.W + 2 * xo - 1;  // window corner (may lie outside)
        const unsigned ym = (unsigned)(yo > 0) | 2u | ((unsigned)(2 * yo + 1 < p.H) << 2);
        const unsigned xm = (unsigned)(xo > 0) | 2u | ((unsigned)(2 * xo + 1 < p.W) << 2);
        const unsigned tapmask =
            mv ? (((ym & 1u) ? xm : 0u) | ((ym & 2u) ? xm << 3 : 0u) | ((ym & 4u) ? xm << 6 : 0u)) : 0u;
        okb = 0;
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            const int c = cpk[r];
            const unsigned ok = (c >= 0) ? ((tapmask >> (c & 15)) & 1u) : 0u;
            okb |= ok << r;
            rb[r] = p.Bm[ok ? b_base + (c >> 4) : 0];
        }
    }
    // As / Bs: row kk of the stage, column rg; A and B rows 8 apart
    __device__ __forceinline__ void store(float *As, float *Bs, unsigned a_mask) const {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            As[8 * r] = (mv && ((a_mask >> r) & 1u)) ? ra[r] : 0.f;
            if (r < NB) Bs[8 * r] = ((okb >> r) & 1u) ? rb[r] : 0.f;
        }
    }
};
