// bf16-operand versions of the sparse-convolution kernels (lidog_amd/precision.py): the two forward kernels (the gathered
// GEMM also serves the data gradient of a training step, over the exchanged map with the transposed kernel) and the
// weight gradient.
// Activations stay fp32 in memory: the gathered feature rows are rounded to bf16 (nearest even, v_cvt_pk_bf16_f32) on
// their way into LDS, the weights are packed to bf16 once per run (lidog_pack_kernels_bf16), accumulation is fp32 in
// v_mfma_f32_32x32x16_bf16 (16 x the multiply-adds per instruction of the exact-f32 32x32x2 form of sconv_mfma.hip).
// Products of two bf16 numbers are exact in fp32, so against a float64 convolution of the ROUNDED operands all that is
// left is the fp32 accumulation (tests/test_gpu_bf16.py).  Results are NOT the bits of the fp32 kernels.
//
// MFMA 32x32x16 bf16 lane maps (cdna_hip_programming.md, section 3): lane l holds A[row l & 31][k = 8 (l >> 5) + j] and
// B[k = 8 (l >> 5) + j][col l & 31], j = 0..7, i.e. 16 contiguous bytes of a k-contiguous row -- which is why the
// packed weights are [K][Cout][Cin]; D[i][j]: j = l & 31, i = (e & 3) + 8 (e >> 2) + 4 (l >> 5) for accumulator
// register e, the layout of the 32x32x2 form.
#include <stdlib.h>

#include "common.h"
#include "sconv_mfma.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

#define BF_TM 128
#define BF_BK 32
// bf16 elements per LDS row: 32 of a chunk + 8 of padding = 80 bytes.  Rows stay 16-byte aligned (one 16-byte read per
// operand fragment) and 16 consecutive rows start in 16 different 16-byte bank groups of the 256-byte bank cycle.
#define BF_SA 40
#define BF_MAXK 27

__device__ __forceinline__ uint32_t bf_pack2(float a, float b) {
    bf16x2 v = {(__bf16)a, (__bf16)b};      // round to nearest even; NaN and infinities stay what they are
    return __builtin_bit_cast(uint32_t, v);
}

// ------------------------------------------------------------------ weights: fp32 [K][Cin][Cout] -> bf16 [K][Cout][Cin]
// Every eligible kernel of a model in ONE launch, after lidog_transpose_batched (sconv.hip): desc[m] = (src offset in
// floats from `src`, dst offset in bf16 elements from `dst`, K, Cin, Cout, first tile); tiles are 32 x 32, enumerated
// per matrix as (k, ci tile, co tile).
__global__ __launch_bounds__(256) void k_pack_kernels_bf16(const float *__restrict__ src, uint16_t *__restrict__ dst,
                                                           const int64_t *__restrict__ desc, int n_mats) {
    __shared__ float tile[32][33];
    __shared__ int64_t s_d[6];
    const int64_t t = blockIdx.x;
    if (threadIdx.x == 0) {
        int lo = 0, hi = n_mats - 1;   // last matrix whose first tile is <= t
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (desc[(size_t)mid * 6 + 5] <= t) lo = mid;
            else hi = mid - 1;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) s_d[j] = desc[(size_t)lo * 6 + j];
    }
    __syncthreads();
    const int K = (int)s_d[2], Cin = (int)s_d[3], Cout = (int)s_d[4];
    const int tco = (Cout + 31) / 32, tci = (Cin + 31) / 32;
    const int64_t local = t - s_d[5];
    const int k = (int)(local / (tci * tco));
    if (k >= K) return;                // a tile count larger than the table's: nothing to do
    const int r = (int)(local - (int64_t)k * tci * tco);
    const int ci0 = (r / tco) * 32, co0 = (r % tco) * 32;
    const float *W = src + s_d[0] + (size_t)k * Cin * Cout;
    uint16_t *Wp = dst + s_d[1] + (size_t)k * Cin * Cout;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int rr = ty; rr < 32; rr += 8)
        if (ci0 + rr < Cin && co0 + tx < Cout) tile[rr][tx] = W[(size_t)(ci0 + rr) * Cout + co0 + tx];
    __syncthreads();
    for (int rr = ty; rr < 32; rr += 8)
        if (co0 + rr < Cout && ci0 + tx < Cin) {
            const __bf16 v = (__bf16)tile[tx][rr];
            Wp[(size_t)(co0 + rr) * Cin + ci0 + tx] = __builtin_bit_cast(uint16_t, v);
        }
}

extern "C" int lidog_pack_kernels_bf16(const float *src, uint16_t *dst, const int64_t *desc, int32_t n_mats,
                                       int64_t total_tiles, void *stream) {
    if (n_mats == 0 || total_tiles == 0) return 0;
    LIDOG_REQUIRE(src && dst && desc && n_mats > 0, "pack_kernels_bf16: null argument");
    LIDOG_REQUIRE(total_tiles > 0 && total_tiles < ((int64_t)1 << 31), "pack_kernels_bf16: bad tile count");
    k_pack_kernels_bf16<<<(unsigned)total_tiles, 256, 0, (hipStream_t)stream>>>(src, dst, desc, n_mats);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ shared pieces of the two kernels
// Staging of one 32-channel chunk: 128 rows x 32 floats of A (thread: the float4 (tid & 7) of rows (tid >> 3) + 32 j,
// as the fp32 kernels) and 32 NT columns x 32 bf16 of the packed weights (16 bytes per thread and slot).  LDS row R of
// the weights holds column (R & 31) * NT + (R >> 5) of the tile: MFMA column tile t of a wave = columns {li * NT + t}
// (a lane's NT results are adjacent in memory, as in sconv_mfma.hip), read at a lane stride of one LDS row.
template <int NT>
struct BfStage {
    static constexpr int TN = 32 * NT;
    static constexpr int NB = TN * 4;       // 16-byte pieces of the weights per chunk
    float4 ra[4];
    uint4 rb0, rb1;

    __device__ __forceinline__ void load(const float *const (&a_row)[4], int kb, const uint16_t *Wk, int Cin) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ra[j] = *reinterpret_cast<const float4 *>(a_row[j] + kb);
        const int tid = threadIdx.x;
        {   // slots past the end of the tile re-read its last piece (an unconditional load) and are not stored
            const int f = tid < NB ? tid : NB - 1;
            const int R = f >> 2, q = f & 3;
            rb0 = *reinterpret_cast<const uint4 *>(Wk + (size_t)((R & 31) * NT + (R >> 5)) * Cin + kb + q * 8);
        }
        if constexpr (NB > 256) {
            const int f = tid + 256 < NB ? tid + 256 : NB - 1;
            const int R = f >> 2, q = f & 3;
            rb1 = *reinterpret_cast<const uint4 *>(Wk + (size_t)((R & 31) * NT + (R >> 5)) * Cin + kb + q * 8);
        }
    }

    // `ok[j]`: the row exists; a missing one becomes a row of zeros by a SELECT (its registers hold row 0 of A, which
    // may be anything, NaN included)
    __device__ __forceinline__ void store(uint16_t *As, uint16_t *Bs, const bool (&ok)[4]) const {
        const int tid = threadIdx.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int f = tid + 256 * j;
            uint2 p;
            p.x = ok[j] ? bf_pack2(ra[j].x, ra[j].y) : 0u;
            p.y = ok[j] ? bf_pack2(ra[j].z, ra[j].w) : 0u;
            *reinterpret_cast<uint2 *>(&As[(f >> 3) * BF_SA + (f & 7) * 4]) = p;
        }
        if (tid < NB) *reinterpret_cast<uint4 *>(&Bs[(tid >> 2) * BF_SA + (tid & 3) * 8]) = rb0;
        if constexpr (NB > 256) {
            const int f = tid + 256;
            if (f < NB) *reinterpret_cast<uint4 *>(&Bs[(f >> 2) * BF_SA + (f & 3) * 8]) = rb1;
        }
    }
};

// the two MFMAs per column tile of one staged chunk
template <int NT>
__device__ __forceinline__ void bf_multiply(const uint16_t *As, const uint16_t *Bs, f32x16 (&acc)[NT]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, kh = lane >> 5;
    const uint16_t *arow = &As[(wave * 32 + li) * BF_SA + 8 * kh];
    const bf16x8 a0 = *reinterpret_cast<const bf16x8 *>(arow);
    const bf16x8 a1 = *reinterpret_cast<const bf16x8 *>(arow + 16);
    bf16x8 b0[NT], b1[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const uint16_t *brow = &Bs[(t * 32 + li) * BF_SA + 8 * kh];
        b0[t] = *reinterpret_cast<const bf16x8 *>(brow);
        b1[t] = *reinterpret_cast<const bf16x8 *>(brow + 16);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0[t], acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1[t], acc[t], 0, 0, 0);
}

template <int NT>
__device__ __forceinline__ void bf_store_row(float *o, const float (&v)[NT]) {
    if constexpr (NT == 4) {
        *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (NT == 2) {
        *reinterpret_cast<float2 *>(o) = make_float2(v[0], v[1]);
    } else {
#pragma unroll
        for (int t = 0; t < NT; ++t) o[t] = v[t];
    }
}

// ------------------------------------------------------------------ gathered GEMM
// T[dst] = bf16(A[src]) . bf16 W[k] (+ bias) for the pairs of one tile (tile_k / tile_row0 / tile_rows of the rule book,
// at most 128 pair-rows of one offset) x 32 NT columns; wave w owns rows [32 w, 32 w + 32) and all NT column tiles.
// gather == NULL: src = the pair-row itself (1x1 convolutions); scatter == NULL: dst = the pair-row (product rows for
// lidog_sconv_reduce_rows[_bn]), else dst = scatter[pair-row] (transposed k2 s2: every output row has one pair).
template <int NT>
__global__ __launch_bounds__(256) void k_sconv_gemm_bf16(const float *__restrict__ A, const int32_t *__restrict__ gather,
                                                         const uint16_t *__restrict__ Wp, const float *__restrict__ bias,
                                                         const int32_t *__restrict__ tile_k,
                                                         const int32_t *__restrict__ tile_row0,
                                                         const int32_t *__restrict__ tile_rows, int Cin, int Cout,
                                                         float *__restrict__ T, const int32_t *__restrict__ scatter) {
    constexpr int TN = 32 * NT;
    __shared__ __attribute__((aligned(16))) uint16_t As[BF_TM * BF_SA];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[TN * BF_SA];
    __shared__ int32_t s_src[BF_TM];
    __shared__ int32_t s_dst[BF_TM];

    const int tile = blockIdx.x;
    const int k = tile_k[tile], row0 = tile_row0[tile];
    const int rows = tile_rows[tile] < BF_TM ? tile_rows[tile] : BF_TM;
    const int col0 = blockIdx.y * TN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kh = lane >> 5;

    if (tid < BF_TM) {
        int src = -1, dst = -1;
        if (tid < rows) {
            src = gather ? gather[row0 + tid] : (row0 + tid);
            dst = scatter ? scatter[row0 + tid] : (row0 + tid);
        }
        s_src[tid] = src;
        s_dst[tid] = dst;
    }
    __syncthreads();

    // rows past the end of the tile and negative gather indices: the load goes to row 0, the staged row is zeros
    const float *a_row[4];
    bool ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int src = s_src[(tid >> 3) + 32 * j];
        ok[j] = src >= 0;
        a_row[j] = A + (size_t)(src < 0 ? 0 : src) * Cin + (tid & 7) * 4;
    }
    const uint16_t *Wk = Wp + ((size_t)k * Cout + col0) * Cin;

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    float bv[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bv[t] = bias ? bias[col0 + li * NT + t] : -0.0f;     // x + -0 == x, also for x = -0

    BfStage<NT> st;
    st.load(a_row, 0, Wk, Cin);
    for (int kb = 0; kb < Cin; kb += BF_BK) {
        __syncthreads();
        st.store(As, Bs, ok);
        __syncthreads();
        // unconditional prefetch: the last iteration re-reads its own chunk
        st.load(a_row, kb + BF_BK < Cin ? kb + BF_BK : kb, Wk, Cin);
        bf_multiply<NT>(As, Bs, acc);
    }

#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int dst = s_dst[wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * kh];
        if (dst >= 0) {       // rows past the end of the tile reach no store
            float v[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) v[t] = acc[t][e] + bv[t];
            bf_store_row<NT>(T + (size_t)dst * Cout + col0 + li * NT, v);
        }
    }
}

static int bf_nt(int Cout) { return (Cout % 128 == 0) ? 4 : (Cout % 96 == 0) ? 3 : (Cout % 64 == 0) ? 2 : 1; }

extern "C" int lidog_sconv_gemm_bf16(const float *A, const int32_t *gather, const uint16_t *Wp, const float *bias,
                                     const int32_t *tile_k, const int32_t *tile_row0, const int32_t *tile_rows,
                                     int32_t n_tiles, int32_t Cin, int32_t Cout, float *T, const int32_t *scatter,
                                     void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n_tiles == 0) return 0;
    LIDOG_REQUIRE(Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % 32 == 0,
                  "sconv_gemm_bf16: channel counts must be multiples of 32 (got %d -> %d)", Cin, Cout);
    LIDOG_REQUIRE(n_tiles > 0 && A && Wp && T && tile_k && tile_row0 && tile_rows, "sconv_gemm_bf16: bad arguments");
    const int nt = bf_nt(Cout);
    dim3 grid((unsigned)n_tiles, (unsigned)(Cout / (32 * nt)));
#define BF_GEMM(NT_) \
    k_sconv_gemm_bf16<NT_><<<grid, 256, 0, st>>>(A, gather, Wp, bias, tile_k, tile_row0, tile_rows, Cin, Cout, T, scatter)
    switch (nt) {
        case 4: BF_GEMM(4); break;
        case 3: BF_GEMM(3); break;
        case 2: BF_GEMM(2); break;
        default: BF_GEMM(1);
    }
#undef BF_GEMM
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ output-stationary form over sorted rows
// The tile / offset walk of sconv_os.hip:k_sconv_os_mfma (perm / wave_masks / tile_order of lidog_kernel_map_sorted) with
// bf16 operands and the evaluation-mode BatchNorm (+ residual + ReLU) epilogue only.  The fp32 kernel keeps a scratch
// accumulator per offset to reproduce the bits of the two-pass path; there is no such promise here, so the offsets
// accumulate straight into one set of registers.
struct BfBn {
    const float *mean, *invstd, *w, *b, *res;
    int relu;
};

template <int NT>
__global__ __launch_bounds__(256) void k_sconv_os_bn_bf16(const float *__restrict__ A, const int32_t *__restrict__ nbr,
                                                          int64_t n, int K, const int32_t *__restrict__ perm,
                                                          const uint32_t *__restrict__ wave_masks,
                                                          const int32_t *__restrict__ tile_order,
                                                          const uint16_t *__restrict__ Wp, const float *__restrict__ bias,
                                                          int Cin, int Cout, float *__restrict__ out, BfBn bn,
                                                          int xcd_group) {
    constexpr int TN = 32 * NT;
    __shared__ __attribute__((aligned(16))) uint16_t As[BF_TM * BF_SA];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[TN * BF_SA];
    __shared__ int32_t s_row[BF_TM];
    __shared__ int32_t s_nbr[BF_MAXK * BF_TM];   // neighbour row of (offset, tile row), -1 = none

    // heaviest tiles first, runs of xcd_group consecutive tiles of the order on one XCD (as k_sconv_os_mfma)
    int slot = blockIdx.x;
    if (xcd_group > 0) {
        const int per_round = 8 * xcd_group, full = ((int)gridDim.x / per_round) * per_round;
        if (slot < full) {
            const int xcd = slot & 7, j = slot >> 3;
            slot = ((j / xcd_group) * 8 + xcd) * xcd_group + j % xcd_group;
        }
    }
    const int tile = tile_order[slot];
    const int col0 = blockIdx.y * TN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kh = lane >> 5;

    const uint32_t wm = wave_masks[tile * 4 + wave];
    const uint32_t tm = wave_masks[tile * 4] | wave_masks[tile * 4 + 1] | wave_masks[tile * 4 + 2] | wave_masks[tile * 4 + 3];
    if (tid < BF_TM) s_row[tid] = perm[(int64_t)tile * BF_TM + tid];
    __syncthreads();
    for (int e = tid; e < K * BF_TM; e += 256) {
        const int k = e / BF_TM, r = e - k * BF_TM;
        const int row = s_row[r];
        s_nbr[e] = (row >= 0 && ((tm >> k) & 1u)) ? nbr[(int64_t)k * n + row] : -1;
    }
    __syncthreads();

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    // the epilogue's per-column vectors, fetched before the loop (nothing but stores pending at the end)
    float bv[NT], e_m[NT], e_is[NT], e_w[NT], e_b[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = col0 + li * NT + t;
        bv[t] = bias ? bias[c] : -0.0f;
        e_m[t] = bn.mean[c]; e_is[t] = bn.invstd[c]; e_w[t] = bn.w[c]; e_b[t] = bn.b[c];
    }

    const float *a_row[4];
    bool ok_cur[4], ok_nxt[4];
    const int q4 = (tid & 7) * 4;
    auto rows_of = [&](int k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int src = s_nbr[k * BF_TM + (tid >> 3) + 32 * j];
            ok_nxt[j] = src >= 0;
            a_row[j] = A + (size_t)(src < 0 ? 0 : src) * Cin + q4;
        }
    };
    auto weights_of = [&](int k) { return Wp + ((size_t)k * Cout + col0) * Cin; };

    BfStage<NT> st;
    uint32_t rem = tm;
    if (rem != 0) {
        int k_cur = __builtin_ctz(rem);
        rem &= ~(1u << k_cur);
        int kb_cur = 0;
        rows_of(k_cur);
#pragma unroll
        for (int j = 0; j < 4; ++j) ok_cur[j] = ok_nxt[j];
        st.load(a_row, 0, weights_of(k_cur), Cin);
        for (;;) {
            __syncthreads();
            st.store(As, Bs, ok_cur);
            __syncthreads();
            // the chunk after this one: the next 32 channels of this offset, or the first 32 of the tile's next offset;
            // past the end the current chunk is fetched again
            const bool last_of_offset = kb_cur + BF_BK >= Cin;
            const bool more = !last_of_offset || rem != 0;
            int k_nxt = k_cur, kb_nxt = kb_cur + BF_BK;
            if (last_of_offset) {
                kb_nxt = 0;
                if (rem != 0) {
                    k_nxt = __builtin_ctz(rem);
                    rem &= ~(1u << k_nxt);
                    rows_of(k_nxt);
                }
            }
            st.load(a_row, kb_nxt, weights_of(k_nxt), Cin);
            if ((wm >> k_cur) & 1u) bf_multiply<NT>(As, Bs, acc);      // a wave skips the offsets none of its rows has
            if (!more) break;
            if (last_of_offset) {
#pragma unroll
                for (int j = 0; j < 4; ++j) ok_cur[j] = ok_nxt[j];
            }
            k_cur = k_nxt;
            kb_cur = kb_nxt;
        }
    }

    // epilogue: rows in two batches of eight, the residual loads of a batch issued before the first use (a row behind
    // the end of the map reads row 0 and is masked afterwards)
#pragma unroll
    for (int eb = 0; eb < 16; eb += 8) {
        int dst[8];
        float resv[8][NT];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = eb + u;
            dst[u] = s_row[wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * kh];
            const size_t at = (size_t)(dst[u] < 0 ? 0 : dst[u]) * Cout + col0 + li * NT;
#pragma unroll
            for (int t = 0; t < NT; ++t) resv[u][t] = bn.res ? bn.res[at + t] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float v[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t)
                v[t] = bn_res_relu(bn_affine(acc[t][eb + u] + bv[t], e_m[t], e_is[t], e_w[t], e_b[t]), bn.res != nullptr,
                                   resv[u][t], bn.relu);
            if (dst[u] >= 0) bf_store_row<NT>(out + (size_t)dst[u] * Cout + col0 + li * NT, v);
        }
    }
}

// out [n, Cout] = relu(BatchNorm_eval(sum_k bf16(A[nbr[k][row]]) . bf16 W[k] (+ bias)) (+ residual)), rows in canonical
// order; Wp: the packed weights [K][Cout][Cin] of lidog_pack_kernels_bf16.
extern "C" int lidog_sconv_os_bn_bf16(const float *A, const int32_t *nbr, int64_t n, int32_t K, const int32_t *perm,
                                      const uint32_t *wave_masks, const int32_t *tile_order, const uint16_t *Wp,
                                      const float *bias, int32_t Cin, int32_t Cout, const float *mean, const float *invstd,
                                      const float *w, const float *b, const float *residual, int32_t relu, float *out,
                                      void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return 0;
    LIDOG_REQUIRE(K >= 1 && K <= BF_MAXK && Cin % 32 == 0 && Cout % 32 == 0 && Cin > 0 && Cout > 0,
                  "sconv_os_bn_bf16: K <= %d, channel counts multiples of 32 (got K %d, %d -> %d)", BF_MAXK, K, Cin, Cout);
    LIDOG_REQUIRE(n > 0 && n < ((int64_t)1 << 31) && A && nbr && perm && wave_masks && tile_order && Wp && out,
                  "sconv_os_bn_bf16: bad arguments");
    LIDOG_REQUIRE(mean && invstd && w && b, "sconv_os_bn_bf16: BatchNorm vectors missing");
    const int nt = bf_nt(Cout);
    dim3 grid((unsigned)((n + BF_TM - 1) / BF_TM), (unsigned)(Cout / (32 * nt)));
    const BfBn bn = {mean, invstd, w, b, residual, relu};
    const int xcd_group = 4;
#define BF_OS(NT_)                                                                                                   \
    k_sconv_os_bn_bf16<NT_><<<grid, 256, 0, st>>>(A, nbr, n, K, perm, wave_masks, tile_order, Wp, bias, Cin, Cout, out, \
                                                  bn, xcd_group)
    switch (nt) {
        case 4: BF_OS(4); break;
        case 3: BF_OS(3); break;
        case 2: BF_OS(2); break;
        default: BF_OS(1);
    }
#undef BF_OS
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ weight gradient
// gW[k] tile (32 MT) x (32 NT) = sum over the pairs of a work item of bf16(A_row)^T (x) bf16(G_row), fp32 accumulation.
// The outer structure is sconv_mfma.hip:k_sconv_wgrad_mfma's: the same work items, tile selection, wave shapes, two-level
// software pipeline of pair indices and gathered rows, unconditional clamped loads and zero-select at the LDS store.
//
// The reduction dimension is the PAIR index: for the 32x32x16 instruction lane (li, kh) holds A[row = ci][k = 8 kh + j]
// and B[k = 8 kh + j][col = co], eight consecutive pairs of ONE channel for both operands.  Both images are therefore
// staged already transposed, [channel][pair], one chunk of 32 pairs = 64 bytes per channel row + 16 of padding (BF_SA),
// and a fragment is one 16-byte read of a row -- the read pattern of bf_multiply above.
//
// Bank conflicts.  Reads (ds_read_b128, 64 banks of 4 bytes, 256-byte cycle): the 32 lanes of a half read rows li at the
// same column; rows are 80 bytes apart, so 16 consecutive rows start in 16 different 16-byte groups of the cycle
// (80 li mod 256 = 16 (5 li mod 16), 5 odd) and the second 16 repeat them in the instruction's other lane group: no
// conflict, as in the two forward kernels.  Writes (ds_write_b32, 32 banks, per 32-lane half): a staging thread holds
// the SAME four channels of two consecutive pairs (two float4 loads) and writes four words {bf16(pair 2r), bf16(pair
// 2r+1)}, one per channel row.  Cell f of a chunk = (pair duo r = f & 15, channel quad c4 = f >> 4): a half-wave is 16
// duos x 2 quads, word address (4 c4 + i) 20 + r, i.e. banks r for the even quad and 16 + r for the odd one (80 mod 32
// = 16): every one of the four writes is conflict-free.  The price is the global side: a wave's load touches 64
// contiguous bytes of 16 rows instead of whole rows (the rest of each line is another wave's, served by the cache).
// Rows past the end of the item are exact zeros in BOTH images (0 x NaN would be NaN).
template <int MT, int NT, int NW, int NGRP>
__global__ __launch_bounds__(64 * NW) void k_sconv_wgrad_bf16(const float *__restrict__ A, const int32_t *__restrict__ pa,
                                                              const float *__restrict__ G, const int32_t *__restrict__ pg,
                                                              const int32_t *__restrict__ items, int n_items, int Cin,
                                                              int Cout, float *__restrict__ partial) {
    constexpr int TM = 32 * MT, TN = 32 * NT, NTH = 64 * NW;
    constexpr int TILES = MT * NT;
    constexpr int WPG = NW / NGRP;                  // waves per group
    constexpr int TPW = (TILES + WPG - 1) / WPG;    // tiles per wave
    static_assert(NGRP == 1 || NGRP == 2, "a chunk is two k = 16 steps: one group takes both, or two take one each");
    __shared__ __attribute__((aligned(16))) uint16_t At[TM * BF_SA];
    __shared__ __attribute__((aligned(16))) uint16_t Gt[TN * BF_SA];
    // row 3 of the item table = launch order (me.py:_wgrad_items_host)
    const int item = items[3 * n_items + blockIdx.x];
    const int tiles_n = Cout / TN;
    const int ci0 = (blockIdx.y / tiles_n) * TM, co0 = (blockIdx.y % tiles_n) * TN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kh = lane >> 5;
    const int grp = wave / WPG, wig = wave % WPG;
    const int64_t p0 = items[n_items + item], p1 = items[2 * n_items + item];

    int a_off[TPW], g_off[TPW];
    bool own[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int tt = wig * TPW + t;   // tiles enumerated column-major: tt = nj * MT + mi
        own[t] = tt < TILES;
        const int mi = own[t] ? tt % MT : 0, nj = own[t] ? tt / MT : 0;
        a_off[t] = (32 * mi + li) * BF_SA + 8 * kh;
        g_off[t] = (32 * nj + li) * BF_SA + 8 * kh;
    }
    f32x16 acc[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

    constexpr int AC = TM * 4, GC = TN * 4;         // cells of a chunk: (channels / 4) quads x 16 pair duos
    constexpr int AV = (AC + NTH - 1) / NTH, GV = (GC + NTH - 1) / NTH;
    float4 ra[AV][2], rg[GV][2];
    int ia[AV][2], ig[GV][2];
    auto load_idx = [&](int64_t p) {
#pragma unroll
        for (int j = 0; j < AV; ++j) {
            int f = tid + NTH * j;
            f = f < AC ? f : AC - 1;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int64_t pr = p + 2 * (f & 15) + u;
                ia[j][u] = pa[pr < p1 ? pr : p1 - 1];
            }
        }
#pragma unroll
        for (int j = 0; j < GV; ++j) {
            int f = tid + NTH * j;
            f = f < GC ? f : GC - 1;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int64_t pr = p + 2 * (f & 15) + u;
                ig[j][u] = pg[pr < p1 ? pr : p1 - 1];
            }
        }
    };
    auto load_rows = [&]() {
#pragma unroll
        for (int j = 0; j < AV; ++j) {
            int f = tid + NTH * j;
            f = f < AC ? f : AC - 1;
#pragma unroll
            for (int u = 0; u < 2; ++u)
                ra[j][u] = *reinterpret_cast<const float4 *>(A + (size_t)ia[j][u] * Cin + ci0 + (f >> 4) * 4);
        }
#pragma unroll
        for (int j = 0; j < GV; ++j) {
            int f = tid + NTH * j;
            f = f < GC ? f : GC - 1;
#pragma unroll
            for (int u = 0; u < 2; ++u)
                rg[j][u] = *reinterpret_cast<const float4 *>(G + (size_t)ig[j][u] * Cout + co0 + (f >> 4) * 4);
        }
    };
    if (p0 < p1) {
        load_idx(p0);
        load_rows();
        load_idx(p0 + BF_BK);
    }
    uint32_t *At32 = reinterpret_cast<uint32_t *>(At), *Gt32 = reinterpret_cast<uint32_t *>(Gt);
    for (int64_t p = p0; p < p1; p += BF_BK) {
        __syncthreads();
        // pairs past the end of the item are zeroed here, not at load time (a select right after the load would make the
        // wave wait for the gather before its MFMA phase instead of after it)
#pragma unroll
        for (int j = 0; j < AV; ++j) {
            const int f = tid + NTH * j;
            const int r = f & 15, c = (f >> 4) * 4;
            const bool ok0 = p + 2 * r < p1, ok1 = p + 2 * r + 1 < p1;
            const float4 v0 = ra[j][0], v1 = ra[j][1];
            if (f < AC) {
                uint32_t *d = At32 + c * (BF_SA / 2) + r;
                d[0] = bf_pack2(ok0 ? v0.x : 0.f, ok1 ? v1.x : 0.f);
                d[BF_SA / 2] = bf_pack2(ok0 ? v0.y : 0.f, ok1 ? v1.y : 0.f);
                d[2 * (BF_SA / 2)] = bf_pack2(ok0 ? v0.z : 0.f, ok1 ? v1.z : 0.f);
                d[3 * (BF_SA / 2)] = bf_pack2(ok0 ? v0.w : 0.f, ok1 ? v1.w : 0.f);
            }
        }
#pragma unroll
        for (int j = 0; j < GV; ++j) {
            const int f = tid + NTH * j;
            const int r = f & 15, c = (f >> 4) * 4;
            const bool ok0 = p + 2 * r < p1, ok1 = p + 2 * r + 1 < p1;
            const float4 v0 = rg[j][0], v1 = rg[j][1];
            if (f < GC) {
                uint32_t *d = Gt32 + c * (BF_SA / 2) + r;
                d[0] = bf_pack2(ok0 ? v0.x : 0.f, ok1 ? v1.x : 0.f);
                d[BF_SA / 2] = bf_pack2(ok0 ? v0.y : 0.f, ok1 ? v1.y : 0.f);
                d[2 * (BF_SA / 2)] = bf_pack2(ok0 ? v0.z : 0.f, ok1 ? v1.z : 0.f);
                d[3 * (BF_SA / 2)] = bf_pack2(ok0 ? v0.w : 0.f, ok1 ? v1.w : 0.f);
            }
        }
        __syncthreads();
        if (p + BF_BK < p1) {
            load_rows();
            load_idx(p + 2 * BF_BK);
        }
        // k = 16 steps of the chunk: pairs [16 s, 16 s + 16); with two groups each takes one step and its own slab
#pragma unroll
        for (int q = 0; q < 2 / NGRP; ++q) {
            const int ks = 16 * (q * NGRP + grp);
            bf16x8 af[TPW], gf[TPW];
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                af[t] = *reinterpret_cast<const bf16x8 *>(&At[a_off[t] + ks]);
                gf[t] = *reinterpret_cast<const bf16x8 *>(&Gt[g_off[t] + ks]);
            }
#pragma unroll
            for (int t = 0; t < TPW; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[t], gf[t], acc[t], 0, 0, 0);
        }
    }
    float *dst = partial + (size_t)(item * NGRP + grp) * Cin * Cout;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        if (!own[t]) continue;
        const int tt = wig * TPW + t;
        const int mi = tt % MT, nj = tt / MT;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ci = ci0 + 32 * mi + (e & 3) + 8 * (e >> 2) + 4 * kh;
            dst[(size_t)ci * Cout + co0 + 32 * nj + li] = acc[t][e];
        }
    }
}

// (MT, NT, NW, NGRP) per tile shape, tiles as sconv_mfma.hip:tile32; every wave gets the same number of MFMA tiles, or
// the two k = 16 steps of a chunk are split over two groups of waves that each emit their own partial slab
#define BF_WG_SHAPES(X)                                                                                             \
    X(1, 1, 2, 2) X(1, 2, 4, 2) X(2, 1, 4, 2) X(1, 3, 3, 1) X(3, 1, 3, 1) X(1, 4, 4, 1) X(4, 1, 4, 1) X(2, 2, 4, 1) \
    X(2, 3, 3, 1) X(3, 2, 3, 1) X(2, 4, 4, 1) X(4, 2, 4, 1) X(3, 3, 3, 1) X(3, 4, 4, 1) X(4, 3, 4, 1) X(4, 4, 4, 1)

static bool bf_wgrad_shape(int Cin, int Cout) { return Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % 32 == 0; }

// partial slots (Cin * Cout floats each) the caller must provide for n_items work items; 0: not a bf16 shape
extern "C" int32_t lidog_sconv_wgrad_bf16_slabs(int32_t Cin, int32_t Cout, int32_t n_items) {
    if (!bf_wgrad_shape(Cin, Cout) || n_items < 0) return 0;
    return n_items * (bf_nt(Cin) * bf_nt(Cout) <= 2 ? 2 : 1);
}

// workgroups of the Cin x Cout kernel resident on the chip at a time (per-CU occupancy x CUs), what me._wgrad_chunk
// fits a launch to; 0: not a bf16 shape, or no device
extern "C" int32_t lidog_sconv_wgrad_bf16_slots(int32_t Cin, int32_t Cout) {
    if (!bf_wgrad_shape(Cin, Cout)) return 0;
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return 0;
    hipError_t e = hipErrorInvalidValue;
    switch (bf_nt(Cin) * 10 + bf_nt(Cout)) {
#define X(MT_, NT_, NW_, NG_)                                                                                          \
    case MT_ * 10 + NT_:                                                                                               \
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_sconv_wgrad_bf16<MT_, NT_, NW_, NG_>, 64 * NW_, 0); \
        break;
        BF_WG_SHAPES(X)
#undef X
    }
    return (e == hipSuccess && per > 0) ? per * cus : 0;
}

// gW [K][Cin][Cout] = sum over the pairs of offset k of bf16(A[pair_a])^T bf16(G[pair_g]): arguments and semantics of
// lidog_sconv_wgrad (work items of me._wgrad_items_host, never straddling an offset; one partial slab per item, or per
// item and k-step group: lidog_sconv_wgrad_bf16_slabs; summed per offset in fixed order by sconv.hip:k_items_sum4).
extern "C" int lidog_sconv_wgrad_bf16(const float *A, const int32_t *pair_a, const float *G, const int32_t *pair_g,
                                      const int32_t *items, int32_t n_items, const int32_t *item_off, int32_t K,
                                      int32_t Cin, int32_t Cout, float *partial, float *gW, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(bf_wgrad_shape(Cin, Cout), "sconv_wgrad_bf16: channel counts must be multiples of 32 (got %d -> %d)",
                  Cin, Cout);
    LIDOG_REQUIRE(K >= 1 && n_items >= 0 && item_off && gW, "sconv_wgrad_bf16: bad K / n_items / arguments");
    LIDOG_REQUIRE(n_items == 0 || (partial && A && G && pair_a && pair_g && items),
                  "sconv_wgrad_bf16: operands or partial workspace missing");
    const int mt = bf_nt(Cin), nt = bf_nt(Cout);
    if (n_items > 0) {
        dim3 grid((unsigned)n_items, (unsigned)((Cin / (32 * mt)) * (Cout / (32 * nt))));
        switch (mt * 10 + nt) {
#define X(MT_, NT_, NW_, NG_)                                                                                    \
    case MT_ * 10 + NT_:                                                                                         \
        k_sconv_wgrad_bf16<MT_, NT_, NW_, NG_><<<grid, 64 * NW_, 0, st>>>(A, pair_a, G, pair_g, items, n_items, Cin, \
                                                                          Cout, partial);                       \
        break;
            BF_WG_SHAPES(X)
#undef X
        }
    }
    lidog_launch_items_sum(partial, item_off, lidog_sconv_wgrad_bf16_slabs(Cin, Cout, 1), K, (int64_t)Cin * Cout, gW, st);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
