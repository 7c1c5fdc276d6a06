// Sparse pooling (ME.Minkowski{Sum,Avg,Max}Pooling, MinkowskiPoolingTranspose, MinkowskiGlobal{Sum,Avg,Max}Pooling of
// MinkowskiEngine 0.5.4; utils/models/resnet_old.py:28,53, utils/models/common.py:126,180,208): weightless reductions
// over the rule book (local) and over the scans of a coordinate map (global).  Contract: include/lidog_amd.h.
//
// Every kernel is a gather: a result row walks its own pair list (lidog_kernel_map_rows) and reads the rows on the other
// side of its pairs, so forward passes AND gradients are written with plain vector stores -- no atomics, the same bits on
// every call.  Layout of the library's other row kernels (sconv.hip:reduce_row_list): thread idx handles row idx / CG,
// column group idx % CG (CG = C / 4 float4 groups, or C scalars when C % 4 != 0), so consecutive lanes read consecutive
// 16-byte pieces of ONE gathered row and a wave covers 64 / CG rows; the row's list bounds and neighbour indices are
// loads of one address by all lanes of the row (one request).  Loads go out in unconditional batches of 4 (index clamped
// to the row's last entry, masked by a select afterwards: 0 * inf never happens).  The local kernels use no LDS; the global
// reduction adds the rows of a workgroup through 8 KB of it.
#include "common.h"

namespace {

constexpr int POOL_SUM = 0, POOL_AVG = 1, POOL_MAX = 2;

template <int V>
__device__ __forceinline__ void ldv(const float *__restrict__ p, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 t = *(const float4 *)p;
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void ldv(const int32_t *__restrict__ p, int (&v)[V]) {
    if constexpr (V == 4) {
        const int4 t = *(const int4 *)p;
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void stv(float *__restrict__ p, const float (&v)[V]) {
    if constexpr (V == 4) *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}
template <int V>
__device__ __forceinline__ void stv(int32_t *__restrict__ p, const int (&v)[V]) {
    if constexpr (V == 4) *(int4 *)p = make_int4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}

// THE maximum rule, for a candidate that comes later in list order than everything `best` has seen: strict >, so a tie
// stays with the earlier entry; a NaN is taken unless `best` is one already (the first NaN stays), torch.amax's result
__device__ __forceinline__ void max_take_later(float &best, int &arg, float v, int row) {
    const bool take = arg < 0 || (!(best != best) && (v > best || v != v));
    best = take ? v : best;
    arg = take ? row : arg;
}

// the same rule for two partial results whose entries interleave: list order is ascending row index there (the rows of a
// scan in lidog_in_segments' stable order), so equal values and two NaNs go to the smaller row
__device__ __forceinline__ void max_merge(float &best, int &arg, float v, int row) {
    if (row < 0) return;
    const bool bn = best != best, vn = v != v;
    const bool take = arg < 0 || (vn ? (!bn || row < arg) : (!bn && (v > best || (v == best && row < arg))));
    best = take ? v : best;
    arg = take ? row : arg;
}

// ---------------------------------------------------------------- local: sum / avg (forward, backward, transposed)
template <int V>
__global__ __launch_bounds__(256) void k_pool_rows(const float *__restrict__ x, const int32_t *__restrict__ row_ptr,
                                                   const int32_t *__restrict__ row_list,
                                                   const int32_t *__restrict__ other,
                                                   const int32_t *__restrict__ other_row_ptr, int64_t n, int CG, int avg,
                                                   float *__restrict__ y) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * CG) return;
    const int64_t r = idx / CG;
    const int cg = (int)(idx % CG);
    const int b = row_ptr[r], e = row_ptr[r + 1];
    float acc[V];
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] = 0.f;
    for (int p = b; p < e; p += 4) {
        int o[4];
        float div[4];
        float t[4][V];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = other[row_list[p + j < e ? p + j : e - 1]];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ldv<V>(x + ((int64_t)o[j] * CG + cg) * V, t[j]);
            div[j] = other_row_ptr ? (float)(other_row_ptr[o[j] + 1] - other_row_ptr[o[j]]) : 1.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = p + j < e;
#pragma unroll
            for (int u = 0; u < V; ++u) {
                const float term = other_row_ptr ? t[j][u] / div[j] : t[j][u];
                acc[u] += ok ? term : 0.f;
            }
        }
    }
    if (avg && e > b) {   // an empty list stays exact zeros: no 0 / 0
        const float cnt = (float)(e - b);
#pragma unroll
        for (int u = 0; u < V; ++u) acc[u] = acc[u] / cnt;
    }
    stv<V>(y + idx * V, acc);
}

// ---------------------------------------------------------------- local: max
template <int V>
__global__ __launch_bounds__(256) void k_pool_rows_max(const float *__restrict__ x, const int32_t *__restrict__ row_ptr,
                                                       const int32_t *__restrict__ row_list,
                                                       const int32_t *__restrict__ other, int64_t n, int CG,
                                                       float *__restrict__ y, int32_t *__restrict__ arg) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * CG) return;
    const int64_t r = idx / CG;
    const int cg = (int)(idx % CG);
    const int b = row_ptr[r], e = row_ptr[r + 1];
    float best[V];
    int at[V];
#pragma unroll
    for (int u = 0; u < V; ++u) { best[u] = 0.f; at[u] = -1; }
    for (int p = b; p < e; p += 4) {
        int o[4];
        float t[4][V];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = other[row_list[p + j < e ? p + j : e - 1]];
#pragma unroll
        for (int j = 0; j < 4; ++j) ldv<V>(x + ((int64_t)o[j] * CG + cg) * V, t[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (p + j < e) {
#pragma unroll
                for (int u = 0; u < V; ++u) max_take_later(best[u], at[u], t[j][u], o[j]);
            }
        }
    }
    stv<V>(y + idx * V, best);
    stv<V>(arg + idx * V, at);
}

// gx[i][c] = sum over the pairs of input row i of gy[o][c] where arg[o][c] == i: the gradient of a window reaches the
// one input its forward pass chose, gathered from the input side
template <int V>
__global__ __launch_bounds__(256) void k_pool_rows_max_bwd(const float *__restrict__ gy, const int32_t *__restrict__ arg,
                                                           const int32_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ row_list,
                                                           const int32_t *__restrict__ other, int64_t n, int CG,
                                                           float *__restrict__ gx) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * CG) return;
    const int64_t r = idx / CG;
    const int cg = (int)(idx % CG);
    const int b = row_ptr[r], e = row_ptr[r + 1];
    float acc[V];
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] = 0.f;
    for (int p = b; p < e; p += 4) {
        int o[4];
        float t[4][V];
        int a[4][V];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = other[row_list[p + j < e ? p + j : e - 1]];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ldv<V>(gy + ((int64_t)o[j] * CG + cg) * V, t[j]);
            ldv<V>(arg + ((int64_t)o[j] * CG + cg) * V, a[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = p + j < e;
#pragma unroll
            for (int u = 0; u < V; ++u) acc[u] += (ok && a[j][u] == (int)r) ? t[j][u] : 0.f;
        }
    }
    stv<V>(gx + idx * V, acc);
}

// ---------------------------------------------------------------- global: one reduction per scan
// Shape of the partial table, a function of (n, B, C) alone so that the summation order is too: LW column groups per
// workgroup (all of them up to 256), RB = 256 / LW rows of a scan in flight per workgroup (at most 32), `chunks` pieces
// per scan of about 8 rows per thread (at most 64).  Workgroup (chunk, b, column tile) adds its RB row sums in ascending
// order through LDS and writes ONE partial row; the finish kernel adds a scan's partial rows in workgroup order.
struct GlobalShape {
    int V, CG, LW, RB, chunks, ctiles;
};

GlobalShape global_shape(int64_t n, int B, int C) {
    GlobalShape s;
    s.V = (C % 4 == 0) ? 4 : 1;
    s.CG = C / s.V;
    s.LW = s.CG < 256 ? s.CG : 256;
    s.RB = 256 / s.LW < 32 ? 256 / s.LW : 32;
    s.ctiles = (s.CG + s.LW - 1) / s.LW;
    int64_t c = cdiv64(n, (int64_t)(B > 0 ? B : 1) * s.RB * 8);
    s.chunks = (int)(c < 1 ? 1 : c > 64 ? 64 : c);
    return s;
}

template <int V, int MODE>
__global__ __launch_bounds__(256) void k_pool_global_part(const float *__restrict__ x, const int32_t *__restrict__ perm,
                                                          const int32_t *__restrict__ seg_off, int CG, int LW, int RB,
                                                          float *__restrict__ part, int32_t *__restrict__ part_arg) {
    __shared__ float s_val[256 * V];
    __shared__ int s_arg[MODE == POOL_MAX ? 256 * V : 1];
    const int chunk = blockIdx.x, chunks = gridDim.x, b = blockIdx.y;
    const int tid = threadIdx.x;
    const int r = tid / LW;
    const int cg = blockIdx.z * LW + tid % LW;
    const bool active = r < RB && cg < CG;
    const int s0 = seg_off[b], nb = seg_off[b + 1] - s0;
    const int len = (nb + chunks - 1) / chunks;
    const int lo = s0 + chunk * len;
    const int hi = (lo + len < s0 + nb) ? lo + len : s0 + nb;
    float acc[V];
    int at[V];
#pragma unroll
    for (int u = 0; u < V; ++u) { acc[u] = 0.f; at[u] = -1; }
    if (active) {
        for (int q = lo + r; q < hi; q += 4 * RB) {   // rows q, q + RB, ... of this thread, ascending
            int row[4];
            float t[4][V];
#pragma unroll
            for (int j = 0; j < 4; ++j) row[j] = perm[q + j * RB < hi ? q + j * RB : q];
#pragma unroll
            for (int j = 0; j < 4; ++j) ldv<V>(x + ((int64_t)row[j] * CG + cg) * V, t[j]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = q + j * RB < hi;
#pragma unroll
                for (int u = 0; u < V; ++u) {
                    if (MODE == POOL_MAX) {
                        if (ok) max_take_later(acc[u], at[u], t[j][u], row[j]);
                    } else {
                        acc[u] += ok ? t[j][u] : 0.f;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < V; ++u) {
        s_val[tid * V + u] = acc[u];
        if (MODE == POOL_MAX) s_arg[tid * V + u] = at[u];
    }
    __syncthreads();
    if (!active || r != 0) return;
    for (int rr = 1; rr < RB; ++rr) {   // the workgroup's rows r = 1 .. RB - 1 onto r = 0, ascending
        const int t = rr * LW + tid;    // (r == 0: tid is the lane's column group inside the tile)
#pragma unroll
        for (int u = 0; u < V; ++u) {
            if (MODE == POOL_MAX) max_merge(acc[u], at[u], s_val[t * V + u], s_arg[t * V + u]);
            else acc[u] += s_val[t * V + u];
        }
    }
    const int64_t prow = (int64_t)b * chunks + chunk;
    stv<V>(part + (prow * CG + cg) * V, acc);
    if (MODE == POOL_MAX) stv<V>(part_arg + (prow * CG + cg) * V, at);
}

// y[b][c] from the scan's partial rows in workgroup order (one thread per element, eight loads in flight)
__global__ __launch_bounds__(256) void k_pool_global_finish(const float *__restrict__ part,
                                                            const int32_t *__restrict__ part_arg,
                                                            const int32_t *__restrict__ seg_off, int B, int C, int rows,
                                                            int mode, float *__restrict__ y, int32_t *__restrict__ arg) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * C) return;
    const int b = idx / C, c = idx % C;
    const float *p = part + (int64_t)b * rows * C + c;
    const int32_t *pa = part_arg + (int64_t)b * rows * C + c;
    float acc = 0.f;
    int at = -1;
    for (int j0 = 0; j0 < rows; j0 += 8) {
        float v[8];
        int a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int jj = j0 + j < rows ? j0 + j : rows - 1;
            v[j] = p[(int64_t)jj * C];
            a[j] = mode == POOL_MAX ? pa[(int64_t)jj * C] : 0;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j0 + j < rows) {
                if (mode == POOL_MAX) max_merge(acc, at, v[j], a[j]);
                else acc += v[j];
            }
        }
    }
    if (mode == POOL_MAX) {
        arg[idx] = at;
    } else {
        const int nb = seg_off[b + 1] - seg_off[b];
        if (mode == POOL_AVG && nb > 0) acc = acc / (float)nb;
    }
    y[idx] = acc;
}

template <int V>
__global__ __launch_bounds__(256) void k_pool_global_bwd(const float *__restrict__ gy, const int32_t *__restrict__ arg,
                                                         const int32_t *__restrict__ bid,
                                                         const int32_t *__restrict__ seg_off, int64_t n, int CG, int mode,
                                                         float *__restrict__ gx) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * CG) return;
    const int64_t i = idx / CG;
    const int cg = (int)(idx % CG);
    const int b = bid[i];
    float g[V];
    ldv<V>(gy + ((int64_t)b * CG + cg) * V, g);
    if (mode == POOL_AVG) {
        const float cnt = (float)(seg_off[b + 1] - seg_off[b]);   // >= 1: row i is in it
#pragma unroll
        for (int u = 0; u < V; ++u) g[u] = g[u] / cnt;
    } else if (mode == POOL_MAX) {
        int a[V];
        ldv<V>(arg + ((int64_t)b * CG + cg) * V, a);
#pragma unroll
        for (int u = 0; u < V; ++u) g[u] = (a[u] == (int)i) ? g[u] : 0.f;
    }
    stv<V>(gx + idx * V, g);
}

int rows_args_ok(const void *x, const int32_t *row_ptr, const int32_t *row_list, const int32_t *other, const void *y,
                 int64_t n, int32_t C, const char *who) {
    LIDOG_REQUIRE(C >= 1, "%s: C must be >= 1 (got %d)", who, (int)C);
    LIDOG_REQUIRE(n >= 0, "%s: negative row count", who);
    if (n == 0) return 0;
    LIDOG_REQUIRE(x && row_ptr && row_list && other && y, "%s: null argument", who);
    LIDOG_REQUIRE(n < (int64_t)1 << 31 && cdiv64(n * (C % 4 ? C : C / 4), 256) < (int64_t)1 << 31, "%s: too many rows", who);
    return 0;
}

}  // namespace

extern "C" int lidog_pool_rows(const float *x, const int32_t *row_ptr, const int32_t *row_list, const int32_t *other,
                               int64_t n, int32_t C, int32_t avg, const int32_t *other_row_ptr, float *y, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = rows_args_ok(x, row_ptr, row_list, other, y, n, C, "pool_rows")) return rc;
    if (n == 0) return 0;
    if (C % 4 == 0)
        k_pool_rows<4><<<(unsigned)cdiv64(n * (C / 4), 256), 256, 0, st>>>(x, row_ptr, row_list, other, other_row_ptr, n,
                                                                           C / 4, avg, y);
    else
        k_pool_rows<1><<<(unsigned)cdiv64(n * C, 256), 256, 0, st>>>(x, row_ptr, row_list, other, other_row_ptr, n, C,
                                                                     avg, y);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_pool_rows_max(const float *x, const int32_t *row_ptr, const int32_t *row_list,
                                   const int32_t *other, int64_t n, int32_t C, float *y, int32_t *arg, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = rows_args_ok(x, row_ptr, row_list, other, y, n, C, "pool_rows_max")) return rc;
    if (n == 0) return 0;
    LIDOG_REQUIRE(arg, "pool_rows_max: null argument");
    if (C % 4 == 0)
        k_pool_rows_max<4><<<(unsigned)cdiv64(n * (C / 4), 256), 256, 0, st>>>(x, row_ptr, row_list, other, n, C / 4, y,
                                                                               arg);
    else
        k_pool_rows_max<1><<<(unsigned)cdiv64(n * C, 256), 256, 0, st>>>(x, row_ptr, row_list, other, n, C, y, arg);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_pool_rows_max_bwd(const float *gy, const int32_t *arg, const int32_t *row_ptr,
                                       const int32_t *row_list, const int32_t *other, int64_t n, int32_t C, float *gx,
                                       void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = rows_args_ok(gy, row_ptr, row_list, other, gx, n, C, "pool_rows_max_bwd")) return rc;
    if (n == 0) return 0;
    LIDOG_REQUIRE(arg, "pool_rows_max_bwd: null argument");
    if (C % 4 == 0)
        k_pool_rows_max_bwd<4><<<(unsigned)cdiv64(n * (C / 4), 256), 256, 0, st>>>(gy, arg, row_ptr, row_list, other, n,
                                                                                   C / 4, gx);
    else
        k_pool_rows_max_bwd<1><<<(unsigned)cdiv64(n * C, 256), 256, 0, st>>>(gy, arg, row_ptr, row_list, other, n, C, gx);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t lidog_pool_global_ws(int64_t n, int32_t B, int32_t C) {
    if (n <= 0 || B <= 0 || C < 1) return 0;
    const GlobalShape s = global_shape(n, B, C);
    return (int64_t)B * s.chunks * C * 8;   // a float and an int32 per partial element
}

extern "C" int lidog_pool_global(const float *x, int64_t n, int32_t C, int32_t B, const int32_t *perm,
                                 const int32_t *seg_off, int32_t mode, float *y, int32_t *arg, void *ws,
                                 int64_t ws_bytes, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(C >= 1, "pool_global: C must be >= 1 (got %d)", (int)C);
    LIDOG_REQUIRE(n >= 0 && B >= 0 && B <= 4096, "pool_global: bad row or scan count");
    LIDOG_REQUIRE(mode >= POOL_SUM && mode <= POOL_MAX, "pool_global: mode must be 0 (sum), 1 (avg) or 2 (max)");
    if (B == 0) return 0;
    LIDOG_REQUIRE(y && (mode != POOL_MAX || arg), "pool_global: null result");
    if (n == 0) {   // no rows at all: zeros and arg = -1, nothing read
        LIDOG_CHECK_HIP(hipMemsetAsync(y, 0, sizeof(float) * (size_t)B * C, st));
        if (mode == POOL_MAX) LIDOG_CHECK_HIP(hipMemsetAsync(arg, 0xFF, sizeof(int32_t) * (size_t)B * C, st));
        return 0;
    }
    LIDOG_REQUIRE(x && perm && seg_off && ws, "pool_global: null argument");
    LIDOG_REQUIRE(n < (int64_t)1 << 31, "pool_global: too many rows");
    LIDOG_REQUIRE(ws_bytes >= lidog_pool_global_ws(n, B, C), "pool_global: workspace too small");
    const GlobalShape s = global_shape(n, B, C);
    const int rows = s.chunks;
    float *part = (float *)ws;
    int32_t *part_arg = (int32_t *)(part + (size_t)B * rows * C);
    const dim3 grid((unsigned)s.chunks, (unsigned)B, (unsigned)s.ctiles);
#define POOL_GLOBAL_PART(V, MODE) \
    k_pool_global_part<V, MODE><<<grid, 256, 0, st>>>(x, perm, seg_off, s.CG, s.LW, s.RB, part, part_arg)
    if (s.V == 4) {
        if (mode == POOL_MAX) POOL_GLOBAL_PART(4, POOL_MAX); else POOL_GLOBAL_PART(4, POOL_SUM);
    } else {
        if (mode == POOL_MAX) POOL_GLOBAL_PART(1, POOL_MAX); else POOL_GLOBAL_PART(1, POOL_SUM);
    }
#undef POOL_GLOBAL_PART
    LIDOG_LAUNCH_CHECK();
    k_pool_global_finish<<<(unsigned)cdiv64((int64_t)B * C, 256), 256, 0, st>>>(part, part_arg, seg_off, B, C, rows, mode,
                                                                                y, arg);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_pool_global_bwd(const float *gy, const int32_t *arg, int64_t n, int32_t C, int32_t B,
                                     const int32_t *bid, const int32_t *seg_off, int32_t mode, float *gx, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(C >= 1, "pool_global_bwd: C must be >= 1 (got %d)", (int)C);
    LIDOG_REQUIRE(n >= 0 && B >= 0, "pool_global_bwd: bad row or scan count");
    LIDOG_REQUIRE(mode >= POOL_SUM && mode <= POOL_MAX, "pool_global_bwd: mode must be 0 (sum), 1 (avg) or 2 (max)");
    if (n == 0) return 0;
    LIDOG_REQUIRE(gy && bid && seg_off && gx && (mode != POOL_MAX || arg), "pool_global_bwd: null argument");
    LIDOG_REQUIRE(B >= 1 && n < (int64_t)1 << 31, "pool_global_bwd: rows without a scan, or too many rows");
    if (C % 4 == 0)
        k_pool_global_bwd<4><<<(unsigned)cdiv64(n * (C / 4), 256), 256, 0, st>>>(gy, arg, bid, seg_off, n, C / 4, mode, gx);
    else
        k_pool_global_bwd<1><<<(unsigned)cdiv64(n * C, 256), 256, 0, st>>>(gy, arg, bid, seg_off, n, C, mode, gx);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
