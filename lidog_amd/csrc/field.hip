// Point <-> voxel family (ME.TensorField, SparseTensor.slice / cat_slice / features_at_coordinates / interpolate,
// MinkowskiInterpolation of MinkowskiEngine 0.5; the reference never calls them, semantics restated [ME-mem]).
// Contract: include/lidog_amd.h.
//
// Every result is a gather written with plain stores, in an order the contract names: no atomics, the same bits on
// every call.  The lists a gradient walks come from ONE stable sort (lidog_group_by_key of prims.hip, as
// lidog_in_segments uses it): entry j of an index table goes to the list of the row it names, ascending j inside a list.
// For a field that table is the inverse map (point -> voxel); for the interpolation gradient it is the neighbour table
// nbr [8][Q] itself, whose flat index j = k * Q + q ascends in k and then in q -- the order the contract gives the sum.
// (The rule book's pos_in holds ONE pair per (offset, input row); many queries share a cell, so it cannot list them.)
// Row kernels follow pool.hip: thread idx = row idx / CG, column group idx % CG (float4 groups when C % 4 == 0), so the
// lanes of a row read consecutive 16-byte pieces of one gathered row; loads go out in unconditional batches of 4.
#include "common.h"
#include "prims.h"

namespace {

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
__device__ __forceinline__ void stv(float *__restrict__ p, const float (&v)[V]) {
    if constexpr (V == 4) *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}

// ---------------------------------------------------------------- floor of a field's coordinates
constexpr int FIELD_ERR_BATCH = 1, FIELD_ERR_NONFINITE = 2;

__device__ __forceinline__ bool finite_f(float v) { return v - v == 0.f; }

__global__ __launch_bounds__(256) void k_field_floor(const float4 *__restrict__ pts, int64_t n, float s,
                                                     int4 *__restrict__ rows, int32_t *__restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    int bad = 0;
    int b = -1;   // a row with a bad batch column matches no map row
    if (p.x >= 0.f && p.x <= 4095.f && floorf(p.x) == p.x) b = (int)p.x;
    else bad |= FIELD_ERR_BATCH;
    if (!finite_f(p.y) || !finite_f(p.z) || !finite_f(p.w)) bad |= FIELD_ERR_NONFINITE;
    rows[i] = make_int4(b, lidog_voxel_coord(floorf(p.y / s) * s), lidog_voxel_coord(floorf(p.z / s) * s),
                        lidog_voxel_coord(floorf(p.w / s) * s));
    if (bad) atomicOr(err, bad);
}

// ---------------------------------------------------------------- per-row lists of an index table
__global__ __launch_bounds__(256) void k_field_keys(const int32_t *__restrict__ inv, int64_t n, int32_t m,
                                                    uint32_t *__restrict__ keys, int32_t *__restrict__ vals) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int32_t v = inv[j];
    keys[j] = ((uint32_t)v < (uint32_t)m) ? (uint32_t)v : (uint32_t)m;   // names no row: behind every list
    vals[j] = (int32_t)j;
}

// ---------------------------------------------------------------- ordered segment sum / mean
template <int V>
__global__ __launch_bounds__(256) void k_field_reduce(const float *__restrict__ x, int64_t n_x,
                                                      const int32_t *__restrict__ row_ptr,
                                                      const int32_t *__restrict__ row_list, int64_t m, int CG, int mean,
                                                      float *__restrict__ y) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= m * CG) return;
    const int64_t r = idx / CG;
    const int cg = (int)(idx % CG);
    const int b = row_ptr[r], e = row_ptr[r + 1];
    float acc[V];
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] = 0.f;
    for (int p = b; p < e; p += 4) {
        int o[4];
        float t[4][V];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = row_list[p + j < e ? p + j : e - 1];
            o[j] = ((uint32_t)o[j] < (uint64_t)n_x) ? o[j] : 0;   // never an address outside x
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) ldv<V>(x + ((int64_t)o[j] * CG + cg) * V, t[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = p + j < e;
            const bool first = p + j == b;
#pragma unroll
            for (int u = 0; u < V; ++u) acc[u] = first ? t[j][u] : (ok ? acc[u] + t[j][u] : acc[u]);
        }
    }
    if (mean && e > b) {   // an empty list stays exact zeros: no 0 / 0
        const float cnt = (float)(e - b);
#pragma unroll
        for (int u = 0; u < V; ++u) acc[u] = acc[u] / cnt;
    }
    stv<V>(y + idx * V, acc);
}

// ---------------------------------------------------------------- y[p] = x[inv[p]] (/ count of that row)
template <int V>
__global__ __launch_bounds__(256) void k_field_gather(const float *__restrict__ x, const int32_t *__restrict__ inv,
                                                      int64_t n, int64_t m, int CG,
                                                      const int32_t *__restrict__ row_ptr, float *__restrict__ y) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * CG) return;
    const int64_t p = idx / CG;
    const int cg = (int)(idx % CG);
    const int32_t v = inv[p];
    float g[V];
#pragma unroll
    for (int u = 0; u < V; ++u) g[u] = 0.f;
    if ((uint32_t)v < (uint64_t)m) {   // an entry that names no row: zeros
        ldv<V>(x + ((int64_t)v * CG + cg) * V, g);
        if (row_ptr) {
            const float cnt = (float)(row_ptr[v + 1] - row_ptr[v]);   // >= 1: p is in it
#pragma unroll
            for (int u = 0; u < V; ++u) g[u] = g[u] / cnt;
        }
    }
    stv<V>(y + idx * V, g);
}

// ---------------------------------------------------------------- trilinear interpolation
// per axis lo = floor(x / s) * s and the factors (lower, upper) of the two neighbours; w_k = f_x * f_y * f_z (that
// order), k = bx + 2 by + 4 bz.  The distance to the lattice point on the side of zero is exact in float32 and the other
// one is not (-4e-14 - (-1) rounds to 1 and would take all weight from the point's own cell), so the fraction is taken
// from the exact one: x >= 0: t = (x - lo) / s, factors (1 - t, t); x < 0: r = ((lo + s) - x) / s, factors (r, 1 - r).
struct Frac {
    float lo[3], up[3];
};
__device__ __forceinline__ void interp_axis(float x, float s, float &lower, float &upper) {
    const float lo = floorf(x / s) * s;
    if (x >= 0.f) {
        const float t = (x - lo) / s;
        lower = 1.f - t;
        upper = t;
    } else {
        const float r = ((lo + s) - x) / s;
        lower = r;
        upper = 1.f - r;
    }
}
__device__ __forceinline__ Frac interp_frac(const float4 q, float s) {
    Frac f;
    interp_axis(q.y, s, f.lo[0], f.up[0]);
    interp_axis(q.z, s, f.lo[1], f.up[1]);
    interp_axis(q.w, s, f.lo[2], f.up[2]);
    return f;
}
__device__ __forceinline__ float interp_weight(const Frac &f, int k) {
    const float fx = (k & 1) ? f.up[0] : f.lo[0];
    const float fy = (k & 2) ? f.up[1] : f.lo[1];
    const float fz = (k & 4) ? f.up[2] : f.lo[2];
    return fx * fy * fz;
}

template <int V>
__global__ __launch_bounds__(256) void k_interp_fwd(const float *__restrict__ F, int64_t m,
                                                    const float4 *__restrict__ query, const int32_t *__restrict__ nbr,
                                                    int64_t nq, int CG, float s, float *__restrict__ y) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nq * CG) return;
    const int64_t q = idx / CG;
    const int cg = (int)(idx % CG);
    const Frac f = interp_frac(query[q], s);
    int r[8];
    float t[8][V];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = nbr[(int64_t)k * nq + q];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        r[k] = ((uint32_t)r[k] < (uint64_t)m) ? r[k] : -1;   // absent, or no row of F
#pragma unroll
        for (int u = 0; u < V; ++u) t[k][u] = 0.f;
        if (r[k] >= 0) ldv<V>(F + ((int64_t)r[k] * CG + cg) * V, t[k]);
    }
    float acc[V];
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (r[k] >= 0) {
            const float w = interp_weight(f, k);
#pragma unroll
            for (int u = 0; u < V; ++u) acc[u] = fmaf(w, t[k][u], acc[u]);
        }
    }
    stv<V>(y + idx * V, acc);
}

// gF[i] = sum over the entries j = k * Q + q of row i's list (ascending j) of w_k(q) gy[q]
template <int V>
__global__ __launch_bounds__(256) void k_interp_bwd(const float *__restrict__ gy, const float4 *__restrict__ query,
                                                    int64_t nq, const int32_t *__restrict__ row_ptr,
                                                    const int32_t *__restrict__ row_list, int64_t m, int CG, float s,
                                                    float *__restrict__ gF) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= m * CG) return;
    const int64_t i = idx / CG;
    const int cg = (int)(idx % CG);
    const int b = row_ptr[i], e = row_ptr[i + 1];
    float acc[V];
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] = 0.f;
    for (int p = b; p < e; p += 4) {
        int64_t q[4];
        int k[4];
        float4 c[4];
        float t[4][V];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int64_t e_j = row_list[p + j < e ? p + j : e - 1];
            e_j = (e_j >= 0 && e_j < 8 * nq) ? e_j : 0;   // never an address outside gy / query
            k[j] = (int)(e_j / nq);
            q[j] = e_j % nq;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[j] = query[q[j]];
            ldv<V>(gy + (q[j] * CG + cg) * V, t[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (p + j < e) {
                const float w = interp_weight(interp_frac(c[j], s), k[j]);
#pragma unroll
                for (int u = 0; u < V; ++u) acc[u] = fmaf(w, t[j][u], acc[u]);
            }
        }
    }
    stv<V>(gF + idx * V, acc);
}

int field_shape_ok(int64_t rows, int32_t C, const char *who) {
    LIDOG_REQUIRE(C >= 1, "%s: C must be >= 1 (got %d)", who, (int)C);
    LIDOG_REQUIRE(rows >= 0, "%s: negative row count", who);
    LIDOG_REQUIRE(rows < (int64_t)1 << 31 && cdiv64(rows * (C % 4 ? C : C / 4), 256) < (int64_t)1 << 31,
                  "%s: too many rows", who);
    return 0;
}

}  // namespace

extern "C" int lidog_field_floor(const float *points, int64_t n, int32_t stride, int32_t *rows, int32_t *err,
                                 void *stream) {
    LIDOG_REQUIRE(stride >= 1, "field_floor: tensor stride must be >= 1 (got %d)", (int)stride);
    LIDOG_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "field_floor: bad row count");
    if (n == 0) return 0;
    LIDOG_REQUIRE(points && rows && err, "field_floor: null argument");
    k_field_floor<<<(unsigned)cdiv64(n, 256), 256, 0, (hipStream_t)stream>>>((const float4 *)points, n, (float)stride,
                                                                           (int4 *)rows, err);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t lidog_field_lists_ws(int64_t n, int64_t m) {
    if (n <= 0 || m < 0) return 256;
    return lidog_group_ws(n, lidog_radix_passes(m));
}

extern "C" int lidog_field_lists(const int32_t *inv, int64_t n, int64_t m, int32_t *row_ptr, int32_t *row_list, void *ws,
                                 int64_t ws_bytes, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0 && n < (int64_t)1 << 31 && m >= 0 && m < ((int64_t)1 << 31) - 1, "field_lists: n, m < 2^31");
    LIDOG_REQUIRE(row_ptr != nullptr, "field_lists: row_ptr [m + 1] required");
    if (n == 0) {
        LIDOG_CHECK_HIP(hipMemsetAsync(row_ptr, 0, sizeof(int32_t) * (size_t)(m + 1), st));
        return 0;
    }
    LIDOG_REQUIRE(inv && row_list && ws, "field_lists: inv, row_list and the workspace are required");
    LIDOG_REQUIRE(ws_bytes >= lidog_field_lists_ws(n, m), "field_lists: workspace too small");
    // row_ptr[v] = first sorted position whose key is >= v (v = 0 .. m): rows nobody names get empty lists
    const int passes = lidog_radix_passes(m);   // keys 0 .. m
    const LidogGroupBufs g = lidog_group_bufs(ws, n, passes, row_list);
    k_field_keys<<<(unsigned)cdiv64(n, 256), 256, 0, st>>>(inv, n, (int32_t)m, g.ka, g.va);
    LIDOG_LAUNCH_CHECK();
    return lidog_group_by_key(g, n, passes, m, row_ptr, st);
}

extern "C" int lidog_field_reduce(const float *x, int64_t n_x, const int32_t *row_ptr, const int32_t *row_list,
                                  int64_t m, int32_t C, int32_t mean, float *y, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = field_shape_ok(m, C, "field_reduce")) return rc;
    LIDOG_REQUIRE(n_x >= 0 && n_x < (int64_t)1 << 31, "field_reduce: bad source row count");
    if (m == 0) return 0;
    LIDOG_REQUIRE(row_ptr && y && (n_x == 0 || (x && row_list)), "field_reduce: null argument");
    if (n_x == 0) {   // every list is empty
        LIDOG_CHECK_HIP(hipMemsetAsync(y, 0, sizeof(float) * (size_t)m * C, st));
        return 0;
    }
    if (C % 4 == 0)
        k_field_reduce<4><<<(unsigned)cdiv64(m * (C / 4), 256), 256, 0, st>>>(x, n_x, row_ptr, row_list, m, C / 4, mean, y);
    else
        k_field_reduce<1><<<(unsigned)cdiv64(m * C, 256), 256, 0, st>>>(x, n_x, row_ptr, row_list, m, C, mean, y);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_field_gather(const float *x, const int32_t *inv, int64_t n, int64_t m, int32_t C,
                                  const int32_t *row_ptr, float *y, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = field_shape_ok(n, C, "field_gather")) return rc;
    LIDOG_REQUIRE(m >= 0 && m < (int64_t)1 << 31, "field_gather: bad source row count");
    if (n == 0) return 0;
    LIDOG_REQUIRE(inv && y && (m == 0 || x), "field_gather: null argument");
    if (C % 4 == 0)
        k_field_gather<4><<<(unsigned)cdiv64(n * (C / 4), 256), 256, 0, st>>>(x, inv, n, m, C / 4, row_ptr, y);
    else
        k_field_gather<1><<<(unsigned)cdiv64(n * C, 256), 256, 0, st>>>(x, inv, n, m, C, row_ptr, y);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_interp_fwd(const float *F, int64_t m, int32_t C, const float *query, const int32_t *nbr,
                                int64_t n_query, int32_t stride, float *y, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = field_shape_ok(n_query, C, "interp_fwd")) return rc;
    LIDOG_REQUIRE(stride >= 1, "interp_fwd: tensor stride must be >= 1 (got %d)", (int)stride);
    LIDOG_REQUIRE(m >= 0 && m < (int64_t)1 << 31 && n_query < (int64_t)1 << 28, "interp_fwd: bad row or query count");
    if (n_query == 0) return 0;
    LIDOG_REQUIRE(query && nbr && y && (m == 0 || F), "interp_fwd: null argument");
    if (C % 4 == 0)
        k_interp_fwd<4><<<(unsigned)cdiv64(n_query * (C / 4), 256), 256, 0, st>>>(F, m, (const float4 *)query, nbr,
                                                                                   n_query, C / 4, (float)stride, y);
    else
        k_interp_fwd<1><<<(unsigned)cdiv64(n_query * C, 256), 256, 0, st>>>(F, m, (const float4 *)query, nbr, n_query, C,
                                                                             (float)stride, y);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

extern "C" int lidog_interp_bwd(const float *gy, const float *query, int64_t n_query, const int32_t *row_ptr,
                                const int32_t *row_list, int64_t m, int32_t C, int32_t stride, float *gF, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = field_shape_ok(m, C, "interp_bwd")) return rc;
    LIDOG_REQUIRE(stride >= 1, "interp_bwd: tensor stride must be >= 1 (got %d)", (int)stride);
    LIDOG_REQUIRE(n_query >= 0 && n_query < (int64_t)1 << 28, "interp_bwd: bad query count");
    if (m == 0) return 0;
    LIDOG_REQUIRE(row_ptr && gF && (n_query == 0 || (gy && query && row_list)), "interp_bwd: null argument");
    if (n_query == 0) {   // nobody hits any row
        LIDOG_CHECK_HIP(hipMemsetAsync(gF, 0, sizeof(float) * (size_t)m * C, st));
        return 0;
    }
    if (C % 4 == 0)
        k_interp_bwd<4><<<(unsigned)cdiv64(m * (C / 4), 256), 256, 0, st>>>(gy, (const float4 *)query, n_query, row_ptr,
                                                                             row_list, m, C / 4, (float)stride, gF);
    else
        k_interp_bwd<1><<<(unsigned)cdiv64(m * C, 256), 256, 0, st>>>(gy, (const float4 *)query, n_query, row_ptr,
                                                                       row_list, m, C, (float)stride, gF);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
