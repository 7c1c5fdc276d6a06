// Density clustering for the SN (statistical normalisation) baseline: sklearn.cluster.DBSCAN(eps, min_samples)
// .fit_predict(coordinates * voxel_size) as train_scaling_based.py:35-87 (get_average_dims) calls it on the car voxels
// of a scan, the per-cluster voxel counts and integer bounding boxes its statistics are made of, and the coordinate
// scaling of SingleSNSourceDataset.__getitem__ / MultiSNSourceDataset.merge_data (utils/datasets/sn_scaling.py:36-71,
// 107-175).
//
// DBSCAN's labels are a pure function of the neighbour graph:
//   core[i]   = #{j : dist(i, j) <= eps, i itself included} >= min_samples
//   clusters  = connected components of the core points under the neighbour relation, numbered 0, 1, 2, ... in the
//               order of their smallest member (sklearn grows them in index order)
//   border    = a non-core point takes the smallest cluster number among its core neighbours, none -> noise (-1)
// The neighbour predicate is sklearn's: on x = float32(c) * float32(voxel), the float32 array the reference hands over,
// sum_k (double(x_i[k]) - double(x_j[k]))^2 <= eps^2 in float64, summed in axis order.  Voxels are lattice points: a
// pair exactly on the sphere (offset (6, 8, 0) at eps 0.5, voxel 0.05) is decided by the float32 rounding of c * voxel,
// which the integer test d^2 <= 100 gets wrong, so every candidate pair goes through the float64 test.
//
// The points are binned into cubic cells of `cell` >= eps / voxel voxels (relative to the input's bounding box, so the
// cell key fits 32 bits) and sorted by cell with the tree's stable radix sort; a point's candidates are the 27 cells
// around its own, found as 9 contiguous key ranges by binary search.  Components: every core point first hangs under
// its smallest core neighbour, then union-find over the core-core pairs, the larger root hooked under the smaller with
// an integer atomicMin, so a component's root is its smallest member whatever the arrival order.  Only integer atomics whose result does not depend on their order, and no position taken
// by an atomic counter: the same bytes on every run.
#include <limits.h>

#include "common.h"
#include "prims.h"

#define CL_THREADS 256
#define CL_WAVES (CL_THREADS / 64)
#define CL_MAX_KEY 0xffffffffll // the cell key has 32 bits
#define CL_BOX_BINS 256         // clusters per LDS pass of the box kernel
#define CL_MAX_COORD 65535      // the coordinate hash's documented range (common.h:lidog_pack)
#define CL_ERR_RANGE 1
#define CL_ERR_GRID 2

// grid[0..2] = min, grid[3..5] = max of the coordinates, grid[6..8] = cells per axis
#define CL_GRID_INTS 16

__device__ __forceinline__ int cl_load(const int32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void k_cl_init(int32_t *grid, int32_t *info) {
    const int t = threadIdx.x;
    if (t < 3) grid[t] = INT_MAX;
    else if (t < 6) grid[t] = INT_MIN;
    else if (t < CL_GRID_INTS) grid[t] = 0;
    if (t < 2) info[t] = 0;
}

__global__ __launch_bounds__(CL_THREADS) void k_cl_bbox(const int32_t *__restrict__ coords, int64_t n, int32_t *grid,
                                                        int32_t *info) {
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
    int bad = 0;
    const int64_t stride = (int64_t)gridDim.x * CL_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x; i < n; i += stride) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int c = coords[3 * i + d];
            lo[d] = min(lo[d], c);
            hi[d] = max(hi[d], c);
            bad |= (c > CL_MAX_COORD) | (c < -CL_MAX_COORD);
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        for (int o = 32; o > 0; o >>= 1) {
            lo[d] = min(lo[d], __shfl_xor(lo[d], o));
            hi[d] = max(hi[d], __shfl_xor(hi[d], o));
        }
    }
    const bool any_bad = __ballot(bad) != 0ull;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            atomicMin(&grid[d], lo[d]);
            atomicMax(&grid[3 + d], hi[d]);
        }
        if (any_bad) atomicOr(&info[0], CL_ERR_RANGE);
    }
}

__global__ void k_cl_grid(int32_t *grid, int32_t cell, int32_t *info) {
    if (threadIdx.x != 0 || info[0]) return;
    uint64_t cells = 1;
    for (int d = 0; d < 3; ++d) {
        const int dim = (grid[3 + d] - grid[d]) / cell + 1;
        grid[6 + d] = dim;
        cells *= (uint64_t)dim;       // three factors below 2^18
    }
    if (cells > ((uint64_t)1 << 32)) info[0] = CL_ERR_GRID;
}

__global__ __launch_bounds__(CL_THREADS) void k_cl_keys(const int32_t *__restrict__ coords, int64_t n,
                                                        const int32_t *__restrict__ grid, int32_t cell,
                                                        const int32_t *__restrict__ info, uint32_t *__restrict__ keys,
                                                        int32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t key = 0;
    if (!info[0]) {
        const int cx = (coords[3 * i] - grid[0]) / cell, cy = (coords[3 * i + 1] - grid[1]) / cell,
                  cz = (coords[3 * i + 2] - grid[2]) / cell;
        key = (uint32_t)(((uint64_t)cx * grid[7] + cy) * grid[8] + cz);
    }
    keys[i] = key;
    vals[i] = (int32_t)i;
}

// sorted[j] = (x, y, z, input row) of the j-th point in cell order; parent[i] = i
__global__ __launch_bounds__(CL_THREADS) void k_cl_gather(const int32_t *__restrict__ coords,
                                                          const int32_t *__restrict__ rows, int64_t n,
                                                          int4 *__restrict__ sorted, int32_t *__restrict__ parent) {
    const int64_t j = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
    if (j >= n) return;
    const int i = rows[j];
    sorted[j] = make_int4(coords[3 * i], coords[3 * i + 1], coords[3 * i + 2], i);
    parent[j] = (int32_t)j;
}

struct ClSpace {
    const uint32_t *keys;   // sorted cell keys
    const int4 *sorted;     // (x, y, z, input row) in the same order
    const int32_t *grid;
    int64_t n;
    int32_t cell;
    float voxel;
    double eps2;
};

// One wave per point: the lanes share the candidate ranges, 64 candidates per round, so that a scan of ten thousand
// points keeps tens of waves per compute unit in flight behind the loads of its candidate walks (one thread per point
// left one wave per unit and ran at one memory latency per candidate).
// f(hit, j2, point j2) is called by all 64 lanes for every round of candidates; hit: the lane's candidate exists,
// passes pre(point) and lies within eps of `me` (`me` itself included).  f returns a wave-uniform "go on".
template <class P, class F>
__device__ __forceinline__ void cl_neighbours(const ClSpace &s, int4 me, int lane, P pre, F f) {
    const int cx = (me.x - s.grid[0]) / s.cell, cy = (me.y - s.grid[1]) / s.cell, cz = (me.z - s.grid[2]) / s.cell;
    const int dx = s.grid[6], dy = s.grid[7], dz = s.grid[8];
    const double mx = (double)((float)me.x * s.voxel), my = (double)((float)me.y * s.voxel),
                 mz = (double)((float)me.z * s.voxel);
    const int z0 = max(cz - 1, 0), z1 = min(cz + 1, dz - 1);
    for (int ax = -1; ax <= 1; ++ax) {
        const int nx = cx + ax;
        if (nx < 0 || nx >= dx) continue;
        for (int ay = -1; ay <= 1; ++ay) {
            const int ny = cy + ay;
            if (ny < 0 || ny >= dy) continue;
            const uint64_t base = ((uint64_t)nx * dy + ny) * dz;     // the cells (nx, ny, z0..z1) are consecutive keys
            const int64_t lo = key_lower_bound(s.keys, s.n, base + z0);
            const int64_t hi = key_lower_bound(s.keys, s.n, base + z1 + 1);
            for (int64_t j0 = lo; j0 < hi; j0 += 64) {
                const int64_t j2 = j0 + lane;
                const bool active = j2 < hi;
                const int4 o = active ? s.sorted[j2] : me;
                bool hit = active && pre(o);
                if (hit) {
                    const double a = (double)((float)o.x * s.voxel) - mx, b = (double)((float)o.y * s.voxel) - my,
                                 c = (double)((float)o.z * s.voxel) - mz;
                    const double d2 = a * a + b * b + c * c;
                    hit = d2 <= s.eps2;
                }
                if (!f(hit, j2, o)) return;
            }
        }
    }
}

// the point of this wave, -1 past the end (wave-uniform)
__device__ __forceinline__ int64_t cl_wave_point(int64_t n) {
    const int64_t j = (int64_t)blockIdx.x * CL_WAVES + (threadIdx.x >> 6);
    return j < n ? j : -1;
}

// core flags, in sorted order (core_s) and in input order (core_o); the count stops at min_samples
__global__ __launch_bounds__(CL_THREADS) void k_cl_count(ClSpace s, int32_t min_samples,
                                                         const int32_t *__restrict__ info,
                                                         int32_t *__restrict__ core_s, int32_t *__restrict__ core_o) {
    const int64_t j = cl_wave_point(s.n);
    if (j < 0 || info[0]) return;
    const int lane = threadIdx.x & 63;
    const int4 me = s.sorted[j];
    int cnt = 0;
    cl_neighbours(s, me, lane, [](int4) { return true; }, [&](bool hit, int64_t, int4) {
        cnt += __popcll(__ballot(hit));
        return cnt < min_samples;
    });
    if (lane == 0) {
        const int c = cnt >= min_samples;
        core_s[j] = c;
        core_o[me.w] = c;
    }
}

// root of x; every parent is <= its child, so the walk ends.  Halves the path on the way (atomicMin: a parent only
// ever moves to an ancestor, whatever else is going on).
__device__ __forceinline__ int cl_find(int32_t *parent, int x) {
    int px = cl_load(parent + x);
    while (px != x) {
        const int gp = cl_load(parent + px);
        if (gp != px) atomicMin(&parent[x], gp);
        x = px;
        px = gp;
    }
    return x;
}

__device__ __forceinline__ int cl_root(const int32_t *parent, int x) {
    for (;;) {
        const int px = cl_load(parent + x);
        if (px == x) return x;
        x = px;
    }
}

__device__ __forceinline__ void cl_union(int32_t *parent, int a, int b) {
    for (;;) {
        a = cl_find(parent, a);
        b = cl_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        // hook the larger root a under b.  old == a: a was still a root, done.  Otherwise someone hooked a under
        // `old` first (parent[a] is now min(old, b), an ancestor either way) and old and b are still to be joined.
        const int old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}

// Before any union: every core point hangs itself under its smallest core neighbour (itself included), a plain store
// to its own entry.  Parents stay <= children and inside the component, and the forest already has one tree per
// local minimum instead of one per point; k_cl_compress then points every entry at its tree's root.  The union pass
// that follows finds nearly every pair joined already: it is bound by the loads of the few hot root entries, and this
// cuts them to the pairs that straddle two basins.
__global__ __launch_bounds__(CL_THREADS) void k_cl_hook(ClSpace s, const int32_t *__restrict__ info,
                                                        const int32_t *__restrict__ core_s,
                                                        int32_t *__restrict__ parent) {
    const int64_t j = cl_wave_point(s.n);
    if (j < 0 || info[0] || !core_s[j]) return;
    const int4 me = s.sorted[j];
    int best = me.w;
    cl_neighbours(s, me, threadIdx.x & 63, [&](int4 o) { return o.w < me.w; }, [&](bool hit, int64_t j2, int4 o) {
        if (hit && core_s[j2]) best = min(best, o.w);
        return true;
    });
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
    if ((threadIdx.x & 63) == 0) parent[me.w] = best;
}

// parent[i] = root of i.  Entries move to ancestors only, so a walk that meets a half-updated chain still ends at the root.
__global__ __launch_bounds__(CL_THREADS) void k_cl_compress(int32_t *parent, int64_t n, const int32_t *__restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
    if (i >= n || info[0]) return;
    const int r = cl_root(parent, (int)i);
    if (r != (int)i) atomicMin(&parent[i], r);
}

__global__ __launch_bounds__(CL_THREADS) void k_cl_union(ClSpace s, const int32_t *__restrict__ info,
                                                         const int32_t *__restrict__ core_s, int32_t *parent) {
    const int64_t j = cl_wave_point(s.n);
    if (j < 0 || info[0] || !core_s[j]) return;
    const int4 me = s.sorted[j];
    int root = cl_find(parent, me.w);
    // every pair once, from its larger row.  Most pairs join points that are joined already: one load tells when the
    // neighbour hangs directly under this point's last known root.
    cl_neighbours(s, me, threadIdx.x & 63, [&](int4 o) { return o.w < me.w; }, [&](bool hit, int64_t j2, int4 o) {
        if (hit && core_s[j2] && cl_load(parent + o.w) != root) {
            cl_union(parent, me.w, o.w);
            root = cl_find(parent, me.w);
        }
        return true;
    });
}

// number[i] = core roots among the rows before i (exclusive scan in input order, one workgroup, chunks of
// 4 * CL_THREADS with a carry); info[1] = the number of clusters
__global__ __launch_bounds__(CL_THREADS) void k_cl_number(const int32_t *__restrict__ core_o,
                                                          const int32_t *__restrict__ parent, int64_t n,
                                                          int32_t *__restrict__ number, int32_t *info) {
    if (info[0]) return;
    const int tot = block_scan_chunks<CL_THREADS, 4>(
        n, [&](int64_t i) { return (int)(core_o[i] && parent[i] == (int32_t)i); },
        [&](int64_t i, int e) { number[i] = e; });
    if (threadIdx.x == 0) info[1] = tot;
}

__global__ __launch_bounds__(CL_THREADS) void k_cl_label(ClSpace s, const int32_t *__restrict__ info,
                                                         const int32_t *__restrict__ core_s,
                                                         const int32_t *__restrict__ parent,
                                                         const int32_t *__restrict__ number,
                                                         int32_t *__restrict__ labels) {
    const int64_t j = cl_wave_point(s.n);
    if (j < 0 || info[0]) return;
    const int lane = threadIdx.x & 63;
    const int4 me = s.sorted[j];
    if (core_s[j]) {
        if (lane == 0) labels[me.w] = number[cl_root(parent, me.w)];
        return;
    }
    int best = INT_MAX;
    cl_neighbours(s, me, lane, [](int4) { return true; }, [&](bool hit, int64_t j2, int4 o) {
        if (hit && core_s[j2]) best = min(best, number[cl_root(parent, o.w)]);
        return true;
    });
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
    if (lane == 0) labels[me.w] = best == INT_MAX ? -1 : best;
}

extern "C" int64_t lidog_dbscan_ws(int64_t n) {
    if (n <= 0) return 256;
    return lidog_align256(4 * CL_GRID_INTS) + 8 * lidog_align256(4 * n) + lidog_align256(16 * n) +
           lidog_align256(4 * lidog_radix_sort_hist_ints(n, lidog_radix_passes(CL_MAX_KEY)));
}

extern "C" int lidog_dbscan(const int32_t *coords, int64_t n, float voxel_size, double eps, int32_t min_samples,
                            int32_t *labels, int32_t *info, void *ws, int64_t ws_bytes, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX, "lidog_dbscan: n = %lld out of range", (long long)n);
    LIDOG_REQUIRE(voxel_size > 0.f && eps > 0.0 && min_samples >= 1,
                  "lidog_dbscan: voxel_size %g, eps %g, min_samples %d (all must be positive)", (double)voxel_size, eps,
                  min_samples);
    LIDOG_REQUIRE(info != nullptr, "lidog_dbscan: info [2] required");
    if (n == 0) {
        LIDOG_CHECK_HIP(hipMemsetAsync(info, 0, 2 * sizeof(int32_t), st));
        return 0;
    }
    LIDOG_REQUIRE(coords && labels && ws, "lidog_dbscan: coords, labels and the workspace are required");
    LIDOG_REQUIRE(ws_bytes >= lidog_dbscan_ws(n), "lidog_dbscan: workspace too small");
    // cell edge in voxels.  Two points in cells two apart differ by >= cell + 1 voxels on an axis, i.e. by at least
    // (cell + 1) * voxel - voxel / 128 metres (|c| <= 65535: float32(c) * voxel is off by at most 2^-24 of 65536
    // voxels), which is more than eps when cell >= eps / voxel.
    const double ratio = eps / (double)voxel_size;
    LIDOG_REQUIRE(ratio < 4096.0, "lidog_dbscan: eps / voxel_size = %g (at most 4096)", ratio);
    int32_t cell = (int32_t)ratio;
    if ((double)cell < ratio) ++cell;
    if (cell < 1) cell = 1;

    char *p = (char *)ws;
    int32_t *grid = (int32_t *)p;     p += lidog_align256(4 * CL_GRID_INTS);
    uint32_t *ka = (uint32_t *)p;     p += lidog_align256(4 * n);
    uint32_t *kb = (uint32_t *)p;     p += lidog_align256(4 * n);
    int32_t *va = (int32_t *)p;       p += lidog_align256(4 * n);
    int32_t *vb = (int32_t *)p;       p += lidog_align256(4 * n);
    int32_t *core_s = (int32_t *)p;   p += lidog_align256(4 * n);
    int32_t *core_o = (int32_t *)p;   p += lidog_align256(4 * n);
    int32_t *parent = (int32_t *)p;   p += lidog_align256(4 * n);
    int32_t *number = (int32_t *)p;   p += lidog_align256(4 * n);
    int4 *sorted = (int4 *)p;         p += lidog_align256(16 * n);
    int32_t *hist = (int32_t *)p;

    const unsigned blocks = (unsigned)cdiv64(n, CL_THREADS);
    k_cl_init<<<1, 64, 0, st>>>(grid, info);
    k_cl_bbox<<<blocks < 256u ? blocks : 256u, CL_THREADS, 0, st>>>(coords, n, grid, info);
    k_cl_grid<<<1, 64, 0, st>>>(grid, cell, info);
    k_cl_keys<<<blocks, CL_THREADS, 0, st>>>(coords, n, grid, cell, info, ka, va);
    LIDOG_LAUNCH_CHECK();
    const int passes = lidog_radix_passes(CL_MAX_KEY);
    if (lidog_radix_sort_pairs(ka, va, kb, vb, n, passes, hist, st)) return 1;
    // an odd count of passes leaves the sorted pairs in (kb, vb)
    k_cl_gather<<<blocks, CL_THREADS, 0, st>>>(coords, (passes & 1) ? vb : va, n, sorted, parent);
    ClSpace s = {(passes & 1) ? kb : ka, sorted, grid, n, cell, voxel_size, eps * eps};
    const unsigned wblocks = (unsigned)cdiv64(n, CL_WAVES);      // one wave per point
    k_cl_count<<<wblocks, CL_THREADS, 0, st>>>(s, min_samples, info, core_s, core_o);
    k_cl_hook<<<wblocks, CL_THREADS, 0, st>>>(s, info, core_s, parent);
    k_cl_compress<<<blocks, CL_THREADS, 0, st>>>(parent, n, info);
    k_cl_union<<<wblocks, CL_THREADS, 0, st>>>(s, info, core_s, parent);
    k_cl_number<<<1, CL_THREADS, 0, st>>>(core_o, parent, n, number, info);
    k_cl_label<<<wblocks, CL_THREADS, 0, st>>>(s, info, core_s, parent, number, labels);
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ per-cluster counts and integer boxes
__global__ __launch_bounds__(CL_THREADS) void k_cl_box_init(int32_t k, unsigned long long *counts, int32_t *lo,
                                                            int32_t *hi) {
    const int i = blockIdx.x * CL_THREADS + threadIdx.x;
    if (i < k) counts[i] = 0ull;
    if (i < 3 * k) {
        lo[i] = INT_MAX;
        hi[i] = INT_MIN;
    }
}

// LDS counts / minima / maxima per workgroup (one pass per CL_BOX_BINS clusters), then one global integer atomic per
// workgroup per non-empty cluster
__global__ __launch_bounds__(CL_THREADS) void k_cl_boxes(const int32_t *__restrict__ coords,
                                                         const int32_t *__restrict__ labels, int64_t n, int32_t k,
                                                         unsigned long long *counts, int32_t *lo, int32_t *hi) {
    __shared__ int32_t c[CL_BOX_BINS], l[3 * CL_BOX_BINS], h[3 * CL_BOX_BINS];
    const int64_t stride = (int64_t)gridDim.x * CL_THREADS;
    for (int32_t b0 = 0; b0 < k; b0 += CL_BOX_BINS) {
        const int32_t nb = min(CL_BOX_BINS, k - b0);
        for (int q = threadIdx.x; q < nb; q += CL_THREADS) c[q] = 0;
        for (int q = threadIdx.x; q < 3 * nb; q += CL_THREADS) {
            l[q] = INT_MAX;
            h[q] = INT_MIN;
        }
        __syncthreads();
        for (int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x; i < n; i += stride) {
            const int64_t q = (int64_t)labels[i] - b0;
            if (q < 0 || q >= nb) continue;
            atomicAdd(&c[q], 1);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const int v = coords[3 * i + d];
                atomicMin(&l[3 * q + d], v);
                atomicMax(&h[3 * q + d], v);
            }
        }
        __syncthreads();
        for (int q = threadIdx.x; q < nb; q += CL_THREADS) {
            if (!c[q]) continue;
            atomicAdd(&counts[b0 + q], (unsigned long long)c[q]);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                atomicMin(&lo[3 * (b0 + q) + d], l[3 * q + d]);
                atomicMax(&hi[3 * (b0 + q) + d], h[3 * q + d]);
            }
        }
        __syncthreads();
    }
}

extern "C" int lidog_cluster_boxes(const int32_t *coords, const int32_t *labels, int64_t n, int32_t k, int64_t *counts,
                                   int32_t *lo, int32_t *hi, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0 && k >= 0, "lidog_cluster_boxes: n = %lld, k = %d", (long long)n, k);
    if (k == 0) return 0;
    LIDOG_REQUIRE(counts && lo && hi, "lidog_cluster_boxes: counts, lo and hi are required");
    k_cl_box_init<<<(unsigned)cdiv64(3 * (int64_t)k, CL_THREADS), CL_THREADS, 0, st>>>(
        k, (unsigned long long *)counts, lo, hi);
    if (n) {
        LIDOG_REQUIRE(coords && labels, "lidog_cluster_boxes: coords and labels are required");
        const int64_t blocks = cdiv64(n, CL_THREADS);
        k_cl_boxes<<<(unsigned)(blocks < 256 ? blocks : 256), CL_THREADS, 0, st>>>(
            coords, labels, n, k, (unsigned long long *)counts, lo, hi);
    }
    LIDOG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ SN coordinate scaling
// out[i][d] = (float(c[i][d]) * voxel) * scale[d]: `coordinates * voxel_size` (an int tensor times a Python float:
// float32), then `x[:, d] = x[:, d] * scaling[d]`, a float32 product (sn_scaling.py:39,53-55); two roundings
__global__ __launch_bounds__(CL_THREADS) void k_sn_scale(const int32_t *__restrict__ coords, int64_t n, float voxel,
                                                         float sx, float sy, float sz, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
    if (i >= n) return;
    const float x = (float)coords[3 * i] * voxel, y = (float)coords[3 * i + 1] * voxel,
                z = (float)coords[3 * i + 2] * voxel;
    out[3 * i] = x * sx;
    out[3 * i + 1] = y * sy;
    out[3 * i + 2] = z * sz;
}

extern "C" int lidog_sn_scale_coords(const int32_t *coords, int64_t n, float voxel_size, float sx, float sy, float sz,
                                     float *out, void *stream) {
    LIDOG_REQUIRE(n >= 0, "lidog_sn_scale_coords: n = %lld", (long long)n);
    if (n == 0) return 0;
    LIDOG_REQUIRE(coords && out, "lidog_sn_scale_coords: coords and out are required");
    k_sn_scale<<<(unsigned)cdiv64(n, CL_THREADS), CL_THREADS, 0, (hipStream_t)stream>>>(coords, n, voxel_size, sx, sy,
                                                                                      sz, out);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
