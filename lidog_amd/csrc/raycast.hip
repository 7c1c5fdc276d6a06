// The Raycast baseline's resampler (configs/raycast/*): a source scan re-sampled onto a target sensor's (beam, azimuth)
// grid as a point-splat range image.  Every cell keeps the nearest source point that falls into it; the kept points
// leave in ascending cell order, optionally placed on their cell's ray.  DESIGN.md section 3y states the definition.
//
// The winner of a cell is one 64-bit integer atomicMin on (bits(r2) << 32) | row: r2 > 0, so its float32 bits order as
// the values do, and equal r2 falls to the smallest row.  An integer minimum does not depend on the order of arrival,
// and the kept cells take their positions from lidog_compact_rows (prims.hip), never from an atomic: the same bytes on
// every run.  Angles are float64 atan2 of the float32 differences; the positions of snapped points use the host's float64
// tables only (multiplies and a square root, IEEE on both sides).
#include "common.h"
#include "prims.h"

#define RC_THREADS 256
#define RC_MAX_BLOCKS 2048
#define RC_EMPTY 0xFFFFFFFFFFFFFFFFull
#define RC_TWO_PI 6.283185307179586

// int32 words in front of the compaction's own workspace: table [n_cells] uint64, occupied [n_cells], kept [n_cells],
// two spare words (ABI version 9 fixes the size)
static inline int64_t rc_ws_head(int64_t n_cells) { return 4 * n_cells + 2; }

__global__ __launch_bounds__(RC_THREADS) void k_rc_fill(unsigned long long *__restrict__ table, int64_t n_cells) {
    const int64_t step = (int64_t)gridDim.x * RC_THREADS;
    for (int64_t c = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; c < n_cells; c += step) table[c] = RC_EMPTY;
}

// the cell of every source row (-1: dropped) and the per-cell minimum of (bits(r2) << 32) | row
__global__ __launch_bounds__(RC_THREADS) void k_rc_splat(const float *__restrict__ pts, int64_t n,
                                                         const float *__restrict__ origin,
                                                         const double *__restrict__ edges, int32_t n_beams,
                                                         int32_t n_az, double az0, float min2, int32_t use_max,
                                                         float max2, int32_t *__restrict__ cell_out,
                                                         unsigned long long *table) {
#pragma clang fp contract(off)
    const float ox = origin ? origin[0] : 0.0f, oy = origin ? origin[1] : 0.0f, oz = origin ? origin[2] : 0.0f;
    const double az_step = RC_TWO_PI / (double)n_az;
    const double e_lo = edges[0], e_hi = edges[n_beams];
    const int64_t step = (int64_t)gridDim.x * RC_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; i < n; i += step) {
        const float qx = pts[3 * i] - ox, qy = pts[3 * i + 1] - oy, qz = pts[3 * i + 2] - oz;
        const float xx = qx * qx, yy = qy * qy, zz = qz * qz;
        const float xy = xx + yy;
        const float r2 = xy + zz;
        int32_t cell = -1;
        // written so that a NaN fails: r2 > 0 and the elevation inside [edges[0], edges[n_beams])
        if (r2 > 0.0f && !(r2 < min2) && !(use_max && r2 >= max2)) {
            const double dx = (double)qx, dy = (double)qy, dz = (double)qz;
            const double el = atan2(dz, sqrt(dx * dx + dy * dy));
            if (el >= e_lo && el < e_hi) {
                const double az = atan2(dy, dx);
                const long long k = (long long)floor((az - az0) / az_step + 0.5);
                int32_t c = (int32_t)(k % (long long)n_az);
                if (c < 0) c += n_az;
                int lo = 0, hi = n_beams;      // the last edge <= el: edges[lo] <= el < edges[hi] throughout
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (edges[mid] <= el) lo = mid;
                    else hi = mid;
                }
                cell = lo * n_az + c;
                atomicMin(&table[cell], ((unsigned long long)__float_as_uint(r2) << 32) | (unsigned long long)i);
            }
        }
        if (cell_out) cell_out[i] = cell;
    }
}

// occupied[c] = 1 for a cell with a winner, 0 otherwise: the flags of lidog_compact_rows
__global__ __launch_bounds__(RC_THREADS) void k_rc_flag(const unsigned long long *__restrict__ table, int64_t n_cells,
                                                        int32_t *__restrict__ occupied) {
    const int64_t step = (int64_t)gridDim.x * RC_THREADS;
    for (int64_t c = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; c < n_cells; c += step)
        occupied[c] = table[c] != RC_EMPTY ? 1 : 0;
}

// output row r: the winner of cell kept[r], r < *count
__global__ __launch_bounds__(RC_THREADS) void k_rc_emit(const float *__restrict__ pts, int64_t n,
                                                        const float *__restrict__ origin,
                                                        const unsigned long long *__restrict__ table,
                                                        const int32_t *__restrict__ kept,
                                                        const int32_t *__restrict__ count_dev, int64_t n_cells,
                                                        int32_t n_az, int32_t snap, const double *__restrict__ cos_el,
                                                        const double *__restrict__ sin_el,
                                                        const double *__restrict__ cos_az,
                                                        const double *__restrict__ sin_az,
                                                        float *__restrict__ points_out, int32_t *__restrict__ rows_out,
                                                        int32_t *m_dev) {
#pragma clang fp contract(off)
    const float ox = origin ? origin[0] : 0.0f, oy = origin ? origin[1] : 0.0f, oz = origin ? origin[2] : 0.0f;
    int64_t count = (int64_t)*count_dev;
    if (count > n) count = n;                                // one winner per cell, every winner a distinct row
    if (count > n_cells) count = n_cells;
    if (blockIdx.x == 0 && threadIdx.x == 0) m_dev[0] = (int32_t)count;
    const int64_t step = (int64_t)gridDim.x * RC_THREADS;
    for (int64_t r = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; r < count; r += step) {
        const int64_t cell = (int64_t)kept[r];
        if (cell < 0 || cell >= n_cells) continue;           // never read outside the table
        const int64_t i = (int64_t)(table[cell] & 0xFFFFFFFFull);
        if (i >= n) continue;                                // never read outside the scan
        const float qx = pts[3 * i] - ox, qy = pts[3 * i + 1] - oy, qz = pts[3 * i + 2] - oz;
        float *o = points_out + 3 * r;
        if (snap) {
            const int64_t b = cell / n_az, c = cell - b * n_az;
            const double dx = (double)qx, dy = (double)qy, dz = (double)qz;
            const double rr = sqrt(dx * dx + dy * dy + dz * dz);
            const double rc = rr * cos_el[b];
            o[0] = (float)(rc * cos_az[c]);
            o[1] = (float)(rc * sin_az[c]);
            o[2] = (float)(rr * sin_el[b]);
        } else {
            o[0] = qx; o[1] = qy; o[2] = qz;
        }
        rows_out[r] = (int32_t)i;
    }
}

extern "C" int64_t lidog_raycast_ws(int64_t n, int64_t n_cells) {
    (void)n;
    const int64_t c = n_cells > 0 ? n_cells : 0;
    return rc_ws_head(c) + lidog_compact_ws_ints(c);
}

extern "C" int lidog_raycast(const float *points, int64_t n, const float *origin, const double *edges, int32_t n_beams,
                             int32_t n_az, double az0, float min2, int32_t use_max, float max2, int32_t snap,
                             const double *cos_el, const double *sin_el, const double *cos_az, const double *sin_az,
                             int32_t *cell_out, float *points_out, int32_t *rows_out, int32_t *m_dev, int32_t *ws,
                             void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LIDOG_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX, "lidog_raycast: n = %lld out of range", (long long)n);
    LIDOG_REQUIRE(n_beams >= 2 && n_az >= 1, "lidog_raycast: %d beams x %d columns (at least 2 x 1)", n_beams, n_az);
    const int64_t n_cells = (int64_t)n_beams * n_az;
    LIDOG_REQUIRE(n_cells < (int64_t)INT32_MAX, "lidog_raycast: %lld cells out of range", (long long)n_cells);
    LIDOG_REQUIRE(az0 >= -RC_TWO_PI && az0 <= RC_TWO_PI, "lidog_raycast: az0 = %g outside [-2 pi, 2 pi]", az0);
    LIDOG_REQUIRE(m_dev, "lidog_raycast: m_dev is required");
    LIDOG_CHECK_HIP(hipMemsetAsync(m_dev, 0, sizeof(int32_t), st));
    if (n == 0) return 0;
    LIDOG_REQUIRE(points && edges && points_out && rows_out && ws,
                  "lidog_raycast: an input array, an output array or the workspace is missing");
    LIDOG_REQUIRE(!snap || (cos_el && sin_el && cos_az && sin_az), "lidog_raycast: snap without the four tables");
    LIDOG_REQUIRE(((uintptr_t)ws & 7) == 0, "lidog_raycast: the workspace must be 8-byte aligned");
    unsigned long long *table = (unsigned long long *)ws;
    int32_t *occupied = ws + 2 * n_cells, *kept = ws + 3 * n_cells, *compact_ws = ws + rc_ws_head(n_cells);
    const int32_t *count = nullptr;
    const int64_t cb = cdiv64(n_cells, RC_THREADS), pb = cdiv64(n, RC_THREADS);
    const unsigned cgrid = (unsigned)(cb < RC_MAX_BLOCKS ? cb : RC_MAX_BLOCKS);
    const unsigned pgrid = (unsigned)(pb < RC_MAX_BLOCKS ? pb : RC_MAX_BLOCKS);
    k_rc_fill<<<cgrid, RC_THREADS, 0, st>>>(table, n_cells);
    k_rc_splat<<<pgrid, RC_THREADS, 0, st>>>(points, n, origin, edges, n_beams, n_az, az0, min2, use_max, max2, cell_out,
                                             table);
    k_rc_flag<<<cgrid, RC_THREADS, 0, st>>>(table, n_cells, occupied);
    LIDOG_LAUNCH_CHECK();
    if (lidog_compact_rows(occupied, n_cells, kept, compact_ws, &count, st)) return 1;
    const int64_t most = n < n_cells ? n : n_cells;
    const int64_t eb = cdiv64(most, RC_THREADS);
    k_rc_emit<<<(unsigned)(eb < RC_MAX_BLOCKS ? eb : RC_MAX_BLOCKS), RC_THREADS, 0, st>>>(
        points, n, origin, table, kept, count, n_cells, n_az, snap, cos_el, sin_el, cos_az, sin_az, points_out,
        rows_out, m_dev);
    LIDOG_LAUNCH_CHECK();
    return 0;
}
