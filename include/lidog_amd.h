/*
 * lidog_amd.h -- C ABI of the MI355X-native sparse-voxel engine (liblidog_amd.so).
 *
 * This is the drop-in boundary for LiDOG's hot path.  The reference reaches
 * this functionality through the python package MinkowskiEngine 0.5.4 and
 * torch.nn; each entry point below cites the reference call site it replaces
 * (paths relative to the reference repository root).  INTEGRATION.md shows the
 * ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless its name ends in _host;
 *   - the caller owns all memory; the library never allocates or frees
 *     caller-visible buffers and keeps no state between calls;
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on it
 *     unless documented as synchronising;
 *   - return value 0 = success, non-zero = failure with a message in
 *     lidog_last_error() (thread-local);
 *   - coordinates are int32 rows (batch, x, y, z); features are float32
 *     row-major [rows, channels]; all index tables are int32.
 *   - coordinate components must lie in [-65536, 65535], batch in [0, 4095]
 *     (63-bit packed hash key); violations set *err_flag (device int32) to 1.
 *
 * Grammar.  lidog_amd/_lib.py derives its ctypes binding from the prototypes below and refuses what it cannot read:
 * scalars are int, int32_t, int64_t, uint32_t, float or double (returns: int, int32_t, int64_t, const char *),
 * anything else travels as a pointer; every parameter is named; no function-pointer parameters, no macros in types.
 */
#ifndef LIDOG_AMD_H
#define LIDOG_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char *lidog_last_error(void);
/* 9.  Bumped whenever an entry point changes its arguments or their meaning (additive entries leave it alone);
 * 8 -> 9: the workspaces of lidog_coords_compact / lidog_coords_stride are sized by their _ws functions. */
#define LIDOG_ABI_VERSION 9
int lidog_abi_version(void);

/* ------------------------------------------------------------------ coordinate maps
 * Replaces MinkowskiEngine's CoordinateManager (insert_and_map / stride / kernel map),
 * reached from ME.SparseTensor(...) at utils/pipelines/trainer_lighting_2d.py:151 and
 * implicitly from every ME.MinkowskiConvolution call in utils/models/minkunet_bev.py:307-371. */

/* slots needed for n rows (power of two, load factor <= 0.5) */
int64_t lidog_hash_capacity(int64_t n);

/* Build the hash table of a coordinate map: keys[cap] (uint64), vals[cap] (int32 row of the FIRST
 * occurrence of that coordinate).  first_row[i] = vals of row i's key (== i for unique input).
 * n_unique_dev receives the number of distinct coordinates (device int64).
 * Range: -65536 <= x, y, z <= 65535 and 0 <= batch <= 4095.  A row outside it sets *err_flag = 1, enters no key,
 * counts as a distinct coordinate of its own and gets first_row[i] = i; the caller reads the flag and refuses the map. */
int lidog_coords_insert(const int32_t *coords, int64_t n, uint64_t *keys, int32_t *vals, int64_t cap,
                        int32_t *first_row, int64_t *n_unique_dev, int32_t *err_flag, void *stream);
/* the same, and in the same pass what a caller needs to size occupancy bitmaps and batch loops:
 * info [9] int64 (device) = (unique rows, error flag, largest batch index, lowest x, y, z, highest x, y, z) -- one
 * read-back instead of n_unique + err + three device-wide min / max reductions of the caller's own.  The extrema are
 * taken over ALL n rows, out-of-range ones included (the caller refuses such a map anyway); for n = 0 they are the
 * placeholders -2^40 (largest batch index, highest x, y, z) and 2^40 (lowest x, y, z). */
int lidog_coords_insert_info(const int32_t *coords, int64_t n, uint64_t *keys, int32_t *vals, int64_t cap,
                             int32_t *first_row, int64_t *info, int32_t *err_flag, void *stream);

/* Compact a map with duplicates: unique_rows[j] = first-occurrence row of output row j (ascending),
 * inverse[i] = output row of input row i; rewrites vals to output rows.  scan_ws: int32[lidog_coords_compact_ws(n)]
 * (the required size: n + ceil(n / 1024) + 1 words, n < 0 counting as 0; the entry point cannot check it).
 * Terminates on any input: a row that lidog_coords_insert flagged as out of range keeps its unique_rows / inverse
 * entries (every output is defined) and rewrites no slot, and a probe ends at an empty slot.  A caller may therefore
 * launch it before it has read the range flag (lidog_amd.data.quantize_rows: one read-back after the last launch). */
int64_t lidog_coords_compact_ws(int64_t n);
int lidog_coords_compact(const int32_t *first_row, int64_t n, const uint64_t *keys, int32_t *vals, int64_t cap,
                         const int32_t *coords, int32_t *unique_rows, int32_t *inverse, int32_t *scan_ws,
                         void *stream);

/* Strided map (conv kernel 2 stride 2, minkunet_bev.py:62,69,76,83): out coordinate =
 * floor(c / new_stride) * new_stride per spatial dim, duplicates collapsed, rows in first-occurrence
 * order of the parent.  coords_out has room for n_in rows; n_out_dev (device int64) gets the count.
 * parent2child[i] = output row of parent row i.  ws: int32[lidog_coords_stride_ws(n_in)] (the required size:
 * 2 n_in + ceil(n_in / 1024) + 1 words, n_in < 0 counting as 0). */
int64_t lidog_coords_stride_ws(int64_t n_in);
int lidog_coords_stride(const int32_t *coords_in, int64_t n_in, int32_t new_stride, uint64_t *keys,
                        int32_t *vals, int64_t cap, int32_t *parent2child, int32_t *coords_out,
                        int64_t *n_out_dev, int32_t *ws, int32_t *err_flag, void *stream);

/* Occupancy bitmap of a coordinate map over its bounding box (one bit per cell, x fastest, then y, z, batch; x0 / y0 / z0
 * and every coordinate multiples of `stride`): lidog_kernel_map_bits tests the bit of a neighbour's cell before it
 * probes the hash table -- 84 % (3^3) to 90 % (5^3) of the neighbours of a LiDAR voxel do not exist, and each of those
 * probes was a random 64-byte fetch.  lidog_bitmap_words: uint32 words of the bitmap, -1 if it would exceed max_bytes
 * (the caller then passes bits = NULL: plain probes).  lidog_bitmap_set: bits zeroed by the caller; *err_flag = 2 if a
 * coordinate lies outside the box.  The neighbour table is the same with or without the bitmap. */
int64_t lidog_bitmap_words(int32_t nx, int32_t ny, int32_t nz, int32_t nb, int64_t max_bytes);
int lidog_bitmap_set(const int32_t *coords, int64_t n, int32_t x0, int32_t y0, int32_t z0, int32_t nx, int32_t ny,
                     int32_t nz, int32_t stride, int32_t nb, uint32_t *bits, int32_t *err_flag, void *stream);
int lidog_kernel_map_bits(const int32_t *coords_out, int64_t n_out, const uint64_t *in_keys, const int32_t *in_vals,
                          int64_t in_cap, const int32_t *offsets_host, int32_t K, const uint32_t *bits, int32_t x0,
                          int32_t y0, int32_t z0, int32_t nx, int32_t ny, int32_t nz, int32_t stride, int32_t nb,
                          int32_t *nbr, void *stream);
/* Neighbour table of a kernel map whose offsets are a SUBSET of another map's over the same coordinate map (same tensor
 * stride and dilation): the 3^3 map of the stride-1 BasicBlocks (minkunet_bev.py:371, block8) from the stem's 5^3 table
 * (:57, conv0p1s1).  nbr [K, n] row k = nbr_big [K_big, n] row sel_host[k]; no hash probes, same table bit for bit. */
int lidog_kernel_map_subset(const int32_t *nbr_big, int64_t n, int32_t K_big, const int32_t *sel_host, int32_t K,
                            int32_t *nbr, void *stream);

/* Kernel map, neighbour-table form, k-major: nbr[k * n_out + o] = row of the input map holding
 * coordinate out[o] + offsets[k], or -1.  offsets_host is a HOST array [K,3] (x,y,z), K <= 125. */
int lidog_kernel_map(const int32_t *coords_out, int64_t n_out, const uint64_t *in_keys, const int32_t *in_vals,
                     int64_t in_cap, const int32_t *offsets_host, int32_t K, int32_t *nbr, void *stream);

/* Rule book from the neighbour table (wavefront ballot + prefix-sum compaction): for each k the pairs
 * (pair_in, pair_out) in ascending out-row order, k_off_dev[K+1] segment offsets (device int64),
 * pos_out[k*n_out+o] = pair position or -1, pos_in[k*n_in+i] = pair position or -1 (both may be NULL when the map
 * is never walked by row: the 5^3 stem).
 * pair_* need room for n_out*K entries unless the caller knows P.  ws: int32[(blocks+1)*K + K + 2],
 * blocks = ceil(n_out / 1024). */
int lidog_kernel_map_pairs(const int32_t *nbr, int64_t n_out, int64_t n_in, int32_t K, int64_t *k_off_dev,
                           int32_t *pair_in, int32_t *pair_out, int32_t *pos_out, int32_t *pos_in, int32_t *ws,
                           void *stream);
/* Per-row lists of a rule book: row_ptr [n+1], row_list [P] = the pair positions of row o (entries of pos [K][n] that
 * are >= 0) in ascending offset order; what lidog_sconv_reduce_rows[_stats] walk.  mark_k >= 0: the entry of that
 * offset is stored as -1 (a consumer that computes that offset's product itself; unused by this library's path).  ws: ceil((n+1)/1024)+1 ints. */
int lidog_kernel_map_rows(const int32_t *pos, int64_t n, int32_t K, int32_t mark_k, int32_t *row_ptr,
                          int32_t *row_list, int32_t *ws, void *stream);

/* ------------------------------------------------------------------ sparse convolution
 * Replaces ME.MinkowskiConvolution / MinkowskiConvolutionTranspose forward and backward
 * (minkunet_bev.py:57-123 construction, :307-371 calls; kernel layout [K,Cin,Cout], :404). */

/* Gathered GEMM over the rule book: for every tile t (tile_k[t], tile_row0[t], tile_rows[t] <= 128)
 *   T[dst(p)][:] = A[gather[p]][:] . B[tile_k]      p = tile_row0 .. tile_row0 + tile_rows
 * B is [K, Cin, Cout] row-major.  dst(p) = p when scatter == NULL, else scatter[p] (each destination
 * written once).  The product of one row is an fmaf chain over ci ascending starting from 0
 * (bit-identical to oracle/me_oracle.c:orc_conv_fwd before its scatter-add).
 * bias (may be NULL) [Cout] is added after the chain.
 * a_rows: rows of A, or 0 = not known.  When non-zero it is a HARD upper bound and a precondition: every gather index
 * (every p when gather == NULL) must lie in [0, a_rows).  It chooses the kernel -- an A below 4 GiB (a_rows * Cin * 4
 * bytes) lets a workgroup walk several tiles with 32-bit byte offsets built from the gather indices -- so an understated
 * a_rows wraps those offsets and reads outside A without any diagnostic; the kernels never check an index against it.
 * Pass the exact row count, as every caller of this library does, or 0. */
int lidog_sconv_gemm(const float *A, const int32_t *gather, const float *B, const float *bias,
                     const int32_t *tile_k, const int32_t *tile_row0, const int32_t *tile_rows, int32_t n_tiles,
                     int32_t Cin, int32_t Cout, float *T, const int32_t *scatter, int64_t a_rows, void *stream);
/* The matrix-core gathered GEMM gives a workgroup several (tile, column tile) units -- the next unit's rows are fetched
 * while the current one is multiplied -- when a launch is more than one round of resident workgroups, A is below 4 GiB
 * (a_rows known) and there is neither a scatter index nor a bias; results are bit-identical either way.  multi: 1 / 0 =
 * on / off (< 0: unchanged; default on, LIDOG_GEMM_MULTI=0 in the environment turns it off); slots > 0: plan as if that
 * many workgroups were resident (0: ask the device).  Returns the previous `multi`. */
int32_t lidog_sconv_gemm_units(int32_t multi, int32_t slots);
/* T = addend + product of the same gathered GEMM, narrow inputs only (Cin <= 8, Cout % 4 == 0): the data gradient of the
 * classifier `final` (minkunet_bev.py:118-123, 7 -> 96) lands on rows that already hold the BEV head's gradient.  Same
 * bits as lidog_sconv_gemm + lidog_add(addend, product).  Returns 3 for other shapes (nothing launched). */
int lidog_sconv_gemm_addend(const float *A, const int32_t *gather, const float *B, const int32_t *tile_k,
                            const int32_t *tile_row0, const int32_t *tile_rows, int32_t n_tiles, int32_t Cin,
                            int32_t Cout, const float *addend, float *T, const int32_t *scatter, void *stream);

/* out[o][:] = sum over k ascending of T[pos[k*n + o]][:] (skipping -1), plus bias if not NULL.
 * The gather->GEMM->scatter-add order of the ME CPU algorithm, without atomics. */
int lidog_sconv_reduce(const float *T, const int32_t *pos, int64_t n, int32_t K, int32_t C, const float *bias,
                       const float *addend /* [n,C] added last (may be NULL): a second gradient of the same tensor */,
                       float *out, void *stream);

/* lidog_sconv_reduce with the BatchNorm statistics of `out` folded into the same pass: sums[0..C) = sum over
 * rows of out, sums[C..2C) = sum of squares (fp64, added in a fixed order: bit-reproducible; overwritten).
 * partial_ws: lidog_sconv_reduce_stats_ws(n, C) doubles.  C % 4 == 0. */
int64_t lidog_sconv_reduce_stats_ws(int64_t n, int32_t C);
int lidog_sconv_reduce_stats(const float *T, const int32_t *pos, int64_t n, int32_t K, int32_t C, const float *bias,
                             float *out, double *sums, double *partial_ws, double count, float eps, float momentum,
                             float *mean, float *invstd, float *running_mean, float *running_var, void *stream);
/* The same two reductions over the per-row lists of lidog_kernel_map_rows (only the offsets a voxel really has are
 * read; same additions in the same order: bit-identical results). */
int lidog_sconv_reduce_rows(const float *T, const int32_t *row_ptr, const int32_t *row_list, int64_t n, int32_t C,
                            const float *bias, const float *addend, float *out, void *stream);
int lidog_sconv_reduce_rows_stats(const float *T, const int32_t *row_ptr, const int32_t *row_list, int64_t n,
                                  int32_t C, const float *bias, float *out, double *sums, double *partial_ws,
                                  double count, float eps, float momentum, float *mean, float *invstd,
                                  float *running_mean, float *running_var, void *stream);
/* Data-gradient reduction (lidog_sconv_reduce_rows without bias) whose epilogue is lidog_bn_bwd_reduce of the layer that
 * produced the rows: `out` is the complete gradient dy of that layer's BatchNorm (+ ReLU) output
 * (ME.MinkowskiBatchNorm backward, minkunet_bev.py:60), `pre` / mean / invstd its saved input and statistics,
 * relu_y or (relu_w, relu_b) its ReLU mask as in lidog_bn_bwd_reduce.  sums / count / dw / db as there; the sums are
 * bit-identical to calling lidog_bn_bwd_reduce on `out` afterwards (same partial sums in the same order), one pass
 * over dy less.  relu_bits: the mask as written by lidog_bn_apply_bits instead of relu_y.
 * partial_ws: lidog_bn_reduce_ws(C, 1) doubles. */
int lidog_sconv_reduce_rows_bwdstats(const float *T, const int32_t *row_ptr, const int32_t *row_list, int64_t n,
                                     int32_t C, const float *addend, float *out, const float *pre,
                                     const float *relu_y, const uint32_t *relu_bits, const float *mean,
                                     const float *invstd, const float *relu_w, const float *relu_b, double *sums,
                                     double *partial_ws, double count, float *dw, float *db, void *stream);
/* Validation path (running statistics, minkunet_bev.py:376-393): the reduction with the evaluation-mode BatchNorm
 * (+ residual + ReLU) in its epilogue, same expression and order as lidog_bn_apply. */
int lidog_sconv_reduce_rows_bn(const float *T, const int32_t *row_ptr, const int32_t *row_list, int64_t n, int32_t C,
                               const float *bias, const float *mean, const float *invstd, const float *w,
                               const float *b, const float *residual, int32_t relu, float *out, void *stream);
/* count / eps / momentum / mean / invstd / running_*: as for lidog_bn_stats below (the last kernel of the
 * reduction also stores the row count behind the sums and, when mean != NULL, finalises the statistics). */

/* Cin == 1 convolution (the 5^3 stem) straight from the neighbour table nbr [K][n] of lidog_kernel_map, no product
 * rows: out[o] = sum_k x[nbr[k][o]] * W[k][:] (+ bias), bit-identical to lidog_sconv_gemm + lidog_sconv_reduce.
 * Cout in {16, 32, 64}. */
int lidog_sconv_cin1(const float *x, const int32_t *nbr, const float *W, const float *bias, int64_t n, int32_t K,
                     int32_t C, float *out, void *stream);

/* gW[k] = sum over the pairs p of offset k of A[pair_a[p]]^T . G[pair_g[p]]   ([Cin,Cout] per k).
 * The pair list is cut on the host into work items of (nearly) equal length that never straddle an offset:
 * items [3, n_items] int32 = (k, first pair, end pair), ordered by k; item_off [K+1] = first item of every k.
 * Every item writes its own partial [Cin,Cout] slot(s); the slots of one offset are then summed in order.
 * partial: lidog_sconv_wgrad_slabs(Cin, Cout, n_items) * Cin * Cout floats. */
int lidog_sconv_wgrad(const float *A, const int32_t *pair_a, const float *G, const int32_t *pair_g,
                      const int32_t *items, int32_t n_items, const int32_t *item_off, int32_t K, int32_t Cin,
                      int32_t Cout, float *partial, float *gW, void *stream);

/* slots of Cin*Cout floats that `partial` must hold for lidog_sconv_wgrad with n_items work items */
int lidog_sconv_wgrad_slabs(int32_t Cin, int32_t Cout, int32_t n_items);
/* workgroups of lidog_sconv_wgrad (fold != 0: lidog_sconv_wgrad_in_bn) for Cin x Cout that are resident on the chip at a
 * time (occupancy x CUs): the caller cuts the rule book so that a launch is a whole number of rounds (me._wgrad_items;
 * ME's own weight gradient, MinkowskiConvolution backward, has no such knob).  0: not a matrix-core shape. */
int32_t lidog_sconv_wgrad_slots(int32_t Cin, int32_t Cout, int32_t fold);

/* Arithmetic core of lidog_sconv_gemm / lidog_sconv_wgrad: 1 = exact-f32 MFMA (default), 0 = vector FMA.
 * Both produce bit-identical results (an f32 MFMA is a k-ordered fmaf chain); kept selectable for A/B. */
int lidog_set_sparse_core(int32_t core);
int lidog_get_sparse_core(void);

/* Wt[k][co][ci] = W[k][ci][co] */
int lidog_transpose_kernel(const float *W, int32_t K, int32_t Cin, int32_t Cout, float *Wt, void *stream);
/* all kernels of a model at once (after the optimiser step): desc int64 [n_mats][6] = (src offset, dst offset, K, Cin,
 * Cout, first 32x32 tile), offsets in floats into src / dst */
int lidog_transpose_batched(const float *src, float *dst, const int64_t *desc, int32_t n_mats, int64_t total_tiles,
                            void *stream);

/* ------------------------------------------------------------------ BatchNorm / ReLU on COO features
 * Replaces ME.MinkowskiBatchNorm (nn.BatchNorm1d over all rows, minkunet_bev.py:60,406-408) and
 * ME.MinkowskiReLU (:124).  layout: x[n, C] when hw == 1; NCHW with hw = H*W otherwise
 * (nn.BatchNorm2d of utils/models/conv2d.py:18,21). */

/* per-channel sums in double: sums[0..2C) = (sum x, sum x^2), overwritten.  ws: lidog_bn_reduce_ws(C, hw) doubles of
 * scratch -- for NCHW input (hw > 1) that many PER IMAGE (n x) -- holding per-workgroup partials that are added in a
 * fixed order: no atomics anywhere, every sum is run-to-run reproducible (0 = not needed, ws may be NULL).
 * count > 0: also stored at sums[2*C] (SyncBatchNorm all-reduces the row count together with the sums).
 * mean != NULL: lidog_bn_finalize(sums, count, ...) is folded into the same launch (local BatchNorm). */
int64_t lidog_bn_reduce_ws(int32_t C, int64_t hw);
int lidog_bn_stats(const float *x, int64_t n, int32_t C, int64_t hw, double *sums, double *ws, double count,
                   float eps, float momentum, float *mean, float *invstd, float *running_mean, float *running_var,
                   void *stream);
/* mean/invstd from sums and count; updates running stats (momentum, unbiased var) when not NULL.
 * count <= 0: the count is read from sums[2*C] on the device (SyncBatchNorm all-reduces it with the sums);
 * the same convention holds for lidog_bn_bwd_apply. */
int lidog_bn_finalize(const double *sums, double count, int32_t C, float eps, float momentum, float *mean,
                      float *invstd, float *running_mean, float *running_var, void *stream);
/* y = (x - mean) * invstd * w + b (+ residual) (relu).  In-place (y == x) allowed. */
int lidog_bn_apply(const float *x, int64_t n, int32_t C, int64_t hw, const float *mean, const float *invstd,
                   const float *w, const float *b, const float *residual, int32_t relu, float *y, void *stream);
/* backward reduce: sums[0..2C) = (sum dy', sum dy'*xhat) with dy' = dy * (y > 0) when relu_y != NULL; ws as above;
 * count > 0: stored at sums[2*C]; db / dw != NULL: the LOCAL parameter gradients (float copies of the two sums) */
/* relu_w / relu_b (both or neither; relu_y must then be NULL; [rows, C] with C % 4 == 0 only): the ReLU mask is
 * recomputed from x with the forward pass's own expression ((x - mean) * invstd * w + b > 0, same bits) instead of
 * being read from the saved output -- for a BatchNorm + ReLU WITHOUT residual, one tensor less to stream. */
/* upper bound of the workgroups (= rows of fp64 partial sums) of the per-row statistics reductions */
int32_t lidog_stats_max_blocks(void);
/* workgroups (= rows of partial sums) lidog_bn_bwd_reduce uses for [n, C] rows, C % 4 == 0 */
int64_t lidog_bn_bwd_reduce_blocks(int64_t n, int32_t C);
int lidog_bn_bwd_reduce(const float *dy, const float *x, const float *relu_y, int64_t n, int32_t C, int64_t hw,
                        const float *mean, const float *invstd, double *sums, double *ws, double count, float *dw,
                        float *db, const float *relu_w, const float *relu_b, void *stream);
/* dx = w*invstd*(dy' - s0/count - xhat*s1/count); dres = dy' when dres != NULL; dw = s1, db = s0 when != NULL;
 * relu_b: as above (w is the BatchNorm weight already) */
int lidog_bn_bwd_apply(const float *dy, const float *x, const float *relu_y, int64_t n, int32_t C, int64_t hw,
                       const float *mean, const float *invstd, const float *w, const double *sums, double count,
                       float *dx, float *dres, float *dw, float *db, const float *relu_b, void *stream);
/* ReLU masks as bits ([rows, C] with C % 4 == 0; MinkowskiReLU after a residual add, resnet_block.py:8-56): the apply
 * pass also writes bit 4 * (q % 8) + j of word q / 8 = (element j of float4 number q of y) > 0 into relu_bits
 * [lidog_relu_bits_words(n, C)], and the two backward passes read that instead of the saved output y (1/32 of the
 * bytes; same mask, same results).  relu_bits == NULL: exactly the functions above. */
int64_t lidog_relu_bits_words(int64_t n, int32_t C);
int lidog_bn_apply_bits(const float *x, int64_t n, int32_t C, int64_t hw, const float *mean, const float *invstd,
                        const float *w, const float *b, const float *residual, int32_t relu, float *y,
                        uint32_t *relu_bits, void *stream);
/* SyncBatchNorm forward in one launch: mean / invstd / running statistics from the ALL-REDUCED sums (the row count
 * behind them) + the apply pass; = lidog_bn_finalize(sums, -1, ...) followed by lidog_bn_apply_bits, bit for bit */
int lidog_bn_apply_sync(const float *x, int64_t n, int32_t C, const double *sums, float eps, float momentum, float *mean,
                        float *invstd, float *running_mean, float *running_var, const float *w, const float *b,
                        const float *residual, int32_t relu, float *y, uint32_t *relu_bits, void *stream);
int lidog_bn_bwd_reduce_bits(const float *dy, const float *x, const float *relu_y, const uint32_t *relu_bits, int64_t n,
                             int32_t C, int64_t hw, const float *mean, const float *invstd, double *sums, double *ws,
                             double count, float *dw, float *db, const float *relu_w, const float *relu_b,
                             void *stream);
int lidog_bn_bwd_apply_bits(const float *dy, const float *x, const float *relu_y, const uint32_t *relu_bits, int64_t n,
                            int32_t C, int64_t hw, const float *mean, const float *invstd, const float *w,
                            const double *sums, double count, float *dx, float *dres, float *dw, float *db,
                            const float *relu_b, void *stream);
/* out[c] = sum over the n rows of x[., c] for a narrow matrix (C <= 16; the classifier's bias gradient); ws: 512*C
 * doubles */
int lidog_colsum(const float *x, int64_t n, int32_t C, float *out, double *ws, void *stream);
int64_t lidog_colsum_ws(int32_t C); /* doubles of workspace lidog_colsum needs */
/* evaluation-mode BatchNorm (running statistics, minkunet_bev.py:376-393 validation path): invstd = 1/sqrt(var+eps) */
int lidog_bn_eval_invstd(const float *running_var, float eps, int32_t C, float *invstd, void *stream);
/* ME.cat(a, b) on one coordinate map (minkunet_bev.py:337,348,359,370) and its backward (two contiguous gradients) */
int lidog_cat2(const float *a, int32_t Ca, const float *b, int32_t Cb, int64_t n, float *out, void *stream);
int lidog_split2(const float *g, int32_t Ca, int32_t Cb, int64_t n, float *ga, float *gb, void *stream);
int lidog_relu_fwd(const float *x, int64_t n, float *y, void *stream);
int lidog_relu_bwd(const float *dy, const float *y, int64_t n, float *dx, void *stream);
int lidog_add(const float *a, const float *b, int64_t n, float *out, void *stream);

/* ------------------------------------------------------------------ BEV projection
 * Replaces MinkUNetBaseBEV.sparse2super (minkunet_bev.py:158-230) without materialising the
 * [H,W,C] tensor: a [B,H,W] int32 winner map (last row wins) + fused view-scramble + MaxPool2d. */
int lidog_bev_winner(const int32_t *coords, int64_t n, const int32_t *lut_x, const int32_t *lut_y, int32_t lut_lo,
                     int32_t lut_n, int32_t H, int32_t W, int32_t *winner /*[B,H,W], pre-filled -1*/,
                     int32_t *pixel /*[n] linear b*H*W+py*W+px or -1*/, void *stream);
/* winner/pixel/n: as produced by lidog_bev_winner for the same rows (only windows that contain a cell of an
 * occupied pixel are computed; the rest of out/argsrc is filled with 0 / -1).
 * rowbits (may be NULL; when given, argsrc is written for the computed windows only and NOT filled elsewhere):
 * uint64 [B*C*Ho][ceil(Wo/64)], bit x of row (b,c,yo) set for every computed window: the
 * structural support of `out` (a superset of argsrc >= 0) in the form lidog_conv2d_support keeps at the start of
 * its `act` buffer -- pass that buffer here and call lidog_conv2d_support(NULL, ...). */
int lidog_bev_pool_fwd(const float *feats, int32_t C, const int32_t *winner, const int32_t *pixel, int64_t n,
                       int32_t B, int32_t H, int32_t W, int32_t pk, int32_t ps, int32_t pp, int32_t Ho, int32_t Wo,
                       float *out /*[B,C,Ho,Wo]*/,
                       int32_t *argsrc /*[B,C,Ho,Wo] row*C+c of the arg-max cell or -1*/, uint64_t *rowbits,
                       void *stream);
/* Backward of lidog_bev_pool_fwd as a gather over (voxel row, channel), no atomics (bit-reproducible): every row that
 * targets a pixel receives the gradient of the pixel's winning row's cells (index_put's backward, minkunet_bev.py:217),
 * a cell's gradient is the sum over the windows whose arg-max it was, in ascending window order.  Only the (argsrc, gout)
 * pairs of windows that cover a cell of an occupied pixel enter the result; the kernel may LOAD a neighbouring pair of
 * the same plane (index clamped) and drop it, so both images must be allocated in full but need not be initialised there. */
int lidog_bev_pool_bwd(const float *gout /*[B,C,Ho,Wo]*/, const int32_t *argsrc, const int32_t *winner,
                       const int32_t *pixel, int64_t n, int32_t C, int32_t B, int32_t H, int32_t W, int32_t pk,
                       int32_t ps, int32_t pp, int32_t Ho, int32_t Wo, float *gfeats /*[n,C]*/, void *stream);

/* ------------------------------------------------------------------ dense 2-D BEV head (MFMA)
 * Replaces nn.Conv2d(k3,s2,p1,bias=False) x2 and nn.Conv2d(k1) of Encoder2D
 * (utils/models/conv2d.py:16-22,116,184-185).  NCHW float32, exact-f32 MFMA. */
int lidog_conv2d_fwd(const float *x, const float *w, const float *bias, int32_t B, int32_t Cin, int32_t H,
                     int32_t W, int32_t Cout, int32_t ksize, int32_t stride, int32_t pad, float *y, void *stream);
/* ws: 9*Cin*Cout floats (parity-class repacked weights) for k3 s2 p1; unused for k1 */
int lidog_conv2d_dgrad(const float *gy, const float *w, int32_t B, int32_t Cin, int32_t H, int32_t W,
                       int32_t Cout, int32_t ksize, int32_t stride, int32_t pad, float *gx, float *ws,
                       void *stream);
/* ws: split-K partial slabs, summed in order (no atomics).  k3 s2 p1: as many slabs of Cout*Cin*9 floats as fit
 * (32 are enough); k1: 4*B slabs of Cout*Cin + Cout floats. */
int lidog_conv2d_wgrad(const float *x, const float *gy, int32_t B, int32_t Cin, int32_t H, int32_t W,
                       int32_t Cout, int32_t ksize, int32_t stride, int32_t pad, float *gw, float *gbias,
                       float *ws, int64_t ws_floats, void *stream);

/* Conv2d(k3,s2,p1,bias=False) over a structurally sparse input (the image made by sparse2super: ~95 % empty cells).
 * support [B,Cin,H,W] int32: >= 0 where the cell can be non-zero / its gradient is needed (the arg-max source map
 * of lidog_bev_pool_fwd), < 0 where x is exactly 0 and its gradient is never read.
 * lidog_conv2d_support turns it into per-tile lists of active input channels (act: lidog_conv2d_support_ws int32;
 * support == NULL: the row bitmasks at the start of act were already written by lidog_bev_pool_fwd);
 * fwd_sparse = lidog_conv2d_fwd restricted to them (bit-identical result); dgrad_sparse writes gx ONLY for the
 * active channels of every 128-pixel tile (a superset of the cells with support >= 0), the rest of gx is untouched;
 * wgrad_sparse = lidog_conv2d_wgrad visiting, for every group of 3 input channels, only the pixel tiles in which
 * one of them is active (equal up to the order of the split sums).
 * ws: Cin*9*Cout floats (transposed / parity-class repacked weights); wgrad: lidog_conv2d_wgrad_sparse_ws floats
 * (one slab of Cout*Cin*9 per work item of a channel group).  Cin <= 128, Cout % 128 == 0. */
int64_t lidog_conv2d_support_ws(int32_t B, int32_t Cin, int32_t H, int32_t W);
int lidog_conv2d_support(const int32_t *support, int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t *act,
                         void *stream);
int lidog_conv2d_fwd_sparse(const float *x, const float *w, const int32_t *act, int32_t B, int32_t Cin, int32_t H,
                            int32_t W, int32_t Cout, float *y, float *ws, void *stream);
int lidog_conv2d_dgrad_sparse(const float *gy, const float *w, const int32_t *act, int32_t B, int32_t Cin, int32_t H,
                              int32_t W, int32_t Cout, float *gx, float *ws, void *stream);
/* FLOPs the three support-restricted kernels execute for the lists in `act` (out[0] forward, [1] data gradient,
 * [2] weight gradient; padded stages included): measurement only, reads the list headers back (synchronises) */
int lidog_conv2d_support_work(const int32_t *act, int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout,
                              double *out, void *stream);
int64_t lidog_conv2d_wgrad_sparse_ws(int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout); /* floats of ws */
int lidog_conv2d_wgrad_sparse(const float *x, const float *gy, const int32_t *act, int32_t B, int32_t Cin, int32_t H,
                              int32_t W, int32_t Cout, float *gw, float *ws, int64_t ws_floats, void *stream);

/* ------------------------------------------------------------------ DICE losses
 * utils/losses/losses.py:56-97 (DICELoss: soft = 0) and :100-187 (SoftDICELoss: soft = 1, label smoothing eps,
 * powerize, present-class mask), as called by trainer_lighting_2d.py:172-190.  logits [n, C] float32 (C in
 * 2..20), target [n] int64; rows with target == ignore_label are skipped when has_ignore != 0.
 * fwd: loss[0] = 1 - mean present-class DICE + offset (offset = -1 for neg_range); coef [2C] receives the
 * per-class gradient coefficients bwd needs; ws: lidog_dice_ws(C) doubles.  bwd: glogits = d loss / d logits * gout[0]. */
int64_t lidog_dice_ws(int32_t C);
int lidog_dice_fwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                   int32_t has_ignore, float eps, int32_t soft, int32_t powerize, int32_t use_tmask, float offset,
                   double *ws, float *loss, float *coef, void *stream);
int lidog_dice_bwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                   int32_t has_ignore, float eps, int32_t soft, int32_t powerize, const float *coef, const float *gout,
                   float *glogits, void *stream);
/* SoftDICELoss(is_kitti=True) (get_kitti_soft, losses.py:112-126): the label-smoothed targets, except that a row
 * labelled 1 or 6 carries (1 - eps) / 2 on classes 1 and 6 both; the present-class mask still counts the hard label.
 * Same workspace, coefficients and contract as lidog_dice_fwd / _bwd with soft = 1; C in 7..20, anything else returns 2
 * before any launch. */
int lidog_dice_kitti_fwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                         int32_t has_ignore, float eps, int32_t powerize, int32_t use_tmask, float offset, double *ws,
                         float *loss, float *coef, void *stream);
int lidog_dice_kitti_bwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                         int32_t has_ignore, float eps, int32_t powerize, const float *coef, const float *gout,
                         float *glogits, void *stream);

/* ------------------------------------------------------------------ weighted cross-entropy and focal loss
 * utils/losses/losses.py:8-25 (CELoss = nn.CrossEntropyLoss(weight, ignore_index), mean reduction) and :423-436
 * (FocalLoss: alpha (1 - exp(-ce))^gamma ce, a scalar function of that mean).  logits [n, C] float32 (C in 2..20),
 * target [n] int64, weight [C] float32 or NULL (all ones).  A row takes part when its label is not ignore_label (with
 * has_ignore != 0) and lies in [0, C); torch asserts on the device for a label outside, here such a row has zero weight
 * and a zero gradient, and weight is never read for it.
 * fwd: ce = sum w[t] (lse(x) - x[t]) / sum w[t]; loss[0] = ce (focal = 0) or the focal loss; coef[0] =
 * (d loss / d ce) / sum w[t]; ws: lidog_ce_ws(C) doubles (per-workgroup partials, added in a fixed order).
 * bwd: glogits[r][c] = gout[0] * coef[0] * w[t] * (softmax(x_r)[c] - [c == t]); +0 in the rows that take no part.
 * Both return 2 on a bad shape before any launch; bwd returns 0 for n == 0. */
int64_t lidog_ce_ws(int32_t C);
int lidog_ce_fwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                 int32_t has_ignore, const float *weight, int32_t focal, double alpha, double gamma, double *ws,
                 float *loss, float *coef, void *stream);
int lidog_ce_bwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                 int32_t has_ignore, const float *weight, const float *coef, const float *gout, float *glogits,
                 void *stream);

/* ------------------------------------------------------------------ Lovasz-softmax, the auxiliary point criterion
 * Berman et al., CVPR 2018 (lovasz_softmax_flat, classes='present'); not in the reference.  logits [n, C] float32 (C in
 * 2..20, n C < 2^31), target [n] int64.  A row is valid when its label is not ignore_label (with has_ignore != 0) and
 * lies in [0, C), the rule of lidog_ce_fwd; m = the valid rows, p = the fp32 row softmax.  For a class c that a valid
 * row carries (P of them):  fg_i = [t_i == c], e_i = |fg_i - p_ic|; the valid rows by descending e as float32 values,
 * ties by ascending row; G = sum fg, cf_j = the fg among the first j (integers); J(0, .) = 0,
 * J(j, cf) = 1.0 - (double)(G - cf) / (double)(G + j - cf); g_j = J(j, cf_j) - J(j - 1, cf_j - fg_j);
 * loss_c = sum_j e_j g_j in float64.  loss = sum_c loss_c / P, 0 when P = 0.
 * fwd: loss [1]; coef [n C + 1] float32: coef[i C + c] = g sign(p_ic - fg_i) with sign(0) = 0, +0 for the invalid rows
 * and the absent classes, every entry written once (no memset needed), and coef[n C] = 1 / P (0 when P = 0).  err_out:
 * NULL, or [C, n] float32 that receives the errors e as sorted on, 0 for the invalid rows.  ws: lidog_lovasz_ws(n, C)
 * BYTES (0 for a shape fwd refuses).  One stable radix sort of the C n pairs and one stable pass on the class; the
 * number of launches does not depend on n, nothing is read back to the host, no floating-point atomics: the same bytes on
 * every run.
 * bwd: g is a constant (as in the published code): glogits_i = gout[0] p_i (q_i - <q_i, p_i>) with q = coef invP[0];
 * +0 in the invalid rows.  invP: the tail word of coef, or any device float.
 * Both return 2 before any launch for another C or n C >= 2^31; n == 0: loss 0, coef[0] = 0, return 0. */
int64_t lidog_lovasz_ws(int64_t n, int32_t C);
int lidog_lovasz_fwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                     int32_t has_ignore, void *ws, float *loss, float *coef, float *err_out, void *stream);
int lidog_lovasz_bwd(const float *logits, const int64_t *target, int64_t n, int32_t C, int64_t ignore_label,
                     int32_t has_ignore, const float *coef, const float *invP, const float *gout, float *glogits,
                     void *stream);

/* ------------------------------------------------------------------ entropy, the criterion of test-time adaptation
 * csrc/entropy.hip; TENT (Wang et al., ICLR 2021) minimises it on unlabelled target batches (lidog_amd.adapt); not in the
 * reference.  logits [n, C] float32 (C in 2..20); mask [n] uint8 or NULL; row_h [n] float32.  Per row r:
 *   m = max_c x_c,  s = sum_c exp(x_c - m),  lse = m + log s,  p_c = exp(x_c - lse),  H = lse - sum_c p_c x_c
 * and row_h[r] = (float)H is written for EVERY row, whether the row takes part or not.  The kernels evaluate this in
 * double on the shifted logits x_c - m (lse - x_c = log s - (x_c - m), H = log s - sum_c p_c (x_c - m)), so a value is
 * rounded to float once, at its store.  A row takes part when both hold:
 *   mask == NULL || mask[r] != 0,    margin <= 0 || row_h[r] < margin   (compared as float32)
 * the second being the reliable-sample filter of EATA / SAR, whose usual margin is 0.4 ln C.
 * fwd, with k the number of rows that take part: loss[0] = sum over them of H / k, summed in double (0 when k == 0);
 * coef[0] = (float)(1.0 / k) (0 when k == 0); coef[1] = (float)k.  ws: lidog_entropy_ws(C) doubles (per-workgroup
 * partials, added in a fixed order).
 * bwd decides participation again from mask, row_h and margin (it never recomputes H for that decision):
 *   glogits[r][j] = gout[0] * coef[0] * p_j * ((lse - x_j) - H)  in the rows that take part, +0 in every other row;
 * every entry is written exactly once.  A row with one logit far above the rest (1e4, say) has H == 0 and a zero gradient
 * row: no NaN, no infinity.  No floating-point atomics, nothing read back: the same call gives the same bytes every time.
 * Both return 2 for another C before any launch; n == 0: fwd gives loss 0 and coef (0, 0), bwd launches nothing, both
 * return 0. */
int64_t lidog_entropy_ws(int32_t C);
int lidog_entropy_fwd(const float *logits, const uint8_t *mask, int64_t n, int32_t C, float margin, double *ws,
                      float *loss, float *coef, float *row_h, void *stream);
int lidog_entropy_bwd(const float *logits, const uint8_t *mask, const float *row_h, int64_t n, int32_t C, float margin,
                      const float *coef, const float *gout, float *glogits, void *stream);

/* ------------------------------------------------------------------ calibration of the row softmax
 * csrc/calib.hip (lidog_amd.calibration; eval_target --calibration); not in the reference, whose metrics are IoU only.
 * logits [n, C] float32, C in 2..32; labels [n] int64.  A row is LABELLED iff 0 <= label < C and label != ignore_label
 * (lidog_eval_confusion's rule); every other row is not read and adds nothing.  beta: a DEVICE double, the inverse
 * temperature 1 / T > 0, or NULL for 1.0 (a device 1.0 gives the same bytes as NULL).  Per labelled row, in double:
 *   m = max_c x_c,  z_c = beta ((double)x_c - (double)m),  s = sum_c exp(z_c) in class order,  p_c = exp(z_c) / s,
 *   pred = the first maximal class (so lidog_eval_confusion's, for any beta > 0),  conf = 1 / s,
 *   nll = log s - z_label,  brier = sum_c (p_c - [c == label])^2 in class order,
 *   bin = min(B - 1, (int)floor(conf B))                       B = n_bins in 1..64, equal-width bins of [0, 1]
 * lidog_calib_stats ADDS a batch into accumulators the caller keeps (and zeroes before the first call):
 *   table [B, 3] int64: (count, correct = rows with pred == label, conf_q += llrint(conf 2^32)) per bin
 *   totals [2] int64:   (rows, brier_q += llrint(brier 2^32))
 *   nll_sum [1] double
 * The bounded quantities are fixed-point integers on purpose: integer addition is associative, so table and totals do
 * not depend on the order of rows, the grid or the cut of a dataset into calls (one call over n rows and calls over its
 * slices give the same bytes).  They hold 2^30 rows.  nll_sum is unbounded and stays a double: per-workgroup partial
 * sums in ws (compensated: every addition keeps its rounding error, Knuth's two-sum, so a batch's sum is the rounded
 * sum of its rows whatever their spread), added in a fixed order by the last workgroup to arrive (an integer ticket),
 * then added to nll_sum once;
 * the same sequence of calls gives the same bytes, another cut into calls another rounding.  No floating-point atomic.
 * A labelled row with a NaN or infinite logit (or whose conf is no positive number: a beta that is not positive and
 * finite) is left out of everything and sets bit 1 (value 2) of *err (device int32, the caller zeroes it).
 * ws: lidog_calib_ws(n) doubles, 8-byte aligned; ws[0] is the ticket and must be 8 zero bytes before the FIRST call that
 * uses this workspace; every call leaves it zero.  One workspace serves one stream at a time.
 * n == 0 launches nothing and returns 0; C outside 2..32, n_bins outside 1..64 or n C >= 2^31 return 2 before any launch.
 *
 * Temperature scaling minimises NLL(beta) = (1 / N) sum_rows [log sum_c exp(beta x_c) - beta x_label] over the N labelled
 * rows (finite logits) of a calibration set: convex in beta, gradient g = (1 / N) sum (E_p[x] - x_label), curvature
 * h = (1 / N) sum Var_p[x] >= 0, so g is non-decreasing.  state [8] double (device), trace [3] double (device):
 *   state = (beta, lo, hi, last nll, last g, last h, iterations done, labelled rows of the last launch)
 * lidog_calib_fit_init: state = (min(max(1, beta_min), beta_max), beta_min, beta_max, 0, 0, 0, 0, 0).
 * lidog_calib_fit_step, ONE launch: reads beta = state[0]; sums over the rows, in double on z_c = x_c - m (the shift
 * cancels in g and h), e_c = exp(beta z_c), s = sum e_c, E = (sum e_c z_c) / s:
 *   L += log s - beta z_label,   G += E - z_label,   H += (sum_c e_c (z_c - E)^2) / s,   N += 1
 * (fixed-order partials, as nll_sum); then its last workgroup writes trace = (beta, L / N, G / N) and updates
 *   g > 0: hi = beta;  g < 0: lo = beta;  g == 0: lo = hi = beta
 *   cand = beta - g / h  (h > 0; else -inf, +inf or beta by the sign of g)
 *   next = beta                      if cand == beta (the step is below beta's spacing: converged)
 *        = cand                      else if lo < cand < hi (false for a NaN)
 *        = beta_max                  else if g < 0, cand >= hi, hi == beta_max and beta != beta_max
 *        = beta_min                  else if g > 0, cand <= lo, lo == beta_min and beta != beta_min
 *        = lo + (hi - lo) / 2        else
 *   next = min(max(next, beta_min), beta_max)
 * The first line keeps a converged iterate: beta is then an end of the bracket, the step is not strictly inside, and the
 * midpoint would throw the iterate away and bisect back from the far end.  The two bound lines look at the interval's own
 * bound once the step leaves through it, so a set on which g has one sign over [beta_min, beta_max] ends AT that bound
 * (lo == hi == the bound) instead of halving towards it for ever.
 * N == 0 (no labelled row, or n == 0: the launch still happens): beta, lo, hi stay, nll = g = h = 0.  No NaN either way.
 * `iters` launches are queued back to back; nothing is read back in between.  err, ws: as lidog_calib_stats.
 * Returns 2 before any launch for another C, n C >= 2^31 or bounds that are not 0 < beta_min <= beta_max < inf. */
#define LIDOG_CALIB_STATE 8
#define LIDOG_CALIB_BETA 0
#define LIDOG_CALIB_LO 1
#define LIDOG_CALIB_HI 2
#define LIDOG_CALIB_NLL 3
#define LIDOG_CALIB_G 4
#define LIDOG_CALIB_H 5
#define LIDOG_CALIB_ITER 6
#define LIDOG_CALIB_ROWS 7
int64_t lidog_calib_ws(int64_t n);
int lidog_calib_stats(const float *logits, const int64_t *labels, int64_t n, int32_t C, int64_t ignore_label,
                      const double *beta, int32_t n_bins, int64_t *table, int64_t *totals, double *nll_sum, int32_t *err,
                      double *ws, void *stream);
int lidog_calib_fit_init(double *state, double beta_min, double beta_max, void *stream);
int lidog_calib_fit_step(const float *logits, const int64_t *labels, int64_t n, int32_t C, int64_t ignore_label,
                         double beta_min, double beta_max, double *state, double *trace, int32_t *err, double *ws,
                         void *stream);

/* ------------------------------------------------------------------ data path next to the hot path
 * ME.utils.sparse_quantize (utils/datasets/semantickitti_bev.py:232-238) = lidog_voxel_floor +
 * lidog_coords_insert + lidog_coords_compact + lidog_label_vote; PC2ImgConverter.getBEVImageNew
 * (utils/datasets/semantickitti_bev.py:433-464) = lidog_bev_label_raster. */
/* rows[i] = (batch, floor(x/qx), floor(y/qy), floor(z/qz)) in float32 arithmetic (a true division, as numpy's on a
 * float32 array); points [n,3].  A quotient that is NaN, infinite or beyond int32 gives INT32_MIN, which
 * lidog_coords_insert flags as out of range: such a point is refused, never put into voxel 0.  lidog_augment_points
 * and lidog_mix_gather_aug write their voxel rows by the same rule. */
int lidog_voxel_floor(const float *points, int64_t n, float qx, float qy, float qz, int32_t batch, int32_t *rows,
                      void *stream);
/* voxel_labels[j] = label of the voxel's first point, or ignore_label when its points disagree */
int lidog_label_vote(const int32_t *labels, const int32_t *unique_rows, const int32_t *inverse, int64_t n, int64_t m,
                     int32_t ignore_label, int32_t *voxel_labels, void *stream);
/* point_idx [B,S,S] (pre-filled with -1) = index inside its scan of the last labelled in-bounds voxel per pixel,
 * img_labels [B,S,S] int64 = its label or -1.  lut_x/lut_y: pixel per integer coordinate or -1, lut_z: 1 inside
 * the z range.  batch_start [B+1]: first row of every scan. */
int lidog_bev_label_raster(const int32_t *coords, const int32_t *labels, int64_t n, const int32_t *lut_x,
                           const int32_t *lut_y, const int32_t *lut_z, int32_t lut_lo, int32_t lut_n, int32_t B,
                           int32_t S, const int64_t *batch_start, int32_t *point_idx, int64_t *img_labels,
                           void *stream);

/* ------------------------------------------------------------------ optimiser
 * Replaces torch.optim.Adam(lr, weight_decay) of trainer_lighting_2d.py:356-358 on a flat buffer. */
int lidog_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                    float beta1, float beta2, float eps, float weight_decay, int32_t step, float grad_scale,
                    void *stream);
/* torch.optim.SGD(lr, momentum=0.98, weight_decay, nesterov=True) of trainer_lighting_2d.py:351-355 (and
 * trainer_lighting.py:337-341) on a slice of the flat buffers; momentum_buf starts at zero. */
/* dst[i] = dst[i] + src[i] (plain fp32 adds) over n_segs segments; segs [n_segs][3] HOST int64: dst, src (device
 * addresses), element count.  Up to 8 segments per launch; float4 where dst and src share their alignment mod 16, scalar
 * elsewhere.  The trunk executor's accumulate mode (convolution table column 19) adds its second pass's parameter
 * gradients into the optimiser's flat buffer with it. */
int lidog_grad_accumulate(const int64_t *segs, int32_t n_segs, void *stream);
int lidog_sgd_step(float *param, const float *grad, float *momentum_buf, int64_t n, float lr, float momentum,
                   float weight_decay, int32_t nesterov, float grad_scale, void *stream);

/* ------------------------------------------------------------------ weight averaging (csrc/wavg.hip)
 * The average of a model's weights along the training trajectory, lidog_amd.optim.WeightAverage: the exponential moving
 * average of the reference's MomentumUpdater (utils/common/momentum.py: mp = tau * mp + (1 - tau) * op; no trainer of the
 * reference uses it) and the uniform average of torch.optim.swa_utils.AveragedModel.  With p the live element and a the
 * average, every operation rounded separately and the division IEEE-correct: */
#define LIDOG_WAVG_COPY 0 /* a = p */
#define LIDOG_WAVG_EMA 1  /* a = c0 * a + c1 * p        (c0 = tau, c1 = 1 - tau) */
#define LIDOG_WAVG_SWA 2  /* a = a + (p - a) / c0       (c0 = updates so far + 1) */
#define LIDOG_WAVG_SWAP 3 /* exchange a and p */
/* ONE launch of n_blocks workgroups over n_segs segments.  table: DEVICE int64 [3 n_segs + n_segs + 1]: the (live address,
 * average address, element count) triples of lidog_grad_accumulate, then block0 [n_segs + 1]: the first workgroup of every
 * segment, non-decreasing from block0[0] = 0 to block0[n_segs] = n_blocks (a segment with elements needs at least one
 * workgroup; one without may have none).  The two ranges of a segment must not overlap, nor may those of different
 * segments; the entry point cannot read the table, so whoever builds it checks it (lidog_amd.optim.wavg_table).  float4
 * where a segment's two addresses share their alignment mod 16, scalar elsewhere.  No atomics, nothing is read back.
 * n_segs == 0 or n_blocks == 0: nothing is launched.  c0, c1: unused by COPY and SWAP; c1 unused by SWA. */
int lidog_wavg_apply(const int64_t *table, int32_t n_segs, int64_t n_blocks, int32_t mode, float c0, float c1,
                     void *stream);

/* ------------------------------------------------------------------ gradient norm, clipping, SAM (csrc/sam.hip)
 * The global gradient norm over the optimiser's flat gradient buffer and its two users, lidog_amd.optim: torch's
 * clip_grad_norm_ (Lightning's gradient_clip_val) and the ascent step of sharpness-aware minimisation (SAM, Foret et al.,
 * ICLR 2021; adaptive: ASAM, Kwon et al., ICML 2021, in its common form e = rho w^2 g / || |w| g ||).  Nothing in the
 * reference uses either.  The norm stays a double in DEVICE memory: the two users read it there, nothing is read back.
 * Every fp32 operation below is rounded on its own (no contraction into a fused multiply-add), sqrt and the divisions in
 * double are the IEEE operations, so a numpy restatement gives the same bits (tests/sam_ref.py).  Every kernel walks at
 * most LIDOG_FLAT_MAX_BLOCKS workgroups of 256 threads, one float4 per thread and sweep, grid-strided beyond: float4
 * where the buffers of a call share their alignment mod 16 (a scalar head up to the first 16-byte boundary, a scalar
 * tail), scalar elsewhere.  No atomics, no state kept between launches. */
#define LIDOG_FLAT_MAX_BLOCKS 2048
#define LIDOG_SQNORM_PLAIN 0    /* t = g */
#define LIDOG_SQNORM_ADAPTIVE 1 /* t = |w| * g, rounded to fp32 */
/* out[0] = sum over i < n of (double)t_i * (double)t_i (the product of two fp32 values is exact in fp64), summed in
 * fp64 in a FIXED order: a thread sums its elements in index order into four lanes that are added pairwise, a workgroup
 * adds its threads in a fixed tree and stores one partial sum into `ws`; a second launch of one workgroup adds the
 * partial sums in the same way and stores out[0].  The same call gives the same bytes every time; the order (not the
 * value beyond n 2^-53 relative) depends on n and on the alignment of g.  w: NULL in plain mode.  n == 0: out[0] = 0.
 * ws: lidog_flat_sqnorm_ws(n) bytes of device memory, 8-byte aligned, written before it is read. */
int64_t lidog_flat_sqnorm_ws(int64_t n);
int lidog_flat_sqnorm(const float *g, const float *w, int64_t n, int32_t mode, void *ws, double *out, void *stream);
/* SAM's ascent step in one launch: backup[i] = w[i], then w[i] = w[i] + e[i] with
 *   coef = (float)((double)rho / (sqrt(*sqnorm) + 1e-12))           (every thread computes it from the device word)
 *   plain:    e = coef * g            adaptive:    e = ((w * w) * g) * coef
 * An element whose gradient is +-0 (a parameter that received none: FlatParams.zero_grad clears the buffer) is not
 * added to: w[i] keeps its bits, a -0.0 included, whatever coef is.  Restoring is a copy of backup into w (hipMemcpyAsync, or lidog_wavg_apply's COPY), never w - e.  The three
 * ranges must not overlap. */
int lidog_sam_perturb(float *w, const float *g, float *backup, int64_t n, const double *sqnorm, float rho,
                      int32_t adaptive, void *stream);
/* torch.nn.utils.clip_grad_norm_(max_norm, norm_type=2) on the flat gradient: norm = grad_scale * sqrt(*sqnorm) in
 * double (grad_scale: the 1 / world the optimiser kernels fold into the gradient; 1 on one rank),
 *   coef = min(1.0f, (float)((double)max_norm / (norm + 1e-6))),    g[i] = g[i] * coef for every i
 * so coef = 1 leaves every byte (x * 1.0f is x). */
int lidog_flat_clip(float *g, int64_t n, const double *sqnorm, float max_norm, float grad_scale, void *stream);

/* ------------------------------------------------------------------ collectives (RCCL over xGMI)
 * The two collectives of the data-parallel path for hosts that do not go through torch.distributed: the gradient
 * all-reduce of Lightning DDP (train_lidog.py:227-231, strategy='ddp'; sum, the caller folds 1/world into the
 * optimiser step) and the SyncBatchNorm statistics all-reduce (ME.MinkowskiSyncBatchNorm, train_lidog.py:228; the
 * (sum, sum, rows) vectors of lidog_bn_stats / lidog_bn_bwd_reduce are fp64).  librccl is loaded at first use.
 * One process per GPU: rank 0 calls lidog_comm_unique_id and ships the bytes to the others (any host channel),
 * every rank calls lidog_comm_init_rank with its device current.  In place, asynchronous on `stream`. */
int32_t lidog_comm_unique_id_bytes(void);
int lidog_comm_unique_id(void *id_out);
int lidog_comm_init_rank(const void *id, int32_t nranks, int32_t rank, void **comm_out);
int lidog_comm_destroy(void *comm);
int32_t lidog_comm_count(void *comm);   /* ranks of the communicator as RCCL reports them (ncclCommCount); -1 on error */
int lidog_allreduce_f32(float *buf, int64_t n, void *comm, void *stream);
int lidog_allreduce_f64(double *buf, int64_t n, void *comm, void *stream);

/* One-shot peer all-reduce for the small SyncBatchNorm statistics messages (241 messages of
 * <= 4 KB per step, all on the dependent chain): every rank pushes its vector into a mailbox in every peer's memory
 * over its direct xGMI link, waits for the N senders of its own mailbox and adds them in rank order (same bits on
 * every rank) -- one single-workgroup launch on the caller's stream instead of a ring / tree collective.
 * Set-up: every rank allocates a mailbox (lidog_peer_mailbox_alloc: fine-grained device memory + its hipIpc handle of
 * lidog_peer_handle_bytes() bytes), the handles travel through whatever the host has (torch.distributed here), every
 * rank opens the others' (lidog_peer_mailbox_open) and builds the communicator.  Waits are bounded: lidog_peer_status
 * != 0 means a sender's flag never arrived (the caller falls back to lidog_allreduce_f64). */
int32_t lidog_peer_handle_bytes(void);
int64_t lidog_peer_mailbox_bytes(int32_t nranks, int32_t max_doubles);
int lidog_peer_mailbox_alloc(int64_t bytes, void **ptr_out, void *handle_out);
int lidog_peer_mailbox_open(const void *handle, void **ptr_out);
int lidog_peer_comm_create(int32_t rank, int32_t nranks, int32_t max_doubles, void *local, void *const *peer_ptrs,
                           void **comm_out);
int32_t lidog_peer_max_doubles(void *comm);
int lidog_peer_set_spin_limit(void *comm, int64_t polls /* ~1-2 us each; 0 = default, several minutes */);
int lidog_peer_allreduce_f64(void *comm, double *buf, int64_t n, void *stream);
int32_t lidog_peer_status(void *comm);   /* 0 ok, 1 a sender's flag never arrived, 2 a sender was ahead (desynchronised) */
/* Frees the local mailbox and (close_peers != 0) unmaps the peers'.  PRECONDITION the library cannot check: every rank
 * has synchronised its stream and ALL ranks have passed a barrier after their last call -- a peer may otherwise still
 * store into (or poll) this rank's mailbox through its hipIpc mapping when the memory goes away. */
int lidog_peer_comm_destroy(void *comm, int32_t close_peers);
/* A communicator's calls must all be queued on one stream (the mailbox slots are reused in stream order): the first
 * call binds it, a call on another stream is refused; lidog_peer_rebind_stream waits for the old stream and moves it. */
int lidog_peer_rebind_stream(void *comm, void *stream);
int64_t lidog_peer_calls(void *comm);    /* calls made so far (= the sequence number of the last one) */
/* test hook of the failure path: the call with this (1-based) sequence number raises no flags on this rank, so every
 * rank's wait for it runs into the limit, sets the error word and -- from then on -- waits for nothing */
int lidog_peer_inject_skip_flag(void *comm, int64_t seq);
/* frees a mailbox that never became part of a communicator (set-up failed half way) */
int lidog_peer_mailbox_free(void *ptr);
int lidog_peer_mailbox_close(void *peer_ptr);

/* ------------------------------------------------------------------ output-stationary 3^3 convolution (csrc/sconv_os.hip)
 * MinkowskiConvolution(kernel_size=3, stride=1) without product rows: a workgroup owns 128 output rows, walks the
 * kernel offsets in ascending order and adds each offset's product -- the same fmaf chain from zero as a row of
 * lidog_sconv_gemm's T -- to the rows' running sum in the order lidog_sconv_reduce_rows adds them: identical results,
 * no 4 P Cout bytes written and read back (utils/models/minkunet_bev.py:425-439, resnet_block.py:8-56).
 * lidog_kernel_map_sorted: rows sorted by their neighbour mask (rarest offset = most significant bit) so that the rows
 * of a tile share their offsets; perm [pad128(n)] (-1 behind the last row), wave_masks [pad128(n) / 32]: OR of the
 * masks of every 32 sorted rows; tile_order [pad128(n) / 128]: the 128-row tiles in launch order (most work first).
 * nbr / k_off: lidog_kernel_map(_bits) / lidog_kernel_map_pairs of the same map.
 * lidog_sconv_os: out [n, Cout] = sum_k A[nbr[k][row]] W[k] (+ bias) (+ addend); reverse != 0 = the data gradient over
 * the (symmetric) map: offsets from the top, weights W[K-1-k] (pass the transposed kernels, Cin / Cout swapped). */
int64_t lidog_kernel_map_sorted_ws(int64_t n);
int lidog_kernel_map_sorted(const int32_t *nbr, int64_t n, int32_t K, const int64_t *k_off, int32_t *perm,
                            uint32_t *wave_masks, int32_t *tile_order, void *ws, int64_t ws_bytes, void *stream);
int lidog_sconv_os(const float *A, const int32_t *nbr, int64_t n, int32_t K, const int32_t *perm,
                   const uint32_t *wave_masks, const int32_t *tile_order, const float *W, int32_t reverse,
                   const float *bias, const float *addend, int32_t Cin, int32_t Cout, float *out, void *stream);
/* lidog_sconv_os_stats: the forward form with the BatchNorm statistics of its result in the epilogue (one partial row
 * per tile, finished in-kernel; arguments as lidog_sconv_reduce_rows_stats).  ws: lidog_sconv_os_stats_ws(n, Cout) doubles. */
int64_t lidog_sconv_os_stats_ws(int64_t n, int32_t C);
/* lidog_sconv_os_bn: the forward form with an evaluation-mode BatchNorm (+ residual + ReLU) in the epilogue -- the
 * validation path (arguments as lidog_sconv_reduce_rows_bn) */
int lidog_sconv_os_bn(const float *A, const int32_t *nbr, int64_t n, int32_t K, const int32_t *perm,
                      const uint32_t *wave_masks, const int32_t *tile_order, const float *W, const float *bias, int32_t Cin,
                      int32_t Cout, const float *mean, const float *invstd, const float *w, const float *b,
                      const float *residual, int32_t relu, float *out, void *stream);
int lidog_sconv_os_stats(const float *A, const int32_t *nbr, int64_t n, int32_t K, const int32_t *perm,
                         const uint32_t *wave_masks, const int32_t *tile_order, const float *W, const float *bias,
                         int32_t Cin, int32_t Cout, float *out, double *sums, double *ws, double count, float eps,
                         float momentum, float *mean, float *invstd, float *running_mean, float *running_var,
                         void *stream);

/* ------------------------------------------------------------------ BatchNorm + ReLU applied in the consumer's staging
 * conv1 -> BatchNorm -> ReLU -> conv2 inside a BasicBlock (ME modules/resnet_block.py as called from
 * utils/models/minkunet_bev.py:312-371): conv2 is the only reader of the normalised rows, so they need not exist in
 * memory.  The three forms below take the RAW output of conv1 as A plus conv1's BatchNorm vectors in_* [Cin] (batch mean,
 * 1/sqrt(var + eps), weight, bias) and apply ((x - mean) * invstd) * w + b (and max(., 0) when in_relu) to every
 * gathered row on its way into LDS -- lidog_bn_apply_bits' expression and operation order, so each form equals
 * lidog_bn_apply_bits followed by the plain entry point bit for bit.  Matrix-core kernels only (channel counts multiples
 * of 32, lidog_set_sparse_core(1)).  Other arguments as lidog_sconv_gemm / lidog_sconv_os_stats / lidog_sconv_wgrad. */
int lidog_sconv_gemm_in_bn(const float *A, const int32_t *gather, const float *B, const float *bias,
                           const int32_t *tile_k, const int32_t *tile_row0, const int32_t *tile_rows, int32_t n_tiles,
                           int32_t Cin, int32_t Cout, float *T, const int32_t *scatter, const float *in_mean,
                           const float *in_invstd, const float *in_w, const float *in_b, int32_t in_relu, int64_t a_rows,
                           void *stream);
int lidog_sconv_os_stats_in_bn(const float *A, const int32_t *nbr, int64_t n, int32_t K, const int32_t *perm,
                               const uint32_t *wave_masks, const int32_t *tile_order, const float *W, const float *bias,
                               int32_t Cin, int32_t Cout, float *out, double *sums, double *ws, double count, float eps,
                               float momentum, float *mean, float *invstd, float *running_mean, float *running_var,
                               const float *in_mean, const float *in_invstd, const float *in_w, const float *in_b,
                               int32_t in_relu, void *stream);
int lidog_sconv_wgrad_in_bn(const float *A, const int32_t *pair_a, const float *G, const int32_t *pair_g,
                            const int32_t *items, int32_t n_items, const int32_t *item_off, int32_t K, int32_t Cin,
                            int32_t Cout, float *partial, float *gW, const float *in_mean, const float *in_invstd,
                            const float *in_w, const float *in_b, int32_t in_relu, void *stream);

/* ------------------------------------------------------------------ host-side tables of a kernel map (csrc/hostprep.hip)
 * Pure host code.  k_off_host [K+1]: the rule book's offsets (lidog_kernel_map_pairs' k_off copied to the host).
 * lidog_tiles_host: the (tile_k, tile_row0, tile_rows) descriptors lidog_sconv_gemm takes, `tile_rows` (128) pairs per
 * tile, never straddling an offset, in launch order; skip_k >= 0 leaves that offset out.  Written as a contiguous
 * [3][n_tiles] int32 array at `out` (capacity `cap` tiles); returns n_tiles or -1.
 * lidog_wgrad_items_host: the work items lidog_sconv_wgrad takes ([4][n]: k, first pair, end pair, launch order;
 * item_off [K+1]); order_mode 0 = by offset, 1 = same relative position together, 2 = 1 in XCD-sized groups of
 * `group`.  Returns n or -1. */
int64_t lidog_tiles_host(const int64_t *k_off_host, int32_t K, int32_t skip_k, int32_t tile_rows, int32_t *out,
                         int64_t cap);
int64_t lidog_wgrad_items_host(const int64_t *k_off_host, int32_t K, int64_t chunk, int32_t order_mode, int32_t group,
                               int32_t *items, int32_t *item_off, int64_t cap);

/* ------------------------------------------------------------------ trunk executor (csrc/trunk.hip)
 * The whole MinkUNet encoder-decoder -- stem, 4 x (strided convolution + BasicBlocks), 4 x (transposed convolution +
 * ME.cat + BasicBlocks), classifier: utils/models/minkunet_bev.py:302-374, utils/models/minkunet.py:97-158 -- forward
 * and backward in ONE call each.  The reference's forward is ~190 python-level ME calls per pass; the operator path of
 * this library (one entry point per operator) costs ~12 ms of host dispatch per training step.  Here the launch
 * sequence comes from tables: the same entry points above are called in the same order with the same arguments, so
 * results are bit-identical to calling them one by one.
 *
 * Tables (int64 rows, host memory; pointers are device pointers stored as integers):
 *   convs [n_convs][20]: kind (0 = 3^3 stride 1, 1 = 2^3 stride 2, 2 = transposed 2^3 stride 2, 3 = 1x1, 4 = C_in 1
 *         stem through the neighbour table), map row, C_in, C_out, K, W [K,C_in,C_out], Wt [K,C_out,C_in] or 0
 *         (transposed here), gW, bias or 0, g_bias or 0, BatchNorm weight, bias, running_mean, running_var, g_weight,
 *         g_bias (0 for a convolution without BatchNorm), weight-gradient work items, their count, item_off
 *         (lidog_sconv_wgrad), accumulate (0: the parameter gradients are WRITTEN to gW / g_bias / g_weight / g_bias;
 *         1: they are computed into garena and ADDED to those slices by lidog_grad_accumulate -- the kernel gradient on
 *         the stream of its weight-gradient kernel, the others on `stream` -- before the convolution's parameters are
 *         counted down; backward only);   conv_f [n_convs][2]: BatchNorm eps, momentum
 *   maps  [n_maps][16]: K, n_in, n_out, pairs, pair_in, pair_out, row_ptr / row_list of the output rows, of the input
 *         rows (lidog_kernel_map_rows; 0 where unused), tile descriptors [3][n_tiles], n_tiles, neighbour table
 *         (stem) or 0, identity rows 0..n-1 (1x1) or 0
 *   ops   [n_ops][8]: type (0 = convolution + BatchNorm, 1 = concatenation, 2 = convolution), convolution row, input
 *         buffer, output buffer, ReLU, residual buffer or -1, fold (the gradient already accumulated for the input
 *         buffer -- the residual branch of a BasicBlock -- enters the data gradient's reduction as its addend), second
 *         input of a concatenation
 *   bufs  [n_bufs][4]: level (index into level_rows), channels, external slot or -1 (lives in the arena)
 *   ext / ext_grad [slots]: the caller's tensors: slot 0 = input features (no gradient), the others outputs; incoming
 *         gradients (0 = none)
 * Memory: see the notes on arena / garena / scratch / lane_scratch in csrc/trunk.hip.  dry != 0: nothing is launched,
 * need[] receives the bytes of each region for this batch.  rec [n_ops * 4 + n_bufs]: written by forward, read by
 * backward (arena offsets).  Training-mode BatchNorm.
 *
 * Data parallelism (train_lidog.py:227-231: Lightning DDP + MinkowskiSyncBatchNorm.convert_sync_batchnorm) --
 * dp [12] int64, NULL = single process:
 *   [0] SyncBatchNorm on: every BatchNorm's (sum, sum, rows) message is summed over the ranks between the kernel that
 *       produces it and the kernel that consumes it (forward: statistics -> finalise + apply, one message for conv1 +
 *       downsample of a block; backward: reduce -> apply), IN ORDER ON `stream`
 *   [1] communicator for those messages (lidog_comm_init_rank) or 0
 *   [2] host callback `int cb(int32_t what, int64_t a, int64_t b)` or 0, used where a communicator is 0:
 *       what 0 = all-reduce (sum) of b doubles at device address a, ordered on `stream`; what 1 = gradient bucket a
 *       has all its gradients queued (the callee reduces it)
 *   [3] communicator of the gradient buckets, [4] its hipStream_t, [5] base of the flat fp32 gradient buffer
 *   [6] number of buckets (0 = none), [7] int64 [n][2] element ranges (lo, hi) of the buckets in that buffer,
 *   [8] int32 [n] HOST countdown per bucket (gradients still missing; shared with the caller, who counts the
 *       parameters that are not the trunk's), [9] int32 [n_convs][4] HOST: bucket of (kernel, bias, BatchNorm weight,
 *       BatchNorm bias) of every convolution or -1,
 *   [10] peer all-reduce communicator (lidog_peer_comm_create) or 0: takes the statistics messages that fit its mailbox.
 * A bucket whose countdown reaches 0 inside lidog_trunk_backward is all-reduced (sum) on its stream behind events
 * recorded on `stream` and `lane`; the caller makes its optimiser step wait for that stream. */
int lidog_trunk_forward(const int64_t *convs, const double *conv_f, int32_t n_convs, const int64_t *maps,
                        int32_t n_maps, const int64_t *ops, int32_t n_ops, const int64_t *bufs, int32_t n_bufs,
                        const int64_t *level_rows, const int64_t *ext, void *arena, int64_t arena_bytes,
                        void *scratch, int64_t scratch_bytes, int64_t *rec, int64_t *need /*[2]*/, int32_t dry,
                        const int64_t *dp /*[12] or NULL*/, void *stream, void *lane /* or NULL */);
/* forward, lane: second stream (NULL = everything in line): the 1x1 downsample convolution + BatchNorm of a layer's first
 * block (minkunet_bev.py:414-420) runs on it next to conv1 / conv2 of that block and is joined in front of the residual add
 * (local BatchNorm only; same results).  Its scratch comes from the arena, so dry and real calls must pass the same lane.
 * backward, lane: second stream for the weight gradients (NULL = in line), forked behind each data gradient's GEMM
 * (wgrad_first = 0) or before it; joined into `stream` before the call returns. */
int lidog_trunk_backward(const int64_t *convs, const double *conv_f, int32_t n_convs, const int64_t *maps,
                         int32_t n_maps, const int64_t *ops, int32_t n_ops, const int64_t *bufs, int32_t n_bufs,
                         const int64_t *level_rows, const int64_t *ext, const int64_t *ext_grad, void *arena,
                         const int64_t *rec, void *garena, int64_t garena_bytes, void *scratch,
                         int64_t scratch_bytes, void *lane_scratch, int64_t lane_bytes, int64_t *need /*[3]*/,
                         int32_t *conv_done_host /*[n_convs]: 1 = this convolution's parameter gradients were written*/,
                         int32_t dry, int32_t wgrad_first, const int64_t *dp /*[12] or NULL*/, void *stream,
                         void *lane);
/* Fusions the executor applies on top of the operator path's launch sequence (bit mask; results are bit-identical
 * either way): 1 = BatchNorm-backward statistics in the epilogue of the producing data-gradient reduction
 * (lidog_sconv_reduce_rows_bwdstats); 2 = the ReLU masks of BatchNorm + residual + ReLU layers kept as bits
 * (lidog_bn_apply_bits); 4 = the BatchNorm + ReLU between the two convolutions of a block applied in the second one's
 * staging (lidog_sconv_*_in_bn) instead of by a pass of its own.  mask >= 0 sets it; returns the previous mask.  Set it between passes, not between a forward
 * pass and its backward pass. */
int32_t lidog_trunk_fusions(int32_t mask);
/* readers [n_ops]: which op (a 3^3 convolution + BatchNorm) applies op o's BatchNorm + ReLU in its staging under fusion 4,
 * -1 where the BatchNorm keeps its own pass -- conv1 of every BasicBlock in MinkUNet34.  Host only (tables as above). */
int lidog_trunk_in_bn_readers(const int64_t *convs, int32_t n_convs, const int64_t *maps, int32_t n_maps,
                              const int64_t *ops, int32_t n_ops, const int64_t *bufs, int32_t n_bufs, int32_t *readers);
/* Timing of the executor's gathered-GEMM launches for the roofline figure of bench.py: on != 0 brackets every such
 * launch with HIP events on its stream; _read waits for the recorded launches, returns (launches, total ms, algorithmic
 * FLOPs, algorithmic bytes: SURVEY.md 8(d)) in out[0..3] and forgets them.  One timing client per process. */
int lidog_trunk_gemm_timing(int32_t on);
int lidog_trunk_gemm_timing_read(double *out /*[4]*/);
/* algorithmic bytes of the executor's MFMA weight-gradient and per-row reduction launches while the timing is on:
 * out[0] launches / out[1] bytes (weight gradient), out[2] / out[3] (reduction), out[4] / out[5] (output-stationary
 * convolution); reading resets the counters */
int lidog_trunk_work_read(double *out /*[6]*/);

/* ------------------------------------------------------------------ instance norm (IBN-Net blocks)
 * Replaces ME.MinkowskiInstanceNorm (ME 0.5.4) and the IBN block's normalisation + ME.cat + ReLU,
 * utils/models/minkunet_ibn.py:26 (in_norm1) and :38-40 (bn_norm1 | in_norm1 -> ME.cat -> ReLU).
 * Every channel is normalised per scan: mean / invstd [B, C] over the rows of batch index b (biased variance,
 * invstd = 1 / sqrt(var + eps)); y = (x - mean[b]) * invstd[b] * w + bias with w, bias [C].  All sums in double,
 * finished in a fixed order (no float atomics: the same bits on every run).  [rows, C] with C % 4 == 0, C <= 1024 and
 * 2 B C <= 4096 take float4 kernels; any other shape plain scalar ones. */

/* bytes of workspace lidog_in_segments needs for a map of n rows */
int64_t lidog_in_segments_ws(int64_t n);
/* The segments of a coordinate map (minkunet_ibn.py:26): perm [n] = the rows in stable batch order (the radix sort
 * of csrc/prims.hip on the batch column), seg_off [B + 1] = where each batch index starts in perm (empty scans: empty
 * ranges), bid [n] = the batch index of every row.  B = largest batch index + 1 (<= 4096).  Rows may be in any order; build once per map. */
int lidog_in_segments(const int32_t *coords, int64_t n, int32_t B, int32_t *perm, int32_t *seg_off, int32_t *bid,
                      void *ws, int64_t ws_bytes, void *stream);
/* doubles of workspace the per-(b, c) reductions below need (minkunet_ibn.py:26,38-40) */
int64_t lidog_in_reduce_ws(int32_t B, int32_t C);
/* forward statistics (minkunet_ibn.py:26,38-40): mean / invstd [B, C] of x [n, C]; a scan without rows gets mean 0,
 * invstd 1 / sqrt(eps).  perm / seg_off from lidog_in_segments; ws: lidog_in_reduce_ws(B, C) doubles. */
int lidog_in_stats(const float *x, int64_t n, int32_t C, int32_t B, const int32_t *perm, const int32_t *seg_off,
                   float eps, float *mean, float *invstd, double *ws, void *stream);
/* y = (x - mean[bid[row]]) * invstd[bid[row]] * w + b (minkunet_ibn.py:26,38-40) */
int lidog_in_apply(const float *x, int64_t n, int32_t C, int32_t B, const int32_t *bid, const float *mean,
                   const float *invstd, const float *w, const float *b, float *y, void *stream);
/* backward reduction (minkunet_ibn.py:26,38-40): per (b, c) sum dy and sum dy * xhat, xhat = (x - mean) * invstd;
 * coef [2, B, C] = (sum dy / n_b, sum dy xhat / n_b); dw [C] = sum dy * xhat, db [C] = sum dy (sums over b ascending) */
int lidog_in_bwd_reduce(const float *dy, const float *x, int64_t n, int32_t C, int32_t B, const int32_t *perm,
                        const int32_t *seg_off, const float *mean, const float *invstd, double *ws, float *coef,
                        float *dw, float *db, void *stream);
/* dx = (dy - m0 - xhat * m1) * invstd * w with (m0, m1) = coef of the row's scan (minkunet_ibn.py:26,38-40) */
int lidog_in_bwd_apply(const float *dy, const float *x, int64_t n, int32_t C, int32_t B, const int32_t *bid,
                       const float *mean, const float *invstd, const float *w, const float *coef, float *dx,
                       void *stream);
/* The IBN block's forward pass after conv1 (minkunet_ibn.py:38-40): y [n, 2C] = ReLU(BN(x)) | ReLU(IN(x)) in one pass
 * over x [n, C], BatchNorm with mean / invstd [C] (lidog_bn_stats), instance norm with mean / invstd [B, C]
 * (lidog_in_stats), and the ReLU bit mask of y in relu_bits [lidog_relu_bits_words(n, 2 C)] (lidog_bn_apply_bits'
 * layout).  Equals lidog_bn_apply + lidog_in_apply + lidog_cat2 + lidog_relu_fwd bit for bit.  C % 4 == 0, n > 0. */
int lidog_ibn_apply(const float *x, int64_t n, int32_t C, int32_t B, const float *bn_mean, const float *bn_invstd,
                    const float *bn_w, const float *bn_b, const int32_t *bid, const float *in_mean,
                    const float *in_invstd, const float *in_w, const float *in_b, float *y, uint32_t *relu_bits,
                    void *stream);
/* Its backward reductions (minkunet_ibn.py:38-40) from dy [n, 2C] and the bit mask: the BatchNorm half's
 * (bn_sums [2C + 1], bn_dw / bn_db [C]; workspace lidog_bn_reduce_ws(C, 1) doubles) equal lidog_bn_bwd_reduce on the
 * ReLU-masked first half bit for bit; the instance-norm half's (in_coef, in_dw, in_db; in_ws lidog_in_reduce_ws(B, C))
 * equal lidog_in_bwd_reduce on the masked second half. */
int lidog_ibn_bwd_reduce(const float *dy, const uint32_t *relu_bits, const float *x, int64_t n, int32_t C, int32_t B,
                         const float *bn_mean, const float *bn_invstd, double *bn_sums, double *bn_ws, float *bn_dw,
                         float *bn_db, const int32_t *perm, const int32_t *seg_off, const float *in_mean,
                         const float *in_invstd, double *in_ws, float *in_coef, float *in_dw, float *in_db,
                         void *stream);
/* dx [n, C] = dx_BN + dx_IN in one pass (minkunet_ibn.py:38-40): lidog_bn_bwd_apply's and lidog_in_bwd_apply's
 * expressions on the masked halves of dy, added; bn_count = rows of the BatchNorm statistics */
int lidog_ibn_bwd_apply(const float *dy, const uint32_t *relu_bits, const float *x, int64_t n, int32_t C, int32_t B,
                        const float *bn_mean, const float *bn_invstd, const float *bn_w, const double *bn_sums,
                        double bn_count, const int32_t *bid, const float *in_mean, const float *in_invstd,
                        const float *in_w, const float *in_coef, float *dx, void *stream);

/* ------------------------------------------------------------------ MixStyle (csrc/mixstyle.hip)
 * MixStyle (Zhou et al., ICLR 2021): during training, every scan's per-channel feature statistics are interpolated with
 * those of another scan of the batch.  Not in the reference repository; this comment is the definition, restated in
 * float64 in tests/mixstyle_ref.py.
 * x [n, C] float32 are the rows of a sparse tensor, scan b has the n_b rows of batch index b (B scans, the segments of
 * lidog_in_segments).  lam [B] float32, partner [B] int32 and eps (a float, widened to double) come from the caller.
 * Per (b, c), all in double from double sums added in a fixed order (no float atomics, the same bytes on every run):
 *   mu  = sum x / n_b                                            (0 for a scan without rows)
 *   var = max(0, (sum x^2 - (sum x)^2 / n_b) / (n_b - 1))        the UNBIASED variance (0 for n_b < 2)
 *   sig = sqrt(var + eps)
 *   mu_mix = lam_b mu_b + (1 - lam_b) mu_p,  sig_mix = lam_b sig_b + (1 - lam_b) sig_p,  p = partner[b]
 * Three float32 tables [B, C], each rounded once from double: sub = mu_b, scale = sig_mix / sig_b, add = mu_mix.
 *   forward   y = fmaf(x - sub[b], scale[b], add[b]) in float32
 *   backward  dx = dy * scale[b], one float32 product: the statistics are constants to autograd (the paper's code
 *             detaches them)
 * IDENTITY SCANS.  n_b < 2, n_p < 2, partner[b] == b or lam_b == 1 make b an identity scan: its table rows are
 * (sub, scale, add) = (0, 1, 0) exactly (add carries the sign bit: fmaf(x, 1, -0) keeps the sign of a zero), so y == x and
 * dx == dy bit for bit.  A scan without rows is an identity scan.  partner need not be a permutation.
 * [rows, C] with C % 4 == 0, 4 <= C <= 1024 and 2 B C <= 4096 take float4 kernels and ONE launch for the statistics;
 * any other shape plain scalar kernels (two launches; no performance target). */

/* doubles of workspace lidog_mixstyle_stats needs: lidog_in_reduce_ws(B, C) and B more for lam / partner */
int64_t lidog_mixstyle_ws(int32_t B, int32_t C);
/* mean, sig [B, C] (float32 of mu and sig, for tests and benches) and the tables sub, scale, add [B, C].  perm / seg_off
 * from lidog_in_segments.  lam and partner are HOST arrays [B]: an entry of partner outside [0, B) is an error (return
 * code, lidog_last_error) with nothing queued; both are then copied to the end of the workspace by hipMemcpyAsync on
 * `stream`.  From pinned memory that copy does not wait for the device, and the arrays must stay unchanged until it
 * has run.  The last workgroup of the reduction finishes mean / sig of every (b, c) and, behind a workgroup barrier,
 * writes the tables: no host wait. */
int lidog_mixstyle_stats(const float *x, int64_t n, int32_t C, int32_t B, const int32_t *perm, const int32_t *seg_off,
                         const float *lam, const int32_t *partner, float eps, float *mean, float *sig, float *sub,
                         float *scale, float *add, double *ws, void *stream);
/* y [n, C] = fmaf(x - sub[b], scale[b], add[b]), b = bid[row] (lidog_in_segments' bid, every entry in [0, B)) */
int lidog_mixstyle_apply(const float *x, int64_t n, int32_t C, int32_t B, const int32_t *bid, const float *sub,
                         const float *scale, const float *add, float *y, void *stream);
/* dx [n, C] = dy * scale[bid[row]] */
int lidog_mixstyle_bwd(const float *dy, int64_t n, int32_t C, int32_t B, const int32_t *bid, const float *scale,
                       float *dx, void *stream);

/* ------------------------------------------------------------------ instance-whitening loss (RobustNet)
 * IWLoss (utils/losses/losses.py:464-485) of PLTRobustNet.training_step (trainer_lighting_robustnet.py) in closed form.
 * For a map x [n, C] (float32, row-major; n >= 2): S = sum_i sum_k |x_ik| P_ik with P_ik = sum_{j<k} |x_ij|, and the
 * reference's loss is L = S / (n (n - 1)) (pass w = 1 / (n (n - 1))).  Up to 8 maps per launch, any C; C % 4 == 0 and
 * C <= 128 take the float4 kernels (16-byte aligned maps).  Sums in double, finished in a fixed order: no float
 * atomics, the same bits on every run. */

/* doubles of workspace lidog_iw_fwd needs (any M) */
int64_t lidog_iw_ws(void);
/* per_map [M] and total [1] (device, float32): per_map[m] = w[m] * S(x[m]), total = scale * sum_m per_map[m] (ascending m,
 * in double).  x, n, C, w are HOST arrays of M entries; x[m] device pointers. */
int lidog_iw_fwd(const float *const *x, const int64_t *n, const int32_t *C, const double *w, int32_t M, double scale,
                 double *ws, float *total, float *per_map, void *stream);
/* gx[m] [n_m, C_m] = sign(x) (P + Q) * gout[0] * scale * w[m], Q_ik = sum_{j>k} |x_ij| (reverse scan); gout is a
 * device scalar (the gradient of total); gx HOST array of M device pointers. */
int lidog_iw_bwd(const float *const *x, const int64_t *n, const int32_t *C, const double *w, int32_t M, double scale,
                 const float *gout, float *const *gx, void *stream);

/* ------------------------------------------------------------------ scan mixing (PointCutMix, CoSMix)
 * The per-point work of PointCutMixSourceDataset.merge_data (utils/datasets/pointcutmix.py:43-135) and
 * CoSMixSourceDataset.merge_data (utils/datasets/cosmix.py:50-171), which the reference runs with numpy in DataLoader
 * workers.  The random draws stay on the host; both quantisations are lidog_voxel_floor + lidog_coords_insert +
 * lidog_coords_compact.  Every position is computed from counts and scans, never taken by an atomic: the same result on
 * every run. */
/* counts[b] = number of keys equal to b for b in [0, nbins); keys outside are skipped; counts is zeroed here.
 * np.unique(inverse_map, return_counts=True) of the 10 m cells (pointcutmix.py:91-92) and the classes present in the
 * source, np.unique(source_sem_labels) (cosmix.py:108-112) */
int lidog_mix_histogram(const int32_t *keys, int64_t n, int32_t nbins, int32_t *counts, void *stream);
/* int32 workspace of lidog_mix_split */
int64_t lidog_mix_split_ws(int64_t n, int32_t n_slots);
/* Stable multi-way split: row i goes to slot slot_of_key[keys[i]] (a key outside [0, n_keys) or a slot outside
 * [0, n_slots): not taken).  rows_out (room for n) = the taken rows grouped by slot in ascending slot order, ascending
 * row order inside a slot; slot_start [n_slots + 1] (device) = start of each slot in rows_out, then the total.
 * n_slots <= 256.  The reference's concatenation of `source[inverse_map == sv]` over the drawn cells
 * (pointcutmix.py:100-106) and of `source[source_sem_labels == sv]` over the drawn classes (cosmix.py:120-126). */
int lidog_mix_split(const int32_t *keys, int64_t n, const int32_t *slot_of_key, int32_t n_keys, int32_t n_slots,
                    int32_t *rows_out, int32_t *slot_start, int32_t *ws, void *stream);
/* The merged point set before its re-quantisation (pointcutmix.py:94-112, cosmix.py:114-148): merged row r < n_target
 * is target row r; row n_target + j is source row rows[j] when perm is NULL (every row of every slot), else
 * rows[slot_start[s] + perm[j]] for the slot s with take_start[s] <= j < take_start[s + 1] (device, n_slots + 1
 * entries): the random sub-sample of cosmix.py:56-63,128-133, perm[j] < size of slot s.  coords_out [n_target + n_take, 3]
 * = float(coordinate) * voxel_size in float32 (`coordinates * self.voxel_size`, pointcutmix.py:45-46, cosmix.py:68-69).  Columns: cols_host
 * holds 3 * n_cols HOST-side entries (target, source, merged device pointers of column k) and col_words_host the 32-bit
 * words per row of each column (features, labels, xyz, sampled_idx); n_cols <= 6. */
int lidog_mix_gather(const int32_t *coords_t, int64_t n_target, const int32_t *coords_s, const int32_t *rows,
                     const int32_t *slot_start, const int32_t *perm, const int32_t *take_start, int32_t n_slots,
                     int64_t n_take, float voxel_size, float *coords_out, int32_t n_cols, void *const *cols_host,
                     const int32_t *col_words_host, void *stream);
/* The same merged set with CoSMix's in-merge augmentation (cosmix.py:135-136: `self.augmentations(coords_tmp)` on every
 * pasted class), written as voxel rows in ONE launch, without atomics: merged row r < n_target is target row r, row
 * n_target + j is source row rows[slot_start[s] + perm[j]] (perm NULL: rows[j]) of the slot s with take_start[s] <= j <
 * take_start[s + 1]; take_start (device, n_slots + 1) is always read.  coords_s has n_source rows, and rows room for
 * n_source entries: an index outside is clamped, nothing outside is read.  A class row float(c) * voxel_size (float32) is
 * transformed by the n_ops <= 4 operations op_kinds_host (HOST, shared by the slots; 0 rotation, 1 scale, the
 * arithmetic of lidog_augment_points) with the slot's own parameters slot_params[(s * n_ops + o) * 9 ..] (device,
 * float64, n_slots <= 256); a target row is left as it is.  f64 != 0: the concatenation is float64 (torch.cat of the
 * float32 target rows with rotated class rows), so EVERY row is floored as float64, floor(double(x) / q); f64 == 0:
 * every row is float32 and floored as lidog_voxel_floor does.  rows_out [n_target + n_take, 4] int32 = (0, voxel), ready
 * for lidog_coords_insert.  Columns as lidog_mix_gather. */
int lidog_mix_gather_aug(const int32_t *coords_t, int64_t n_target, const int32_t *coords_s, int64_t n_source,
                         const int32_t *rows, const int32_t *slot_start, const int32_t *perm,
                         const int32_t *take_start, int32_t n_slots, int64_t n_take, float voxel_size,
                         const int32_t *op_kinds_host, int32_t n_ops, const double *slot_params, int32_t f64, double qx,
                         double qy, double qz, int32_t *rows_out, int32_t n_cols, void *const *cols_host,
                         const int32_t *col_words_host, void *stream);

/* ------------------------------------------------------------------ sensor-aware scan mixing (PolarMix, LaserMix)
 * PolarMix (Xiao et al., NeurIPS 2022) swaps an azimuth sector between two voxelised scans and pastes rotated copies of
 * the instance classes; LaserMix (Kong et al., CVPR 2023) interleaves the two scans by inclination band.  Neither is in
 * the reference: the arithmetic below IS the definition (lidog_amd.data.polarmix_merge / lasermix_merge,
 * tests/sensormix_ref.py).  Geometry is decided on the voxel centre in doubled integer units, X = 2x + 1, Y = 2y + 1,
 * Z = 2z + 1, the sensor at the origin; azimuth and inclination do not depend on the voxel size.  The device evaluates
 * no atan2, sqrt, sin or cos: the host passes float64 constants.  Every float64 product, sum and difference named below
 * is rounded on its own, never fused.  Every position comes from the stable split of csrc/prims.hip: no atomics, the
 * same bytes on every run. */
/* One launch over the rows of both scans (coords0 [n0, 3], coords1 [n1, 3] int32; labels0 / labels1 int32 per row, NULL:
 * no row is an instance row): keys [n0 + n1] int32, scan 0's rows first,
 *   bit 0      in the sector: sa = ax * Y - ay * X, sb = bx * Y - by * X; wide == 0: sa >= 0 && sb < 0 (the sector from
 *              direction a counter-clockwise to direction b, narrower than pi); wide != 0: sa >= 0 || sb < 0
 *   bits 1-3   band = the number of the n_bounds <= 7 ascending inclination boundaries the row is at or above.
 *              Boundary j is t2_host[j] = tan(theta_j)^2 >= 0 with neg_host[j] = (tan theta_j < 0) (HOST arrays); with
 *              R = X * X + Y * Y (exact in int64 and in float64) a row is at or above it when
 *              neg == 0: Z > 0 && double(Z * Z) >= t2 * double(R);  neg != 0: Z > 0 || double(Z * Z) <= t2 * double(R)
 *   bit 4      0 <= label < 32 and bit `label` of instance_mask is set
 * Precondition |x|, |y|, |z| < 2^24.  info [1] (device, int32) is zeroed here; a row outside the range sets info[0] = 1
 * and its key is not written: the caller raises.  n0 + n1 == 0: info zeroed, nothing launched. */
int lidog_sensormix_keys(const int32_t *coords0, const int32_t *labels0, int64_t n0, const int32_t *coords1,
                         const int32_t *labels1, int64_t n1, double ax, double ay, double bx, double by, int32_t wide,
                         const double *t2_host, const int32_t *neg_host, int32_t n_bounds, uint32_t instance_mask,
                         int32_t *keys, int32_t *info, void *stream);
/* int32 workspace of lidog_sensormix_select */
int64_t lidog_sensormix_select_ws(int64_t n_base, int64_t n_donor);
/* The three row lists of a merge, each ascending (lidog_split_rows with one slot): rows_keep = the base rows i with bit
 * keys_base[i] of keep_keys set, rows_take / rows_paste = the donor rows with bit keys_donor[i] of take_keys /
 * paste_keys set (a key outside [0, 32): in no list).  rows_keep has room for n_base, rows_take and rows_paste for
 * n_donor entries.  sizes [6] (device, int32) = (0, |keep|, 0, |take|, 0, |paste|): the one read-back of a merge.  A
 * set of keys that is 0 and an empty scan launch nothing for their list. */
int lidog_sensormix_select(const int32_t *keys_base, int64_t n_base, const int32_t *keys_donor, int64_t n_donor,
                           uint32_t keep_keys, uint32_t take_keys, uint32_t paste_keys, int32_t *rows_keep,
                           int32_t *rows_take, int32_t *rows_paste, int32_t *sizes, int32_t *ws, void *stream);
/* The merged voxel rows in one launch.  rows_out [n_keep + n_take + n_copies * n_paste, 4] int32 = (0, voxel), ready for
 * lidog_coords_insert (16-byte aligned): base row rows_keep[r] for r < n_keep, then donor row rows_take[j], then for
 * copy k = 0 .. n_copies - 1 (n_copies <= 8) donor row rows_paste[j] rotated about z by (c, s) = (cs_host[2k],
 * cs_host[2k + 1]) (HOST, float64: cos and sin of the angle): U = double(x) + 0.5, V = double(y) + 0.5, x' = c * U -
 * s * V, y' = s * U + c * V, voxel (floor(x'), floor(y'), z).  Base rows, taken rows and a copy with (c, s) == (1, 0)
 * keep their integer voxel without a float round trip.  A list entry outside its scan (n_base, n_donor rows) is
 * clamped, nothing outside is read.  Columns as lidog_mix_gather (base, donor, merged pointer triples), copied from the
 * source row unchanged.  No row at all: nothing launched. */
int lidog_sensormix_gather(const int32_t *coords_base, int64_t n_base, const int32_t *coords_donor, int64_t n_donor,
                           const int32_t *rows_keep, int64_t n_keep, const int32_t *rows_take, int64_t n_take,
                           const int32_t *rows_paste, int64_t n_paste, const double *cs_host, int32_t n_copies,
                           int32_t *rows_out, int32_t n_cols, void *const *cols_host, const int32_t *col_words_host,
                           void *stream);

/* ------------------------------------------------------------------ SN car-size scaling: DBSCAN, cluster boxes, scaling
 * The start-up statistics of train_scaling_based.py:35-129 (get_average_dims clusters the car voxels of every drawn
 * scan with sklearn.cluster.DBSCAN) and the per-item scaling of utils/datasets/sn_scaling.py.  Integer atomics whose
 * result does not depend on their order only: the same bytes on every run. */
/* bytes of workspace lidog_dbscan needs for n points */
int64_t lidog_dbscan_ws(int64_t n);
/* labels [n] (device, int32) = sklearn.cluster.DBSCAN(eps, min_samples).fit_predict(x), x = float32(coords) *
 * float32(voxel_size) (`coordinates * voxel_size`, train_scaling_based.py:46), label for label: -1 noise, clusters
 * numbered in the order of their smallest core row, a border point in the smallest-numbered cluster it touches.  Two
 * points are neighbours when sum_k (double(x_i[k]) - double(x_j[k]))^2 <= eps^2 in float64 (a point is its own
 * neighbour).  coords [n, 3] int32, distinct rows, |c| <= 65535.  info [2] (device, int32): info[0] = 0, or 1 (a
 * coordinate out of range) or 2 (the grid of eps-sized cells over the bounding box has more than 2^32 cells) and then
 * labels are not written; info[1] = the number of clusters.  n = 0: info zeroed, nothing else touched. */
int lidog_dbscan(const int32_t *coords, int64_t n, float voxel_size, double eps, int32_t min_samples, int32_t *labels,
                 int32_t *info, void *ws, int64_t ws_bytes, void *stream);
/* counts [k] (int64), lo / hi [k, 3] (int32): rows and per-axis minimum / maximum coordinate of every label in [0, k)
 * (other labels are skipped; a label without rows keeps count 0, lo INT32_MAX, hi INT32_MIN).  The integer form of
 * np.sum(cluster_idx == c) and np.min / np.max of the cluster's columns (train_scaling_based.py:58-79). */
int lidog_cluster_boxes(const int32_t *coords, const int32_t *labels, int64_t n, int32_t k, int64_t *counts,
                        int32_t *lo, int32_t *hi, void *stream);
/* out [n, 3] float32 = (float(coords) * voxel_size) * (sx, sy, sz), each product rounded to float32
 * (sn_scaling.py:39,53-55 / :109-110,133-139): the input of the item's re-quantisation */
int lidog_sn_scale_coords(const int32_t *coords, int64_t n, float voxel_size, float sx, float sy, float sz, float *out,
                          void *stream);

/* ------------------------------------------------------------------ training augmentation (sub_p, augmentation_list)
 * The per-point part of a training item of the reference's datasets when `augmentation_list` is not null
 * (utils/datasets/semantickitti_bev.py:209-238, synth4d.py:141-162): the sub-sample gather (dataset.py:58-72),
 * RandomRotation / RandomScale (utils/common/augmentation.py:7-44) under numpy's dtype rules, the bounds filter
 * (semantickitti_bev.py:155-172) and the voxel floor of ME.utils.sparse_quantize in the point's own dtype.  The host
 * makes the draws.  Positions of the kept rows come from the ordered compaction of csrc/prims.hip (lidog_mix_split's
 * kernels with one slot): the same bytes on every run. */
/* 1 when the list holds a rotation: the points leave as float64 (`coords @ R`, R float64), else 0 (float32) */
int32_t lidog_augment_is_f64(const int32_t *op_kinds_host, int32_t n_ops);
/* int32 workspace of lidog_augment_points for k sampled rows (read only with use_bounds) */
int64_t lidog_augment_ws(int64_t k);
/* points [n, 3] float32; sampled_idx [k] int32 (device; NULL: every row in order, k = n; an entry outside [0, n) is
 * clamped and info[1] set).  Operations, applied in order (HOST arrays, n_ops <= 4): op_kinds_host[o] = 0 rotation
 * (op_params_host[9 o ..] = R row-major, p <- p @ R, each output (p0 R0j + p1 R1j) + p2 R2j in float64, the point is
 * float64 from here on) or 1 scale (three float64 factors; a float64 point takes one float64 product per axis, a point
 * that is still float32 takes float32(float64(p_k) * s_k)).  use_bounds: only rows with -60 < x, y < 60, -10 < z < 8
 * outside the ego box (-3 < x < 3 and -2 < y < 2) are kept, in order.  Per kept row r (all device, room for k rows):
 * rows [k, 4] int32 = (batch, floor(p / q)) with float64 division for a float64 point and float32 division by
 * float32(q) otherwise; xyz [k, 3] float64 or float32 (lidog_augment_is_f64); src [k] = its row in `points`;
 * labels_out [k] = labels[src] when labels (int32 [n]) is given.  info [2] int32 (device): info[0] = kept rows, info[1]
 * = 1 when a sampled index was out of range.  ws: lidog_augment_ws(k) int32. */
int lidog_augment_points(const float *points, int64_t n, const int32_t *sampled_idx, int64_t k,
                         const int32_t *op_kinds_host, const double *op_params_host, int32_t n_ops, int32_t use_bounds,
                         double qx, double qy, double qz, int32_t batch, const int32_t *labels, int32_t *rows, void *xyz,
                         int32_t *src, int32_t *labels_out, int32_t *info, int32_t *ws, void *stream);

/* ------------------------------------------------------------------ evaluation statistics (eval_target)
 * What test_step computes per loader batch (utils/pipelines/trainer_lighting.py:186-253, trainer_lighting_bev.py:
 * 265-323) up to integer counts: the arg-max and the confusion counts that sklearn's jaccard_score and the
 * present-label mask are made of, and the packed records of the prediction dump.  Integer LDS bins, one global integer
 * atomic per non-empty bin and block, positions from lidog_mix_split: the same bytes on every run. */
/* logits [n, n_classes] float32 (n_classes <= 32), labels [n] int64, coords [n, 4] int32 (column 0 = scan of the row).
 * preds [n] int64 = torch's CPU `logits.max(dim=1)[1]`: the first maximal index, the first NaN in a row holding one.
 * counts [n_scans, n_classes + 1, n_classes] int64 is ADDED to: counts[scan, label + 1, pred] for labels in
 * [0, n_classes) other than ignore_label, counts[scan, 0, pred] for every other label.  A row whose scan is outside
 * [0, n_scans) is not counted and sets err[0] = 1 (device int32, never cleared here).  Rows of one scan need not be
 * contiguous. */
int lidog_eval_confusion(const float *logits, const int64_t *labels, const int32_t *coords, int64_t n,
                         int32_t n_classes, int32_t n_scans, int64_t ignore_label, int64_t *preds, int64_t *counts,
                         int32_t *err, void *stream);
/* int32 workspace of lidog_eval_pack */
int64_t lidog_eval_pack_ws(int64_t n, int32_t n_scans);
/* The prediction dump of test_step: per scan the rows with label != ignore_label in ascending row order.  out (int32,
 * room for n_scans + 1 + 5 n): out[s] = first record of scan s, out[n_scans] = number of records, then the records
 * (x, y, z, prediction, label) grouped by scan: the voxel coordinates, as the reference writes them.  n_scans <= 256.
 * A row whose scan is outside [0, n_scans) is left out and sets err[0] = 1. */
int lidog_eval_pack(const int32_t *coords, const int64_t *preds, const int64_t *labels, int64_t n, int32_t n_scans,
                    int64_t ignore_label, int32_t *out, int32_t *err, int32_t *ws, void *stream);

/* ------------------------------------------------------------------ training-step statistics (log_losses)
 * The batch-wide confusion counts behind the per-step training metrics (utils/pipelines/trainer_lighting_2d.py:203-291,
 * trainer_lighting.py:118-153) of up to 8 tensors ("segments": the point logits of each source, every BEV level) in ONE
 * launch.  logits, labels and n are HOST arrays of n_segments entries (1..8); the table travels as a kernel argument.
 * Segment s is n[s] contiguous rows of n_classes float32 (1..32 classes) with one int64 label per row; n[s] == 0 is
 * legal and its pointers are not read.  A BEV level is passed as it is: the rows of n_classes consecutive floats of the
 * contiguous NCHW buffer are what `bev_preds.view(b, h, w, -1).argmax(-1)` reads, n = b * h * w.
 * counts [n_segments, n_classes + 1, n_classes] int64 is ADDED to (the caller zeroes it): counts[s, label + 1, pred]
 * for labels in [0, n_classes) other than ignore_label, counts[s, 0, pred] for every other label; pred = the first
 * maximal index, the first NaN in a row holding one (lidog_eval_confusion's rule).  A label other than ignore_label
 * outside [0, n_classes) also sets bit s of err[0] (device int32, never cleared here).  Nothing outside counts and err
 * is written.  Integer LDS bins, one global integer atomic per non-empty bin and block: the same bytes on every run. */
int lidog_train_confusion(const float *const *logits, const int64_t *const *labels, const int64_t *n,
                          int32_t n_segments, int32_t n_classes, int64_t ignore_label, int64_t *counts, int32_t *err,
                          void *stream);

/* ------------------------------------------------------------------ scans read from files (SemanticKITTI, nuScenes, Synth4D)
 * What the reference's datasets do with numpy between the file and the cached `data` dict of __getitem__
 * (utils/datasets/semantickitti.py:100-131,190-197, nuscenes.py:144-178,238-248, synth4d.py:106-137) and in
 * get_dataset_stats (semantickitti.py:199-213): unpack the records, map the labels, apply the radius mask, compact the
 * kept rows in order, count the labels per class.  The host uploads the files' bytes unmodified.  Positions come from
 * the ordered compaction of csrc/prims.hip and the statistics are integer counts: the same bytes on every run.  No
 * allocation, synchronisation or
 * blocking copy inside. */
/* int32 workspace of lidog_scan_load for a file of n rows */
int64_t lidog_scan_load_ws(int64_t n);
/* points_raw: n records of point_stride >= 3 float32, the first three x y z (4: SemanticKITTI .bin, 5: nuScenes .bin);
 * NULL: the labels alone (the statistics of a label file), nothing but counts and info[1] is written.
 * labels_raw [n]: label_kind 1 = int32, 2 = uint8, 0 = none (label 0 for every row, unmapped; labels_raw is not read).
 * Mapped label = lut[idx] under numpy's indexing, idx = raw & label_mask for int32 labels (-1: no mask; 0xFFFF for
 * SemanticKITTI) or the byte itself: 0 <= idx < lut_len as is, -lut_len <= idx < 0 wraps, anything else adds one to
 * info[1] (numpy's IndexError).  use_radius: only rows with ((x x + y y) + z z) < radius_sq are kept, every product and
 * sum rounded to float32 on its own (no fused multiply-add), the comparison strict, a NaN dropped:
 * `np.sum(np.square(points), axis=1) < in_R ** 2` with radius_sq = float32(in_R ** 2).
 * points_out [n, 3] float32 and labels_out [n] int32 (room for n rows): the kept rows in ascending order, the
 * coordinates copied bit for bit.  counts [num_classes] int64 (optional, num_classes <= 256) is ADDED to: the mapped
 * labels of ALL n rows, before the radius mask, labels outside [0, num_classes) skipped.  info [4] int32 (device,
 * cleared here): kept rows, label errors, kept rows with a non-finite coordinate (only possible without the radius
 * mask), 0.  ws: lidog_scan_load_ws(n) int32. */
int lidog_scan_load(const float *points_raw, int32_t point_stride, const void *labels_raw, int32_t label_kind,
                    int32_t label_mask, int64_t n, const int32_t *lut, int32_t lut_len, int32_t use_radius,
                    float radius_sq, float *points_out, int32_t *labels_out, int64_t *counts, int32_t num_classes,
                    int32_t *info, int32_t *ws, void *stream);

/* ------------------------------------------------------------------ one label per point of a scan file (csrc/pointlabels.hip)
 * What the SemanticKITTI and nuScenes-lidarseg benchmarks score: a class for every record of the file, in file order.
 * The voxel logits go back to the points through the row every record has in lidog_scan_load's output (keep_row) and
 * the voxel every kept row fell into (inverse_map).  Positions come from the ordered compaction of csrc/prims.hip and the
 * counts are integers:
 * the same bytes on every run.  No allocation, synchronisation or blocking copy inside. */
/* int32 workspace of lidog_scan_keep_rows for a file of n rows */
int64_t lidog_scan_keep_rows_ws(int64_t n);
/* points_raw, point_stride, n, use_radius, radius_sq: as lidog_scan_load takes them (the same radius test, the same
 * stable compaction).  keep_row [n] int32: the row of record i among lidog_scan_load's kept rows, -1 for a record the
 * mask dropped (without use_radius: i itself).  info [1] int32 (device): the number of kept rows.  n = 0 launches
 * nothing and writes info = 0.  ws: lidog_scan_keep_rows_ws(n) int32 (not read without use_radius). */
int lidog_scan_keep_rows(const float *points_raw, int32_t point_stride, int64_t n, int32_t use_radius, float radius_sq,
                         int32_t *keep_row, int32_t *info, int32_t *ws, void *stream);
/* int32 workspace of lidog_point_labels: the arg-max of every voxel row */
int64_t lidog_point_labels_ws(int64_t n_voxels);
/* A loader batch of n_scans (1..64) files.  logits [n_voxels, n_classes] float32 (n_classes <= 32): the batch's voxel
 * rows, scan after scan.  row_off / kept_off / vox_off [n_scans + 1] int64, HOST arrays (they travel as a kernel
 * argument: nothing is copied in front of the launch): where every scan's file rows, kept rows and voxel rows start in the
 * concatenated arrays, from 0, non-decreasing, ending at n_rows / n_kept / n_voxels (checked here); any of a scan's
 * three ranges may be empty.  keep_row [n_rows]
 * int32: lidog_scan_keep_rows' output of every file, concatenated.  inverse_map [n_kept] int64: the voxel row, within
 * its scan, of every kept row.  Prediction of a voxel row = the first maximal index, the first NaN in a row holding one
 * (lidog_eval_confusion's rule), taken once per voxel row into ws.
 * labels_out [n_rows] uint32: out_lut[prediction] (out_lut [n_classes] int32) of the record's voxel, `fill` for a
 * record with keep_row = -1.
 * label_kind 1 / 2 (0: no labels, counts is not touched): labels_raw [n_rows], label_mask, lut, lut_len as
 * lidog_scan_load takes them, the files' label words concatenated.  counts [n_scans, n_classes, n_classes] int64 is
 * ADDED to: counts[scan, label, prediction] over the kept records whose mapped label lies in [0, n_classes) and is not
 * ignore_label.
 * err [1] int32 (device, never cleared here) collects bits: 1 a file row outside every scan's range (excluded by the
 * offset checks), 2 a raw label outside the table, 4 an inverse_map entry outside its scan's voxel rows, 8 a keep_row entry
 * outside its scan's kept rows.  Such a record keeps `fill` and is counted nowhere; no value is used as an index before
 * it is checked.  ws: lidog_point_labels_ws(n_voxels) int32. */
int lidog_point_labels(const float *logits, int64_t n_voxels, int32_t n_classes, int32_t n_scans,
                       const int64_t *row_off, const int64_t *kept_off, const int64_t *vox_off, int64_t n_rows,
                       int64_t n_kept, const int32_t *keep_row, const int64_t *inverse_map, const int32_t *out_lut,
                       uint32_t fill, const void *labels_raw, int32_t label_kind, int32_t label_mask,
                       const int32_t *lut, int32_t lut_len, int64_t ignore_label, uint32_t *labels_out, int64_t *counts,
                       int32_t *err, int32_t *ws, void *stream);

/* ------------------------------------------------------------------ bf16-operand forward kernels (csrc/sconv_bf16.hip)
 * Opt-in evaluation path (lidog_amd/precision.py): activations stay fp32 in memory, the gathered rows are rounded to bf16
 * (nearest even) as they are staged, the weights are packed once, accumulation is fp32 (v_mfma_f32_32x32x16_bf16).
 * Cin and Cout must be multiples of 32.  The results are NOT the bits of the fp32 kernels.
 *
 * lidog_pack_kernels_bf16: fp32 [K][Cin][Cout] -> bf16 [K][Cout][Cin] for every kernel of a table in one launch:
 * desc int64 [n_mats][6] = (src offset in floats from `src` (may be negative), dst offset in bf16 elements from `dst`,
 * K, Cin, Cout, first 32x32 tile); total_tiles = sum of K ceil(Cin / 32) ceil(Cout / 32). */
int lidog_pack_kernels_bf16(const float *src, uint16_t *dst, const int64_t *desc, int32_t n_mats, int64_t total_tiles,
                            void *stream);
/* lidog_sconv_gemm_bf16: the gathered GEMM (arguments as lidog_sconv_gemm; Wp = the packed weights): gather == NULL
 * takes the pair-rows themselves, scatter != NULL writes row scatter[pair] instead of the pair-row, a negative gather
 * index is a row of zeros.  T is fp32, what lidog_sconv_reduce_rows[_bn] consume. */
int lidog_sconv_gemm_bf16(const float *A, const int32_t *gather, const uint16_t *Wp, const float *bias,
                          const int32_t *tile_k, const int32_t *tile_row0, const int32_t *tile_rows, int32_t n_tiles,
                          int32_t Cin, int32_t Cout, float *T, const int32_t *scatter, void *stream);
/* lidog_sconv_os_bn_bf16: lidog_sconv_os_bn (forward, evaluation-mode BatchNorm + residual + ReLU) with bf16 operands;
 * the offsets accumulate into one set of registers. */
int lidog_sconv_os_bn_bf16(const float *A, const int32_t *nbr, int64_t n, int32_t K, const int32_t *perm,
                           const uint32_t *wave_masks, const int32_t *tile_order, const uint16_t *Wp, const float *bias,
                           int32_t Cin, int32_t Cout, const float *mean, const float *invstd, const float *w,
                           const float *b, const float *residual, int32_t relu, float *out, void *stream);

/* ------------------------------------------------------------------ bf16-operand weight gradient (csrc/sconv_bf16.hip)
 * Opt-in mixed-precision training (lidog_amd/precision.py): the forward pass and the data gradient of an eligible
 * convolution run lidog_sconv_gemm_bf16 (the data gradient over the exchanged map with the packed transposed kernel);
 * the weight gradient is lidog_sconv_wgrad_bf16: arguments and semantics of lidog_sconv_wgrad, both gathered operands
 * rounded to bf16 (nearest even) as they are staged, fp32 accumulation, fp32 partial slots and fp32 gW (summed per
 * offset in fixed order: bit-reproducible).  Cin and Cout must be multiples of 32.
 * lidog_sconv_wgrad_bf16_slabs: Cin * Cout-float slots `partial` needs for n_items work items (0: not a bf16 shape).
 * lidog_sconv_wgrad_bf16_slots: workgroups of the Cin x Cout kernel resident on the chip at a time (0: unknown). */
int32_t lidog_sconv_wgrad_bf16_slabs(int32_t Cin, int32_t Cout, int32_t n_items);
int32_t lidog_sconv_wgrad_bf16_slots(int32_t Cin, int32_t Cout);
int lidog_sconv_wgrad_bf16(const float *A, const int32_t *pair_a, const float *G, const int32_t *pair_g,
                           const int32_t *items, int32_t n_items, const int32_t *item_off, int32_t K, int32_t Cin,
                           int32_t Cout, float *partial, float *gW, void *stream);

/* ------------------------------------------------------------------ sparse pooling (csrc/pool.hip)
 * Replaces ME.Minkowski{Sum,Avg,Max}Pooling, MinkowskiPoolingTranspose and MinkowskiGlobal{Sum,Avg,Max}Pooling of
 * MinkowskiEngine 0.5.4 (utils/models/resnet_old.py:28,53; utils/models/common.py:126,180,208).  Features fp32 [rows, C],
 * any C >= 1 (float4 kernels when C % 4 == 0, scalar ones otherwise).  Every entry is a gather written with plain
 * stores: no atomics, the same bits on every call.  n == 0 returns without a launch.
 *
 * Local pooling walks the per-row lists of lidog_kernel_map_rows of the RESULT side: row r owns the pair positions
 * row_list[row_ptr[r] .. row_ptr[r + 1]) (ascending offset), other[p] is the row on the other side of pair p (pair_in
 * when the result rows are the map's output rows, pair_out when they are its input rows).
 *
 * lidog_pool_rows: y[r] = sum over p of x[other[p]]; avg != 0: divided by the number of pairs of r (the neighbours
 * that exist, not the kernel volume); other_row_ptr != NULL: every term x[o] is divided by the pair count of o on ITS
 * side (other_row_ptr[o + 1] - other_row_ptr[o]) before it is added -- the gradient of an average, gathered from the
 * input side.  A row without pairs gets exact zeros.  Serves the forward pass (output rows), the gradients of sum and
 * avg (input rows), the transposed pooling (input rows, avg) and its gradient (output rows, other_row_ptr). */
int lidog_pool_rows(const float *x, const int32_t *row_ptr, const int32_t *row_list, const int32_t *other, int64_t n,
                    int32_t C, int32_t avg, const int32_t *other_row_ptr, float *y, void *stream);
/* y[r][c] = max over p of x[other[p]][c], arg[r][c] = other[p] of the FIRST maximum in list order (strict >: a tie
 * stays with the lowest offset).  A NaN wins over every number and the first NaN stays (torch.amax's value).  A row
 * without pairs gets y = 0, arg = -1. */
int lidog_pool_rows_max(const float *x, const int32_t *row_ptr, const int32_t *row_list, const int32_t *other,
                        int64_t n, int32_t C, float *y, int32_t *arg, void *stream);
/* gx[i][c] = sum over the pairs p of INPUT row i of gy[other[p]][c] where arg[other[p]][c] == i (row lists of the
 * input side, other = the output row of a pair; arg [n_out, C] of lidog_pool_rows_max). */
int lidog_pool_rows_max_bwd(const float *gy, const int32_t *arg, const int32_t *row_ptr, const int32_t *row_list,
                            const int32_t *other, int64_t n, int32_t C, float *gx, void *stream);
/* Global pooling: one reduction per scan over the segments of lidog_in_segments (perm, seg_off [B + 1], bid).
 * mode 0 = sum, 1 = avg (sum / rows of the scan), 2 = max with arg [B, C] = the row of the maximum (ties and two NaNs
 * go to the smaller row index = the first in the scan's order).  y [B, C]; a batch index without rows gets zeros (and
 * arg = -1).  The sums are per-workgroup partials added in workgroup order; the cut into workgroups depends on
 * (n, B, C) alone.
 * ws: lidog_pool_global_ws(n, B, C) bytes. */
int64_t lidog_pool_global_ws(int64_t n, int32_t B, int32_t C);
int lidog_pool_global(const float *x, int64_t n, int32_t C, int32_t B, const int32_t *perm, const int32_t *seg_off,
                      int32_t mode, float *y, int32_t *arg /* mode 2 only */, void *ws, int64_t ws_bytes, void *stream);
/* gx[i] = gy[bid[i]] (sum), gy[bid[i]] / rows of that scan (avg), gy[b][c] where arg[b][c] == i else 0 (max) */
int lidog_pool_global_bwd(const float *gy, const int32_t *arg, int64_t n, int32_t C, int32_t B, const int32_t *bid,
                          const int32_t *seg_off, int32_t mode, float *gx, void *stream);

/* ------------------------------------------------------------------ point <-> voxel family (csrc/field.hip)
 * ME.TensorField / TensorField.sparse, SparseTensor.slice / cat_slice / features_at_coordinates / interpolate and
 * MinkowskiInterpolation of MinkowskiEngine 0.5.  The reference never calls them and MinkowskiEngine's sources were not
 * at hand: every rule below is restated from memory [ME-mem] and THIS text is the contract the tests hold the kernels to.
 * Features fp32 [rows, C], any C >= 1 (float4 kernels when C % 4 == 0).  Plain stores in a stated order everywhere: no
 * atomics on floats, the same bits on every call.  An entry with nothing to do returns without a launch.
 *
 * lidog_field_floor [ME-mem]: points [n, 4] float32 rows (batch, x, y, z) -> rows [n, 4] int32.  Spatial columns:
 * floor(v / s) * s in float32 (a true division, s = (float)stride), then lidog_voxel_floor's conversion: NaN, an infinity
 * or a value no int32 holds gives INT32_MIN, which matches no map row.  The batch column must be integer-valued in
 * 0 .. 4095, else the row gets batch -1 (matches no map row).  err [1] int32 (device, never cleared here) collects bits:
 * 1 a bad batch column, 2 a NaN or infinite spatial column.  A finite value beyond the coordinate range sets no bit: such
 * a point simply has no neighbours. */
int lidog_field_floor(const float *points, int64_t n, int32_t stride, int32_t *rows, int32_t *err, void *stream);
/* Per-row lists of an index table (the stable radix sort of csrc/prims.hip): inv [n] names a row in [0, m) per entry
 * (any other value:
 * the entry is in no list).  row_ptr [m + 1], row_list [n]: the entries j with inv[j] == v are
 * row_list[row_ptr[v] .. row_ptr[v + 1]) in ASCENDING j; row_ptr[m] entries are listed, what lies behind them in
 * row_list is unspecified.  Serves a field (inv = point -> voxel row) and the interpolation gradient (inv = the neighbour
 * table nbr [8][Q] read flat: entry j = k * Q + q, so a list ascends in k and then in q).
 * ws: lidog_field_lists_ws(n, m) bytes. */
int64_t lidog_field_lists_ws(int64_t n, int64_t m);
int lidog_field_lists(const int32_t *inv, int64_t n, int64_t m, int32_t *row_ptr, int32_t *row_list, void *ws,
                      int64_t ws_bytes, void *stream);
/* Ordered segment sum [ME-mem: UNWEIGHTED_SUM / UNWEIGHTED_AVERAGE]: y[v][c] = x[l0][c] + x[l1][c] + ... over the list of
 * v in list order, float32, starting FROM the first element (not from 0); mean != 0: followed by ONE division by
 * (float)count.  An empty list gives exact zeros.  x [n_x, C]; an entry outside [0, n_x) is never used as an address.
 * TensorField.sparse() forward and the gradient of slice. */
int lidog_field_reduce(const float *x, int64_t n_x, const int32_t *row_ptr, const int32_t *row_list, int64_t m, int32_t C,
                       int32_t mean, float *y, void *stream);
/* y[p][c] = x[inv[p]][c], row_ptr != NULL: divided by (float)(row_ptr[inv[p] + 1] - row_ptr[inv[p]]).  x [m, C]; an
 * inv[p] outside [0, m) gives a row of zeros.  slice forward and the gradient of TensorField.sparse(). */
int lidog_field_gather(const float *x, const int32_t *inv, int64_t n, int64_t m, int32_t C, const int32_t *row_ptr,
                       float *y, void *stream);
/* Trilinear interpolation [ME-mem: features_at_coordinates / MinkowskiInterpolation] of F [m, C], the features of a map
 * of tensor stride s, at query [Q, 4] float32 rows (batch, x, y, z).  Per axis: lo = floor(x / s) * s,
 * t = (x - lo) / s; a lower neighbour has factor 1 - t, an upper one t.  In float32 (s a power of two: everything
 * but one subtraction is exact) the fraction is taken from the lattice point on the side of zero, whose distance is exact:
 *   x >= 0: t = (x - lo) / s, factors (1 - t, t);      x < 0: r = ((lo + s) - x) / s, factors (r, 1 - r).
 * (x - lo itself rounds below zero: -4e-14 - (-1) = 1, which would leave the point's own cell without weight.)  So one
 * factor of an axis is exact, the other rounds once, and the factor of the cell that holds the point is never 0.
 * The 8 neighbours are lo + bit * s with k = bx + 2 by + 4 bz (x fastest, the order of
 * the 2^3 kernel offsets {0, s}^3), weight w_k = f_x * f_y * f_z multiplied in that order.  nbr [8][Q]: row of F holding neighbour k of query q or -1 -- lidog_kernel_map[_bits]
 * of the floored queries (lidog_field_floor) with those 8 offsets; a neighbour in another batch index is never found.
 *   y[q][c] = 0, then y = fmaf(w_k, F[nbr[k][q]][c], y) over the neighbours that exist, ascending k.
 * Missing neighbours add nothing and nothing is renormalised; a query without neighbours gives a row of zeros.  The
 * weights are recomputed from the query, never stored.  Q < 2^28. */
int lidog_interp_fwd(const float *F, int64_t m, int32_t C, const float *query, const int32_t *nbr, int64_t n_query,
                     int32_t stride, float *y, void *stream);
/* gF[i][c] = 0, then gF = fmaf(w_k(q), gy[q][c], gF) over the pairs (k, q) with nbr[k][q] == i, ascending k and then
 * ascending q: the list of row i from lidog_field_lists(nbr, 8 Q, m).  A row nobody hits gets zeros.  No gradient with
 * respect to the coordinates. */
int lidog_interp_bwd(const float *gy, const float *query, int64_t n_query, const int32_t *row_ptr,
                     const int32_t *row_list, int64_t m, int32_t C, int32_t stride, float *gF, void *stream);

/* ---- the Raycast baseline's resampler (raycast.hip): a scan re-sampled onto a target sensor's
 * (beam, azimuth) grid; every cell keeps the nearest source point that falls into it (a point-splat range image).
 * int32 workspace (8-byte aligned) of lidog_raycast for n points and n_cells = n_beams * n_az cells */
int64_t lidog_raycast_ws(int64_t n, int64_t n_cells);
/* points [n, 3] float32; origin [3] float32 on the device (NULL: 0): q = points - origin in float32.
 * r2 = (qx qx + qy qy) + qz qz in float32, unfused; a row is dropped if r2 == 0, r2 < min2, or use_max and r2 >= max2.
 * az = atan2(qy, qx), el = atan2(qz, sqrt(qx^2 + qy^2)) in float64 from the float32 q.
 * column c = floor((az - az0) / (2 pi / n_az) + 0.5) mod n_az (non-negative); row b: edges[b] <= el < edges[b + 1],
 * edges [n_beams + 1] float64 ascending; a row outside [edges[0], edges[n_beams]) is dropped.  cell = b n_az + c.
 * The winner of a cell has the smallest r2, among equal r2 bits the smallest row (one 64-bit integer atomicMin).
 * cell_out [n] int32 (may be NULL): the cell of every row, -1 for a dropped one.  Output row k is the winner of the
 * k-th occupied cell in ascending cell order: rows_out [k] its source row, points_out [k] q of that row (snap == 0) or,
 * with r = sqrt(qx^2 + qy^2 + qz^2) in float64, float32 of ((r cos_el[b]) cos_az[c], (r cos_el[b]) sin_az[c],
 * r sin_el[b]) (snap != 0; the four float64 tables [n_beams] / [n_az] come from the host).  points_out and rows_out
 * hold min(n, n_cells) rows; m_dev [1] int32 = the number of output rows.  Nothing is read back or synchronised.
 * n, n_cells < 2^31 - 1, n_beams >= 2, |az0| <= 2 pi. */
int lidog_raycast(const float *points, int64_t n, const float *origin, const double *edges, int32_t n_beams,
                  int32_t n_az, double az0, float min2, int32_t use_max, float max2, int32_t snap,
                  const double *cos_el, const double *sin_el, const double *cos_az, const double *sin_az,
                  int32_t *cell_out, float *points_out, int32_t *rows_out, int32_t *m_dev, int32_t *ws, void *stream);

/* ---- test-time augmentation at the point level (tta.hip): the scores of one view of a loader batch,
 * gathered per kept point and accumulated.  logits [m, n_classes] float32 (n_classes 1..32, lidog_point_labels' range):
 * the view's voxel rows; inverse [k] int64: the voxel row of every kept point; acc [k, n_classes] float32.
 * With r = inverse[p] and s = the softmax of logits[r] (mode 0: the row maximum subtracted in fp32, expf, the sum in
 * class order, one division per class), logits[r] itself (mode 1) or the one-hot of its arg-max (mode 2: the first
 * maximal index, the first NaN in a row holding one, lidog_eval_confusion's rule):
 *   acc[p] = s (first != 0)   or   acc[p] = acc[p] + s (first == 0), one unfused fp32 addition per element.
 * One thread owns a row of acc and there are no atomics on it: the same bytes on every run.  A NaN or +inf logit makes
 * row p NaN in mode 0, as torch.softmax; no other row sees it.  An entry of inverse outside [0, m) sets bit 0 of err [1]
 * int32 (device, never cleared here); that row of acc is neither read nor written, and no address is formed from the
 * entry.  k == 0 launches nothing.  No allocation, synchronisation or copy inside. */
int lidog_tta_vote(const float *logits, int64_t m, int32_t n_classes, const int64_t *inverse, int64_t k, int32_t mode,
                   int32_t first, float *acc, int32_t *err, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LIDOG_AMD_H */
