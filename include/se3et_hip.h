/* se3et_hip.h -- C ABI of libse3et_hip.so: MI355X (gfx950) kernels for the SE3ET hot path.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes, no framework types; pointers are DEVICE pointers unless the name ends in _host;
 *   - tensors are dense, row-major, float32 / int64 / int32 / uint8 as typed below;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); launches are asynchronous;
 *   - outputs and workspaces are caller-allocated; the library never allocates or frees device memory
 *     and keeps no global state (one stream per process is enough, several are safe: one workspace per stream);
 *   - three workspaces begin with arrival counters of an in-kernel reduction (se3_dense_norm_fwd, se3_group_norm_stats,
 *     se3_kpconv_so3_fused's split form): they must be ZERO before their first use; every completed call leaves them zero;
 *   - return value: 0 = ok, otherwise an SE3_ERR_* code (the Python host raises RuntimeError, mirroring the
 *     TORCH_CHECK failures of the reference extension, geotransformer/extensions/common/torch_helper.h:6-35);
 *   - this file is the only declaration: the Python binding (se3et_amd/_lib.py) reads each prototype and each integer `#define SE3_*`
 *     from it.  It maps pointers, int / int32_t, int64_t, uint64_t / unsigned long long, size_t, float and double, and refuses anything
 *     else (a struct by value, an array or function-pointer parameter), so an entry point keeps to these.
 *
 * Hard limits (requests beyond them return SE3_ERR_UNSUPPORTED, nothing is truncated silently):
 *   - stacked calls take at most SE3_MAX_BATCH = 32 clouds (16 registration pairs per forward);
 *   - radius search keeps at most SE3_MAX_NEIGHBOR_LIMIT = 64 neighbours per query (the reference's limits are 36 / 38);
 *   - point_to_node_partition: point_limit <= 128 (the KITTI configuration's patch size);
 *   - attention: anchors * heads <= 32, head dimension in {8, 16, 32, 64}, channels of the relative-position kernel in {32, 64, 128, 256};
 *   - KPConv matrix-core path: input channels a multiple of 8, output channels a multiple of 32, num_support * 6 * in_channels < 2^31, the
 *     SE3ET slot tables (kanchor 6, 15 kernel points), |orbit sums| < 65504; se3_linear_f16: in_features a multiple of 32, |x| < 65504;
 *   - se3_dense_norm_fwd: in_features a power of two 32..1024, out_features 32 / 64 / 128 or a multiple of 256 up to 4096, channels per group
 *     a power of two <= 32, at most 16 segments; the f16 attention form (kv_pieces_workspace): head dimension 64.
 *
 * Each entry point names the reference interface it replaces (paths under the reference repository).
 */
#ifndef SE3ET_HIP_H_
#define SE3ET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SE3_OK 0
#define SE3_ERR_INVALID_ARG 1
#define SE3_ERR_UNSUPPORTED 2
#define SE3_ERR_LAUNCH 3
#define SE3_ERR_WORKSPACE 4

#define SE3_MAX_BATCH 32          /* clouds per stacked call = 16 registration pairs per forward (the reference always stacks 2: ref, src) */
#define SE3_MAX_NEIGHBOR_LIMIT 64 /* radius search keeps at most this many nearest neighbours */
/* Counter prefixes of the three workspaces of the conventions above, in bytes.  The prefix holds int32 arrival counters and nothing else: it
 * is zero before the first use and every completed call leaves it zero.  The rest of such a workspace (partial statistics, split partial
 * sums) has NO required content: every word of it that a call reads was written earlier in that same call. */
#define SE3_GN_COUNTER_BYTES 1024          /* se3_dense_norm_fwd, se3_group_norm_stats: 16 segments x 16 column blocks x one int32 */
#define SE3_KPCONV_SPLIT_COUNTER_BYTES 65536          /* se3_kpconv_so3_fused, split form (both kernels): one int32 per (tile or group, 32 output channels) */

/* Library / build identification. */
const char* se3_version(void);
const char* se3_last_error(void);   /* text of the last failure on the calling thread */
/* se3_log_sinkhorn_fwd: 0 = the iteration in base 2 with the previous iteration's logsumexp as the shift (default), 1 = natural base with the exact
 * maximum in every pass (the reference's order of operations) -- A/B runs. */
void se3_debug_set_sinkhorn_variant(int variant);
/* Rows of dense launches (se3_linear_stream*, se3_dense_norm_fwd, se3_dense_residual_fwd, se3_linear_f16) whose values left the headroom of the
 * row's f16-split scale -- more than 2^8 times the largest magnitude of the row's first 32 values -- or held NaN / Inf, since the last
 * reset: such values are clamped to the f16 range (finite, wrong) and counted here (events: once per row, K-step and column block).  Synchronises the device; reset != 0 zeroes the count. */
unsigned long long se3_debug_dense_saturated_rows(int reset);
/* NaN / Inf values of K / V^T (and of the equivariant cross attention's q) that the operand split of the f16 attention kernels clamped since the
 * last reset.  Finite values of any size are not clamped: a query row of one head, 8 key rows of one head and a value channel of one cloud are
 * each scaled by their own power of two before the f16 hi / lo split and the kernels take the scales out of the f32 logits / output
 * (csrc/attention.hip: x6_split_kernel).  A non-zero count says the input already held NaN / Inf. */
unsigned long long se3_debug_attention_saturated(int reset);
/* Per-launch timing of the two RPE self-attention kernels (bench.py): while enabled every launch carries its own start / stop
 * HIP event pair (hipExtLaunchKernelGGL) on the launch stream; collect_ex() waits for them, returns the count and fills the
 * durations (us) and tags (1 = relative-position logits kernel, 2 = attention kernel) in launch order, plus per record the algorithmic bytes
 * of the call (negative = equivariant call) for the logits launches (tag 1) of se3_rpe_self_attention_stack*_fwd and 0 for every
 * other launch. */
void se3_debug_kernel_timing(int enable);
int se3_debug_kernel_timing_collect_ex(float* microseconds, int* tags, double* aux, int capacity);

/* ---- A2: stack-mode radius neighbour search ---------------------------------------------------------------
 * Replaces geotransformer.ext.radius_neighbors (geotransformer/extensions/pybind.cpp:6-11,
 * cpu/radius_neighbors/radius_neighbors.cpp:5-76, radius_neighbors_cpu.cpp:3-91) together with the column
 * truncation of modules/ops/radius_search.py:25-27.
 * For every query the support points of the same batch element with d2 = (dx*dx + dy*dy) + dz*dz < radius*radius
 * (float32, unfused) are ranked by (d2, index); the first `limit` indices go to neighbors[q * limit + j], unused
 * entries are filled with ns (the total support count).  max_count (`batch` int32, DEVICE) receives per batch element the
 * max over its queries of the number of in-radius points (the caller keeps min(limit, max over the elements) columns; with
 * several registration pairs stacked, a pair's own width is the max over its two clouds).  q_lengths_host / s_lengths_host are HOST
 * arrays of `batch` int64.  limit <= SE3_MAX_NEIGHBOR_LIMIT. */
int se3_radius_neighbors(const float* q_points, int64_t nq, const float* s_points, int64_t ns,
                         const int64_t* q_lengths_host, const int64_t* s_lengths_host, int batch, float radius,
                         int limit, int64_t* neighbors, int32_t* max_count, void* stream);

/* Several pairs stacked in one table (se3et_amd/data.py): out (rows, width) = the first `width` columns of full (rows, full_width), with the
 * columns at and beyond a PAIR's own width set to -1 (pair p = rows [pair_row_ends[p-1], pair_row_ends[p]); a pair run alone keeps
 * min(limit, its largest neighbour count) columns -- the reference's collate, geotransformer/utils/data.py precompute_data_stack_mode).
 * HOST arrays, at most 64 pairs. */
int se3_neighbor_table_trim(const int64_t* full, int64_t rows, int full_width, int width, const int64_t* pair_row_ends_host,
                            const int* pair_widths_host, int num_pairs, int64_t* out, void* stream);
/* Uniform-grid variant of se3_radius_neighbors for large supports (identical results).  se3_radius_grid_build bins the
 * support cloud (cells of edge >= radius) into a caller-owned workspace; se3_radius_neighbors_grid then searches any query
 * set against it with the SAME radius.  One grid serves every search sharing support and radius (a stage's neighbour and
 * sub-sampling tables and the previous stage's up-sampling table in geotransformer/utils/data.py:48-84). */
size_t se3_radius_grid_workspace_bytes(int64_t ns, int batch);
int se3_radius_grid_build(const float* s_points, int64_t ns, const int64_t* s_lengths_host, int batch, float radius,
                          void* workspace, size_t workspace_bytes, void* stream);
int se3_radius_neighbors_grid(const float* q_points, int64_t nq, const int64_t* q_lengths_host, const int64_t* s_lengths_host,
                              int64_t ns, int batch, const void* grid_workspace, float radius, int limit, int64_t* neighbors,
                              int32_t* max_count, int max_count_is_zero, void* stream);
/* (max_count_is_zero != 0: the caller cleared max_count itself -- e.g. one fill for the counters of all searches of a pyramid -- and the
 * call does not clear it again; the search only ever raises the values.) */

/* Count-only radius search with the histogram of the counts: what the reference's neighbour-limit calibration needs
 * (geotransformer/utils/data.py:212-252: counts up to hist_n = ceil(4/3 pi (radius / voxel + 1)^3) = 180 / 607, beyond
 * SE3_MAX_NEIGHBOR_LIMIT -- no list is kept here, so no such cap applies).  For every query, count = the number of support points of the
 * same batch element with d2 = (dx*dx + dy*dy) + dz*dz < radius*radius (float32, unfused: the test of se3_radius_neighbors; with
 * q == s the point itself counts).  Cloud b adds into row slot_of_cloud_host[b] of hist (DEVICE int32 (num_slots, hist_n)):
 * hist[slot][count] += 1 when count < hist_n, dropped[slot] += 1 otherwise (DEVICE int32 (num_slots)); max_count[b] (DEVICE int32
 * (batch)) is raised to the cloud's largest, uncapped count.  All three are ACCUMULATED: the caller clears them (once for any number of
 * calls).  Integer-exact and order-independent: the same values run to run, alone or stacked.  grid_workspace: NULL (every support point of
 * the cloud is tested) or what se3_radius_grid_build made for s_points and this radius.  q_lengths_host / s_lengths_host /
 * slot_of_cloud_host are HOST arrays of `batch` entries; 1 <= hist_n <= 4096, batch <= SE3_MAX_BATCH, slots in [0, num_slots). */
int se3_radius_count_hist(const float* q_points, int64_t nq, const float* s_points, int64_t ns, const int64_t* q_lengths_host,
                          const int64_t* s_lengths_host, int batch, float radius, const void* grid_workspace, int hist_n,
                          const int* slot_of_cloud_host, int num_slots, int32_t* hist, int32_t* dropped, int32_t* max_count, void* stream);

/* ---- A2, exact ties: the reference's order of exactly tied distances (round 6; csrc/radius_ties.hip) ----------------------------------
 * The reference's row is the head of ALL in-radius matches in the order of its k-d tree walk, std::sort-ed (unstable) on the distance alone
 * (extensions/extra/nanoflann/nanoflann.hpp:857-1002,1286-1287,1348-1407; cpu/radius_neighbors/radius_neighbors_cpu.cpp:29-90): which
 * member of a group of EXACTLY equal float32 distances comes first -- and which ones a neighbour limit keeps -- depends on that walk.  The
 * searches above order such groups by index.  Their `_ties` forms additionally append the number of every row whose kept columns hold an
 * exact tie (among themselves or with the first column cut) to tie_rows (DEVICE int32, room for nq entries) behind the DEVICE counter
 * tie_count (int32, cleared by the caller; both NULL: the plain search).  For those rows se3_radius_neighbors_tie_order reproduces the
 * reference: one lane per row walks the reference's tree -- built on the HOST by se3_kdtree_build_host from a host copy of the support
 * clouds (se3_kdtree_max_bytes: size of the buffer; *used_bytes: what to upload) -- with the reference's float arithmetic, collects the
 * matches in walk order and sorts them with a restatement of libstdc++'s std::sort.  max_hits >= the search's largest max_count;
 * scratch: DEVICE, se3_radius_tie_scratch_bytes(num_tie_rows, max_hits).  Clouds without ties never pay for any of this. */
int se3_radius_neighbors_ties(const float* q_points, int64_t nq, const float* s_points, int64_t ns, const int64_t* q_lengths_host,
                              const int64_t* s_lengths_host, int batch, float radius, int limit, int64_t* neighbors, int32_t* max_count,
                              int32_t* tie_rows, int32_t* tie_count, void* stream);
int se3_radius_neighbors_grid_ties(const float* q_points, int64_t nq, const int64_t* q_lengths_host, const int64_t* s_lengths_host,
                                   int64_t ns, int batch, const void* grid_workspace, float radius, int limit, int64_t* neighbors,
                                   int32_t* max_count, int max_count_is_zero, int32_t* tie_rows, int32_t* tie_count, void* stream);
size_t se3_kdtree_max_bytes(int64_t ns, int batch);
int se3_kdtree_build_host(const float* s_points_host, int64_t ns, const int64_t* s_lengths_host, int batch, void* tree_host, size_t capacity,
                          size_t* used_bytes);
size_t se3_radius_tie_scratch_bytes(int64_t num_tie_rows, int max_hits);
int se3_radius_neighbors_tie_order(const float* q_points, int64_t nq, const float* s_points, int64_t ns, const int64_t* q_lengths_host,
                                   const int64_t* s_lengths_host, int batch, const void* tree_dev, float radius, int limit,
                                   const int32_t* tie_rows, int64_t num_tie_rows, int max_hits, void* scratch, size_t scratch_bytes,
                                   int64_t* neighbors, void* stream);
/* The code of se3_radius_neighbors_tie_order's kernel run on HOST memory (all pointers host, tree_host as built): lets the walk and the
 * std::sort restatement be checked where there is no GPU.  *overflowed: rows that did not fit max_hits (left untouched). */
int se3_debug_radius_tie_order_host(const float* q_points, int64_t nq, const float* s_points, int64_t ns, const int64_t* q_lengths,
                                    const int64_t* s_lengths, int batch, const void* tree_host, float radius, int limit,
                                    const int32_t* tie_rows, int64_t num_tie_rows, int max_hits, int64_t* neighbors, int* overflowed);
/* The std::sort restatement of that kernel against libstdc++ on the host: mode 0 the whole sort against std::sort, mode 1 its heap sort against
 * std::partial_sort(first, last, last); keys compare on their high 32 bits alone.  Returns the number of differing positions (0: identical). */
int64_t se3_debug_std_sort_host(const unsigned long long* keys, int64_t n, int mode);

/* ---- A1: stack-mode grid subsampling ----------------------------------------------------------------------
 * Replaces geotransformer.ext.grid_subsampling (pybind.cpp:13-17, cpu/grid_subsampling/grid_subsampling.cpp:5-83,
 * grid_subsampling_cpu.cpp:3-109, grid_subsampling_cpu.h:24-74).  Per batch element: voxel hash, per voxel the
 * input point closest to the voxel mean (float32 accumulation in input order, first minimum), emitted in the
 * iteration order of libstdc++'s std::unordered_map<size_t,...> (emulated on the device).
 * s_points / s_normals must hold n rows; s_lengths (DEVICE, `batch` int64) receives the per-cloud counts and the
 * sampled clouds are written back to back.  `normals` may be NULL (then s_normals is not written). */
size_t se3_grid_subsample_workspace_bytes(int64_t n, int batch);
int se3_grid_subsample(const float* points, const float* normals, int64_t n, const int64_t* lengths_host, int batch,
                       float voxel_size, float* s_points, float* s_normals, int64_t* s_lengths, void* workspace,
                       size_t workspace_bytes, void* stream);
/* The same with the clouds' sizes in DEVICE memory (the s_lengths of a previous call): a pyramid stage that follows another without a
 * host synchronisation in between (the reference subsamples stage after stage on the CPU, geotransformer/utils/data.py:33-52).  n_rows =
 * the rows of `points` that exist, an upper bound of the sum of lengths_dev (only the first sum rows are read); outputs and the
 * workspace (se3_grid_subsample_workspace_bytes(n_rows, batch)) are sized by n_rows.  Results are those of se3_grid_subsample. */
int se3_grid_subsample_dev(const float* points, const float* normals, int64_t n_rows, const int64_t* lengths_dev, int batch,
                           float voxel_size, float* s_points, float* s_normals, int64_t* s_lengths, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- E4: log-domain Sinkhorn with dustbin (LearnableLogOptimalTransport.forward) ---------------------------------
 * Replaces geotransformer/modules/sinkhorn/learnable_sinkhorn.py:13-66.  scores (batch, rows, cols) float32,
 * row_masks (batch, rows) / col_masks (batch, cols) uint8 (1 = valid point), alpha: device pointer to the learnable
 * dustbin score, inf: the finite "minus infinity" (1e12 in the reference).  out (batch, rows+1, cols+1).
 * rows, cols <= 143. */
int se3_log_sinkhorn_fwd(const float* scores, const uint8_t* row_masks, const uint8_t* col_masks, const float* alpha,
                         int batch, int rows, int cols, int iterations, float inf, float* out, void* stream);
/* Backward of se3_log_sinkhorn_fwd (training step: autograd through learnable_sinkhorn.py:13-66): grad_out (batch, rows+1, cols+1) ->
 * grad_scores (batch, rows, cols) (0 at masked entries) and grad_alpha_partial (batch): the gradient of the dustbin score per patch pair,
 * summed by the caller.  One workgroup per patch pair: the forward iterations again with every (u_t, v_t) kept in LDS, then the reverse
 * sweep.  iterations * (rows + cols + 2) * 4 bytes of LDS (<= 150 KB). */
int se3_log_sinkhorn_bwd(const float* scores, const uint8_t* row_masks, const uint8_t* col_masks, const float* alpha,
                         const float* grad_out, int batch, int rows, int cols, int iterations, float inf, float* grad_scores,
                         float* grad_alpha_partial, void* stream);

/* ---- B2: GroupNorm over stacked points, fused with "+ residual" and LeakyReLU ------------------------------------
 * Replaces GroupNormEPN (geotransformer/modules/e2pn/blocks_epn.py:684-701) and kpconv GroupNorm
 * (geotransformer/modules/kpconv/modules.py:34-51) plus the activation / shortcut add that follows them
 * (blocks_epn.py:660-664, 741-742, 838-852).  x (rows, channels): every leading dim (points, anchors) is a row; the
 * statistics of a group span all rows.  residual may be NULL.  out = act(norm(x + x_bias) * weight + bias + residual);
 * x_bias (channels, may be NULL) is the bias of the linear layer that produced x (the UnaryBlock mlp): folding it in here lets
 * that GEMM run bias-free. */
size_t se3_group_norm_workspace_bytes(int64_t rows, int channels, int groups);
int se3_group_norm_fwd(const float* x, const float* x_bias, const float* residual, const float* weight, const float* bias,
                       int64_t rows, int channels, int groups, float eps, int apply_leaky_relu, float slope, float* out,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Segmented form: segment_row_offsets_host (num_segments + 1 entries, HOST, first 0, last rows) cuts the rows into independent
 * ranges with their own statistics -- one registration pair each when several pairs share a launch (the reference normalises
 * per pair because it runs one pair per forward).  num_segments <= 16. */
int se3_group_norm_segments_fwd(const float* x, const float* x_bias, const float* residual, const float* weight,
                                const float* bias, int64_t rows, int channels, int groups,
                                const int64_t* segment_row_offsets_host, int num_segments, float eps, int apply_leaky_relu,
                                float slope, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* Backward of se3_group_norm_segments_fwd (training step: autograd of GroupNormEPN / F.leaky_relu, blocks_epn.py:684-701): grad_x (rows,
 * channels); grad_residual (rows, channels) or NULL; grad_params (num_segments, 3, channels) = every segment's contribution to (d weight,
 * d bias, d x_bias), summed over segments by the caller.  workspace: se3_group_norm_bwd_workspace_bytes(channels) bytes. */
size_t se3_group_norm_bwd_workspace_bytes(int channels);
int se3_group_norm_segments_bwd(const float* x, const float* x_bias, const float* residual, const float* weight, const float* bias,
                                const float* grad_out, int64_t rows, int channels, int groups, const int64_t* segment_row_offsets_host,
                                int num_segments, float eps, int apply_leaky_relu, float slope, float* grad_x, float* grad_residual,
                                float* grad_params, void* workspace, size_t workspace_bytes, void* stream);

/* Pending forms (inference path of the bottleneck blocks, blocks_epn.py:798-852): a GroupNorm [+ LeakyReLU] that has been reduced to its
 * affine table [segment][2][channels] (scale, shift: norm(x + x_bias) * weight + bias == x * scale + shift) but not applied -- the consumer
 * applies it while it loads x, so the normalised activation never makes a round trip through HBM.
 *   se3_group_norm_stats   the table of GroupNorm over T(x), T = a pending stage on x itself (in_affine NULL: T = identity).  Workspace:
 *                          se3_group_norm_stats_workspace_bytes(channels) bytes, ZERO before the first call (arrival counters of the
 *                          in-kernel finalize at its start; every call leaves them zero), one per stream.
 *   se3_group_norm_apply   out = lrelu_f( Tb(Ta(x)) + R ),  T.(v) = lrelu_slope(v * scale + shift);  R = residual * scale_r + shift_r
 *                          (residual_affine: the shortcut branch's own pending GroupNorm), the plain residual, or nothing.  A slope of 1
 *                          is "no LeakyReLU".  channels % 4 == 0.  blocked_layout = 1: x is (points, 6, channels) and out is written as
 *                          [point][channels / 16][anchor pair][16][2], the layout se3_kpconv_so3_fused gathers whole cache lines from
 *                          (x_blocked = 1; channels % 16 == 0).  blocked_layout = 2: out as [point][channels / 8][6 anchors][8], the
 *                          layout se3_kpconv_so3_union loads whole 192-byte row chunks from (x_chunked = 1; channels % 8 == 0).
 *   se3_dense_norm_fwd     UnaryBlockEPN (blocks_epn.py:639-665) = mlp + GroupNormEPN with both of the above folded into the GEMM
 *                          (csrc/dense_norm.hip): out = T_b(T_a(x)) W^T WITHOUT the bias (raw), affine_out = the table of
 *                          GroupNorm(out + linear_bias) computed from the accumulators.  weight_pieces: se3_linear_split_weights_f16.
 *                          in_features a power of two 32..1024; out_features 32, 64, 128 or a multiple of 256; f16 hi/lo split arithmetic
 *                          (f32 accuracy, |T(x)| < 65504); out_features / groups a power of two <= 32.  Workspace:
 *                          se3_dense_norm_workspace_bytes(groups) bytes, ZERO before the first call (it starts with the arrival counters
 *                          of the in-kernel finalize; every call leaves them zero), one per stream.  out == NULL: statistics only (the
 *                          product is reduced to affine_out and never stored). */
size_t se3_group_norm_stats_workspace_bytes(int channels);
int se3_group_norm_stats(const float* x, const float* in_affine, float in_slope, const float* x_bias, const float* weight, const float* bias,
                         int64_t rows, int channels, int groups, const int64_t* segment_row_offsets_host, int num_segments, float eps,
                         float* affine_out, void* workspace, size_t workspace_bytes, void* stream);
int se3_group_norm_apply(const float* x, const float* affine_a, float slope_a, const float* affine_b, float slope_b, const float* residual,
                         const float* residual_affine, float final_slope, int64_t rows, int channels,
                         const int64_t* segment_row_offsets_host, int num_segments, int blocked_layout, float* out, void* stream);
/* ... the same with the largest |out| of the call atomicMax-ed (as a bit pattern) into *amax_out (blocked layouts 1 / 2 only; the caller zeroes
 * the word): se3_kpconv_so3_fused_scaled / se3_kpconv_so3_union scale their input by a power of two from it before the f16 split. */
int se3_group_norm_apply_amax(const float* x, const float* affine_a, float slope_a, const float* affine_b, float slope_b, const float* residual,
                              const float* residual_affine, float final_slope, int64_t rows, int channels,
                              const int64_t* segment_row_offsets_host, int num_segments, int blocked_layout, float* out, float* amax_out,
                              void* stream);
size_t se3_dense_norm_workspace_bytes(int groups);
int se3_dense_norm_fwd(const float* x, int64_t rows, int in_features, const float* in_affine_a, float in_slope_a, const float* in_affine_b,
                       float in_slope_b, const void* weight_pieces, int out_features, const float* linear_bias, const float* norm_weight,
                       const float* norm_bias, int groups, float eps, const int64_t* segment_row_offsets_host, int num_segments, float* out,
                       float* affine_out, void* workspace, size_t workspace_bytes, void* stream);
/* Round 4 -- the tail of ResnetBottleneckBlockEPN (blocks_epn.py:838-852: `x = self.unary2(x); return leaky_relu(x + shortcut)`) without the
 * raw output of the expanding layers ever reaching HBM.  (1) se3_dense_norm_fwd with out == NULL: the GEMM of unary2 (and of skip_conv) is run
 * for its GroupNorm statistics only -> affine table.  (2) se3_dense_residual_fwd runs the GEMM again and writes
 *     out = lrelu( (T_b(T_a(x)) W^T) * scale + shift + R, final_slope ),   (scale, shift) = affine[segment] of step (1),
 * R = residual (rows, out_features), or the shortcut layer (x2 W2^T) * scale2 + shift2 (x2 (rows, in_features2) concrete, weight_pieces2,
 * affine2 from its own step (1); its norm weight must be non-zero: the two products share one accumulator set through the ratio
 * scale / scale2), or nothing (both NULL).  Same shape limits as se3_dense_norm_fwd; no workspace. */
int se3_dense_residual_fwd(const float* x, int64_t rows, int in_features, const float* in_affine_a, float in_slope_a, const float* in_affine_b,
                           float in_slope_b, const void* weight_pieces, const float* affine, const float* x2, int in_features2,
                           const void* weight_pieces2, const float* affine2, const float* residual, int out_features, float final_slope,
                           const int64_t* segment_row_offsets_host, int num_segments, float* out, void* stream);
/* Round 4 -- the streaming kernel as a plain dense layer for ANY row count and row strides: out = act(x W^T + bias), weight_pieces from
 * se3_linear_split_weights_f16 (in_features % 32 == 0, |x| < 65504, f32 accuracy).  Replaces the library GEMMs of the transformer's nn.Linear
 * layers (rpe_transformer.py:56-73,134-165; vanilla_transformer.py:22-37; output_layer.py:7-47; geotransformer.py:213-317).
 * se3_linear_stream_transposed stores the product of every block of `block_rows` rows transposed, out_t (rows / block_rows, out_features, ld):
 * the value projection in the attention kernels' operand layout V^T (A, C, Rp) straight from the packed rows (A, R, C). */
int se3_linear_stream(const float* x, int64_t rows, int in_features, int64_t x_row_stride, const void* weight_pieces, const float* bias,
                      int out_features, int apply_relu, float* out, int64_t out_row_stride, void* stream);
int se3_linear_stream_transposed(const float* x, int64_t rows, int in_features, int64_t x_row_stride, const void* weight_pieces,
                                 const float* bias, int out_features, int block_rows, float* out_t, int64_t ld, void* stream);

/* ---- D6: LayerNorm(hidden + residual) ---------------------------------------------------------------------------
 * Replaces the residual + nn.LayerNorm tails of geotransformer/modules/transformer/rpe_transformer.py:163-164,
 * vanilla_transformer.py:910-911 and output_layer.py:21,46.  hidden (rows, channels); residual (residual_rows,
 * channels) is broadcast with row % residual_rows (anchor broadcast).  hidden_bias (channels, may be NULL) is added to hidden
 * first: the bias of the output / FFN linear that produced it. */
int se3_add_layer_norm_fwd(const float* hidden, const float* hidden_bias, const float* residual, const float* weight,
                           const float* bias, int64_t rows, int64_t residual_rows, int channels, float eps, float* out,
                           void* stream);
/* Backward (training step: autograd through the residual + nn.LayerNorm tails): grad_hidden (rows, channels), which is also the gradient
 * of the residual before its anchor broadcast is summed; grad_params (3, channels) = (d weight, d bias, d hidden_bias), zero-initialised
 * by the caller and accumulated with float atomics. */
int se3_add_layer_norm_bwd(const float* hidden, const float* hidden_bias, const float* residual, const float* weight,
                           const float* grad_out, int64_t rows, int64_t residual_rows, int channels, float eps, float* grad_hidden,
                           float* grad_params, void* stream);

/* ---- B2 / D: dense layers on the f16 matrix cores at f32 accuracy (csrc/linear_f16.hip) ------------------------------------------------------
 * y = x W^T [+ bias] [ReLU]: UnaryBlockEPN.mlp / LastUnaryBlockEPN.mlp (blocks_epn.py:639-665,798-852), the kpconv UnaryBlock
 * (modules/kpconv/modules.py:54-93) and the transformer's nn.Linear layers (rpe_transformer.py:56-73, vanilla_transformer.py:22-37,
 * output_layer.py).  weight (out_features, in_features) row-major f32, in_features a multiple of 32; se3_linear_split_weights_f16 turns it
 * into f16 hi / lo MFMA fragments scaled by a power of two (`pieces`: se3_linear_weight_pieces_bytes bytes, once per weight version);
 * se3_linear_f16: x (rows, in_features) with row stride x_row_stride floats (16-byte aligned rows), out (rows, out_features) with row
 * stride out_row_stride; three products hi hi + hi lo + lo hi in f32 (2^-22 per term).  Range |x| < 65504. */
size_t se3_linear_weight_pieces_bytes(int out_features, int in_features);
int se3_linear_split_weights_f16(const float* weight, int out_features, int in_features, void* pieces, void* stream);
int se3_linear_f16(const float* x, int64_t rows, int in_features, int64_t x_row_stride, const void* weight_pieces, const float* bias,
                   int out_features, int apply_relu, float* out, int64_t out_row_stride, void* stream);

/* ---- B2/B3: padded row gather and neighbour max pooling ------------------------------------------------------------
 * Replace nearest_upsample (geotransformer/modules/kpconv/functional.py:6-22), the zero-padded patch gathers of
 * experiments/se3ete.3dmatch/model.py:108-111,190-193 and max_pool (geotransformer/modules/e2pn/blocks.py:93-110).
 * x (n, width); idx entries equal to n address an all-zero row. */
int se3_gather_rows_padded(const float* x, const int64_t* idx, int64_t n, int64_t m, int64_t width, float* out,
                           void* stream);
int se3_neighbor_max_pool(const float* x, const int64_t* idx, int64_t n, int64_t m, int nn, int64_t width, float* out,
                          void* stream);
/* Backward of se3_neighbor_max_pool (autograd of torch.max over the gathered rows, blocks.py:93-110): dx (n, width) += dout of every row
 * at its arg-max neighbour (first in table order on ties; nothing for the zero row of padded entries).  dx zero-initialised by the caller. */
int se3_neighbor_max_pool_bwd(const float* x, const int64_t* idx, const float* dout, int64_t n, int64_t m, int nn, int64_t width,
                              float* dx, void* stream);
/* Maximum over the anchor axis (InvOutBlockEPN, geotransformer/modules/e2pn/blocks_epn.py:908-926; the anchor 'amax' between
 * equivariant and invariant transformer blocks, transformer/conditional_transformer.py:282-283,299-302):
 * out[r, c] = max_a x[a * anchor_stride + r * row_stride + c], out (rows, channels) contiguous.  Serves (A, R, C)
 * (anchor_stride = R*C, row_stride = C) and (R, A, C) (anchor_stride = C, row_stride = A*C).  num_anchors = 6, channels % 4 == 0. */
int se3_anchor_max(const float* x, int num_anchors, int64_t rows, int channels, int64_t anchor_stride, int64_t row_stride,
                   float* out, void* stream);

/* ---- B1: E2PN anchor-group KPConv (KPConvInterSO3), neighbour-gather stage ---------------------------------------
 * Replaces feat_gather_by_perm + the (k, a) part of the weight contraction of
 * geotransformer/modules/e2pn/blocks_epn.py:334-390,454-546.  x (num_support, 6, Cin), idx (num_queries, NN) int64
 * padded with num_support; kernel_points_host (15, 3) float32, kidx_host (15, 6) int64 [k][r] -> weight slot,
 * ridx_host (6, 6) int64 [a][r] -> anchor slot: HOST arrays (tiny constant tables).  Writes
 * G (num_queries, 6[r], 6[s], 6[t], Cin) so that out[(p, r), :] = G[(p, r), (s, t, c)] @ weights[(s, t, c), :]. */
int se3_kpconv_so3_gather(const float* q_pts, const float* s_pts, const int64_t* idx, const float* x,
                          const float* kernel_points_host, const int64_t* kidx_host, const int64_t* ridx_host, float sigma,
                          int64_t num_queries, int64_t num_support, int num_neighbors, int in_channels, float* G,
                          void* stream);
/* Backward of that stage with respect to x (training step, experiments/se3ete.3dmatch: autograd through blocks_epn.py:454-546): with
 * dG = dout @ weights^T (num_queries * 6, 36 Cin) from a library GEMM, dx (num_support, 6, Cin) += gather^T(dG).  dx zero-initialised by
 * the caller; accumulated with float atomics (summation order = arrival order).  The weight gradient is the library GEMM G^T @ dout. */
int se3_kpconv_so3_gather_bwd(const float* q_pts, const float* s_pts, const int64_t* idx, const float* dG,
                              const float* kernel_points_host, const int64_t* kidx_host, const int64_t* ridx_host, float sigma,
                              int64_t num_queries, int64_t num_support, int num_neighbors, int in_channels, float* dx, void* stream);
/* The same with an ORDER-INDEPENDENT sum (round 5): the contributions are added as 64-bit fixed-point integers at a scale taken from max |dG|
 * (max_abs_dG: DEVICE word, any upper bound), so two runs are bit-identical; dx_fixed (num_support, 6, in_channels) int64, ZERO on entry;
 * se3_kpconv_fixed_to_float(dx_fixed, num_support * 6 * in_channels, max_abs_dG, num_queries, dx) converts the sums to float32. */
int se3_kpconv_so3_gather_bwd_fixed(const float* q_pts, const float* s_pts, const int64_t* idx, const float* dG,
                                    const float* kernel_points_host, const int64_t* kidx_host, const int64_t* ridx_host, float sigma,
                                    int64_t num_queries, int64_t num_support, int num_neighbors, int in_channels, const float* max_abs_dG,
                                    long long* dx_fixed, void* stream);
int se3_kpconv_fixed_to_float(const long long* dx_fixed, int64_t count, const float* max_abs_dG, int64_t num_queries, float* dx, void* stream);
/* Order-independent (bit-identical) forms of the other scatter-adds of the training step, the same 64-bit fixed-point scheme (csrc/common.h:
 * se3_fixed_scale_exp): se3_fixed_to_float(fixed, count, bound, terms, growth, out) converts sums accumulated with the same (bound, terms, growth).
 *   se3_neighbor_max_pool_bwd_fixed   backward of se3_neighbor_max_pool (terms = rows of idx, growth 0)
 *   se3_scatter_add_rows_fixed        backward of se3_gather_rows_padded (terms = gathered rows, growth 0)
 *   se3_add_layer_norm_bwd_partials   backward of se3_add_layer_norm_fwd with per-workgroup partial parameter sums
 *                                     (se3_add_layer_norm_bwd_blocks(rows), 3, channels) that the caller adds in order */
int se3_fixed_to_float(const long long* fixed, int64_t count, const float* bound, int64_t terms, int growth, float* out, void* stream);
int se3_neighbor_max_pool_bwd_fixed(const float* x, const int64_t* idx, const float* dout, int64_t n, int64_t m, int nn, int64_t width,
                                    const float* max_abs_dout, long long* dx_fixed, void* stream);
int se3_scatter_add_rows_fixed(const float* g, const int64_t* idx, int64_t n, int64_t m, int64_t width, const float* max_abs_g,
                               long long* dx_fixed, void* stream);
int64_t se3_add_layer_norm_bwd_blocks(int64_t rows);
int se3_add_layer_norm_bwd_partials(const float* hidden, const float* hidden_bias, const float* residual, const float* weight,
                                    const float* grad_out, int64_t rows, int64_t residual_rows, int channels, float eps, float* grad_hidden,
                                    float* grad_params_partials, void* stream);

/* Matrix-core form of the same convolution (csrc/kpconv_sums.h, csrc/kpconv_mfma.hip; input channels a multiple of 8, output channels a
 * multiple of 32, SE3ET slot tables compiled in; num_support * 6 * in_channels < 2^31).  Over all (weight slot s, output anchor r) only 16
 * distinct kernel-point sums occur (6 vertices, centre, 3 equators, 6 face quadruples): the "orbits".
 *   se3_kpconv_neighbor_table: per query point its valid neighbours (compacted; shadow / padded entries carry weight 0 in the reference,
 *     blocks_epn.py:471,377) and their 16 orbit weights hw[o] = sum_{k in o} max(0, 1 - |s - q - kp_k| / sigma) (blocks_epn.py:520-533);
 *     kernel_points_dev (15, 3) DEVICE; table: se3_kpconv_neighbor_table_bytes bytes.  Depends on the geometry only: layers that share
 *     (q_pts, s_pts, idx, kernel points, sigma) may share it.
 *   se3_kpconv_split_weights_f16: weights (36 Cin, Cout) -- KPConvInterSO3.weights (6, 6, Cin, Cout) flattened, blocks_epn.py:105-106 -- as f16
 *     hi / lo MFMA fragments scaled by a power of two (`pieces`: se3_kpconv_weight_pieces_bytes bytes incl. a 256-byte header with 1 / scale).
 *   se3_kpconv_so3_fused: KPConvInterSO3.forward (blocks_epn.py:454-546) in ONE kernel: producer waves form the orbit sums
 *     H[p, o, a, c] = sum_n hw[p, n, o] x[idx[p, n], a, c] of a 16-point tile on the f32 matrix cores and leave them, split into f16 hi + lo
 *     pieces, in LDS; consumer waves multiply them with v_mfma_f32_32x32x16_f16 (hi hi + hi lo + lo hi in f32: 2^-22 per term), reading the
 *     slot sums of blocks_epn.py:503-546 in place: out (P, 6, Cout).  The operand never exists in HBM.  With few tiles (one pair per
 *     forward, the coarse stages) the input channels of a tile are split over several workgroups whose partial outputs the last one to
 *     arrive adds in a fixed order: split_workspace = se3_kpconv_fused_split_workspace_bytes bytes (0: this shape does not split), ZERO
 *     before the first call (arrival counters at its start; every call leaves them zero), one per stream; NULL = never split.
 *     x_blocked = 1: x in the blocked layout written by se3_group_norm_apply(blocked_layout = 1) (in_channels % 16 == 0).
 *   se3_kpconv_so3_gather_sums + se3_kpconv_so3_contract_f16: the same two stages as two launches, H as tile images
 *     [Cin / 8][ceil(P / 16)][piece][point][97 x 16 B] in HBM (se3_kpconv_sums_bytes bytes).
 * Range: |H| < 65504 (f16 hi piece); values below 2^-3 keep an absolute error of 2^-25. */
size_t se3_kpconv_neighbor_table_bytes(int64_t num_queries, int num_neighbors);
int se3_kpconv_neighbor_table(const float* q_pts, const float* s_pts, const int64_t* idx, const float* kernel_points_dev, float sigma,
                              int64_t num_queries, int64_t num_support, int num_neighbors, void* table, size_t table_bytes, void* stream);
size_t se3_kpconv_weight_pieces_bytes(int in_channels, int out_channels);
int se3_kpconv_split_weights_f16(const float* weights, int in_channels, int out_channels, void* pieces, void* stream);
size_t se3_kpconv_fused_split_workspace_bytes(int64_t num_queries, int in_channels, int out_channels);
int se3_kpconv_so3_fused(const float* x, const void* table, int64_t num_queries, int64_t num_support, int num_neighbors, int in_channels,
                         int out_channels, const void* weight_pieces, float* out, void* split_workspace, size_t split_workspace_bytes,
                         int x_blocked, void* stream);
/* ... x_amax: DEVICE word holding the largest |x| (se3_group_norm_apply_amax) or NULL.  Outside [2^-4, 2^7) the features are scaled by the power
 * of two that brings it to [2^6, 2^7) before their f16 split and the output is scaled back: no magnitude window on x (NULL: |H| < 65504 as before). */
int se3_kpconv_so3_fused_scaled(const float* x, const void* table, int64_t num_queries, int64_t num_support, int num_neighbors, int in_channels,
                                int out_channels, const void* weight_pieces, float* out, void* split_workspace, size_t split_workspace_bytes,
                                int x_blocked, const float* x_amax, void* stream);
/* Union-staged form of se3_kpconv_so3_fused (csrc/kpconv_union.hip, round 5): a workgroup owns 16 points that are spatial neighbours, reads
 * the DISTINCT support rows of their neighbour lists once (whole rows, 16 B per lane) and forms every point's orbit sums as a product of
 * its orbit weights, scattered over the tile's row list, with the shared rows.  Tile membership only: no tensor is reordered.
 *   se3_point_order_keys / _place: a spatial order of one stage's stacked points: key = cloud << 32 | 30-bit Morton code of floor(p / cell);
 *     the caller sorts the keys (any stable sort; torch.sort) and _place writes `order` (se3_point_order_groups(lengths) * 16 int32: the point
 *     at every position, -1 = padding; every cloud starts a new group of 16, so a cloud's groups do not depend on what else is stacked).
 *   se3_kpconv_union_plan: per group of 16 order positions the distinct rows of the neighbour lists (se3_kpconv_neighbor_table) sorted by row
 *     number and every list slot's index into them; groups with more than 128 distinct rows are cut into halves (sub-tiles) until they
 *     fit.  plan: se3_kpconv_union_plan_bytes bytes; a function of (order, table) only.
 *   se3_kpconv_so3_union: KPConvInterSO3.forward (blocks_epn.py:454-546) as se3_kpconv_so3_fused; x_chunked = 1: x in the layout written by
 *     se3_group_norm_apply(blocked_layout = 2).  split_workspace: se3_kpconv_union_split_workspace_bytes bytes, same contract as the fused form.
 *     Summation order inside a point's neighbourhood: ascending support row; results agree with se3_kpconv_so3_fused to f32 rounding. */
int64_t se3_point_order_groups(const int64_t* cloud_lengths_host, int num_clouds);
/* (the same order in one launch, one workgroup per cloud sorting in LDS: clouds of at most 8192 points, SE3_ERR_UNSUPPORTED beyond) */
int se3_point_order(const float* points, int64_t num_points, const int64_t* cloud_lengths_host, int num_clouds, float cell, int32_t* order,
                   void* stream);
/* (up to four stages of one pyramid in one launch: arrays of the single-stage arguments) */
int se3_point_order_stages(const float* const* points, const int64_t* num_points, const int64_t* const* cloud_lengths_host, const int* num_clouds,
                           const float* cell, int32_t* const* order, int num_stages, void* stream);
int se3_point_order_keys(const float* points, int64_t num_points, const int64_t* cloud_lengths_host, int num_clouds, float cell, int64_t* keys,
                         void* stream);
int se3_point_order_place(const int64_t* sorted_keys, const int64_t* sorted_index, int64_t num_points, const int64_t* cloud_lengths_host,
                          int num_clouds, int32_t* order, void* stream);
size_t se3_kpconv_union_plan_bytes(int64_t num_groups, int num_neighbors);
int se3_kpconv_union_plan(const void* table, int64_t num_queries, int num_neighbors, const int32_t* order, int64_t num_groups, void* plan,
                          size_t plan_bytes, void* stream);
size_t se3_kpconv_union_split_workspace_bytes(int64_t num_groups, int in_channels, int out_channels);
int se3_kpconv_so3_union(const float* x, const void* table, const void* plan, int64_t num_groups, int64_t num_queries, int64_t num_support,
                         int num_neighbors, int in_channels, int out_channels, const void* weight_pieces, float* out, void* split_workspace,
                         size_t split_workspace_bytes, int x_chunked, const float* x_amax, void* stream);
size_t se3_kpconv_sums_bytes(int64_t num_queries, int in_channels);
int se3_kpconv_so3_gather_sums(const float* x, const void* table, int64_t num_queries, int64_t num_support, int num_neighbors,
                               int in_channels, void* sums, void* stream);
int se3_kpconv_so3_contract_f16(const void* sums, const void* weight_pieces, int64_t num_queries, int in_channels, int out_channels,
                                float* out, void* stream);

/* ---- D1/D2: RPE self attention (RPEMultiHeadAttention.forward) ------------------------------------------------------
 * Replaces geotransformer/modules/transformer/rpe_transformer.py:39-131 in two launches.
 * (1) se3_rpe_bias_fwd streams the (N, M, C) geometric embedding once and writes the relative-position logits
 *     bias[a*H+h, n, m] = qp[a, n, h, :] . emb[n, m, :] (+ qe[a, n, h, :] . eq_emb[a, n, m, :]), where qp = W_p^T q (C values
 *     per head) and qe = W_eq^T q (4 values per head) are the position projections folded onto the query side
 *     (anchors * heads <= 32).  qp and qe are column blocks of one projection output: element (a, n, h, c) of qp lives at
 *     qp[a * anchor_stride + n * row_stride + h * C + c], element (a, n, h, e) of qe at qe[a * anchor_stride + n * row_stride
 *     + 4 h + e] (strides in floats, multiples of 4).
 *     eq_emb (A, N, M, 4) and qe are NULL for non-equivariant layers.  bias has row stride bias_row_stride >= M.
 * (2) se3_attention_fwd: out[a, n, h*d:(h+1)*d] = softmax_m((q_a[n,h] . k_a[m,h] + bias[a*H+h, n, m]) * scale) v_a[m, h].
 *     q/k are (anchors, rows, row_stride >= C) -- column blocks of a wider projection are fine --, out (anchors, N, C);
 *     the values are passed TRANSPOSED, vt (anchors, C, v_row_stride) with v_row_stride a multiple of 4 >= ceil32(M)
 *     (entries beyond M must be finite), so that the P.V operand loads are contiguous; bias_row_stride likewise.  Anchor strides are in floats (0 = the same tensor for every anchor, which is how plain cross attention
 *     vanilla_transformer.py:39-85 with per-anchor values is expressed); bias may be NULL.  C / H in {8, 16, 32, 64}; C in {32,64,128,256} for (1). */
int se3_rpe_bias_fwd(const float* qp, const float* qe, int row_stride, int64_t anchor_stride, const float* emb,
                     const float* eq_emb, int N, int M, int C, int AH, int H, int bias_row_stride, float* bias, void* stream);
int se3_attention_fwd(const float* q, const float* k, const float* vt, const float* bias, int num_anchors, int N, int M, int C,
                      int H, int q_row_stride, int k_row_stride, int v_row_stride, int64_t q_anchor_stride,
                      int64_t k_anchor_stride, int64_t v_anchor_stride, int64_t out_anchor_stride, int bias_row_stride,
                      float scale, float* out, void* stream);

/* Stack mode of the two calls above (the reference runs the same RPETransformerLayer on the ref and the src cloud one after
 * the other, rpe_conditional_transformer.py:49-53; here the clouds of a pair share ONE launch per kernel).  The clouds' rows
 * are packed in one (anchors, rows, row_stride) projection: cloud c owns the query rows q_starts[c] .. + q_lengths[c] and the
 * key rows k_starts[c] .. + k_lengths[c] (self attention: the same rows; k_starts multiples of 32 because the transposed
 * values vt (anchors, C, v_row_stride) are addressed by key column).  emb_ptrs[c] -> (N_c, M_c, C), eq_ptrs[c] -> (A, N_c, M_c, 4)
 * or NULL (all clouds alike).  The logits of cloud c are the block bias + bias_offsets[c] of shape (A*H, N_c, ceil32(M_c)).
 * All arrays are HOST arrays of num_clouds (<= 16) entries.  out is (anchors, rows, C) in the packed row order. */
int se3_rpe_bias_stack_fwd(const float* qp, const float* qe, int row_stride, int64_t anchor_stride,
                           const float* const* emb_ptrs, const float* const* eq_ptrs, const int64_t* q_starts,
                           const int64_t* q_lengths, const int64_t* k_lengths, const int64_t* bias_offsets, int num_clouds,
                           int C, int AH, int H, float* bias, void* stream);
int se3_attention_stack_fwd(const float* q, const float* k, const float* vt, const float* bias, const int64_t* q_starts,
                            const int64_t* q_lengths, const int64_t* k_starts, const int64_t* k_lengths,
                            const int64_t* bias_offsets, int num_clouds, int num_anchors, int C, int H, int q_row_stride,
                            int k_row_stride, int v_row_stride, int64_t q_anchor_stride, int64_t k_anchor_stride,
                            int64_t v_anchor_stride, int64_t out_anchor_stride, float scale, float* out, void* kv_pieces_workspace,
                            size_t kv_pieces_bytes, void* stream);
/* kv_pieces_workspace (may be NULL): se3_attention_kv_pieces_bytes(anchors, max_c(k_starts[c] + k_lengths[c]), C, v_row_stride) bytes, 16-byte
 * aligned, one per stream.  With it (head dimension 64, k_starts multiples of 16, v_row_stride a multiple of 16) k and vt are split once
 * into f16 hi / lo pieces and both products run on the f16 matrix cores (three products, f32 accumulation: the error of an f32 product);
 * without it, or for other shapes, on the f32 matrix cores. */
size_t se3_attention_kv_pieces_bytes(int num_anchors, int64_t key_rows, int C, int v_row_stride);

/* The whole stack-mode RPE self-attention call (the reference's RPEMultiHeadAttention.forward up to the output projection,
 * rpe_transformer.py:39-131, for all clouds of the pair): se3_rpe_bias_stack_fwd into `logits_workspace` followed by
 * se3_attention_stack_fwd, launched back to back.  Queries and keys of cloud c are the packed rows starts[c] .. + lengths[c]
 * (starts multiples of 4, ceil32(lengths[c]) value columns readable); logits_workspace holds
 * sum_c A*H * lengths[c] * ceil32(lengths[c]) floats. */
int se3_rpe_self_attention_stack_fwd(const float* q, const float* k, const float* vt, const float* qp, const float* qe,
                                     int row_stride, int64_t anchor_stride, int v_row_stride, int64_t v_anchor_stride,
                                     const float* const* emb_ptrs, const float* const* eq_ptrs, const int64_t* starts,
                                     const int64_t* lengths, int num_clouds, int num_anchors, int C, int H,
                                     float* logits_workspace, int64_t out_anchor_stride, float* out, void* kv_pieces_workspace,
                                     size_t kv_pieces_bytes, void* stream);

/* bf16 geometric embedding (BASELINE.json configs[2]: "bf16 attention"): the same two calls with emb_ptrs[c] -> (N_c, M_c, C)
 * bfloat16 (16-byte aligned, C a multiple of 32), which halves the N*M*C term of the call's HBM bytes.  Queries, keys, values,
 * the equivariant embedding, the logits and the output stay float32; the folded queries are split into bf16 hi + lo parts
 * inside the kernel, so the only rounding is the stored embedding itself (2^-9 relative per element). */
int se3_rpe_bias_stack_bf16_fwd(const float* qp, const float* qe, int row_stride, int64_t anchor_stride,
                                const uint16_t* const* emb_ptrs, const float* const* eq_ptrs, const int64_t* q_starts,
                                const int64_t* q_lengths, const int64_t* k_lengths, const int64_t* bias_offsets, int num_clouds,
                                int C, int AH, int H, float* bias, void* stream);
int se3_rpe_self_attention_stack_bf16_fwd(const float* q, const float* k, const float* vt, const float* qp, const float* qe,
                                          int row_stride, int64_t anchor_stride, int v_row_stride, int64_t v_anchor_stride,
                                          const uint16_t* const* emb_ptrs, const float* const* eq_ptrs, const int64_t* starts,
                                          const int64_t* lengths, int num_clouds, int num_anchors, int C, int H,
                                          float* logits_workspace, int64_t out_anchor_stride, float* out, void* kv_pieces_workspace,
                                          size_t kv_pieces_bytes, void* stream);

/* ---- D4/D5: anchor-equivariant cross attention (MultiHeadAttentionEQ, 'a_soft' / 'r_soft') ----------------------------
 * Replaces geotransformer/modules/transformer/vanilla_transformer.py:247-476,506-577,751-870.  q (A, N, C), k/v (A, M, C).
 * se3_cross_eq_stats writes partial[(a*A+e) * P + i] whose sum over i is sum_{n,m} (mean_h q_a.k_e * scale)^2
 * (*num_partials_per_pair = P = ceil(N/32)); the caller turns g = sum / (N M) into the (A, A) mixing weights `mix`
 * (a_soft: g / sum_e g; r_soft: the 24 rotation weights collapsed onto anchor pairs) and se3_cross_eq_apply computes
 * out[a] = sum_e mix[a, e] softmax_m(q_a.k_e * scale) v_e (vt: transposed key-padded values (A, C, key_stride)).
 * se3_cross_eq_stats and se3_cross_eq_apply run the f32 kernels of se3_cross_eq_stack_fwd on one pair (a wave per key anchor for
 * A <= 6). */
int se3_cross_eq_stats(const float* q, const float* k, int A, int N, int M, int C, int H, float scale, float* partial,
                       int* num_partials_per_pair, void* stream);
/* mode 0 = a_soft (weights: A*A values = mix), mode 1 = r_soft (weights: num_rotations values; trace_idx (R, A) int64) */
int se3_cross_eq_mix(const float* partial, int num_partials_per_pair, int A, int N, int M, int mode, const int64_t* trace_idx,
                     int num_rotations, float* mix, float* weights, void* stream);
int se3_cross_eq_apply(const float* q, const float* k, const float* vt, const float* mix, int A, int N, int M, int C, int H,
                       int key_stride, float scale, float* out, void* stream);
/* Stack mode: statistics, mixing weights and weighted attention of ALL pairs of a batch in three launches.  q (A, Rq, C) and
 * k (A, Rk, C) hold the packed rows of all pairs (pair p: query rows q_starts[p] .. + q_lengths[p], key rows k_starts[p] .. +
 * k_lengths[p]; row stride C, anchor strides given), vt (A, C, v_row_stride) the transposed values addressed by key column
 * (k_starts multiples of 4, ceil32(k_lengths[p]) columns readable).  partial_workspace: num_pairs * A*A * max_p ceil(N_p/32)
 * floats; with sums_given != 0 its first num_pairs * A*A floats already hold sum_{n,m} (mean_h S[a,e,h,n,m])^2 of every
 * (pair, a, e) and the statistics launch is skipped (mean_h S = (scale/H) q_a[n].k_e[m] over all C channels, so the caller can
 * get the sums from two Gram matrices per pair: (scale/H)^2 <Q_a^T Q_a, K_e^T K_e>_F -- 3.5x fewer flops, library GEMMs); mix (num_pairs, A, A); weights (num_pairs, A*A) for mode 0 / (num_pairs, num_rotations) for mode 1; out (A, Rq, C) in
 * the packing of q.  num_pairs <= 16. */
/* Gram matrices of packed rows: out (num_anchors, num_pairs, C, C) = X^T X over the rows [starts[p], starts[p] + lengths[p]) of x[a]
 * (x (num_anchors, rows, C), row stride C, anchor_stride floats between anchors); C = 128 or 256, HOST arrays, at most 16 pairs. */
int se3_gram_stack(const float* x, int num_anchors, int C, int64_t anchor_stride, const int64_t* starts, const int64_t* lengths, int num_pairs,
                   float* out, void* stream);
/* The sums_given statistics of the stack mode from per-pair Gram matrices: out (num_pairs, A, A) = factor * <gq[a, p], gk[e, p]>_F, gq / gk
 * (A, num_pairs, elements) contiguous (elements = C * C, a multiple of 4). */
int se3_gram_frobenius(const float* gq, const float* gk, int A, int num_pairs, int64_t elements, float factor, float* out, void* stream);
int se3_cross_eq_stack_fwd(const float* q, const float* k, const float* vt, const int64_t* q_starts, const int64_t* q_lengths,
                           const int64_t* k_starts, const int64_t* k_lengths, int num_pairs, int A, int C, int H,
                           int64_t q_anchor_stride, int64_t k_anchor_stride, int v_row_stride, int64_t v_anchor_stride, int mode,
                           const int64_t* trace_idx, int num_rotations, int sums_given, float* partial_workspace, float* mix,
                           float* weights, float* out, void* stream);
/* The same on the f16 matrix cores at f32 accuracy (head dimension 64, A <= 6, key starts and v_row_stride multiples of 16, sums_given
 * != 0; anything else is forwarded to se3_cross_eq_stack_fwd): q, k and vt are split once into f16 hi / lo pieces in `workspace`
 * (se3_cross_eq_x6_workspace_bytes bytes, 16-byte aligned; q (A, q_rows, C), k (A, k_rows, C) packed rows) and the three piece products
 * above 2^-22 are accumulated in f32.
 * out (A, q_rows, out_groups * C) with anchor stride out_anchor_stride floats: out_groups = 1 is the result itself (out_anchor_stride =
 * q_anchor_stride for an output in the layout of q).  out_groups = G > 1 (a divisor of A; few pairs, where one workgroup per (query tile,
 * head, anchor) leaves most of the chip idle): workgroup group g sums the key anchors [g, g + 1) * A / G and writes its partial result at
 * channel offset g * C; the result is the sum of the G channel blocks, which the caller gets for free from the output projection that
 * follows by stacking its weights G times along the input dimension.  (G > 1 is refused when the call has to take the f32 kernels.) */
size_t se3_cross_eq_x6_workspace_bytes(int A, int64_t q_rows, int64_t k_rows, int C, int v_row_stride);
int se3_cross_eq_stack_x6_fwd(const float* q, const float* k, const float* vt, const int64_t* q_starts, const int64_t* q_lengths,
                              const int64_t* k_starts, const int64_t* k_lengths, int num_pairs, int A, int C, int H, int64_t q_rows,
                              int64_t k_rows, int64_t q_anchor_stride, int64_t k_anchor_stride, int v_row_stride,
                              int64_t v_anchor_stride, int mode, const int64_t* trace_idx, int num_rotations, int sums_given,
                              float* partial_workspace, float* mix, float* weights, float* out, int out_groups,
                              int64_t out_anchor_stride, void* workspace, size_t workspace_bytes, void* stream);


/* ---- G1/G2: geometric structure embedding --------------------------------------------------------------------------
 * Replaces GeometricStructureEmbedding.forward (geotransformer/modules/geotransformer/geotransformer.py:57-121 with
 * transformer/positional_embedding.py:8-34).  points (N, 3); knn (N, 3) int64: the 3 nearest other points of each point.
 * table_d / table_a: (entries, C, 2) float32 = (f, df/dx) of f(x) = W emb(x) + b sampled at x = j / entries_per_unit
 * (built by the caller with two small GEMMs); indices beyond a table fall back to the exact sinusoid sum with
 * w_* (C, C), b_* (C,), div_term (C/2,).  emb (N, N, C); eq_emb (num_anchors, N, N, 4) or NULL, wigner_d1 (num_anchors, 3, 3).
 * workspace: se3_geo_embedding_workspace_bytes(N) bytes of device scratch (per-pair index records), or NULL: the single-kernel form that
 * needs none (2-3x slower: every table read then comes from L2). */
size_t se3_geo_embedding_workspace_bytes(int N);
int se3_geo_embedding_fwd(const float* points, const int64_t* knn, int N, int C, const float* table_d, int d_entries,
                          float d_entries_per_unit, const float* table_a, int a_entries, float a_entries_per_unit,
                          float sigma_d, float sigma_a, const float* w_d, const float* b_d, const float* w_a, const float* b_a,
                          const float* div_term, const float* wigner_d1, int num_anchors, float* emb, float* eq_emb,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Operands of the embedding's weight gradients (training step: autograd through proj_d / proj_a and the max over the 3 angles,
 * geotransformer.py:92-121): S (4, N, N, C) = the sinusoid embeddings of the distance index and of the three angle indices; dEk (3, N, N, C)
 * = grad_emb masked to the channels where angle k holds the maximum.  d proj_d.weight = grad_emb^T S[0], d proj_a.weight = sum_k
 * dEk[k]^T S[1 + k] (library GEMMs), both bias gradients = sum grad_emb. */
int se3_geo_embedding_bwd_operands(const float* points, const int64_t* knn, int N, int C, const float* table_a, int a_entries,
                                   float a_entries_per_unit, float sigma_d, float sigma_a, const float* w_a, const float* b_a,
                                   const float* div_term, const float* grad_emb, float* S, float* dEk, void* stream);
/* Builds / validates such a table on the device (replaces the caller-side GEMMs): table (entries, C, 2) float32 = (f, df/dx) of
 * f(x) = weight emb(x) + bias at x = j / entries_per_unit (float64 accumulation), emb = SinusoidalPositionalEmbedding
 * (transformer/positional_embedding.py:8-34) with div_term (C/2,).  state: se3_embedding_table_state_bytes() zero-initialised bytes owned by the caller next to
 * the table; the kernel keeps a content hash of (weight, bias, div_term, sizes) there and returns immediately when the table
 * already belongs to the current values -- call it in front of every se3_geo_embedding_*_fwd; no host synchronisation.  A (table, state)
 * pair has ONE writer: calls for it must be ordered (one stream); concurrent streams keep their own pair. */
size_t se3_embedding_table_state_bytes(void);
int se3_embedding_table_refresh(const float* weight, const float* bias, const float* div_term, int C, int entries,
                                float entries_per_unit, float* table, void* state, void* stream);
/* Same, emb (N, N, C) written as bfloat16 (round to nearest even of the float32 value); eq_emb stays float32. */
int se3_geo_embedding_bf16_fwd(const float* points, const int64_t* knn, int N, int C, const float* table_d, int d_entries,
                               float d_entries_per_unit, const float* table_a, int a_entries, float a_entries_per_unit,
                               float sigma_d, float sigma_a, const float* w_d, const float* b_d, const float* w_a,
                               const float* b_a, const float* div_term, const float* wigner_d1, int num_anchors, uint16_t* emb,
                               float* eq_emb, void* workspace, size_t workspace_bytes, void* stream);

/* ---- G1 / E3: nearest-neighbour selections on the superpoint level ----------------------------------------------------
 * se3_knn3: knn (N, 3) int64 = the 3 nearest OTHER points of every point (get_embedding_indices,
 * geotransformer/modules/geotransformer/geotransformer.py:69-90: topk(k + 1) of the distance map, first column dropped).
 * se3_point_to_node_partition replaces point_to_node_partition (geotransformer/modules/ops/pointcloud_partition.py:60-107):
 * point_to_node (N) int64 = nearest node of every point; node_masks (M) uint8 = node owns at least one point;
 * node_knn_indices (M, limit) int64 = the `limit` nearest of the node's OWN points in ascending distance, padded with N;
 * node_knn_masks (M, limit) uint8.  Distances as pairwise_distance (modules/ops/pairwise_distance.py:4-30), ties by index.
 * limit <= 128.  se3_knn3 and se3_point_to_node_partition run the kernels of their stack forms on one cloud. */
int se3_knn3(const float* points, int N, int64_t* knn, void* stream);
/* se3_knn3 for num_clouds (<= 16) stacked clouds in one launch: points (sum lengths, 3), lengths HOST array; knn (sum lengths, 3)
 * holds indices LOCAL to the point's own cloud. */
int se3_knn3_stack(const float* points, const int64_t* lengths, int num_clouds, int64_t* knn, void* stream);
int se3_point_to_node_partition(const float* points, const float* nodes, int N, int M, int limit, int64_t* point_to_node,
                                uint8_t* node_masks, int64_t* node_knn_indices, uint8_t* node_knn_masks, void* stream);
/* Stack mode: the same partition for num_clouds (<= 16) clouds in one launch per kernel.  points / nodes are the stacked fine
 * points / superpoints of all clouds (cloud c: point_lengths[c] points, node_lengths[c] nodes; HOST arrays).  All outputs use
 * GLOBAL indices into the stacked arrays: point_to_node (total points) = nearest node of the point's own cloud;
 * node_knn_indices (total nodes, limit) padded with the total point count; masks as above. */
int se3_point_to_node_partition_stack(const float* points, const float* nodes, const int64_t* point_lengths,
                                      const int64_t* node_lengths, int num_clouds, int limit, int64_t* point_to_node,
                                      uint8_t* node_masks, int64_t* node_knn_indices, uint8_t* node_knn_masks, void* stream);

/* ---- E1: pairwise squared distances ---------------------------------------------------------------------------------
 * Replaces pairwise_distance (geotransformer/modules/ops/pairwise_distance.py:4-30, channel-last form): x (batch, N, C), y (batch, M, C)
 * with unit channel stride, row stride C and the given batch strides (floats; 0 = the same rows for every batch); out (batch, N, M)
 * contiguous = max(|x_n|^2 - 2 x_n.y_m + |y_m|^2, 0), or max(2 - 2 x_n.y_m, 0) with normalized != 0 (unit vectors).  Any C >= 1 (C = 3:
 * point coordinates), batch <= 65535; f32 matrix cores.  (The superpoint scores and the point-to-node partition have the distance
 * matrix fused into their own kernels: E2, E3.) */
int se3_pairwise_distance(const float* x, const float* y, int64_t batch, int N, int M, int C, int64_t x_batch_stride,
                          int64_t y_batch_stride, int normalized, float* out, void* stream);

/* ---- E2: superpoint matching scores --------------------------------------------------------------------------------
 * Replaces the score part of SuperPointMatching.forward (geotransformer/modules/geotransformer/superpoint_matching.py:31-39):
 * scores[n, m] = exp(-clamp(2 - 2 ref[n].src[m], 0)), optionally dual-normalised (S / rowsum * S / colsum).
 * ref (N, C), src (M, C) L2-normalised; workspace: N + M floats.  The kernels of the stack form on one pair with every node
 * present; ref and src may be separate allocations. */
int se3_superpoint_scores(const float* ref_feats, const float* src_feats, int N, int M, int C, int dual_normalization,
                          float* scores, float* workspace, void* stream);
/* Stack mode: the score matrices of num_pairs (<= 16) registration pairs in one launch per kernel.  feats (rows, C): the
 * L2-normalised superpoint features of all clouds; pair p: ref rows ref_rows[p] .. + ref_lengths[p], src rows src_rows[p] .. +
 * src_lengths[p]; node_masks (uint8): entries ref_mask_offsets[p] + n / src_mask_offsets[p] + m tell whether the node owns a
 * fine point -- nodes with mask 0 are absent (superpoint_matching.py:24-29 drops them before scoring): they do not enter the
 * normalisation sums and their scores are -1.  scores (num_pairs, score_stride): pair p's (N_p, M_p) matrix row-major at the
 * start of row p, -1 beyond it, so that ONE top-k over the rows selects per pair.  workspace: sum(N_p) + sum(M_p) floats.
 * All arrays are HOST arrays. */
int se3_superpoint_scores_stack(const float* feats, const uint8_t* node_masks, const int64_t* ref_rows, const int64_t* src_rows,
                                const int64_t* ref_lengths, const int64_t* src_lengths, const int64_t* ref_mask_offsets,
                                const int64_t* src_mask_offsets, int num_pairs, int C, int dual_normalization,
                                int64_t score_stride, float* scores, float* workspace, void* stream);

/* ---- F1: weighted Procrustes / inlier voting for local-to-global registration -------------------------------------------
 * Replace weighted_procrustes (geotransformer/modules/registration/procrustes.py:6-73, SVD on the CPU in the reference) and
 * the hypothesis voting of LocalGlobalRegistration (geotransformer/modules/geotransformer/local_global_registration.py:139-194).
 * Correspondences are stacked: src/ref (total, 3), scores (total,); problem s uses rows [segment_offsets[s],
 * segment_offsets[s+1]) (int64, DEVICE, num_segments + 1 entries).  If gate_transform (4x4 row-major, DEVICE) is not NULL the
 * weight of a correspondence is score * [ |ref - T src| < gate_radius ] (the refinement re-weighting).  Weights are
 * normalised by (sum + eps).  transforms: (num_segments, 4, 4).  se3_count_inliers: votes[b] = #{i : |ref_i - T_b src_i| < radius}.
 * src/ref/scores may be NULL when there is no row to read (every segment empty; count_inliers: num_points == 0), as an empty
 * tensor's data pointer is. */
int se3_weighted_procrustes(const float* src_points, const float* ref_points, const float* scores,
                            const int64_t* segment_offsets, int num_segments, const float* gate_transform, float gate_radius,
                            float eps, float* transforms, void* stream);
int se3_count_inliers(const float* src_points, const float* ref_points, int64_t num_points, const float* transforms,
                      int num_transforms, float radius, int32_t* votes, void* stream);
/* Several registration pairs at once: gate_per_segment != 0 -> gate_transforms holds one (4, 4) per segment (the pair's
 * current estimate); range_begin / range_end (DEVICE int64, one per transform) restrict hypothesis t to the correspondences
 * [range_begin[t], range_end[t]) of its own pair. */
int se3_weighted_procrustes_segments(const float* src_points, const float* ref_points, const float* scores,
                                     const int64_t* segment_offsets, int num_segments, const float* gate_transforms,
                                     int gate_per_segment, float gate_radius, float eps, float* transforms, void* stream);
int se3_count_inliers_ranges(const float* src_points, const float* ref_points, int64_t num_points, const float* transforms,
                             int num_transforms, const int64_t* range_begin, const int64_t* range_end, float radius,
                             int32_t* votes, void* stream);

/* ---- Evaluation: ground-truth patch overlaps and the Evaluator's metrics for stacked pairs -----------------------------------
 * se3_gt_node_overlaps_stack replaces get_node_correspondences (geotransformer/modules/registration/matching.py:230-315) for
 * num_clouds / 2 pairs stacked ref0, src0, ref1, src1, ... (even num_clouds <= SE3_MAX_BATCH): points_f / points_c the stacked fine
 * points / nodes, node_lengths (HOST, num_clouds) the nodes per cloud; knn (total nodes, K) int64 GLOBAL fine-point indices, knn_masks
 * (total nodes, K) and node_masks (total nodes) uint8 as se3_point_to_node_partition_stack returns them; K in {64, 128}; transforms
 * (pairs, 4, 4) DEVICE ground truth (src -> ref).  pos_radius_sq = pos_radius^2 rounded to float.  Outputs, pair p's block starting
 * at D_p = sum_{q<p} N_q M_q (N / M = its ref / src node counts): overlaps (D_B) float32, row-major (N_p, M_p) blocks, 0 where the
 * patches do not overlap; corr_indices (D_B, 2) int64 pair-local (ref, src) node indices and corr_overlaps (D_B) of the pairs with
 * overlap > 0 in row-major order, pair_counts[p] (DEVICE int64) of them valid from D_p on.  workspace: se3_gt_node_overlaps_workspace_bytes(
 * total nodes) bytes.  Three launches, no host synchronisation. */
size_t se3_gt_node_overlaps_workspace_bytes(int64_t total_nodes);
int se3_gt_node_overlaps_stack(const float* points_f, const float* points_c, const int64_t* node_lengths, int num_clouds,
                               const int64_t* knn, const uint8_t* knn_masks, const uint8_t* node_masks, int K, const float* transforms,
                               float pos_radius, float pos_radius_sq, void* workspace, float* overlaps, int64_t* corr_indices,
                               float* corr_overlaps, int64_t* pair_counts, void* stream);
/* se3_registration_metrics_stack: the Evaluator of experiments/se3ete.3dmatch/loss.py:198-262 (kitti == 0) or
 * experiments/se3eti.kitti/loss.py:94-151 (kitti != 0) for num_pairs pairs in one launch.  pair_table (DEVICE, num_pairs x 16 int64),
 * one row per pair: [0] overlaps block (float*, (N, M) as above), [1] N, [2] M, [3] / [4] predicted ref / src node indices (int64*),
 * [5] their count, [6] / [7] ref / src correspondence points (float* (n, 3)), [8] their count n, [9] estimated transform (float* 4x4),
 * [10] ground-truth transform (float* 4x4), [11] stage-0 src points (float* (m, 3), 3DMatch only), [12] m; [13..15] unused.
 * rows (num_pairs, 6) float32: PIR, IR, RRE (degrees), RTE, RMSE (NaN with kitti), RR.  Empty sets give NaN as the mean of an empty
 * tensor does; a predicted node index outside the pair's block makes PIR NaN.  Counts are integers and the RMSE sum has a fixed order:
 * a pair's row does not depend on the others. */
int se3_registration_metrics_stack(const int64_t* pair_table, int num_pairs, float acceptance_overlap, float acceptance_radius,
                                   float rmse_threshold, float rre_threshold, float rte_threshold, int kitti, float* rows, void* stream);

/* ---- RANSAC registration from correspondences for stacked pairs (csrc/ransac.hip) ----------------------------------------------------
 * Replaces registration_with_ransac_from_correspondences (geotransformer/utils/open3d.py:169-198, Open3D's CPU RANSAC) for num_pairs
 * pairs: src_points / ref_points (total, 3) float32, pair p owns rows [offsets[p], offsets[p+1]) (int64, DEVICE, num_pairs + 1 entries,
 * n_p rows).  Each pair scores H = num_iterations hypotheses of ransac_n (3..16) correspondences drawn uniformly with replacement:
 *   idx_j(h) = ((splitmix64(splitmix64(seed) + h * ransac_n + j) >> 32) * n_p) >> 32        (uint64 wrap-around; splitmix64 with the
 *   standard constants 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB -- csrc/splitmix.h), independent of the pair's position,
 * or taken from hypothesis_indices (DEVICE (num_pairs, H, ransac_n) int32, pair-local; an index outside [0, n_p) voids the hypothesis).
 * A hypothesis is the unweighted float64 Kabsch fit of its sample (src -> ref) rounded to float32; correspondence i is its inlier iff
 * |T s_i - r_i|^2 < distance_threshold^2 in float32.  The winner has the most inliers, then the smallest inlier error sum, then the lowest
 * h, and needs at least one inlier: otherwise -- and when ransac_n < 3, n_p < ransac_n or distance_threshold <= 0 -- the pair's result is
 * the identity with fitness 0, RMSE 0 and best_hypothesis -1.  Outputs: transforms (num_pairs, 4, 4) the winner's own fit (no refit),
 * fitness (num_pairs) = inliers / n_p, inlier_rmse (num_pairs) = sqrt(error sum / inliers), best_hypothesis (num_pairs) int32; counts /
 * err_sums (num_pairs, H) int32 / float32 per hypothesis, or both NULL.  Non-finite correspondences are never inliers and a non-finite
 * sample has 0 inliers.  Each error sum runs serially in correspondence order: a pair's result does not depend on its batch or the run.
 * ransac_n > 16: SE3_ERR_UNSUPPORTED.  workspace: se3_ransac_correspondences_workspace_bytes(num_pairs, num_iterations) bytes, 16-byte
 * aligned.  Three launches (fit, score, select), no host synchronisation. */
size_t se3_ransac_correspondences_workspace_bytes(int num_pairs, int num_iterations);
int se3_ransac_correspondences_stack(const float* src_points, const float* ref_points, const int64_t* offsets, int num_pairs,
                                     float distance_threshold, int ransac_n, int num_iterations, uint64_t seed,
                                     const int32_t* hypothesis_indices, void* workspace, size_t workspace_bytes, float* transforms,
                                     float* fitness, float* inlier_rmse, int32_t* best_hypothesis, int32_t* counts, float* err_sums,
                                     void* stream);
/* The same with Open3D's correspondence checkers (registration_with_ransac_from_feats, geotransformer/utils/open3d.py:133-166); the kernels
 * are shared.  edge_length_similarity t in (0, 1] (0: off): before the fit, a hypothesis is rejected if two of its sampled correspondences
 * a, b have |s_a - s_b| < t |r_a - r_b| or |r_a - r_b| < t |s_a - s_b| (float64).  check_distance != 0: after the fit, it is rejected if a
 * sampled correspondence has d^2 > distance_threshold^2 in the scoring arithmetic.  A rejected hypothesis scores 0 inliers.  passed
 * (num_pairs, H) uint8 or NULL: 1 for a hypothesis with a valid sample that no checker rejected.  With t = 0 and check_distance = 0 every
 * output is bit-identical to se3_ransac_correspondences_stack.  Workspace as above. */
int se3_ransac_correspondences_checked_stack(const float* src_points, const float* ref_points, const int64_t* offsets, int num_pairs,
                                             float distance_threshold, int ransac_n, int num_iterations, uint64_t seed,
                                             const int32_t* hypothesis_indices, double edge_length_similarity, int check_distance,
                                             void* workspace, size_t workspace_bytes, float* transforms, float* fitness,
                                             float* inlier_rmse, int32_t* best_hypothesis, int32_t* counts, float* err_sums, uint8_t* passed,
                                             void* stream);

/* ---- feature-space matching for stacked pairs (csrc/feature_nn.hip) ---------------------------------------------------------------------
 * The nearest neighbour in descriptor space of every row in the other cloud of its pair, both directions in one call, without an (N, M)
 * array: extract_correspondences_from_feats (geotransformer/modules/registration/matching.py:135-170) and extract_corr_indices_from_feats
 * (utils/registration.py:179-212).  ref_feats (num_ref_rows, channels) / src_feats (num_src_rows, channels) float32; pair p owns rows
 * [ref_offsets[p], ref_offsets[p+1]) and [src_offsets[p], src_offsets[p+1]) (int64, DEVICE, num_pairs + 1 entries from 0 to the row count).
 * Candidates are ranked by v = (|x|^2 - 2 x.y) + |y|^2 with float32 MFMA products (x the query row); among equal v the lowest index wins; a
 * NaN or infinite v is never chosen.  Outputs per ref row: nn_src_indices (pair-local int64, -1 without a candidate) and
 * nn_src_sq_distances (float32, sum_k (x_k - y_k)^2 recomputed for the winner, +inf for -1); the same per src row in nn_ref_*.  Results are
 * bit-identical from run to run and for a pair alone or in any batch.  workspace: se3_feature_nn_workspace_bytes bytes (O(rows)).  Three
 * launches, no host synchronisation.
 *   se3_feature_corr_count_stack   entry_offsets (num_ref_rows + num_src_rows + 1) int64: the exclusive scan of the entries each element of
 *       the pair-major sequence [ref rows of pair 0, src rows of pair 0, ref rows of pair 1, ...] contributes, the total last; pair p's
 *       entries are [entry_offsets[ref_offsets[p] + src_offsets[p]], entry_offsets[ref_offsets[p+1] + src_offsets[p+1]]).
 *       mode 0: (i, nn_src(i)) per ref row; 1: those with nn_ref(nn_src(i)) == i; 2: the union of (i, nn_src(i)) and (nn_ref(j), j) without
 *       duplicates in row-major (i, j) order; 3: the ref rows' entries followed by the src rows' (nn_ref(j), j), duplicates kept.  A row
 *       with index -1 contributes nothing.
 *   se3_feature_corr_fill_stack    ref_corr_indices / src_corr_indices (total) int64, pair-local, with the same arrays, mode and offsets. */
size_t se3_feature_nn_workspace_bytes(int64_t num_ref_rows, int64_t num_src_rows);
int se3_feature_nn_stack(const float* ref_feats, const float* src_feats, const int64_t* ref_offsets, const int64_t* src_offsets,
                         int num_pairs, int64_t num_ref_rows, int64_t num_src_rows, int channels, void* workspace, size_t workspace_bytes,
                         int64_t* nn_src_indices, float* nn_src_sq_distances, int64_t* nn_ref_indices, float* nn_ref_sq_distances,
                         void* stream);
int se3_feature_corr_count_stack(const int64_t* nn_src_indices, const int64_t* nn_ref_indices, const int64_t* ref_offsets,
                                 const int64_t* src_offsets, int num_pairs, int64_t num_ref_rows, int64_t num_src_rows, int mode,
                                 int64_t* entry_offsets, void* stream);
int se3_feature_corr_fill_stack(const int64_t* nn_src_indices, const int64_t* nn_ref_indices, const int64_t* ref_offsets,
                                const int64_t* src_offsets, int num_pairs, int64_t num_ref_rows, int64_t num_src_rows, int mode,
                                const int64_t* entry_offsets, int64_t total, int64_t* ref_corr_indices, int64_t* src_corr_indices,
                                void* stream);

/* ---- eval.py's benchmark metrics for stacked pairs (csrc/benchmark.hip) ---------------------------------------------------------------
 * The per-pair metrics and summaries of experiments/se3ete.3dmatch/eval.py:42-357 and experiments/se3eti.kitti/eval.py:32-185.  Every call
 * handles all pairs (groups) in a fixed number of launches with no host synchronisation; counts are integers and sums run in a fixed order,
 * so a pair's row is bit-identical alone or in any batch.  The arithmetic contract is stated at the top of csrc/benchmark.hip.
 *
 * se3_benchmark_correspondences_stack: evaluate_correspondences (geotransformer/utils/registration.py:133-250).  ref_points / src_points
 * (total, 3) float32, pair p owns rows [offsets[p], offsets[p+1]) (DEVICE int64, num_pairs + 1); max_count (HOST) >= every pair's count
 * sizes the grid (a longer pair gets overlap NaN); transforms (num_pairs, 4, 4) DEVICE float32 ground truth (src -> ref).  out
 * (num_pairs, 4) float64: overlap (nearest transformed src point closer than positive_radius, float32 distances), inlier_ratio,
 * residual (float64), num_corr; 0 / 0 = NaN for a pair without correspondences.  workspace:
 * se3_benchmark_correspondences_workspace_bytes(num_pairs) bytes.  A memset and two launches. */
size_t se3_benchmark_correspondences_workspace_bytes(int num_pairs);
int se3_benchmark_correspondences_stack(const float* ref_points, const float* src_points, const int64_t* offsets, int num_pairs,
                                        int64_t max_count, const float* transforms, float positive_radius, void* workspace,
                                        size_t workspace_bytes, double* out, void* stream);
/* se3_benchmark_sparse_stack: evaluate_sparse_correspondences (registration.py:253-280) with its set semantics (duplicates count once).
 * Predicted node pairs ref_node_indices / src_node_indices (DEVICE int64), pair p's on [pred_offsets[p], pred_offsets[p+1]); ground truth
 * gt_node_corr_indices (g, 2) DEVICE int64 on [gt_offsets[p], gt_offsets[p+1]); node_counts (num_pairs, 2) DEVICE int64 (N_p, M_p);
 * word_offsets (num_pairs + 1) DEVICE int64 the prefix sums of se3_benchmark_sparse_words(N_p, M_p) (32-bit bitmap words of the pair:
 * 2 ceil(N M / 32) + 2 ceil(N / 32) + 2 ceil(M / 32)).  Indices outside [0, N) x [0, M) are ignored.  out (num_pairs, 3) float64:
 * precision, recall, hit_ratio with the reference's + 1e-12 denominators.  workspace: se3_benchmark_sparse_workspace_bytes(node_counts
 * (HOST, num_pairs x 2), num_pairs) bytes, zeroed by the call.  A memset and one launch. */
int64_t se3_benchmark_sparse_words(int64_t num_ref_nodes, int64_t num_src_nodes);
size_t se3_benchmark_sparse_workspace_bytes(const int64_t* node_counts, int num_pairs);
int se3_benchmark_sparse_stack(const int64_t* ref_node_indices, const int64_t* src_node_indices, const int64_t* pred_offsets,
                               const int64_t* gt_node_corr_indices, const int64_t* gt_offsets, const int64_t* node_counts,
                               const int64_t* word_offsets, int num_pairs, void* workspace, size_t workspace_bytes, double* out, void* stream);
/* se3_benchmark_transform_error_stack: compute_transform_error (datasets/registration/threedmatch/utils.py:131-137, nibabel's mat2quat) and
 * compute_registration_error (registration.py:51-67) in float64.  gt_transforms / est_transforms (num_pairs, 4, 4), covariances
 * (num_pairs, 6, 6) float64 DEVICE, has_covariance (num_pairs) DEVICE int32 (0: no covariance; NULL: none has one).  out (num_pairs, 3)
 * float64: err (NaN without covariance), RRE (degrees), RTE.  One launch. */
int se3_benchmark_transform_error_stack(const double* gt_transforms, const double* est_transforms, const double* covariances,
                                        const int32_t* has_covariance, int num_pairs, double* out, void* stream);
/* se3_benchmark_summary: eval.py's per-group and overall numbers.  rows (P, 6) DEVICE float64 per pair: precision, inlier_ratio, overlap,
 * err, rre, rte; is_gt (P) DEVICE int32 (3DMatch: 1 for a benchmark pair -- listed in gt.log with id1 > id0 + 1 -- otherwise 0; unused for
 * KITTI); group g owns pairs [group_offsets[g], group_offsets[g+1]) (DEVICE int64, num_groups + 1); max_group_pairs (HOST) the largest
 * group, at most 4096 (SE3_ERR_UNSUPPORTED beyond).  group_out (num_groups, 14) and overall (14) float64: PIR, PMR>0, PMR>=0.1, PMR>=0.3,
 * PMR>=0.5, FMR (inlier_ratio >= inlier_ratio_threshold), IR, OV, FMR_std, RR, mean_RRE, mean_RTE, median_RRE, median_RTE.  3DMatch
 * (kitti == 0): a benchmark pair is accepted iff err < rmse_threshold^2, RR is over the benchmark pairs, the overall row is the mean over
 * groups of each group value and FMR_std the population std of the groups' FMR.  KITTI: accepted iff rre < rre_threshold and rte <
 * rte_threshold over all pairs, exactly one group, FMR_std over its pairs.  Means, medians and stds of empty sets are NaN.  Two launches. */
int se3_benchmark_summary(const double* rows, const int32_t* is_gt, const int64_t* group_offsets, int num_groups, int64_t max_group_pairs,
                          int kitti, double inlier_ratio_threshold, double rmse_threshold, double rre_threshold, double rte_threshold,
                          double* group_out, double* overall, void* stream);

/* Mutual top-k correspondence mask (local_global_registration.py:104-131): mask[b, i, j] = 1 iff scores[b, i, j] is among the k
 * largest of row i AND of column j of patch pair b (ties by index), exceeds `threshold`, and row_masks[b, i] & col_masks[b, j].
 * scores (batch, rows, cols) float32, masks uint8; rows * cols <= 16384; NULL pointers only with batch == 0.  A NaN score is never
 * kept and takes no top-k slot (torch.topk would rank it first). */
int se3_mutual_topk_mask(const float* scores, const uint8_t* row_masks, const uint8_t* col_masks, int batch, int rows, int cols,
                         int k, float threshold, uint8_t* mask, void* stream);



/* grouping.anchor_query (grouping_cuda_kernel.cu:166-233, grouping_cuda.cpp:88-108): anchor_weights (b, np, na, ks, nn) =
 * (kw_k - r)^2 + ((kh_k - theta) r)^2 for the local neighbour coordinates grouped_xyz (b, 3, np, nn), r = |x| + 1e-6,
 * theta = acos(x . anchors[a] / r), kernel_points (ks, 2) = (radial, angular) positions.  (sample_idx, grouped_indices and nq of the
 * reference's signature are not read by its kernel.) */
int se3_vgtk_anchor_query(const float* grouped_xyz, const float* anchors, const float* kernel_points, int batch, int num_points,
                          int num_neighbors, int num_anchors, int kernel_size, float* anchor_weights, void* stream);
/* grouping.initial_anchor_query (grouping_cuda_kernel.cu:102-152, grouping_cuda.cpp:138-158): centers (b, 3, nc), xyz (m, 3) shared by the
 * batch, kernel_points (ks, na, 3): anchor_weights / anchor_counts (b, ks, nc, na) = sum / number over the points within `radius` of the
 * centre of the positive part of 1 - |kernel point + centre - point|^2 / sigma.  Summed in point order (the reference: atomicAdd). */
int se3_vgtk_initial_anchor_query(const float* centers, const float* xyz, const float* kernel_points, int batch, int num_centers,
                                  int num_points, int num_anchors, int kernel_size, float radius, float sigma, float* anchor_weights,
                                  float* anchor_counts, void* stream);
/* ---- EPN toolkit (vgtk) equivalents: SURVEY section 8f row 4 -------------------------------------------------------------------------
 * Replace the CUDA extensions vgtk.cuda.{gathering, grouping, zpconv} (geotransformer/modules/e2pn/vgtk/vgtk/cuda: gathering_cuda.cpp,
 * grouping_cuda.cpp, zpconv_cuda.cpp and their *_kernel.cu) entry for entry: same tensor layouts (channel-first, int32 indices), same
 * edge cases; float sums are gathers in a fixed order (the reference scatters with atomicAdd), errors come back as status codes, every
 * launch takes a stream.  Called from se3et_amd/vgtk.py (mirror of vgtk/spconv/functional.py, vgtk/pc/sample.py).
 *   gather_points: out[b, c, j] = points[b, c, idx[b, j]]; backward scatter-adds in ascending j           (gathering_cuda_kernel.cu:42-98)
 *     (num_indices == 0: idx and the (b, c, 0) tensor may be NULL; the backward then writes an all-zero gradient)
 *   ball_query: the first nsample support indices (ascending) within `radius` of each query, a short list repeats itself, a list short
 *     by exactly one keeps a trailing 0, an empty one is all 0                                            (grouping_cuda_kernel.cu:52-99)
 *   furthest_point_sampling: idxs[b, 0] = 0, then iteratively the point furthest from the chosen set; points with |p|^2 <= 1e-3 are
 *     never chosen; exact ties resolve as in the reference's block reduction; temp_workspace (b, n) floats (grouping_cuda_kernel.cu:337-452)
 *   inter_zpconv: out[b, c, k, p, a] = sum_n w[b, p, a, k, n] feats[b, c, nbr[b, p, a, k, n], a]; backward = its transpose
 *     (workspace: se3_vgtk_inter_zpconv_bwd_workspace_bytes)                                               (zpconv_cuda_kernel.cu:32-116)
 *   intra_zpconv: out[b, c, k, p, a] = sum_n w[a, k, n] feats[b, c, p, nbr[a, n]]; backward = its transpose (zpconv_cuda_kernel.cu:119-195) */
int se3_vgtk_gather_points_fwd(const float* points, const int32_t* idx, int batch, int channels, int num_points, int num_indices,
                               float* out, void* stream);
int se3_vgtk_gather_points_bwd(const float* grad_out, const int32_t* idx, int batch, int channels, int num_points, int num_indices,
                               float* grad_points, void* stream);
int se3_vgtk_ball_query(const float* new_xyz, const float* xyz, int batch, int num_support, int num_queries, float radius, int nsample,
                        int32_t* idx, void* stream);
int se3_vgtk_furthest_point_sampling(const float* dataset, int batch, int num_points, int num_samples, float* temp_workspace,
                                     int32_t* idxs, void* stream);
int se3_vgtk_inter_zpconv_fwd(const int32_t* neighbors, const float* weights, const float* feats, int batch, int num_samples,
                              int num_support, int num_anchors, int kernel_size, int num_nn, int channels, float* out, void* stream);
size_t se3_vgtk_inter_zpconv_bwd_workspace_bytes(int batch, int num_samples, int num_support, int num_anchors, int kernel_size, int num_nn);
int se3_vgtk_inter_zpconv_bwd(const int32_t* neighbors, const float* weights, const float* grad_out, int batch, int num_samples,
                              int num_support, int num_anchors, int kernel_size, int num_nn, int channels, float* grad_feats,
                              void* workspace, size_t workspace_bytes, void* stream);
int se3_vgtk_intra_zpconv_fwd(const int32_t* neighbors, const float* weights, const float* feats, int batch, int num_points,
                              int anchors_in, int anchors_out, int kernel_size, int num_nn, int channels, float* out, void* stream);
int se3_vgtk_intra_zpconv_bwd(const int32_t* neighbors, const float* weights, const float* grad_out, int batch, int num_points,
                              int anchors_in, int anchors_out, int kernel_size, int num_nn, int channels, float* grad_feats, void* stream);


/* ---- host-pointer variants of geotransformer.ext for DataLoader worker processes -----------------------------------------
 * Same contract as ext.grid_subsampling / ext.radius_neighbors (extensions/pybind.cpp:6-18; CPU, contiguous float32 / int64 tensors):
 * plain host memory in and out, no GPU, no global state, callable from forked workers.  grid: s_points / s_normals hold n rows, the first
 * sum(s_lengths) are valid, in the reference's emission order.  radius: out == NULL computes *max_count only (the width the reference's
 * result would have); otherwise out is (nq, limit) int64, rows ascending in distance, padded with ns.  Bound by se3et_amd/ext.py. */
int se3_grid_subsample_host(const float* points, const float* normals, int64_t n, const int64_t* lengths, int batch, float voxel_size,
                            float* s_points, float* s_normals, int64_t* s_lengths);
int se3_radius_neighbors_host(const float* q_points, int64_t nq, const float* s_points, int64_t ns, const int64_t* q_lengths,
                              const int64_t* s_lengths, int batch, float radius, int64_t limit, int64_t* out, int64_t* max_count);
/* se3_radius_count_hist on HOST memory (every pointer host; same contract, same numbers): a cell list of its own, linear in the points.
 * The queries of a cloud are shared among SE3_HOST_THREADS threads (environment, default 1). */
int se3_radius_count_hist_host(const float* q_points, int64_t nq, const float* s_points, int64_t ns, const int64_t* q_lengths,
                               const int64_t* s_lengths, int batch, float radius, int hist_n, const int* slot_of_cloud, int num_slots,
                               int32_t* hist, int32_t* dropped, int32_t* max_count);

/* ---- round 4: the remaining library products of the inference forward as kernels --------------------------------------------------------
 * se3_patch_scores   experiments/se3ete.3dmatch/model.py:186-203 -- the fine-matching score matrices of all patch pairs with the two feature
 *                    gathers fused: out (num_patches, K, K) = <feats[ref_idx[b, n]], feats[src_idx[b, m]]> * scale; an index outside
 *                    [0, num_rows) selects a zero row (the reference's padded feature row); K = patch_points in {64, 128}, C % 64 == 0.
 * se3_anchor_mix_stack  conditional_transformer.py:209-249 (eq2inv_soft) for all pairs of a batch: out[a, r, :] = sum_e mix[p(r)][a, e]
 *                    x[e, r, :] for the packed rows r of pair p (rows of no pair: zero); x, out (6, rows, channels), mix (pairs, 6, 6). */
int se3_patch_scores(const float* feats, const int64_t* ref_idx, const int64_t* src_idx, int64_t num_patches, int patch_points,
                     int64_t num_rows, int C, float scale, float* out, void* stream);
int se3_anchor_mix_stack(const float* x, int64_t rows, int channels, const float* mix, const int64_t* starts_host, const int64_t* lengths_host,
                         int num_pairs, float* out, void* stream);

/* ---- D7 / D8: the coarse transformer of a batch of pairs, every launch issued from C ---------------------------------------------------------
 * RPEConditionalTransformer.forward (conditional_transformer.py:251-390) with the layers it schedules (rpe_transformer.py:134-194,
 * vanilla_transformer.py:872-946, output_layer.py:7-47) and GeometricTransformer's out_proj (geotransformer.py:310-317) as ONE host call:
 * about 130 launches on the caller's stream, no interpreter between them (one pair per forward was bound by ~480 Python-issued launches).
 * The plan is a HOST structure of device pointers: weights as se3_linear_split_weights_f16 pieces (+ f32 biases), the per-cloud geometric
 * embeddings, the packed-row layout (refs of all pairs first, then srcs; cloud starts multiples of 32).  x_in (A, rows, C) = in_proj of the
 * superpoint features in that layout, out (rows, out_proj.out_features).  Block types: 0 'self', 1 'self_eq', 2 'cross', 3 'cross_a_soft',
 * 4 'cross_r_soft' (followed by eq2inv_soft + RotCompressOutput when the next block is invariant).  Supported: the SE3ET-E / -E2 and
 * SE3ET-I / -I2 / KITTI block lists, A = 6, head dimension 64 for the key-anchor groups of the equivariant cross attention. */
#define SE3_MAX_BLOCKS 16
typedef struct {
  const void* pieces;       /* se3_linear_split_weights_f16 of the (out_features, in_features) weight */
  const float* bias;        /* (out_features) or NULL */
  int in_features, out_features;
} se3_linear_t;
typedef struct {
  int type;
  int off_q, off_k, off_qp, off_qe;        /* self blocks: column offsets of [q | k | W_p^T q | W_eq^T q] in the stacked projection (off_qe < 0: none) */
  se3_linear_t stack;                      /* self blocks: the composed projection */
  se3_linear_t q, k, v;                    /* cross blocks: proj_q, proj_k; all blocks: proj_v */
  se3_linear_t out;                        /* attention.linear (its bias is applied by the LayerNorm kernel) */
  const void* out_pieces_g2;               /* equivariant cross blocks: the same weight repeated 2 / 3 times along in_features (key-anchor groups) */
  const void* out_pieces_g3;
  const float* ln1_w;
  const float* ln1_b;
  float ln1_eps;
  se3_linear_t expand, squeeze;            /* AttentionOutput (the squeeze bias is applied by the LayerNorm kernel) */
  const float* ln2_w;
  const float* ln2_b;
  float ln2_eps;
  const int64_t* trace_idx;                /* equivariant cross blocks: (num_rotations, 6) int64 on the device */
  int num_rotations;
} se3_layer_t;
typedef struct {
  int A, C, H, num_blocks, num_pairs, emb_bf16;
  se3_layer_t layers[SE3_MAX_BLOCKS];
  se3_linear_t rc_expand, rc_squeeze;      /* RotCompressOutput (only read behind a cross_r_soft block) */
  const float* rc_ln_w;
  const float* rc_ln_b;
  float rc_ln_eps;
  se3_linear_t out_proj;
  int64_t starts[SE3_MAX_BATCH], lengths[SE3_MAX_BATCH];   /* packed row start / length of every cloud: ref0 .. ref(B-1), src0 .. src(B-1) */
  int64_t rows0, rows;                     /* packed rows of all refs; of all clouds */
  const float* emb[SE3_MAX_BATCH];         /* (N_c, N_c, C) geometric embedding of cloud c (bfloat16 when emb_bf16) */
  const float* eq[SE3_MAX_BATCH];          /* (A, N_c, N_c, 4) equivariant embedding or NULL */
} se3_transformer_plan_t;
size_t se3_transformer_workspace_bytes(const se3_transformer_plan_t* plan);
/* layout[6] = sizeof(se3_linear_t), sizeof(se3_layer_t), sizeof(se3_transformer_plan_t), offsetof(plan, layers), offsetof(plan, starts),
 * offsetof(plan, emb): a binding in another language checks its mirror of the structs against the library it loaded. */
void se3_transformer_plan_layout(size_t* layout);
int se3_transformer_forward(const se3_transformer_plan_t* plan, const float* x_in, float* out, void* workspace, size_t workspace_bytes,
                            void* stream);
int se3_linear_stream_segments(const float* x, int64_t rows, int in_features, int seg_channels, int64_t seg_stride, const void* weight_pieces,
                               const float* bias, int out_features, int apply_relu, float* out, int64_t out_row_stride, void* stream);

/* ---- pair ground truth: nearest neighbour, overlap, correspondences, gt.info covariance (csrc/pair_geometry.hip, csrc/pair_grid.h) ------------
 * The reference's get_nearest_neighbor (utils/pointcloud.py:11-22), compute_overlap / get_correspondences (utils/registration.py:149-173) and
 * calibrate_ground_truth (threedmatch/utils.py:197-228) for up to SE3_PAIR_MAX_PAIRS stacked pairs per call, all float64; the arithmetic
 * contract is the header comment of csrc/pair_geometry.hip.  Points are (rows, 3) on the device, float32 (elem 0) or float64 (elem 1), promoted
 * on load; pair p owns rows [offsets_host[p], offsets_host[p + 1]) of a stacked array (HOST int64, num_pairs + 1 entries from 0);
 * transforms_host is (num_pairs, 4, 4) float64 on the HOST (checked finite), applied to the SUPPORT cloud.  Indices are pair-local.
 *   se3_pair_grid_build     the float64 cell grid over each pair's transformed support.  cell_hint > 0: the cell size (the ball radius);
 *                           0: from the point density (nearest neighbour).  The workspace then serves any number of searches.
 *   se3_pair_nearest_neighbor_stack   distances (nq) float64 and indices (nq) int64 of the exact nearest support point of every query row;
 *                           the lowest index among equal distances; inf / -1 for an empty support.
 *   se3_pair_ball_count_stack   row_offsets (nq + 1) int64 on the device: the exclusive scan of the per-row hit counts, the total last.
 *   se3_pair_ball_fill_stack    out (total, 2) int64: (i, j) of every hit, rows ascending in i, j ascending within a row; row_offsets and
 *                           total as the count call left them (the same grid, points and radius).
 *   se3_pair_ball_count_radii_stack / se3_pair_ball_fill_radii_stack   the same two passes with one radius per pair: radii_host (num_pairs)
 *                           float64 on the HOST, each finite and >= 0 (csrc/iss.hip: clouds whose default radii differ).
 *   se3_pair_overlap_stack  out (num_pairs) float64 = count(d * d < radius * radius) / rows of the pair's nearest-neighbour distances (NaN
 *                           for a pair without rows).
 *   se3_pair_info_covariance_stack   out (num_pairs, 6, 6) float64 = sum G^T G, G = [I3 | -[p]x], over the transformed src points
 *                           src[selected[k]] of each pair (selected: pair-local int64 on the device, pair p's on
 *                           [selected_offsets_host[p], selected_offsets_host[p + 1])); the zero matrix without a point.
 *   se3_debug_pair_*_host   the same search core (pair_grid.h) on HOST memory for one pair: every pointer a host pointer.  ball: counts (nq)
 *                           always; out (capacity, 2) may be NULL; *total may exceed capacity (rows that do not fit are not written). */
#define SE3_PAIR_MAX_PAIRS 32
size_t se3_pair_grid_workspace_bytes(int64_t ns_total, int num_pairs);
int se3_pair_grid_build(const void* s_points, int elem, const int64_t* s_offsets_host, int num_pairs, const double* transforms_host,
                        double cell_hint, void* workspace, size_t workspace_bytes, void* stream);
int se3_pair_nearest_neighbor_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                                    const int64_t* q_offsets_host, int num_pairs, double* distances, int64_t* indices, void* stream);
int se3_pair_ball_count_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                              const int64_t* q_offsets_host, int num_pairs, double radius, int64_t* row_offsets, void* stream);
int se3_pair_ball_fill_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                             const int64_t* q_offsets_host, int num_pairs, double radius, const int64_t* row_offsets, int64_t total,
                             int64_t* out, void* stream);
int se3_pair_ball_count_radii_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                                    const int64_t* q_offsets_host, int num_pairs, const double* radii_host, int64_t* row_offsets, void* stream);
int se3_pair_ball_fill_radii_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                                   const int64_t* q_offsets_host, int num_pairs, const double* radii_host, const int64_t* row_offsets,
                                   int64_t total, int64_t* out, void* stream);
int se3_pair_overlap_stack(const double* nn_distances, const int64_t* q_offsets_host, int num_pairs, double radius, double* out, void* stream);
int se3_pair_info_covariance_stack(const void* src_points, int elem, const int64_t* s_offsets_host, const double* transforms_host,
                                   const int64_t* selected, const int64_t* selected_offsets_host, int num_pairs, double* out, void* stream);
int se3_debug_pair_nearest_neighbor_host(const void* q_points, int64_t nq, const void* s_points, int64_t ns, int elem, const double* transform,
                                         double* distances, int64_t* indices);
int se3_debug_pair_ball_host(const void* q_points, int64_t nq, const void* s_points, int64_t ns, int elem, const double* transform,
                             double radius, int64_t* counts, int64_t* out, int64_t capacity, int64_t* total);

/* ---- scan preparation: voxel downsampling, k nearest neighbours, k-NN normals (csrc/voxel_downsample.hip, csrc/knn_normals.hip) ---------------
 * Open3D's voxel_down_sample and estimate_normals (utils/open3d.py:49-65) for up to SE3_PAIR_MAX_PAIRS stacked clouds per call, all float64;
 * the contract is the header comment of the two kernel files.  Points (and normals) are (rows, 3) on the device, float32 (elem 0) or float64
 * (elem 1), promoted on load; cloud c owns rows [offsets_host[c], offsets_host[c + 1]) (HOST int64, num_clouds + 1 entries from 0).
 *   se3_voxel_downsample_stack   out_points (and out_normals when normals is given) sized by the input row count, float64: the clouds'
 *                           voxel means back to back, cloud c's out_counts[c] rows (DEVICE int) in the order of each voxel's first member.
 *                           status (DEVICE int): 0, or bit 1 = a non-finite point or normal, bit 2 = an axis needs 2^21 voxels or more (the
 *                           clouds concerned give no rows, and out_counts[c] holds MINUS their bits); read it with the counts.
 *                           voxel_size must be positive and finite; at most 2^30 - 64 points per call.  A voxel above 64 members is
 *                           ordered by one workgroup (quadratic in its members) and summed by one thread: correct, slow.
 *   se3_knn_stack           on a grid built by se3_pair_grid_build over the support clouds (identity transforms, cell_hint 0): out_idx
 *                           (nq, k) int64 cloud-local and out_d2 (nq, k) float64 squared distances, rows ascending by (d^2, index); -1 and
 *                           +inf in the columns a smaller cloud leaves.  k in [1, SE3_KNN_MAX].
 *   se3_knn_normals_stack   the fused form: out_normals (nq, 3) float64 from each row's k neighbours, the tables never leave the registers.
 *                           viewpoints_host: NULL, or (num_clouds, 3) float64 on the HOST (checked finite): n . (viewpoint - p) >= 0.
 *   se3_debug_*_host        the same text on HOST memory for one cloud, no GPU: every pointer a host pointer.  voxel: *status as above;
 *                           normals: the cloud searched in itself, out_covariances (n, 6: xx xy xz yy yz zz) may be NULL. */
#define SE3_KNN_MAX 64
size_t se3_voxel_downsample_workspace_bytes(int64_t n_total, int num_clouds);
int se3_voxel_downsample_stack(const void* points, int elem, const void* normals, const int64_t* offsets_host, int num_clouds, double voxel_size,
                               double* out_points, double* out_normals, int* out_counts, int* status, void* workspace, size_t workspace_bytes,
                               void* stream);
int se3_knn_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                  const int64_t* q_offsets_host, int num_clouds, int k, int64_t* out_idx, double* out_d2, void* stream);
int se3_knn_normals_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                          const int64_t* q_offsets_host, int num_clouds, int k, const double* viewpoints_host, double* out_normals, void* stream);
int se3_debug_voxel_downsample_host(const void* points, int64_t n, int elem, const void* normals, double voxel_size, double* out_points,
                                    double* out_normals, int64_t* out_count, int* status);
int se3_debug_knn_host(const void* q_points, int64_t nq, const void* s_points, int64_t ns, int elem, int k, int64_t* out_idx, double* out_d2);
int se3_debug_knn_normals_host(const void* points, int64_t n, int elem, int k, const double* viewpoint, double* out_normals,
                               double* out_covariances);

/* ---- ICP refinement of stacked pairs (csrc/icp.hip, csrc/icp_core.h) ---------------------------------------------------------------------------
 * Open3D's registration_icp, point-to-point (no scale) or point-to-plane -- and, through the weighted entries below, its robust loss
 * kernels and registration_generalized_icp -- for up to SE3_PAIR_MAX_PAIRS stacked pairs per call, all float64 and
 * resident on the device: a call enqueues every evaluation and update and waits for nothing; the contract is the header comment of
 * csrc/icp.hip.  Points and normals are (rows, 3) on the device, float32 (elem 0) or float64 (elem 1), promoted on load; pair p owns rows
 * [src_offsets_host[p], src_offsets_host[p + 1]) of the stacked source (HOST int64, num_pairs + 1 entries from 0).
 *   se3_icp_stack           grid_workspace: se3_pair_grid_build over the REFERENCE clouds with identity transforms and cell_hint = the
 *                           correspondence distance (nref_total rows; the reference points are read from it).  ref_normals: (nref_total, 3) of
 *                           normals_elem, NULL for point-to-point.  T0: (num_pairs, 4, 4) float64 on the DEVICE, ref ~ T0 src.  Results, all on
 *                           the device: out_transforms (num_pairs, 4, 4) float64, out_fitness and out_rmse float64, out_iterations,
 *                           out_converged and out_status int per pair; out_correspondences NULL or int64 per stacked source row: the
 *                           pair-local reference row of the final evaluation, -1 for none.  status is a sum of SE3_ICP_* bits: NONFINITE
 *                           refuses the pair (NaN transform); TOO_FEW, SINGULAR and EMPTY mark an identity update; STEP_REFUSED a
 *                           point-to-plane step of 1 rad or more, at which the pair ends with its previous transform.
 *                           max_iteration in [0, SE3_ICP_MAX_ITERATION]; 0 evaluates T0 only.
 *   se3_debug_icp_host      the same text for one pair on HOST memory, no GPU, in the same summation order: every pointer a host pointer,
 *                           T0 and out_transform (4, 4).  trace: NULL, or (max_iteration + 1, n) int64 whose row k receives evaluation k's
 *                           correspondence per source row; rows of evaluations not made are left untouched.
 *   se3_debug_icp_sincos_host   the series the point-to-plane update takes sin and cos from, on n HOST values of (-1, 1).
 *
 * Robust loss kernels and generalized ICP: the weighted entries.  se3_icp_stack and se3_debug_icp_host keep their signatures and every
 * output bit; they take no loss and refuse SE3_ICP_GENERALIZED.
 *   se3_icp_weighted_stack  se3_icp_stack with, in addition: src_normals (stacked source rows, 3) of src_normals_elem, read by
 *                           SE3_ICP_GENERALIZED alone (NULL otherwise); loss, one of SE3_ICP_LOSS_*; loss_k, the loss's width k (finite,
 *                           > 0; not read by NONE and L2); gicp_epsilon in (0, 1] (Open3D's default 1e-3; read by GENERALIZED alone).
 *                           Weights w(r) of a scalar residual r: L2 1; HUBER 1 for |r| <= k, else k / |r|; CAUCHY 1 / (1 + (r / k)^2);
 *                           GM k / (k + r^2)^2; TUKEY (1 - (r / k)^2)^2 for |r| <= k, else 0 (Open3D's RobustKernel; its L1Loss is not
 *                           offered: 1 / |r| is unbounded at an exact match, and HUBER covers its use).  NONE runs the instantiation
 *                           without weight code: for the two modes of se3_icp_stack, that entry's kernels and bits.
 *                           Point-to-plane: r = (p - q) . n, (sum w J^T J) x = -sum w J^T r, Open3D's TransformationEstimationPointToPlane
 *                           (kernel).  Point-to-point: r = sqrt(d^2) and a weighted Kabsch (weighted centroids and cross-covariance);
 *                           Open3D's point-to-point takes no kernel, so this is the project's definition; a weight sum that is not > 0
 *                           sets SE3_ICP_SINGULAR with the identity update.
 *                           SE3_ICP_GENERALIZED: Open3D's registration_generalized_icp with covariances I - (1 - eps) n n^T from the unit
 *                           normals of BOTH clouds (ref_normals and src_normals are required; their signs do not matter): with m = R
 *                           ns, M = 2 I - (1 - eps)(nt nt^T + m m^T), A = [-[p]_x | I], d = p - q: (sum w A^T M^-1 A) x = -sum w A^T M^-1 d,
 *                           solved, refused and applied as a point-to-plane step; at least 6 correspondences.  Its loss acts on the
 *                           Mahalanobis residual sqrt(d^T M^-1 d); Open3D weights the three rows of M^(-1/2) d one by one (the same
 *                           system under L2).  fitness and rmse stay Euclidean.  A non-finite source normal refuses the pair.
 *   se3_icp_weighted_workspace_bytes   its workspace (that of se3_icp_stack).
 *   se3_debug_icp_weighted_host   the same text for one pair on HOST memory, with the trace of se3_debug_icp_host. */
enum {                             /* (an enum, not limits: se3et_amd/ops.py reads the names and values from this block) */
  SE3_ICP_POINT_TO_POINT = 0,      /* mode */
  SE3_ICP_POINT_TO_PLANE = 1,
  SE3_ICP_NONFINITE = 1,           /* status bits */
  SE3_ICP_TOO_FEW = 2,
  SE3_ICP_SINGULAR = 4,
  SE3_ICP_EMPTY = 8,
  SE3_ICP_STEP_REFUSED = 16,
  SE3_ICP_MAX_ITERATION = 1000
};
size_t se3_icp_workspace_bytes(int64_t nsrc_total, int num_pairs);
int se3_icp_stack(const void* grid_workspace, size_t grid_workspace_bytes, int64_t nref_total, const void* src_points, int elem,
                  const int64_t* src_offsets_host, int num_pairs, const void* ref_normals, int normals_elem, const double* T0,
                  double max_correspondence_distance, int mode, double relative_fitness, double relative_rmse, int max_iteration,
                  double* out_transforms, double* out_fitness, double* out_rmse, int* out_iterations, int* out_converged, int* out_status,
                  int64_t* out_correspondences, void* workspace, size_t workspace_bytes, void* stream);
int se3_debug_icp_host(const void* src_points, int64_t n, const void* ref_points, int64_t nref, int elem, const void* ref_normals,
                       int normals_elem, const double* T0, double max_correspondence_distance, int mode, double relative_fitness,
                       double relative_rmse, int max_iteration, double* out_transform, double* out_fitness, double* out_rmse,
                       int* out_iterations, int* out_converged, int* out_status, int64_t* out_correspondences, int64_t* trace);
int se3_debug_icp_sincos_host(const double* x, int64_t n, double* out_sin, double* out_cos);
enum se3_icp_option {              /* (a NAMED enum: the binding reads it as a table of its own, beside the limits and the enum above) */
  SE3_ICP_GENERALIZED = 2,         /* mode, beside SE3_ICP_POINT_TO_POINT and SE3_ICP_POINT_TO_PLANE: the weighted entries alone */
  SE3_ICP_LOSS_NONE = -1,          /* loss */
  SE3_ICP_LOSS_L2 = 0,
  SE3_ICP_LOSS_HUBER = 1,
  SE3_ICP_LOSS_CAUCHY = 2,
  SE3_ICP_LOSS_GM = 3,
  SE3_ICP_LOSS_TUKEY = 4
};
size_t se3_icp_weighted_workspace_bytes(int64_t nsrc_total, int num_pairs);
int se3_icp_weighted_stack(const void* grid_workspace, size_t grid_workspace_bytes, int64_t nref_total, const void* src_points, int elem,
                           const int64_t* src_offsets_host, int num_pairs, const void* ref_normals, int normals_elem, const void* src_normals,
                           int src_normals_elem, const double* T0, double max_correspondence_distance, int mode, int loss, double loss_k,
                           double gicp_epsilon, double relative_fitness, double relative_rmse, int max_iteration, double* out_transforms,
                           double* out_fitness, double* out_rmse, int* out_iterations, int* out_converged, int* out_status,
                           int64_t* out_correspondences, void* workspace, size_t workspace_bytes, void* stream);
int se3_debug_icp_weighted_host(const void* src_points, int64_t n, const void* ref_points, int64_t nref, int elem, const void* ref_normals,
                                int normals_elem, const void* src_normals, int src_normals_elem, const double* T0,
                                double max_correspondence_distance, int mode, int loss, double loss_k, double gicp_epsilon,
                                double relative_fitness, double relative_rmse, int max_iteration, double* out_transform, double* out_fitness,
                                double* out_rmse, int* out_iterations, int* out_converged, int* out_status, int64_t* out_correspondences,
                                int64_t* trace);

/* ---- coloured ICP of stacked pairs (csrc/color_gradient.hip, csrc/icp.hip, csrc/icp_colored_core.h) ---------------------------------------------
 * Open3D's registration_colored_icp (Park, Zhou, Koltun, ICCV 2017) for up to SE3_PAIR_MAX_PAIRS stacked pairs per call, all float64 and
 * resident on the device: the colour gradients of the reference clouds once per call, then se3_icp_stack's loop with one more row per
 * correspondence; the contracts are the header comments of csrc/color_gradient.hip and csrc/icp.hip.  Points, normals and colours are
 * (rows, 3) on the device, float32 (elem 0) or float64 (elem 1), promoted on load; an intensity is ((c0 + c1) + c2) / 3.0.
 *   se3_color_gradient_stack   cloud c owns rows [offsets_host[c], offsets_host[c + 1]) (HOST int64, num_clouds + 1 entries from 0).
 *                           knn_idx (rows, k) int64 cloud-local and knn_d2 (rows, k) float64: se3_knn_stack's tables of the clouds searched
 *                           in themselves, k in [1, SE3_KNN_MAX] (Open3D's 30).  radius finite and >= 0: of a row's list the entries with
 *                           d^2 < radius^2 are its m members, the others of them than the row itself its neighbours.  out_gradients
 *                           (rows, 3) float64: the least-squares gradient of the intensity in the row's tangent plane (the neighbours
 *                           projected along the normal as given, the row (m - 1) n with right-hand side 0, a 3x3 Cholesky solve); zero for
 *                           m < 4 or a pivot not above 1e-13 of its diagonal entry.  status (num_clouds + 1) DEVICE int: zeroed, then bit 1
 *                           of word c for a non-finite point, normal or colour of cloud c, and of the last word for any; the rows of such
 *                           a cloud are not to be read.  One thread per row, no atomics.
 *   se3_debug_color_gradient_host   the same text for one cloud on HOST memory, no GPU, the list from se3_debug_knn_host's search: every
 *                           pointer a host pointer; *status: bit 1 as above (nothing is computed).
 *   se3_icp_colored_stack   se3_icp_stack's arguments with, in addition: src_colors (stacked source rows, 3) and ref_colors (nref_total, 3)
 *                           of their elems; ref_gradients (nref_total, 3) float64 from se3_color_gradient_stack over the reference clouds;
 *                           lambda_geometric in [0, 1] (Open3D's default 0.968); loss and loss_k as se3_icp_weighted_stack (NONE: no weight
 *                           code).  ref_normals is required.  With a = sqrt(lambda), b = sqrt(1 - lambda), p the moved source row, q its
 *                           reference row, nt, g, I_t that row's normal, gradient and intensity, I_s the source row's intensity:
 *                           r_g = a (p - q) . nt, J_g = a [p x nt, nt];  p' = p - ((p - q) . nt) nt, r_c = b (I_s - g . (p' - q) - I_t),
 *                           d = -(g - (nt . g) nt), J_c = b [p x d, d];  (sum w_g J_g J_g^T + w_c J_c J_c^T) x = -sum (w_g J_g r_g +
 *                           w_c J_c r_c), solved, refused and applied as a point-to-plane step.  Evaluation, loop, results and status bits
 *                           are se3_icp_stack's; TOO_FEW below 6 correspondences; a non-finite point, normal, colour, gradient or T0 sets
 *                           NONFINITE for that pair alone.
 *   se3_icp_colored_workspace_bytes   its workspace (that of se3_icp_stack).
 *   se3_debug_icp_colored_host   the same text for one pair on HOST memory, with the trace of se3_debug_icp_host. */
enum se3_icp_colored_option {      /* (a NAMED enum of its own: the mode tables of the entries above stay as they are) */
  SE3_ICP_COLORED = 3              /* mode, beside SE3_ICP_POINT_TO_POINT, SE3_ICP_POINT_TO_PLANE and SE3_ICP_GENERALIZED: the coloured entries alone */
};
int se3_color_gradient_stack(const void* points, int elem, const void* normals, int normals_elem, const void* colors, int colors_elem,
                             const int64_t* offsets_host, int num_clouds, const int64_t* knn_idx, const double* knn_d2, int k, double radius,
                             double* out_gradients, int* status, void* stream);
int se3_debug_color_gradient_host(const void* points, const void* normals, const void* colors, int64_t n, int elem, int normals_elem,
                                  int colors_elem, int k, double radius, double* out_gradients, int* status);
size_t se3_icp_colored_workspace_bytes(int64_t nsrc_total, int num_pairs);
int se3_icp_colored_stack(const void* grid_workspace, size_t grid_workspace_bytes, int64_t nref_total, const void* src_points, int elem,
                          const int64_t* src_offsets_host, int num_pairs, const void* ref_normals, int normals_elem, const void* src_colors,
                          int src_colors_elem, const void* ref_colors, int ref_colors_elem, const double* ref_gradients, const double* T0,
                          double max_correspondence_distance, double lambda_geometric, int loss, double loss_k, double relative_fitness,
                          double relative_rmse, int max_iteration, double* out_transforms, double* out_fitness, double* out_rmse,
                          int* out_iterations, int* out_converged, int* out_status, int64_t* out_correspondences, void* workspace,
                          size_t workspace_bytes, void* stream);
int se3_debug_icp_colored_host(const void* src_points, int64_t n, const void* ref_points, int64_t nref, int elem, const void* ref_normals,
                               int normals_elem, const void* src_colors, int src_colors_elem, const void* ref_colors, int ref_colors_elem,
                               const double* ref_gradients, const double* T0, double max_correspondence_distance, double lambda_geometric,
                               int loss, double loss_k, double relative_fitness, double relative_rmse, int max_iteration, double* out_transform,
                               double* out_fitness, double* out_rmse, int* out_iterations, int* out_converged, int* out_status,
                               int64_t* out_correspondences, int64_t* trace);

/* ---- keypoint selection: radius non-maximum suppression in score order (csrc/keypoint_nms.hip) -------------------------------------------------
 * The loop of the reference's sample_keypoints_with_nms / random_sample_keypoints_with_nms (utils/pointcloud.py:191-248) in an exact parallel
 * form, for up to SE3_PAIR_MAX_PAIRS stacked clouds per call, one workgroup per cloud; the contract is the header comment of
 * csrc/keypoint_nms.hip.  Cloud c owns rows [offsets_host[c], offsets_host[c + 1]) (HOST int64, num_clouds + 1 entries from 0 to n_total).
 *   se3_keypoint_nms_stack  grid_workspace: se3_pair_grid_build over the clouds themselves with identity transforms and cell_hint = radius
 *                           (n_total rows; the points are read from it).  order: DEVICE int64 per stacked row, cloud-local, rank -> index
 *                           (score descending, then index ascending: the caller's ranking).  max_keep: the number of keypoints wanted per
 *                           cloud, <= 0 for all survivors.  out_indices: DEVICE int64 sized n_total; cloud c's kept indices, cloud-local and
 *                           in rank order, start at offsets_host[c]; out_counts[c] (DEVICE int) of them are written.  status (DEVICE int): 0,
 *                           or bit 1 = a non-finite point, bit 2 = an order that is not a permutation of its cloud's rows (the clouds
 *                           concerned give no rows, and out_counts[c] holds MINUS their bits); read it with the counts.  radius must be
 *                           positive and finite; fewer than 2^31 rows per call.  A radius far above the point spacing is correct, slow.
 *   se3_debug_keypoint_nms_host   the same tile step for one cloud on HOST memory, no GPU: every pointer a host pointer, out_indices sized
 *                           n, *status as above (then *out_count = 0). */
size_t se3_keypoint_nms_workspace_bytes(int64_t n_total, int num_clouds);
int se3_keypoint_nms_stack(const void* grid_workspace, size_t grid_workspace_bytes, int64_t n_total, const int64_t* order,
                           const int64_t* offsets_host, int num_clouds, double radius, int max_keep, int64_t* out_indices, int* out_counts,
                           int* status, void* workspace, size_t workspace_bytes, void* stream);
int se3_debug_keypoint_nms_host(const void* points, int64_t n, int elem, const int64_t* order, double radius, int max_keep,
                                int64_t* out_indices, int64_t* out_count, int* status);

/* ---- FPFH descriptors of stacked clouds (csrc/fpfh.hip, csrc/fpfh_core.h) ----------------------------------------------------------------------
 * Open3D's compute_fpfh_feature (33 bins from point-pair angles over a point's neighbourhood) for up to SE3_PAIR_MAX_PAIRS stacked clouds per
 * call, all float64; the contract is the header comment of csrc/fpfh.hip.  Points and normals are (rows, 3) on the device, float32 (elem 0) or
 * float64 (elem 1), promoted on load; cloud c owns rows [offsets_host[c], offsets_host[c + 1]) (HOST int64, num_clouds + 1 entries from 0).
 * The neighbour list is the caller's, from the searches above: for the row slice [row_begin, row_begin + row_count) of the stacked rows,
 * row_offsets (row_count + 1) int64 on the DEVICE, from 0 to total, and pairs (total, 2) int64 on the DEVICE as se3_pair_ball_fill_stack
 * leaves them: slice row r owns pairs[row_offsets[r] .. row_offsets[r + 1]), column 1 the neighbour's cloud-local index, ascending within a
 * row; an entry equal to the row's own index is skipped.  A slice bounds the list's memory; the output arrays are those of the whole call.
 *   se3_fpfh_check_stack    status (num_clouds + 1) DEVICE int: zeroed, then bit 1 of word c for a non-finite point or normal of cloud c, and
 *                           of the last word for any.  (A list entry outside its cloud, or row offsets outside the list, are skipped by
 *                           both passes: nothing is read through them.)
 *   se3_spfh_stack          out_spfh (n_total, 33) float64: the slice's rows, bin count x (100 / m); theta at 0-10, f1 at 11-21, f2 at 22-32.
 *   se3_fpfh_stack          out_fpfh (n_total, 33) float64: the slice's rows from spfh (n_total, 33), which must hold every row of the clouds
 *                           the slice touches.
 *   se3_debug_fpfh_host     the same text for one cloud on HOST memory, no GPU, in the same summation order: every pointer a host pointer,
 *                           the list over all n rows; *status: bit 1 as above (nothing is computed), bit 2 for a list entry or row offsets that were skipped.
 *   se3_debug_fpfh_sectors_host   the twenty constants of the sector rule: out[2 (k - 1)] = cos, out[2 (k - 1) + 1] = sin of
 *                           -pi + 2 pi k / 11, k = 1 .. 10. */
int se3_fpfh_check_stack(const void* points, int elem, const void* normals, int normals_elem, const int64_t* offsets_host, int num_clouds,
                         int* status, void* stream);
int se3_spfh_stack(const void* points, int elem, const void* normals, int normals_elem, const int64_t* offsets_host, int num_clouds,
                   int64_t row_begin, int64_t row_count, const int64_t* row_offsets, const int64_t* pairs, int64_t total, double* out_spfh,
                   void* stream);
int se3_fpfh_stack(const void* points, int elem, const double* spfh, const int64_t* offsets_host, int num_clouds, int64_t row_begin,
                   int64_t row_count, const int64_t* row_offsets, const int64_t* pairs, int64_t total, double* out_fpfh, void* stream);
int se3_debug_fpfh_host(const void* points, const void* normals, int64_t n, int elem, int normals_elem, const int64_t* row_offsets,
                        const int64_t* pairs, int64_t total, double* out_spfh, double* out_fpfh, int* status);
int se3_debug_fpfh_sectors_host(double* out);

/* ---- ISS keypoints of stacked clouds (csrc/iss.hip, csrc/iss_core.h, csrc/cov3.h) ---------------------------------------------------------------
 * Open3D's compute_iss_keypoints (the eigenvalue ratios of a neighbourhood's scatter matrix, a radius non-maximum test on the smallest
 * eigenvalue) for up to SE3_PAIR_MAX_PAIRS stacked clouds per call, all float64; the contract is the header comment of csrc/iss.hip.  Points are
 * (rows, 3) on the device, float32 (elem 0) or float64 (elem 1), promoted on load; cloud c owns rows [offsets_host[c], offsets_host[c + 1])
 * (HOST int64, num_clouds + 1 entries from 0).  The finite check of the points is se3_fpfh_check_stack with the points in both places.
 *   se3_iss_saliency_stack  out_saliency (n_total) float64: rows [row_begin, row_begin + row_count) from their ball lists at salient_radius,
 *                           row_offsets (row_count + 1, from 0) and pairs (total, 2) int64 as the ball query's count and fill calls leave
 *                           them (members ascending within a row; only column 1 is read; an entry outside its cloud zeroes the row).
 *                           gamma_21, gamma_32 positive and finite, min_neighbors >= 1.
 *   se3_iss_select_stack    out_mask (n_total) bytes: 1 for a keypoint, on a grid built by se3_pair_grid_build over the clouds themselves
 *                           (identity transforms, cell_hint = the largest radius); radii_host (num_clouds) float64 on the HOST: each
 *                           cloud's non_max_radius, finite and >= 0; saliency (n_total) as the first pass left it.
 *   se3_debug_iss_host      the same text for one cloud on HOST memory, no GPU, in the same summation order: every pointer a host pointer.
 *                           out_eigenvalues (n, 3: l1 >= l2 >= l3, zeros without a member or for C = 0) and out_counts (n, 2: the member
 *                           counts at the two radii) may be NULL; *status: 0, or bit 1 for a non-finite point (nothing is computed). */
int se3_iss_saliency_stack(const void* points, int elem, const int64_t* offsets_host, int num_clouds, int64_t row_begin, int64_t row_count,
                           const int64_t* row_offsets, const int64_t* pairs, int64_t total, double gamma_21, double gamma_32, int min_neighbors,
                           double* out_saliency, void* stream);
int se3_iss_select_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                         const int64_t* q_offsets_host, int num_clouds, const double* radii_host, const double* saliency, int min_neighbors,
                         uint8_t* out_mask, void* stream);
int se3_debug_iss_host(const void* points, int64_t n, int elem, double salient_radius, double non_max_radius, double gamma_21, double gamma_32,
                       int min_neighbors, double* out_saliency, double* out_eigenvalues, int64_t* out_counts, uint8_t* out_mask, int* status);

/* ---- outlier removal and model resolution of stacked clouds (csrc/outliers.hip, csrc/outliers_core.h, csrc/fixed_sum.h) -----------------------
 * Open3D's remove_statistical_outlier for up to SE3_PAIR_MAX_PAIRS stacked clouds per call, all float64; the contract is the header comment of
 * csrc/outliers.hip.  (remove_radius_outlier is se3_pair_grid_build and se3_pair_ball_count_stack: a row is kept iff its count > nb_points.)
 *   se3_knn_distance_stack  out (nq) float64 on a grid built over the clouds themselves (identity transforms, cell_hint 0), from each row's
 *                           k nearest (k in [1, SE3_KNN_MAX]): column < 0: (the sum of the roots of the list's d^2 in list order) / the
 *                           list's length; column in [0, k): the root of that column, 0 where the list is shorter.
 *   se3_distance_stats_stack   out_stats (num_clouds, 4) float64: mean, std, thr = mean + std_ratio std, model resolution, from the row
 *                           values a (n_total) in the fixed summation shape of csrc/fixed_sum.h; out_mask (n_total) bytes: a > 0 and
 *                           a < thr.  std_ratio positive and finite.
 *   se3_debug_*_host        the same text for one cloud on HOST memory, no GPU: every pointer a host pointer; out_mask may be NULL. */
int se3_knn_distance_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                           const int64_t* q_offsets_host, int num_clouds, int k, int column, double* out, void* stream);
int se3_distance_stats_stack(const double* a, const int64_t* offsets_host, int num_clouds, double std_ratio, double* out_stats, uint8_t* out_mask,
                             void* stream);
int se3_debug_knn_distance_host(const void* points, int64_t n, int elem, int k, int column, double* out);
int se3_debug_distance_stats_host(const double* a, int64_t n, double std_ratio, double* out_stats, uint8_t* out_mask);

/* ---- Fast Global Registration of stacked pairs (csrc/fgr.hip, csrc/fgr_core.h) ------------------------------------------------------------------
 * Open3D's registration_fgr_based_on_correspondence (Zhou, Park, Koltun, ECCV 2016: the tuple test, then graduated non-convexity over the
 * kept correspondences, 6x6 Gauss-Newton steps) for up to SE3_PAIR_MAX_PAIRS stacked pairs per call, all float64, three launches and no
 * host round trip; the contract is the header comment of csrc/fgr.hip.  Points are (rows, 3) on the device, float32 (elem 0) or float64
 * (elem 1), promoted on load; pair p owns the source rows [src_offsets_host[p], src_offsets_host[p + 1]), the reference rows and the
 * correspondences likewise (HOST int64, num_pairs + 1 entries from 0).  correspondences: DEVICE (K_total, 2) int64 rows of pair-local
 * (source row, reference row), at most SE3_FGR_MAX_CORRESPONDENCES per pair (100 K trials stay below 2^31).
 *   se3_fgr_stack           maximum_correspondence_distance finite and > 0 (compared with mu: in normalised units unless
 *                           use_absolute_scale); division_factor finite and >= 1; iteration_number in [0, SE3_FGR_MAX_ITERATION];
 *                           tuple_scale in (0, 1]; maximum_tuple_count in [0, SE3_FGR_MAX_TUPLE_COUNT].  out_transforms (P, 4, 4)
 *                           float64, ref ~ T src; out_status: a sum of SE3_FGR_* bits -- NONFINITE (a non-finite coordinate: NaN
 *                           transform), BAD_INDEX (a correspondence outside its cloud: NaN transform), EMPTY (an empty cloud or K = 0:
 *                           identity), TOO_FEW (|C'| < 10: identity), SINGULAR (a scale that is not > 0: identity; or a 6x6 system that is
 *                           not positive definite: that step is the identity), STEP_REFUSED (a step angle that is not finite or of 4 rad and
 *                           more: the pair ends with what it has); out_num_correspondences |C'|; out_num_tuples the accepted trials that
 *                           were kept (0 without the tuple test).  Optional (NULL): out_mu (P) the last mu; out_tuples
 *                           (P, 3 maximum_tuple_count, 2) int64, pair p's C' in its first out_num_correspondences[p] rows (written by the
 *                           tuple test alone); out_trials (P, maximum_tuple_count) int64, the kept trials' indices.  Every output is on the
 *                           DEVICE; nothing waits on the host.  workspace: se3_fgr_workspace_bytes.
 *   se3_debug_fgr_host      the same text for one pair on HOST memory, no GPU, run serially over the lanes: every pointer a host pointer.
 *   se3_debug_fgr_sincos_host   the sine and cosine of the update, on n HOST values of (-4, 4): the series of the ICP update at a / 4
 *                           and two double-angle steps. */
enum se3_fgr_status {              /* (a NAMED enum: the binding reads it as a table of its own; the shared names carry ICP's values) */
  SE3_FGR_NONFINITE = 1,
  SE3_FGR_TOO_FEW = 2,
  SE3_FGR_SINGULAR = 4,
  SE3_FGR_EMPTY = 8,
  SE3_FGR_STEP_REFUSED = 16,
  SE3_FGR_BAD_INDEX = 32
};
enum se3_fgr_limit {               /* (NAMED too: the flat table of #defines and anonymous enumerators stays as it is) */
  SE3_FGR_MAX_ITERATION = 1000,
  SE3_FGR_MAX_CORRESPONDENCES = 21474836,   /* per pair: 100 K trials stay below 2^31 */
  SE3_FGR_MAX_TUPLE_COUNT = 1000000,
  SE3_FGR_TUPLE_CHUNK = 256,       /* trials per step of the tuple test */
  SE3_FGR_MAX_ANGLE = 4            /* rad */
};
size_t se3_fgr_workspace_bytes(int num_pairs, int maximum_tuple_count, int tuple_test);
int se3_fgr_stack(const void* src_points, int src_elem, const int64_t* src_offsets_host, const void* ref_points, int ref_elem,
                  const int64_t* ref_offsets_host, const int64_t* correspondences, const int64_t* corr_offsets_host, int num_pairs,
                  double maximum_correspondence_distance, double division_factor, int use_absolute_scale, int decrease_mu,
                  int iteration_number, double tuple_scale, int maximum_tuple_count, int tuple_test, uint64_t seed, double* out_transforms,
                  int* out_status, int* out_num_correspondences, int* out_num_tuples, double* out_mu, int64_t* out_tuples,
                  int64_t* out_trials, void* workspace, size_t workspace_bytes, void* stream);
int se3_debug_fgr_host(const void* src_points, int64_t ns, int src_elem, const void* ref_points, int64_t nr, int ref_elem,
                       const int64_t* correspondences, int64_t num_correspondences, double maximum_correspondence_distance,
                       double division_factor, int use_absolute_scale, int decrease_mu, int iteration_number, double tuple_scale,
                       int maximum_tuple_count, int tuple_test, uint64_t seed, double* out_transform, int* out_status,
                       int* out_num_correspondences, int* out_num_tuples, double* out_mu, int64_t* out_tuples, int64_t* out_trials);
int se3_debug_fgr_sincos_host(const double* x, int64_t n, double* out_sin, double* out_cos);

/* ---- Multiway registration: information matrices and pose graphs (csrc/pose_graph.hip, csrc/pose_graph_core.h) ------------------------------
 * Open3D's get_information_matrix_from_point_clouds and global_optimization (GlobalOptimization.cpp: Levenberg-Marquardt with a line
 * process, pruning, a second optimisation) for up to SE3_PAIR_MAX_PAIRS stacked pairs / graphs per call, all float64, nothing read back;
 * the contract is the header comment of csrc/pose_graph.hip.
 *   se3_pair_information_stack   grid: se3_pair_grid_build over the REFERENCE clouds with identity transforms and cell_hint = the
 *                           correspondence distance; src_points (rows, 3) float32 (elem 0) / float64 (elem 1) on the device, pair p on
 *                           rows [src_offsets_host[p], src_offsets_host[p + 1]); transforms (P, 4, 4) float64 on the DEVICE, ref ~ T src.
 *                           out_information (P, 6, 6) float64, out_count (P) float64 (= information[5][5]), out_status (P): NONFINITE (a NaN
 *                           matrix) or EMPTY (the zero matrix).  workspace: se3_pair_information_workspace_bytes.
 *   se3_debug_pair_information_host   the same text for one pair on HOST memory; out_correspondences (n) int64 or NULL: the reference row of
 *                           every source row, -1 for none.
 *   se3_pose_graph_optimize_stack   graph g owns the nodes [node_offsets_host[g], node_offsets_host[g + 1]) of poses (nodes, 4, 4) and the
 *                           edges [edge_offsets_host[g], ..) of edges (E, 2) int64 graph-local (source node, target node), transforms
 *                           (E, 4, 4), informations (E, 6, 6), uncertain (E) bytes, all on the DEVICE; at most SE3_PGO_MAX_NODES nodes and
 *                           SE3_PGO_MAX_EDGES edges per graph.  reference_nodes_host (num_graphs) HOST ints, -1 for none, or NULL for none
 *                           at all.  max_iteration in [0, SE3_PGO_MAX_ITERATION], max_iteration_lm in [0, SE3_PGO_MAX_ITERATION_LM]; the
 *                           doubles are checked on the device (a non-finite one refuses every graph: NONFINITE).  One workgroup of 256
 *                           threads per graph, one launch.  out_poses (nodes, 4, 4); out_confidence (2, E) the line process after each pass
 *                           (a pruned edge has 0 in the second row); out_kept (E) bytes; out_status (G) a sum of SE3_PGO_* bits; out_info
 *                           (G, 6) ints: stop reason, iterations, trials of pass 1, then of pass 2; out_residuals (G, 2) the accepted
 *                           residual of each pass.  workspace: se3_pose_graph_workspace_bytes of the same offsets (0 for
 *                           offsets or sizes that the call would refuse).
 *   se3_debug_pose_graph_host   the same text for one graph on HOST memory, run serially over the lanes.  trace: NULL, or (trace_rows, 4)
 *                           float64: per trial lambda, rho, accepted (1 / 0), the trial's residual (NaN where none was formed);
 *                           out_trace_count (2): the trials of each pass that were written, pass 2's after pass 1's.
 *   se3_debug_pgo_atan2_host   the residual's arc tangent on n HOST pairs (y, x). */
enum se3_pgo_status {              /* (NAMED: the shared names carry ICP's and FGR's values) */
  SE3_PGO_NONFINITE = 1,
  SE3_PGO_SINGULAR = 4,
  SE3_PGO_EMPTY = 8,
  SE3_PGO_STEP_REFUSED = 16,
  SE3_PGO_BAD_INDEX = 32
};
enum se3_pgo_limit {
  SE3_PGO_MAX_NODES = 64,
  SE3_PGO_MAX_EDGES = 2016,        /* the complete graph on 64 nodes */
  SE3_PGO_MAX_ITERATION = 1000,
  SE3_PGO_MAX_ITERATION_LM = 100,
  SE3_PGO_MAX_ANGLE = 4            /* rad: FGR's sine and cosine */
};
enum se3_pgo_stop {                /* why a pass ended: the first test that fired */
  SE3_PGO_STOP_NONE = 0,
  SE3_PGO_STOP_RIGHT_TERM = 1,
  SE3_PGO_STOP_RELATIVE_INCREMENT = 2,
  SE3_PGO_STOP_RELATIVE_RESIDUAL = 3,
  SE3_PGO_STOP_RESIDUAL = 4,
  SE3_PGO_STOP_MAX_ITERATION = 5,
  SE3_PGO_STOP_MAX_ITERATION_LM = 6,
  SE3_PGO_STOP_REFUSED = 7
};
size_t se3_pair_information_workspace_bytes(int64_t nsrc_total, int num_pairs);
int se3_pair_information_stack(const void* grid_workspace, size_t grid_workspace_bytes, int64_t nref_total, const void* src_points, int elem,
                               const int64_t* src_offsets_host, int num_pairs, const double* transforms, double max_correspondence_distance,
                               double* out_information, double* out_count, int* out_status, void* workspace, size_t workspace_bytes,
                               void* stream);
int se3_debug_pair_information_host(const void* src_points, int64_t n, const void* ref_points, int64_t nref, int elem, const double* transform,
                                    double max_correspondence_distance, double* out_information, double* out_count, int* out_status,
                                    int64_t* out_correspondences);
size_t se3_pose_graph_workspace_bytes(const int64_t* node_offsets_host, const int64_t* edge_offsets_host, int num_graphs);
int se3_pose_graph_optimize_stack(const double* poses, const int64_t* node_offsets_host, const int64_t* edges, const double* transforms,
                                  const double* informations, const uint8_t* uncertain, const int64_t* edge_offsets_host, int num_graphs,
                                  const int* reference_nodes_host, int max_iteration, int max_iteration_lm, double min_relative_increment,
                                  double min_relative_residual_increment, double min_right_term, double min_residual,
                                  double upper_scale_factor, double lower_scale_factor, double max_correspondence_distance,
                                  double edge_prune_threshold, double preference_loop_closure, double* out_poses, double* out_confidence,
                                  uint8_t* out_kept, int* out_status, int* out_info, double* out_residuals, void* workspace,
                                  size_t workspace_bytes, void* stream);
int se3_debug_pose_graph_host(const double* poses, int64_t num_nodes, const int64_t* edges, const double* transforms,
                              const double* informations, const uint8_t* uncertain, int64_t num_edges, int reference_node, int max_iteration,
                              int max_iteration_lm, double min_relative_increment, double min_relative_residual_increment,
                              double min_right_term, double min_residual, double upper_scale_factor, double lower_scale_factor,
                              double max_correspondence_distance, double edge_prune_threshold, double preference_loop_closure,
                              double* out_poses, double* out_confidence, uint8_t* out_kept, int* out_status, int* out_info,
                              double* out_residuals, double* trace, int64_t trace_rows, int* out_trace_count);
int se3_debug_pgo_atan2_host(const double* y, const double* x, int64_t n, double* out);

/* ---- Plane segmentation and DBSCAN clustering of stacked clouds (csrc/plane.hip, csrc/plane_core.h, csrc/dbscan.hip, csrc/dbscan_core.h) ------
 * Open3D's segment_plane and cluster_dbscan for up to SE3_PAIR_MAX_PAIRS stacked clouds per call, float64, nothing read back; the contracts
 * are the header comments of csrc/plane.hip and csrc/dbscan.hip.  points (rows, 3) float32 (elem 0) / float64 (elem 1) on the device, cloud
 * c on rows [offsets_host[c], offsets_host[c + 1]) (HOST int64, num_clouds + 1 entries from 0).
 *   se3_plane_segment_stack   distance_threshold positive and finite, ransac_n in [3, SE3_PLANE_MAX_SAMPLE], num_iterations in
 *                           [1, SE3_PLANE_MAX_ITERATIONS].  out_planes (P, 4) float64 (a, b, c, d), out_mask (rows) bytes: 1 for an inlier of
 *                           the returned plane, out_counts (P) ints, out_fitness and out_rmse (P) float64, out_status (P): SE3_PLANE_OK,
 *                           SE3_PLANE_TOO_FEW (fewer than ransac_n rows) or SE3_PLANE_NONE (no hypothesis with 3 inliers), out_best (P) the
 *                           winning hypothesis, -1 for none.  Optional (both or neither NULL): out_hyp_counts (P, num_iterations) ints and
 *                           out_hyp_errs (P, num_iterations) float64, every hypothesis' inlier count and error sum.  Every output is on
 *                           the DEVICE.  workspace: se3_plane_segment_workspace_bytes of the same offsets (0 for what the call refuses).
 *   se3_dbscan_stack        grid: se3_pair_grid_build over the clouds themselves with identity transforms and cell_hint = eps (ns_total =
 *                           the rows of the clouds).  eps positive and finite, min_points >= 1.  out_labels (rows) ints: -1 noise, clusters
 *                           0 .. k - 1 per cloud; out_num_clusters (P) int64.  workspace: se3_dbscan_workspace_bytes(rows).
 *   se3_debug_plane_host / se3_debug_dbscan_host   the same text for one cloud on HOST memory, no GPU, run serially over the lanes: every
 *                           pointer a host pointer. */
enum se3_plane_status {            /* (NAMED: the flat table of #defines and anonymous enumerators stays as it is) */
  SE3_PLANE_OK = 0,
  SE3_PLANE_TOO_FEW = 2,
  SE3_PLANE_NONE = 64
};
enum se3_plane_limit {
  SE3_PLANE_MAX_SAMPLE = 16,       /* ransac_n at most */
  SE3_PLANE_TILE = 128,            /* hypotheses per scoring workgroup */
  SE3_PLANE_SEGMENT = 1024,        /* rows per segment of the error sum */
  SE3_PLANE_MAX_ITERATIONS = 1048576
};
size_t se3_plane_segment_workspace_bytes(const int64_t* offsets_host, int num_clouds, int num_iterations);
int se3_plane_segment_stack(const void* points, int elem, const int64_t* offsets_host, int num_clouds, double distance_threshold, int ransac_n,
                            int num_iterations, uint64_t seed, double* out_planes, uint8_t* out_mask, int* out_counts, double* out_fitness,
                            double* out_rmse, int* out_status, int* out_best, int* out_hyp_counts, double* out_hyp_errs, void* workspace,
                            size_t workspace_bytes, void* stream);
int se3_debug_plane_host(const void* points, int64_t n, int elem, double distance_threshold, int ransac_n, int num_iterations, uint64_t seed,
                         double* out_plane, uint8_t* out_mask, int* out_count, double* out_fitness, double* out_rmse, int* out_status,
                         int* out_best, int* out_hyp_counts, double* out_hyp_errs);
size_t se3_dbscan_workspace_bytes(int64_t n_total);
int se3_dbscan_stack(const void* grid_workspace, size_t grid_workspace_bytes, int64_t ns_total, const void* points, int elem,
                     const int64_t* offsets_host, int num_clouds, double eps, int64_t min_points, int* out_labels, int64_t* out_num_clusters,
                     void* workspace, size_t workspace_bytes, void* stream);
int se3_debug_dbscan_host(const void* points, int64_t n, int elem, double eps, int64_t min_points, int* out_labels, int64_t* out_num_clusters);

/* ---- TSDF fusion of depth frames and depth images as clouds (csrc/tsdf.hip, csrc/tsdf_core.h) ---------------------------------------------------
 * Open3D's UniformTSDFVolume (integrate, extract_point_cloud) for up to SE3_PAIR_MAX_PAIRS volumes per call, and the reference's
 * convert_depth_mat_to_points / Open3D's create_from_depth_image for any number of images; the contract is the header comment of
 * csrc/tsdf.hip.  A volume is resolution^3 voxels, planar, voxel [x, y, z] at (x R + y) R + z: tsdf and weight (V, R, R, R) float32, color
 * (V, 3, R, R, R) float32 or NULL, origins (V, 3) float64, all on the DEVICE.
 *   se3_tsdf_integrate_stack  depths (F, H, W) uint16 (depth_elem 0) / float32 (1); colors NULL (color_elem 0), (F, H, W, 3) uint8 (1) /
 *                           float32 (2), required exactly when color is given; frames (F, SE3_TSDF_FRAME_WORDS) float32: the 3 x 4
 *                           world-to-camera extrinsic by rows, then fx, fy, cx, cy; volume v takes the frames [frame_offsets_host[v],
 *                           frame_offsets_host[v + 1]) in ascending order (HOST int64, V + 1 entries from 0).  One launch: every voxel is
 *                           read once and written once, and only where a frame touched it.
 *   se3_tsdf_extract_stack  two passes over the same state.  out_points NULL: the count pass and the scan; row_offsets (V R R + 1) int64
 *                           becomes the exclusive offsets of the rows (v, x, y) and the total.  Otherwise the write pass: out_points,
 *                           out_normals and (with color) out_colors (capacity, 3) float64, volume v's rows at [row_offsets[v R R],
 *                           row_offsets[(v + 1) R R]); nothing is written at or past `capacity`.
 *   se3_depth_points_stack  the same two passes over the rows of F images: row_offsets (F H + 1) int64; intrinsics (F, 4) float64 (fx, fy,
 *                           cx, cy) on the device; convention SE3_DEPTH_REFERENCE or SE3_DEPTH_OPEN3D.
 *   se3_debug_tsdf_integrate_host / se3_debug_tsdf_extract_host / se3_debug_depth_points_host   the same text for one volume / one image on
 *                           HOST memory, no GPU, serially: every pointer a host pointer.  out_points NULL: *out_count alone. */
enum se3_tsdf_limit {              /* (NAMED) */
  SE3_TSDF_MIN_RESOLUTION = 4,
  SE3_TSDF_MAX_RESOLUTION = 1024,
  SE3_TSDF_MAX_IMAGE = 8192,       /* height and width of an image at most */
  SE3_TSDF_MAX_TRUNC_VOXELS = 64,  /* sdf_trunc in (0, this many voxel lengths] */
  SE3_TSDF_FRAME_TILE = 64,        /* frames of the table staged through LDS at a time */
  SE3_TSDF_FRAME_WORDS = 16        /* float32 words of a frame's row of the table */
};
enum se3_depth_convention {
  SE3_DEPTH_REFERENCE = 0,
  SE3_DEPTH_OPEN3D = 1
};
int se3_tsdf_integrate_stack(float* tsdf, float* weight, float* color, int num_volumes, int resolution, double voxel_length, double sdf_trunc,
                             const double* origins, const void* depths, int depth_elem, const void* colors, int color_elem, int height,
                             int width, const float* frames, const int64_t* frame_offsets_host, double depth_scale, double depth_trunc,
                             void* stream);
int se3_tsdf_extract_stack(const float* tsdf, const float* weight, const float* color, int num_volumes, int resolution, double voxel_length,
                           const double* origins, int64_t* row_offsets, int64_t capacity, double* out_points, double* out_normals,
                           double* out_colors, void* stream);
int se3_depth_points_stack(const void* depths, int depth_elem, int64_t num_images, int height, int width, const double* intrinsics,
                           double scaling_factor, double distance_limit, int convention, int64_t* row_offsets, int64_t capacity,
                           double* out_points, void* stream);
int se3_debug_tsdf_integrate_host(float* tsdf, float* weight, float* color, int resolution, double voxel_length, double sdf_trunc,
                                  const double* origin, const void* depths, int depth_elem, const void* colors, int color_elem,
                                  int64_t num_frames, int height, int width, const float* frames, double depth_scale, double depth_trunc);
int se3_debug_tsdf_extract_host(const float* tsdf, const float* weight, const float* color, int resolution, double voxel_length,
                                const double* origin, int64_t capacity, double* out_points, double* out_normals, double* out_colors,
                                int64_t* out_count);
int se3_debug_depth_points_host(const void* depth, int depth_elem, int height, int width, const double* intrinsics, double scaling_factor,
                                double distance_limit, int convention, int64_t capacity, double* out_points, int64_t* out_count);

/* ---- block-sparse TSDF volumes (csrc/tsdf_sparse.hip, csrc/tsdf_sparse_core.h) ---------------------------------------------------------------------
 * Open3D's ScalableTSDFVolume (integrate, extract_point_cloud) for up to SE3_PAIR_MAX_PAIRS volumes per object; the contract is the header
 * comment of csrc/tsdf_sparse.hip.  A block is SE3_STSDF_BLOCK^3 voxels; the storage is tsdf, weight (S, 16, 16, 16) float32 and color
 * (S, 3, 16, 16, 16) float32 or NULL in slots; the directory is the blocks' int64 keys, ascending (5 bits of volume above 3 x
 * SE3_STSDF_COORD_BITS bits of coordinate + 2^18), with each block's slot (int).  Everything on the DEVICE unless it is called _host.
 *   se3_stsdf_touch_groups   the pixel tiles of a call: the length of group_offsets is this + 1 (0 for sizes that the call would refuse).
 *   se3_stsdf_touch_stack    depths (F, H, W) uint16 (depth_elem 0) / float32 (1); poses (F, SE3_STSDF_POSE_WORDS) float64: the 3 x 4
 *                           camera-to-world pose by rows, then fx, fy, cx, cy; volume v owns the frames [frame_offsets_host[v],
 *                           frame_offsets_host[v + 1]) (HOST int64).  out_keys NULL: the count pass and the scan; group_offsets becomes the
 *                           exclusive offsets of the tiles and the total; bad_frames (F) ints, zeroed by the caller, gets a 1 for every
 *                           frame that touches a block coordinate out of range.  Otherwise the write pass: the (key, frame) records of
 *                           tile g at [group_offsets[g], group_offsets[g + 1]), in frame order, nothing at or past `capacity`.  The records
 *                           are a multiset: the caller sorts them (stably, by key) and drops duplicates.
 *   se3_stsdf_neighbors      out_neighbors (B, 27) ints: the slot of block b + d at [(dx + 1) 9 + (dy + 1) 3 + (dz + 1)], -1 where absent.
 *   se3_stsdf_integrate_stack  the touched blocks' keys and slots (num_blocks) and their frame lists in CSR form: block i takes the frames
 *                           block_frames[block_frame_offsets[i], block_frame_offsets[i + 1]) (indices among the call's images, ascending)
 *                           with the frame table of se3_tsdf_integrate_stack.  A slot outside [0, num_slots) is not touched.
 *   se3_stsdf_extract_stack  two passes, as se3_tsdf_extract_stack: group_offsets (16 B + 1) int64 over the groups (block, x) in key order.
 *   se3_debug_stsdf_*_host   the same text on HOST memory, serially: every pointer a host pointer.  The touch entry returns the records
 *                           sorted by (key, frame) without duplicates (out_keys NULL: *out_count alone) and *out_bad_frame, the first
 *                           frame out of range or -1; the extract entry finds the neighbours itself and returns the blocks' offsets
 *                           (B + 1) (out_points NULL: those alone). */
enum se3_stsdf_limit {             /* (NAMED) */
  SE3_STSDF_BLOCK = 16,            /* voxels per block side */
  SE3_STSDF_COORD_BITS = 19,       /* a block coordinate lies in [-2^18, 2^18) */
  SE3_STSDF_MAX_TRUNC_VOXELS = 16, /* sdf_trunc in (0, this many voxel lengths]: one block at most */
  SE3_STSDF_MAX_STRIDE = 64,       /* largest allocation stride */
  SE3_STSDF_POSE_WORDS = 16        /* float64 words of a frame's row of the pose table */
};
int64_t se3_stsdf_touch_groups(int64_t num_frames, int height, int width, int stride);
int se3_stsdf_touch_stack(const void* depths, int depth_elem, int64_t num_frames, int height, int width, const double* poses,
                          const int64_t* frame_offsets_host, int num_volumes, double voxel_length, double sdf_trunc, int stride,
                          double depth_scale, double depth_trunc, int64_t* group_offsets, int* bad_frames, int64_t capacity, int64_t* out_keys,
                          int* out_frames, void* stream);
int se3_stsdf_neighbors(const int64_t* keys, const int* slots, int64_t num_blocks, int* out_neighbors, void* stream);
int se3_stsdf_integrate_stack(float* tsdf, float* weight, float* color, int64_t num_slots, const int64_t* block_keys, const int* block_slots,
                              int64_t num_blocks, const int64_t* block_frame_offsets, const int* block_frames, double voxel_length,
                              double sdf_trunc, const void* depths, int depth_elem, const void* colors, int color_elem, int64_t num_frames,
                              int height, int width, const float* frames, double depth_scale, double depth_trunc, void* stream);
int se3_stsdf_extract_stack(const float* tsdf, const float* weight, const float* color, const int64_t* keys, const int* neighbors,
                            int64_t num_blocks, double voxel_length, int64_t* group_offsets, int64_t capacity, double* out_points,
                            double* out_normals, double* out_colors, void* stream);
int se3_debug_stsdf_touch_host(const void* depths, int depth_elem, int64_t num_frames, int height, int width, const double* poses,
                               const int64_t* frame_offsets, int num_volumes, double voxel_length, double sdf_trunc, int stride,
                               double depth_scale, double depth_trunc, int64_t capacity, int64_t* out_keys, int* out_frames, int64_t* out_count,
                               int64_t* out_bad_frame);
int se3_debug_stsdf_integrate_host(float* tsdf, float* weight, float* color, int64_t num_slots, const int64_t* block_keys,
                                   const int* block_slots, int64_t num_blocks, const int64_t* block_frame_offsets, const int* block_frames,
                                   double voxel_length, double sdf_trunc, const void* depths, int depth_elem, const void* colors,
                                   int color_elem, int64_t num_frames, int height, int width, const float* frames, double depth_scale,
                                   double depth_trunc);
int se3_debug_stsdf_extract_host(const float* tsdf, const float* weight, const float* color, const int64_t* keys, const int* slots,
                                 int64_t num_blocks, double voxel_length, int64_t capacity, double* out_points, double* out_normals,
                                 double* out_colors, int64_t* out_block_offsets);

/* ---- RGB-D odometry of frame pairs (csrc/rgbd_odometry.hip, csrc/rgbd_odometry_core.h) -----------------------------------------------------------
 * Open3D's legacy ComputeRGBDOdometry (hybrid and colour Jacobians) with CreateInformationMatrix for up to SE3_PAIR_MAX_PAIRS pairs of frames
 * per call, nothing read back; the contract is the header comment of csrc/rgbd_odometry.hip.  Frames are the unit of preparation: a call
 * prepares the pyramids of all F frames once, and pairs name frames.
 *   se3_rgbd_odometry_stack   depths (F, H, W) uint16 (depth_elem 0) / float32 (1); colors (F, H, W, color_channels) uint8 (color_elem 1) /
 *                           float32 (2), color_channels 3 or 1; target_flags (F) bytes on the DEVICE: 1 for a frame that is some pair's
 *                           target (it gets Sobel images).  prepare 1: the pyramids are built into frames_workspace first; 0: they are
 *                           there from an earlier call with the same frames (the next chunk of pairs).  pairs_host (P, 2) HOST ints
 *                           (source frame, target frame), intrinsics_host (P, 4) HOST float64 (fx, fy, cx, cy) of level 0,
 *                           init_transforms (P, 4, 4) float64 on the DEVICE, iterations_host (num_levels) HOST ints, coarsest level first.
 *                           out_transforms (P, 4, 4) source camera to target camera, out_success (P) bytes, out_status (P) a sum of
 *                           SE3_RGBD_* bits, out_information (P, 6, 6), out_count (P) int64, all on the DEVICE.  The whole schedule is
 *                           issued on `stream`: 3 launches per iteration.  Workspaces: se3_rgbd_frames_workspace_bytes and
 *                           se3_rgbd_pairs_workspace_bytes (0 for sizes that the call would refuse).
 *   se3_debug_rgbd_odometry_host   the same text on HOST memory, serially, any number of pairs up to SE3_PAIR_MAX_PAIRS.  stop: SE3_RGBD_STOP_*;
 *                           PREPARED ends after the pyramids (out_pyramids (SE3_RGBD_IMAGES, F, S) float32, S the pixels of all levels, a
 *                           level after the one before it); CLAIMED after one correspondence pass at stop_level under the initial
 *                           transform (out_map (P, H W) 64-bit words: all ones, or hi32(q_z) << 32 | source index, a level's H_l W_l
 *                           entries first); EVALUATED after the normalisation and one iteration at stop_level (out_sums (P,
 *                           SE3_RGBD_SUMS), out_scales (P, 2), out_transforms the updated transform).  The last four may be NULL. */
enum se3_rgbd_limit {              /* (NAMED) */
  SE3_RGBD_MAX_LEVELS = 4,
  SE3_RGBD_MAX_IMAGE = 8192,       /* height and width of an image at most: SE3_TSDF_MAX_IMAGE */
  SE3_RGBD_MIN_SIDE = 3,           /* height and width of the coarsest level at least */
  SE3_RGBD_CHUNK = 2048,           /* target pixels per accumulation workgroup */
  SE3_RGBD_SUMS = 29,              /* 21 of J^T J, 6 of J^T r, the squared residual, the count */
  SE3_RGBD_IMAGES = 6,             /* images a frame's pyramid holds per level: I, D, Ix, Iy, Dx, Dy */
  SE3_RGBD_MAX_ITERATIONS = 1000   /* iterations of one level at most */
};
enum se3_rgbd_status {             /* (NAMED: the shared names carry ICP's values) */
  SE3_RGBD_NONFINITE = 1,
  SE3_RGBD_TOO_FEW = 2,
  SE3_RGBD_SINGULAR = 4,
  SE3_RGBD_EMPTY = 8,              /* no correspondence under the initial transform */
  SE3_RGBD_STEP_REFUSED = 16
};
enum se3_rgbd_method {
  SE3_RGBD_HYBRID = 0,
  SE3_RGBD_COLOR = 1
};
enum se3_rgbd_stop {
  SE3_RGBD_STOP_NONE = 0,
  SE3_RGBD_STOP_PREPARED = 1,
  SE3_RGBD_STOP_CLAIMED = 2,
  SE3_RGBD_STOP_EVALUATED = 3
};
size_t se3_rgbd_frames_workspace_bytes(int64_t num_frames, int height, int width, int num_levels);
size_t se3_rgbd_pairs_workspace_bytes(int num_pairs, int height, int width);
int se3_rgbd_odometry_stack(const void* depths, int depth_elem, const void* colors, int color_elem, int color_channels, int64_t num_frames,
                            int height, int width, const uint8_t* target_flags, int prepare, const int* pairs_host,
                            const double* intrinsics_host, int num_pairs, const double* init_transforms, int method,
                            const int* iterations_host, int num_levels, double depth_scale, double depth_trunc, double min_depth,
                            double max_depth, double max_depth_diff, double* out_transforms, uint8_t* out_success, int* out_status,
                            double* out_information, int64_t* out_count, void* frames_workspace, size_t frames_workspace_bytes,
                            void* pairs_workspace, size_t pairs_workspace_bytes, void* stream);
int se3_debug_rgbd_odometry_host(const void* depths, int depth_elem, const void* colors, int color_elem, int color_channels,
                                 int64_t num_frames, int height, int width, const uint8_t* target_flags, const int* pairs,
                                 const double* intrinsics, int num_pairs, const double* init_transforms, int method, const int* iterations,
                                 int num_levels, double depth_scale, double depth_trunc, double min_depth, double max_depth,
                                 double max_depth_diff, int stop, int stop_level, double* out_transforms, uint8_t* out_success,
                                 int* out_status, double* out_information, int64_t* out_count, float* out_pyramids, uint64_t* out_map,
                                 double* out_sums, double* out_scales);

/* ---- triangle meshes from the TSDF volumes (csrc/tsdf_mesh.hip, csrc/tsdf_mesh_core.h, csrc/mesh_table.h) -----------------------------------------
 * Open3D's extract_triangle_mesh for the uniform and the block-sparse volumes above, up to SE3_PAIR_MAX_PAIRS volumes per call: marching
 * cubes with a deterministic vertex numbering and no atomics; the contract, the rule of the triangle table included, is the header comment
 * of csrc/tsdf_mesh.hip.  The state is that of se3_tsdf_extract_stack / se3_stsdf_extract_stack.  Everything on the DEVICE unless it is
 * called _host.
 *   se3_tsdf_mesh_stack     two passes.  out_vertices NULL: the count pass and the scans; vertex_offsets and triangle_offsets (V R R + 1)
 *                           int64 each become the exclusive offsets of the rows (v, x, y) and the totals.  Otherwise the write pass:
 *                           out_vertices, out_normals and (with color) out_colors (vertex_capacity, 3) float64, out_triangles
 *                           (triangle_capacity, 3) int64; volume v's vertices at [vertex_offsets[v R R], vertex_offsets[(v + 1) R R]), its
 *                           triangles likewise, and a triangle names vertices by their number within the volume.  Nothing is written
 *                           at or past a capacity.  No workspace.
 *   se3_stsdf_mesh_stack    the same two passes over the groups (block, x) in key order: offsets of (16 B + 1) int64.  The write pass
 *                           needs vertex_plane, num_slots x 4096 ints of scratch (it need not be zeroed; as many bytes as the tsdf
 *                           storage), and a vertex_capacity below 2^31.
 *   se3_debug_tsdf_mesh_host / se3_debug_stsdf_mesh_host   the same text on HOST memory, serially, one volume / one directory.
 *                           out_vertices NULL: the counts alone.  out_counts: vertices, triangles.  out_block_offsets (2, B + 1): the
 *                           blocks' vertex offsets, then their triangle offsets.
 *   se3_debug_mesh_table    the triangle table (256, SE3_MESH_TABLE_WIDTH) signed bytes, -1 terminated rows of cube edges, and (unless
 *                           NULL) the 256 triangle counts, on the HOST. */
enum se3_mesh_limit {              /* (NAMED) */
  SE3_MESH_TABLE_WIDTH = 16,       /* entries of a row of the triangle table */
  SE3_MESH_MAX_TRIANGLES = 5       /* triangles of one cube at most */
};
int se3_tsdf_mesh_stack(const float* tsdf, const float* weight, const float* color, int num_volumes, int resolution, double voxel_length,
                        const double* origins, int64_t* vertex_offsets, int64_t* triangle_offsets, int64_t vertex_capacity,
                        int64_t triangle_capacity, double* out_vertices, double* out_normals, double* out_colors, int64_t* out_triangles,
                        void* stream);
int se3_stsdf_mesh_stack(const float* tsdf, const float* weight, const float* color, const int64_t* keys, const int* neighbors,
                         int64_t num_blocks, double voxel_length, int64_t* vertex_offsets, int64_t* triangle_offsets,
                         int64_t vertex_capacity, int64_t triangle_capacity, int* vertex_plane, double* out_vertices, double* out_normals,
                         double* out_colors, int64_t* out_triangles, void* stream);
int se3_debug_tsdf_mesh_host(const float* tsdf, const float* weight, const float* color, int resolution, double voxel_length,
                             const double* origin, int64_t vertex_capacity, int64_t triangle_capacity, double* out_vertices,
                             double* out_normals, double* out_colors, int64_t* out_triangles, int64_t* out_counts);
int se3_debug_stsdf_mesh_host(const float* tsdf, const float* weight, const float* color, const int64_t* keys, const int* slots,
                              int64_t num_blocks, double voxel_length, int64_t vertex_capacity, int64_t triangle_capacity,
                              double* out_vertices, double* out_normals, double* out_colors, int64_t* out_triangles,
                              int64_t* out_block_offsets);
int se3_debug_mesh_table(signed char* out_table, int* out_counts);

/* ---- ray casting of the TSDF volumes (csrc/tsdf_raycast.hip, csrc/tsdf_raycast_core.h) -------------------------------------------------------------
 * Open3D's VoxelBlockGrid.ray_cast for the uniform and the block-sparse volumes above, up to SE3_PAIR_MAX_PAIRS volumes per call: one ray per
 * pixel, no atomics, nothing read back; the contract is the header comment of csrc/tsdf_raycast.hip.  The state is that of
 * se3_tsdf_extract_stack / of the sparse directory (keys ascending with their slots; num_slots: the slots of the storage).  Everything on
 * the DEVICE unless it is called _host.
 *   se3_tsdf_raycast_stack / se3_stsdf_raycast_stack   views (F, SE3_RAYCAST_VIEW_WORDS) float64: the 3 x 4 camera-to-world pose by rows,
 *                           then fx, fy, cx, cy; view_volumes (F) ints: the volume each view looks at (a value outside [0, num_volumes)
 *                           renders no hit).  Outputs, each NULL or whole: out_depth (F, H, W) float32, out_points and out_normals
 *                           (F, H, W, 3) float64, out_colors (F, H, W, 3) float32 (only with color), out_mask (F, H, W) bytes.  Every
 *                           pixel of every map given is written: a pixel without a hit holds 0, NaN, NaN, 0, 0.  No workspace.
 *   se3_debug_tsdf_raycast_host / se3_debug_stsdf_raycast_host   the same text on HOST memory, serially, the views of one volume. */
enum se3_raycast_limit {           /* (NAMED) */
  SE3_RAYCAST_VIEW_WORDS = 16,     /* float64 words of a view's row of the table: SE3_STSDF_POSE_WORDS */
  SE3_RAYCAST_TILE = 16,           /* a workgroup casts a tile of this many pixels squared */
  SE3_RAYCAST_MAX_STEPS = 1048576  /* (depth_max - depth_min) / voxel_length at most */
};
int se3_tsdf_raycast_stack(const float* tsdf, const float* weight, const float* color, int num_volumes, int resolution, double voxel_length,
                           double sdf_trunc, const double* origins, const double* views, const int* view_volumes, int64_t num_views,
                           int height, int width, double depth_min, double depth_max, double weight_threshold, float* out_depth,
                           double* out_points, double* out_normals, float* out_colors, uint8_t* out_mask, void* stream);
int se3_stsdf_raycast_stack(const float* tsdf, const float* weight, const float* color, const int64_t* keys, const int* slots,
                            int64_t num_blocks, int64_t num_slots, int num_volumes, double voxel_length, double sdf_trunc,
                            const double* views, const int* view_volumes, int64_t num_views, int height, int width, double depth_min,
                            double depth_max, double weight_threshold, float* out_depth, double* out_points, double* out_normals,
                            float* out_colors, uint8_t* out_mask, void* stream);
int se3_debug_tsdf_raycast_host(const float* tsdf, const float* weight, const float* color, int resolution, double voxel_length,
                                double sdf_trunc, const double* origin, const double* views, int64_t num_views, int height, int width,
                                double depth_min, double depth_max, double weight_threshold, float* out_depth, double* out_points,
                                double* out_normals, float* out_colors, uint8_t* out_mask);
int se3_debug_stsdf_raycast_host(const float* tsdf, const float* weight, const float* color, const int64_t* keys, const int* slots,
                                 int64_t num_blocks, int64_t num_slots, int volume, double voxel_length, double sdf_trunc,
                                 const double* views, int64_t num_views, int height, int width, double depth_min, double depth_max,
                                 double weight_threshold, float* out_depth, double* out_points, double* out_normals, float* out_colors,
                                 uint8_t* out_mask);

/* ---- mesh post-processing of stacked triangle meshes (csrc/mesh_ops.hip, csrc/mesh_ops_core.h) -----------------------------------------------------
 * Open3D's cluster_connected_triangles, remove_triangles_by_mask + remove_unreferenced_vertices, compute_triangle_normals /
 * compute_vertex_normals and filter_smooth_simple / _laplacian / _taubin for up to SE3_PAIR_MAX_PAIRS meshes per call, float64; the contract
 * is the header comment of csrc/mesh_ops.hip.  The meshes are stacked as se3_tsdf_mesh_stack leaves them: vertices (N, 3) float64, triangles
 * (M, 3) int64 naming vertices by their number within their own mesh, attributes (N, 3) float64, all on the DEVICE unless an entry is called
 * _host; vertex_offsets_host and triangle_offsets_host (B + 1) int64 on the HOST, from 0, not decreasing; a mesh has fewer than 2^31
 * vertices and triangles.  out_counts (B, SE3_MESH_OPS_COUNT_WORDS) int64 on the device: word 0 of a mesh is its status (a se3_mesh_ops_status
 * bit: a triangle names a vertex outside [0, n); such a triangle is skipped, never dereferenced), the other words are named per entry.
 *   se3_mesh_incidence_stack   two passes.  nbr_rows NULL: tri_row_offsets and nbr_row_offsets (N + 1) int64 become the exclusive offsets of
 *                           the vertices' rows, tri_rows (3 M) ints holds each vertex's incident triangles ascending; counts words 1, 2: the
 *                           mesh's incidences and neighbours.  Otherwise the write pass: nbr_rows (nbr_capacity) ints, each vertex's
 *                           distinct neighbours ascending; nothing is written at or past the capacity.  Rows hold mesh-local numbers.
 *                           workspace: se3_mesh_incidence_workspace_bytes(N).
 *   se3_mesh_components_stack  out_clusters (M) int64: 0 .. k - 1 per mesh in ascending order of a cluster's lowest triangle;
 *                           out_cluster_n_triangles (M) int64: cluster c of mesh b at triangle_offsets[b] + c, the slots past k hold 0;
 *                           counts word 1: k.  workspace: se3_mesh_components_workspace_bytes(M).
 *   se3_mesh_cluster_area_stack  out_cluster_area (M) float64 in the same slots.  order (M) int64: the stacked triangle rows sorted by
 *                           (slot, row), i.e. a stable sort of out_clusters + triangle_offsets[mesh]; a place that names no row adds 0.
 *                           workspace: se3_mesh_cluster_area_workspace_bytes(M).
 *   se3_mesh_select_stack   two passes over one workspace (se3_mesh_select_workspace_bytes(N, M)), keep (M) bytes.  out_vertex_offsets_host
 *                           NULL: out_vertex_map (N) int64 (the new number, -1 for a dropped vertex) and counts words 1, 2: the vertices and
 *                           triangles kept.  Otherwise the write pass into the rows the output offsets name; normals and colors may be NULL.
 *   se3_mesh_normals_stack  out_triangle_normals (M, 3) and out_vertex_normals (N, 3), either NULL; the tables only for the latter.  out_counts
 *                           may be NULL; given, the triangle normals' pass sets the status words.
 *   se3_mesh_smooth_stack   method: a se3_mesh_smooth_method; every step of `iterations` iterations is issued by the call, one launch per
 *                           step; normals and colors may be NULL and are filtered like the positions.  0 iterations copies.  The outputs
 *                           must not alias the inputs.  workspace: se3_mesh_smooth_workspace_bytes(N, arrays given).
 *   se3_mesh_cluster_vertices_stack   simplify_vertex_clustering with the mean as contraction, in the four passes of se3_mesh_cluster_pass over one
 *                           workspace (se3_mesh_cluster_vertices_workspace_bytes(N, M)); the caller sorts between them.  KEYS: keys (N) int64, a
 *                           vertex's cell with x in the high bits (0 for a refused mesh), and the status words.  VERTICES: sorted_keys and
 *                           vertex_order (N) int64, the stacked vertex rows sorted by (mesh, key, row); writes vertex_map (N) int64, rotated
 *                           (M, 3) int64 (the remapped triangle with its lowest vertex first, -1 for a dropped one) and counts word 1, the new
 *                           vertices.  TRIANGLES: triangle_order (M) int64, the stacked triangle rows sorted by (mesh, rotated triple, row), the
 *                           dropped ones anywhere; counts word 2: the triangles that stay.  WRITE: into the rows the output offsets name.  A
 *                           place of an order that names no row of its mesh is passed over.
 *   se3_debug_mesh_*_host   the same text on HOST memory, serially, one mesh of n vertices and m triangles; the cluster outputs have m
 *                           slots of which the first k are used; se3_debug_mesh_smooth_host filters one (n, 3) array. */
enum se3_mesh_ops_limit {              /* (NAMED) */
  SE3_MESH_OPS_COUNT_WORDS = 4,        /* int64 words of a mesh's row of out_counts */
  SE3_MESH_OPS_AREA_LANES = 64,        /* lanes of the reduction tree of a cluster's area */
  SE3_MESH_OPS_MAX_ITERATIONS = 100000 /* smoothing iterations of one call at most */
};
enum se3_mesh_ops_status {             /* (NAMED) */
  SE3_MESH_OPS_BAD_TRIANGLE = 1,       /* a triangle names a vertex outside [0, n) */
  SE3_MESH_OPS_NONFINITE = 2,          /* vertex clustering: a vertex or an attribute is not finite */
  SE3_MESH_OPS_TOO_MANY_CELLS = 4      /* vertex clustering: an axis would need 2^21 cells or more */
};
enum se3_mesh_cluster_pass {           /* (NAMED) */
  SE3_MESH_CLUSTER_KEYS = 0,
  SE3_MESH_CLUSTER_VERTICES = 1,
  SE3_MESH_CLUSTER_TRIANGLES = 2,
  SE3_MESH_CLUSTER_WRITE = 3
};
enum se3_mesh_smooth_method {          /* (NAMED) */
  SE3_MESH_SMOOTH_SIMPLE = 0,
  SE3_MESH_SMOOTH_LAPLACIAN = 1,
  SE3_MESH_SMOOTH_TAUBIN = 2
};
size_t se3_mesh_incidence_workspace_bytes(int64_t n_total);
int se3_mesh_incidence_stack(const int64_t* triangles, const int64_t* vertex_offsets_host, const int64_t* triangle_offsets_host, int num_meshes,
                             int64_t* tri_row_offsets, int* tri_rows, int64_t* nbr_row_offsets, int64_t nbr_capacity, int* nbr_rows,
                             int64_t* out_counts, void* workspace, size_t workspace_bytes, void* stream);
size_t se3_mesh_components_workspace_bytes(int64_t m_total);
int se3_mesh_components_stack(const int64_t* triangles, const int64_t* vertex_offsets_host, const int64_t* triangle_offsets_host, int num_meshes,
                              const int64_t* tri_row_offsets, const int* tri_rows, int64_t* out_clusters, int64_t* out_cluster_n_triangles,
                              int64_t* out_counts, void* workspace, size_t workspace_bytes, void* stream);
size_t se3_mesh_cluster_area_workspace_bytes(int64_t m_total);
int se3_mesh_cluster_area_stack(const double* vertices, const int64_t* triangles, const int64_t* vertex_offsets_host,
                                const int64_t* triangle_offsets_host, int num_meshes, const int64_t* cluster_n_triangles, const int64_t* order,
                                double* out_cluster_area, void* workspace, size_t workspace_bytes, void* stream);
size_t se3_mesh_select_workspace_bytes(int64_t n_total, int64_t m_total);
int se3_mesh_select_stack(const double* vertices, const double* normals, const double* colors, const int64_t* triangles, const uint8_t* keep,
                          const int64_t* vertex_offsets_host, const int64_t* triangle_offsets_host, int num_meshes,
                          const int64_t* out_vertex_offsets_host, const int64_t* out_triangle_offsets_host, double* out_vertices,
                          double* out_normals, double* out_colors, int64_t* out_triangles, int64_t* out_vertex_map, int64_t* out_counts,
                          void* workspace, size_t workspace_bytes, void* stream);
int se3_mesh_normals_stack(const double* vertices, const int64_t* triangles, const int64_t* vertex_offsets_host,
                           const int64_t* triangle_offsets_host, int num_meshes, const int64_t* tri_row_offsets, const int* tri_rows,
                           int normalized, double* out_triangle_normals, double* out_vertex_normals, int64_t* out_counts, void* stream);
size_t se3_mesh_cluster_vertices_workspace_bytes(int64_t n_total, int64_t m_total);
int se3_mesh_cluster_vertices_stack(int pass, const double* vertices, const double* normals, const double* colors, const int64_t* triangles,
                                    const int64_t* vertex_offsets_host, const int64_t* triangle_offsets_host, int num_meshes, double voxel_size,
                                    int64_t* keys, const int64_t* sorted_keys, const int64_t* vertex_order, int64_t* vertex_map, int64_t* rotated,
                                    const int64_t* triangle_order, const int64_t* out_vertex_offsets_host,
                                    const int64_t* out_triangle_offsets_host, double* out_vertices, double* out_normals, double* out_colors,
                                    int64_t* out_triangles, int64_t* out_counts, void* workspace, size_t workspace_bytes, void* stream);
int se3_debug_mesh_cluster_vertices_host(const double* vertices, const double* normals, const double* colors, const int64_t* triangles, int64_t n,
                                         int64_t m, double voxel_size, int64_t vertex_capacity, int64_t triangle_capacity, double* out_vertices,
                                         double* out_normals, double* out_colors, int64_t* out_triangles, int64_t* out_vertex_map,
                                         int64_t* out_counts);
size_t se3_mesh_smooth_workspace_bytes(int64_t n_total, int num_arrays);
int se3_mesh_smooth_stack(const double* vertices, const double* normals, const double* colors, const int64_t* vertex_offsets_host, int num_meshes,
                          const int64_t* nbr_row_offsets, const int* nbr_rows, int method, int iterations, double lambda, double mu,
                          double* out_vertices, double* out_normals, double* out_colors, void* workspace, size_t workspace_bytes, void* stream);
int se3_debug_mesh_incidence_host(const int64_t* triangles, int64_t n, int64_t m, int64_t* tri_row_offsets, int* tri_rows,
                                  int64_t* nbr_row_offsets, int64_t nbr_capacity, int* nbr_rows, int64_t* out_counts);
int se3_debug_mesh_components_host(const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const int64_t* tri_row_offsets,
                                   const int* tri_rows, int64_t* out_clusters, int64_t* out_cluster_n_triangles, double* out_cluster_area,
                                   int64_t* out_counts);
int se3_debug_mesh_select_host(const double* vertices, const double* normals, const double* colors, const int64_t* triangles,
                               const uint8_t* keep, int64_t n, int64_t m, int64_t vertex_capacity, int64_t triangle_capacity,
                               double* out_vertices, double* out_normals, double* out_colors, int64_t* out_triangles, int64_t* out_vertex_map,
                               int64_t* out_counts);
int se3_debug_mesh_normals_host(const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const int64_t* tri_row_offsets,
                                const int* tri_rows, int normalized, double* out_triangle_normals, double* out_vertex_normals);
int se3_debug_mesh_smooth_host(const double* values, int64_t n, const int64_t* nbr_row_offsets, const int* nbr_rows, int method, int iterations,
                               double lambda, double mu, double* out_values);

/* ---- ray casting and closest points on stacked triangle meshes (csrc/mesh_query.hip, csrc/mesh_query_core.h) ----------------------------------------
 * Open3D's RaycastingScene (cast_rays, test_occlusions, compute_closest_points, compute_distance) and a depth rendering for up to
 * SE3_PAIR_MAX_PAIRS meshes per call, float64, over a bounding volume hierarchy built on the device; the contract is the header comment
 * of csrc/mesh_query.hip.  The meshes are stacked as for the mesh post-processing above.  nodes: 2 max(M, 1) nodes of
 * SE3_MESH_QUERY_NODE_BYTES bytes; counts (B, SE3_MESH_OPS_COUNT_WORDS) int64 on the device: status (SE3_MESH_OPS_BAD_TRIANGLE,
 * SE3_MESH_QUERY_NONFINITE_VERTEX), live triangles, zero-area triangles, root.  Everything on the DEVICE unless an entry is called _host.
 *   se3_mesh_bvh_stack      two passes over one workspace (se3_mesh_bvh_workspace_bytes(M)) and one counts array.  SE3_MESH_BVH_KEYS: keys (M)
 *                           int64, a live triangle's 63-bit Morton key, -1 for an inert one, and the first three count words.
 *                           SE3_MESH_BVH_TREE: sorted_keys and order (M) int64, the stacked triangle rows sorted per mesh by (key < 0, key,
 *                           row); writes the nodes and each mesh's root.
 *   se3_mesh_cast_rays_stack   rays (R, 6) float64 origin and direction, ray_meshes (R) ints (outside [0, B): a miss); out_t (R) float64,
 *                           out_ids (R) int64, out_uvs (R, 2), out_normals (R, 3), each NULL or whole.  any_hit: only out_hit (R) bytes is
 *                           written and a ray's walk ends at its first hit.
 *   se3_mesh_render_stack   views (F, SE3_RAYCAST_VIEW_WORDS) float64 as se3_tsdf_raycast_stack takes them, view_meshes (F) ints; out_depth
 *                           (F, H, W) float32, out_points and out_normals (F, H, W, 3) float64, out_primitive_ids (F, H, W) int64, out_mask
 *                           (F, H, W) bytes, each NULL or whole; a pixel without a hit holds 0, NaN, NaN, -1, 0.
 *   se3_mesh_closest_points_stack   queries (Q, 3) float64, query_meshes (Q) ints; out_points (Q, 3), out_distances (Q), out_ids (Q) int64,
 *                           out_uvs (Q, 2), out_normals (Q, 3), each NULL or whole.
 *   se3_debug_mesh_bvh_host   the same two passes on HOST memory, serially, one mesh: order (m) holds the triangle of every sorted place.
 *   se3_debug_mesh_cast_rays_host / _closest_points_host / _render_host   BRUTE FORCE over every triangle on HOST memory, one mesh: no tree.
 *   se3_debug_mesh_walk_rays_host / _walk_points_host   the kernels' walk over a tree of se3_debug_mesh_bvh_host, on HOST memory. */
enum se3_mesh_query_limit {            /* (NAMED) */
  SE3_MESH_QUERY_NODE_BYTES = 64,      /* bytes of a node: six float64 bounds, two children, the parent, padding */
  SE3_MESH_QUERY_KEY_BITS = 21,        /* bits of a Morton key per axis */
  SE3_MESH_QUERY_MAX_DEPTH = 94,       /* inner nodes on a path from the root at most: 63 key bits + 31 position bits */
  SE3_MESH_QUERY_TRAIL_BITS = 128      /* levels that the walk can remember */
};
enum se3_mesh_query_status {           /* (NAMED) a bit of the status word beside those of se3_mesh_ops_status */
  SE3_MESH_QUERY_NONFINITE_VERTEX = 8  /* a triangle has a vertex that is not finite */
};
enum se3_mesh_bvh_pass {               /* (NAMED) */
  SE3_MESH_BVH_KEYS = 0,
  SE3_MESH_BVH_TREE = 1
};
size_t se3_mesh_bvh_workspace_bytes(int64_t m_total);
int se3_mesh_bvh_stack(int pass, const double* vertices, const int64_t* triangles, const int64_t* vertex_offsets_host,
                       const int64_t* triangle_offsets_host, int num_meshes, int64_t* keys, const int64_t* sorted_keys, const int64_t* order,
                       void* out_nodes, int64_t* out_counts, void* workspace, size_t workspace_bytes, void* stream);
int se3_mesh_cast_rays_stack(const double* vertices, const int64_t* triangles, const int64_t* vertex_offsets_host,
                             const int64_t* triangle_offsets_host, int num_meshes, const void* nodes, const int64_t* tree_counts,
                             const double* rays, const int* ray_meshes, int64_t num_rays, double t_min, double t_max, int any_hit,
                             double* out_t, int64_t* out_ids, double* out_uvs, double* out_normals, uint8_t* out_hit, void* stream);
int se3_mesh_render_stack(const double* vertices, const int64_t* triangles, const int64_t* vertex_offsets_host,
                          const int64_t* triangle_offsets_host, int num_meshes, const void* nodes, const int64_t* tree_counts,
                          const double* views, const int* view_meshes, int64_t num_views, int height, int width, double depth_min,
                          double depth_max, float* out_depth, double* out_points, double* out_normals, int64_t* out_primitive_ids,
                          uint8_t* out_mask, void* stream);
int se3_mesh_closest_points_stack(const double* vertices, const int64_t* triangles, const int64_t* vertex_offsets_host,
                                  const int64_t* triangle_offsets_host, int num_meshes, const void* nodes, const int64_t* tree_counts,
                                  const double* queries, const int* query_meshes, int64_t num_queries, double* out_points,
                                  double* out_distances, int64_t* out_ids, double* out_uvs, double* out_normals, void* stream);
int se3_debug_mesh_bvh_host(int pass, const double* vertices, const int64_t* triangles, int64_t n, int64_t m, int64_t* keys,
                            const int64_t* sorted_keys, const int64_t* order, void* out_nodes, int64_t* out_counts);
int se3_debug_mesh_cast_rays_host(const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const double* rays, int64_t num_rays,
                                  double t_min, double t_max, int any_hit, double* out_t, int64_t* out_ids, double* out_uvs,
                                  double* out_normals, uint8_t* out_hit);
int se3_debug_mesh_closest_points_host(const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const double* queries,
                                       int64_t num_queries, double* out_points, double* out_distances, int64_t* out_ids, double* out_uvs,
                                       double* out_normals);
int se3_debug_mesh_walk_rays_host(const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const void* nodes, int64_t root,
                                  const double* rays, int64_t num_rays, double t_min, double t_max, int any_hit, double* out_t,
                                  int64_t* out_ids, double* out_uvs, double* out_normals, uint8_t* out_hit);
int se3_debug_mesh_walk_points_host(const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const void* nodes, int64_t root,
                                    const double* queries, int64_t num_queries, double* out_points, double* out_distances, int64_t* out_ids,
                                    double* out_uvs, double* out_normals);
int se3_debug_mesh_render_host(const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const double* views, int64_t num_views,
                               int height, int width, double depth_min, double depth_max, float* out_depth, double* out_points,
                               double* out_normals, int64_t* out_primitive_ids, uint8_t* out_mask);

#ifdef __cplusplus
}
#endif
#endif /* SE3ET_HIP_H_ */
