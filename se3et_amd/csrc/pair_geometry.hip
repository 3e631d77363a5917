// Ground truth of a registration pair for stacked pairs: what the reference computes on the host with scipy's cKDTree --
// get_nearest_neighbor (geotransformer/utils/pointcloud.py:11-22), compute_overlap and get_correspondences (utils/registration.py:149-173)
// and calibrate_ground_truth (datasets/registration/threedmatch/utils.py:197-228: the overlap and 6x6 covariance of a gt.info record).
// The query cloud of a pair is searched in the OTHER cloud of the pair after a rigid transform; csrc/pair_grid.h holds the grid and the
// search core, this file the grid's device build, se3et_amd/pair_geometry.py carries the same contract.
//
//   pair_grid_*_kernel          the build: transform + exact bounding box, cell histogram, scan, scatter; batched over pairs.
//   pair_nearest_kernel         exact 1-NN, one wave per query row of the stacked rows: lanes stride the points of the cells of a ring,
//                               the wave reduces on (d^2, index), the running best stays in registers, the rings stop by the shell rule.
//   pair_ball_count_kernel      ball query, pass 1: hits per row, then se3_exclusive_scan_i64 over the stacked rows (block_ops.h).
//   pair_ball_fill_kernel       pass 2: each row's (i, j), j ascending (sorted as it is written: no result depends on an atomic).
//   pair_overlap_kernel         one workgroup per pair: integer count of d_nn < r in a fixed tree, one division.
//   pair_covariance_kernel      one workgroup per pair: the ten float64 sums of a gt.info covariance, each lane serially over a fixed
//                               stride, then a fixed tree.  No float atomics anywhere.
//
// Arithmetic contract.  Everything is float64, as the reference computes it with numpy and scipy on float64 arrays.  Inputs may be float32
// or float64 on the device; they are promoted on load inside the kernels and never copied.  Transforms are (P, 4, 4) float64.
//   - A transformed support point is fma(R[k][2], z, fma(R[k][1], y, R[k][0] * x)) + t[k], the expression benchmark.hip documents.
//   - A distance is sqrt((dx*dx + dy*dy) + dz*dz).
//   - Tests are d < r on d*d < r*r, strict: the ball query compares (dx*dx + dy*dy) + dz*dz with r*r and takes no root; the overlap and
//     the gt.info selection compare the nearest-neighbour distances this library returned, squared again, with r*r.
//   - This is not bit-for-bit the BLAS or k-d tree arithmetic of the reference.  Only a distance within float64 rounding of a threshold,
//     or of another candidate's distance, can come out differently.
//   nearest neighbour   for every query row the float64 distance to the nearest transformed support point of its own pair and that point's
//            pair-local index (int64).  The search is exact; the grid is only an accelerator: the ring of cells widens until the best
//            distance found is no larger than the distance to the unvisited shell, so a query far outside the support's bounding box
//            terminates and is correct.  Among exactly equal distances the lowest index wins.  An empty support gives inf and -1.
//   overlap  count(d_nn < r) / n_ref in float64: the count is an integer and the division is done once (np.mean of the reference exactly);
//            n_ref = 0 gives NaN.
//   correspondences   all (i, j) with |ref_i - (R src_j + t)| < r; rows ascending in i, j ascending within a row (the order of scipy's
//            multi-point query_ball_point); int64 (n, 2).  Two passes: count per row, exclusive scan, fill.  A pair's rows are
//            bit-identical whether the pair is alone or in any batch, and from run to run.
//   gt.info  overlap at 5 voxel_size; the covariance is sum G^T G over the selected transformed src points, G = [I3 | -[p]x] in the sign
//            layout of utils.py:214-221, i.e. with S = sum over the points:
//              [0][0] = [1][1] = [2][2] = n,  [0][4] = S z, [0][5] = -S y, [1][3] = -S z, [1][5] = S x, [2][3] = S y, [2][4] = -S x,
//              [3][3] = S (z z + y y), [4][4] = S (z z + x x), [5][5] = S (y y + x x), [3][4] = -S x y, [3][5] = -S x z, [4][5] = -S y z,
//            symmetric, summed in a fixed order; no selected point gives the zero matrix.  (The selection and its draw are the host's:
//            se3et_amd/pair_geometry.py.)
#include <math.h>

#include "common.h"
#include "pair_grid.h"

namespace {

static_assert(kPairMaxPairs == SE3_PAIR_MAX_PAIRS, "stack_rows.h and include/se3et_hip.h name one limit");
constexpr int kNnWaves = 4;          // query rows per nearest-neighbour workgroup
constexpr int kBallThreads = 64;     // query rows per ball-query workgroup
constexpr int kRowThreads = 256;
constexpr int kSums = 10;            // n, x, y, z, zz+yy, zz+xx, yy+xx, xy, xz, yz

// ---- the build as kernels, batched over pairs --------------------------------------------------------------------------------------------
struct PairTransforms {
  double T[kPairMaxPairs][12];
};

constexpr int kPairBoundsThreads = 256;

// one workgroup per pair: transform the support into `moved`, exact bounding box, grid geometry
__global__ __launch_bounds__(kPairBoundsThreads) void pair_grid_bounds_kernel(const void* __restrict__ s, int elem, PairRows rows, PairTransforms tf,
                                                                double cell_hint, PairGridLayout G) {
  __shared__ double sh[kPairBoundsThreads / 64];
  const int p = blockIdx.x;
  const int64_t s0 = rows.start[p], n = rows.start[p + 1] - s0;
  double T[12];
  for (int k = 0; k < 12; k++) T[k] = tf.T[p][k];
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = s0 + threadIdx.x; i < s0 + n; i += kPairBoundsThreads) {
    double w[3];        // (the loads written out: through pg_load3 hipcc 7.2 orders this loop's address arithmetic differently)
    pg_transform(T, pg_load(s, elem, 3 * i), pg_load(s, elem, 3 * i + 1), pg_load(s, elem, 3 * i + 2), w);
    for (int d = 0; d < 3; d++) {
      G.moved[3 * i + d] = w[d];
      mn[d] = fmin(mn[d], w[d]);
      mx[d] = fmax(mx[d], w[d]);
    }
  }
  se3_block_bounds<double, kPairBoundsThreads>(mn, mx, sh);
  if (threadIdx.x == 0) {
    PairGridMeta* m = G.meta + p;
    for (int k = 0; k < 12; k++) m->T[k] = T[k];
    m->s_start = s0, m->ns = n;
    pg_make_grid(mn, mx, n, cell_hint, m);
  }
}

// cell histogram (the only atomics of the build: integer adds, order-free)
__global__ __launch_bounds__(256) void pair_grid_count_kernel(PairRows rows, int64_t ns_total, PairGridLayout G) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ns_total) return;
  const int p = pg_pair_of_row(rows, i);
  atomicAdd(&G.cells[(size_t)p * (kPairCellCap + 1) + pg_cell_of(G.meta[p], G.moved + 3 * i)], 1);
}

// one workgroup per pair: counts -> INCLUSIVE ends (the scatter counts each end down to its cell's start); cells[ncells] = ns
__global__ __launch_bounds__(1024) void pair_grid_scan_kernel(PairGridLayout G) {
  __shared__ int sh[1024];
  const int n = G.meta[blockIdx.x].ncells;
  int* a = G.cells + (size_t)blockIdx.x * (kPairCellCap + 1);
  const int total = se3_block_scan<kSe3ScanInclusive>(a, n, sh);
  if (threadIdx.x == 0) a[n] = total;
}

__global__ __launch_bounds__(256) void pair_grid_scatter_kernel(PairRows rows, int64_t ns_total, PairGridLayout G) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ns_total) return;
  const int p = pg_pair_of_row(rows, i);
  const int64_t s0 = rows.start[p];
  const int pos = atomicSub(&G.cells[(size_t)p * (kPairCellCap + 1) + pg_cell_of(G.meta[p], G.moved + 3 * i)], 1) - 1;
  for (int d = 0; d < 3; d++) G.sorted[3 * (s0 + pos) + d] = G.moved[3 * i + d];
  G.sorted_idx[s0 + pos] = (int)(i - s0);
}

__global__ __launch_bounds__(kNnWaves* SE3_WAVE) void pair_nearest_kernel(PairGridView g, const void* __restrict__ q, int elem, PairRows rows,
                                                                          int64_t nq_total, double* __restrict__ dist,
                                                                          int64_t* __restrict__ index) {
  const int64_t i = (int64_t)blockIdx.x * kNnWaves + (threadIdx.x >> 6);
  if (i >= nq_total) return;                               // (uniform over the wave)
  const int p = pg_pair_of_row(rows, i);
  double qv[3], d2;
  int j;
  pg_load3(q, elem, i, qv);
  pg_wave_nearest(g, p, qv, &d2, &j);
  if (se3_lane() == 0) {
    dist[i] = sqrt(d2);
    index[i] = j;
  }
}

__global__ __launch_bounds__(kBallThreads) void pair_ball_count_kernel(PairGridView g, const void* __restrict__ q, int elem, PairRows rows,
                                                                       int64_t nq_total, PairRadii radii, int64_t* __restrict__ row_offsets) {
  const int64_t i = (int64_t)blockIdx.x * kBallThreads + threadIdx.x;
  if (i >= nq_total) return;
  const int p = pg_pair_of_row(rows, i);
  const double r = radii.r[p];
  double qv[3];
  pg_load3(q, elem, i, qv);
  row_offsets[i] = pg_ball_count(g, p, qv, r, r * r);
}

__global__ __launch_bounds__(kBallThreads) void pair_ball_fill_kernel(PairGridView g, const void* __restrict__ q, int elem, PairRows rows,
                                                                      int64_t nq_total, PairRadii radii, const int64_t* __restrict__ row_offsets,
                                                                      int64_t total, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBallThreads + threadIdx.x;
  if (i >= nq_total) return;
  const int64_t base = row_offsets[i], room = row_offsets[i + 1] - base;
  if (base < 0 || room <= 0 || base + room > total) return;           // (offsets that do not belong to `out`: nothing is written)
  const int p = pg_pair_of_row(rows, i);
  double qv[3];
  pg_load3(q, elem, i, qv);
  const double r = radii.r[p];
  pg_ball_fill(g, p, qv, r, r * r, i - rows.start[p], out + 2 * base, room);
}

__global__ __launch_bounds__(kRowThreads) void pair_overlap_kernel(const double* __restrict__ dist, PairRows rows, double r2,
                                                                   double* __restrict__ out) {
  __shared__ long long s_cnt[kRowThreads];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t b0 = rows.start[p], n = rows.start[p + 1] - b0;
  long long cnt = 0;
  for (int64_t i = tid; i < n; i += kRowThreads) {
    const double d = dist[b0 + i];
    cnt += d * d < r2;
  }
  s_cnt[tid] = cnt;
  __syncthreads();
  for (int o = kRowThreads / 2; o > 0; o >>= 1) {
    if (tid < o) s_cnt[tid] += s_cnt[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[p] = (double)s_cnt[0] / (double)n;              // 0 / 0 = NaN: np.mean of an empty array
}

__device__ __forceinline__ double block_sum(double v, double* scratch) {   // fixed order: wave trees, then the four wave sums in wave order
  v = se3_wave_sum(v);
  __syncthreads();
  if (se3_lane() == 0) scratch[threadIdx.x / SE3_WAVE] = v;
  __syncthreads();
  return ((scratch[0] + scratch[1]) + scratch[2]) + scratch[3];
}

__global__ __launch_bounds__(kRowThreads) void pair_covariance_kernel(const void* __restrict__ src, int elem, PairRows src_rows, PairTransforms tf,
                                                                      const int64_t* __restrict__ selected, PairRows sel_rows,
                                                                      double* __restrict__ out) {
  __shared__ double scratch[kRowThreads / SE3_WAVE];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t s0 = src_rows.start[p], ns = src_rows.start[p + 1] - s0;
  const int64_t k0 = sel_rows.start[p], nk = sel_rows.start[p + 1] - k0;
  double T[12];
  for (int k = 0; k < 12; k++) T[k] = tf.T[p][k];
  double acc[kSums];
  for (int c = 0; c < kSums; c++) acc[c] = 0.0;
  for (int64_t k = tid; k < nk; k += kRowThreads) {
    const int64_t j = selected[k0 + k];
    if (j < 0 || j >= ns) continue;                                  // (refused on the host where the host sees the indices)
    double w[3];
    pg_transform_row(T, src, elem, s0 + j, w);
    const double x = w[0], y = w[1], z = w[2];
    acc[0] += 1.0, acc[1] += x, acc[2] += y, acc[3] += z;
    acc[4] += z * z + y * y, acc[5] += z * z + x * x, acc[6] += y * y + x * x;
    acc[7] += x * y, acc[8] += x * z, acc[9] += y * z;
  }
  for (int c = 0; c < kSums; c++) acc[c] = block_sum(acc[c], scratch);
  if (tid == 0) {
    double* C = out + 36 * p;
    for (int c = 0; c < 36; c++) C[c] = 0.0;
    if (acc[0] > 0.0) {
      const double n = acc[0], sx = acc[1], sy = acc[2], sz = acc[3];
      C[0] = C[7] = C[14] = n;
      C[6 * 0 + 4] = C[6 * 4 + 0] = sz, C[6 * 0 + 5] = C[6 * 5 + 0] = -sy;
      C[6 * 1 + 3] = C[6 * 3 + 1] = -sz, C[6 * 1 + 5] = C[6 * 5 + 1] = sx;
      C[6 * 2 + 3] = C[6 * 3 + 2] = sy, C[6 * 2 + 4] = C[6 * 4 + 2] = -sx;
      C[6 * 3 + 3] = acc[4], C[6 * 4 + 4] = acc[5], C[6 * 5 + 5] = acc[6];
      C[6 * 3 + 4] = C[6 * 4 + 3] = -acc[7], C[6 * 3 + 5] = C[6 * 5 + 3] = -acc[8], C[6 * 4 + 5] = C[6 * 5 + 4] = -acc[9];
    }
  }
}

bool finite_transforms(const double* T, int num_pairs) {
  for (int i = 0; i < 16 * num_pairs; i++)
    if (!isfinite(T[i])) return false;
  return true;
}

void fill_transforms(PairTransforms* tf, const double* T, int num_pairs) {
  for (int p = 0; p < kPairMaxPairs; p++)
    for (int k = 0; k < 12; k++) tf->T[p][k] = p < num_pairs ? T[16 * p + k] : 0.0;
}

}  // namespace

extern "C" size_t se3_pair_grid_workspace_bytes(int64_t ns_total, int num_pairs) {
  if (ns_total < 0 || num_pairs < 0 || num_pairs > kPairMaxPairs) return 0;
  return pg_carve(ns_total, num_pairs, nullptr, nullptr);
}

extern "C" int se3_pair_grid_build(const void* s_points, int elem, const int64_t* s_offsets_host, int num_pairs, const double* transforms_host,
                                   double cell_hint, void* workspace, size_t workspace_bytes, void* stream) {
  SE3_REQUIRE(s_points && s_offsets_host && transforms_host && workspace, SE3_ERR_INVALID_ARG, "pair_grid_build: null pointer");
  SE3_REQUIRE(num_pairs >= 0 && num_pairs <= kPairMaxPairs && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG,
              "pair_grid_build: %d pairs (at most %d), elem %d", num_pairs, kPairMaxPairs, elem);
  SE3_REQUIRE(pg_radius_ok(cell_hint), SE3_ERR_INVALID_ARG, "pair_grid_build: cell size hint %g", cell_hint);
  SE3_REQUIRE(finite_transforms(transforms_host, num_pairs), SE3_ERR_INVALID_ARG, "pair_grid_build: non-finite transform");
  PairRows rows;
  SE3_REQUIRE(pg_fill_rows(&rows, s_offsets_host, num_pairs), SE3_ERR_INVALID_ARG, "pair_grid_build: offsets must start at 0 and not decrease");
  const int64_t ns_total = rows.start[num_pairs];
  SE3_REQUIRE(ns_total < (1ll << 31), SE3_ERR_UNSUPPORTED, "pair_grid_build: %lld support points in one call", (long long)ns_total);
  PairGridLayout G;
  SE3_REQUIRE(pg_carve(ns_total, num_pairs, (char*)workspace, &G) <= workspace_bytes, SE3_ERR_WORKSPACE,
              "pair_grid_build: workspace of %zu bytes is too small", workspace_bytes);
  if (num_pairs == 0) return SE3_OK;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(G.cells, 0, sizeof(int) * (size_t)num_pairs * (kPairCellCap + 1), st) != hipSuccess) {
    se3_set_error("pair_grid_build: hipMemsetAsync failed");
    return SE3_ERR_LAUNCH;
  }
  PairTransforms tf;
  fill_transforms(&tf, transforms_host, num_pairs);
  pair_grid_bounds_kernel<<<(unsigned)num_pairs, kPairBoundsThreads, 0, st>>>(s_points, elem, rows, tf, cell_hint, G);
  if (ns_total > 0) pair_grid_count_kernel<<<(unsigned)se3_cdiv(ns_total, 256), 256, 0, st>>>(rows, ns_total, G);
  pair_grid_scan_kernel<<<(unsigned)num_pairs, 1024, 0, st>>>(G);
  if (ns_total > 0) pair_grid_scatter_kernel<<<(unsigned)se3_cdiv(ns_total, 256), 256, 0, st>>>(rows, ns_total, G);
  SE3_CHECK_LAUNCH("pair_grid_build");
  return SE3_OK;
}

extern "C" int se3_pair_nearest_neighbor_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                                               const int64_t* q_offsets_host, int num_pairs, double* distances, int64_t* indices, void* stream) {
  PairGridCall c;
  if (const int rc = pg_grid_call("pair_nearest_neighbor_stack", "pairs", q_points && distances && indices, grid_workspace, workspace_bytes,
                                  ns_total, elem, q_offsets_host, num_pairs, 1ll << 31, &c))
    return rc;
  if (c.n_total == 0) return SE3_OK;
  pair_nearest_kernel<<<(unsigned)se3_cdiv(c.n_total, kNnWaves), kNnWaves * SE3_WAVE, 0, (hipStream_t)stream>>>(c.G.view(), q_points, elem, c.rows,
                                                                                                               c.n_total, distances, indices);
  SE3_CHECK_LAUNCH("pair_nearest_neighbor_stack");
  return SE3_OK;
}

// the ball query's two passes with one radius per pair (radii_host: num_pairs host doubles); the entries with one radius for all fill the table
static int ball_count(const char* name, const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                      const int64_t* q_offsets_host, int num_pairs, const double* radii_host, double radius, int64_t* row_offsets, void* stream) {
  PairGridCall c;
  if (const int rc = pg_grid_call(name, "pairs", q_points && row_offsets, grid_workspace, workspace_bytes, ns_total, elem, q_offsets_host,
                                  num_pairs, 1ll << 31, &c))
    return rc;
  PairRadii radii;
  SE3_REQUIRE(pg_fill_radii(&radii, radii_host, radius, num_pairs), SE3_ERR_INVALID_ARG, "%s: radius %g", name, pg_bad_radius(radii));
  hipStream_t st = (hipStream_t)stream;
  if (c.n_total > 0)
    pair_ball_count_kernel<<<(unsigned)se3_cdiv(c.n_total, kBallThreads), kBallThreads, 0, st>>>(c.G.view(), q_points, elem, c.rows, c.n_total,
                                                                                                 radii, row_offsets);
  se3_exclusive_scan_i64(row_offsets, c.n_total, st);
  SE3_CHECK_LAUNCH(name);
  return SE3_OK;
}

static int ball_fill(const char* name, const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                     const int64_t* q_offsets_host, int num_pairs, const double* radii_host, double radius, const int64_t* row_offsets,
                     int64_t total, int64_t* out, void* stream) {
  PairGridCall c;
  if (const int rc = pg_grid_call(name, "pairs", q_points && row_offsets && (out || total == 0), grid_workspace, workspace_bytes, ns_total, elem,
                                  q_offsets_host, num_pairs, 1ll << 31, &c))
    return rc;
  PairRadii radii;
  SE3_REQUIRE(pg_fill_radii(&radii, radii_host, radius, num_pairs) && total >= 0, SE3_ERR_INVALID_ARG, "%s: radius %g, total %lld", name,
              pg_bad_radius(radii), (long long)total);
  if (c.n_total == 0 || total == 0) return SE3_OK;
  pair_ball_fill_kernel<<<(unsigned)se3_cdiv(c.n_total, kBallThreads), kBallThreads, 0, (hipStream_t)stream>>>(
      c.G.view(), q_points, elem, c.rows, c.n_total, radii, row_offsets, total, out);
  SE3_CHECK_LAUNCH(name);
  return SE3_OK;
}

extern "C" int se3_pair_ball_count_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                                         const int64_t* q_offsets_host, int num_pairs, double radius, int64_t* row_offsets, void* stream) {
  return ball_count("pair_ball_count_stack", grid_workspace, workspace_bytes, ns_total, q_points, elem, q_offsets_host, num_pairs, nullptr, radius,
                    row_offsets, stream);
}

extern "C" int se3_pair_ball_fill_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                                        const int64_t* q_offsets_host, int num_pairs, double radius, const int64_t* row_offsets, int64_t total,
                                        int64_t* out, void* stream) {
  return ball_fill("pair_ball_fill_stack", grid_workspace, workspace_bytes, ns_total, q_points, elem, q_offsets_host, num_pairs, nullptr, radius,
                   row_offsets, total, out, stream);
}

extern "C" int se3_pair_ball_count_radii_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                                               const int64_t* q_offsets_host, int num_pairs, const double* radii_host, int64_t* row_offsets,
                                               void* stream) {
  SE3_REQUIRE(radii_host, SE3_ERR_INVALID_ARG, "pair_ball_count_radii_stack: null pointer");
  return ball_count("pair_ball_count_radii_stack", grid_workspace, workspace_bytes, ns_total, q_points, elem, q_offsets_host, num_pairs, radii_host,
                    0.0, row_offsets, stream);
}

extern "C" int se3_pair_ball_fill_radii_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                                              const int64_t* q_offsets_host, int num_pairs, const double* radii_host, const int64_t* row_offsets,
                                              int64_t total, int64_t* out, void* stream) {
  SE3_REQUIRE(radii_host, SE3_ERR_INVALID_ARG, "pair_ball_fill_radii_stack: null pointer");
  return ball_fill("pair_ball_fill_radii_stack", grid_workspace, workspace_bytes, ns_total, q_points, elem, q_offsets_host, num_pairs, radii_host,
                   0.0, row_offsets, total, out, stream);
}

extern "C" int se3_pair_overlap_stack(const double* nn_distances, const int64_t* q_offsets_host, int num_pairs, double radius, double* out,
                                      void* stream) {
  SE3_REQUIRE(nn_distances && q_offsets_host && out, SE3_ERR_INVALID_ARG, "pair_overlap_stack: null pointer");
  SE3_REQUIRE(num_pairs >= 0 && num_pairs <= kPairMaxPairs, SE3_ERR_INVALID_ARG, "pair_overlap_stack: %d pairs (at most %d)", num_pairs,
              kPairMaxPairs);
  SE3_REQUIRE(pg_radius_ok(radius), SE3_ERR_INVALID_ARG, "pair_overlap_stack: radius %g", radius);
  PairRows rows;
  SE3_REQUIRE(pg_fill_rows(&rows, q_offsets_host, num_pairs), SE3_ERR_INVALID_ARG, "pair_overlap_stack: offsets must start at 0 and not decrease");
  if (num_pairs == 0) return SE3_OK;
  pair_overlap_kernel<<<(unsigned)num_pairs, kRowThreads, 0, (hipStream_t)stream>>>(nn_distances, rows, radius * radius, out);
  SE3_CHECK_LAUNCH("pair_overlap_stack");
  return SE3_OK;
}

extern "C" int se3_pair_info_covariance_stack(const void* src_points, int elem, const int64_t* s_offsets_host, const double* transforms_host,
                                              const int64_t* selected, const int64_t* selected_offsets_host, int num_pairs, double* out,
                                              void* stream) {
  SE3_REQUIRE(src_points && s_offsets_host && transforms_host && selected && selected_offsets_host && out, SE3_ERR_INVALID_ARG,
              "pair_info_covariance_stack: null pointer");
  SE3_REQUIRE(num_pairs >= 0 && num_pairs <= kPairMaxPairs && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG,
              "pair_info_covariance_stack: %d pairs (at most %d), elem %d", num_pairs, kPairMaxPairs, elem);
  SE3_REQUIRE(finite_transforms(transforms_host, num_pairs), SE3_ERR_INVALID_ARG, "pair_info_covariance_stack: non-finite transform");
  PairRows src_rows, sel_rows;
  SE3_REQUIRE(pg_fill_rows(&src_rows, s_offsets_host, num_pairs) && pg_fill_rows(&sel_rows, selected_offsets_host, num_pairs), SE3_ERR_INVALID_ARG,
              "pair_info_covariance_stack: offsets must start at 0 and not decrease");
  if (num_pairs == 0) return SE3_OK;
  PairTransforms tf;
  fill_transforms(&tf, transforms_host, num_pairs);
  pair_covariance_kernel<<<(unsigned)num_pairs, kRowThreads, 0, (hipStream_t)stream>>>(src_points, elem, src_rows, tf, selected, sel_rows, out);
  SE3_CHECK_LAUNCH("pair_info_covariance_stack");
  return SE3_OK;
}

// ---- the header's search core on host memory (tests/test_pair_geometry_cpu.py) -------------------------------------------------------------
extern "C" int se3_debug_pair_nearest_neighbor_host(const void* q_points, int64_t nq, const void* s_points, int64_t ns, int elem,
                                                    const double* transform, double* distances, int64_t* indices) {
  SE3_REQUIRE(q_points && s_points && transform && distances && indices, SE3_ERR_INVALID_ARG, "debug_pair_nearest_neighbor_host: null pointer");
  SE3_REQUIRE(nq >= 0 && ns >= 0 && ns < (1ll << 31) && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG,
              "debug_pair_nearest_neighbor_host: nq %lld, ns %lld, elem %d", (long long)nq, (long long)ns, elem);
  SE3_REQUIRE(finite_transforms(transform, 1), SE3_ERR_INVALID_ARG, "debug_pair_nearest_neighbor_host: non-finite transform");
  PairHostGrid H(s_points, ns, elem, transform, 0.0);
  const PairGridView g = H.G.view();
  for (int64_t i = 0; i < nq; i++) {
    double qv[3];
    pg_load3(q_points, elem, i, qv);
    double d2;
    int j;
    pg_nearest(g, 0, qv, 0, 1, [](double*, int*) {}, &d2, &j);
    distances[i] = sqrt(d2);
    indices[i] = j;
  }
  return SE3_OK;
}

// counts (nq) always; out (capacity, 2) may be NULL (count only).  *total = the number of pairs found, which may exceed capacity (then
// only the rows that fit entirely are written).
extern "C" int se3_debug_pair_ball_host(const void* q_points, int64_t nq, const void* s_points, int64_t ns, int elem, const double* transform,
                                        double radius, int64_t* counts, int64_t* out, int64_t capacity, int64_t* total) {
  SE3_REQUIRE(q_points && s_points && transform && counts && total, SE3_ERR_INVALID_ARG, "debug_pair_ball_host: null pointer");
  SE3_REQUIRE(nq >= 0 && ns >= 0 && ns < (1ll << 31) && capacity >= 0 && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG,
              "debug_pair_ball_host: nq %lld, ns %lld, capacity %lld, elem %d", (long long)nq, (long long)ns, (long long)capacity, elem);
  SE3_REQUIRE(pg_radius_ok(radius), SE3_ERR_INVALID_ARG, "debug_pair_ball_host: radius %g", radius);
  SE3_REQUIRE(finite_transforms(transform, 1), SE3_ERR_INVALID_ARG, "debug_pair_ball_host: non-finite transform");
  PairHostGrid H(s_points, ns, elem, transform, radius);
  const PairGridView g = H.G.view();
  const double r2 = radius * radius;
  int64_t run = 0;
  for (int64_t i = 0; i < nq; i++) {
    double qv[3];
    pg_load3(q_points, elem, i, qv);
    counts[i] = pg_ball_count(g, 0, qv, radius, r2);
    if (out && run + counts[i] <= capacity) pg_ball_fill(g, 0, qv, radius, r2, i, out + 2 * run, counts[i]);
    run += counts[i];
  }
  *total = run;
  return SE3_OK;
}
