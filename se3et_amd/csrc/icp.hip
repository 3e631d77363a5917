// ICP refinement of stacked pairs, resident on the device: Open3D's registration_icp with TransformationEstimationPointToPoint (no
// scale) or TransformationEstimationPointToPlane, for up to SE3_PAIR_MAX_PAIRS pairs per call and without a host round trip per
// iteration.  csrc/icp_core.h holds the iteration as __host__ __device__ text, csrc/pair_grid.h the search, csrc/kabsch.h the 3x3 solve;
// se3et_amd/icp.py carries the same contract.
// (SE3_EXACT_FP: the file is built with contraction off, and every contract function fences itself as well.)
//
//   icp_init_kernel      one workgroup per pair, once: T <- T0, the finiteness check.
//   icp_nearest_kernel   (a) one wave per stacked source row: the row moved by its pair's current T, the pair_grid.h nearest-neighbour walk,
//                        (index, d^2) to the workspace.
//   icp_step_kernel      (b) one workgroup per pair: fitness, rmse, the convergence test, and for a pair that goes on the fixed-order sums,
//                        the solve and T <- U T.
//   A call enqueues init and then (a), (b) max_iteration + 1 times; nothing waits on the host.  Every pair has a `done` word on the
//   device: the kernels of a converged, stopped or refused pair read it (uniform over the wave / the workgroup) and return.
//
// Contract.  Pair p has a source cloud, a reference cloud and an initial transform T0_p with ref ~ T src.  Everything is float64; points
// and normals may be float32 (elem 0) or float64 (elem 1) and are promoted on load.
//   Evaluation under T.  Every source row is moved by pg_transform (the fma chain of pair_geometry.hip); its exact nearest reference point
//     q is taken, the lowest index among equal distances; d^2 = (dx dx + dy dy) + dz dz, unfused.  The row is a correspondence iff
//     d^2 < r^2 (r = max_correspondence_distance; strict, like se3_pair_overlap_stack).  fitness = n_corr / n_src (0 for an empty source);
//     inlier_rmse = sqrt(sum d^2 / n_corr), 0 without a correspondence.
//   Loop (Open3D's defaults: relative_fitness = relative_rmse = 1e-6, max_iteration = 30).  E_0 = evaluate(T0).  For k = 1 ..
//     max_iteration: T_k = U_k T_(k-1) with U_k estimated from the correspondences of E_(k-1); E_k = evaluate(T_k); the pair stops with
//     converged = 1 when |fitness_k - fitness_(k-1)| < relative_fitness and |rmse_k - rmse_(k-1)| < relative_rmse.  iterations = the k of
//     the last evaluation; max_iteration = 0 evaluates only.  The accumulated T_k is always applied to the ORIGINAL source (Open3D moves
//     its copy of the cloud by each U_k in turn: a difference of rounding only).
//   Point-to-point.  Kabsch without scale over the correspondences (p = T src_i, q): centroids, the 3x3 cross-covariance about the
//     centroids, the rotation from kabsch.h, t = qc - R pc.
//   Point-to-plane.  Residual r_i = (p - q) . n with n the reference normal of q; J_i = [p x n, n]; (sum J^T J) x = -sum J^T r by a 6x6
//     Cholesky factorisation; U = [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5] (Open3D's TransformVector6dToMatrix4d).  sin and cos are one shared
//     series (icp_sin / icp_cos), since the host's and the device's libraries differ.  A step with an |angle| >= 1 rad sets
//     SE3_ICP_STEP_REFUSED and ends the pair at its previous transform, converged = 0: a linearised step of that size is not a refinement
//     (Open3D applies it).
//   Degenerate cases.  The update is the identity -- and the pair ends at the next comparison, its result being unchanged -- with fewer
//     than 3 (point-to-point) or 6 (point-to-plane) correspondences (SE3_ICP_TOO_FEW), with a system that is not positive definite, i.e. a
//     Cholesky pivot not above 1e-13 of its diagonal entry (SE3_ICP_SINGULAR), and with an empty cloud (SE3_ICP_EMPTY).  A non-finite
//     point, normal or T0 refuses the pair: SE3_ICP_NONFINITE, a NaN transform, correspondences -1; the other pairs are unaffected.
//   Sums.  No float atomics.  Every sum over a pair's rows is formed by lane l of 256 adding rows l, l + 256, .. serially and a fixed
//     tree over the lanes (icp_sum), so it depends on the pair's row count alone: results are bit-identical from run to run, for a pair
//     alone and anywhere in a batch, and between the device and se3_debug_icp_host.
//   No robust loss kernels, no captured graphs.
#include <math.h>

#include <vector>

#include "common.h"
#include "icp_core.h"          // (and through it pair_grid.h and kabsch.h)

namespace {

constexpr int kIcpNnWaves = 4;          // source rows per nearest-neighbour workgroup

struct IcpLayout {
  int* nn_idx;
  double* nn_d2;
  int* done;
};

size_t icp_carve(int64_t nsrc_total, int num_pairs, char* base, IcpLayout* L) {
  Se3Carver c(base);
  IcpLayout l;
  l.nn_idx = c.take<int>((size_t)(nsrc_total > 0 ? nsrc_total : 1));
  l.nn_d2 = c.take<double>((size_t)(nsrc_total > 0 ? nsrc_total : 1));
  l.done = c.take<int>((size_t)(num_pairs > 0 ? num_pairs : 1));
  if (L) *L = l;
  return c.bytes();
}

// what the kernels get: the stacked arrays of a call
struct IcpCall {
  const void* src;
  int elem;
  PairRows rows;                  // source rows of every pair
  const double* ref;              // the grid's `moved`
  const void* normals;
  int normals_elem;
  IcpLayout ws;
  double* T;
  double* fitness;
  double* rmse;
  int* iterations;
  int* converged;
  int* status;
  int64_t* corr;
};

__host__ __device__ IcpPair icp_pair_of(const IcpCall& c, const PairGridMeta* meta, int p) {
  IcpPair v;
  const int64_t s0 = c.rows.start[p], r0 = meta[p].s_start;
  v.src = c.elem ? (const void*)((const double*)c.src + 3 * s0) : (const void*)((const float*)c.src + 3 * s0);
  v.elem = c.elem;
  v.n = c.rows.start[p + 1] - s0;
  v.ref = c.ref + 3 * r0;
  v.nref = meta[p].ns;
  v.normals = !c.normals ? nullptr
                         : (c.normals_elem ? (const void*)((const double*)c.normals + 3 * r0) : (const void*)((const float*)c.normals + 3 * r0));
  v.normals_elem = c.normals_elem;
  v.nn_idx = c.ws.nn_idx + s0, v.nn_d2 = c.ws.nn_d2 + s0;
  v.T = c.T + 16 * p, v.fitness = c.fitness + p, v.rmse = c.rmse + p;
  v.iterations = c.iterations + p, v.converged = c.converged + p, v.status = c.status + p, v.done = c.ws.done + p;
  v.corr = c.corr ? c.corr + s0 : nullptr;
  return v;
}

__global__ __launch_bounds__(kIcpLanes) void icp_init_kernel(IcpCall c, const PairGridMeta* __restrict__ meta, const double* __restrict__ T0,
                                                             int mode) {
  __shared__ double sh[kIcpLanes];
  const IcpPair v = icp_pair_of(c, meta, blockIdx.x);
  icp_pair_init(v, T0 + 16 * blockIdx.x, mode, threadIdx.x, threadIdx.x + 1, sh, [] { __syncthreads(); });
}

__global__ __launch_bounds__(kIcpNnWaves* SE3_WAVE) void icp_nearest_kernel(PairGridView g, IcpCall c, int64_t n_total) {
  const int64_t i = (int64_t)blockIdx.x * kIcpNnWaves + (threadIdx.x >> 6);
  if (i >= n_total) return;                                // (uniform over the wave)
  const int p = pg_pair_of_row(c.rows, i);
  if (c.ws.done[p]) return;                                // (one word per pair: uniform over the wave)
  double T[12], qv[3];
  for (int k = 0; k < 12; k++) T[k] = c.T[16 * p + k];
  pg_transform_row(T, c.src, c.elem, i, qv);
  double d2;
  int j;
  pg_wave_nearest(g, p, qv, &d2, &j);
  if (se3_lane() == 0) {
    c.ws.nn_idx[i] = j;
    c.ws.nn_d2[i] = d2;
  }
}

__global__ __launch_bounds__(kIcpLanes) void icp_step_kernel(IcpCall c, const PairGridMeta* __restrict__ meta, IcpCriteria crit, int k) {
  __shared__ double sh[kIcpMaxSums * kIcpLanes];
  const IcpPair v = icp_pair_of(c, meta, blockIdx.x);
  icp_pair_step(v, crit, k, threadIdx.x, threadIdx.x + 1, sh, [] { __syncthreads(); });
}

bool icp_criteria(IcpCriteria* crit, double r, int mode, double relative_fitness, double relative_rmse, int max_iteration) {
  if (!pg_radius_ok(r) || (mode != SE3_ICP_POINT_TO_POINT && mode != SE3_ICP_POINT_TO_PLANE)) return false;
  if (!(relative_fitness >= 0.0) || !(relative_rmse >= 0.0) || max_iteration < 0 || max_iteration > SE3_ICP_MAX_ITERATION) return false;
  crit->r2 = r * r, crit->relative_fitness = relative_fitness, crit->relative_rmse = relative_rmse;
  crit->max_iteration = max_iteration, crit->mode = mode;
  return true;
}

}  // namespace

extern "C" size_t se3_icp_workspace_bytes(int64_t nsrc_total, int num_pairs) {
  if (nsrc_total < 0 || num_pairs < 0 || num_pairs > kPairMaxPairs) return 0;
  return icp_carve(nsrc_total, num_pairs, nullptr, nullptr);
}

extern "C" int se3_icp_stack(const void* grid_workspace, size_t grid_workspace_bytes, int64_t nref_total, const void* src_points, int elem,
                             const int64_t* src_offsets_host, int num_pairs, const void* ref_normals, int normals_elem, const double* T0,
                             double max_correspondence_distance, int mode, double relative_fitness, double relative_rmse, int max_iteration,
                             double* out_transforms, double* out_fitness, double* out_rmse, int* out_iterations, int* out_converged,
                             int* out_status, int64_t* out_correspondences, void* workspace, size_t workspace_bytes, void* stream) {
  SE3_REQUIRE(grid_workspace && src_points && src_offsets_host && T0 && workspace, SE3_ERR_INVALID_ARG, "icp_stack: null pointer");
  SE3_REQUIRE(out_transforms && out_fitness && out_rmse && out_iterations && out_converged && out_status, SE3_ERR_INVALID_ARG,
              "icp_stack: null result pointer");
  SE3_REQUIRE(num_pairs >= 0 && num_pairs <= kPairMaxPairs && nref_total >= 0 && (elem == 0 || elem == 1) && (normals_elem == 0 || normals_elem == 1),
              SE3_ERR_INVALID_ARG, "icp_stack: %d pairs (at most %d), nref_total %lld, elem %d, normals_elem %d", num_pairs, kPairMaxPairs,
              (long long)nref_total, elem, normals_elem);
  IcpCriteria crit;
  SE3_REQUIRE(icp_criteria(&crit, max_correspondence_distance, mode, relative_fitness, relative_rmse, max_iteration), SE3_ERR_INVALID_ARG,
              "icp_stack: distance %g, mode %d, criteria %g %g %d (at most %d iterations)", max_correspondence_distance, mode, relative_fitness,
              relative_rmse, max_iteration, SE3_ICP_MAX_ITERATION);
  SE3_REQUIRE(mode != SE3_ICP_POINT_TO_PLANE || ref_normals, SE3_ERR_INVALID_ARG, "icp_stack: point-to-plane needs the reference normals");
  PairGridCall gc;                // (the count above and the row bound below are worded by this entry: the call makes the other checks)
  if (const int rc = pg_grid_call("icp_stack", "pairs", true, grid_workspace, grid_workspace_bytes, nref_total, elem, src_offsets_host, num_pairs,
                                  INT64_MAX, &gc))
    return rc;
  const int64_t n_total = gc.n_total;
  SE3_REQUIRE(n_total < (1ll << 31), SE3_ERR_UNSUPPORTED, "icp_stack: %lld source rows in one call", (long long)n_total);
  const PairGridLayout& G = gc.G;
  IcpCall c;
  c.rows = gc.rows;
  SE3_REQUIRE(icp_carve(n_total, num_pairs, (char*)workspace, &c.ws) <= workspace_bytes, SE3_ERR_WORKSPACE,
              "icp_stack: workspace of %zu bytes is too small", workspace_bytes);
  if (num_pairs == 0) return SE3_OK;
  c.src = src_points, c.elem = elem, c.ref = G.moved, c.normals = ref_normals, c.normals_elem = normals_elem;
  c.T = out_transforms, c.fitness = out_fitness, c.rmse = out_rmse, c.iterations = out_iterations, c.converged = out_converged;
  c.status = out_status, c.corr = out_correspondences;
  hipStream_t st = (hipStream_t)stream;
  icp_init_kernel<<<(unsigned)num_pairs, kIcpLanes, 0, st>>>(c, G.meta, T0, mode);
  for (int k = 0; k <= max_iteration; k++) {
    if (n_total > 0) icp_nearest_kernel<<<(unsigned)se3_cdiv(n_total, kIcpNnWaves), kIcpNnWaves * SE3_WAVE, 0, st>>>(G.view(), c, n_total);
    icp_step_kernel<<<(unsigned)num_pairs, kIcpLanes, 0, st>>>(c, G.meta, crit, k);
  }
  SE3_CHECK_LAUNCH("icp_stack");
  return SE3_OK;
}

// ---- the same text on host memory, one pair, no GPU (tests/test_icp_cpu.py) -------------------------------------------------------------------
// trace: NULL, or (max_iteration + 1, n) int64: row k receives evaluation k's correspondence of every source row (-1 for none); the rows
// of evaluations that were not made are left as they are.
extern "C" int se3_debug_icp_host(const void* src_points, int64_t n, const void* ref_points, int64_t nref, int elem, const void* ref_normals,
                                  int normals_elem, const double* T0, double max_correspondence_distance, int mode, double relative_fitness,
                                  double relative_rmse, int max_iteration, double* out_transform, double* out_fitness, double* out_rmse,
                                  int* out_iterations, int* out_converged, int* out_status, int64_t* out_correspondences, int64_t* trace) {
  SE3_REQUIRE(src_points && ref_points && T0, SE3_ERR_INVALID_ARG, "debug_icp_host: null pointer");
  SE3_REQUIRE(out_transform && out_fitness && out_rmse && out_iterations && out_converged && out_status, SE3_ERR_INVALID_ARG,
              "debug_icp_host: null result pointer");
  SE3_REQUIRE(n >= 0 && n < (1ll << 31) && nref >= 0 && nref < (1ll << 31) && (elem == 0 || elem == 1) && (normals_elem == 0 || normals_elem == 1),
              SE3_ERR_INVALID_ARG, "debug_icp_host: n %lld, nref %lld, elem %d, normals_elem %d", (long long)n, (long long)nref, elem, normals_elem);
  IcpCriteria crit;
  SE3_REQUIRE(icp_criteria(&crit, max_correspondence_distance, mode, relative_fitness, relative_rmse, max_iteration), SE3_ERR_INVALID_ARG,
              "debug_icp_host: distance %g, mode %d, criteria %g %g %d (at most %d iterations)", max_correspondence_distance, mode,
              relative_fitness, relative_rmse, max_iteration, SE3_ICP_MAX_ITERATION);
  SE3_REQUIRE(mode != SE3_ICP_POINT_TO_PLANE || ref_normals, SE3_ERR_INVALID_ARG, "debug_icp_host: point-to-plane needs the reference normals");
  PairHostGrid H(ref_points, nref, elem, nullptr, max_correspondence_distance);
  const PairGridLayout& G = H.G;
  std::vector<int> nn_idx((size_t)n + 1);
  std::vector<double> nn_d2((size_t)n + 1), sh((size_t)kIcpMaxSums * kIcpLanes);
  int done = 0;
  IcpCall c;
  c.rows = pg_single_rows(n);
  c.src = src_points, c.elem = elem, c.ref = G.moved, c.normals = ref_normals, c.normals_elem = normals_elem;
  c.ws.nn_idx = nn_idx.data(), c.ws.nn_d2 = nn_d2.data(), c.ws.done = &done;
  c.T = out_transform, c.fitness = out_fitness, c.rmse = out_rmse, c.iterations = out_iterations, c.converged = out_converged;
  c.status = out_status, c.corr = out_correspondences;
  const IcpPair v = icp_pair_of(c, G.meta, 0);
  const PairGridView g = G.view();
  icp_pair_init(v, T0, mode, 0, kIcpLanes, sh.data(), [] {});
  for (int k = 0; k <= max_iteration && !done; k++) {
    for (int64_t i = 0; i < n; i++) {
      double qv[3];
      icp_moved(v, v.T, i, qv);
      pg_nearest(g, 0, qv, 0, 1, [](double*, int*) {}, &nn_d2[(size_t)i], &nn_idx[(size_t)i]);
      if (trace) trace[(int64_t)k * n + i] = nn_d2[(size_t)i] < crit.r2 ? nn_idx[(size_t)i] : -1;
    }
    icp_pair_step(v, crit, k, 0, kIcpLanes, sh.data(), [] {});
  }
  return SE3_OK;
}

extern "C" int se3_debug_icp_sincos_host(const double* x, int64_t n, double* out_sin, double* out_cos) {
  SE3_REQUIRE(x && out_sin && out_cos && n >= 0, SE3_ERR_INVALID_ARG, "debug_icp_sincos_host: null pointer or n %lld", (long long)n);
  for (int64_t i = 0; i < n; i++) {
    SE3_REQUIRE(fabs(x[i]) < kIcpMaxAngle, SE3_ERR_INVALID_ARG, "debug_icp_sincos_host: %g is outside (-1, 1)", x[i]);
    out_sin[i] = icp_sin(x[i]), out_cos[i] = icp_cos(x[i]);
  }
  return SE3_OK;
}
