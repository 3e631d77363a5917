// ICP refinement of stacked pairs, resident on the device: Open3D's registration_icp with TransformationEstimationPointToPoint (no
// scale) or TransformationEstimationPointToPlane, and its registration_generalized_icp in the normals form, each with or without one of
// Open3D's robust loss kernels, for up to SE3_PAIR_MAX_PAIRS pairs per call and without a host round trip per iteration.  csrc/icp_core.h holds the iteration as __host__ __device__ text, csrc/pair_grid.h the search, csrc/kabsch.h the 3x3 solve;
// se3et_amd/icp.py carries the same contract.
// (SE3_EXACT_FP: the file is built with contraction off, and every contract function fences itself as well.)
//
//   icp_init_kernel      one workgroup per pair, once: T <- T0, the finiteness check.
//   icp_nearest_kernel   (a) one wave per stacked source row: the row moved by its pair's current T, the pair_grid.h nearest-neighbour walk,
//                        (index, d^2) to the workspace.
//   icp_step_kernel      (b) one workgroup per pair: fitness, rmse, the convergence test, and for a pair that goes on the fixed-order sums,
//                        the solve and T <- U T.  <kWeighted, kGeneral>: four instantiations; <false, false> is se3_icp_stack's and holds no
//                        weight code, so a call without a loss gives the bits it gave before the losses existed.  kGeneral keeps 27 sum
//                        columns in LDS (27 x 256 doubles = 54 KiB of the 64 KiB a workgroup may declare; one workgroup per pair, so the
//                        occupancy it costs is of no account) and forms them in ONE pass over the rows: the row's M^-1 is formed once.
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
//   Loss kernels (se3_icp_weighted_stack; se3_icp_stack has none).  Open3D's RobustKernel weights of a scalar residual r, k > 0:
//     l2: 1;  huber: 1 for |r| <= k, else k / |r|;  cauchy: 1 / (1 + (r / k)^2);  gm: k / (k + r^2)^2;  tukey: (1 - (r / k)^2)^2 for
//     |r| <= k, else 0.  Every weight is continuous at its branch.  Open3D's L1Loss is not offered: its weight 1 / |r| is unbounded at an
//     exact match, and huber covers its use.  Iteratively reweighted least squares, the weights from the current evaluation; the
//     evaluation itself (correspondences, fitness, inlier_rmse), the loop, the too-few counts (which count correspondences, not weights)
//     and the status bits are untouched.
//     Point-to-plane: w_i = w(r_i), (sum w_i J_i^T J_i) x = -sum w_i J_i^T r_i: Open3D's TransformationEstimationPointToPlane(kernel).
//       Weights that leave the system rank-deficient are caught by the pivot test.
//     Point-to-point: w_i = w(sqrt(d_i^2)) and the weighted Kabsch pc = sum w p / W, qc = sum w q / W, H = sum w (p - pc)(q - qc)^T,
//       W = sum w.  A W that is not > 0 is SE3_ICP_SINGULAR with the identity update (tukey with every correspondence beyond k).
//       Open3D's legacy point-to-point takes no kernel: this is the project's definition.
//   Generalized ICP (SE3_ICP_GENERALIZED).  Open3D's registration_generalized_icp with the covariances of its normals form: a point with
//     unit normal n has C = I - (1 - eps) n n^T (= R diag(eps, 1, 1) R^T with n the first column of R), eps = gicp_epsilon in (0, 1],
//     Open3D's default 1e-3.  It needs the unit normals of BOTH clouds and nothing else, and does not depend on a normal's sign.  For a
//     correspondence under T = [R | t]: p the moved source row, q its reference row, nt the normal of q, m = R ns the source normal turned
//     by T, d = p - q, M = 2 I - (1 - eps)(nt nt^T + m m^T) (eigenvalues >= 2 eps) inverted by its cofactors, A = [-[p]_x | I];
//     (sum w A^T M^-1 A) x = -sum w A^T M^-1 d, then the solve, the 1 rad refusal and the update matrix of point-to-plane.  The too-few
//     count is 6; fitness and inlier_rmse stay Euclidean, as Open3D's result fields are.  A non-finite source normal refuses the pair.
//     The loss acts on the Mahalanobis residual: w = w(sqrt(d^T M^-1 d)).  Open3D weights the three rows of M^(-1/2) d one by one, which
//     needs a matrix square root; with l2 the two systems are the same in exact arithmetic.
//   Coloured ICP (se3_icp_colored_stack; csrc/icp_colored_core.h, the gradients from csrc/color_gradient.hip).  Open3D's
//     registration_colored_icp: TransformationEstimationForColoredICP(lambda_geometric, kernel).  Evaluation, the loop and the convergence
//     rule, the application of the accumulated T_k to the original source, the 256-lane serial sums with the fixed tree, the 6x6 Cholesky
//     solve with its 1e-13 pivot rule, the update matrix and its shared sin / cos series, the 1 rad refusal, the status bits and the
//     correspondences are the text above; only the per-correspondence term is new.  For a correspondence under T = [R | t]: p the moved
//     source row, q its reference row, nt that row's normal as given, I_t its intensity, g its gradient (color_gradient.hip), I_s the
//     source row's intensity (an intensity is ((c0 + c1) + c2) / 3.0), lambda = lambda_geometric in [0, 1] (Open3D's default 0.968),
//     a = sqrt(lambda), b = sqrt(1 - lambda).
//     Geometric row.  r_g = a (p - q) . nt, J_g = a [p x nt, nt].
//     Photometric row.  p' = p - ((p - q) . nt) nt, I_proj = g . (p' - q) + I_t, r_c = b (I_s - I_proj), d = -(M g) with
//       M = I - nt nt^T, J_c = b [p x d, d].
//     System.  (sum w_g J_g J_g^T + w_c J_c J_c^T) x = -sum (w_g J_g r_g + w_c J_c r_c), w_g = w(r_g), w_c = w(r_c) from the loss table
//       above; SE3_ICP_LOSS_NONE gives weights 1 and no weight code.  The 27 sums are formed in one pass, as generalized ICP's.
//     Degenerate cases follow point-to-plane: fewer than 6 correspondences SE3_ICP_TOO_FEW, a failed pivot SE3_ICP_SINGULAR, an empty
//       cloud SE3_ICP_EMPTY; a non-finite point, normal, colour, gradient or T0 sets SE3_ICP_NONFINITE for that pair alone.
//   No captured graphs.
#include <math.h>

#include <vector>

#include "common.h"
#include "icp_colored_core.h"  // (and through it icp_core.h, pair_grid.h and kabsch.h)

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
  const void* src_normals;        // generalized ICP alone
  int src_normals_elem;
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
  v.src_normals = !c.src_normals ? nullptr
                                 : (c.src_normals_elem ? (const void*)((const double*)c.src_normals + 3 * s0)
                                                       : (const void*)((const float*)c.src_normals + 3 * s0));
  v.src_normals_elem = c.src_normals_elem;
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

template <bool kWeighted, bool kGeneral>
__global__ __launch_bounds__(kIcpLanes) void icp_step_kernel(IcpCall c, const PairGridMeta* __restrict__ meta, IcpCriteria crit, int k) {
  __shared__ double sh[(kGeneral ? kIcpGeneralSums : kIcpMaxSums) * kIcpLanes];
  const IcpPair v = icp_pair_of(c, meta, blockIdx.x);
  icp_pair_step<kWeighted, kGeneral>(v, crit, k, threadIdx.x, threadIdx.x + 1, sh, [] { __syncthreads(); });
}

using IcpStepKernel = void (*)(IcpCall, const PairGridMeta*, IcpCriteria, int);
IcpStepKernel icp_step_kernel_of(const IcpCriteria& crit) {
  const bool weighted = crit.loss != SE3_ICP_LOSS_NONE;
  if (crit.mode == SE3_ICP_GENERALIZED) return weighted ? icp_step_kernel<true, true> : icp_step_kernel<false, true>;
  return weighted ? icp_step_kernel<true, false> : icp_step_kernel<false, false>;
}

// coloured ICP: the stacked colours and gradients of a call, beside IcpCall
struct IcpColorCall {
  const void* src_colors;         // stacked source rows
  int src_colors_elem;
  const void* ref_colors;         // stacked reference rows
  int ref_colors_elem;
  const double* gradients;        // stacked reference rows
  double a, b;
};

__host__ __device__ IcpColors icp_colors_of(const IcpColorCall& cc, const IcpCall& c, const PairGridMeta* meta, int p) {
  IcpColors v;
  const int64_t s0 = c.rows.start[p], r0 = meta[p].s_start;
  v.src_colors = cc.src_colors_elem ? (const void*)((const double*)cc.src_colors + 3 * s0) : (const void*)((const float*)cc.src_colors + 3 * s0);
  v.src_colors_elem = cc.src_colors_elem;
  v.ref_colors = cc.ref_colors_elem ? (const void*)((const double*)cc.ref_colors + 3 * r0) : (const void*)((const float*)cc.ref_colors + 3 * r0);
  v.ref_colors_elem = cc.ref_colors_elem;
  v.gradients = cc.gradients + 3 * r0;
  v.a = cc.a, v.b = cc.b;
  return v;
}

__global__ __launch_bounds__(kIcpLanes) void icp_colored_init_kernel(IcpCall c, IcpColorCall cc, const PairGridMeta* __restrict__ meta,
                                                                     const double* __restrict__ T0) {
  __shared__ double sh[kIcpLanes];
  const IcpPair v = icp_pair_of(c, meta, blockIdx.x);
  icp_colored_pair_init(v, icp_colors_of(cc, c, meta, blockIdx.x), T0 + 16 * blockIdx.x, threadIdx.x, threadIdx.x + 1, sh,
                        [] { __syncthreads(); });
}

template <bool kWeighted>
__global__ __launch_bounds__(kIcpLanes) void icp_colored_step_kernel(IcpCall c, IcpColorCall cc, const PairGridMeta* __restrict__ meta,
                                                                     IcpCriteria crit, int k) {
  __shared__ double sh[kIcpGeneralSums * kIcpLanes];
  const IcpPair v = icp_pair_of(c, meta, blockIdx.x);
  icp_colored_pair_step<kWeighted>(v, icp_colors_of(cc, c, meta, blockIdx.x), crit, k, threadIdx.x, threadIdx.x + 1, sh, [] { __syncthreads(); });
}

// one step of the host entries
void icp_host_step(const IcpPair& v, const IcpCriteria& crit, int k, double* sh) {
  const bool weighted = crit.loss != SE3_ICP_LOSS_NONE;
  auto none = [] {};
  if (crit.mode == SE3_ICP_GENERALIZED) {
    if (weighted) icp_pair_step<true, true>(v, crit, k, 0, kIcpLanes, sh, none);
    else icp_pair_step<false, true>(v, crit, k, 0, kIcpLanes, sh, none);
  } else {
    if (weighted) icp_pair_step<true, false>(v, crit, k, 0, kIcpLanes, sh, none);
    else icp_pair_step<false, false>(v, crit, k, 0, kIcpLanes, sh, none);
  }
}

bool icp_criteria(IcpCriteria* crit, double r, int mode, double relative_fitness, double relative_rmse, int max_iteration) {
  if (!pg_radius_ok(r) || (mode != SE3_ICP_POINT_TO_POINT && mode != SE3_ICP_POINT_TO_PLANE && mode != SE3_ICP_GENERALIZED)) return false;
  if (!(relative_fitness >= 0.0) || !(relative_rmse >= 0.0) || max_iteration < 0 || max_iteration > SE3_ICP_MAX_ITERATION) return false;
  crit->r2 = r * r, crit->relative_fitness = relative_fitness, crit->relative_rmse = relative_rmse;
  crit->max_iteration = max_iteration, crit->mode = mode;
  crit->loss = SE3_ICP_LOSS_NONE, crit->loss_k = 1.0, crit->eps = 1.0;
  return true;
}

// the loss, its width and generalized ICP's epsilon of the weighted entries
bool icp_loss_criteria(IcpCriteria* crit, int loss, double loss_k, double eps) {
  if (loss != SE3_ICP_LOSS_NONE && (loss < SE3_ICP_LOSS_L2 || loss > SE3_ICP_LOSS_TUKEY)) return false;
  if (!(loss_k > 0.0) || !(loss_k < INFINITY) || !(eps > 0.0) || !(eps <= 1.0)) return false;
  crit->loss = loss, crit->loss_k = loss_k, crit->eps = eps;
  return true;
}

}  // namespace

extern "C" size_t se3_icp_workspace_bytes(int64_t nsrc_total, int num_pairs) {
  if (nsrc_total < 0 || num_pairs < 0 || num_pairs > kPairMaxPairs) return 0;
  return icp_carve(nsrc_total, num_pairs, nullptr, nullptr);
}

namespace {

// the body of se3_icp_stack and se3_icp_weighted_stack (`what` words the errors); crit is checked
int icp_stack_run(const char* what, const IcpCriteria& crit, const void* grid_workspace, size_t grid_workspace_bytes, int64_t nref_total,
                  const void* src_points, int elem, const int64_t* src_offsets_host, int num_pairs, const void* ref_normals, int normals_elem,
                  const void* src_normals, int src_normals_elem, const double* T0, double* out_transforms, double* out_fitness, double* out_rmse,
                  int* out_iterations, int* out_converged, int* out_status, int64_t* out_correspondences, void* workspace,
                  size_t workspace_bytes, void* stream, const IcpColorCall* colors = nullptr) {
  SE3_REQUIRE(grid_workspace && src_points && src_offsets_host && T0 && workspace, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(out_transforms && out_fitness && out_rmse && out_iterations && out_converged && out_status, SE3_ERR_INVALID_ARG,
              "%s: null result pointer", what);
  SE3_REQUIRE(num_pairs >= 0 && num_pairs <= kPairMaxPairs && nref_total >= 0 && (elem == 0 || elem == 1) && (normals_elem == 0 || normals_elem == 1) &&
                  (src_normals_elem == 0 || src_normals_elem == 1),
              SE3_ERR_INVALID_ARG, "%s: %d pairs (at most %d), nref_total %lld, elem %d, normals_elem %d, src_normals_elem %d", what, num_pairs,
              kPairMaxPairs, (long long)nref_total, elem, normals_elem, src_normals_elem);
  SE3_REQUIRE(crit.mode == SE3_ICP_POINT_TO_POINT || ref_normals, SE3_ERR_INVALID_ARG, "%s: %s needs the reference normals", what,
              crit.mode == SE3_ICP_GENERALIZED ? "generalized" : "point-to-plane");
  SE3_REQUIRE(crit.mode != SE3_ICP_GENERALIZED || src_normals, SE3_ERR_INVALID_ARG, "%s: generalized needs the source normals", what);
  PairGridCall gc;                // (the count above and the row bound below are worded by this entry: the call makes the other checks)
  if (const int rc = pg_grid_call(what, "pairs", true, grid_workspace, grid_workspace_bytes, nref_total, elem, src_offsets_host, num_pairs,
                                  INT64_MAX, &gc))
    return rc;
  const int64_t n_total = gc.n_total;
  SE3_REQUIRE(n_total < (1ll << 31), SE3_ERR_UNSUPPORTED, "%s: %lld source rows in one call", what, (long long)n_total);
  const PairGridLayout& G = gc.G;
  IcpCall c;
  c.rows = gc.rows;
  SE3_REQUIRE(icp_carve(n_total, num_pairs, (char*)workspace, &c.ws) <= workspace_bytes, SE3_ERR_WORKSPACE,
              "%s: workspace of %zu bytes is too small", what, workspace_bytes);
  if (num_pairs == 0) return SE3_OK;
  c.src = src_points, c.elem = elem, c.ref = G.moved, c.normals = ref_normals, c.normals_elem = normals_elem;
  c.src_normals = crit.mode == SE3_ICP_GENERALIZED ? src_normals : nullptr, c.src_normals_elem = src_normals_elem;
  c.T = out_transforms, c.fitness = out_fitness, c.rmse = out_rmse, c.iterations = out_iterations, c.converged = out_converged;
  c.status = out_status, c.corr = out_correspondences;
  hipStream_t st = (hipStream_t)stream;
  if (colors) {                   // se3_icp_colored_stack: its own init and step kernels round the same search
    const bool weighted = crit.loss != SE3_ICP_LOSS_NONE;
    icp_colored_init_kernel<<<(unsigned)num_pairs, kIcpLanes, 0, st>>>(c, *colors, G.meta, T0);
    for (int k = 0; k <= crit.max_iteration; k++) {
      if (n_total > 0) icp_nearest_kernel<<<(unsigned)se3_cdiv(n_total, kIcpNnWaves), kIcpNnWaves * SE3_WAVE, 0, st>>>(G.view(), c, n_total);
      if (weighted) icp_colored_step_kernel<true><<<(unsigned)num_pairs, kIcpLanes, 0, st>>>(c, *colors, G.meta, crit, k);
      else icp_colored_step_kernel<false><<<(unsigned)num_pairs, kIcpLanes, 0, st>>>(c, *colors, G.meta, crit, k);
    }
    SE3_CHECK_LAUNCH(what);
    return SE3_OK;
  }
  const IcpStepKernel step = icp_step_kernel_of(crit);
  icp_init_kernel<<<(unsigned)num_pairs, kIcpLanes, 0, st>>>(c, G.meta, T0, crit.mode);
  for (int k = 0; k <= crit.max_iteration; k++) {
    if (n_total > 0) icp_nearest_kernel<<<(unsigned)se3_cdiv(n_total, kIcpNnWaves), kIcpNnWaves * SE3_WAVE, 0, st>>>(G.view(), c, n_total);
    step<<<(unsigned)num_pairs, kIcpLanes, 0, st>>>(c, G.meta, crit, k);
  }
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

}  // namespace

extern "C" int se3_icp_stack(const void* grid_workspace, size_t grid_workspace_bytes, int64_t nref_total, const void* src_points, int elem,
                             const int64_t* src_offsets_host, int num_pairs, const void* ref_normals, int normals_elem, const double* T0,
                             double max_correspondence_distance, int mode, double relative_fitness, double relative_rmse, int max_iteration,
                             double* out_transforms, double* out_fitness, double* out_rmse, int* out_iterations, int* out_converged,
                             int* out_status, int64_t* out_correspondences, void* workspace, size_t workspace_bytes, void* stream) {
  IcpCriteria crit;
  SE3_REQUIRE(mode != SE3_ICP_GENERALIZED && icp_criteria(&crit, max_correspondence_distance, mode, relative_fitness, relative_rmse, max_iteration),
              SE3_ERR_INVALID_ARG, "icp_stack: distance %g, mode %d, criteria %g %g %d (at most %d iterations)", max_correspondence_distance, mode,
              relative_fitness, relative_rmse, max_iteration, SE3_ICP_MAX_ITERATION);
  return icp_stack_run("icp_stack", crit, grid_workspace, grid_workspace_bytes, nref_total, src_points, elem, src_offsets_host, num_pairs,
                       ref_normals, normals_elem, nullptr, 0, T0, out_transforms, out_fitness, out_rmse, out_iterations, out_converged,
                       out_status, out_correspondences, workspace, workspace_bytes, stream);
}

extern "C" size_t se3_icp_weighted_workspace_bytes(int64_t nsrc_total, int num_pairs) { return se3_icp_workspace_bytes(nsrc_total, num_pairs); }

extern "C" int se3_icp_weighted_stack(const void* grid_workspace, size_t grid_workspace_bytes, int64_t nref_total, const void* src_points,
                                      int elem, const int64_t* src_offsets_host, int num_pairs, const void* ref_normals, int normals_elem,
                                      const void* src_normals, int src_normals_elem, const double* T0, double max_correspondence_distance,
                                      int mode, int loss, double loss_k, double gicp_epsilon, double relative_fitness, double relative_rmse,
                                      int max_iteration, double* out_transforms, double* out_fitness, double* out_rmse, int* out_iterations,
                                      int* out_converged, int* out_status, int64_t* out_correspondences, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  IcpCriteria crit;
  SE3_REQUIRE(icp_criteria(&crit, max_correspondence_distance, mode, relative_fitness, relative_rmse, max_iteration), SE3_ERR_INVALID_ARG,
              "icp_weighted_stack: distance %g, mode %d, criteria %g %g %d (at most %d iterations)", max_correspondence_distance, mode,
              relative_fitness, relative_rmse, max_iteration, SE3_ICP_MAX_ITERATION);
  SE3_REQUIRE(icp_loss_criteria(&crit, loss, loss_k, gicp_epsilon), SE3_ERR_INVALID_ARG,
              "icp_weighted_stack: loss %d, loss_k %g (positive and finite), gicp_epsilon %g (in (0, 1])", loss, loss_k, gicp_epsilon);
  return icp_stack_run("icp_weighted_stack", crit, grid_workspace, grid_workspace_bytes, nref_total, src_points, elem, src_offsets_host,
                       num_pairs, ref_normals, normals_elem, src_normals, src_normals_elem, T0, out_transforms, out_fitness, out_rmse,
                       out_iterations, out_converged, out_status, out_correspondences, workspace, workspace_bytes, stream);
}

// ---- the same text on host memory, one pair, no GPU (tests/test_icp_cpu.py, tests/test_icp_robust_cpu.py) --------------------------------------
// icp_host_run is the body of se3_debug_icp_host and se3_debug_icp_weighted_host (`what` words the errors); crit is checked.
// trace: NULL, or (max_iteration + 1, n) int64: row k receives evaluation k's correspondence of every source row (-1 for none); the rows
// of evaluations that were not made are left as they are.
namespace {

int icp_host_run(const char* what, const IcpCriteria& crit, const void* src_points, int64_t n, const void* ref_points, int64_t nref, int elem,
                 const void* ref_normals, int normals_elem, const void* src_normals, int src_normals_elem, const double* T0,
                 double max_correspondence_distance, double* out_transform, double* out_fitness, double* out_rmse, int* out_iterations,
                 int* out_converged, int* out_status, int64_t* out_correspondences, int64_t* trace, const IcpColorCall* colors = nullptr) {
  SE3_REQUIRE(src_points && ref_points && T0, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(out_transform && out_fitness && out_rmse && out_iterations && out_converged && out_status, SE3_ERR_INVALID_ARG,
              "%s: null result pointer", what);
  SE3_REQUIRE(n >= 0 && n < (1ll << 31) && nref >= 0 && nref < (1ll << 31) && (elem == 0 || elem == 1) && (normals_elem == 0 || normals_elem == 1) &&
                  (src_normals_elem == 0 || src_normals_elem == 1),
              SE3_ERR_INVALID_ARG, "%s: n %lld, nref %lld, elem %d, normals_elem %d, src_normals_elem %d", what, (long long)n, (long long)nref,
              elem, normals_elem, src_normals_elem);
  SE3_REQUIRE(crit.mode == SE3_ICP_POINT_TO_POINT || ref_normals, SE3_ERR_INVALID_ARG, "%s: %s needs the reference normals", what,
              crit.mode == SE3_ICP_GENERALIZED ? "generalized" : "point-to-plane");
  SE3_REQUIRE(crit.mode != SE3_ICP_GENERALIZED || src_normals, SE3_ERR_INVALID_ARG, "%s: generalized needs the source normals", what);
  PairHostGrid H(ref_points, nref, elem, nullptr, max_correspondence_distance);
  const PairGridLayout& G = H.G;
  std::vector<int> nn_idx((size_t)n + 1);
  std::vector<double> nn_d2((size_t)n + 1), sh((size_t)kIcpGeneralSums * kIcpLanes);
  int done = 0;
  IcpCall c;
  c.rows = pg_single_rows(n);
  c.src = src_points, c.elem = elem, c.ref = G.moved, c.normals = ref_normals, c.normals_elem = normals_elem;
  c.src_normals = crit.mode == SE3_ICP_GENERALIZED ? src_normals : nullptr, c.src_normals_elem = src_normals_elem;
  c.ws.nn_idx = nn_idx.data(), c.ws.nn_d2 = nn_d2.data(), c.ws.done = &done;
  c.T = out_transform, c.fitness = out_fitness, c.rmse = out_rmse, c.iterations = out_iterations, c.converged = out_converged;
  c.status = out_status, c.corr = out_correspondences;
  const IcpPair v = icp_pair_of(c, G.meta, 0);
  const PairGridView g = G.view();
  IcpColors col{};
  if (colors) {
    col = icp_colors_of(*colors, c, G.meta, 0);
    icp_colored_pair_init(v, col, T0, 0, kIcpLanes, sh.data(), [] {});
  } else {
    icp_pair_init(v, T0, crit.mode, 0, kIcpLanes, sh.data(), [] {});
  }
  for (int k = 0; k <= crit.max_iteration && !done; k++) {
    for (int64_t i = 0; i < n; i++) {
      double qv[3];
      icp_moved(v, v.T, i, qv);
      pg_nearest(g, 0, qv, 0, 1, [](double*, int*) {}, &nn_d2[(size_t)i], &nn_idx[(size_t)i]);
      if (trace) trace[(int64_t)k * n + i] = nn_d2[(size_t)i] < crit.r2 ? nn_idx[(size_t)i] : -1;
    }
    if (!colors) icp_host_step(v, crit, k, sh.data());
    else if (crit.loss != SE3_ICP_LOSS_NONE) icp_colored_pair_step<true>(v, col, crit, k, 0, kIcpLanes, sh.data(), [] {});
    else icp_colored_pair_step<false>(v, col, crit, k, 0, kIcpLanes, sh.data(), [] {});
  }
  return SE3_OK;
}

}  // namespace

extern "C" int se3_debug_icp_host(const void* src_points, int64_t n, const void* ref_points, int64_t nref, int elem, const void* ref_normals,
                                  int normals_elem, const double* T0, double max_correspondence_distance, int mode, double relative_fitness,
                                  double relative_rmse, int max_iteration, double* out_transform, double* out_fitness, double* out_rmse,
                                  int* out_iterations, int* out_converged, int* out_status, int64_t* out_correspondences, int64_t* trace) {
  IcpCriteria crit;
  SE3_REQUIRE(mode != SE3_ICP_GENERALIZED && icp_criteria(&crit, max_correspondence_distance, mode, relative_fitness, relative_rmse, max_iteration),
              SE3_ERR_INVALID_ARG, "debug_icp_host: distance %g, mode %d, criteria %g %g %d (at most %d iterations)", max_correspondence_distance,
              mode, relative_fitness, relative_rmse, max_iteration, SE3_ICP_MAX_ITERATION);
  return icp_host_run("debug_icp_host", crit, src_points, n, ref_points, nref, elem, ref_normals, normals_elem, nullptr, 0, T0,
                      max_correspondence_distance, out_transform, out_fitness, out_rmse, out_iterations, out_converged, out_status,
                      out_correspondences, trace);
}

// the weighted entry on host memory: se3_icp_weighted_stack's text for one pair, with se3_debug_icp_host's trace
extern "C" int se3_debug_icp_weighted_host(const void* src_points, int64_t n, const void* ref_points, int64_t nref, int elem,
                                           const void* ref_normals, int normals_elem, const void* src_normals, int src_normals_elem,
                                           const double* T0, double max_correspondence_distance, int mode, int loss, double loss_k,
                                           double gicp_epsilon, double relative_fitness, double relative_rmse, int max_iteration,
                                           double* out_transform, double* out_fitness, double* out_rmse, int* out_iterations, int* out_converged,
                                           int* out_status, int64_t* out_correspondences, int64_t* trace) {
  IcpCriteria crit;
  SE3_REQUIRE(icp_criteria(&crit, max_correspondence_distance, mode, relative_fitness, relative_rmse, max_iteration), SE3_ERR_INVALID_ARG,
              "debug_icp_weighted_host: distance %g, mode %d, criteria %g %g %d (at most %d iterations)", max_correspondence_distance, mode,
              relative_fitness, relative_rmse, max_iteration, SE3_ICP_MAX_ITERATION);
  SE3_REQUIRE(icp_loss_criteria(&crit, loss, loss_k, gicp_epsilon), SE3_ERR_INVALID_ARG,
              "debug_icp_weighted_host: loss %d, loss_k %g (positive and finite), gicp_epsilon %g (in (0, 1])", loss, loss_k, gicp_epsilon);
  return icp_host_run("debug_icp_weighted_host", crit, src_points, n, ref_points, nref, elem, ref_normals, normals_elem, src_normals,
                      src_normals_elem, T0, max_correspondence_distance, out_transform, out_fitness, out_rmse, out_iterations, out_converged,
                      out_status, out_correspondences, trace);
}

// ---- coloured ICP: the entries (the contract is in the header comment) ---------------------------------------------------------------------------
namespace {

// the criteria and the colour call of the coloured entries (`what` words the errors)
int icp_colored_args(const char* what, IcpCriteria* crit, IcpColorCall* cc, const void* ref_normals, const void* src_colors, int src_colors_elem,
                     const void* ref_colors, int ref_colors_elem, const double* ref_gradients, double max_correspondence_distance,
                     double lambda_geometric, int loss, double loss_k, double relative_fitness, double relative_rmse, int max_iteration) {
  SE3_REQUIRE(icp_criteria(crit, max_correspondence_distance, SE3_ICP_POINT_TO_PLANE, relative_fitness, relative_rmse, max_iteration),
              SE3_ERR_INVALID_ARG, "%s: distance %g, criteria %g %g %d (at most %d iterations)", what, max_correspondence_distance, relative_fitness,
              relative_rmse, max_iteration, SE3_ICP_MAX_ITERATION);
  SE3_REQUIRE(icp_loss_criteria(crit, loss, loss_k, 1.0), SE3_ERR_INVALID_ARG, "%s: loss %d, loss_k %g (positive and finite)", what, loss, loss_k);
  SE3_REQUIRE(lambda_geometric >= 0.0 && lambda_geometric <= 1.0, SE3_ERR_INVALID_ARG, "%s: lambda_geometric %g is not in [0, 1]", what,
              lambda_geometric);
  SE3_REQUIRE(ref_normals && src_colors && ref_colors && ref_gradients, SE3_ERR_INVALID_ARG,
              "%s: coloured ICP needs the reference normals, the colours of both clouds and the reference gradients", what);
  SE3_REQUIRE((src_colors_elem == 0 || src_colors_elem == 1) && (ref_colors_elem == 0 || ref_colors_elem == 1), SE3_ERR_INVALID_ARG,
              "%s: src_colors_elem %d, ref_colors_elem %d", what, src_colors_elem, ref_colors_elem);
  crit->mode = SE3_ICP_COLORED;
  cc->src_colors = src_colors, cc->src_colors_elem = src_colors_elem, cc->ref_colors = ref_colors, cc->ref_colors_elem = ref_colors_elem;
  cc->gradients = ref_gradients, cc->a = pg_sqrt(lambda_geometric), cc->b = pg_sqrt(1.0 - lambda_geometric);
  return SE3_OK;
}

}  // namespace

extern "C" size_t se3_icp_colored_workspace_bytes(int64_t nsrc_total, int num_pairs) { return se3_icp_workspace_bytes(nsrc_total, num_pairs); }

extern "C" int se3_icp_colored_stack(const void* grid_workspace, size_t grid_workspace_bytes, int64_t nref_total, const void* src_points, int elem,
                                     const int64_t* src_offsets_host, int num_pairs, const void* ref_normals, int normals_elem,
                                     const void* src_colors, int src_colors_elem, const void* ref_colors, int ref_colors_elem,
                                     const double* ref_gradients, const double* T0, double max_correspondence_distance, double lambda_geometric,
                                     int loss, double loss_k, double relative_fitness, double relative_rmse, int max_iteration,
                                     double* out_transforms, double* out_fitness, double* out_rmse, int* out_iterations, int* out_converged,
                                     int* out_status, int64_t* out_correspondences, void* workspace, size_t workspace_bytes, void* stream) {
  IcpCriteria crit;
  IcpColorCall cc;
  if (const int rc = icp_colored_args("icp_colored_stack", &crit, &cc, ref_normals, src_colors, src_colors_elem, ref_colors, ref_colors_elem,
                                      ref_gradients, max_correspondence_distance, lambda_geometric, loss, loss_k, relative_fitness, relative_rmse,
                                      max_iteration))
    return rc;
  return icp_stack_run("icp_colored_stack", crit, grid_workspace, grid_workspace_bytes, nref_total, src_points, elem, src_offsets_host, num_pairs,
                       ref_normals, normals_elem, nullptr, 0, T0, out_transforms, out_fitness, out_rmse, out_iterations, out_converged, out_status,
                       out_correspondences, workspace, workspace_bytes, stream, &cc);
}

// the coloured entry on host memory: se3_icp_colored_stack's text for one pair, with se3_debug_icp_host's trace
extern "C" int se3_debug_icp_colored_host(const void* src_points, int64_t n, const void* ref_points, int64_t nref, int elem, const void* ref_normals,
                                          int normals_elem, const void* src_colors, int src_colors_elem, const void* ref_colors,
                                          int ref_colors_elem, const double* ref_gradients, const double* T0, double max_correspondence_distance,
                                          double lambda_geometric, int loss, double loss_k, double relative_fitness, double relative_rmse,
                                          int max_iteration, double* out_transform, double* out_fitness, double* out_rmse, int* out_iterations,
                                          int* out_converged, int* out_status, int64_t* out_correspondences, int64_t* trace) {
  IcpCriteria crit;
  IcpColorCall cc;
  if (const int rc = icp_colored_args("debug_icp_colored_host", &crit, &cc, ref_normals, src_colors, src_colors_elem, ref_colors, ref_colors_elem,
                                      ref_gradients, max_correspondence_distance, lambda_geometric, loss, loss_k, relative_fitness, relative_rmse,
                                      max_iteration))
    return rc;
  return icp_host_run("debug_icp_colored_host", crit, src_points, n, ref_points, nref, elem, ref_normals, normals_elem, nullptr, 0, T0,
                      max_correspondence_distance, out_transform, out_fitness, out_rmse, out_iterations, out_converged, out_status,
                      out_correspondences, trace, &cc);
}

extern "C" int se3_debug_icp_sincos_host(const double* x, int64_t n, double* out_sin, double* out_cos) {
  SE3_REQUIRE(x && out_sin && out_cos && n >= 0, SE3_ERR_INVALID_ARG, "debug_icp_sincos_host: null pointer or n %lld", (long long)n);
  for (int64_t i = 0; i < n; i++) {
    SE3_REQUIRE(fabs(x[i]) < kIcpMaxAngle, SE3_ERR_INVALID_ARG, "debug_icp_sincos_host: %g is outside (-1, 1)", x[i]);
    out_sin[i] = icp_sin(x[i]), out_cos[i] = icp_cos(x[i]);
  }
  return SE3_OK;
}
