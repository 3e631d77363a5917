// Multiway registration on the device: the information matrix of stacked pairs and the global optimisation of stacked pose graphs --
// Open3D's get_information_matrix_from_point_clouds and global_optimization (GlobalOptimization.cpp: Levenberg-Marquardt with a line
// process, a pruning pass, a second optimisation) for up to SE3_PAIR_MAX_PAIRS pairs / graphs per call, nothing read back.
// csrc/pose_graph_core.h holds the text as __host__ __device__ functions, csrc/icp_core.h and csrc/fgr_core.h the ordered sum, the
// composition, the update matrix and its sine and cosine, csrc/pair_grid.h the search; se3et_amd/pose_graph.py carries the same contract.
// (SE3_EXACT_FP: the file is built with contraction off, and every contract function fences itself as well.)
//
//   pgo_info_nearest_kernel   one wave per stacked source row: the row moved by its pair's transform, the pair_grid.h nearest-neighbour walk.
//   pgo_info_sum_kernel       one workgroup of 256 threads per pair: the refusals and the 21 ordered sums.  LDS 21 x 256 x 8 = 42 KiB.
//   pgo_optimize_kernel       one workgroup of 256 threads per graph, ONE launch for the whole optimisation: both passes, every
//                             iteration and every trial, the pruning and the reference node.  H and its damped, factorised copy live in
//                             the global workspace (2 x (6 N)^2 doubles: 2.4 MB at 64 nodes), the per-edge vectors, W and g beside them;
//                             LDS holds two sum columns, the current Cholesky panel (row j of L) and the solves' vector: 10 KiB.  No float
//                             atomics, no captured graphs; every branch on a graph's state is uniform over its workgroup.
//
// Contract, part A: the information matrix of a pair.  Source S, reference R and T with ref ~ T src, as in icp.hip.  Source row i has a
//   correspondence iff its moved point (pg_transform) has a nearest reference point with d^2 < r^2: ICP's evaluation rule, strict, the same
//   arithmetic, the same pg_nearest.  With q = (x, y, z) the REFERENCE point of the correspondence:
//     G = [[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]],   Lambda = sum G^T G
//   over the correspondences; a row's term of entry (a, b) is (G0a G0b + G1a G1b) + G2a G2b; the 21 distinct entries are each taken in the
//   order of icp_sum over the source rows, a row without a correspondence adding +0.  Lambda[5][5] is the correspondence count.  A
//   non-finite coordinate or transform gives a NaN matrix and SE3_PGO_NONFINITE; an empty cloud gives the zero matrix and SE3_PGO_EMPTY.
//   A pair's Lambda is bit-identical alone or anywhere in a batch.
//
// Contract, part B: one pose graph.  N nodes with poses X_i (node frame -> common frame); E edges (s, t, T, Lambda, uncertain), T mapping
//   node s's cloud into node t's frame: a consistent graph has X_s = X_t T.  Everything is float64 with contraction off; every square
//   root is pg_sqrt; every 4x4 product is icp_compose ((a b + c d) + e f per entry, the translation added last).
//   0. Refusals, tested in this order, only the first one set: a non-finite pose, T, Lambda or option: SE3_PGO_NONFINITE, NaN poses;
//      N = 0: SE3_PGO_EMPTY, no pose written; an edge index outside [0, N) or s = t: SE3_PGO_BAD_INDEX, NaN poses.  More nodes or edges
//      than the limits is SE3_ERR_INVALID_ARG for the call.  E = 0 is no refusal: the right-term test stops each pass at once.
//   1. Residual of an edge.  M = (T^-1 X_t^-1) X_s with the rigid inverses in closed form (R^T, -R^T t).  e = vec6(M): with
//      sy = sqrt(M00^2 + M10^2); unless sy < 1e-6: alpha = atan2(M21, M22), beta = atan2(-M20, sy), gamma = atan2(M10, M00); otherwise
//      alpha = atan2(-M12, M11), beta = atan2(-M20, sy), gamma = 0; e = (alpha, beta, gamma, M03, M13, M23).  atan2 is pgo_atan2, one text
//      for host and device (its header comment has the reduction and the exact cases).
//   2. Jacobians.  D_0 .. D_5 the generators (D_0: [1][2] = -1, [2][1] = 1; D_1: [2][0] = -1, [0][2] = 1; D_2: [0][1] = -1, [1][0] = 1;
//      D_3 .. D_5: a single 1 at [0 .. 2][3]).  With A = T^-1 X_t^-1, column i of J_s is lin6(A (D_i X_s)),
//      lin6(M) = ((M21 - M12) / 2, (M02 - M20) / 2, (M10 - M01) / 2, M03, M13, M23); J_t = -J_s.
//   3. Line process.  mu = (preference_loop_closure max_correspondence_distance^2) (mean of Lambda[5][5] over the pass's edges: the
//      icp_sum over the edge index, divided by their number; 0 without an edge).  l = 1 for a certain edge, (mu / (mu + e^T L e))^2 for an
//      uncertain one, e^T L e = sum_a e_a (sum_b L_ab e_b), ascending.
//   4. Residual of the graph.  F = sum over the edges of l e^T L e + (uncertain ? mu (sqrt(l) - 1)^2 : 0), in the order of icp_sum.
//   5. Linear system.  Per edge W = l (J_s^T (Lambda J_s)) and g = l (J_s^T (Lambda e)), every inner sum ascending from zero; the edge
//      adds W to the diagonal blocks of s and of t, -W to the two off-diagonal blocks, g to b_s and -g to b_t (J_t = -J_s: a negation is
//      exact).  Only the lower triangle of H is formed and read.  Every entry of H and b is the sum of its edges' terms in ascending
//      edge index from zero; duplicate edges each add.  (H + lambda I) delta = -b by the Cholesky factorisation
//      L_ij = (a_ij - sum_{k<j} L_ik L_jk) / L_jj, the k-sum in ascending k, each product and subtraction rounded on its own; the forward
//      solve subtracts in ascending k, the backward solve in descending k.  A pivot that is not > 0 (or not finite) sets SE3_PGO_SINGULAR
//      and ends the pass at the poses it had (stop reason REFUSED).
//   6. Loop of one pass (pgo_pass; Open3D's defaults: 100, 20, 1e-6, 1e-6, 1e-6, 1e-6, 2/3, 1/3):
//        e <- residuals; l <- line process; F <- step 4; H, b <- step 5
//        lambda <- 1e-5 max |diag H|; nu <- 2; stop <- max_k |b_k| < min_right_term
//        for it = 0; not stop; it++:
//          lm <- 0
//          do:
//            delta <- solve (H + lambda I) delta = -b
//            stop |= |delta| < min_relative_increment (|x| + min_relative_increment)      x = vec6 of all poses; ordered sums of squares
//            rho <- 0
//            if not stop:
//              X'_i <- U(delta_i) X_i        U = [Rz(d2) Ry(d1) Rx(d0) | d3 d4 d5]: icp_sincos_to_matrix with fgr_sincos; a non-finite
//                                            angle or |a| >= 4 sets SE3_PGO_STEP_REFUSED, the pass ends at X (stop reason REFUSED)
//              e' <- residuals of X'; F' <- step 4 with the CURRENT l
//              rho <- (F - F') / (sum_k delta_k (lambda delta_k - b_k) + 1e-3)
//              if rho > 0:
//                if F - F' < min_relative_residual_increment F: stop; break          (X' is NOT taken)
//                c = 2 rho - 1; lambda <- lambda max(lower, min(1 - c c c, upper)); nu <- 2
//                F <- F'; e <- e'; X <- X'; l <- step 3; H, b <- step 5
//                if max |b| < min_right_term: stop; break
//              else: lambda <- lambda nu; nu <- 2 nu
//            lm++; stop |= lm >= max_iteration_lm
//          while not (rho > 0 or stop)
//          stop |= F < min_residual or it + 1 >= max_iteration
//      The stop reason is the first test that fired; iterations = the outer bodies run, trials = the solves.
//   7. Whole optimisation.  Pass 1 on all edges; kept = certain, or l > edge_prune_threshold (0.25); pass 2 on the kept edges, in their
//      order, from pass 1's poses, with mu over the kept edges; with a reference node every pose is left-multiplied by
//      X_ref(input) X_ref(output)^-1 and the node itself gets its input pose, exactly.  A pruned edge keeps its pass-1 confidence; its
//      pass-2 slot is 0.
//   A graph's result is bit-identical from run to run, alone or anywhere in a batch, and between the device and se3_debug_pose_graph_host.
//   Differences from Open3D: the arc tangent and the sine and cosine (own series); |b| in the right-term test; the line process applied
//   before the first residual; the summation orders; the dense Cholesky in place of Eigen's solver; the refusals.
#include <math.h>

#include <vector>

#include "common.h"
#include "pose_graph_core.h"   // (and through it fgr_core.h, icp_core.h, pair_grid.h)

namespace {

constexpr int kPgoNnWaves = 4;          // source rows per nearest-neighbour workgroup

// ---- the information matrix ------------------------------------------------------------------------------------------------------------------
struct PgoInfoLayout {
  int* nn_idx;
  double* nn_d2;
};

size_t pgo_info_carve(int64_t nsrc_total, char* base, PgoInfoLayout* L) {
  Se3Carver c(base);
  PgoInfoLayout l;
  l.nn_idx = c.take<int>((size_t)(nsrc_total > 0 ? nsrc_total : 1));
  l.nn_d2 = c.take<double>((size_t)(nsrc_total > 0 ? nsrc_total : 1));
  if (L) *L = l;
  return c.bytes();
}

__global__ __launch_bounds__(kPgoNnWaves* SE3_WAVE) void pgo_info_nearest_kernel(PairGridView g, const void* __restrict__ src, int elem,
                                                                                 PairRows rows, const double* __restrict__ transforms,
                                                                                 PgoInfoLayout ws, int64_t n_total) {
  const int64_t i = (int64_t)blockIdx.x * kPgoNnWaves + (threadIdx.x >> 6);
  if (i >= n_total) return;                                // (uniform over the wave)
  const int p = pg_pair_of_row(rows, i);
  double T[12], qv[3];
  for (int k = 0; k < 12; k++) T[k] = transforms[16 * p + k];
  pg_transform_row(T, src, elem, i, qv);
  double d2;
  int j;
  pg_wave_nearest(g, p, qv, &d2, &j);
  if (se3_lane() == 0) {
    ws.nn_idx[i] = j;
    ws.nn_d2[i] = d2;
  }
}

__global__ __launch_bounds__(kPgoLanes) void pgo_info_sum_kernel(const PairGridMeta* __restrict__ meta, const double* __restrict__ moved,
                                                                 const void* __restrict__ src, int elem, PairRows rows,
                                                                 const double* __restrict__ transforms, PgoInfoLayout ws, double r2,
                                                                 double* __restrict__ out, double* __restrict__ count,
                                                                 int* __restrict__ status) {
  __shared__ double sh[kIcpMaxSums * kPgoLanes];
  const int p = blockIdx.x;
  const int64_t s0 = rows.start[p], n = rows.start[p + 1] - s0;
  const void* s = elem ? (const void*)((const double*)src + 3 * s0) : (const void*)((const float*)src + 3 * s0);
  pgo_information(s, elem, n, moved + 3 * meta[p].s_start, meta[p].ns, transforms + 16 * p, ws.nn_idx + s0, ws.nn_d2 + s0, r2, out + 36 * p,
                  count + p, status + p, threadIdx.x, threadIdx.x + 1, sh, [] { __syncthreads(); });
}

// ---- the pose graphs -------------------------------------------------------------------------------------------------------------------------
// what the kernel gets: the stacked arrays of a call
struct PgoCall {
  const double* poses;
  PairRows nodes;
  const int64_t* edges;
  const double* T;
  const double* info;
  const uint8_t* uncertain;
  PairRows edge_rows;
  int reference[kPairMaxPairs];
  int64_t scratch[kPairMaxPairs];       // byte offset of every graph's scratch in the workspace
  char* workspace;
  double* out_poses;
  double* out_conf;                     // (2, E_total)
  uint8_t* out_kept;
  int* out_status;
  int* out_info;
  double* out_residuals;
};

__host__ __device__ PgoGraph pgo_graph_of(const PgoCall& c, int g) {
  PgoGraph v;
  const int64_t n0 = c.nodes.start[g], e0 = c.edge_rows.start[g], e_total = c.edge_rows.start[c.edge_rows.n];
  v.N = (int)(c.nodes.start[g + 1] - n0), v.E = (int)(c.edge_rows.start[g + 1] - e0), v.reference_node = c.reference[g];
  v.X0 = c.poses + 16 * n0, v.edges = c.edges + 2 * e0, v.T = c.T + 16 * e0, v.info = c.info + 36 * e0, v.uncertain = c.uncertain + e0;
  v.X = c.out_poses + 16 * n0, v.conf1 = c.out_conf + e0, v.conf2 = c.out_conf + e_total + e0, v.kept = c.out_kept + e0;
  v.status = c.out_status + g, v.out_info = c.out_info + 6 * g, v.residuals = c.out_residuals + 2 * g;
  v.trace = nullptr, v.trace_rows = 0, v.trace_count = nullptr;
  pgo_scratch(v.N, v.E, c.workspace + c.scratch[g], &v);
  return v;
}

__global__ __launch_bounds__(kPgoLanes) void pgo_optimize_kernel(PgoCall c, PgoOptions o) {
  __shared__ double sh[kPgoShDoubles];
  const PgoGraph v = pgo_graph_of(c, blockIdx.x);
  pgo_graph_optimize(v, o, threadIdx.x, threadIdx.x + 1, sh, [] { __syncthreads(); });
}

bool pgo_options(PgoOptions* o, int max_iteration, int max_iteration_lm, double min_relative_increment,
                 double min_relative_residual_increment, double min_right_term, double min_residual, double upper_scale_factor,
                 double lower_scale_factor, double max_correspondence_distance, double edge_prune_threshold, double preference_loop_closure) {
  if (max_iteration < 0 || max_iteration > SE3_PGO_MAX_ITERATION || max_iteration_lm < 0 || max_iteration_lm > SE3_PGO_MAX_ITERATION_LM) return false;
  o->max_iteration = max_iteration, o->max_iteration_lm = max_iteration_lm, o->min_relative_increment = min_relative_increment;
  o->min_relative_residual_increment = min_relative_residual_increment, o->min_right_term = min_right_term, o->min_residual = min_residual;
  o->upper_scale_factor = upper_scale_factor, o->lower_scale_factor = lower_scale_factor;
  o->max_correspondence_distance = max_correspondence_distance, o->edge_prune_threshold = edge_prune_threshold;
  o->preference_loop_closure = preference_loop_closure;
  return true;
}

}  // namespace

extern "C" size_t se3_pair_information_workspace_bytes(int64_t nsrc_total, int num_pairs) {
  if (nsrc_total < 0 || num_pairs < 0 || num_pairs > kPairMaxPairs) return 0;
  return pgo_info_carve(nsrc_total, nullptr, nullptr);
}

extern "C" int se3_pair_information_stack(const void* grid_workspace, size_t grid_workspace_bytes, int64_t nref_total, const void* src_points,
                                          int elem, const int64_t* src_offsets_host, int num_pairs, const double* transforms,
                                          double max_correspondence_distance, double* out_information, double* out_count, int* out_status,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "pair_information_stack";
  SE3_REQUIRE(grid_workspace && src_points && src_offsets_host && transforms && workspace, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(out_information && out_count && out_status, SE3_ERR_INVALID_ARG, "%s: null result pointer", what);
  SE3_REQUIRE(pg_radius_ok(max_correspondence_distance), SE3_ERR_INVALID_ARG, "%s: distance %g (finite, >= 0)", what, max_correspondence_distance);
  PairGridCall gc;
  if (const int rc = pg_grid_call(what, "pairs", true, grid_workspace, grid_workspace_bytes, nref_total, elem, src_offsets_host, num_pairs,
                                  1ll << 31, &gc))
    return rc;
  PgoInfoLayout L;
  SE3_REQUIRE(pgo_info_carve(gc.n_total, (char*)workspace, &L) <= workspace_bytes, SE3_ERR_WORKSPACE, "%s: workspace of %zu bytes is too small",
              what, workspace_bytes);
  if (num_pairs == 0) return SE3_OK;
  hipStream_t st = (hipStream_t)stream;
  const double r2 = max_correspondence_distance * max_correspondence_distance;
  if (gc.n_total > 0)
    pgo_info_nearest_kernel<<<(unsigned)se3_cdiv(gc.n_total, kPgoNnWaves), kPgoNnWaves * SE3_WAVE, 0, st>>>(gc.G.view(), src_points, elem, gc.rows,
                                                                                                          transforms, L, gc.n_total);
  pgo_info_sum_kernel<<<(unsigned)num_pairs, kPgoLanes, 0, st>>>(gc.G.meta, gc.G.moved, src_points, elem, gc.rows, transforms, L, r2,
                                                                 out_information, out_count, out_status);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" int se3_debug_pair_information_host(const void* src_points, int64_t n, const void* ref_points, int64_t nref, int elem,
                                               const double* transform, double max_correspondence_distance, double* out_information,
                                               double* out_count, int* out_status, int64_t* out_correspondences) {
  const char* what = "debug_pair_information_host";
  SE3_REQUIRE(src_points && ref_points && transform && out_information && out_count && out_status, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(n >= 0 && n < (1ll << 31) && nref >= 0 && nref < (1ll << 31) && (elem == 0 || elem == 1) && pg_radius_ok(max_correspondence_distance),
              SE3_ERR_INVALID_ARG, "%s: n %lld, nref %lld, elem %d, distance %g", what, (long long)n, (long long)nref, elem,
              max_correspondence_distance);
  PairHostGrid H(ref_points, nref, elem, nullptr, max_correspondence_distance);
  const PairGridView g = H.G.view();
  std::vector<int> nn_idx((size_t)n + 1);
  std::vector<double> nn_d2((size_t)n + 1), sh((size_t)kIcpMaxSums * kPgoLanes);
  const double r2 = max_correspondence_distance * max_correspondence_distance;
  for (int64_t i = 0; i < n; i++) {
    double qv[3];
    pg_transform_row(transform, src_points, elem, i, qv);
    pg_nearest(g, 0, qv, 0, 1, [](double*, int*) {}, &nn_d2[(size_t)i], &nn_idx[(size_t)i]);
    if (out_correspondences) out_correspondences[i] = nn_d2[(size_t)i] < r2 ? nn_idx[(size_t)i] : -1;
  }
  pgo_information(src_points, elem, n, H.G.moved, nref, transform, nn_idx.data(), nn_d2.data(), r2, out_information, out_count, out_status, 0,
                  kPgoLanes, sh.data(), [] {});
  return SE3_OK;
}

extern "C" size_t se3_pose_graph_workspace_bytes(const int64_t* node_offsets_host, const int64_t* edge_offsets_host, int num_graphs) {
  PairRows nodes, edge_rows;
  if (!node_offsets_host || !edge_offsets_host || num_graphs < 0 || num_graphs > kPairMaxPairs) return 0;
  if (!pg_fill_rows(&nodes, node_offsets_host, num_graphs) || !pg_fill_rows(&edge_rows, edge_offsets_host, num_graphs)) return 0;
  size_t bytes = 256;
  for (int g = 0; g < num_graphs; g++) {
    const int64_t N = nodes.start[g + 1] - nodes.start[g], E = edge_rows.start[g + 1] - edge_rows.start[g];
    if (N > SE3_PGO_MAX_NODES || E > SE3_PGO_MAX_EDGES) return 0;
    bytes += pgo_scratch((int)N, (int)E, nullptr, nullptr);
  }
  return bytes;
}

extern "C" int se3_pose_graph_optimize_stack(const double* poses, const int64_t* node_offsets_host, const int64_t* edges,
                                             const double* transforms, const double* informations, const uint8_t* uncertain,
                                             const int64_t* edge_offsets_host, int num_graphs, const int* reference_nodes_host,
                                             int max_iteration, int max_iteration_lm, double min_relative_increment,
                                             double min_relative_residual_increment, double min_right_term, double min_residual,
                                             double upper_scale_factor, double lower_scale_factor, double max_correspondence_distance,
                                             double edge_prune_threshold, double preference_loop_closure, double* out_poses,
                                             double* out_confidence, uint8_t* out_kept, int* out_status, int* out_info, double* out_residuals,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "pose_graph_optimize_stack";
  SE3_REQUIRE(poses && node_offsets_host && edges && transforms && informations && uncertain && edge_offsets_host && workspace,
              SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(out_poses && out_confidence && out_kept && out_status && out_info && out_residuals, SE3_ERR_INVALID_ARG,
              "%s: null result pointer", what);
  SE3_REQUIRE(num_graphs >= 0 && num_graphs <= kPairMaxPairs, SE3_ERR_INVALID_ARG, "%s: %d graphs (at most %d)", what, num_graphs, kPairMaxPairs);
  PgoOptions o;
  SE3_REQUIRE(pgo_options(&o, max_iteration, max_iteration_lm, min_relative_increment, min_relative_residual_increment, min_right_term,
                          min_residual, upper_scale_factor, lower_scale_factor, max_correspondence_distance, edge_prune_threshold,
                          preference_loop_closure),
              SE3_ERR_INVALID_ARG, "%s: max_iteration %d (0 .. %d), max_iteration_lm %d (0 .. %d)", what, max_iteration, SE3_PGO_MAX_ITERATION,
              max_iteration_lm, SE3_PGO_MAX_ITERATION_LM);
  PgoCall c;
  SE3_REQUIRE(pg_fill_rows(&c.nodes, node_offsets_host, num_graphs) && pg_fill_rows(&c.edge_rows, edge_offsets_host, num_graphs),
              SE3_ERR_INVALID_ARG, "%s: offsets must start at 0 and not decrease", what);
  size_t off = 0;
  for (int g = 0; g < kPairMaxPairs; g++) c.reference[g] = -1, c.scratch[g] = 0;
  for (int g = 0; g < num_graphs; g++) {
    const int64_t N = c.nodes.start[g + 1] - c.nodes.start[g], E = c.edge_rows.start[g + 1] - c.edge_rows.start[g];
    SE3_REQUIRE(N <= SE3_PGO_MAX_NODES && E <= SE3_PGO_MAX_EDGES, SE3_ERR_INVALID_ARG, "%s: graph %d has %lld nodes and %lld edges (at most %d, %d)",
                what, g, (long long)N, (long long)E, SE3_PGO_MAX_NODES, SE3_PGO_MAX_EDGES);
    const int ref = reference_nodes_host ? reference_nodes_host[g] : -1;
    SE3_REQUIRE(ref >= -1 && (ref < N || ref == -1), SE3_ERR_INVALID_ARG, "%s: graph %d: reference node %d of %lld nodes", what, g, ref,
                (long long)N);
    c.reference[g] = ref;
    c.scratch[g] = (int64_t)off;
    off += pgo_scratch((int)N, (int)E, nullptr, nullptr);
  }
  SE3_REQUIRE(off <= workspace_bytes, SE3_ERR_WORKSPACE, "%s: workspace of %zu bytes is too small (%zu needed)", what, workspace_bytes, off);
  if (num_graphs == 0) return SE3_OK;
  c.poses = poses, c.edges = edges, c.T = transforms, c.info = informations, c.uncertain = uncertain, c.workspace = (char*)workspace;
  c.out_poses = out_poses, c.out_conf = out_confidence, c.out_kept = out_kept, c.out_status = out_status, c.out_info = out_info;
  c.out_residuals = out_residuals;
  pgo_optimize_kernel<<<(unsigned)num_graphs, kPgoLanes, 0, (hipStream_t)stream>>>(c, o);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" int se3_debug_pose_graph_host(const double* poses, int64_t num_nodes, const int64_t* edges, const double* transforms,
                                         const double* informations, const uint8_t* uncertain, int64_t num_edges, int reference_node,
                                         int max_iteration, int max_iteration_lm, double min_relative_increment,
                                         double min_relative_residual_increment, double min_right_term, double min_residual,
                                         double upper_scale_factor, double lower_scale_factor, double max_correspondence_distance,
                                         double edge_prune_threshold, double preference_loop_closure, double* out_poses,
                                         double* out_confidence, uint8_t* out_kept, int* out_status, int* out_info, double* out_residuals,
                                         double* trace, int64_t trace_rows, int* out_trace_count) {
  const char* what = "debug_pose_graph_host";
  SE3_REQUIRE(poses && edges && transforms && informations && uncertain, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(out_poses && out_confidence && out_kept && out_status && out_info && out_residuals, SE3_ERR_INVALID_ARG,
              "%s: null result pointer", what);
  SE3_REQUIRE(num_nodes >= 0 && num_nodes <= SE3_PGO_MAX_NODES && num_edges >= 0 && num_edges <= SE3_PGO_MAX_EDGES, SE3_ERR_INVALID_ARG,
              "%s: %lld nodes and %lld edges (at most %d, %d)", what, (long long)num_nodes, (long long)num_edges, SE3_PGO_MAX_NODES,
              SE3_PGO_MAX_EDGES);
  SE3_REQUIRE(reference_node >= -1 && (reference_node < num_nodes || reference_node == -1), SE3_ERR_INVALID_ARG,
              "%s: reference node %d of %lld nodes", what, reference_node, (long long)num_nodes);
  SE3_REQUIRE((!trace || out_trace_count) && trace_rows >= 0, SE3_ERR_INVALID_ARG, "%s: a trace needs its count", what);
  PgoOptions o;
  SE3_REQUIRE(pgo_options(&o, max_iteration, max_iteration_lm, min_relative_increment, min_relative_residual_increment, min_right_term,
                          min_residual, upper_scale_factor, lower_scale_factor, max_correspondence_distance, edge_prune_threshold,
                          preference_loop_closure),
              SE3_ERR_INVALID_ARG, "%s: max_iteration %d (0 .. %d), max_iteration_lm %d (0 .. %d)", what, max_iteration, SE3_PGO_MAX_ITERATION,
              max_iteration_lm, SE3_PGO_MAX_ITERATION_LM);
  std::vector<char> mem(pgo_scratch((int)num_nodes, (int)num_edges, nullptr, nullptr) + 256);
  std::vector<double> sh(kPgoShDoubles);
  int counts[2] = {0, 0};
  PgoGraph v;
  v.N = (int)num_nodes, v.E = (int)num_edges, v.reference_node = reference_node;
  v.X0 = poses, v.edges = edges, v.T = transforms, v.info = informations, v.uncertain = uncertain;
  v.X = out_poses, v.conf1 = out_confidence, v.conf2 = out_confidence + num_edges, v.kept = out_kept;
  v.status = out_status, v.out_info = out_info, v.residuals = out_residuals;
  v.trace = trace, v.trace_rows = trace_rows, v.trace_count = counts;
  char* base = mem.data() + (256 - (uintptr_t)mem.data() % 256) % 256;
  pgo_scratch(v.N, v.E, base, &v);
  pgo_graph_optimize(v, o, 0, kPgoLanes, sh.data(), [] {});
  if (out_trace_count) out_trace_count[0] = counts[0], out_trace_count[1] = counts[1];
  return SE3_OK;
}

extern "C" int se3_debug_pgo_atan2_host(const double* y, const double* x, int64_t n, double* out) {
  SE3_REQUIRE(y && x && out && n >= 0, SE3_ERR_INVALID_ARG, "debug_pgo_atan2_host: null pointer or n %lld", (long long)n);
  for (int64_t i = 0; i < n; i++) out[i] = pgo_atan2(y[i], x[i]);
  return SE3_OK;
}
