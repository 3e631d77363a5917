// ISS keypoints of stacked clouds (Open3D's compute_iss_keypoints: intrinsic shape signatures, the eigenvalue ratios of a point's
// neighbourhood scatter matrix and a radius non-maximum test on the smallest eigenvalue), for up to SE3_PAIR_MAX_PAIRS clouds per call.
// se3et_amd/iss.py carries the same contract; the searches are the tested ones of csrc/pair_geometry.hip (ball query: count, scan, fill)
// and csrc/pair_grid.h (pg_ball_walk), the scatter matrix and the Jacobi solver those of csrc/cov3.h, shared with csrc/knn_normals.hip.
// (SE3_EXACT_FP: the file is built with contraction off, and every contract function of cov3.h and iss_core.h fences itself as well.)
//
//   iss_saliency_kernel   one wave per row over the row's ball list (rows sorted by index): the lanes fetch 64 members at a time, every lane
//                         then forms the same sequential sums in list order from the lanes' values (kn_covariance, as knn_normals_kernel);
//                         the eigenvalues and the saliency tests run in registers; lane 0 writes s_i.
//   iss_select_kernel     one thread per row, no list: rows with s_i = 0 write 0; the others walk the grid at non_max_radius
//                         (pg_ball_walk) for the member count and for a member with a larger saliency, and write one mask byte.
//
// Contract.  The structure is Open3D's ComputeISSKeypoints (geometry/keypoint/Keypoint.cpp); the arithmetic is the project's: float64,
// contraction off, float32 points promoted on load, no libm call other than the square root (pg_sqrt) and division.
//   Neighbourhood.  The members of a ball of radius r around row i are the points of the same cloud with d^2 < r r, d^2 = (dx dx + dy dy)
//     + dz dz unfused (pg_dist2), r r formed in float64; the test is strict.  The row itself is a member, a duplicate is a member.  m_i is
//     the member count at salient_radius, c_i the member count at non_max_radius.
//   Scatter matrix.  Over the m_i members in ascending cloud-local index: mean = (sequential sum) / m_i; the six entries of
//     C_i = sum (p - mean)(p - mean)^T / m_i are each a sequential sum in the same order (kn_covariance: two passes).
//   Eigenvalues.  Those of C_i by the cyclic Jacobi of csrc/cov3.h (kn_rotate, kJacobiSweeps sweeps over (0,1), (0,2), (1,2)), sorted
//     l1 >= l2 >= l3.
//   Saliency.  s_i = l3 when m_i >= min_neighbors, C_i is not the zero matrix, l2 / l1 < gamma_21, l3 / l2 < gamma_32 and l3 > 0 (true
//     divisions; a comparison with NaN is false); otherwise s_i = 0.
//   Selection.  Row i is a keypoint iff s_i > 0, c_i >= min_neighbors, and no member j of its non_max_radius ball has s_j > s_i.  Exactly
//     equal saliencies keep both rows (Open3D's IsLocalMaxima).  The output is the keypoints' cloud-local indices, ascending, int64.
//   Default radii.  A radius of 0 takes Open3D's default: salient_radius = 6 res, non_max_radius = 4 res, res the cloud's model resolution:
//     (the sum over its rows of pg_sqrt of the second column of a 2-nearest search) / n, summed in the fixed shape of csrc/fixed_sum.h
//     (csrc/outliers.hip); n < 2 gives 0.  The radii reach the kernels as host doubles, one per cloud (PairRadii): a batch whose clouds
//     default differently runs stacked like any other.
//   Refusals.  A non-finite point raises bit 1 of its cloud's status word (se3_fpfh_check_stack on the points).  A list entry outside its
//     cloud, or row offsets outside the list, are not read through: the row's saliency is 0.  n = 0 gives an empty output.
//   Determinism.  No float atomics.  A cloud's saliencies and keypoints are bit-identical alone, anywhere in a batch, from run to run, and
//     between the device and se3_debug_iss_host.
//   Cost.  The saliency pass is linear in the list: a salient radius far above the point spacing makes lists long (a ball that holds the
//     cloud is quadratic), and every lane of a row's wave walks its list serially, as the fixed order demands.
#include <math.h>

#include <vector>

#include "common.h"
#include "iss_core.h"

namespace {

constexpr int kIssWaves = 4;            // rows per workgroup of the saliency kernel
constexpr int kIssThreads = 256;        // rows per workgroup of the selection kernel

// what the saliency kernel gets: the stacked points of a call and the row slice [row_begin, row_begin + row_count) the list covers
struct IssCall {
  const void* points;
  int elem;
  PairRows rows;
  int64_t row_begin, row_count;
  const int64_t* row_offsets;          // (row_count + 1): slice row r owns list entries [row_offsets[r], row_offsets[r + 1])
  const int64_t* pairs;                // (total, 2): (i, j), j the member's cloud-local index, ascending within a row; only j is read
  int64_t total;
};

__global__ __launch_bounds__(kIssWaves* SE3_WAVE) void iss_saliency_kernel(IssCall c, double gamma_21, double gamma_32, int min_neighbors,
                                                                           double* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * kIssWaves + (threadIdx.x >> 6);
  if (r >= c.row_count) return;                            // (uniform over the wave)
  const int lane = se3_lane();
  const int64_t row = c.row_begin + r;
  const int cl = pg_pair_of_row(c.rows, row);
  const int64_t s0 = c.rows.start[cl], n = c.rows.start[cl + 1] - s0;
  int64_t b = c.row_offsets[r], e = c.row_offsets[r + 1];
  bool bad = b < 0 || e < b || e > c.total || e - b > n;
  if (bad) b = 0, e = 0;
  const int m = (int)(e - b);                              // (e - b <= n < 2^31)
  // point(t): at the start of every tile of 64 the lanes fetch members t .. t + 63 side by side; then lane t & 63 hands its point to all
  double mine[3] = {0.0, 0.0, 0.0};
  const auto point = [&](int t, double* pt) {
    if ((t & (SE3_WAVE - 1)) == 0) {                       // (uniform over the wave)
      const int64_t u = b + t + lane;
      const int64_t j = u < e ? c.pairs[2 * u + 1] : 0;
      const bool inside = j >= 0 && j < n;
      mine[0] = mine[1] = mine[2] = 0.0;
      if (u < e && inside) pg_load3(c.points, c.elem, s0 + j, mine);
      bad = bad || __ballot(u < e && !inside) != 0ull;
    }
    const int src = t & (SE3_WAVE - 1);
    pt[0] = __shfl(mine[0], src), pt[1] = __shfl(mine[1], src), pt[2] = __shfl(mine[2], src);
  };
  double C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (m > 0) kn_covariance(m, point, C);
  const double s = bad ? 0.0 : iss_saliency(m, C, gamma_21, gamma_32, min_neighbors);
  if (lane == 0) out[row] = s;
}

__global__ __launch_bounds__(kIssThreads) void iss_select_kernel(PairGridView g, const void* __restrict__ q, int elem, PairRows rows,
                                                                 int64_t n_total, PairRadii radii, const double* __restrict__ saliency,
                                                                 int min_neighbors, unsigned char* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * kIssThreads + threadIdx.x;
  if (i >= n_total) return;
  const int p = pg_pair_of_row(rows, i);
  double qv[3];
  pg_load3(q, elem, i, qv);
  const double r = radii.r[p];
  mask[i] = iss_is_keypoint(g, p, qv, r, r * r, saliency + rows.start[p], saliency[i], min_neighbors) ? 1 : 0;
}

bool iss_params_ok(double gamma_21, double gamma_32, int min_neighbors) {
  return isfinite(gamma_21) && gamma_21 > 0.0 && isfinite(gamma_32) && gamma_32 > 0.0 && min_neighbors >= 1;
}

}  // namespace

extern "C" int se3_iss_saliency_stack(const void* points, int elem, const int64_t* offsets_host, int num_clouds, int64_t row_begin,
                                      int64_t row_count, const int64_t* row_offsets, const int64_t* pairs, int64_t total, double gamma_21,
                                      double gamma_32, int min_neighbors, double* out_saliency, void* stream) {
  SE3_REQUIRE(points && offsets_host && row_offsets && (pairs || total == 0) && out_saliency, SE3_ERR_INVALID_ARG,
              "iss_saliency_stack: null pointer");
  SE3_REQUIRE(num_clouds >= 0 && num_clouds <= kPairMaxPairs && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG,
              "iss_saliency_stack: %d clouds (at most %d), elem %d", num_clouds, kPairMaxPairs, elem);
  SE3_REQUIRE(iss_params_ok(gamma_21, gamma_32, min_neighbors), SE3_ERR_INVALID_ARG,
              "iss_saliency_stack: gamma_21 %g, gamma_32 %g (positive and finite), min_neighbors %d (at least 1)", gamma_21, gamma_32, min_neighbors);
  IssCall c;
  SE3_REQUIRE(pg_fill_rows(&c.rows, offsets_host, num_clouds), SE3_ERR_INVALID_ARG, "iss_saliency_stack: offsets must start at 0 and not decrease");
  const int64_t n_total = c.rows.start[num_clouds];
  SE3_REQUIRE(n_total < (1ll << 31), SE3_ERR_UNSUPPORTED, "iss_saliency_stack: %lld rows in one call (below 2^31)", (long long)n_total);
  SE3_REQUIRE(row_begin >= 0 && row_count >= 0 && row_begin + row_count <= n_total && total >= 0, SE3_ERR_INVALID_ARG,
              "iss_saliency_stack: rows [%lld, %lld + %lld) of %lld, %lld list entries", (long long)row_begin, (long long)row_begin,
              (long long)row_count, (long long)n_total, (long long)total);
  if (row_count == 0) return SE3_OK;
  c.points = points, c.elem = elem, c.row_begin = row_begin, c.row_count = row_count, c.row_offsets = row_offsets, c.pairs = pairs, c.total = total;
  iss_saliency_kernel<<<(unsigned)se3_cdiv(row_count, kIssWaves), kIssWaves * SE3_WAVE, 0, (hipStream_t)stream>>>(c, gamma_21, gamma_32,
                                                                                                                min_neighbors, out_saliency);
  SE3_CHECK_LAUNCH("iss_saliency_stack");
  return SE3_OK;
}

extern "C" int se3_iss_select_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                                    const int64_t* q_offsets_host, int num_clouds, const double* radii_host, const double* saliency,
                                    int min_neighbors, uint8_t* out_mask, void* stream) {
  PairGridCall c;
  if (const int rc = pg_grid_call("iss_select_stack", "clouds", q_points && radii_host && saliency && out_mask, grid_workspace, workspace_bytes,
                                  ns_total, elem, q_offsets_host, num_clouds, 1ll << 31, &c))
    return rc;
  PairRadii radii;
  SE3_REQUIRE(pg_fill_radii(&radii, radii_host, 0.0, num_clouds) && min_neighbors >= 1, SE3_ERR_INVALID_ARG,
              "iss_select_stack: radius %g, min_neighbors %d", pg_bad_radius(radii), min_neighbors);
  SE3_REQUIRE(c.n_total == ns_total, SE3_ERR_INVALID_ARG, "iss_select_stack: the grid is built over the clouds themselves: %lld rows, %lld in it",
              (long long)c.n_total, (long long)ns_total);
  if (c.n_total == 0) return SE3_OK;
  iss_select_kernel<<<(unsigned)se3_cdiv(c.n_total, kIssThreads), kIssThreads, 0, (hipStream_t)stream>>>(
      c.G.view(), q_points, elem, c.rows, c.n_total, radii, saliency, min_neighbors, out_mask);
  SE3_CHECK_LAUNCH("iss_select_stack");
  return SE3_OK;
}

// ---- the same text on host memory, one cloud, no GPU (tests/test_iss_cpu.py) -------------------------------------------------------------------
// The members of every row come from pg_ball_fill (ascending index), the sums run in that order (kn_covariance), the selection walks the
// grid of non_max_radius (iss_is_keypoint).  out_saliency (n), out_mask (n); out_eigenvalues (n, 3: l1 l2 l3, zeros for a row without a
// member or with C = 0) and out_counts (n, 2: m_i, c_i) may be NULL.  *status: 0, or bit 1 for a non-finite point (nothing is computed).
extern "C" int se3_debug_iss_host(const void* points, int64_t n, int elem, double salient_radius, double non_max_radius, double gamma_21,
                                  double gamma_32, int min_neighbors, double* out_saliency, double* out_eigenvalues, int64_t* out_counts,
                                  uint8_t* out_mask, int* status) {
  SE3_REQUIRE(points && out_saliency && out_mask && status, SE3_ERR_INVALID_ARG, "debug_iss_host: null pointer");
  SE3_REQUIRE(n >= 0 && n < (1ll << 31) && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG, "debug_iss_host: n %lld, elem %d", (long long)n, elem);
  SE3_REQUIRE(pg_radius_ok(salient_radius) && pg_radius_ok(non_max_radius), SE3_ERR_INVALID_ARG, "debug_iss_host: radii %g, %g", salient_radius,
              non_max_radius);
  SE3_REQUIRE(iss_params_ok(gamma_21, gamma_32, min_neighbors), SE3_ERR_INVALID_ARG,
              "debug_iss_host: gamma_21 %g, gamma_32 %g (positive and finite), min_neighbors %d (at least 1)", gamma_21, gamma_32, min_neighbors);
  *status = 0;
  for (int64_t i = 0; i < n; i++) {
    double p[3];
    pg_load3(points, elem, i, p);
    if (!(fabs(p[0]) < INFINITY) || !(fabs(p[1]) < INFINITY) || !(fabs(p[2]) < INFINITY)) *status |= 1;
  }
  if (*status) return SE3_OK;
  {
    PairHostGrid H(points, n, elem, nullptr, salient_radius);
    const PairGridView g = H.G.view();
    const double r2 = salient_radius * salient_radius;
    std::vector<int64_t> list;
    for (int64_t i = 0; i < n; i++) {
      double qv[3];
      pg_load3(points, elem, i, qv);
      const int64_t m = pg_ball_count(g, 0, qv, salient_radius, r2);
      list.assign((size_t)(2 * m + 2), 0);
      pg_ball_fill(g, 0, qv, salient_radius, r2, i, list.data(), m);
      double C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (m > 0) kn_covariance((int)m, [&](int t, double* pt) { pg_load3(points, elem, list[(size_t)(2 * t + 1)], pt); }, C);
      out_saliency[i] = iss_saliency((int)m, C, gamma_21, gamma_32, min_neighbors);
      if (out_counts) out_counts[2 * i] = m;
      if (out_eigenvalues) {
        double l[3] = {0.0, 0.0, 0.0};
        if (m > 0 && !(C[0] == 0.0 && C[1] == 0.0 && C[2] == 0.0 && C[3] == 0.0 && C[4] == 0.0 && C[5] == 0.0)) kn_eigenvalues(C, l);
        for (int d = 0; d < 3; d++) out_eigenvalues[3 * i + d] = l[d];
      }
    }
  }
  PairHostGrid H(points, n, elem, nullptr, non_max_radius);
  const PairGridView g = H.G.view();
  const double r2 = non_max_radius * non_max_radius;
  for (int64_t i = 0; i < n; i++) {
    double qv[3];
    pg_load3(points, elem, i, qv);
    out_mask[i] = iss_is_keypoint(g, 0, qv, non_max_radius, r2, out_saliency, out_saliency[i], min_neighbors) ? 1 : 0;
    if (out_counts) out_counts[2 * i + 1] = pg_ball_count(g, 0, qv, non_max_radius, r2);
  }
  return SE3_OK;
}
