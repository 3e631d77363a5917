// Outlier removal of stacked clouds (Open3D's remove_statistical_outlier; remove_radius_outlier is a composition of the ball count of
// csrc/pair_geometry.hip and has no kernel here) and the model resolution of the ISS detector, for up to SE3_PAIR_MAX_PAIRS clouds per call
// on the float64 grid of csrc/pair_grid.h.  se3et_amd/scan_prep.py carries the same contract.
// (SE3_EXACT_FP: the file is built with contraction off, and every contract function of outliers_core.h and fixed_sum.h fences itself.)
//
//   knn_distance_kernel   one wave per row: the exact k nearest (pg_knn, the wave's list of knn_kernel), lane t takes the root of entry t,
//                         every lane forms the same sequential sum in list order; nothing is written but a_i.
//   cloud_stats_kernel    one workgroup of 256 threads per cloud: the two sums in the fixed shape of fs_sum, then mean, std, thr, resolution.
//   outlier_mask_kernel   one thread per row: the mask byte.
//
// Contract.  Statistical filter, Open3D's RemoveStatisticalOutliers including its quirks; float64, contraction off, float32 points
// promoted on load.
//   Per-row mean distance.  m = min(nb_neighbors, n); the row's list is knn_clouds' (the m nearest INCLUDING the row itself at d = 0,
//     (d^2, index) ascending); a_i = (the sequential sum in list order of pg_sqrt(d2_t)) / m.
//   Cloud mean.  mean = (sum of a_i over the rows with a_i > 0) / n.
//   Standard deviation.  std = pg_sqrt((sum over the same rows of (a_i - mean)^2) / (n - 1)).
//   Threshold and test.  thr = mean + std_ratio std (the product rounded, then the sum).  A row is kept iff a_i > 0 and a_i < thr.
//   Summation.  Both cloud sums have the shape of csrc/fixed_sum.h: lane l of 256 adds its rows l, l + 256, .. in ascending order from 0.0
//     (a row with a_i <= 0 adds nothing), then sh[l] = sh[l] + sh[l + o] for o = 128, 64, .., 1; the sum is sh[0].
//   Small clouds.  n < 2 keeps nothing: n = 1 has a_0 = 0; the statistics of n = 0 and the std of n = 1 are NaN, as the formulas give.
//   Model resolution (se3et_amd/iss.py).  The same kernels with k = 2 and the row value pg_sqrt(d2 of column 1) (0 in a one-point cloud):
//     res = mean when n >= 2, else 0: the mean distance to the nearest other point.  (A duplicate's 0 adds nothing to either form.)
//   Determinism.  No float atomics: a cloud's values are bit-identical alone, anywhere in a batch, from run to run, and between the device
//     and the se3_debug_*_host entries.
#include <math.h>

#include <vector>

#include "common.h"
#include "outliers_core.h"

namespace {

constexpr int kOdWaves = 4;             // rows per workgroup of knn_distance_kernel
constexpr int kOdThreads = 256;         // rows per workgroup of outlier_mask_kernel
constexpr int64_t kOdMaxRows = 1ll << 31;
static_assert(kPairKnnMax == SE3_KNN_MAX, "pair_grid.h and include/se3et_hip.h name one limit");

__global__ __launch_bounds__(kOdWaves* SE3_WAVE) void knn_distance_kernel(PairGridView g, const void* __restrict__ q, int elem, PairRows rows,
                                                                          int64_t nq_total, int k, int column, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kOdWaves + (threadIdx.x >> 6);
  if (i >= nq_total) return;                               // (uniform over the wave)
  double qv[3];
  pg_load3(q, elem, i, qv);
  WaveKnnList list;
  list.init(k);
  pg_knn(g, pg_pair_of_row(rows, i), qv, se3_lane(), SE3_WAVE, list);
  const int cnt = __popcll(__ballot(se3_lane() < k && list.j != kPairKnnEmpty));
  const double mine = se3_lane() < cnt ? pg_sqrt(list.d2) : 0.0;
  const double a = od_row_distance(cnt, column, [&](int t) { return __shfl(mine, t); });
  if (se3_lane() == 0) out[i] = a;
}

__global__ __launch_bounds__(kFsLanes) void cloud_stats_kernel(const double* __restrict__ a, PairRows rows, double std_ratio,
                                                               double* __restrict__ out) {
  __shared__ double sh[kFsLanes];
  const int p = blockIdx.x, t = threadIdx.x;
  const int64_t s0 = rows.start[p], n = rows.start[p + 1] - s0;
  double stats[kOdStats];
  od_cloud_stats(a + s0, n, std_ratio, t, t + 1, sh, [] { __syncthreads(); }, stats);
  if (t < kOdStats) out[kOdStats * p + t] = stats[t];
}

__global__ __launch_bounds__(kOdThreads) void outlier_mask_kernel(const double* __restrict__ a, PairRows rows, int64_t n_total,
                                                                  const double* __restrict__ stats, unsigned char* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * kOdThreads + threadIdx.x;
  if (i >= n_total) return;
  mask[i] = od_kept(a[i], stats[kOdStats * pg_pair_of_row(rows, i) + 2]) ? 1 : 0;
}

}  // namespace

extern "C" int se3_knn_distance_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                                      const int64_t* q_offsets_host, int num_clouds, int k, int column, double* out, void* stream) {
  SE3_REQUIRE(k >= 1 && k <= kPairKnnMax && column < k, SE3_ERR_INVALID_ARG, "knn_distance_stack: k %d not in [1, %d], or column %d not below it", k,
              kPairKnnMax, column);
  PairGridCall c;
  if (const int rc = pg_grid_call("knn_distance_stack", "clouds", q_points && out, grid_workspace, workspace_bytes, ns_total, elem, q_offsets_host,
                                  num_clouds, kOdMaxRows, &c))
    return rc;
  if (c.n_total == 0) return SE3_OK;
  knn_distance_kernel<<<(unsigned)se3_cdiv(c.n_total, kOdWaves), kOdWaves * SE3_WAVE, 0, (hipStream_t)stream>>>(c.G.view(), q_points, elem, c.rows,
                                                                                                              c.n_total, k, column, out);
  SE3_CHECK_LAUNCH("knn_distance_stack");
  return SE3_OK;
}

extern "C" int se3_distance_stats_stack(const double* a, const int64_t* offsets_host, int num_clouds, double std_ratio, double* out_stats,
                                        uint8_t* out_mask, void* stream) {
  SE3_REQUIRE(a && offsets_host && out_stats && out_mask, SE3_ERR_INVALID_ARG, "distance_stats_stack: null pointer");
  SE3_REQUIRE(num_clouds >= 0 && num_clouds <= kPairMaxPairs, SE3_ERR_INVALID_ARG, "distance_stats_stack: %d clouds (at most %d)", num_clouds,
              kPairMaxPairs);
  SE3_REQUIRE(isfinite(std_ratio) && std_ratio > 0.0, SE3_ERR_INVALID_ARG, "distance_stats_stack: std_ratio %g is not a positive finite number",
              std_ratio);
  PairRows rows;
  SE3_REQUIRE(pg_fill_rows(&rows, offsets_host, num_clouds), SE3_ERR_INVALID_ARG, "distance_stats_stack: offsets must start at 0 and not decrease");
  const int64_t n_total = rows.start[num_clouds];
  SE3_REQUIRE(n_total < kOdMaxRows, SE3_ERR_UNSUPPORTED, "distance_stats_stack: %lld rows in one call (below 2^31)", (long long)n_total);
  if (num_clouds == 0) return SE3_OK;
  hipStream_t st = (hipStream_t)stream;
  cloud_stats_kernel<<<(unsigned)num_clouds, kFsLanes, 0, st>>>(a, rows, std_ratio, out_stats);
  if (n_total > 0) outlier_mask_kernel<<<(unsigned)se3_cdiv(n_total, kOdThreads), kOdThreads, 0, st>>>(a, rows, n_total, out_stats, out_mask);
  SE3_CHECK_LAUNCH("distance_stats_stack");
  return SE3_OK;
}

// ---- the same text on host memory, one cloud, no GPU (tests/test_outlier_cpu.py) ----------------------------------------------------------------
// out (n): the row values of the cloud searched in itself
extern "C" int se3_debug_knn_distance_host(const void* points, int64_t n, int elem, int k, int column, double* out) {
  SE3_REQUIRE(points && out, SE3_ERR_INVALID_ARG, "debug_knn_distance_host: null pointer");
  SE3_REQUIRE(n >= 0 && n < (1ll << 31) && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG, "debug_knn_distance_host: n %lld, elem %d", (long long)n,
              elem);
  SE3_REQUIRE(k >= 1 && k <= kPairKnnMax && column < k, SE3_ERR_INVALID_ARG, "debug_knn_distance_host: k %d not in [1, %d], or column %d not below it",
              k, kPairKnnMax, column);
  PairHostGrid H(points, n, elem, nullptr, 0.0);
  const PairGridView g = H.G.view();
  for (int64_t i = 0; i < n; i++) {
    double qv[3];
    pg_load3(points, elem, i, qv);
    PairKnnSerialList list;
    list.init(k);
    pg_knn(g, 0, qv, 0, 1, list);
    int cnt = 0;
    while (cnt < k && list.j[cnt] != kPairKnnEmpty) cnt++;
    out[i] = od_row_distance(cnt, column, [&](int t) { return pg_sqrt(list.d2[t]); });
  }
  return SE3_OK;
}

// out_stats (4: mean, std, thr, resolution) and out_mask (n, may be NULL) of one cloud's row values a (n)
extern "C" int se3_debug_distance_stats_host(const double* a, int64_t n, double std_ratio, double* out_stats, uint8_t* out_mask) {
  SE3_REQUIRE(a && out_stats, SE3_ERR_INVALID_ARG, "debug_distance_stats_host: null pointer");
  SE3_REQUIRE(n >= 0 && n < (1ll << 31), SE3_ERR_INVALID_ARG, "debug_distance_stats_host: n %lld", (long long)n);
  SE3_REQUIRE(isfinite(std_ratio) && std_ratio > 0.0, SE3_ERR_INVALID_ARG, "debug_distance_stats_host: std_ratio %g is not a positive finite number",
              std_ratio);
  std::vector<double> sh(kFsLanes);
  od_cloud_stats(a, n, std_ratio, 0, kFsLanes, sh.data(), [] {}, out_stats);
  if (out_mask)
    for (int64_t i = 0; i < n; i++) out_mask[i] = od_kept(a[i], out_stats[2]) ? 1 : 0;
  return SE3_OK;
}
