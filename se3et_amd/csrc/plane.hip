// Plane segmentation of stacked clouds by RANSAC (Open3D's segment_plane) for up to SE3_PAIR_MAX_PAIRS clouds per call.  Cloud c owns the
// rows [offsets[c], offsets[c + 1]) of the stacked points; n = their count, H = num_iterations hypotheses per cloud.
// se3et_amd/segmentation.py carries the same contract; csrc/plane_core.h holds the text that the kernels and se3_debug_plane_host share.
// (SE3_EXACT_FP: the file is built with contraction off, and every contract function fences itself as well.)
//
// Contract (all float64; float32 points are promoted on load).
//   1. Refusals.  A cloud with fewer than ransac_n rows gets status SE3_PLANE_TOO_FEW, plane (0, 0, 0, 0) and no inliers.  ransac_n lies in
//      [3, SE3_PLANE_MAX_SAMPLE = 16].
//   2. Sampling.  Hypothesis h draws ransac_n cloud-local rows with splitmix_draw(splitmix64(seed), h, ransac_n, j, n) (csrc/splitmix.h): it
//      depends on (seed, h, j, n) alone, never on the cloud's place in the batch.
//   3. The plane of a row set (pl_plane_of_rows; samples and the refit).  Exactly 3 rows: n = (p1 - p0) x (p2 - p0), every product and
//      difference rounded on its own, normalised with pg_sqrt, through c = p0.  More rows: the centroid c, the scatter matrix
//      (kn_covariance) and the unit eigenvector of its smallest eigenvalue (csrc/cov3.h).  In both cases the sign is canonical (the first
//      non-zero component is positive) and d = -((a c_x + b c_y) + c c_z).  A plane that is not defined scores 0 inliers: a zero or
//      non-finite cross product, a zero scatter matrix.
//   4. Scoring.  dist_i = ((a x + b y) + c z) + d, unfused.  Row i is an inlier iff |dist_i| < distance_threshold, strictly.  The count is
//      an integer.  The error sum adds dist^2 of the inliers in a fixed shape that depends on the cloud's row count alone: rows are cut into
//      segments of SE3_PLANE_SEGMENT = 1024; within a segment the sum runs in ascending row order from 0.0; the segment sums are then
//      added in ascending segment order from 0.0.
//   5. Order.  More inliers wins, then the smaller error sum, then the lower h.  All num_iterations hypotheses are evaluated.  A hypothesis
//      needs at least 3 inliers to win; otherwise the status is SE3_PLANE_NONE (plane (0, 0, 0, 0), no inliers, h = -1).
//   6. Refit.  The plane of item 3 is fitted over the winner's inliers: centroid and scatter through fs_sum (csrc/fixed_sum.h) over the
//      rows in ascending order, one workgroup per cloud.  Inliers, count, fitness = count / n and inlier_rmse = pg_sqrt(error sum / count)
//      are then recomputed against the refit plane and returned.  If the refit is undefined the winner's own plane is returned.
//   7. Departures from Open3D.  The sampler (counter based, with replacement; Open3D shuffles without replacement).  No early exit
//      (`probability` has no effect: every hypothesis is evaluated).  An eigenvector fit for more than 3 rows and for the refit instead of
//      its determinant formula.  The canonical sign (Open3D returns whichever orientation its fit produced).  The summation orders above.
//   Determinism.  No float atomics: a cloud's result is bit-identical alone, anywhere in a batch, from run to run, and between the device
//   and se3_debug_plane_host.
//
// Three launches, nothing read back:
//   plane_fit_kernel      one thread per (cloud, hypothesis): sample, the plane of item 3, four doubles to the workspace (NaN for an invalid
//                         hypothesis: it then scores 0 inliers).
//   plane_score_kernel    one workgroup of SE3_PLANE_TILE = 128 threads per (tile of hypotheses, segment of rows, cloud): a lane owns one
//                         hypothesis, the segment's rows pass through LDS in chunks of 256 and are read at one address per wave, the lane
//                         adds its hypothesis' dist^2 serially in row order and writes (count, segment sum).  Splitting over row segments is
//                         what fills the GPU at Open3D's default of 100 hypotheses.
//   plane_select_kernel   one workgroup of 256 threads per cloud: pl_select (the fold over the segments, the order of item 5, the refit of
//                         item 6, the outputs; on request every hypothesis' count and error sum).
#include <math.h>

#include <vector>

#include "common.h"
#include "plane_core.h"

namespace {

constexpr int kPlaneFitThreads = 128;
constexpr int kPlaneChunk = 256;          // rows per LDS stage
constexpr int kPlaneMaxIterations = 1 << 20;
constexpr int64_t kPlaneMaxRows = 1ll << 31;
static_assert(kPlaneMaxSample == SE3_PLANE_MAX_SAMPLE && kPlaneTile == SE3_PLANE_TILE && kPlaneSegment == SE3_PLANE_SEGMENT &&
                  kPlaneMaxIterations == SE3_PLANE_MAX_ITERATIONS,
              "plane_core.h and include/se3et_hip.h name the same limits");
static_assert(kPlaneOk == SE3_PLANE_OK && kPlaneTooFew == SE3_PLANE_TOO_FEW && kPlaneNone == SE3_PLANE_NONE, "and the same status codes");
static_assert(kPlaneSegment % kPlaneChunk == 0, "a segment is whole LDS stages");

struct PlaneLayout {
  double* hyp;          // [P][H][4]
  int* part_count;      // [P][Smax][H]
  double* part_sum;     // [P][Smax][H]
  double* seg_sums;     // [P][Smax]
};

size_t plane_carve(int num_clouds, int H, int64_t smax, char* base, PlaneLayout* L) {
  Se3Carver c(base);
  const size_t P = (size_t)(num_clouds > 0 ? num_clouds : 1), h = (size_t)(H > 0 ? H : 1), s = (size_t)(smax > 0 ? smax : 1);
  PlaneLayout l;
  l.hyp = c.take<double>(P * h * 4);
  l.part_count = c.take<int>(P * s * h);
  l.part_sum = c.take<double>(P * s * h);
  l.seg_sums = c.take<double>(P * s);
  if (L) *L = l;
  return c.bytes();
}

// the most segments of a cloud; -1 for offsets that do not start at 0 or decrease
int64_t plane_smax(const int64_t* offsets, int num_clouds) {
  if (offsets[0] != 0) return -1;
  int64_t smax = 0;
  for (int p = 0; p < num_clouds; p++) {
    if (offsets[p + 1] < offsets[p]) return -1;
    const int64_t s = se3_cdiv(offsets[p + 1] - offsets[p], kPlaneSegment);
    if (s > smax) smax = s;
  }
  return smax;
}

__global__ __launch_bounds__(kPlaneFitThreads) void plane_fit_kernel(const void* __restrict__ points, int elem, PairRows rows, int H, int rn,
                                                                     uint64_t key, double* __restrict__ hyp) {
  const int p = blockIdx.y;
  const int h = blockIdx.x * kPlaneFitThreads + threadIdx.x;
  if (h >= H) return;
  const int64_t s0 = rows.start[p], n = rows.start[p + 1] - s0;
  double plane[4];
  const bool ok = n >= rn && pl_plane_of_rows(
                                 rn,
                                 [&](int t, double* pt) {
                                   pg_load3(points, elem, s0 + splitmix_draw(key, (uint64_t)h, (uint64_t)rn, (uint64_t)t, (uint64_t)n), pt);
                                 },
                                 plane);
  double* out = hyp + ((int64_t)p * H + h) * 4;
  for (int k = 0; k < 4; k++) out[k] = ok ? plane[k] : NAN;
}

__global__ __launch_bounds__(kPlaneTile) void plane_score_kernel(const void* __restrict__ points, int elem, PairRows rows, int H, int64_t smax,
                                                                 double thr, const double* __restrict__ hyp, int* __restrict__ part_count,
                                                                 double* __restrict__ part_sum) {
  __shared__ double lds[3 * kPlaneChunk];
  const int p = blockIdx.z;
  const int64_t seg = blockIdx.y;
  const int64_t s0 = rows.start[p], n = rows.start[p + 1] - s0;
  const int64_t r0 = seg * kPlaneSegment;
  if (r0 >= n) return;                                                  // (uniform over the workgroup: a cloud with fewer segments)
  const int64_t r1 = r0 + kPlaneSegment < n ? r0 + kPlaneSegment : n;
  const int h = blockIdx.x * kPlaneTile + threadIdx.x;
  double plane[4];
  for (int k = 0; k < 4; k++) plane[k] = h < H ? hyp[((int64_t)p * H + h) * 4 + k] : NAN;
  int count = 0;
  double sum = 0.0;
  for (int64_t base = r0; base < r1; base += kPlaneChunk) {
    const int m = (int)(r1 - base < kPlaneChunk ? r1 - base : kPlaneChunk);
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * m; i += kPlaneTile) lds[i] = pg_load(points, elem, 3 * (s0 + base) + i);
    __syncthreads();
    for (int i = 0; i < m; i++) pl_add(pl_distance(plane, lds + 3 * i), thr, &count, &sum);          // one address per wave: an LDS broadcast
  }
  if (h < H) {
    const int64_t at = ((int64_t)p * smax + seg) * H + h;
    part_count[at] = count, part_sum[at] = sum;
  }
}

struct PlaneOutputs {
  double* planes;
  uint8_t* mask;
  int *counts, *status, *best;
  double *fitness, *rmse;
  int* hyp_counts;
  double* hyp_errs;
};

PG_HD PlaneJob plane_job(const void* points, int elem, int64_t s0, int64_t n, int p, int rn, int H, int64_t smax, double thr, const PlaneLayout& L,
                         const PlaneOutputs& o) {
  PlaneJob j;
  j.points = points, j.elem = elem, j.s0 = s0, j.n = n, j.rn = rn, j.H = H, j.S = (n + kPlaneSegment - 1) / kPlaneSegment, j.thr = thr;
  j.hyp = L.hyp + (int64_t)p * H * 4;
  j.part_count = L.part_count + (int64_t)p * smax * H;
  j.part_sum = L.part_sum + (int64_t)p * smax * H;
  j.seg_sums = L.seg_sums + (int64_t)p * smax;
  j.plane = o.planes + 4 * p, j.mask = o.mask + s0, j.count = o.counts + p, j.status = o.status + p, j.best = o.best + p;
  j.fitness = o.fitness + p, j.rmse = o.rmse + p;
  j.hyp_counts = o.hyp_counts ? o.hyp_counts + (int64_t)p * H : nullptr;
  j.hyp_errs = o.hyp_errs ? o.hyp_errs + (int64_t)p * H : nullptr;
  return j;
}

__global__ __launch_bounds__(kFsLanes) void plane_select_kernel(const void* __restrict__ points, int elem, PairRows rows, int rn, int H,
                                                                int64_t smax, double thr, PlaneLayout L, PlaneOutputs o) {
  __shared__ PlaneShared sh;
  const int p = blockIdx.x, t = threadIdx.x;
  const int64_t s0 = rows.start[p];
  const PlaneJob j = plane_job(points, elem, s0, rows.start[p + 1] - s0, p, rn, H, smax, thr, L, o);
  pl_select(j, t, t + 1, &sh, [] { __syncthreads(); });
}

bool plane_args(const char* what, double thr, int rn, int H) {
  if (!(isfinite(thr) && thr > 0.0)) return se3_set_error("%s: distance_threshold %g is not a positive finite number", what, thr), false;
  if (rn < 3 || rn > kPlaneMaxSample) return se3_set_error("%s: ransac_n %d not in [3, %d]", what, rn, kPlaneMaxSample), false;
  if (H < 1 || H > kPlaneMaxIterations) return se3_set_error("%s: num_iterations %d not in [1, %d]", what, H, kPlaneMaxIterations), false;
  return true;
}

}  // namespace

extern "C" size_t se3_plane_segment_workspace_bytes(const int64_t* offsets_host, int num_clouds, int num_iterations) {
  if (!offsets_host || num_clouds < 0 || num_clouds > kPairMaxPairs || num_iterations < 1 || num_iterations > kPlaneMaxIterations) return 0;
  const int64_t smax = plane_smax(offsets_host, num_clouds);
  if (smax < 0) return 0;
  return plane_carve(num_clouds, num_iterations, smax, nullptr, nullptr);
}

extern "C" int se3_plane_segment_stack(const void* points, int elem, const int64_t* offsets_host, int num_clouds, double distance_threshold,
                                       int ransac_n, int num_iterations, uint64_t seed, double* out_planes, uint8_t* out_mask, int* out_counts,
                                       double* out_fitness, double* out_rmse, int* out_status, int* out_best, int* out_hyp_counts,
                                       double* out_hyp_errs, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "plane_segment_stack";
  SE3_REQUIRE(points && offsets_host && out_planes && out_mask && out_counts && out_fitness && out_rmse && out_status && out_best && workspace,
              SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE((out_hyp_counts == nullptr) == (out_hyp_errs == nullptr), SE3_ERR_INVALID_ARG, "%s: the per-hypothesis outputs go together", what);
  SE3_REQUIRE(num_clouds >= 0 && num_clouds <= kPairMaxPairs && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG, "%s: %d clouds (at most %d), elem %d",
              what, num_clouds, kPairMaxPairs, elem);
  if (!plane_args(what, distance_threshold, ransac_n, num_iterations)) return SE3_ERR_INVALID_ARG;
  PairRows rows;
  SE3_REQUIRE(pg_fill_rows(&rows, offsets_host, num_clouds), SE3_ERR_INVALID_ARG, "%s: offsets must start at 0 and not decrease", what);
  SE3_REQUIRE(rows.start[num_clouds] < kPlaneMaxRows, SE3_ERR_UNSUPPORTED, "%s: %lld rows in one call (below 2^31)", what,
              (long long)rows.start[num_clouds]);
  if (num_clouds == 0) return SE3_OK;
  const int H = num_iterations;
  const int64_t smax = plane_smax(offsets_host, num_clouds);
  SE3_REQUIRE(smax <= 65535, SE3_ERR_UNSUPPORTED, "%s: a cloud of more than %lld rows", what, 65535ll * kPlaneSegment);
  PlaneLayout L;
  SE3_REQUIRE(plane_carve(num_clouds, H, smax, (char*)workspace, &L) <= workspace_bytes, SE3_ERR_WORKSPACE,
              "%s: workspace of %zu bytes is too small", what, workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  plane_fit_kernel<<<dim3((unsigned)se3_cdiv(H, kPlaneFitThreads), (unsigned)num_clouds), kPlaneFitThreads, 0, st>>>(
      points, elem, rows, H, ransac_n, splitmix64(seed), L.hyp);
  if (smax > 0)
    plane_score_kernel<<<dim3((unsigned)se3_cdiv(H, kPlaneTile), (unsigned)smax, (unsigned)num_clouds), kPlaneTile, 0, st>>>(
        points, elem, rows, H, smax, distance_threshold, L.hyp, L.part_count, L.part_sum);
  const PlaneOutputs o{out_planes, out_mask, out_counts, out_status, out_best, out_fitness, out_rmse, out_hyp_counts, out_hyp_errs};
  plane_select_kernel<<<(unsigned)num_clouds, kFsLanes, 0, st>>>(points, elem, rows, ransac_n, H, smax, distance_threshold, L, o);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

// ---- the same text on host memory, one cloud, no GPU (tests/test_segmentation_cpu.py) ---------------------------------------------------------
// out_plane (4), out_mask (n), the scalars (1 each); out_hyp_counts / out_hyp_errs (num_iterations) may both be NULL
extern "C" int se3_debug_plane_host(const void* points, int64_t n, int elem, double distance_threshold, int ransac_n, int num_iterations,
                                    uint64_t seed, double* out_plane, uint8_t* out_mask, int* out_count, double* out_fitness, double* out_rmse,
                                    int* out_status, int* out_best, int* out_hyp_counts, double* out_hyp_errs) {
  const char* what = "debug_plane_host";
  SE3_REQUIRE(points && out_plane && out_mask && out_count && out_fitness && out_rmse && out_status && out_best, SE3_ERR_INVALID_ARG,
              "%s: null pointer", what);
  SE3_REQUIRE((out_hyp_counts == nullptr) == (out_hyp_errs == nullptr), SE3_ERR_INVALID_ARG, "%s: the per-hypothesis outputs go together", what);
  SE3_REQUIRE(n >= 0 && n < kPlaneMaxRows && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG, "%s: n %lld, elem %d", what, (long long)n, elem);
  if (!plane_args(what, distance_threshold, ransac_n, num_iterations)) return SE3_ERR_INVALID_ARG;
  const int H = num_iterations;
  const int64_t smax = se3_cdiv(n, kPlaneSegment);
  std::vector<char> mem(plane_carve(1, H, smax, nullptr, nullptr));
  PlaneLayout L;
  plane_carve(1, H, smax, mem.data(), &L);
  const uint64_t key = splitmix64(seed);
  for (int h = 0; h < H; h++) {
    double plane[4];
    const bool ok = n >= ransac_n && pl_plane_of_rows(
                                         ransac_n,
                                         [&](int t, double* pt) {
                                           pg_load3(points, elem, splitmix_draw(key, (uint64_t)h, (uint64_t)ransac_n, (uint64_t)t, (uint64_t)n), pt);
                                         },
                                         plane);
    for (int k = 0; k < 4; k++) L.hyp[4 * (int64_t)h + k] = ok ? plane[k] : NAN;
    for (int64_t seg = 0; seg < smax; seg++) {
      const int64_t r1 = (seg + 1) * kPlaneSegment < n ? (seg + 1) * kPlaneSegment : n;
      int count = 0;
      double sum = 0.0, p[3];
      for (int64_t i = seg * kPlaneSegment; i < r1; i++) {
        pg_load3(points, elem, i, p);
        pl_add(pl_distance(L.hyp + 4 * (int64_t)h, p), distance_threshold, &count, &sum);
      }
      L.part_count[seg * H + h] = count, L.part_sum[seg * H + h] = sum;
    }
  }
  const PlaneOutputs o{out_plane, out_mask, out_count, out_status, out_best, out_fitness, out_rmse, out_hyp_counts, out_hyp_errs};
  const PlaneJob j = plane_job(points, elem, 0, n, 0, ransac_n, H, smax, distance_threshold, L, o);
  PlaneShared sh;
  pl_select(j, 0, kFsLanes, &sh, [] {});
  return SE3_OK;
}
