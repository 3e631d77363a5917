// Scan preparation, part 2: exact k nearest neighbours and k-NN normals of stacked clouds (Open3D's estimate_normals with a k-NN 33 search,
// geotransformer/utils/open3d.py:49-54), on the float64 grid of csrc/pair_grid.h.  se3et_amd/scan_prep.py carries the same contract.
// (SE3_EXACT_FP: the file is built with contraction off, and every contract function fences itself as well.)
//
//   knn_kernel           one wave per query row: lanes stride the points of a ring's cells (pg_knn), the wave keeps its best list as one
//                        (d^2, index) entry per lane, sorted across lanes, the k-th value wave-uniform; a candidate that beats it is
//                        broadcast and inserted by a compare-and-shift across lanes.  Lane t < k writes column t.
//   knn_normals_kernel   the same search, then the normal from the list in registers: the (n, k) tables never go to memory.
//
// Contract.
//   k nearest neighbours (k in [1, 64]).  For every query row the min(k, n_support) support points of its own cloud with the smallest
//     d^2 = (dx dx + dy dy) + dz dz, float64 and unfused (pg_dist2); rows sorted ascending by (d^2, index): among equal distances the
//     lower index comes first and wins the last slot.  A cloud searched in itself returns each point as its own first neighbour (as
//     Open3D's search does); duplicates are ordered by index.  Missing columns hold index -1 and distance +inf.  The search is exact; the
//     grid is only an accelerator: the rings widen until the k-th best d^2 is no larger than pg_shell_bound2.
//   normals (knn = 33 by default).  Over the row's m = min(knn, n) neighbours in list order: mean = (sequential sum) / m; the six entries
//     of C = sum (p - mean)(p - mean)^T / m are each a sequential sum in list order, contraction off.  The normal is a unit eigenvector of
//     C for its smallest eigenvalue, float64 (cyclic Jacobi, a fixed number of sweeps), with the canonical sign: z > 0, or z == 0 and
//     y > 0, or z == y == 0 and x > 0.  It is exactly (0, 0, 1) when m < 3 or C is the zero matrix (Open3D's fallback).  With viewpoints
//     each normal is then oriented so that n . (viewpoint - p) >= 0.
//     This is not Open3D's arithmetic (single-pass cumulants, an analytic 3x3 solver): a row whose two smallest eigenvalues are within
//     rounding of each other, or which has a distance tie at the k-th place, can differ beyond rounding.
//   No float atomics; a row's result does not depend on the batch it is in, nor on the run.
#include <math.h>

#include "common.h"
#include "cov3.h"
#include "pair_grid.h"

namespace {

static_assert(kPairKnnMax == SE3_KNN_MAX, "pair_grid.h and include/se3et_hip.h name one limit");
constexpr int kKnnWaves = 4;          // query rows per workgroup
constexpr int64_t kKnnMaxRows = (1ll << 31) / kPairKnnMax;          // out_idx and out_d2 index row * k + column below 2^31

// ---- the normal of a neighbour list: the same text on the host and on the device (kn_covariance, kn_rotate, kn_jacobi: csrc/cov3.h) ---------
// unit eigenvector of the symmetric C for its smallest eigenvalue, canonical sign; (0, 0, 1) for m < 3 or C = 0
PG_HD void kn_normal(int m, const double* C, double* n) {
#pragma clang fp contract(off)
  n[0] = 0.0, n[1] = 0.0, n[2] = 1.0;
  if (m < 3 || (C[0] == 0.0 && C[1] == 0.0 && C[2] == 0.0 && C[3] == 0.0 && C[4] == 0.0 && C[5] == 0.0)) return;
  double a[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  kn_jacobi(a, v);
  double x = v[0][0], y = v[1][0], z = v[2][0], best = a[0][0];
  if (a[1][1] < best) x = v[0][1], y = v[1][1], z = v[2][1], best = a[1][1];
  if (a[2][2] < best) x = v[0][2], y = v[1][2], z = v[2][2];
  const double xx = x * x, yy = y * y, zz = z * z;
  const double len = pg_sqrt((xx + yy) + zz);
  if (!(len > 0.0) || !(len < INFINITY)) return;                                  // (non-finite input: the fallback)
  x = x / len, y = y / len, z = z / len;
  // the canonical sign: that of the last non-zero of (x, y, z) is made positive, by selects and an exact product by +-1.  (Observed with
  // hipcc 7.2 for gfx950: written as `keep = z > 0 || (z == 0 && (y > 0 || (y == 0 && x > 0))); if (!keep) negate`, the kernel returned
  // rows with z == 0 and y < 0 un-negated while the host build of the same text negated them; the cause was not isolated.)
  const double lead = z != 0.0 ? z : (y != 0.0 ? y : x);
  const double sign = lead < 0.0 ? -1.0 : 1.0;
  n[0] = sign * x, n[1] = sign * y, n[2] = sign * z;
}

// n . (viewpoint - p) >= 0
PG_HD void kn_orient(const double* view, const double* p, double* n) {
#pragma clang fp contract(off)
  const double dx = view[0] - p[0], dy = view[1] - p[1], dz = view[2] - p[2];
  const double a = n[0] * dx, b = n[1] * dy, c = n[2] * dz;
  if ((a + b) + c < 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
}

struct KnnViewpoints {
  double v[kPairMaxPairs][3];
  int on;
};

__global__ __launch_bounds__(kKnnWaves* SE3_WAVE) void knn_kernel(PairGridView g, const void* __restrict__ q, int elem, PairRows rows,
                                                                  int64_t nq_total, int k, int64_t* __restrict__ out_idx,
                                                                  double* __restrict__ out_d2) {
  const int64_t i = (int64_t)blockIdx.x * kKnnWaves + (threadIdx.x >> 6);
  if (i >= nq_total) return;                               // (uniform over the wave)
  double qv[3];
  pg_load3(q, elem, i, qv);
  WaveKnnList list;
  list.init(k);
  pg_knn(g, pg_pair_of_row(rows, i), qv, se3_lane(), SE3_WAVE, list);
  const int l = se3_lane();
  if (l < k) {
    out_idx[i * k + l] = list.j == kPairKnnEmpty ? -1 : list.j;
    out_d2[i * k + l] = list.j == kPairKnnEmpty ? INFINITY : list.d2;
  }
}

__global__ __launch_bounds__(kKnnWaves* SE3_WAVE) void knn_normals_kernel(PairGridView g, const double* __restrict__ moved,
                                                                          const void* __restrict__ q, int elem, PairRows rows,
                                                                          int64_t nq_total, int k, KnnViewpoints views,
                                                                          double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kKnnWaves + (threadIdx.x >> 6);
  if (i >= nq_total) return;
  const int p = pg_pair_of_row(rows, i);
  double qv[3];
  pg_load3(q, elem, i, qv);
  WaveKnnList list;
  list.init(k);
  pg_knn(g, p, qv, se3_lane(), SE3_WAVE, list);
  // lane t fetches neighbour t; every lane then forms the same sums in list order from the lanes' values (a fixed serial order)
  const int m = __popcll(__ballot(se3_lane() < k && list.j != kPairKnnEmpty));
  double mine[3] = {0.0, 0.0, 0.0};
  if (se3_lane() < m) {
    const double* s = moved + 3 * (g.meta[p].s_start + list.j);
    mine[0] = s[0], mine[1] = s[1], mine[2] = s[2];
  }
  double C[6], n[3];
  kn_covariance(m, [&](int t, double* pt) { pt[0] = __shfl(mine[0], t), pt[1] = __shfl(mine[1], t), pt[2] = __shfl(mine[2], t); }, C);
  kn_normal(m, C, n);
  if (views.on) kn_orient(views.v[p], qv, n);
  if (se3_lane() == 0) out[3 * i] = n[0], out[3 * i + 1] = n[1], out[3 * i + 2] = n[2];
}

}  // namespace

extern "C" int se3_knn_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                             const int64_t* q_offsets_host, int num_clouds, int k, int64_t* out_idx, double* out_d2, void* stream) {
  SE3_REQUIRE(k >= 1 && k <= kPairKnnMax, SE3_ERR_INVALID_ARG, "knn_stack: k %d not in [1, %d]", k, kPairKnnMax);
  PairGridCall c;
  if (const int rc = pg_grid_call("knn_stack", "clouds", q_points && out_idx && out_d2, grid_workspace, workspace_bytes, ns_total, elem,
                                  q_offsets_host, num_clouds, kKnnMaxRows, &c))
    return rc;
  if (c.n_total == 0) return SE3_OK;
  knn_kernel<<<(unsigned)se3_cdiv(c.n_total, kKnnWaves), kKnnWaves * SE3_WAVE, 0, (hipStream_t)stream>>>(c.G.view(), q_points, elem, c.rows,
                                                                                                        c.n_total, k, out_idx, out_d2);
  SE3_CHECK_LAUNCH("knn_stack");
  return SE3_OK;
}

extern "C" int se3_knn_normals_stack(const void* grid_workspace, size_t workspace_bytes, int64_t ns_total, const void* q_points, int elem,
                                     const int64_t* q_offsets_host, int num_clouds, int k, const double* viewpoints_host, double* out_normals,
                                     void* stream) {
  SE3_REQUIRE(k >= 1 && k <= kPairKnnMax, SE3_ERR_INVALID_ARG, "knn_normals_stack: k %d not in [1, %d]", k, kPairKnnMax);
  PairGridCall c;
  if (const int rc = pg_grid_call("knn_normals_stack", "clouds", q_points && out_normals, grid_workspace, workspace_bytes, ns_total, elem,
                                  q_offsets_host, num_clouds, kKnnMaxRows, &c))
    return rc;
  KnnViewpoints views;
  views.on = viewpoints_host != nullptr;
  for (int p = 0; p < kPairMaxPairs; p++)
    for (int d = 0; d < 3; d++) {
      views.v[p][d] = views.on && p < num_clouds ? viewpoints_host[3 * p + d] : 0.0;
      SE3_REQUIRE(isfinite(views.v[p][d]), SE3_ERR_INVALID_ARG, "knn_normals_stack: non-finite viewpoint");
    }
  if (c.n_total == 0) return SE3_OK;
  knn_normals_kernel<<<(unsigned)se3_cdiv(c.n_total, kKnnWaves), kKnnWaves * SE3_WAVE, 0, (hipStream_t)stream>>>(
      c.G.view(), c.G.moved, q_points, elem, c.rows, c.n_total, k, views, out_normals);
  SE3_CHECK_LAUNCH("knn_normals_stack");
  return SE3_OK;
}

// ---- the same text on host memory, one cloud, no GPU (tests/test_scan_prep_cpu.py) -----------------------------------------------------------
extern "C" int se3_debug_knn_host(const void* q_points, int64_t nq, const void* s_points, int64_t ns, int elem, int k, int64_t* out_idx,
                                  double* out_d2) {
  SE3_REQUIRE(q_points && s_points && out_idx && out_d2, SE3_ERR_INVALID_ARG, "debug_knn_host: null pointer");
  SE3_REQUIRE(nq >= 0 && ns >= 0 && ns < (1ll << 31) && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG, "debug_knn_host: nq %lld, ns %lld, elem %d",
              (long long)nq, (long long)ns, elem);
  SE3_REQUIRE(k >= 1 && k <= kPairKnnMax, SE3_ERR_INVALID_ARG, "debug_knn_host: k %d not in [1, %d]", k, kPairKnnMax);
  PairHostGrid H(s_points, ns, elem, nullptr, 0.0);
  const PairGridView g = H.G.view();
  for (int64_t i = 0; i < nq; i++) {
    double qv[3];
    pg_load3(q_points, elem, i, qv);
    PairKnnSerialList list;
    list.init(k);
    pg_knn(g, 0, qv, 0, 1, list);
    for (int t = 0; t < k; t++) {
      out_idx[i * k + t] = list.j[t] == kPairKnnEmpty ? -1 : list.j[t];
      out_d2[i * k + t] = list.j[t] == kPairKnnEmpty ? INFINITY : list.d2[t];
    }
  }
  return SE3_OK;
}

// normals (n, 3) of a cloud searched in itself; covariances (n, 6: xx xy xz yy yz zz) may be NULL; viewpoint (3) may be NULL
extern "C" int se3_debug_knn_normals_host(const void* points, int64_t n, int elem, int k, const double* viewpoint, double* out_normals,
                                          double* out_covariances) {
  SE3_REQUIRE(points && out_normals, SE3_ERR_INVALID_ARG, "debug_knn_normals_host: null pointer");
  SE3_REQUIRE(n >= 0 && n < (1ll << 31) && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG, "debug_knn_normals_host: n %lld, elem %d", (long long)n,
              elem);
  SE3_REQUIRE(k >= 1 && k <= kPairKnnMax, SE3_ERR_INVALID_ARG, "debug_knn_normals_host: k %d not in [1, %d]", k, kPairKnnMax);
  SE3_REQUIRE(!viewpoint || (isfinite(viewpoint[0]) && isfinite(viewpoint[1]) && isfinite(viewpoint[2])), SE3_ERR_INVALID_ARG,
              "debug_knn_normals_host: non-finite viewpoint");
  PairHostGrid H(points, n, elem, nullptr, 0.0);
  const PairGridView g = H.G.view();
  for (int64_t i = 0; i < n; i++) {
    double qv[3];
    pg_load3(points, elem, i, qv);
    PairKnnSerialList list;
    list.init(k);
    pg_knn(g, 0, qv, 0, 1, list);
    int m = 0;
    while (m < k && list.j[m] != kPairKnnEmpty) m++;
    double C[6], nrm[3];
    kn_covariance(m, [&](int t, double* pt) { for (int d = 0; d < 3; d++) pt[d] = H.G.moved[3 * (int64_t)list.j[t] + d]; }, C);
    kn_normal(m, C, nrm);
    if (viewpoint) kn_orient(viewpoint, qv, nrm);
    for (int d = 0; d < 3; d++) out_normals[3 * i + d] = nrm[d];
    if (out_covariances)
      for (int e = 0; e < 6; e++) out_covariances[6 * i + e] = C[e];
  }
  return SE3_OK;
}
