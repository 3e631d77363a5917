// Colour gradients of stacked clouds: the per-point intensity gradient in the tangent plane that Open3D's registration_colored_icp prepares
// once per reference cloud (ColoredICP.cpp: InitializePointCloudForColoredICP), for up to SE3_PAIR_MAX_PAIRS stacked clouds per call, all
// float64.  se3et_amd/icp.py carries the same contract; csrc/icp.hip reads the result (se3_icp_colored_stack).
// (SE3_EXACT_FP: the file is built with contraction off, and every contract function fences itself as well.)
//
//   color_gradient_kernel   one thread per stacked row: the finiteness check of the row (a plain store of 1 to its cloud's status word: no
//                           atomics), then cg_row over the row's line of the (n, K) table of se3_knn_stack.
//
// The search is NOT fused.  csrc/pair_grid.h searches the k nearest with one wave per row and leaves the list one entry per lane; the sums
// below are sequential in list order, so a fused kernel would either walk the list through 30 shuffles per lane with 63 lanes idle, as
// knn_normals_kernel does for its nine sums, or redo the search per thread.  The table costs 16 bytes x K per row once per call and scale
// (58 MB for 120 000 rows at K = 30), which the search itself outweighs; the kernel reads a table the caller already has a kernel for,
// and the host entry reuses the serial list of se3_debug_knn_host.
//
// Contract.  Points, normals and colours are (rows, 3) of float32 or float64, promoted on load.
//   Intensity.  The intensity of a row with colour (c0, c1, c2) is ((c0 + c1) + c2) / 3.0.  Any finite range is accepted.
//   Neighbours of row i: the hybrid search with the rules of se3et_amd/fpfh.py.  Take the K = max_nn nearest rows of row i's own cloud,
//     including row i, K in [1, SE3_KNN_MAX] (Open3D's value is 30), ordered ascending by (d^2, index).  Of those, keep the rows with
//     d^2 < r^2, strict, r^2 = r r in float64; m is the size of that result.  The neighbours are its members other than row i itself,
//     chosen by index.  (Open3D drops entry 0 of the result instead: the two rules differ only where a duplicate point has a lower index.)
//     m < 4 gives the zero gradient.
//   Sums, formed by one thread per row sequentially, in the list's order, unfused.  For a neighbour j: u = p_j - p_i, s = (u . n) with
//     dots as (a b + c d) + e f and n the normal as given (not normalised), pr = u - s n, G += pr pr^T, h += pr (I_j - I_i).  Afterwards
//     G += (m - 1)^2 n n^T: Open3D's orthogonality row (m - 1) n with right-hand side 0.
//   Solve.  G x = h by a 3x3 Cholesky factorisation; a pivot not above 1e-13 of its diagonal entry gives the zero gradient (ICP's rule;
//     Open3D solves by LDLT without a guard).
//   Refusals.  A non-finite point, normal or colour refuses the cloud: bit 1 of the cloud's status word, and of the last word for any (as
//     se3_fpfh_check_stack); the rows of a refused cloud are not to be read.  n = 0 gives an empty output.
//   Determinism.  No atomics.  A cloud's rows are bit-identical alone, anywhere in a batch, and from run to run.
#include <math.h>

#include <vector>

#include "common.h"
#include "pair_grid.h"

namespace {

constexpr double kCgPivotTol = 1e-13;           // kIcpPivotTol of csrc/icp_core.h: a pivot must exceed this share of its diagonal entry
constexpr int kCgMinMembers = 4;                // m below this: the zero gradient

PG_HD double cg_intensity(const void* colors, int elem, int64_t row) {
#pragma clang fp contract(off)
  double c[3];
  pg_load3(colors, elem, row, c);
  const double s = (c[0] + c[1]) + c[2];
  return s / 3.0;
}

PG_HD double cg_dot(const double* a, const double* b) {
#pragma clang fp contract(off)
  const double x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
  return (x + y) + z;
}

// Solves G x = h for the symmetric 3x3 G (xx xy xz yy yz zz) by a Cholesky factorisation; false when a pivot is not above kCgPivotTol of
// its diagonal entry.
PG_HD bool cg_cholesky3(const double* g, const double* h, double* x) {
#pragma clang fp contract(off)
  const double A[3][3] = {{g[0], g[1], g[2]}, {g[1], g[3], g[4]}, {g[2], g[4], g[5]}};
  double L[3][3];
  for (int j = 0; j < 3; j++) {
    double d = A[j][j];
    for (int k = 0; k < j; k++) {
      const double sq = L[j][k] * L[j][k];
      d = d - sq;
    }
    if (!(d > kCgPivotTol * A[j][j]) || !(d < INFINITY)) return false;
    L[j][j] = pg_sqrt(d);
    for (int i = j + 1; i < 3; i++) {
      double s = A[i][j];
      for (int k = 0; k < j; k++) {
        const double m = L[i][k] * L[j][k];
        s = s - m;
      }
      L[i][j] = s / L[j][j];
    }
  }
  double y[3];
  for (int i = 0; i < 3; i++) {
    double s = h[i];
    for (int k = 0; k < i; k++) {
      const double m = L[i][k] * y[k];
      s = s - m;
    }
    y[i] = s / L[i][i];
  }
  for (int i = 2; i >= 0; i--) {
    double s = y[i];
    for (int k = i + 1; k < 3; k++) {
      const double m = L[k][i] * x[k];
      s = s - m;
    }
    x[i] = s / L[i][i];
  }
  return true;
}

// The gradient of cloud-local row i of a cloud of n rows whose first row is row s0 of the stacked arrays.  idx / d2: the row's K list
// entries, cloud-local, ascending by (d^2, index); an entry outside [0, n) (the -1 of a smaller cloud) is no member.
PG_HD void cg_row(const void* points, int elem, const void* normals, int normals_elem, const void* colors, int colors_elem, int64_t s0, int64_t n,
                  int64_t i, const int64_t* idx, const double* d2, int K, double r2, double* out) {
#pragma clang fp contract(off)
  out[0] = 0.0, out[1] = 0.0, out[2] = 0.0;
  int m = 0;
  for (int t = 0; t < K; t++)
    if (idx[t] >= 0 && idx[t] < n && d2[t] < r2) m++;
  if (m < kCgMinMembers) return;
  double p[3], nr[3];
  pg_load3(points, elem, s0 + i, p);
  pg_load3(normals, normals_elem, s0 + i, nr);
  const double Ii = cg_intensity(colors, colors_elem, s0 + i);
  double G[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, h[3] = {0.0, 0.0, 0.0};
  for (int t = 0; t < K; t++) {
    const int64_t j = idx[t];
    if (!(j >= 0 && j < n && d2[t] < r2) || j == i) continue;
    double pj[3];
    pg_load3(points, elem, s0 + j, pj);
    const double u[3] = {pj[0] - p[0], pj[1] - p[1], pj[2] - p[2]};
    const double s = cg_dot(u, nr);
    double pr[3];
    for (int a = 0; a < 3; a++) {
      const double sn = s * nr[a];
      pr[a] = u[a] - sn;
    }
    const double dI = cg_intensity(colors, colors_elem, s0 + j) - Ii;
    for (int a = 0, e = 0; a < 3; a++) {
      for (int b = a; b < 3; b++, e++) {
        const double v = pr[a] * pr[b];
        G[e] += v;
      }
      const double v = pr[a] * dI;
      h[a] += v;
    }
  }
  const double w = (double)(m - 1) * (double)(m - 1);
  for (int a = 0, e = 0; a < 3; a++)
    for (int b = a; b < 3; b++, e++) {
      const double nn = nr[a] * nr[b];
      const double v = w * nn;
      G[e] += v;
    }
  double x[3];
  if (!cg_cholesky3(G, h, x)) return;
  out[0] = x[0], out[1] = x[1], out[2] = x[2];
}

PG_HD bool cg_finite3(const void* a, int elem, int64_t row) {
  return isfinite(pg_load(a, elem, 3 * row)) && isfinite(pg_load(a, elem, 3 * row + 1)) && isfinite(pg_load(a, elem, 3 * row + 2));
}

struct CgCall {
  const void* points;
  const void* normals;
  const void* colors;
  int elem, normals_elem, colors_elem;
  PairRows rows;
  int64_t n_total;
  const int64_t* idx;             // (n_total, K) cloud-local, se3_knn_stack's
  const double* d2;               // (n_total, K)
  int K;
  double r2;
};

__global__ __launch_bounds__(256) void color_gradient_kernel(CgCall c, double* __restrict__ out, int* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= c.n_total) return;
  const int p = pg_pair_of_row(c.rows, i);
  if (!(cg_finite3(c.points, c.elem, i) && cg_finite3(c.normals, c.normals_elem, i) && cg_finite3(c.colors, c.colors_elem, i)))
    status[p] = 1, status[c.rows.n] = 1;                   // (every writer stores the same word: no atomic is needed)
  const int64_t s0 = c.rows.start[p];
  double g[3];
  cg_row(c.points, c.elem, c.normals, c.normals_elem, c.colors, c.colors_elem, s0, c.rows.start[p + 1] - s0, i - s0, c.idx + i * c.K,
         c.d2 + i * c.K, c.K, c.r2, g);
  out[3 * i] = g[0], out[3 * i + 1] = g[1], out[3 * i + 2] = g[2];
}

bool cg_elems_ok(int elem, int normals_elem, int colors_elem) {
  return (elem == 0 || elem == 1) && (normals_elem == 0 || normals_elem == 1) && (colors_elem == 0 || colors_elem == 1);
}

}  // namespace

extern "C" int se3_color_gradient_stack(const void* points, int elem, const void* normals, int normals_elem, const void* colors, int colors_elem,
                                        const int64_t* offsets_host, int num_clouds, const int64_t* knn_idx, const double* knn_d2, int k,
                                        double radius, double* out_gradients, int* status, void* stream) {
  SE3_REQUIRE(points && normals && colors && offsets_host && knn_idx && knn_d2 && out_gradients && status, SE3_ERR_INVALID_ARG,
              "color_gradient_stack: null pointer");
  SE3_REQUIRE(num_clouds >= 0 && num_clouds <= kPairMaxPairs && cg_elems_ok(elem, normals_elem, colors_elem), SE3_ERR_INVALID_ARG,
              "color_gradient_stack: %d clouds (at most %d), elem %d, normals_elem %d, colors_elem %d", num_clouds, kPairMaxPairs, elem,
              normals_elem, colors_elem);
  SE3_REQUIRE(k >= 1 && k <= kPairKnnMax, SE3_ERR_INVALID_ARG, "color_gradient_stack: k %d not in [1, %d]", k, kPairKnnMax);
  SE3_REQUIRE(pg_radius_ok(radius), SE3_ERR_INVALID_ARG, "color_gradient_stack: radius %g is not finite and >= 0", radius);
  CgCall c;
  SE3_REQUIRE(pg_fill_rows(&c.rows, offsets_host, num_clouds), SE3_ERR_INVALID_ARG, "color_gradient_stack: offsets must start at 0 and not decrease");
  c.n_total = c.rows.start[num_clouds];
  SE3_REQUIRE(c.n_total < (1ll << 31) / kPairKnnMax, SE3_ERR_UNSUPPORTED, "color_gradient_stack: %lld rows in one call", (long long)c.n_total);
  hipStream_t st = (hipStream_t)stream;
  SE3_REQUIRE(hipMemsetAsync(status, 0, sizeof(int) * (size_t)(num_clouds + 1), st) == hipSuccess, SE3_ERR_LAUNCH,
              "color_gradient_stack: memset failed");
  if (c.n_total == 0) return SE3_OK;
  c.points = points, c.normals = normals, c.colors = colors, c.elem = elem, c.normals_elem = normals_elem, c.colors_elem = colors_elem;
  c.idx = knn_idx, c.d2 = knn_d2, c.K = k, c.r2 = radius * radius;
  color_gradient_kernel<<<(unsigned)se3_cdiv(c.n_total, 256), 256, 0, st>>>(c, out_gradients, status);
  SE3_CHECK_LAUNCH("color_gradient_stack");
  return SE3_OK;
}

// ---- the same text on host memory, one cloud, no GPU (tests/test_colored_icp_cpu.py) ----------------------------------------------------------
// The list of every row is se3_debug_knn_host's: the cloud searched in itself.  *status: 0, or bit 1 for a non-finite point, normal or
// colour (nothing is computed).
extern "C" int se3_debug_color_gradient_host(const void* points, const void* normals, const void* colors, int64_t n, int elem, int normals_elem,
                                             int colors_elem, int k, double radius, double* out_gradients, int* status) {
  SE3_REQUIRE(points && normals && colors && out_gradients && status, SE3_ERR_INVALID_ARG, "debug_color_gradient_host: null pointer");
  SE3_REQUIRE(n >= 0 && n < (1ll << 31) / kPairKnnMax && cg_elems_ok(elem, normals_elem, colors_elem), SE3_ERR_INVALID_ARG,
              "debug_color_gradient_host: n %lld, elem %d, normals_elem %d, colors_elem %d", (long long)n, elem, normals_elem, colors_elem);
  SE3_REQUIRE(k >= 1 && k <= kPairKnnMax, SE3_ERR_INVALID_ARG, "debug_color_gradient_host: k %d not in [1, %d]", k, kPairKnnMax);
  SE3_REQUIRE(pg_radius_ok(radius), SE3_ERR_INVALID_ARG, "debug_color_gradient_host: radius %g is not finite and >= 0", radius);
  *status = 0;
  for (int64_t i = 0; i < n; i++)
    if (!(cg_finite3(points, elem, i) && cg_finite3(normals, normals_elem, i) && cg_finite3(colors, colors_elem, i))) *status = 1;
  if (*status || n == 0) return SE3_OK;
  PairHostGrid H(points, n, elem, nullptr, 0.0);
  const PairGridView g = H.G.view();
  const double r2 = radius * radius;
  for (int64_t i = 0; i < n; i++) {
    double qv[3];
    pg_load3(points, elem, i, qv);
    PairKnnSerialList list;
    list.init(k);
    pg_knn(g, 0, qv, 0, 1, list);
    int64_t idx[kPairKnnMax];
    for (int t = 0; t < k; t++) idx[t] = list.j[t] == kPairKnnEmpty ? -1 : list.j[t];
    cg_row(points, elem, normals, normals_elem, colors, colors_elem, 0, n, i, idx, list.d2, k, r2, out_gradients + 3 * i);
  }
  return SE3_OK;
}
