// The ICP iteration of csrc/icp.hip as __host__ __device__ text: one pair's finiteness check (icp_pair_init) and one pair's evaluation,
// convergence test and update (icp_pair_step), with the summation order they share.  The kernels run it with one workgroup of kIcpLanes
// threads per pair (each thread one lane, `barrier` = __syncthreads); se3_debug_icp_host runs the same text serially over all lanes with
// a no-op barrier.  The contract is the header comment of icp.hip.
//
// icp_pair_step<kWeighted, kGeneral> is four instantiations.  kWeighted = false holds no weight code at all: <false, false> is the text
// of se3_icp_stack, and its sums are not multiplied by 1.  kGeneral = true is generalized ICP alone, whose 27 sums are formed in one pass.
#pragma once
#include <math.h>
#include <stdint.h>

#include "kabsch.h"
#include "pair_grid.h"

// Summation order of every sum over a pair's rows: lane l of kIcpLanes adds rows l, l + kIcpLanes, .. serially from zero, then the
// lanes are added by the tree lane[l] += lane[l + o], o = kIcpLanes / 2 .. 1.  It depends on the pair's row count alone.
constexpr int kIcpLanes = 256;
constexpr int kIcpMaxSums = 21;                 // the widest sum: the upper triangle of the point-to-plane J^T J
constexpr int kIcpGeneralSums = 27;             // generalized ICP: the upper triangle of sum A^T M^-1 A and sum A^T M^-1 d, one pass
constexpr double kIcpPivotTol = 1e-13;          // a Cholesky pivot must exceed this share of its diagonal entry: below it is rounding
constexpr double kIcpMaxAngle = 1.0;            // rad: a linearised step with an angle this large is refused

struct IcpMath {                                // the Kabsch solve's root, rounded alike on the host and on the device
  static PG_HD double root(double x) { return pg_sqrt(x); }
};

struct IcpCriteria {
  double r2, relative_fitness, relative_rmse;
  int max_iteration, mode;                      // SE3_ICP_POINT_TO_POINT / SE3_ICP_POINT_TO_PLANE / SE3_ICP_GENERALIZED
  int loss;                                     // SE3_ICP_LOSS_*; SE3_ICP_LOSS_NONE selects the instantiations without weight code
  double loss_k, eps;                           // the loss's width k > 0; generalized ICP's epsilon in (0, 1]
};

// one pair's rows and results; every pointer already points at the pair's first entry
struct IcpPair {
  const void* src;          // (n, 3), elem
  int elem;
  int64_t n;
  const double* ref;        // (nref, 3): the grid's `moved` rows of the pair
  int64_t nref;
  const void* normals;      // (nref, 3), normals_elem; may be null for point-to-point
  int normals_elem;
  const void* src_normals;  // (n, 3), src_normals_elem: generalized ICP alone, null otherwise
  int src_normals_elem;
  int* nn_idx;              // (n): nearest reference row of the last evaluation
  double* nn_d2;            // (n)
  double* T;                // (4, 4): the current transform, the result at the end
  double* fitness;
  double* rmse;
  int* iterations;
  int* converged;
  int* status;
  int* done;
  int64_t* corr;            // (n) or null: the final correspondence of every row, -1 for none
};

// out[c] = the sum over rows 0 .. n - 1 of what term(i, acc) adds to acc[c], in the order above.  The caller owns lanes
// [lane_begin, lane_end); sh holds K * kIcpLanes values and is free again on return.  Every caller's lane gets the sums.
template <int K, class Term, class Barrier>
PG_HD void icp_sum(int64_t n, int lane_begin, int lane_end, Term&& term, double* sh, Barrier&& barrier, double* out) {
#pragma clang fp contract(off)
  for (int l = lane_begin; l < lane_end; l++) {
    double acc[K];
    for (int c = 0; c < K; c++) acc[c] = 0.0;
    for (int64_t i = l; i < n; i += kIcpLanes) term(i, acc);
    for (int c = 0; c < K; c++) sh[c * kIcpLanes + l] = acc[c];
  }
  barrier();
  for (int o = kIcpLanes / 2; o > 0; o >>= 1) {
    for (int l = lane_begin; l < lane_end; l++)
      if (l < o)
        for (int c = 0; c < K; c++) sh[c * kIcpLanes + l] = sh[c * kIcpLanes + l] + sh[c * kIcpLanes + l + o];
    barrier();
  }
  for (int c = 0; c < K; c++) out[c] = sh[c * kIcpLanes];
  barrier();
}

// sin and cos for |x| < 1 as Taylor polynomials in x^2, Horner form, every product and sum rounded on its own: the same bits from the
// host's and the device's compiler, which their libraries' sin and cos do not give.  Truncation below 1e-18, error below 2 ulp.
PG_HD double icp_sin(double x) {
#pragma clang fp contract(off)
  const double z = x * x;
  double p = -1.0 / 121645100408832000.0;                  // -1 / 19!
  p = p * z + 1.0 / 355687428096000.0;                     //  1 / 17!
  p = p * z - 1.0 / 1307674368000.0;                       // -1 / 15!
  p = p * z + 1.0 / 6227020800.0;                          //  1 / 13!
  p = p * z - 1.0 / 39916800.0;                            // -1 / 11!
  p = p * z + 1.0 / 362880.0;                              //  1 / 9!
  p = p * z - 1.0 / 5040.0;                                // -1 / 7!
  p = p * z + 1.0 / 120.0;                                 //  1 / 5!
  p = p * z - 1.0 / 6.0;                                   // -1 / 3!
  const double xz = x * z;
  const double tail = xz * p;
  return x + tail;
}
PG_HD double icp_cos(double x) {
#pragma clang fp contract(off)
  const double z = x * x;
  double p = 1.0 / 2432902008176640000.0;                  //  1 / 20!
  p = p * z - 1.0 / 6402373705728000.0;                    // -1 / 18!
  p = p * z + 1.0 / 20922789888000.0;                      //  1 / 16!
  p = p * z - 1.0 / 87178291200.0;                         // -1 / 14!
  p = p * z + 1.0 / 479001600.0;                           //  1 / 12!
  p = p * z - 1.0 / 3628800.0;                             // -1 / 10!
  p = p * z + 1.0 / 40320.0;                               //  1 / 8!
  p = p * z - 1.0 / 720.0;                                 // -1 / 6!
  p = p * z + 1.0 / 24.0;                                  //  1 / 4!
  p = p * z - 0.5;                                         // -1 / 2!
  const double tail = z * p;
  return 1.0 + tail;
}

PG_HD void icp_identity(double* U) {
  for (int k = 0; k < 16; k++) U[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

PG_HD bool icp_finite3(const void* a, int elem, int64_t i) {
  return isfinite(pg_load(a, elem, 3 * i)) && isfinite(pg_load(a, elem, 3 * i + 1)) && isfinite(pg_load(a, elem, 3 * i + 2));
}

// row i of the pair moved by T
PG_HD void icp_moved(const IcpPair& v, const double* T, int64_t i, double* p) { pg_transform_row(T, v.src, v.elem, i, p); }

// J = [p x n, n] and the residual (p - q) . n of correspondence i (point-to-plane): p the moved row, q its reference row, n q's normal
PG_HD void icp_plane_row(const IcpPair& v, const double* T, int64_t i, double* J, double* res) {
#pragma clang fp contract(off)
  double p[3];
  icp_moved(v, T, i, p);
  const int64_t j = v.nn_idx[i];
  const double* q = v.ref + 3 * j;
  const double nx = pg_load(v.normals, v.normals_elem, 3 * j), ny = pg_load(v.normals, v.normals_elem, 3 * j + 1),
               nz = pg_load(v.normals, v.normals_elem, 3 * j + 2);
  const double rx = (p[0] - q[0]) * nx, ry = (p[1] - q[1]) * ny, rz = (p[2] - q[2]) * nz;
  *res = (rx + ry) + rz;
  const double yz = p[1] * nz, zy = p[2] * ny, zx = p[2] * nx, xz = p[0] * nz, xy = p[0] * ny, yx = p[1] * nx;
  J[0] = yz - zy, J[1] = zx - xz, J[2] = xy - yx, J[3] = nx, J[4] = ny, J[5] = nz;
}

// Open3D's RobustKernel weights w(r) of a scalar residual, k > 0; every one is continuous at its branch.  Divisions and products are
// IEEE on both sides, so the host and the device give the same bits.
PG_HD double icp_weight(int loss, double k, double r) {
#pragma clang fp contract(off)
  const double a = fabs(r);
  if (loss == SE3_ICP_LOSS_HUBER) return a <= k ? 1.0 : k / a;
  const double t = r / k;
  const double tt = t * t;
  if (loss == SE3_ICP_LOSS_CAUCHY) return 1.0 / (1.0 + tt);
  if (loss == SE3_ICP_LOSS_GM) {
    const double rr = r * r;
    const double s = k + rr;
    return k / (s * s);
  }
  if (loss == SE3_ICP_LOSS_TUKEY) {
    if (!(a <= k)) return 0.0;
    const double u = 1.0 - tt;
    return u * u;
  }
  return 1.0;                                   // SE3_ICP_LOSS_L2
}

// p x v, every product rounded on its own
PG_HD void icp_cross(const double* p, const double* v, double* out) {
#pragma clang fp contract(off)
  const double yz = p[1] * v[2], zy = p[2] * v[1], zx = p[2] * v[0], xz = p[0] * v[2], xy = p[0] * v[1], yx = p[1] * v[0];
  out[0] = yz - zy, out[1] = zx - xz, out[2] = xy - yx;
}

// Correspondence i of generalized ICP: h[21] = the upper triangle of A^T B A, row by row, g[6] = A^T B d and *rho2 = d^T B d, with
// d = p - q, A = [-[p]_x | I] and B = M^-1, M = 2 I - (1 - eps)(nt nt^T + m m^T), m = R ns, inverted by its cofactors.  A^T = [[p]_x ; I],
// so the blocks are p x (columns of B G), p x (columns of B) and B itself, G = -[p]_x.  Every term is even in nt and in ns.
PG_HD void icp_general_row(const IcpPair& v, const double* T, double eps, int64_t i, double* h, double* g, double* rho2) {
#pragma clang fp contract(off)
  double p[3];
  icp_moved(v, T, i, p);
  const int64_t j = v.nn_idx[i];
  const double* q = v.ref + 3 * j;
  double nt[3], ns[3], m[3];
  for (int a = 0; a < 3; a++) nt[a] = pg_load(v.normals, v.normals_elem, 3 * j + a), ns[a] = pg_load(v.src_normals, v.src_normals_elem, 3 * i + a);
  for (int a = 0; a < 3; a++) {
    const double x = T[4 * a] * ns[0], y = T[4 * a + 1] * ns[1], z = T[4 * a + 2] * ns[2];
    m[a] = (x + y) + z;
  }
  const double c = 1.0 - eps;
  double M[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = a; b < 3; b++) {
      const double tt = nt[a] * nt[b], mm = m[a] * m[b];
      const double s = c * (tt + mm);
      M[a][b] = M[b][a] = (a == b ? 2.0 : 0.0) - s;
    }
  double C[3][3];                                                       // the cofactors of the symmetric M
  {
    const double df = M[1][1] * M[2][2], ee = M[1][2] * M[1][2], ce = M[0][2] * M[1][2], bf = M[0][1] * M[2][2], be = M[0][1] * M[1][2],
                 cd = M[0][2] * M[1][1], af = M[0][0] * M[2][2], cc = M[0][2] * M[0][2], bc = M[0][1] * M[0][2], ae = M[0][0] * M[1][2],
                 ad = M[0][0] * M[1][1], bb = M[0][1] * M[0][1];
    C[0][0] = df - ee, C[0][1] = C[1][0] = ce - bf, C[0][2] = C[2][0] = be - cd;
    C[1][1] = af - cc, C[1][2] = C[2][1] = bc - ae, C[2][2] = ad - bb;
  }
  const double d0 = M[0][0] * C[0][0], d1 = M[0][1] * C[0][1], d2 = M[0][2] * C[0][2];
  const double det = (d0 + d1) + d2;
  double B[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) B[a][b] = C[a][b] / det;
  const double d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
  double e[3];                                                          // B d
  for (int a = 0; a < 3; a++) {
    const double x = B[a][0] * d[0], y = B[a][1] * d[1], z = B[a][2] * d[2];
    e[a] = (x + y) + z;
  }
  {
    const double x = d[0] * e[0], y = d[1] * e[1], z = d[2] * e[2];
    *rho2 = (x + y) + z;
  }
  double F[6][6];                                                       // A^T B A, the upper triangle
  for (int b = 0; b < 3; b++) {
    double col[3], out[3];
    // column b of B G: G = [[0, pz, -py], [-pz, 0, px], [py, -px, 0]]
    for (int a = 0; a < 3; a++) {
      const int b1 = (b + 1) % 3, b2 = (b + 2) % 3;                     // column b of G holds p[b1] in row b2 and -p[b2] in row b1
      const double x = B[a][b2] * p[b1], y = B[a][b1] * p[b2];
      col[a] = x - y;
    }
    icp_cross(p, col, out);
    for (int a = 0; a <= b; a++) F[a][b] = out[a];
    for (int a = 0; a < 3; a++) col[a] = B[a][b];
    icp_cross(p, col, out);
    for (int a = 0; a < 3; a++) F[a][3 + b] = out[a];
    for (int a = 0; a <= b; a++) F[3 + a][3 + b] = B[a][b];
  }
  for (int a = 0, k = 0; a < 6; a++)
    for (int b = a; b < 6; b++, k++) h[k] = F[a][b];
  icp_cross(p, e, g);
  g[3] = e[0], g[4] = e[1], g[5] = e[2];
}

// T <- U T for two rigid 4x4 (the last rows are 0 0 0 1): (a b + c d) + e f per entry, the translation added last
PG_HD void icp_compose(const double* U, const double* T, double* out) {
#pragma clang fp contract(off)
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 4; j++) {
      const double a = U[4 * i] * T[j], b = U[4 * i + 1] * T[4 + j], c = U[4 * i + 2] * T[8 + j];
      const double s = (a + b) + c;
      out[4 * i + j] = j == 3 ? s + U[4 * i + 3] : s;
    }
  }
  out[12] = 0.0, out[13] = 0.0, out[14] = 0.0, out[15] = 1.0;
}

// Solves A x = rhs for the symmetric 6x6 A (upper triangle in a[21], row by row) by a Cholesky factorisation.  False when a pivot is not
// above kIcpPivotTol of its diagonal entry: the system is not positive definite to rounding.
PG_HD bool icp_cholesky6(const double* a, const double* rhs, double* x) {
#pragma clang fp contract(off)
  double A[6][6], L[6][6];
  for (int i = 0, e = 0; i < 6; i++)
    for (int j = i; j < 6; j++, e++) A[i][j] = A[j][i] = a[e];
  for (int j = 0; j < 6; j++) {
    double d = A[j][j];
    for (int k = 0; k < j; k++) {
      const double sq = L[j][k] * L[j][k];
      d = d - sq;
    }
    if (!(d > kIcpPivotTol * A[j][j]) || !(d < INFINITY)) return false;
    L[j][j] = pg_sqrt(d);
    for (int i = j + 1; i < 6; i++) {
      double s = A[i][j];
      for (int k = 0; k < j; k++) {
        const double m = L[i][k] * L[j][k];
        s = s - m;
      }
      L[i][j] = s / L[j][j];
    }
  }
  double y[6];
  for (int i = 0; i < 6; i++) {
    double s = rhs[i];
    for (int k = 0; k < i; k++) {
      const double m = L[i][k] * y[k];
      s = s - m;
    }
    y[i] = s / L[i][i];
  }
  for (int i = 5; i >= 0; i--) {
    double s = y[i];
    for (int k = i + 1; k < 6; k++) {
      const double m = L[k][i] * x[k];
      s = s - m;
    }
    x[i] = s / L[i][i];
  }
  return true;
}

// [Rz Ry Rx | x3 x4 x5] from the sines and cosines of the three angles: Open3D's TransformVector6dToMatrix4d
PG_HD void icp_sincos_to_matrix(double sx, double cx, double sy, double cy, double sz, double cz, const double* x, double* U) {
#pragma clang fp contract(off)
  const double sxsy = sx * sy, cxsy = cx * sy;
  const double a01 = sxsy * cz, b01 = cx * sz, a02 = cxsy * cz, b02 = sx * sz;
  const double a11 = sxsy * sz, b11 = cx * cz, a12 = cxsy * sz, b12 = sx * cz;
  U[0] = cy * cz, U[1] = a01 - b01, U[2] = a02 + b02, U[3] = x[3];
  U[4] = cy * sz, U[5] = a11 + b11, U[6] = a12 - b12, U[7] = x[4];
  U[8] = -sy, U[9] = sx * cy, U[10] = cx * cy, U[11] = x[5];
  U[12] = 0.0, U[13] = 0.0, U[14] = 0.0, U[15] = 1.0;
}

// [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5] for angles of (-1, 1), with the shared sin and cos
PG_HD void icp_vector6_to_matrix(const double* x, double* U) {
  icp_sincos_to_matrix(icp_sin(x[0]), icp_cos(x[0]), icp_sin(x[1]), icp_cos(x[1]), icp_sin(x[2]), icp_cos(x[2]), x, U);
}

// Before the first evaluation: T <- T0, the results cleared; a non-finite T0, point or normal that the mode reads (point-to-plane: the
// reference's; generalized: both clouds') refuses the pair: SE3_ICP_NONFINITE, a NaN transform, done.
template <class Barrier>
PG_HD void icp_pair_init(const IcpPair& v, const double* T0, int mode, int lane_begin, int lane_end, double* sh, Barrier&& barrier) {
  double bad[1], part[1];
  icp_sum<1>(v.n, lane_begin, lane_end,
             [&](int64_t i, double* acc) {
               bool ok = icp_finite3(v.src, v.elem, i);
               if (mode == SE3_ICP_GENERALIZED) ok = ok && icp_finite3(v.src_normals, v.src_normals_elem, i);
               acc[0] += ok ? 0.0 : 1.0;
             },
             sh, barrier, bad);
  icp_sum<1>(v.nref, lane_begin, lane_end,
             [&](int64_t i, double* acc) {
               bool ok = icp_finite3(v.ref, 1, i);
               if (mode != SE3_ICP_POINT_TO_POINT) ok = ok && icp_finite3(v.normals, v.normals_elem, i);
               acc[0] += ok ? 0.0 : 1.0;
             },
             sh, barrier, part);
  bool refused = bad[0] + part[0] > 0.0;
  for (int k = 0; k < 16; k++) refused = refused || !isfinite(T0[k]);
  if (lane_begin == 0) {
    for (int k = 0; k < 16; k++) v.T[k] = refused ? NAN : (k < 12 ? T0[k] : (k == 15 ? 1.0 : 0.0));
    *v.fitness = 0.0, *v.rmse = 0.0, *v.iterations = 0, *v.converged = 0;
    *v.status = refused ? SE3_ICP_NONFINITE : 0;
    *v.done = refused ? 1 : 0;
  }
  if (refused && v.corr)
    for (int l = lane_begin; l < lane_end; l++)
      for (int64_t i = l; i < v.n; i += kIcpLanes) v.corr[i] = -1;
}

// Evaluation k of a pair from the (index, d^2) its rows hold, the convergence test against evaluation k - 1, and, when the pair goes on,
// the update U and T <- U T.  Uniform over the lanes: every lane forms the same sums and solves the same system; lane 0 writes.
// kWeighted: every term of the update's sums carries w(residual) of crit.loss (iteratively reweighted least squares, the weights from
// this evaluation); the counts, fitness and rmse never do.  kGeneral: crit.mode is SE3_ICP_GENERALIZED, and sh holds kIcpGeneralSums
// columns; otherwise it is one of the other two and sh holds kIcpMaxSums.
template <bool kWeighted, bool kGeneral, class Barrier>
PG_HD void icp_pair_step(const IcpPair& v, const IcpCriteria& crit, int k, int lane_begin, int lane_end, double* sh, Barrier&& barrier) {
#pragma clang fp contract(off)
  if (*v.done) return;
  double T[16];
  for (int e = 0; e < 16; e++) T[e] = v.T[e];
  const double prev_fitness = *v.fitness, prev_rmse = *v.rmse;
  int status = *v.status;
  barrier();                                                             // (every lane has read the state lane 0 writes below)
  const double r2 = crit.r2;
  double ev[2];
  icp_sum<2>(v.n, lane_begin, lane_end,
             [&](int64_t i, double* acc) {
               const double d2 = v.nn_d2[i];
               if (d2 < r2) acc[0] += 1.0, acc[1] += d2;
             },
             sh, barrier, ev);
  const double count = ev[0];
  const double fitness = v.n > 0 ? count / (double)v.n : 0.0;
  const double rmse = count > 0.0 ? pg_sqrt(ev[1] / count) : 0.0;
  int converged = 0;
  bool finished = false;
  if (k >= 1 && fabs(fitness - prev_fitness) < crit.relative_fitness && fabs(rmse - prev_rmse) < crit.relative_rmse) converged = 1, finished = true;
  if (k >= crit.max_iteration) finished = true;
  double U[16], Tn[16];
  if (!finished) {
    icp_identity(U);
    if (v.n == 0 || v.nref == 0) {
      status |= SE3_ICP_EMPTY;
    } else if constexpr (kGeneral) {
      if (count < 6.0) {
        status |= SE3_ICP_TOO_FEW;
      } else {
        double s[kIcpGeneralSums];
        icp_sum<kIcpGeneralSums>(v.n, lane_begin, lane_end,
                                 [&](int64_t i, double* acc) {
                                   if (!(v.nn_d2[i] < r2)) return;
                                   double h[21], g[6], rho2;
                                   icp_general_row(v, T, crit.eps, i, h, g, &rho2);
                                   if constexpr (kWeighted) {
                                     const double w = icp_weight(crit.loss, crit.loss_k, pg_sqrt(rho2));
                                     for (int e = 0; e < 21; e++) {
                                       const double m = w * h[e];
                                       acc[e] += m;
                                     }
                                     for (int a = 0; a < 6; a++) {
                                       const double m = w * g[a];
                                       acc[21 + a] += m;
                                     }
                                   } else {
                                     for (int e = 0; e < 21; e++) acc[e] += h[e];
                                     for (int a = 0; a < 6; a++) acc[21 + a] += g[a];
                                   }
                                 },
                                 sh, barrier, s);
        double rhs[6], x[6];
        for (int a = 0; a < 6; a++) rhs[a] = -s[21 + a];
        if (!icp_cholesky6(s, rhs, x)) {
          status |= SE3_ICP_SINGULAR;
        } else if (!(fabs(x[0]) < kIcpMaxAngle) || !(fabs(x[1]) < kIcpMaxAngle) || !(fabs(x[2]) < kIcpMaxAngle)) {
          status |= SE3_ICP_STEP_REFUSED;
          finished = true;
        } else {
          icp_vector6_to_matrix(x, U);
        }
      }
    } else if (crit.mode == SE3_ICP_POINT_TO_POINT) {
      if (count < 3.0) {
        status |= SE3_ICP_TOO_FEW;
      } else if constexpr (kWeighted) {
        // weighted Kabsch: w = w(sqrt(d^2)); W = sum w, the centroids sum w p / W and sum w q / W, H = sum w (p - pc)(q - qc)^T
        double s[7], pc[3], qc[3], h[9];
        icp_sum<7>(v.n, lane_begin, lane_end,
                   [&](int64_t i, double* acc) {
                     if (!(v.nn_d2[i] < r2)) return;
                     const double w = icp_weight(crit.loss, crit.loss_k, pg_sqrt(v.nn_d2[i]));
                     double p[3];
                     icp_moved(v, T, i, p);
                     const double* q = v.ref + 3 * (int64_t)v.nn_idx[i];
                     acc[6] += w;
                     for (int d = 0; d < 3; d++) {
                       const double wp = w * p[d], wq = w * q[d];
                       acc[d] += wp, acc[3 + d] += wq;
                     }
                   },
                   sh, barrier, s);
        if (!(s[6] > 0.0) || !(s[6] < INFINITY)) {
          status |= SE3_ICP_SINGULAR;                                    // no weight left: the identity update
        } else {
          for (int d = 0; d < 3; d++) pc[d] = s[d] / s[6], qc[d] = s[3 + d] / s[6];
          icp_sum<9>(v.n, lane_begin, lane_end,
                     [&](int64_t i, double* acc) {
                       if (!(v.nn_d2[i] < r2)) return;
                       const double w = icp_weight(crit.loss, crit.loss_k, pg_sqrt(v.nn_d2[i]));
                       double p[3];
                       icp_moved(v, T, i, p);
                       const double* q = v.ref + 3 * (int64_t)v.nn_idx[i];
                       for (int a = 0; a < 3; a++) {
                         const double pa = w * (p[a] - pc[a]);
                         for (int b = 0; b < 3; b++) {
                           const double qb = q[b] - qc[b];
                           const double m = pa * qb;
                           acc[3 * a + b] += m;
                         }
                       }
                     },
                     sh, barrier, h);
          double H[3][3];
          for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) H[a][b] = h[3 * a + b];
          kabsch<IcpMath, double>(H, pc, qc, U);
        }
      } else {
        double s[6], pc[3], qc[3], h[9];
        icp_sum<6>(v.n, lane_begin, lane_end,
                   [&](int64_t i, double* acc) {
                     if (!(v.nn_d2[i] < r2)) return;
                     double p[3];
                     icp_moved(v, T, i, p);
                     const double* q = v.ref + 3 * (int64_t)v.nn_idx[i];
                     for (int d = 0; d < 3; d++) acc[d] += p[d], acc[3 + d] += q[d];
                   },
                   sh, barrier, s);
        for (int d = 0; d < 3; d++) pc[d] = s[d] / count, qc[d] = s[3 + d] / count;
        icp_sum<9>(v.n, lane_begin, lane_end,
                   [&](int64_t i, double* acc) {
                     if (!(v.nn_d2[i] < r2)) return;
                     double p[3];
                     icp_moved(v, T, i, p);
                     const double* q = v.ref + 3 * (int64_t)v.nn_idx[i];
                     for (int a = 0; a < 3; a++) {
                       const double pa = p[a] - pc[a];
                       for (int b = 0; b < 3; b++) {
                         const double qb = q[b] - qc[b];
                         const double m = pa * qb;
                         acc[3 * a + b] += m;
                       }
                     }
                   },
                   sh, barrier, h);
        double H[3][3];
        for (int a = 0; a < 3; a++)
          for (int b = 0; b < 3; b++) H[a][b] = h[3 * a + b];
        kabsch<IcpMath, double>(H, pc, qc, U);
      }
    } else {
      if (count < 6.0) {
        status |= SE3_ICP_TOO_FEW;
      } else {
        double s[27];
        icp_sum<21>(v.n, lane_begin, lane_end,
                    [&](int64_t i, double* acc) {
                      if (!(v.nn_d2[i] < r2)) return;
                      double J[6], res;
                      icp_plane_row(v, T, i, J, &res);
                      if constexpr (kWeighted) {
                        const double w = icp_weight(crit.loss, crit.loss_k, res);
                        for (int a = 0, e = 0; a < 6; a++) {
                          const double wJ = w * J[a];
                          for (int b = a; b < 6; b++, e++) {
                            const double m = wJ * J[b];
                            acc[e] += m;
                          }
                        }
                        return;
                      }
                      for (int a = 0, e = 0; a < 6; a++)
                        for (int b = a; b < 6; b++, e++) {
                          const double m = J[a] * J[b];
                          acc[e] += m;
                        }
                    },
                    sh, barrier, s);
        icp_sum<6>(v.n, lane_begin, lane_end,
                   [&](int64_t i, double* acc) {
                     if (!(v.nn_d2[i] < r2)) return;
                     double J[6], res;
                     icp_plane_row(v, T, i, J, &res);
                     if constexpr (kWeighted) {
                       const double wr = icp_weight(crit.loss, crit.loss_k, res) * res;
                       for (int a = 0; a < 6; a++) {
                         const double m = J[a] * wr;
                         acc[a] += m;
                       }
                       return;
                     }
                     for (int a = 0; a < 6; a++) {
                       const double m = J[a] * res;
                       acc[a] += m;
                     }
                   },
                   sh, barrier, s + 21);
        double rhs[6], x[6];
        for (int a = 0; a < 6; a++) rhs[a] = -s[21 + a];
        if (!icp_cholesky6(s, rhs, x)) {
          status |= SE3_ICP_SINGULAR;
        } else if (!(fabs(x[0]) < kIcpMaxAngle) || !(fabs(x[1]) < kIcpMaxAngle) || !(fabs(x[2]) < kIcpMaxAngle)) {
          status |= SE3_ICP_STEP_REFUSED;
          finished = true;                                               // the pair ends at T, whose evaluation this is
        } else {
          icp_vector6_to_matrix(x, U);
        }
      }
    }
    if (!finished) icp_compose(U, T, Tn);
  }
  if (lane_begin == 0) {
    *v.fitness = fitness, *v.rmse = rmse, *v.iterations = k, *v.converged = converged, *v.status = status;
    if (finished) *v.done = 1;
    else
      for (int e = 0; e < 16; e++) v.T[e] = Tn[e];
  }
  if (finished && v.corr)
    for (int l = lane_begin; l < lane_end; l++)
      for (int64_t i = l; i < v.n; i += kIcpLanes) v.corr[i] = v.nn_d2[i] < r2 ? (int64_t)v.nn_idx[i] : -1;
}
