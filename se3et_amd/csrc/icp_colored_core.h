// The coloured ICP iteration of csrc/icp.hip as __host__ __device__ text, on the helpers of csrc/icp_core.h: one pair's finiteness check
// (icp_colored_pair_init) and one pair's evaluation, convergence test and update (icp_colored_pair_step).  The frame of the step -- the
// evaluation sums, the convergence rule, what lane 0 writes and the final correspondences -- follows icp_pair_step line by line, which
// stays as it is (its bits are pinned); only the per-correspondence term and its 27 one-pass sums are this file's own.  The contract is
// the header comment of icp.hip.
#pragma once
#include "icp_core.h"

// one pair's colours and gradients; every pointer already points at the pair's first entry
struct IcpColors {
  const void* src_colors;   // (n, 3), src_colors_elem
  int src_colors_elem;
  const void* ref_colors;   // (nref, 3), ref_colors_elem
  int ref_colors_elem;
  const double* gradients;  // (nref, 3): se3_color_gradient_stack's rows of the reference cloud
  double a, b;              // sqrt(lambda_geometric), sqrt(1 - lambda_geometric)
};

// ((c0 + c1) + c2) / 3.0
PG_HD double icp_intensity(const void* colors, int elem, int64_t row) {
#pragma clang fp contract(off)
  const double c0 = pg_load(colors, elem, 3 * row), c1 = pg_load(colors, elem, 3 * row + 1), c2 = pg_load(colors, elem, 3 * row + 2);
  const double s = (c0 + c1) + c2;
  return s / 3.0;
}

// (a b + c d) + e f
PG_HD double icp_dot3(const double* x, const double* y) {
#pragma clang fp contract(off)
  const double a = x[0] * y[0], b = x[1] * y[1], c = x[2] * y[2];
  return (a + b) + c;
}

// The two rows of correspondence i: Jg = a [p x nt, nt], rg = a (p - q) . nt;  Jc = b [p x d, d], rc = b (I_s - I_proj) with
// p' = p - ((p - q) . nt) nt, I_proj = g . (p' - q) + I_t and d = -(g - (nt . g) nt).
PG_HD void icp_colored_rows(const IcpPair& v, const IcpColors& col, const double* T, int64_t i, double* Jg, double* rg, double* Jc, double* rc) {
#pragma clang fp contract(off)
  double p[3], nt[3], g[3];
  icp_moved(v, T, i, p);
  const int64_t j = v.nn_idx[i];
  const double* q = v.ref + 3 * j;
  for (int e = 0; e < 3; e++) nt[e] = pg_load(v.normals, v.normals_elem, 3 * j + e), g[e] = col.gradients[3 * j + e];
  const double pq[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
  const double s = icp_dot3(pq, nt);
  *rg = col.a * s;
  double c[3];
  icp_cross(p, nt, c);
  for (int e = 0; e < 3; e++) Jg[e] = col.a * c[e], Jg[3 + e] = col.a * nt[e];
  double off[3];                                                        // p' - q
  for (int e = 0; e < 3; e++) {
    const double sn = s * nt[e];
    const double pp = p[e] - sn;
    off[e] = pp - q[e];
  }
  const double proj = icp_dot3(g, off) + icp_intensity(col.ref_colors, col.ref_colors_elem, j);
  const double diff = icp_intensity(col.src_colors, col.src_colors_elem, i) - proj;
  *rc = col.b * diff;
  const double ng = icp_dot3(nt, g);
  double d[3];
  for (int e = 0; e < 3; e++) {
    const double t = ng * nt[e];
    const double mg = g[e] - t;
    d[e] = -mg;
  }
  icp_cross(p, d, c);
  for (int e = 0; e < 3; e++) Jc[e] = col.b * c[e], Jc[3 + e] = col.b * d[e];
}

// icp_pair_init of point-to-plane, and in addition a non-finite source colour, reference colour or gradient refuses the pair
template <class Barrier>
PG_HD void icp_colored_pair_init(const IcpPair& v, const IcpColors& col, const double* T0, int lane_begin, int lane_end, double* sh,
                                 Barrier&& barrier) {
  icp_pair_init(v, T0, SE3_ICP_POINT_TO_PLANE, lane_begin, lane_end, sh, barrier);
  double bad[1], part[1];
  icp_sum<1>(v.n, lane_begin, lane_end,
             [&](int64_t i, double* acc) { acc[0] += icp_finite3(col.src_colors, col.src_colors_elem, i) ? 0.0 : 1.0; }, sh, barrier, bad);
  icp_sum<1>(v.nref, lane_begin, lane_end,
             [&](int64_t i, double* acc) {
               acc[0] += icp_finite3(col.ref_colors, col.ref_colors_elem, i) && icp_finite3(col.gradients, 1, i) ? 0.0 : 1.0;
             },
             sh, barrier, part);
  if (!(bad[0] + part[0] > 0.0)) return;
  if (lane_begin == 0) {
    for (int k = 0; k < 16; k++) v.T[k] = NAN;
    *v.status = SE3_ICP_NONFINITE;
    *v.done = 1;
  }
  if (v.corr)
    for (int l = lane_begin; l < lane_end; l++)
      for (int64_t i = l; i < v.n; i += kIcpLanes) v.corr[i] = -1;
}

// icp_pair_step for the coloured estimation: the frame of icp_pair_step with one update, (sum wg Jg Jg^T + wc Jc Jc^T) x =
// -sum (wg Jg rg + wc Jc rc), the 27 sums formed in one pass; sh holds kIcpGeneralSums columns.  kWeighted = false holds no weight code.
template <bool kWeighted, class Barrier>
PG_HD void icp_colored_pair_step(const IcpPair& v, const IcpColors& col, const IcpCriteria& crit, int k, int lane_begin, int lane_end, double* sh,
                                 Barrier&& barrier) {
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
    } else if (count < 6.0) {
      status |= SE3_ICP_TOO_FEW;
    } else {
      double s[kIcpGeneralSums];
      icp_sum<kIcpGeneralSums>(v.n, lane_begin, lane_end,
                               [&](int64_t i, double* acc) {
                                 if (!(v.nn_d2[i] < r2)) return;
                                 double Jg[6], Jc[6], rg, rc;
                                 icp_colored_rows(v, col, T, i, Jg, &rg, Jc, &rc);
                                 if constexpr (kWeighted) {
                                   const double wg = icp_weight(crit.loss, crit.loss_k, rg), wc = icp_weight(crit.loss, crit.loss_k, rc);
                                   for (int a = 0, e = 0; a < 6; a++) {
                                     const double wJg = wg * Jg[a], wJc = wc * Jc[a];
                                     for (int b = a; b < 6; b++, e++) {
                                       const double mg = wJg * Jg[b], mc = wJc * Jc[b];
                                       acc[e] = (acc[e] + mg) + mc;
                                     }
                                   }
                                   const double wrg = wg * rg, wrc = wc * rc;
                                   for (int a = 0; a < 6; a++) {
                                     const double mg = Jg[a] * wrg, mc = Jc[a] * wrc;
                                     acc[21 + a] = (acc[21 + a] + mg) + mc;
                                   }
                                   return;
                                 }
                                 for (int a = 0, e = 0; a < 6; a++)
                                   for (int b = a; b < 6; b++, e++) {
                                     const double mg = Jg[a] * Jg[b], mc = Jc[a] * Jc[b];
                                     acc[e] = (acc[e] + mg) + mc;
                                   }
                                 for (int a = 0; a < 6; a++) {
                                   const double mg = Jg[a] * rg, mc = Jc[a] * rc;
                                   acc[21 + a] = (acc[21 + a] + mg) + mc;
                                 }
                               },
                               sh, barrier, s);
      double rhs[6], x[6];
      for (int a = 0; a < 6; a++) rhs[a] = -s[21 + a];
      if (!icp_cholesky6(s, rhs, x)) {
        status |= SE3_ICP_SINGULAR;
      } else if (!(fabs(x[0]) < kIcpMaxAngle) || !(fabs(x[1]) < kIcpMaxAngle) || !(fabs(x[2]) < kIcpMaxAngle)) {
        status |= SE3_ICP_STEP_REFUSED;
        finished = true;                                                 // the pair ends at T, whose evaluation this is
      } else {
        icp_vector6_to_matrix(x, U);
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
