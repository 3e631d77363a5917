// The arithmetic of plane segmentation (csrc/plane.hip carries the contract): the plane of a row set, a row's signed distance and the
// inlier step, the order of two hypotheses, and the selection with its refit in the lane-and-barrier shape of csrc/fixed_sum.h.
// __host__ __device__ text that the kernels and se3_debug_plane_host both run; float64, contraction off in every function.
#pragma once
#include <math.h>

#include "cov3.h"
#include "fixed_sum.h"
#include "pair_grid.h"
#include "splitmix.h"

constexpr int kPlaneMaxSample = 16;      // SE3_PLANE_MAX_SAMPLE
constexpr int kPlaneTile = 128;          // SE3_PLANE_TILE: hypotheses per scoring workgroup, one per lane
constexpr int kPlaneSegment = 1024;      // SE3_PLANE_SEGMENT: rows per segment of the error sum
constexpr int kPlaneOk = 0, kPlaneTooFew = 2, kPlaneNone = 64;          // enum se3_plane_status

// the unit normal of direction (x, y, z) with the canonical sign (first non-zero component positive) and d = -(n . c); false, and nothing
// written, for a zero or non-finite direction or a non-finite d
PG_HD bool pl_finish(double x, double y, double z, const double* c, double* plane) {
#pragma clang fp contract(off)
  const double xx = x * x, yy = y * y, zz = z * z;
  const double len = pg_sqrt((xx + yy) + zz);
  if (!(len > 0.0) || !(len < INFINITY)) return false;
  x = x / len, y = y / len, z = z / len;
  const double lead = x != 0.0 ? x : (y != 0.0 ? y : z);                // (selects and an exact product by +-1, as kn_normal's sign)
  const double sign = lead < 0.0 ? -1.0 : 1.0;
  const double a = sign * x, b = sign * y, cc = sign * z;
  const double ax = a * c[0], by = b * c[1], cz = cc * c[2];
  const double d = -((ax + by) + cz);
  if (!(fabs(d) < INFINITY)) return false;
  plane[0] = a, plane[1] = b, plane[2] = cc, plane[3] = d;
  return true;
}

// exactly 3 rows: n = (p1 - p0) x (p2 - p0), every product and difference rounded on its own; the plane passes through p0
PG_HD bool pl_plane_from_three(const double* p0, const double* p1, const double* p2, double* plane) {
#pragma clang fp contract(off)
  const double ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
  const double vx = p2[0] - p0[0], vy = p2[1] - p0[1], vz = p2[2] - p0[2];
  const double a0 = uy * vz, a1 = uz * vy, b0 = uz * vx, b1 = ux * vz, c0 = ux * vy, c1 = uy * vx;
  return pl_finish(a0 - a1, b0 - b1, c0 - c1, p0, plane);
}

// more rows: the unit eigenvector of the smallest eigenvalue of the scatter matrix C (xx, xy, xz, yy, yz, zz) through the centroid c
PG_HD bool pl_plane_from_moments(const double* c, const double* C, double* plane) {
#pragma clang fp contract(off)
  if (C[0] == 0.0 && C[1] == 0.0 && C[2] == 0.0 && C[3] == 0.0 && C[4] == 0.0 && C[5] == 0.0) return false;
  double a[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  kn_jacobi(a, v);
  double x = v[0][0], y = v[1][0], z = v[2][0], best = a[0][0];
  if (a[1][1] < best) x = v[0][1], y = v[1][1], z = v[2][1], best = a[1][1];
  if (a[2][2] < best) x = v[0][2], y = v[1][2], z = v[2][2];
  return pl_finish(x, y, z, c, plane);
}

// the plane of m rows in list order (a sample); point(t, p) gives the t-th.  false: not defined.
template <class Point>
PG_HD bool pl_plane_of_rows(int m, Point&& point, double* plane) {
#pragma clang fp contract(off)
  if (m < 3) return false;
  if (m == 3) {
    double p0[3], p1[3], p2[3];
    point(0, p0), point(1, p1), point(2, p2);
    return pl_plane_from_three(p0, p1, p2, plane);
  }
  double s[3] = {0.0, 0.0, 0.0}, p[3], C[6];
  for (int t = 0; t < m; t++) {
    point(t, p);
    s[0] += p[0], s[1] += p[1], s[2] += p[2];
  }
  const double c[3] = {s[0] / (double)m, s[1] / (double)m, s[2] / (double)m};          // (kn_covariance's own mean)
  kn_covariance(m, point, C);
  return pl_plane_from_moments(c, C, plane);
}

// dist = ((a x + b y) + c z) + d, unfused
PG_HD double pl_distance(const double* plane, const double* p) {
#pragma clang fp contract(off)
  const double ax = plane[0] * p[0], by = plane[1] * p[1], cz = plane[2] * p[2];
  const double s = ax + by;
  const double t = s + cz;
  return t + plane[3];
}
// |dist| < threshold, strictly (false for a NaN plane or point)
PG_HD bool pl_inlier(double dist, double thr) { return fabs(dist) < thr; }

// one row of a serial score: the integer count and the error sum in row order
PG_HD void pl_add(double dist, double thr, int* count, double* sum) {
#pragma clang fp contract(off)
  if (!pl_inlier(dist, thr)) return;
  const double dd = dist * dist;
  *count += 1;
  *sum = *sum + dd;
}

// a beats b: more inliers, then the smaller error sum, then the lower hypothesis index
PG_HD bool pl_beats(int ca, double ea, int ha, int cb, double eb, int hb) { return ca > cb || (ca == cb && (ea < eb || (ea == eb && ha < hb))); }

// one cloud's selection
struct PlaneJob {
  const void* points;       // the stacked rows
  int elem;
  int64_t s0, n;            // the cloud's rows
  int rn, H;
  int64_t S;                // its segments, ceil(n / kPlaneSegment)
  double thr;
  const double* hyp;        // [H][4]: the cloud's hypotheses
  const int* part_count;    // [S][H]: (count, error sum) per segment and hypothesis
  const double* part_sum;
  double* seg_sums;         // [S] scratch
  double* plane;            // [4]
  uint8_t* mask;            // [n]: the cloud's rows
  int *count, *status, *best;
  double *fitness, *rmse;
  int* hyp_counts;          // [H] or NULL
  double* hyp_errs;
};

struct PlaneShared {
  double sum[kFsLanes];
  double be[kFsLanes];
  int bc[kFsLanes], bh[kFsLanes];
  int64_t three[3];
};

// the mask of `plane` over the cloud's rows
PG_HD void pl_mask(const PlaneJob& j, const double* plane, int lane_begin, int lane_end) {
  for (int l = lane_begin; l < lane_end; l++)
    for (int64_t i = l; i < j.n; i += kFsLanes) {
      double p[3];
      pg_load3(j.points, j.elem, j.s0 + i, p);
      j.mask[i] = pl_inlier(pl_distance(plane, p), j.thr) ? 1 : 0;
    }
}

// Folds the segment partials in ascending segment order, takes the best hypothesis, refits over its inliers (centroid and scatter through
// fs_sum over the rows in ascending order; exactly 3 inliers: their cross product), and recomputes mask, count, fitness and rmse against
// the refit plane (the winner's own where the refit is not defined).  The caller owns lanes [lane_begin, lane_end) of kFsLanes.
template <class Barrier>
PG_HD void pl_select(const PlaneJob& j, int lane_begin, int lane_end, PlaneShared* sh, Barrier&& barrier) {
#pragma clang fp contract(off)
  for (int l = lane_begin; l < lane_end; l++) {
    int bc = -1, bh = 0;
    double be = 0.0;
    for (int h = l; h < j.H; h += kFsLanes) {
      int c = 0;
      double e = 0.0;
      for (int64_t s = 0; s < j.S; s++) c += j.part_count[s * j.H + h], e = e + j.part_sum[s * j.H + h];
      if (j.hyp_counts) j.hyp_counts[h] = c, j.hyp_errs[h] = e;
      if (pl_beats(c, e, h, bc, be, bh)) bc = c, be = e, bh = h;
    }
    sh->bc[l] = bc, sh->be[l] = be, sh->bh[l] = bh;
  }
  barrier();
  int bc = -1, bh = 0;
  double be = 0.0;
  for (int l = 0; l < kFsLanes; l++)
    if (pl_beats(sh->bc[l], sh->be[l], sh->bh[l], bc, be, bh)) bc = sh->bc[l], be = sh->be[l], bh = sh->bh[l];
  barrier();
  if (j.n < j.rn || bc < 3) {
    for (int l = lane_begin; l < lane_end; l++)
      for (int64_t i = l; i < j.n; i += kFsLanes) j.mask[i] = 0;
    if (lane_begin == 0) {
      j.plane[0] = j.plane[1] = j.plane[2] = j.plane[3] = 0.0;
      *j.count = 0, *j.fitness = 0.0, *j.rmse = 0.0, *j.best = -1;
      *j.status = j.n < j.rn ? kPlaneTooFew : kPlaneNone;
    }
    return;
  }
  double win[4], fit[4];
  for (int k = 0; k < 4; k++) win[k] = fit[k] = j.hyp[4 * (int64_t)bh + k];
  pl_mask(j, win, lane_begin, lane_end);
  barrier();
  bool refit;
  if (bc == 3) {
    if (lane_begin == 0) {
      int found = 0;
      for (int64_t i = 0; i < j.n && found < 3; i++)
        if (j.mask[i]) sh->three[found++] = i;
    }
    barrier();
    double p0[3], p1[3], p2[3];
    pg_load3(j.points, j.elem, j.s0 + sh->three[0], p0);
    pg_load3(j.points, j.elem, j.s0 + sh->three[1], p1);
    pg_load3(j.points, j.elem, j.s0 + sh->three[2], p2);
    refit = pl_plane_from_three(p0, p1, p2, fit);
    barrier();
  } else {
    double c[3], C[6];
    for (int d = 0; d < 3; d++) {
      const double s = fs_sum(
          j.n, lane_begin, lane_end, [&](int64_t i, double acc) { return j.mask[i] ? acc + pg_load(j.points, j.elem, 3 * (j.s0 + i) + d) : acc; },
          sh->sum, barrier);
      c[d] = s / (double)bc;
    }
    int e = 0;
    for (int a = 0; a < 3; a++)
      for (int b = a; b < 3; b++, e++) {
        const double s = fs_sum(
            j.n, lane_begin, lane_end,
            [&](int64_t i, double acc) {
              if (!j.mask[i]) return acc;
              const double da = pg_load(j.points, j.elem, 3 * (j.s0 + i) + a) - c[a], db = pg_load(j.points, j.elem, 3 * (j.s0 + i) + b) - c[b];
              const double prod = da * db;
              return acc + prod;
            },
            sh->sum, barrier);
        C[e] = s / (double)bc;
      }
    refit = pl_plane_from_moments(c, C, fit);
  }
  if (!refit)
    for (int k = 0; k < 4; k++) fit[k] = win[k];
  barrier();                                                            // (every lane has read the winner's mask)
  pl_mask(j, fit, lane_begin, lane_end);
  barrier();
  const double counted = fs_sum(j.n, lane_begin, lane_end, [&](int64_t i, double acc) { return j.mask[i] ? acc + 1.0 : acc; }, sh->sum, barrier);
  for (int l = lane_begin; l < lane_end; l++)
    for (int64_t s = l; s < j.S; s += kFsLanes) {
      const int64_t end = (s + 1) * kPlaneSegment < j.n ? (s + 1) * kPlaneSegment : j.n;
      int c = 0;
      double e = 0.0, p[3];
      for (int64_t i = s * kPlaneSegment; i < end; i++) {
        pg_load3(j.points, j.elem, j.s0 + i, p);
        pl_add(pl_distance(fit, p), j.thr, &c, &e);
      }
      j.seg_sums[s] = e;
    }
  barrier();
  if (lane_begin != 0) return;
  double err = 0.0;
  for (int64_t s = 0; s < j.S; s++) err = err + j.seg_sums[s];
  const int count = (int)counted;
  for (int k = 0; k < 4; k++) j.plane[k] = fit[k];
  *j.count = count, *j.best = bh, *j.status = kPlaneOk;
  *j.fitness = (double)count / (double)j.n;
  *j.rmse = count > 0 ? pg_sqrt(err / (double)count) : 0.0;
}
