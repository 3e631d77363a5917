// The arithmetic of the FPFH descriptor (csrc/fpfh.hip): the pair feature, its three bins, the SPFH value and the FPFH value, as
// __host__ __device__ text that the kernels and se3_debug_fpfh_host both run, on PG_HD, pg_sqrt and pg_dist2 of pair_grid.h.
// Everything is float64 with contraction off; the only libm call is the square root inside pg_sqrt.  The contract is the header comment
// of csrc/fpfh.hip.
#pragma once
#include "pair_grid.h"

constexpr int kFpfhBins = 11;                 // bins per feature
constexpr int kFpfhDim = 3 * kFpfhBins;       // a row: theta at 0-10, f1 at 11-21, f2 at 22-32

// (cos, sin) of beta_k = -pi + 2 pi k / 11, k = 1 .. 10: the ONE table of the sector rule (tests/fpfh_twin.py holds the same literals)
PG_HD void fpfh_sector(int k, double* c, double* s) {
  const double table[10][2] = {{-0.8412535328311812, -0.5406408174555976}, {-0.41541501300188644, -0.9096319953545183},
                               {0.14231483827328514, -0.9898214418809327}, {0.6548607339452851, -0.7557495743542583},
                               {0.9594929736144974, -0.28173255684142967}, {0.9594929736144974, 0.28173255684142967},
                               {0.6548607339452851, 0.7557495743542583},   {0.14231483827328514, 0.9898214418809327},
                               {-0.41541501300188644, 0.9096319953545183}, {-0.8412535328311812, 0.5406408174555976}};
  *c = table[k - 1][0], *s = table[k - 1][1];
}

// (a b + c d) + e f
PG_HD double fpfh_dot(const double* a, const double* b) {
#pragma clang fp contract(off)
  const double x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
  const double s = x + y;
  return s + z;
}

// a x b, every product rounded on its own
PG_HD void fpfh_cross(const double* a, const double* b, double* out) {
#pragma clang fp contract(off)
  const double yz = a[1] * b[2], zy = a[2] * b[1], zx = a[2] * b[0], xz = a[0] * b[2], xy = a[0] * b[1], yx = a[1] * b[0];
  out[0] = yz - zy, out[1] = zx - xz, out[2] = xy - yx;
}

// The pair feature of (p1, n1) and (p2, n2): f = (f1, f2, x, y), theta = atan2(y, x).  A degenerate pair (d == 0, or dp parallel to the
// first normal) gives four zeros.  The normals are used as given.
PG_HD void fpfh_pair_feature(const double* p1, const double* n1, const double* p2, const double* n2, double* f) {
#pragma clang fp contract(off)
  f[0] = 0.0, f[1] = 0.0, f[2] = 0.0, f[3] = 0.0;
  double dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  const double d = pg_sqrt(fpfh_dot(dp, dp));
  if (d == 0.0) return;
  const double a1 = fpfh_dot(n1, dp) / d, a2 = fpfh_dot(n2, dp) / d;
  const bool swap = fabs(a1) < fabs(a2);
  double na[3], nb[3];
  for (int k = 0; k < 3; k++) {
    na[k] = swap ? n2[k] : n1[k];
    nb[k] = swap ? n1[k] : n2[k];
    dp[k] = swap ? -dp[k] : dp[k];
  }
  const double f2 = swap ? -a2 : a1;
  double v[3], w[3];
  fpfh_cross(dp, na, v);
  const double len = pg_sqrt(fpfh_dot(v, v));
  if (len == 0.0) return;
  v[0] = v[0] / len, v[1] = v[1] / len, v[2] = v[2] / len;
  fpfh_cross(na, v, w);
  f[0] = fpfh_dot(v, nb);
  f[1] = f2;
  f[2] = fpfh_dot(na, nb);
  f[3] = fpfh_dot(w, nb) + 0.0;                                            // (-0.0 becomes 0.0: theta = pi, not -pi)
}

// clamp(floor(11 (f + 1) 0.5), 0, 10); a NaN gives 0
PG_HD int fpfh_linear_bin(double f) {
#pragma clang fp contract(off)
  const double t = f + 1.0;
  const double u = 11.0 * t;
  const double b = floor(u * 0.5);
  if (!(b >= 0.0)) return 0;
  return b > 10.0 ? 10 : (int)b;
}

// the bin of theta = atan2(y, x) in 11 sectors of [-pi, pi], without the angle: the number of sector edges beta_k at or below theta
PG_HD int fpfh_theta_bin(double x, double y) {
#pragma clang fp contract(off)
  if (x == 0.0 && y == 0.0) return 5;
  const bool low = y < 0.0;
  int bin = low ? 0 : 5;
#pragma unroll
  for (int u = 0; u < 5; u++) {                                            // k = 1 + u below the x axis, 6 + u above (constant indices)
    double c_lo, s_lo, c_hi, s_hi;
    fpfh_sector(1 + u, &c_lo, &s_lo);
    fpfh_sector(6 + u, &c_hi, &s_hi);
    const double c = low ? c_lo : c_hi, s = low ? s_lo : s_hi;
    const double cy = c * y, sx = s * x;
    bin += cy - sx >= 0.0 ? 1 : 0;
  }
  return bin;
}

// bins[0] = theta, bins[1] = f1, bins[2] = f2 of one pair; (5, 5, 5) for a degenerate pair
PG_HD void fpfh_pair_bins(const double* p1, const double* n1, const double* p2, const double* n2, int* bins) {
  double f[4];
  fpfh_pair_feature(p1, n1, p2, n2, f);
  bins[0] = fpfh_theta_bin(f[2], f[3]);
  bins[1] = fpfh_linear_bin(f[0]);
  bins[2] = fpfh_linear_bin(f[1]);
}

// count (100 / m); 0 for a row without neighbours
PG_HD double fpfh_spfh_value(int count, int m) {
#pragma clang fp contract(off)
  if (m <= 0) return 0.0;
  const double scale = 100.0 / (double)m;
  return (double)count * scale;
}

// one term of A_j = sum_k spfh(j, k) / d2_k (the caller skips d2 == 0 and keeps the list order)
PG_HD double fpfh_weighted_add(double acc, double spfh, double d2) {
#pragma clang fp contract(off)
  const double q = spfh / d2;
  return acc + q;
}

// F_j = spfh(j, i) + (S_g != 0 ? A_j (100 / S_g) : A_j)
PG_HD double fpfh_value(double own, double a, double group_sum) {
#pragma clang fp contract(off)
  if (group_sum == 0.0) return own + a;
  const double scale = 100.0 / group_sum;
  const double t = a * scale;
  return own + t;
}
