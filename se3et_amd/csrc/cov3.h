// The 3x3 scatter matrix of a point list and its eigen-decomposition, once: csrc/knn_normals.hip (the normal of a k-NN list) and csrc/iss.hip
// (the eigenvalues of a ball's members) run this one text, and the se3_debug_*_host entries of both run it on host memory.
// __host__ __device__, float64, contraction off in every function; no libm call other than the square root (pg_sqrt) and division.
//   kn_covariance    mean and covariance of m points in list order, two passes, every sum sequential in list order.
//   kn_rotate        one Jacobi rotation.            kn_jacobi       the cyclic sweeps: (0,1), (0,2), (1,2), kJacobiSweeps times.
//   kn_eigenvalues   the eigenvalues of C from kn_jacobi, sorted l[0] >= l[1] >= l[2].
#pragma once
#include <math.h>

#include "pair_grid.h"          // PG_HD, pg_sqrt

constexpr int kJacobiSweeps = 10;     // (a 3x3 matrix is diagonal to rounding after 5 or 6)

// mean and covariance of m points in list order; point(t, p) gives the t-th.  C: xx, xy, xz, yy, yz, zz.
template <class Point>
PG_HD void kn_covariance(int m, Point&& point, double* C) {
#pragma clang fp contract(off)
  double s[3] = {0.0, 0.0, 0.0}, p[3];
  for (int t = 0; t < m; t++) {
    point(t, p);
    s[0] += p[0], s[1] += p[1], s[2] += p[2];
  }
  const double mx = s[0] / (double)m, my = s[1] / (double)m, mz = s[2] / (double)m;
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int t = 0; t < m; t++) {
    point(t, p);
    const double dx = p[0] - mx, dy = p[1] - my, dz = p[2] - mz;
    const double xx = dx * dx, xy = dx * dy, xz = dx * dz, yy = dy * dy, yz = dy * dz, zz = dz * dz;
    a[0] += xx, a[1] += xy, a[2] += xz, a[3] += yy, a[4] += yz, a[5] += zz;
  }
  for (int e = 0; e < 6; e++) C[e] = a[e] / (double)m;
}

// one Jacobi rotation that annihilates a[P][Q]; R is the third index
template <int P, int Q, int R>
PG_HD void kn_rotate(double (&a)[3][3], double (&v)[3][3]) {
#pragma clang fp contract(off)
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double den = 2.0 * apq;
  const double theta = (a[Q][Q] - a[P][P]) / den;
  const double tt = theta * theta;
  const double root = pg_sqrt(tt + 1.0);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + root);          // (an overflowing theta gives t = 0: nothing to rotate)
  const double t2 = t * t;
  const double c = 1.0 / pg_sqrt(t2 + 1.0);
  const double s = t * c;
  const double shift = t * apq;
  a[P][P] = a[P][P] - shift;
  a[Q][Q] = a[Q][Q] + shift;
  a[P][Q] = a[Q][P] = 0.0;
  const double arp = a[R][P], arq = a[R][Q];
  const double u0 = c * arp, u1 = s * arq, w0 = s * arp, w1 = c * arq;
  a[R][P] = a[P][R] = u0 - u1;
  a[R][Q] = a[Q][R] = w0 + w1;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double vp = v[k][P], vq = v[k][Q];
    const double x0 = c * vp, x1 = s * vq, y0 = s * vp, y1 = c * vq;
    v[k][P] = x0 - x1;
    v[k][Q] = y0 + y1;
  }
}

// the cyclic sweeps: a becomes diagonal to rounding, the columns of v its eigenvectors
PG_HD void kn_jacobi(double (&a)[3][3], double (&v)[3][3]) {
  for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
    kn_rotate<0, 1, 2>(a, v);
    kn_rotate<0, 2, 1>(a, v);
    kn_rotate<1, 2, 0>(a, v);
  }
}

// the eigenvalues of the symmetric C (xx, xy, xz, yy, yz, zz), l[0] >= l[1] >= l[2]
PG_HD void kn_eigenvalues(const double* C, double* l) {
  double a[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  kn_jacobi(a, v);
  double x = a[0][0], y = a[1][1], z = a[2][2], t;
  if (x < y) t = x, x = y, y = t;
  if (y < z) t = y, y = z, z = t;
  if (x < y) t = x, x = y, y = t;
  l[0] = x, l[1] = y, l[2] = z;
}
