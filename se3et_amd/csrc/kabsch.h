// Float64 3x3 Kabsch solve shared by the registration kernels (csrc/registration.hip: weighted Procrustes; csrc/ransac.hip: RANSAC
// hypotheses; csrc/icp.hip: the point-to-point update): a cyclic Jacobi eigen-solve of H^T H, the left singular vectors from H v, the
// reflection fix by cross products.
// The text is __host__ __device__ and takes its square root from `Math`: KabschLibm is the plain sqrt of the two registration kernels
// (their arithmetic is what it was); icp.hip passes a root that rounds alike on the host and on the device, and asks for a float64 T.
#pragma once
#include <math.h>

#include "common.h"

namespace {

struct KabschLibm {
  static __host__ __device__ __forceinline__ double root(double x) { return sqrt(x); }
};

template <class Math>
__host__ __device__ void jacobi_eig3(double A[3][3], double V[3][3]) {     // symmetric A -> eigenvalues on the diagonal, vectors in V columns
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; sweep++) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (off <= 1e-40 + 1e-32 * diag) break;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        if (fabs(A[p][q]) < 1e-300) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + Math::root(theta * theta + 1.0));
        const double c = 1.0 / Math::root(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; k++) {          // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; k++) {          // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; k++) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

// R = V diag(1, 1, det(V U^T)) U^T for H = U S V^T; t = rc - R sc; writes a row-major 4x4
template <class Math = KabschLibm, class Out = float>
__host__ __device__ void kabsch(const double H_in[3][3], const double sc[3], const double rc[3], Out* __restrict__ T) {
  // R depends only on the direction of H: scale it by an exact power of two so that max |H| lies in [0.5, 1).  The solve's floors
  // below (1e-40, 1e-300) are then relative to H, and R is the same for a problem scaled by 2^k.  A zero H stays zero (identity);
  // NaN entries are skipped by fmax and still reach R; an infinite H is left as it is.
  double mx = 0.0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) mx = fmax(mx, fabs(H_in[i][j]));
  int e = 0;
  if (mx > 0.0 && isfinite(mx)) frexp(mx, &e);
  double H[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) H[i][j] = ldexp(H_in[i][j], -e);
  double A[3][3], V[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) A[i][j] = H[0][i] * H[0][j] + H[1][i] * H[1][j] + H[2][i] * H[2][j];   // H^T H
  jacobi_eig3<Math>(A, V);
  int o[3] = {0, 1, 2};                                   // eigenvalues in descending order
  for (int i = 0; i < 2; i++)
    for (int j = i + 1; j < 3; j++)
      if (A[o[j]][o[j]] > A[o[i]][o[i]]) { int t = o[i]; o[i] = o[j]; o[j] = t; }
  double v[3][3], u[3][3];                                // v[k], u[k]: k-th right / left singular vector
  for (int k = 0; k < 3; k++)
    for (int i = 0; i < 3; i++) v[k][i] = V[i][o[k]];
  for (int k = 0; k < 2; k++) {
    double n2 = 0;
    for (int i = 0; i < 3; i++) {
      u[k][i] = H[i][0] * v[k][0] + H[i][1] * v[k][1] + H[i][2] * v[k][2];
      n2 += u[k][i] * u[k][i];
    }
    if (k == 1) {                                         // re-orthogonalise against u0 (near-degenerate second value)
      const double d = u[1][0] * u[0][0] + u[1][1] * u[0][1] + u[1][2] * u[0][2];
      n2 = 0;
      for (int i = 0; i < 3; i++) { u[1][i] -= d * u[0][i]; n2 += u[1][i] * u[1][i]; }
    }
    const double inv = n2 > 1e-300 ? 1.0 / Math::root(n2) : 0.0;
    for (int i = 0; i < 3; i++) u[k][i] *= inv;
    if (n2 <= 1e-300) {                                   // rank < k+1: any unit vector orthogonal to the previous ones
      const double* b = u[0];
      double e[3] = {fabs(b[0]) < 0.9 ? 1.0 : 0.0, fabs(b[0]) < 0.9 ? 0.0 : 1.0, 0.0};
      if (k == 0) { u[0][0] = 1; u[0][1] = 0; u[0][2] = 0; }
      else {
        const double d = e[0] * b[0] + e[1] * b[1] + e[2] * b[2];
        double m2 = 0;
        for (int i = 0; i < 3; i++) { u[1][i] = e[i] - d * b[i]; m2 += u[1][i] * u[1][i]; }
        for (int i = 0; i < 3; i++) u[1][i] /= Math::root(m2);
      }
    }
  }
  // third vectors by cross products: det([u0 u1 u2]) = det([v0 v1 v2']) = +1 with v2' = v0 x v1, i.e. the reflection fix
  // diag(1, 1, det(V U^T)) is already applied
  u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
  u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
  u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
  double w2[3] = {v[0][1] * v[1][2] - v[0][2] * v[1][1], v[0][2] * v[1][0] - v[0][0] * v[1][2],
                  v[0][0] * v[1][1] - v[0][1] * v[1][0]};
  double R[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[i][j] = v[0][i] * u[0][j] + v[1][i] * u[1][j] + w2[i] * u[2][j];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T[4 * i + j] = (Out)R[i][j];
    T[4 * i + 3] = (Out)(rc[i] - (R[i][0] * sc[0] + R[i][1] * sc[1] + R[i][2] * sc[2]));
  }
  T[12] = (Out)0; T[13] = (Out)0; T[14] = (Out)0; T[15] = (Out)1;
}

}  // namespace
