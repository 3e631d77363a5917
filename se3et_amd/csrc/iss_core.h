// The arithmetic of the ISS keypoint detector (csrc/iss.hip carries the contract): the saliency of a row from its scatter matrix, and the
// selection test of a row over the grid.  __host__ __device__ text that the kernels and se3_debug_iss_host both run, on csrc/cov3.h
// (kn_covariance, kn_eigenvalues) and the ball walk of csrc/pair_grid.h.
#pragma once
#include <math.h>

#include "cov3.h"
#include "pair_grid.h"

// s = l3 when m >= min_neighbors, C != 0, l2 / l1 < gamma_21, l3 / l2 < gamma_32 and l3 > 0; otherwise 0.  True divisions; a comparison
// with NaN is false.  C: the scatter matrix of the row's m members (kn_covariance).
PG_HD double iss_saliency(int m, const double* C, double gamma_21, double gamma_32, int min_neighbors) {
#pragma clang fp contract(off)
  if (m < 1 || m < min_neighbors) return 0.0;
  if (C[0] == 0.0 && C[1] == 0.0 && C[2] == 0.0 && C[3] == 0.0 && C[4] == 0.0 && C[5] == 0.0) return 0.0;
  double l[3];
  kn_eigenvalues(C, l);
  const double r21 = l[1] / l[0], r32 = l[2] / l[1];
  return (r21 < gamma_21 && r32 < gamma_32 && l[2] > 0.0) ? l[2] : 0.0;
}

// Row i (point q, saliency si) is a keypoint iff si > 0, its non_max_radius ball holds at least min_neighbors members, and none of them
// has a larger saliency (equal saliencies keep both).  sal: the cloud's saliencies by cloud-local index.  Count and maximum are order-free:
// the walk's cell order does not matter.
PG_HD bool iss_is_keypoint(const PairGridView& g, int p, const double* q, double r, double r2, const double* sal, double si, int min_neighbors) {
  if (!(si > 0.0)) return false;
  int64_t members = 0;
  bool beaten = false;
  pg_ball_walk(g, p, q, r, r2, [&](int j) {
    members++;
    if (sal[j] > si) beaten = true;
  });
  return members >= (int64_t)min_neighbors && !beaten;
}
