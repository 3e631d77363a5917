// The arithmetic of the statistical outlier filter and of the model resolution (csrc/outliers.hip carries the contract): a row's distance
// from its k-NN list, the cloud statistics in the fixed shape of csrc/fixed_sum.h, the mask test.  __host__ __device__ text that the
// kernels and the se3_debug_*_host entries both run.
#pragma once
#include <math.h>

#include "fixed_sum.h"
#include "pair_grid.h"

constexpr int kOdStats = 4;             // per cloud: mean, std, thr, model resolution

// a row's value from the cnt entries of its k-NN list; root(t) = pg_sqrt(d2_t).  column < 0: (the sequential sum of the roots in list
// order) / cnt; column >= 0: the root of that column, 0 where the list is shorter
template <class Root>
PG_HD double od_row_distance(int cnt, int column, Root&& root) {
#pragma clang fp contract(off)
  if (column >= 0) return column < cnt ? root(column) : 0.0;
  double s = 0.0;
  for (int t = 0; t < cnt; t++) s += root(t);
  return s / (double)cnt;
}

// out[0] = mean = (sum of a_i over rows with a_i > 0) / n; out[1] = std = pg_sqrt((sum over the same rows of (a_i - mean)^2) / (n - 1));
// out[2] = thr = mean + std_ratio std; out[3] = the model resolution: mean when n >= 2, else 0.  Both sums are fs_sum's.
template <class Barrier>
PG_HD void od_cloud_stats(const double* a, int64_t n, double std_ratio, int lane_begin, int lane_end, double* sh, Barrier&& barrier,
                          double* out) {
#pragma clang fp contract(off)
  const double s1 = fs_sum(n, lane_begin, lane_end, [&](int64_t i, double acc) { return a[i] > 0.0 ? acc + a[i] : acc; }, sh, barrier);
  const double mean = s1 / (double)n;
  const double s2 = fs_sum(
      n, lane_begin, lane_end,
      [&](int64_t i, double acc) {
        if (!(a[i] > 0.0)) return acc;
        const double d = a[i] - mean;
        const double dd = d * d;
        return acc + dd;
      },
      sh, barrier);
  const double var = s2 / (double)(n - 1);
  const double sd = pg_sqrt(var);
  const double scaled = std_ratio * sd;
  out[0] = mean, out[1] = sd, out[2] = mean + scaled, out[3] = n >= 2 ? mean : 0.0;
}

// kept iff a_i > 0 and a_i < thr (a comparison with NaN is false)
PG_HD bool od_kept(double a, double thr) { return a > 0.0 && a < thr; }
