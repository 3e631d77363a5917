// A sum over the rows of one cloud in a fixed shape, the same text for one workgroup of kFsLanes threads and for a serial host caller (the
// shape of icp_sum, csrc/icp_core.h): lane l adds rows l, l + kFsLanes, l + 2 kFsLanes, .. in ascending order into its own accumulator
// (starting from 0.0); the kFsLanes accumulators are then folded in halves, sh[l] = sh[l] + sh[l + o] for o = kFsLanes / 2, .., 1; the sum
// is sh[0].  The result depends on the cloud's rows alone: not on the batch, the run, or the device.  csrc/outliers.hip uses it.
#pragma once
#include <stdint.h>

#include "stack_rows.h"         // PG_HD

constexpr int kFsLanes = 256;

// term(i, acc) returns acc with row i's term added (or acc itself for a row that contributes nothing).  The caller owns lanes
// [lane_begin, lane_end); sh holds kFsLanes values and is free again on return.  Every caller's lane gets the sum.
template <class Term, class Barrier>
PG_HD double fs_sum(int64_t n, int lane_begin, int lane_end, Term&& term, double* sh, Barrier&& barrier) {
#pragma clang fp contract(off)
  for (int l = lane_begin; l < lane_end; l++) {
    double acc = 0.0;
    for (int64_t i = l; i < n; i += kFsLanes) acc = term(i, acc);
    sh[l] = acc;
  }
  barrier();
  for (int o = kFsLanes / 2; o > 0; o >>= 1) {
    for (int l = lane_begin; l < lane_end; l++)
      if (l < o) sh[l] = sh[l] + sh[l + o];
    barrier();
  }
  const double out = sh[0];
  barrier();
  return out;
}
