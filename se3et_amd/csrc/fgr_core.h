// Fast Global Registration of csrc/fgr.hip as __host__ __device__ text: one pair's checks and normalisation (fgr_pair_normalize), one
// chunk of its tuple test (fgr_tuple_chunk) and its graduated-non-convexity loop with the way back to the original scale
// (fgr_pair_optimize).  The kernels run it with one workgroup of kFgrLanes threads per pair (each thread one lane, `barrier` =
// __syncthreads); se3_debug_fgr_host runs the same text serially over all lanes with a no-op barrier.  The ordered sum, the 6x6 solve, the
// composition, the update matrix and the sine and cosine series are those of icp_core.h; the sampler is splitmix.h's.  The contract is the
// header comment of fgr.hip.
#pragma once
#include "icp_core.h"
#include "splitmix.h"

constexpr int kFgrLanes = kIcpLanes;                  // the lanes of icp_sum: 256
constexpr int kFgrSums = kIcpGeneralSums;             // 21 terms of sum w J J^T and 6 of sum w J d
constexpr int kFgrChunk = SE3_FGR_TUPLE_CHUNK;        // trials per step of the tuple test: one per lane
constexpr double kFgrMaxAngle = SE3_FGR_MAX_ANGLE;     // rad
constexpr int kFgrMinCorrespondences = 10;
constexpr int64_t kFgrTrialsPerCorrespondence = 100;
static_assert(kFgrChunk == kFgrLanes, "the tuple test runs one trial per lane");

struct FgrParams {
  double maxdist, division_factor, tau2;              // tau2 = tuple_scale * tuple_scale, rounded once
  int use_absolute_scale, decrease_mu, iteration_number, tuple_test, cap;
  uint64_t key;                                       // splitmix64(seed)
};

// one pair's rows and results; every pointer already points at the pair's first entry
struct FgrPair {
  const void* src;          // (ns, 3), src_elem
  int src_elem;
  int64_t ns;
  const void* ref;          // (nr, 3), ref_elem
  int ref_elem;
  int64_t nr;
  const int64_t* corr;      // (K, 2): (src row, ref row)
  int64_t K;
  int64_t* tuples;          // (3 cap, 2): C' of the tuple test; not read without it
  int64_t* trials;          // (cap) or null: the accepted trials
  double* norm;             // 7: the source's mean, the reference's mean, scale
  double* T;                // (4, 4)
  int* status;
  int* ncorr;               // |C'|
  int* ntuples;             // accepted trials that were kept
  double* mu;               // or null: mu at the end
};

// the largest of what value(i) gives over rows 0 .. n - 1 (0 for none; the values are finite and >= 0), in every caller's lane: the
// lanes of icp_sum and its tree.  A maximum does not depend on the order; the form is shared so that host and device run one text.
template <class Value, class Barrier>
PG_HD double fgr_max(int64_t n, int lane_begin, int lane_end, Value&& value, double* sh, Barrier&& barrier) {
  for (int l = lane_begin; l < lane_end; l++) {
    double m = 0.0;
    for (int64_t i = l; i < n; i += kFgrLanes) {
      const double x = value(i);
      m = x > m ? x : m;
    }
    sh[l] = m;
  }
  barrier();
  for (int o = kFgrLanes / 2; o > 0; o >>= 1) {
    for (int l = lane_begin; l < lane_end; l++)
      if (l < o) sh[l] = sh[l + o] > sh[l] ? sh[l + o] : sh[l];
    barrier();
  }
  const double out = sh[0];
  barrier();
  return out;
}

// 0 and 3: the refusals and the normalisation's figures.  Writes norm, status, and |C'| where the tuple test will not: K without the
// test, 0 for a pair that stops here.  One of NONFINITE, EMPTY, BAD_INDEX at the most, in that order: an empty cloud has no index to be
// wrong about.
template <class Barrier>
PG_HD void fgr_pair_normalize(const FgrPair& v, const FgrParams& prm, int lane_begin, int lane_end, double* sh, Barrier&& barrier) {
#pragma clang fp contract(off)
  double bad_s[1], bad_r[1];
  icp_sum<1>(v.ns, lane_begin, lane_end, [&](int64_t i, double* acc) { acc[0] += icp_finite3(v.src, v.src_elem, i) ? 0.0 : 1.0; }, sh, barrier,
             bad_s);
  icp_sum<1>(v.nr, lane_begin, lane_end, [&](int64_t i, double* acc) { acc[0] += icp_finite3(v.ref, v.ref_elem, i) ? 0.0 : 1.0; }, sh, barrier,
             bad_r);
  int status = 0;
  if (bad_s[0] + bad_r[0] > 0.0) {
    status = SE3_FGR_NONFINITE;
  } else if (v.ns == 0 || v.nr == 0 || v.K == 0) {
    status = SE3_FGR_EMPTY;
  } else {
    double bad_c[1];
    icp_sum<1>(v.K, lane_begin, lane_end,
               [&](int64_t i, double* acc) {
                 const int64_t s = v.corr[2 * i], r = v.corr[2 * i + 1];
                 acc[0] += (s < 0 || s >= v.ns || r < 0 || r >= v.nr) ? 1.0 : 0.0;
               },
               sh, barrier, bad_c);
    if (bad_c[0] > 0.0) status = SE3_FGR_BAD_INDEX;
  }
  double nm[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (status == 0) {
    double ss[3], sr[3];
    icp_sum<3>(v.ns, lane_begin, lane_end,
               [&](int64_t i, double* acc) {
                 for (int a = 0; a < 3; a++) acc[a] += pg_load(v.src, v.src_elem, 3 * i + a);
               },
               sh, barrier, ss);
    icp_sum<3>(v.nr, lane_begin, lane_end,
               [&](int64_t i, double* acc) {
                 for (int a = 0; a < 3; a++) acc[a] += pg_load(v.ref, v.ref_elem, 3 * i + a);
               },
               sh, barrier, sr);
    for (int a = 0; a < 3; a++) nm[a] = ss[a] / (double)v.ns, nm[3 + a] = sr[a] / (double)v.nr;
    auto norm2 = [&](const void* pts, int elem, const double* mean, int64_t i) {
      const double dx = pg_load(pts, elem, 3 * i) - mean[0], dy = pg_load(pts, elem, 3 * i + 1) - mean[1],
                   dz = pg_load(pts, elem, 3 * i + 2) - mean[2];
      const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
      return (xx + yy) + zz;
    };
    const double ms = fgr_max(v.ns, lane_begin, lane_end, [&](int64_t i) { return norm2(v.src, v.src_elem, nm, i); }, sh, barrier);
    const double mr = fgr_max(v.nr, lane_begin, lane_end, [&](int64_t i) { return norm2(v.ref, v.ref_elem, nm + 3, i); }, sh, barrier);
    nm[6] = pg_sqrt(ms > mr ? ms : mr);
  }
  if (lane_begin == 0) {
    for (int k = 0; k < 7; k++) v.norm[k] = nm[k];
    *v.status = status;
    *v.ncorr = (status != 0 || prm.tuple_test) ? 0 : (int)v.K;
    *v.ntuples = 0;
  }
}

// the squared edge between rows i and j of a cloud: (dx dx + dy dy) + dz dz
PG_HD double fgr_edge2(const void* pts, int elem, int64_t i, int64_t j) {
#pragma clang fp contract(off)
  const double dx = pg_load(pts, elem, 3 * i) - pg_load(pts, elem, 3 * j), dy = pg_load(pts, elem, 3 * i + 1) - pg_load(pts, elem, 3 * j + 1),
               dz = pg_load(pts, elem, 3 * i + 2) - pg_load(pts, elem, 3 * j + 2);
  const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  return (xx + yy) + zz;
}

// 1: trial t draws a[0..2] and is accepted iff every edge (0, 1), (1, 2), (2, 0) has ls tau2 < lr and lr tau2 < ls
PG_HD bool fgr_tuple_trial(const FgrPair& v, uint64_t key, double tau2, int64_t t, int64_t* a) {
#pragma clang fp contract(off)
  for (int j = 0; j < 3; j++) a[j] = splitmix_draw(key, (uint64_t)t, 3, (uint64_t)j, (uint64_t)v.K);
  bool ok = true;
  for (int e = 0; e < 3; e++) {
    const int64_t i = a[e], j = a[(e + 1) % 3];
    const double ls = fgr_edge2(v.src, v.src_elem, v.corr[2 * i], v.corr[2 * j]);
    const double lr = fgr_edge2(v.ref, v.ref_elem, v.corr[2 * i + 1], v.corr[2 * j + 1]);
    const double a_ = ls * tau2, b_ = lr * tau2;
    ok = ok && a_ < lr && b_ < ls;
  }
  return ok;
}

// One chunk of the tuple test: lane l runs trial base + l.  rank(accepted) gives the number of accepted trials of the chunk's lower
// lanes (the device: a block scan, called once by every thread; the host: a running count); `total` is the number accepted before the
// chunk.  An accepted trial of rank r < cap writes rows 3 r .. 3 r + 2 of C' and its index: the first cap accepted trials in trial order.
template <class Rank>
PG_HD void fgr_tuple_chunk(const FgrPair& v, const FgrParams& prm, int64_t base, int64_t trials, int total, int lane_begin, int lane_end,
                           Rank&& rank) {
  for (int l = lane_begin; l < lane_end; l++) {
    const int64_t t = base + l;
    int64_t a[3] = {0, 0, 0};
    const bool ok = t < trials && fgr_tuple_trial(v, prm.key, prm.tau2, t, a);
    const int64_t r = (int64_t)total + rank(ok);
    if (ok && r < prm.cap) {
      for (int j = 0; j < 3; j++) v.tuples[2 * (3 * r + j)] = v.corr[2 * a[j]], v.tuples[2 * (3 * r + j) + 1] = v.corr[2 * a[j] + 1];
      if (v.trials) v.trials[r] = t;
    }
  }
}

// sin and cos of an angle of (-4, 4): the series of icp_core.h at a / 4, then two double-angle steps, every operation rounded on its own
PG_HD void fgr_sincos(double a, double* s, double* c) {
#pragma clang fp contract(off)
  const double h = a / 4.0;
  double s1 = icp_sin(h), c1 = icp_cos(h);
  for (int k = 0; k < 2; k++) {
    const double t = 2.0 * s1;
    const double sn = t * c1;
    const double cc = c1 * c1, ss = s1 * s1;
    c1 = cc - ss;
    s1 = sn;
  }
  *s = s1, *c = c1;
}

// the place of entry (i, j), i <= j, in the upper triangle stored row by row
PG_HD constexpr int fgr_tri(int i, int j) { return i * (11 - i) / 2 + j; }

// 2, 4 and 5: the count, the loop from M = I, the original scale and the inverse.  Uniform over the lanes: every lane forms the same sums
// and solves the same systems; lane 0 writes.
template <class Barrier>
PG_HD void fgr_pair_optimize(const FgrPair& v, const FgrParams& prm, int lane_begin, int lane_end, double* sh, Barrier&& barrier) {
#pragma clang fp contract(off)
  int status = *v.status;
  const int64_t n = *v.ncorr;
  double nm[7];
  for (int k = 0; k < 7; k++) nm[k] = v.norm[k];
  barrier();                                                             // (every lane has read the state lane 0 writes below)
  const bool refused = (status & (SE3_FGR_NONFINITE | SE3_FGR_BAD_INDEX)) != 0;
  bool identity = (status & SE3_FGR_EMPTY) != 0;
  if (!refused && !identity && n < kFgrMinCorrespondences) status |= SE3_FGR_TOO_FEW, identity = true;
  const double scale = nm[6];
  if (!refused && !identity && !(scale > 0.0)) status |= SE3_FGR_SINGULAR, identity = true;
  double T[16], mu = 0.0;
  icp_identity(T);
  if (refused) {
    for (int k = 0; k < 16; k++) T[k] = NAN;
  } else if (!identity) {
    const double g = prm.use_absolute_scale ? 1.0 : scale;
    mu = prm.use_absolute_scale ? scale : 1.0;
    const int64_t* rows = prm.tuple_test ? v.tuples : v.corr;
    double M[16];
    icp_identity(M);
    for (int it = 0; it < prm.iteration_number; it++) {
      double s[kFgrSums];
      icp_sum<kFgrSums>(n, lane_begin, lane_end,
                        [&](int64_t i, double* acc) {
                          const int64_t si = rows[2 * i], ri = rows[2 * i + 1];
                          double p[3], q[3], qm[3], d[3];
                          for (int a = 0; a < 3; a++) {
                            p[a] = (pg_load(v.src, v.src_elem, 3 * si + a) - nm[a]) / g;
                            q[a] = (pg_load(v.ref, v.ref_elem, 3 * ri + a) - nm[3 + a]) / g;
                          }
                          for (int a = 0; a < 3; a++) {
                            const double x = M[4 * a] * q[0], y = M[4 * a + 1] * q[1], z = M[4 * a + 2] * q[2];
                            const double r = (x + y) + z;
                            qm[a] = r + M[4 * a + 3];
                            d[a] = p[a] - qm[a];
                          }
                          const double xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
                          const double dd = (xx + yy) + zz;
                          const double den = dd + mu;
                          const double t = mu / den;
                          const double w = t * t;
#pragma unroll
                          for (int a = 0; a < 3; a++) {                  // coordinate a's Jacobian row: three entries
                            const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
                            const int idx[3] = {a1, a2, 3 + a};
                            const double val[3] = {-qm[a2], qm[a1], -1.0};
                            const double wd = w * d[a];
#pragma unroll
                            for (int x = 0; x < 3; x++) {
                              const double wj = w * val[x];
#pragma unroll
                              for (int y = 0; y < 3; y++)
                                if (idx[x] <= idx[y]) {
                                  const double m = wj * val[y];
                                  acc[fgr_tri(idx[x], idx[y])] += m;
                                }
                              const double m = val[x] * wd;
                              acc[21 + idx[x]] += m;
                            }
                          }
                        },
                        sh, barrier, s);
      double rhs[6], x[6];
      for (int a = 0; a < 6; a++) rhs[a] = -s[21 + a];
      if (!icp_cholesky6(s, rhs, x)) {
        status |= SE3_FGR_SINGULAR;                                      // the identity update; the loop goes on
      } else if (!(fabs(x[0]) < kFgrMaxAngle) || !(fabs(x[1]) < kFgrMaxAngle) || !(fabs(x[2]) < kFgrMaxAngle)) {
        status |= SE3_FGR_STEP_REFUSED;                                  // the pair ends with the M it has
        break;
      } else {
        double sx, cx, sy, cy, sz, cz, U[16], Mn[16];
        fgr_sincos(x[0], &sx, &cx), fgr_sincos(x[1], &sy, &cy), fgr_sincos(x[2], &sz, &cz);
        icp_sincos_to_matrix(sx, cx, sy, cy, sz, cz, x, U);
        icp_compose(U, M, Mn);
        for (int k = 0; k < 16; k++) M[k] = Mn[k];
      }
      if (prm.decrease_mu && it % 4 == 0 && mu > prm.maxdist) mu = mu / prm.division_factor;
    }
    // M maps the normalised reference onto the normalised source: A = [M_R | -M_R mean_R + g M_t + mean_S]; the result is A's inverse
    double At[3];
    for (int a = 0; a < 3; a++) {
      const double x = M[4 * a] * nm[3], y = M[4 * a + 1] * nm[4], z = M[4 * a + 2] * nm[5];
      const double r = (x + y) + z;
      const double gt = g * M[4 * a + 3];
      const double e = gt - r;
      At[a] = e + nm[a];
    }
    for (int a = 0; a < 3; a++) {
      for (int b = 0; b < 3; b++) T[4 * a + b] = M[4 * b + a];
      const double x = M[a] * At[0], y = M[4 + a] * At[1], z = M[8 + a] * At[2];
      const double r = (x + y) + z;
      T[4 * a + 3] = -r;
    }
  }
  if (lane_begin == 0) {
    for (int k = 0; k < 16; k++) v.T[k] = T[k];
    *v.status = status;
    if (v.mu) *v.mu = mu;
  }
}
