// FPFH descriptors of stacked clouds (Open3D's compute_fpfh_feature: 33 bins from the point-pair angles over a point's neighbourhood), for
// up to SE3_PAIR_MAX_PAIRS clouds per call.  se3et_amd/fpfh.py carries the same contract; the searches are the tested ones of
// csrc/pair_geometry.hip (ball query) and csrc/knn_normals.hip (k nearest), which hand this file a neighbour list.
// (SE3_EXACT_FP: the file is built with contraction off, and every contract function of fpfh_core.h fences itself as well.)
//
//   fpfh_check_kernel    one thread per stacked row: a non-finite point or normal raises bit 1 of its cloud's status word.
//   spfh_kernel          one wave per row: lanes stride the row's neighbours, each lane computes one pair feature and its three bins; the 33
//                        INTEGER counters are formed by ballots (lane b < 33 keeps the count of bin b); lanes 0..32 write count (100 / m).
//   fpfh_kernel          one wave per row, lane j < 33 owns bin j: the lanes fetch a tile of 64 neighbours and their d^2 side by side, then
//                        the wave walks the tile in list order, four SPFH rows (264 contiguous bytes each) loaded ahead of their four
//                        dependent divide-and-adds; the three group sums are taken in ascending lane order; scale, add the row's own
//                        SPFH, one store.
//
// Contract.  The structure is Open3D's (Feature.cpp: ComputePairFeatures, ComputeSPFHFeature, ComputeFPFHFeature); the arithmetic is the
// project's own, chosen so that host and device agree bit for bit: float64, contraction off, no libm call other than the square root
// (pg_sqrt) and division.
//   Neighbours.  The neighbours of row i are the members of its list other than row i itself, chosen by index; m is their number.  A
//     duplicate point at d = 0 is a neighbour.  The list is the caller's: a radius search (d^2 < r^2, strict), the K nearest including
//     the row itself by knn_clouds' rule ((d^2, index) ascending, the lower index wins), or the K nearest masked by d^2 < r^2; within a
//     row the list ascends in the neighbour's index.
//   Pair feature of (p1, n1) and (p2, n2), normals as given (not normalised).  Dot products are (a b + c d) + e f.
//     1. dp = p2 - p1, d = sqrt((dx dx + dy dy) + dz dz).          2. d == 0: degenerate.
//     3. a1 = n1 . dp / d, a2 = n2 . dp / d.
//     4. |a1| < |a2| (strict; Open3D writes acos|a1| > acos|a2|): swap the normals, negate dp, f2 = -a2.  Otherwise f2 = a1.
//     5. v = dp x n1; |v| == 0: degenerate.                         6. v /= |v|; w = n1 x v; f1 = v . n2; y = (w . n2) + 0.0; x = n1 . n2.
//     A degenerate pair has f1 = f2 = 0 and x = y = 0.
//   Bins.  f1 and f2: clamp(floor(11 (f + 1) 0.5), 0, 10).  theta = atan2(y, x) is binned without computing it: with beta_k = -pi +
//     2 pi k / 11, (c_k, s_k) = (cos, sin) beta_k for k = 1..10 (float64 literals, fpfh_sector), the bin is 5 if x == 0 and y == 0; the
//     number of k in 1..5 with c_k y - s_k x >= 0 if y < 0; otherwise 5 plus the number of k in 6..10 with c_k y - s_k x >= 0.  This is
//     clamp(floor(11 (theta + pi) / 2 pi), 0, 10) away from the edges; theta = pi gives bin 10; a degenerate pair gives bins 5, 5, 5 and
//     is counted, as in Open3D.
//   SPFH row.  bin count x (100.0 / m): integer counts and one product, so the order of the neighbours does not matter.  theta at 0-10,
//     f1 at 11-21, f2 at 22-32.  m == 0 gives a zero row.
//   FPFH row.  A_j = sum_k spfh(j, k) / d2_k, a sequential sum over the neighbours k with d2_k != 0 in list order (ascending index),
//     d2 = (dx dx + dy dy) + dz dz recomputed; S_g = the sequential sum of the group's eleven A_j in ascending j;
//     F_j = spfh(j, i) + (S_g != 0 ? A_j (100 / S_g) : A_j).  A row with a neighbour at d > 0 therefore sums to 600.
//   Refusals.  A non-finite point or normal raises bit 1 of its cloud's status word (and of the call's, the last word).  A list entry
//     outside its cloud, or row offsets outside the list, are skipped on the device: nothing is read through them (the host entry reports
//     them as bit 2).  A zero normal is not refused: its pairs are degenerate.  n = 0 gives an empty output.
//   Determinism.  No float atomics (the integer atomicOr raises a status word).  A cloud's rows are bit-identical alone, anywhere in a
//     batch, from run to run, and between the device and se3_debug_fpfh_host.
#include <math.h>

#include <vector>

#include "common.h"
#include "fpfh_core.h"          // (and through it pair_grid.h: pg_dist2 here, pg_sqrt there -- stack_rows.h alone is not enough)

namespace {

constexpr int kFpfhWaves = 4;           // rows per workgroup, of both kernels
constexpr int kFpfhAhead = 4;           // SPFH rows loaded ahead of their adds
constexpr int kFpfhNonFinite = 1;       // status bits
constexpr int kFpfhBadList = 2;         // (the host entry alone reports it)

// what the kernels get: the stacked arrays of a call and the row slice [row_begin, row_begin + row_count) the list covers
struct FpfhCall {
  const void* points;
  const void* normals;
  int elem, normals_elem;
  PairRows rows;
  int64_t row_begin, row_count;
  const int64_t* row_offsets;          // (row_count + 1): slice row r owns list entries [row_offsets[r], row_offsets[r + 1])
  const int64_t* pairs;                // (total, 2): (i, j), j the neighbour's cloud-local index; only j is read
  int64_t total;
};

PG_HD bool fpfh_finite3(const double* v) { return fabs(v[0]) < INFINITY && fabs(v[1]) < INFINITY && fabs(v[2]) < INFINITY; }

// the list range of slice row r, or an empty range and *bad when the offsets do not belong to the list
PG_HD void fpfh_row_range(const FpfhCall& c, int64_t r, int64_t* b, int64_t* e, bool* bad) {
  *b = c.row_offsets[r], *e = c.row_offsets[r + 1];
  *bad = *b < 0 || *e < *b || *e > c.total;
  if (*bad) *b = 0, *e = 0;
}

__global__ __launch_bounds__(256) void fpfh_check_kernel(const void* __restrict__ points, int elem, const void* __restrict__ normals,
                                                         int normals_elem, PairRows rows, int64_t n_total, int* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_total) return;
  double p[3], n[3];
  pg_load3(points, elem, i, p);
  pg_load3(normals, normals_elem, i, n);
  if (fpfh_finite3(p) && fpfh_finite3(n)) return;
  atomicOr(status + pg_pair_of_row(rows, i), kFpfhNonFinite);
  atomicOr(status + rows.n, kFpfhNonFinite);
}

__global__ __launch_bounds__(kFpfhWaves* SE3_WAVE) void spfh_kernel(FpfhCall c, double* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * kFpfhWaves + (threadIdx.x >> 6);
  if (r >= c.row_count) return;                            // (uniform over the wave)
  const int lane = se3_lane();
  const int64_t row = c.row_begin + r;
  const int cl = pg_pair_of_row(c.rows, row);
  const int64_t s0 = c.rows.start[cl], n = c.rows.start[cl + 1] - s0, self = row - s0;
  int64_t b, e;
  bool bad;
  fpfh_row_range(c, r, &b, &e, &bad);
  double p1[3], n1[3];
  pg_load3(c.points, c.elem, row, p1);
  pg_load3(c.normals, c.normals_elem, row, n1);
  int count = 0, m = 0;                                    // lane b < 33: the count of bin b
  for (int64_t t0 = b; t0 < e; t0 += SE3_WAVE) {
    const int64_t t = t0 + lane;
    const int64_t j = t < e ? c.pairs[2 * t + 1] : 0;
    const bool inside = t < e && j >= 0 && j < n;
    const bool use = inside && j != self;
    int bins[3] = {-1, -1, -1};
    if (use) {
      double p2[3], n2[3];
      pg_load3(c.points, c.elem, s0 + j, p2);
      pg_load3(c.normals, c.normals_elem, s0 + j, n2);
      fpfh_pair_bins(p1, n1, p2, n2, bins);
    }
    m += __popcll(__ballot(use));
#pragma unroll
    for (int k = 0; k < kFpfhBins; k++) {
      const int c0 = __popcll(__ballot(bins[0] == k)), c1 = __popcll(__ballot(bins[1] == k)), c2 = __popcll(__ballot(bins[2] == k));
      count += lane == k ? c0 : (lane == kFpfhBins + k ? c1 : (lane == 2 * kFpfhBins + k ? c2 : 0));
    }
  }
  if (lane < kFpfhDim) out[row * kFpfhDim + lane] = fpfh_spfh_value(count, m);
}

__global__ __launch_bounds__(kFpfhWaves* SE3_WAVE) void fpfh_kernel(FpfhCall c, const double* __restrict__ spfh, double* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * kFpfhWaves + (threadIdx.x >> 6);
  if (r >= c.row_count) return;                            // (uniform over the wave)
  const int lane = se3_lane();
  const int bin = lane < kFpfhDim ? lane : kFpfhDim - 1;   // (lanes 33..63 shadow bin 32 and store nothing)
  const int64_t row = c.row_begin + r;
  const int cl = pg_pair_of_row(c.rows, row);
  const int64_t s0 = c.rows.start[cl], n = c.rows.start[cl + 1] - s0, self = row - s0;
  int64_t b, e;
  bool bad;
  fpfh_row_range(c, r, &b, &e, &bad);
  double p1[3];
  pg_load3(c.points, c.elem, row, p1);
  double acc = 0.0;
  for (int64_t t0 = b; t0 < e; t0 += SE3_WAVE) {
    // the tile: lane t holds neighbour t0 + t and its d^2
    const int64_t t = t0 + lane;
    const int64_t j = t < e ? c.pairs[2 * t + 1] : 0;
    const bool inside = t < e && j >= 0 && j < n;
    double d2 = 0.0;
    if (inside && j != self) {
      double p2[3];
      pg_load3(c.points, c.elem, s0 + j, p2);
      d2 = pg_dist2(p1, p2);
    }
    const int jl = (int)j;                                 // (inside: j < n < 2^31)
    unsigned long long mask = __ballot(inside && j != self && d2 != 0.0);
    // the walk, in list order: kFpfhAhead rows loaded, then their dependent adds
    while (mask) {
      double s[kFpfhAhead], w[kFpfhAhead];
      int got = 0;
#pragma unroll
      for (int u = 0; u < kFpfhAhead; u++) {
        if (!mask) break;
        const int src = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        s[u] = spfh[(s0 + __shfl(jl, src)) * kFpfhDim + bin];
        w[u] = __shfl(d2, src);
        got = u + 1;
      }
#pragma unroll
      for (int u = 0; u < kFpfhAhead; u++)
        if (u < got) acc = fpfh_weighted_add(acc, s[u], w[u]);
    }
  }
  // the group's sum, in ascending lane order
  const int first = (bin / kFpfhBins) * kFpfhBins;
  double group = 0.0;
#pragma unroll
  for (int u = 0; u < kFpfhBins; u++) group += __shfl(acc, first + u);
  if (lane < kFpfhDim) out[row * kFpfhDim + lane] = fpfh_value(spfh[row * kFpfhDim + lane], acc, group);
}

// what the entries check; leaves `c` filled.  normals: NULL for the second pass, which reads none
int fpfh_call_args(const char* name, FpfhCall* c, const void* points, int elem, const void* normals, int normals_elem, const int64_t* offsets_host,
                   int num_clouds, int64_t row_begin, int64_t row_count, const int64_t* row_offsets, const int64_t* pairs, int64_t total,
                   const void* out) {
  SE3_REQUIRE(points && offsets_host && row_offsets && (pairs || total == 0) && out, SE3_ERR_INVALID_ARG, "%s: null pointer", name);
  SE3_REQUIRE(num_clouds >= 0 && num_clouds <= kPairMaxPairs && (elem == 0 || elem == 1) && (normals_elem == 0 || normals_elem == 1),
              SE3_ERR_INVALID_ARG, "%s: %d clouds (at most %d), elem %d, normals_elem %d", name, num_clouds, kPairMaxPairs, elem, normals_elem);
  SE3_REQUIRE(pg_fill_rows(&c->rows, offsets_host, num_clouds), SE3_ERR_INVALID_ARG, "%s: offsets must start at 0 and not decrease", name);
  const int64_t n_total = c->rows.start[num_clouds];
  SE3_REQUIRE(n_total < (1ll << 31), SE3_ERR_UNSUPPORTED, "%s: %lld rows in one call (below 2^31)", name, (long long)n_total);
  SE3_REQUIRE(row_begin >= 0 && row_count >= 0 && row_begin + row_count <= n_total && total >= 0, SE3_ERR_INVALID_ARG,
              "%s: rows [%lld, %lld + %lld) of %lld, %lld list entries", name, (long long)row_begin, (long long)row_begin, (long long)row_count,
              (long long)n_total, (long long)total);
  c->points = points, c->normals = normals, c->elem = elem, c->normals_elem = normals_elem;
  c->row_begin = row_begin, c->row_count = row_count, c->row_offsets = row_offsets, c->pairs = pairs, c->total = total;
  return SE3_OK;
}

}  // namespace

extern "C" int se3_fpfh_check_stack(const void* points, int elem, const void* normals, int normals_elem, const int64_t* offsets_host,
                                    int num_clouds, int* status, void* stream) {
  SE3_REQUIRE(points && normals && offsets_host && status, SE3_ERR_INVALID_ARG, "fpfh_check_stack: null pointer");
  SE3_REQUIRE(num_clouds >= 0 && num_clouds <= kPairMaxPairs && (elem == 0 || elem == 1) && (normals_elem == 0 || normals_elem == 1),
              SE3_ERR_INVALID_ARG, "fpfh_check_stack: %d clouds (at most %d), elem %d, normals_elem %d", num_clouds, kPairMaxPairs, elem,
              normals_elem);
  PairRows rows;
  SE3_REQUIRE(pg_fill_rows(&rows, offsets_host, num_clouds), SE3_ERR_INVALID_ARG, "fpfh_check_stack: offsets must start at 0 and not decrease");
  const int64_t n_total = rows.start[num_clouds];
  SE3_REQUIRE(n_total < (1ll << 31), SE3_ERR_UNSUPPORTED, "fpfh_check_stack: %lld rows in one call (below 2^31)", (long long)n_total);
  hipStream_t st = (hipStream_t)stream;
  SE3_REQUIRE(hipMemsetAsync(status, 0, sizeof(int) * (size_t)(num_clouds + 1), st) == hipSuccess, SE3_ERR_LAUNCH,
              "fpfh_check_stack: memset failed");
  if (n_total == 0) return SE3_OK;
  fpfh_check_kernel<<<(unsigned)se3_cdiv(n_total, 256), 256, 0, st>>>(points, elem, normals, normals_elem, rows, n_total, status);
  SE3_CHECK_LAUNCH("fpfh_check_stack");
  return SE3_OK;
}

extern "C" int se3_spfh_stack(const void* points, int elem, const void* normals, int normals_elem, const int64_t* offsets_host, int num_clouds,
                              int64_t row_begin, int64_t row_count, const int64_t* row_offsets, const int64_t* pairs, int64_t total,
                              double* out_spfh, void* stream) {
  SE3_REQUIRE(normals, SE3_ERR_INVALID_ARG, "spfh_stack: null pointer");
  FpfhCall c;
  const int rc = fpfh_call_args("spfh_stack", &c, points, elem, normals, normals_elem, offsets_host, num_clouds, row_begin, row_count, row_offsets,
                                pairs, total, out_spfh);
  if (rc != SE3_OK) return rc;
  if (row_count == 0) return SE3_OK;
  spfh_kernel<<<(unsigned)se3_cdiv(row_count, kFpfhWaves), kFpfhWaves * SE3_WAVE, 0, (hipStream_t)stream>>>(c, out_spfh);
  SE3_CHECK_LAUNCH("spfh_stack");
  return SE3_OK;
}

extern "C" int se3_fpfh_stack(const void* points, int elem, const double* spfh, const int64_t* offsets_host, int num_clouds, int64_t row_begin,
                              int64_t row_count, const int64_t* row_offsets, const int64_t* pairs, int64_t total, double* out_fpfh, void* stream) {
  SE3_REQUIRE(spfh, SE3_ERR_INVALID_ARG, "fpfh_stack: null pointer");
  FpfhCall c;
  const int rc = fpfh_call_args("fpfh_stack", &c, points, elem, nullptr, 1, offsets_host, num_clouds, row_begin, row_count, row_offsets, pairs, total,
                                out_fpfh);
  if (rc != SE3_OK) return rc;
  if (row_count == 0) return SE3_OK;
  fpfh_kernel<<<(unsigned)se3_cdiv(row_count, kFpfhWaves), kFpfhWaves * SE3_WAVE, 0, (hipStream_t)stream>>>(c, spfh, out_fpfh);
  SE3_CHECK_LAUNCH("fpfh_stack");
  return SE3_OK;
}

// ---- the same text on host memory, one cloud, no GPU (tests/test_fpfh_cpu.py) ------------------------------------------------------------------
// row_offsets (n + 1) and pairs (total, 2) as se3_debug_pair_ball_host leaves them (or built from se3_debug_knn_host's table); out_spfh and
// out_fpfh (n, 33); *status: 0, bit 1 as the device's status word (nothing is computed), bit 2 for a list entry or row offsets that were skipped.
extern "C" int se3_debug_fpfh_host(const void* points, const void* normals, int64_t n, int elem, int normals_elem, const int64_t* row_offsets,
                                   const int64_t* pairs, int64_t total, double* out_spfh, double* out_fpfh, int* status) {
  SE3_REQUIRE(points && normals && row_offsets && (pairs || total == 0) && out_spfh && out_fpfh && status, SE3_ERR_INVALID_ARG,
              "debug_fpfh_host: null pointer");
  SE3_REQUIRE(n >= 0 && n < (1ll << 31) && total >= 0 && (elem == 0 || elem == 1) && (normals_elem == 0 || normals_elem == 1), SE3_ERR_INVALID_ARG,
              "debug_fpfh_host: n %lld, total %lld, elem %d, normals_elem %d", (long long)n, (long long)total, elem, normals_elem);
  FpfhCall c;
  c.points = points, c.normals = normals, c.elem = elem, c.normals_elem = normals_elem;
  c.row_begin = 0, c.row_count = n, c.row_offsets = row_offsets, c.pairs = pairs, c.total = total;
  *status = 0;
  for (int64_t i = 0; i < n; i++) {
    double p[3], nr[3];
    pg_load3(points, elem, i, p);
    pg_load3(normals, normals_elem, i, nr);
    if (!fpfh_finite3(p) || !fpfh_finite3(nr)) *status |= kFpfhNonFinite;
  }
  if (*status) return SE3_OK;
  for (int64_t i = 0; i < n; i++) {
    int64_t b, e;
    bool bad;
    fpfh_row_range(c, i, &b, &e, &bad);
    double p1[3], n1[3];
    pg_load3(points, elem, i, p1);
    pg_load3(normals, normals_elem, i, n1);
    int counts[kFpfhDim] = {0}, m = 0;
    for (int64_t t = b; t < e; t++) {
      const int64_t j = pairs[2 * t + 1];
      if (j < 0 || j >= n) {
        bad = true;
        continue;
      }
      if (j == i) continue;
      double p2[3], n2[3];
      int bins[3];
      pg_load3(points, elem, j, p2);
      pg_load3(normals, normals_elem, j, n2);
      fpfh_pair_bins(p1, n1, p2, n2, bins);
      for (int f = 0; f < 3; f++) counts[f * kFpfhBins + bins[f]]++;
      m++;
    }
    if (bad) *status |= kFpfhBadList;
    for (int k = 0; k < kFpfhDim; k++) out_spfh[i * kFpfhDim + k] = fpfh_spfh_value(counts[k], m);
  }
  for (int64_t i = 0; i < n; i++) {
    int64_t b, e;
    bool bad;
    fpfh_row_range(c, i, &b, &e, &bad);
    double p1[3], acc[kFpfhDim] = {0.0};
    pg_load3(points, elem, i, p1);
    for (int64_t t = b; t < e; t++) {
      const int64_t j = pairs[2 * t + 1];
      if (j < 0 || j >= n || j == i) continue;
      double p2[3];
      pg_load3(points, elem, j, p2);
      const double d2 = pg_dist2(p1, p2);
      if (d2 == 0.0) continue;
      for (int k = 0; k < kFpfhDim; k++) acc[k] = fpfh_weighted_add(acc[k], out_spfh[j * kFpfhDim + k], d2);
    }
    for (int g = 0; g < 3; g++) {
      double group = 0.0;
      for (int u = 0; u < kFpfhBins; u++) group += acc[g * kFpfhBins + u];
      for (int u = 0; u < kFpfhBins; u++) {
        const int k = g * kFpfhBins + u;
        out_fpfh[i * kFpfhDim + k] = fpfh_value(out_spfh[i * kFpfhDim + k], acc[k], group);
      }
    }
  }
  return SE3_OK;
}

// the twenty constants of the sector rule: out[2 (k - 1)] = c_k, out[2 (k - 1) + 1] = s_k, k = 1 .. 10
extern "C" int se3_debug_fpfh_sectors_host(double* out) {
  SE3_REQUIRE(out, SE3_ERR_INVALID_ARG, "debug_fpfh_sectors_host: null pointer");
  for (int k = 1; k <= 10; k++) fpfh_sector(k, out + 2 * (k - 1), out + 2 * (k - 1) + 1);
  return SE3_OK;
}
