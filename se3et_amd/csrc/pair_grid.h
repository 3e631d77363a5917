// Uniform float64 grid over the TRANSFORMED support cloud of each pair of a stacked call, and the search core that every tool on it shares:
// csrc/pair_geometry.hip (which also owns the device build, se3_pair_grid_build), knn_normals.hip, icp.hip, keypoint_nms.hip, fpfh.hip, iss.hip, outliers.hip and color_gradient.hip.
//
// The grid is only an accelerator: every answer is defined by the arithmetic contract in pair_geometry.hip (transform by the documented fma
// chain, d^2 = (dx dx + dy dy) + dz dz unfused, strict tests, the lowest index among equal distances), and the walks below visit every
// cell that can hold a point passing the test.
//
// The header is host/device text alone, included at file scope: templates, __forceinline__ and inline functions.  The cell walk, the shell
// termination rule and the candidate test are __host__ __device__: the kernels run them with one wave per query row (nearest neighbour, k
// nearest: `lane` of 64) or one thread per row (ball query), and the se3_debug_*_host entries run the same text on host memory over a
// PairHostGrid (the CPU tests).  Host side: pg_carve lays a workspace out, pg_grid_call is the one check of an entry that searches a grid.
//
// Layout of a grid workspace (pg_carve): meta[P], cells[P][kPairCellCap + 1] (cells[c] .. cells[c + 1] is cell c's run of `sorted`),
// moved (3 float64 per support point, in input order: the transformed cloud), sorted (3 float64 per point, cell by cell), sorted_idx (the
// pair-local index of each sorted point).  The order of the points INSIDE a cell follows the arrival of the scatter's integer atomics; no
// result depends on it: the nearest neighbour reduces on (d^2, index), the ball query sorts each row, counts are integers.
#pragma once
#include <math.h>

#include <vector>

#include "common.h"
#include "stack_rows.h"

constexpr int kPairGridCap = 64;                                       // cells per axis at most (kGridCap of radius_neighbors.hip)
constexpr int kPairCellCap = kPairGridCap * kPairGridCap * kPairGridCap;
constexpr double kPairSlack = 1e-14;                                   // relative safety of every pruning bound: ~90 float64 roundings

struct PairGridMeta {
  double T[12];          // rows of [R | t]
  double org[3], top[3];  // exact bounding box of the transformed support
  double cell, inv_cell;
  int dim[3], ncells;
  int64_t s_start, ns;   // rows of this pair in the stacked support
};

struct PairGridView {
  const PairGridMeta* meta;     // [P]
  const int* cells;             // [P][kPairCellCap + 1]
  const double* sorted;         // [ns_total][3]
  const int* sorted_idx;        // [ns_total]
};

// (fma(R[k][2], z, fma(R[k][1], y, R[k][0] * x)) + t[k])_k
PG_HD void pg_transform(const double* T, double x, double y, double z, double* out) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; k++) {
    const double a = T[4 * k] * x;
    const double b = __builtin_fma(T[4 * k + 1], y, a);
    const double c = __builtin_fma(T[4 * k + 2], z, b);
    out[k] = c + T[4 * k + 3];
  }
}
// row `row` of an (n, 3) array, transformed
PG_HD void pg_transform_row(const double* T, const void* p, int elem, int64_t row, double* out) {
  double s[3];
  pg_load3(p, elem, row, s);
  pg_transform(T, s[0], s[1], s[2], out);
}

// the candidate test's distance: (dx dx + dy dy) + dz dz, every product and sum rounded on its own
PG_HD double pg_dist2(const double* q, const double* s) {
#pragma clang fp contract(off)
  const double dx = q[0] - s[0], dy = q[1] - s[1], dz = q[2] - s[2];
  const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const double a = xx + yy;
  return a + zz;
}

// sqrt rounded to nearest on the host and on the device alike: the device's float64 root is good to an ulp, not to the last bit, so one
// step on the exact residual x - r r (an fma) settles it
PG_HD double pg_sqrt(double x) {
#pragma clang fp contract(off)
  const double r = sqrt(x);
  if (!(r > 0.0) || !(r < INFINITY)) return r;
  const double e = __builtin_fma(-r, r, x);
  const double c = e / (2.0 * r);
  return r + c;
}

// floor((v - org) / cell) kept inside [-1, dim] (a NaN gives -1); monotone in v
PG_HD int pg_cell_floor(double v, double org, double inv_cell, int dim) {
  const double f = floor((v - org) * inv_cell);
  if (!(f >= 0.0)) return -1;
  return f >= (double)dim ? dim : (int)f;
}
// the cell a point is filed under: the same value clamped into the grid (the last cell also holds what the axis cap cut off)
PG_HD int pg_cell_coord(double v, double org, double inv_cell, int dim) {
  const int c = pg_cell_floor(v, org, inv_cell, dim);
  return c < 0 ? 0 : (c >= dim ? dim - 1 : c);
}
PG_HD int pg_cell_of(const PairGridMeta& m, const double* p) {
  const int cx = pg_cell_coord(p[0], m.org[0], m.inv_cell, m.dim[0]);
  const int cy = pg_cell_coord(p[1], m.org[1], m.inv_cell, m.dim[1]);
  const int cz = pg_cell_coord(p[2], m.org[2], m.inv_cell, m.dim[2]);
  return cx + m.dim[0] * (cy + m.dim[1] * cz);
}

// Grid of n points inside [mn, mx].  cell_hint > 0 (ball query: the radius) is the cell size; otherwise it comes from the density, the
// box volume over n (one point per cell if the cloud filled its box).  Either is raised until no axis needs more than kPairGridCap cells.
PG_HD void pg_make_grid(const double* mn, const double* mx, int64_t n, double cell_hint, PairGridMeta* m) {
  double ext[3], big = 0.0;
  for (int d = 0; d < 3; d++) {
    ext[d] = n > 0 ? mx[d] - mn[d] : 0.0;
    if (!(ext[d] >= 0.0) || ext[d] > 1.7e308) ext[d] = 0.0;          // (non-finite points: any grid is safe, no walk leaves it)
    big = fmax(big, ext[d]);
  }
  double cell = cell_hint;
  if (!(cell > 0.0)) {
    double vol = 1.0;
    for (int d = 0; d < 3; d++) vol *= fmax(ext[d], 1e-3 * big);
    cell = n > 0 ? cbrt(vol / (double)n) : 0.0;
  }
  cell = fmax(cell, big / (double)(kPairGridCap - 1));
  if (!(cell > 0.0) || cell > 1.7e308) cell = 1.0;                     // one point, or all points equal
  m->cell = cell;
  m->inv_cell = 1.0 / cell;
  m->ncells = 1;
  for (int d = 0; d < 3; d++) {
    m->org[d] = n > 0 ? mn[d] : 0.0;
    m->top[d] = n > 0 ? mx[d] : 0.0;
    const int dim = pg_cell_coord(m->top[d], m->org[d], m->inv_cell, kPairGridCap) + 1;
    m->dim[d] = dim;
    m->ncells *= dim;
  }
}

// ---- nearest neighbour ----------------------------------------------------------------------------------------------------------------
// The cells of Chebyshev ring k around cell c, clipped to the grid, as runs of consecutive cells [a, b] (cells are linear in x).
template <class Run>
PG_HD void pg_ring_runs(const PairGridMeta& m, const int* c, int k, Run&& run) {
  const int x0 = c[0] - k < 0 ? 0 : c[0] - k, x1 = c[0] + k >= m.dim[0] ? m.dim[0] - 1 : c[0] + k;
  const int y0 = c[1] - k < 0 ? 0 : c[1] - k, y1 = c[1] + k >= m.dim[1] ? m.dim[1] - 1 : c[1] + k;
  const int z0 = c[2] - k < 0 ? 0 : c[2] - k, z1 = c[2] + k >= m.dim[2] ? m.dim[2] - 1 : c[2] + k;
  for (int z = z0; z <= z1; z++)
    for (int y = y0; y <= y1; y++) {
      const int row = m.dim[0] * (y + m.dim[1] * z);
      if (z - c[2] == k || c[2] - z == k || y - c[1] == k || c[1] - y == k) {
        run(row + x0, row + x1);                                       // a face row of the ring: all of its x
      } else {
        if (c[0] - k >= 0) run(row + c[0] - k, row + c[0] - k);        // an inner row: its two end cells
        if (c[0] + k < m.dim[0]) run(row + c[0] + k, row + c[0] + k);
      }
    }
}

// Shell termination rule: a lower bound of d^2 from q to every support point filed outside rings 0 .. k around c, +inf when those rings
// cover the grid.  A cell outside lies beyond ring k on at least one axis and side; on that axis its points are at least `gap` from q (the
// face of the ring, less kPairSlack for the roundings of the filing), on the other axes at least q's distance to the exact bounding box.
PG_HD double pg_shell_bound2(const PairGridMeta& m, const double* q, const int* c, int k) {
  double box2[3];
  for (int d = 0; d < 3; d++) {
    const double o = fmax(fmax(m.org[d] - q[d], q[d] - m.top[d]), 0.0);
    box2[d] = o * o;
  }
  double best = INFINITY;
  for (int a = 0; a < 3; a++) {
    const double others = box2[(a + 1) % 3] + box2[(a + 2) % 3];
    for (int side = 0; side < 2; side++) {
      if (side == 0 ? c[a] - k - 1 < 0 : c[a] + k + 1 > m.dim[a] - 1) continue;   // no cell left on this side
      const double face = m.org[a] + (double)(side == 0 ? c[a] - k : c[a] + k + 1) * m.cell;
      double gap = side == 0 ? q[a] - face : face - q[a];
      gap = fmax(gap - kPairSlack * (fabs(m.org[a]) + fabs(face) + fabs(q[a])), 0.0);
      best = fmin(best, gap * gap + others);
    }
  }
  return best * (1.0 - kPairSlack);
}

// Candidate test of the nearest neighbour: smaller d^2 wins, the lower index among equal d^2.
PG_HD void pg_nearest_update(double d2, int j, double* best_d2, int* best_j) {
  if (d2 < *best_d2 || (d2 == *best_d2 && j < *best_j)) *best_d2 = d2, *best_j = j;
}

// Exact nearest neighbour of q among pair `m`'s support.  Lanes lane, lane + nlanes, .. take the points of each run of a ring; `reduce`
// makes (d^2, index) the minimum over the lanes after every ring (the host calls it with one lane and a no-op).  The rings widen until the
// best d^2 found is no larger than the bound of everything outside them.  Empty support: d^2 = +inf, index -1.
template <class Reduce>
PG_HD void pg_nearest(const PairGridView& g, int p, const double* q, int lane, int nlanes, Reduce&& reduce, double* out_d2, int* out_j) {
  const PairGridMeta& m = g.meta[p];
  const int* cells = g.cells + (size_t)p * (kPairCellCap + 1);
  const double* pts = g.sorted + 3 * m.s_start;
  const int* idx = g.sorted_idx + m.s_start;
  int c[3];
  for (int d = 0; d < 3; d++) c[d] = pg_cell_coord(q[d], m.org[d], m.inv_cell, m.dim[d]);
  double best = INFINITY;
  int best_j = -1;
  for (int k = 0; k < kPairGridCap; k++) {
    pg_ring_runs(m, c, k, [&](int a, int b) {
      const int end = cells[b + 1];
      for (int t = cells[a] + lane; t < end; t += nlanes) pg_nearest_update(pg_dist2(q, pts + 3 * (size_t)t), idx[t], &best, &best_j);
    });
    reduce(&best, &best_j);
    if (best <= pg_shell_bound2(m, q, c, k)) break;
  }
  *out_d2 = best;
  *out_j = best_j;
}

// pg_nearest by one wave per query: the lanes stride the runs, a butterfly makes (d^2, index) the wave's minimum on every lane
__device__ __forceinline__ void pg_wave_nearest(const PairGridView& g, int p, const double* q, double* out_d2, int* out_j) {
  pg_nearest(g, p, q, se3_lane(), SE3_WAVE,
             [](double* best, int* best_j) {
#pragma unroll
               for (int o = 32; o > 0; o >>= 1) pg_nearest_update(__shfl_xor(*best, o), __shfl_xor(*best_j, o), best, best_j);
             },
             out_d2, out_j);
}

// ---- ball query -------------------------------------------------------------------------------------------------------------------------
// hit(j) for every support point of pair `m` with d^2 < r2, in cell order.  The block of cells comes from q -+ r widened by kPairSlack, so
// a point whose rounded d^2 passes while its true distance is a rounding beyond r is still visited.
template <class Hit>
PG_HD void pg_ball_walk(const PairGridView& g, int p, const double* q, double r, double r2, Hit&& hit) {
  const PairGridMeta& m = g.meta[p];
  if (m.ns <= 0) return;
  const int* cells = g.cells + (size_t)p * (kPairCellCap + 1);
  const double* pts = g.sorted + 3 * m.s_start;
  const int* idx = g.sorted_idx + m.s_start;
  int lo[3], hi[3];
  for (int d = 0; d < 3; d++) {
    const double rr = r + kPairSlack * (r + fabs(q[d]) + fabs(m.org[d]));
    lo[d] = pg_cell_coord(q[d] - rr, m.org[d], m.inv_cell, m.dim[d]);
    hi[d] = pg_cell_floor(q[d] + rr, m.org[d], m.inv_cell, m.dim[d]);
    if (hi[d] < 0) return;                                             // the ball ends below the box (or q is NaN)
    if (hi[d] > m.dim[d] - 1) hi[d] = m.dim[d] - 1;
  }
  for (int z = lo[2]; z <= hi[2]; z++)
    for (int y = lo[1]; y <= hi[1]; y++) {
      const int row = m.dim[0] * (y + m.dim[1] * z);
      const int end = cells[row + hi[0] + 1];
      for (int t = cells[row + lo[0]]; t < end; t++)
        if (pg_dist2(q, pts + 3 * (size_t)t) < r2) hit(idx[t]);
    }
}

PG_HD int64_t pg_ball_count(const PairGridView& g, int p, const double* q, double r, double r2) {
  int64_t n = 0;
  pg_ball_walk(g, p, q, r, r2, [&](int) { n++; });
  return n;
}

// Writes row i's hits as (i, j) pairs, j ascending, to out[0, 2 * capacity): each hit is inserted into the sorted part written so far
// (rows are short).  Returns the number of hits met; never writes past capacity.
PG_HD int64_t pg_ball_fill(const PairGridView& g, int p, const double* q, double r, double r2, int64_t i, int64_t* out, int64_t capacity) {
  int64_t n = 0;
  pg_ball_walk(g, p, q, r, r2, [&](int j) {
    if (n < capacity) {
      int64_t k = n;
      for (; k > 0 && out[2 * (k - 1) + 1] > j; k--) out[2 * k + 1] = out[2 * (k - 1) + 1];
      out[2 * k + 1] = j;
      out[2 * n] = i;
    }
    n++;
  });
  return n;
}

// ---- k nearest neighbours (csrc/knn_normals.hip) ---------------------------------------------------------------------------------------------
// The k support points of pair `m` with the smallest d^2 = pg_dist2, ascending by (d^2, index): among equal distances the lower index comes
// first and wins the last slot.  The caller's `list` holds the best k found so far, sorted; it offers every point of a ring's cells and the
// rings widen until the k-th best d^2 is no larger than pg_shell_bound2 of everything outside them (a list that is not full holds +inf
// there, so the walk goes on until the rings cover the grid).  The result is a sorted SET: it does not depend on the order of the points
// inside a cell, nor on which lane met which point.
//   list.offer(valid, d2, j)   every lane of the row calls it together (the kernel inserts across lanes); valid = this lane holds a point
//   list.kth_d2()              the k-th best d^2 so far, the same on every lane
constexpr int kPairKnnMax = 64;               // one list entry per lane of a wave
constexpr int kPairKnnEmpty = 0x7fffffff;     // index of an empty list entry: sorts behind every point at d^2 = +inf

// (d2, j) comes before (e2, ej) in a row
PG_HD bool pg_knn_before(double d2, int j, double e2, int ej) { return d2 < e2 || (d2 == e2 && j < ej); }

template <class List>
PG_HD void pg_knn(const PairGridView& g, int p, const double* q, int lane, int nlanes, List& list) {
  const PairGridMeta& m = g.meta[p];
  const int* cells = g.cells + (size_t)p * (kPairCellCap + 1);
  const double* pts = g.sorted + 3 * m.s_start;
  const int* idx = g.sorted_idx + m.s_start;
  int c[3];
  for (int d = 0; d < 3; d++) c[d] = pg_cell_coord(q[d], m.org[d], m.inv_cell, m.dim[d]);
  for (int k = 0; k < kPairGridCap; k++) {
    pg_ring_runs(m, c, k, [&](int a, int b) {
      const int end = cells[b + 1];
      for (int t0 = cells[a]; t0 < end; t0 += nlanes) {                // (uniform over the lanes: offer is a collective)
        const int t = t0 + lane;
        const bool valid = t < end;
        double d2 = INFINITY;
        int j = kPairKnnEmpty;
        if (valid) d2 = pg_dist2(q, pts + 3 * (size_t)t), j = idx[t];
        list.offer(valid, d2, j);
      }
    });
    if (list.kth_d2() <= pg_shell_bound2(m, q, c, k)) break;
  }
}

// the list of a serial caller (the debug entries): insertion into a sorted array
struct PairKnnSerialList {
  double d2[kPairKnnMax];
  int j[kPairKnnMax];
  int k;
  PG_HD void init(int k_) {
    k = k_;
    for (int t = 0; t < kPairKnnMax; t++) d2[t] = INFINITY, j[t] = kPairKnnEmpty;
  }
  PG_HD double kth_d2() const { return d2[k - 1]; }
  PG_HD void offer(bool valid, double cd, int cj) {
    if (!valid || !pg_knn_before(cd, cj, d2[k - 1], j[k - 1])) return;
    int t = k - 1;
    for (; t > 0 && pg_knn_before(cd, cj, d2[t - 1], j[t - 1]); t--) d2[t] = d2[t - 1], j[t] = j[t - 1];
    d2[t] = cd, j[t] = cj;
  }
};

// the list of a kernel that searches with one wave per query row (knn_normals.hip, outliers.hip): lane t holds the t-th best entry
struct WaveKnnList {
  double d2, kd;
  int j, kj, k;
  __device__ __forceinline__ void init(int k_) { k = k_, d2 = kd = INFINITY, j = kj = kPairKnnEmpty; }
  __device__ __forceinline__ double kth_d2() const { return kd; }
  __device__ __forceinline__ void offer(bool valid, double cd, int cj) {
    unsigned long long mask = __ballot(valid && pg_knn_before(cd, cj, kd, kj));
    while (mask) {                                                               // (few: about k ln(visited / k) per row)
      const int src = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const double bd = __shfl(cd, src);
      const int bj = __shfl(cj, src);
      if (!pg_knn_before(bd, bj, kd, kj)) continue;                              // (an earlier candidate of this ballot moved the k-th)
      const int pos = __popcll(__ballot(pg_knn_before(d2, j, bd, bj)));          // entries are sorted: the lanes that stay are a prefix
      const double ud = __shfl_up(d2, 1);
      const int uj = __shfl_up(j, 1);
      const int l = se3_lane();
      if (l == pos) d2 = bd, j = bj;
      else if (l > pos) d2 = ud, j = uj;
      kd = __shfl(d2, k - 1);
      kj = __shfl(j, k - 1);
    }
  }
};

// ---- host side: the workspace, the entry check, the serial build ------------------------------------------------------------------------------
struct PairGridLayout {
  PairGridMeta* meta;
  int* cells;
  double* moved;
  double* sorted;
  int* sorted_idx;
  PairGridView view() const { return PairGridView{meta, cells, sorted, sorted_idx}; }
};

inline size_t pg_carve(int64_t ns_total, int num_pairs, char* base, PairGridLayout* L) {
  Se3Carver c(base);
  const size_t n = (size_t)(ns_total > 0 ? ns_total : 1), P = (size_t)(num_pairs > 0 ? num_pairs : 1);
  PairGridLayout l;
  l.meta = c.take<PairGridMeta>(P);
  l.cells = c.take<int>(P * (kPairCellCap + 1));
  l.moved = c.take<double>(3 * n);
  l.sorted = c.take<double>(3 * n);
  l.sorted_idx = c.take<int>(n);
  if (L) *L = l;
  return c.bytes();
}

// What an entry that searches a built grid has after its checks: the rows of the stacked query, the grid, the number of query rows.
struct PairGridCall {
  PairRows rows;
  PairGridLayout G;
  int64_t n_total;
};

// The entry check of such a call, in this order: pointers (`pointers`: the entry's others are there), the pair count with ns_total and
// elem, the offsets, the grid workspace's size, fewer than max_rows query rows.  `name` is the entry's, `unit` its word for a pair.  An
// entry that words one of these refusals differently makes that check itself first; its other conditions are its own.
inline int pg_grid_call(const char* name, const char* unit, bool pointers, const void* grid_workspace, size_t workspace_bytes, int64_t ns_total,
                        int elem, const int64_t* offsets_host, int num_pairs, int64_t max_rows, PairGridCall* out) {
  SE3_REQUIRE(pointers && grid_workspace && offsets_host, SE3_ERR_INVALID_ARG, "%s: null pointer", name);
  SE3_REQUIRE(num_pairs >= 0 && num_pairs <= kPairMaxPairs && ns_total >= 0 && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG,
              "%s: %d %s (at most %d), ns_total %lld, elem %d", name, num_pairs, unit, kPairMaxPairs, (long long)ns_total, elem);
  SE3_REQUIRE(pg_fill_rows(&out->rows, offsets_host, num_pairs), SE3_ERR_INVALID_ARG, "%s: offsets must start at 0 and not decrease", name);
  SE3_REQUIRE(pg_carve(ns_total, num_pairs, (char*)grid_workspace, &out->G) <= workspace_bytes, SE3_ERR_WORKSPACE,
              "%s: grid workspace of %zu bytes is too small", name, workspace_bytes);
  out->n_total = out->rows.start[num_pairs];
  SE3_REQUIRE(out->n_total < max_rows, SE3_ERR_UNSUPPORTED, "%s: %lld query rows in one call", name, (long long)out->n_total);
  return SE3_OK;
}

inline bool pg_radius_ok(double radius) { return isfinite(radius) && radius >= 0.0; }

// one ball radius per pair of a stacked call, passed to kernels by value
struct PairRadii {
  double r[kPairMaxPairs];
};
// radii_host[0, num_pairs), or `radius` for every pair when radii_host is NULL; false unless every radius is finite and >= 0
inline bool pg_fill_radii(PairRadii* radii, const double* radii_host, double radius, int num_pairs) {
  bool ok = true;
  for (int p = 0; p < kPairMaxPairs; p++) {
    radii->r[p] = radii_host ? (p < num_pairs ? radii_host[p] : 0.0) : radius;
    ok = ok && pg_radius_ok(radii->r[p]);
  }
  return ok;
}
// the first radius that pg_fill_radii refused (for the message)
inline double pg_bad_radius(const PairRadii& radii) {
  for (int p = 0; p < kPairMaxPairs; p++)
    if (!pg_radius_ok(radii.r[p])) return radii.r[p];
  return 0.0;
}

// The grid build on host memory, serial, over a workspace laid out by pg_carve in `base` (the debug entries).
inline void pg_build_host(const void* s_points, int elem, const PairRows& rows, const double* transforms, double cell_hint, PairGridLayout& G) {
  for (int p = 0; p < rows.n; p++) {
    PairGridMeta& m = G.meta[p];
    const int64_t s0 = rows.start[p], n = rows.start[p + 1] - s0;
    for (int k = 0; k < 12; k++) m.T[k] = transforms[16 * p + k];
    m.s_start = s0, m.ns = n;
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = s0; i < s0 + n; i++) {
      pg_transform_row(m.T, s_points, elem, i, G.moved + 3 * i);
      for (int d = 0; d < 3; d++) mn[d] = fmin(mn[d], G.moved[3 * i + d]), mx[d] = fmax(mx[d], G.moved[3 * i + d]);
    }
    pg_make_grid(mn, mx, n, cell_hint, &m);
    int* cells = G.cells + (size_t)p * (kPairCellCap + 1);
    for (int c = 0; c <= m.ncells; c++) cells[c] = 0;
    for (int64_t i = s0; i < s0 + n; i++) cells[pg_cell_of(m, G.moved + 3 * i)]++;
    int run = 0;
    for (int c = 0; c <= m.ncells; c++) {
      const int v = cells[c];
      cells[c] = run;
      run += v;
    }
    std::vector<int> cursor(cells, cells + m.ncells);
    for (int64_t i = s0; i < s0 + n; i++) {
      const int pos = cursor[(size_t)pg_cell_of(m, G.moved + 3 * i)]++;
      for (int d = 0; d < 3; d++) G.sorted[3 * (s0 + pos) + d] = G.moved[3 * i + d];
      G.sorted_idx[s0 + pos] = (int)(i - s0);
    }
  }
}

// One cloud's grid on host memory (the debug entries): `transform` (4, 4) row-major, or NULL for the identity.
struct PairHostGrid {
  std::vector<char> mem;
  PairGridLayout G;
  PairHostGrid(const void* points, int64_t n, int elem, const double* transform, double cell_hint) : mem(pg_carve(n, 1, nullptr, nullptr)) {
    pg_carve(n, 1, mem.data(), &G);
    const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    pg_build_host(points, elem, pg_single_rows(n), transform ? transform : eye, cell_hint, G);
  }
  PairHostGrid(const PairHostGrid&) = delete;              // (G points into mem)
};
