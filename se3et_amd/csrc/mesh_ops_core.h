// The per-row work of the mesh post-processing entries (csrc/mesh_ops.hip carries the contract): the bounds rule of a triangle, the
// canonical incidence rows, the edge test and the union of the connected components, areas and normals, one smoothing step of a vertex.
// __host__ __device__ text that the kernels and the se3_debug_mesh_*_host entries both run; every float64 step is
// written out and fenced against contraction, so both give the same bits.
//
// A mesh of n vertices and m triangles names its vertices 0 .. n - 1; rows hold mesh-local numbers as ints (n, m < 2^31).
#pragma once
#include <math.h>
#include <stdint.h>

#include "dbscan_core.h"          // db_find / db_union; through pair_grid.h: PG_HD, pg_sqrt
#include "voxel_key.h"            // vd_origin, vd_axis_ok, vd_key_xyz: the cells of vertex clustering

constexpr int kMoAreaLanes = 64;                    // lanes of the area reduction tree (SE3_MESH_OPS_AREA_LANES)

// The first rule: the vertices of triangle t, or false when one of them is outside [0, n).  Nothing indexes a vertex array or a row table
// with a number that did not come through here.
PG_HD bool mo_triangle(const int64_t* tri, int64_t t, int64_t n, int* v) {
  const int64_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
  if (a < 0 || a >= n || b < 0 || b >= n || c < 0 || c >= n) return false;
  v[0] = (int)a, v[1] = (int)b, v[2] = (int)c;
  return true;
}

// triangle t as a row of a table names it: t itself must lie in [0, m) first (a table is trusted no further than that)
PG_HD bool mo_row_triangle(const int64_t* tri, int64_t m, int64_t n, int t, int* v) { return t >= 0 && t < m && mo_triangle(tri, t, n, v); }

// the distinct vertices of a triangle in the order of their first appearance: (a, a, b) is incident to a once
PG_HD int mo_distinct(const int* v, int* d) {
  int k = 0;
  d[k++] = v[0];
  if (v[1] != v[0]) d[k++] = v[1];
  if (v[2] != v[0] && v[2] != v[1]) d[k++] = v[2];
  return k;
}

PG_HD bool mo_names(const int* v, int a) { return v[0] == a || v[1] == a || v[2] == a; }

// ascending, in place; the entries are distinct.  Quadratic in the length: rows arrive almost ordered, and a valence is small.
PG_HD void mo_sort_row(int* row, int64_t len) {
  for (int64_t a = 1; a < len; a++) {
    const int x = row[a];
    int64_t b = a;
    for (; b > 0 && row[b - 1] > x; b--) row[b] = row[b - 1];
    row[b] = x;
  }
}

// The neighbours of vertex v: the distinct other vertices of the triangles of its incident row (ascending), the count as the result and,
// with `out`, the numbers in ascending order.  A vertex is new when no earlier triangle of the row and no earlier corner of this triangle
// names it: no storage for the count pass, and len^2 triangle reads.  Nothing is written at or past out[cap].
PG_HD int mo_neighbors(const int64_t* tri, int64_t m, int64_t n, const int* row, int64_t len, int v, int* out, int64_t cap) {
  int count = 0;
  for (int64_t k = 0; k < len; k++) {
    int w[3];
    if (!mo_row_triangle(tri, m, n, row[k], w)) continue;
    for (int j = 0; j < 3; j++) {
      const int u = w[j];
      bool seen = u == v;
      for (int e = 0; e < j && !seen; e++) seen = w[e] == u;
      for (int64_t e = 0; e < k && !seen; e++) {
        int x[3];
        seen = mo_row_triangle(tri, m, n, row[e], x) && mo_names(x, u);
      }
      if (seen) continue;
      if (out && count < cap) {
        int b = count;
        for (; b > 0 && out[b - 1] > u; b--) out[b] = out[b - 1];
        out[b] = u;
      }
      count++;
    }
  }
  return count;
}

// Triangle t becomes one set with every triangle of a lower number that shares an undirected edge {a, b}, a != b, with it: the lower
// triangles of a's incident row (ascending: the walk stops at t) that also name b.  The relation is symmetric, so the lower side is enough.
template <class Load, class Lower, class Cas>
PG_HD void mo_link_triangle(const int64_t* tri, int64_t m, int64_t n, int t, const int64_t* tri_offsets, const int* tri_rows, Load&& load, Lower&& lower,
                            Cas&& cas) {
  int w[3];
  if (!mo_triangle(tri, t, n, w)) return;
  for (int e = 0; e < 3; e++) {
    const int a = w[e], b = w[e == 2 ? 0 : e + 1];
    if (a == b) continue;
    const int* row = tri_rows + tri_offsets[a];
    const int64_t len = tri_offsets[a + 1] - tri_offsets[a];
    for (int64_t k = 0; k < len && row[k] < t; k++) {
      int x[3];
      if (mo_row_triangle(tri, m, n, row[k], x) && mo_names(x, b)) db_union(t, row[k], load, lower, cas);
    }
  }
}

// cross(v1 - v0, v2 - v0): every difference, product and difference of products rounded on its own
PG_HD void mo_cross(const double* p0, const double* p1, const double* p2, double* out) {
#pragma clang fp contract(off)
  const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
  const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
  const double yz = ay * bz, zy = az * by, zx = az * bx, xz = ax * bz, xy = ax * by, yx = ay * bx;
  out[0] = yz - zy, out[1] = zx - xz, out[2] = xy - yx;
}

PG_HD double mo_norm(const double* v) {
#pragma clang fp contract(off)
  const double xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
  const double a = xx + yy;
  return pg_sqrt(a + zz);
}

// v / |v|; (0, 0, 1) when the length is zero or not a number (Open3D's NormalizeNormals)
PG_HD void mo_normalize(double* v) {
  const double r = mo_norm(v);
  if (!(r > 0.0) || !(r < INFINITY)) {
    v[0] = 0.0, v[1] = 0.0, v[2] = 1.0;
    return;
  }
  v[0] = v[0] / r, v[1] = v[1] / r, v[2] = v[2] / r;
}

// the un-normalised normal of triangle t (zero for a triangle out of range) of the mesh whose vertices start at `vertices`
PG_HD void mo_triangle_normal(const double* vertices, const int64_t* tri, int64_t t, int64_t n, double* out) {
  int w[3];
  out[0] = out[1] = out[2] = 0.0;
  if (mo_triangle(tri, t, n, w)) mo_cross(vertices + 3 * (int64_t)w[0], vertices + 3 * (int64_t)w[1], vertices + 3 * (int64_t)w[2], out);
}

PG_HD double mo_triangle_area(const double* vertices, const int64_t* tri, int64_t t, int64_t n) {
  double c[3];
  mo_triangle_normal(vertices, tri, t, n, c);
  return 0.5 * mo_norm(c);
}

// the normal of a vertex: the sum of the un-normalised normals of its incident row, in row order, then normalised
PG_HD void mo_vertex_normal(const double* vertices, const int64_t* tri, int64_t m, int64_t n, const int* row, int64_t len, double* out) {
#pragma clang fp contract(off)
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t k = 0; k < len; k++) {
    double c[3] = {0.0, 0.0, 0.0};
    if (row[k] >= 0 && row[k] < m) mo_triangle_normal(vertices, tri, row[k], n, c);
    s[0] += c[0], s[1] += c[1], s[2] += c[2];
  }
  mo_normalize(s);
  out[0] = s[0], out[1] = s[1], out[2] = s[2];
}

// One smoothing step of vertex v of the mesh whose rows start at `src`: s = the sum over the neighbour row in row order; simple:
// (x + s) / (len + 1); otherwise x + lambda (s / len - x).  An empty row keeps x.  A row entry outside [0, n) (no table of
// se3_mesh_incidence_stack holds one) is passed over, not read through.
PG_HD void mo_smooth(const double* src, int64_t n, int v, const int* row, int64_t len, bool simple, double lambda, double* out) {
#pragma clang fp contract(off)
  const double* x = src + 3 * (int64_t)v;
  if (len == 0) {
    for (int d = 0; d < 3; d++) out[d] = x[d];
    return;
  }
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t k = 0; k < len; k++) {
    if (row[k] < 0 || row[k] >= n) continue;
    const double* p = src + 3 * (int64_t)row[k];
    for (int d = 0; d < 3; d++) s[d] += p[d];
  }
  for (int d = 0; d < 3; d++) {
    if (simple) {
      const double t = x[d] + s[d];
      out[d] = t / (double)(len + 1);
    } else {
      const double mean = s[d] / (double)len;
      const double diff = mean - x[d];
      const double step = lambda * diff;
      out[d] = x[d] + step;
    }
  }
}

// The sum of a[0, count) by the fixed tree of the cluster areas: lane l of kMoAreaLanes adds a[l], a[l + 64], .. in that order, then the
// lanes are added by the butterfly of se3_wave_sum (offsets 32, 16, .. 1).  The host's form; the device runs one wave.
inline double mo_tree_sum_host(const double* a, int64_t count) {
  double lane[kMoAreaLanes], next[kMoAreaLanes];
  for (int l = 0; l < kMoAreaLanes; l++) {
    double s = 0.0;
    for (int64_t i = l; i < count; i += kMoAreaLanes) s += a[i];
    lane[l] = s;
  }
  for (int o = kMoAreaLanes / 2; o > 0; o >>= 1) {
    for (int l = 0; l < kMoAreaLanes; l++) next[l] = lane[l] + lane[l ^ o];
    for (int l = 0; l < kMoAreaLanes; l++) lane[l] = next[l];
  }
  return lane[0];
}

// ---- vertex clustering ------------------------------------------------------------------------------------------------------------------------------
// the mean of the rows members[0 .. count) (mesh-local numbers from `base` on, ascending) of `src`: summed in that order, divided once; a
// member outside [0, n) is passed over
PG_HD void mo_cluster_mean(const double* src, int64_t n, const int64_t* members, int64_t base, int64_t count, double* out) {
#pragma clang fp contract(off)
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t k = 0; k < count; k++) {
    const int64_t v = members[k] - base;
    if (v < 0 || v >= n) continue;
    for (int d = 0; d < 3; d++) s[d] += src[3 * v + d];
  }
  for (int d = 0; d < 3; d++) out[d] = s[d] / (double)count;
}

// a remapped triangle rotated, not sorted, so that its lowest vertex comes first (the orientation stays); false when two of its vertices are equal
PG_HD bool mo_rotate(int64_t a, int64_t b, int64_t c, int64_t* out) {
  if (a == b || b == c || a == c) return false;
  if (a < b && a < c) out[0] = a, out[1] = b, out[2] = c;
  else if (b < c) out[0] = b, out[1] = c, out[2] = a;
  else out[0] = c, out[1] = a, out[2] = b;
  return true;
}
