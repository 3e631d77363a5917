// The per-triangle, per-node and per-walk text of the mesh queries (csrc/mesh_query.hip carries the contract): which triangles are live,
// the Morton key of a centroid, the radix tree over a sorted order, the watertight ray test, the closest point of a triangle, the two box
// bounds and the walk over the tree.  __host__ __device__ text that the kernels and the se3_debug_mesh_*_host entries both run; every
// float64 step is written out and fenced against contraction, so both give the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mesh_ops_core.h"        // mo_triangle (the first rule), mo_cross, mo_normalize; through pair_grid.h: PG_HD, pg_sqrt, pg_dist2

constexpr int kMqNodeBytes = 64;                    // SE3_MESH_QUERY_NODE_BYTES
constexpr int kMqKeyBits = 21;                      // SE3_MESH_QUERY_KEY_BITS: bits of a Morton key per axis
constexpr int kMqMaxDepth = 94;                     // SE3_MESH_QUERY_MAX_DEPTH: 63 key bits + 31 position bits
constexpr int kMqTrailBits = 128;                   // SE3_MESH_QUERY_TRAIL_BITS: what the walk keeps, one bit a level
constexpr int64_t kMqInertKey = -1;                 // no 63-bit key is negative: the caller's sort is by (key < 0, key)
constexpr double kMqDepthSlack = 0x1p-49;           // contract 6: 16 u of the largest depth of the box
constexpr double kMqPointSlack = 0x1p-48;           // contract 7: 32 u of the largest coordinate of the box, per axis
constexpr double kMqSquareSlack = 0x1p-50;          // contract 7: 8 u of the squared distance
static_assert(kMqMaxDepth < kMqTrailBits, "one trail bit per level of the deepest tree");

enum { kMqLive = 0, kMqBad = 1, kMqNonfinite = 2, kMqFlat = 3 };

// A node: the box of everything below it, its children and its parent as node numbers within its mesh (-1: none).  A leaf has
// left == right == -1 - (its triangle's number).  Mesh b's nodes start at 2 * (its first triangle row): the inner nodes at 0 .. live - 2,
// the leaf of sorted place j at m + j.
struct MqNode {
  double lo[3], hi[3];
  int left, right, parent, pad;
};
static_assert(sizeof(MqNode) == kMqNodeBytes, "a node is one 64-byte line");

// contract 1: the vertices of triangle t and what kind it is; only a live triangle has p0, p1, p2 and is ever tested
PG_HD int mq_triangle(const double* vertices, const int64_t* tri, int64_t t, int64_t n, const double** p0, const double** p1, const double** p2) {
  int w[3];
  if (!mo_triangle(tri, t, n, w)) return kMqBad;
  const double *a = vertices + 3 * (int64_t)w[0], *b = vertices + 3 * (int64_t)w[1], *c = vertices + 3 * (int64_t)w[2];
  for (int k = 0; k < 3; k++)
    if (!(fabs(a[k]) < INFINITY) || !(fabs(b[k]) < INFINITY) || !(fabs(c[k]) < INFINITY)) return kMqNonfinite;
  double x[3];
  mo_cross(a, b, c, x);
  if (x[0] == 0.0 && x[1] == 0.0 && x[2] == 0.0) return kMqFlat;
  *p0 = a, *p1 = b, *p2 = c;
  return kMqLive;
}

// contract 2: the centroid, (a + b) + c over 3, and its key
PG_HD void mq_centroid(const double* a, const double* b, const double* c, double* out) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; k++) {
    const double s = a[k] + b[k];
    const double t = s + c[k];
    out[k] = t / 3.0;
  }
}

PG_HD uint64_t mq_spread(uint64_t x) {          // 21 bits, two zeros behind each
  x &= 0x1fffffull;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}

// the cell of a coordinate among 2^21 between lo and hi (0 when the box is flat there or the quotient is no number); x is the high bit of three
PG_HD int64_t mq_key(const double* centroid, const double* lo, const double* hi) {
#pragma clang fp contract(off)
  uint64_t cell[3];
  for (int k = 0; k < 3; k++) {
    const double ext = hi[k] - lo[k], off = centroid[k] - lo[k];
    const double q = off / ext;
    const double f = floor(q * 2097152.0);
    cell[k] = !(f >= 0.0) ? 0 : (f >= 2097151.0 ? 2097151 : (uint64_t)f);
  }
  return (int64_t)(mq_spread(cell[0]) << 2 | mq_spread(cell[1]) << 1 | mq_spread(cell[2]));
}

// contract 4: the length of the common prefix of places i and j of the sorted keys: the keys' (as 64-bit words), and behind equal keys the
// places'; -1 outside [0, live)
PG_HD int mq_delta(const int64_t* keys, int64_t live, int64_t i, int64_t j) {
  if (j < 0 || j >= live) return -1;
  const uint64_t x = (uint64_t)keys[i] ^ (uint64_t)keys[j];
  if (x) return __builtin_clzll(x);
  return 64 + __builtin_clzll((uint64_t)(i ^ j));
}

// inner node i of `live` >= 2 sorted places: its children as node numbers (leaf of place j: m + j) and the range it covers
PG_HD void mq_topology(const int64_t* keys, int64_t live, int64_t m, int64_t i, int* left, int* right) {
  const int d = mq_delta(keys, live, i, i + 1) - mq_delta(keys, live, i, i - 1) >= 0 ? 1 : -1;
  const int floor_delta = mq_delta(keys, live, i, i - d);
  int64_t reach = 2;
  while (mq_delta(keys, live, i, i + reach * d) > floor_delta) reach *= 2;
  int64_t len = 0;
  for (int64_t step = reach / 2; step >= 1; step /= 2)
    if (mq_delta(keys, live, i, i + (len + step) * d) > floor_delta) len += step;
  const int64_t j = i + len * d;
  const int node_delta = mq_delta(keys, live, i, j);
  int64_t s = 0;
  for (int64_t step = (len + 1) / 2;; step = (step + 1) / 2) {
    if (mq_delta(keys, live, i, i + (s + step) * d) > node_delta) s += step;
    if (step <= 1) break;
  }
  const int64_t split = i + s * d + (d < 0 ? -1 : 0);
  const int64_t a = i < j ? i : j, b = i < j ? j : i;
  *left = (int)(a == split ? m + split : split);
  *right = (int)(b == split + 1 ? m + split + 1 : split + 1);
}

PG_HD void mq_leaf_box(const double* a, const double* b, const double* c, MqNode* node) {
  for (int k = 0; k < 3; k++) {
    const double lo = a[k] < b[k] ? a[k] : b[k], hi = a[k] < b[k] ? b[k] : a[k];
    node->lo[k] = c[k] < lo ? c[k] : lo, node->hi[k] = c[k] > hi ? c[k] : hi;
  }
}

// ---- a ray -----------------------------------------------------------------------------------------------------------------------------------
// contract 5.  The winner so far rides along: t, the triangle, the weights of its second and third vertex.
// (a per-lane array under a lane's own index would live in scratch memory: the three candidates are picked by comparisons instead)
PG_HD double mq_pick(const double* v, int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

struct MqRay {
  double ox, oy, oz, sx, sy, sz, t_min, t_max;          // the origin's kx, ky, kz components
  int kx, ky, kz;
  bool valid, any_hit;
  double t, u, v;
  int64_t tri;

  PG_HD void init(const double* ray, double lo, double hi, bool any) {
#pragma clang fp contract(off)
    t_min = lo, t_max = hi, any_hit = any, t = INFINITY, u = v = 0.0, tri = -1;
    valid = true;
    for (int k = 0; k < 3; k++) valid = valid && fabs(ray[k]) < INFINITY && fabs(ray[3 + k]) < INFINITY;
    const double* d = ray + 3;
    valid = valid && (d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0);
    kz = 0;
    if (valid) {
      double largest = fabs(d[0]);
      if (fabs(d[1]) > largest) kz = 1, largest = fabs(d[1]);
      if (fabs(d[2]) > largest) kz = 2;
    }
    kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    if (valid && mq_pick(d, kz) < 0.0) {
      const int s = kx;
      kx = ky, ky = s;
    }
    ox = mq_pick(ray, kx), oy = mq_pick(ray, ky), oz = mq_pick(ray, kz);
    const double dx = mq_pick(d, kx), dy = mq_pick(d, ky), dz = mq_pick(d, kz);
    sx = valid ? dx / dz : 0.0, sy = valid ? dy / dz : 0.0, sz = valid ? 1.0 / dz : 0.0;
  }
  PG_HD bool done() const { return any_hit && tri >= 0; }
  PG_HD bool better(double s, int64_t id) const { return s < t || (s == t && id < tri); }

  // a vertex relative to the origin, sheared and scaled: x, y and the depth
  PG_HD void shear(const double* p, double* x, double* y, double* z) const {
#pragma clang fp contract(off)
    const double ax = p[kx] - ox, ay = p[ky] - oy, az = p[kz] - oz;
    const double px = sx * az, py = sy * az;
    *x = ax - px, *y = ay - py, *z = sz * az;
  }
  PG_HD void triangle(const double* a, const double* b, const double* c, int64_t id) {
#pragma clang fp contract(off)
    double ax, ay, az, bx, by, bz, cx, cy, cz;
    shear(a, &ax, &ay, &az), shear(b, &bx, &by, &bz), shear(c, &cx, &cy, &cz);
    const double cxby = cx * by, cybx = cy * bx, axcy = ax * cy, aycx = ay * cx, bxay = bx * ay, byax = by * ax;
    const double U = cxby - cybx, V = axcy - aycx, W = bxay - byax;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return;
    const double uv = U + V;
    const double det = uv + W;
    if (det == 0.0) return;
    const double ua = U * az, vb = V * bz, wc = W * cz;
    const double s0 = ua + vb;
    const double T = s0 + wc;
    const double s = T / det;
    if (!(s >= t_min && s <= t_max) || !better(s, id)) return;
    t = s, tri = id, u = V / det, v = W / det;
  }
  // contract 6: false only when no triangle inside the box can become the winner
  PG_HD bool box(const MqNode& n) const {
#pragma clang fp contract(off)
    const double zl = mq_pick(n.lo, kz) - oz, zh = mq_pick(n.hi, kz) - oz;
    const double xa = sx * zl, xb = sx * zh, ya = sy * zl, yb = sy * zh;
    const double xlo = (mq_pick(n.lo, kx) - ox) - (xa > xb ? xa : xb), xhi = (mq_pick(n.hi, kx) - ox) - (xa > xb ? xb : xa);
    const double ylo = (mq_pick(n.lo, ky) - oy) - (ya > yb ? ya : yb), yhi = (mq_pick(n.hi, ky) - oy) - (ya > yb ? yb : ya);
    if (xlo > 0.0 || xhi < 0.0 || ylo > 0.0 || yhi < 0.0) return false;
    const double za = sz * zl, zb = sz * zh;
    const double near = za < zb ? za : zb, far = za < zb ? zb : za;
    const double big = fabs(near) > fabs(far) ? fabs(near) : fabs(far);
    const double slack = big * kMqDepthSlack;
    const double bound = t < t_max ? t : t_max;
    if (near - slack > bound || far + slack < t_min) return false;
    return true;
  }
  // what orders two children: the near end of the box's depths
  PG_HD double key(const MqNode& n) const {
#pragma clang fp contract(off)
    const double za = sz * (mq_pick(n.lo, kz) - oz), zb = sz * (mq_pick(n.hi, kz) - oz);
    return za < zb ? za : zb;
  }
};

// ---- a query point -------------------------------------------------------------------------------------------------------------------------------
PG_HD double mq_dot(const double* a, const double* b) {
#pragma clang fp contract(off)
  const double x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
  const double s = x + y;
  return s + z;
}

// contract 7: the region walk.  out: the point; *v, *w: the weights of b and c.
PG_HD void mq_closest_on_triangle(const double* p, const double* a, const double* b, const double* c, double* out, double* v, double* w) {
#pragma clang fp contract(off)
  double ab[3], ac[3], ap[3], bp[3], cp[3];
  for (int k = 0; k < 3; k++) ab[k] = b[k] - a[k], ac[k] = c[k] - a[k], ap[k] = p[k] - a[k];
  const double d1 = mq_dot(ab, ap), d2 = mq_dot(ac, ap);
  if (d1 <= 0.0 && d2 <= 0.0) {
    for (int k = 0; k < 3; k++) out[k] = a[k];
    *v = 0.0, *w = 0.0;
    return;
  }
  for (int k = 0; k < 3; k++) bp[k] = p[k] - b[k];
  const double d3 = mq_dot(ab, bp), d4 = mq_dot(ac, bp);
  if (d3 >= 0.0 && d4 <= d3) {
    for (int k = 0; k < 3; k++) out[k] = b[k];
    *v = 1.0, *w = 0.0;
    return;
  }
  const double d1d4 = d1 * d4, d3d2 = d3 * d2;
  const double vc = d1d4 - d3d2;
  if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    const double den = d1 - d3;
    const double s = d1 / den;
    for (int k = 0; k < 3; k++) {
      const double along = s * ab[k];
      out[k] = a[k] + along;
    }
    *v = s, *w = 0.0;
    return;
  }
  for (int k = 0; k < 3; k++) cp[k] = p[k] - c[k];
  const double d5 = mq_dot(ab, cp), d6 = mq_dot(ac, cp);
  if (d6 >= 0.0 && d5 <= d6) {
    for (int k = 0; k < 3; k++) out[k] = c[k];
    *v = 0.0, *w = 1.0;
    return;
  }
  const double d5d2 = d5 * d2, d1d6 = d1 * d6;
  const double vb = d5d2 - d1d6;
  if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    const double den = d2 - d6;
    const double s = d2 / den;
    for (int k = 0; k < 3; k++) {
      const double along = s * ac[k];
      out[k] = a[k] + along;
    }
    *v = 0.0, *w = s;
    return;
  }
  const double d3d6 = d3 * d6, d5d4 = d5 * d4;
  const double va = d3d6 - d5d4;
  const double e43 = d4 - d3, e56 = d5 - d6;
  if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {
    const double den = e43 + e56;
    const double s = e43 / den;
    for (int k = 0; k < 3; k++) {
      const double bc = c[k] - b[k];
      const double along = s * bc;
      out[k] = b[k] + along;
    }
    *v = 1.0 - s, *w = s;
    return;
  }
  const double sab = va + vb;
  const double sum = sab + vc;
  const double inv = 1.0 / sum;
  const double sv = vb * inv, sw = vc * inv;
  for (int k = 0; k < 3; k++) {
    const double pv = ab[k] * sv, pw = ac[k] * sw;
    const double q = a[k] + pv;
    out[k] = q + pw;
  }
  *v = sv, *w = sw;
}

struct MqPoint {
  double q[3];
  bool valid, any_hit;
  double d2, point[3], u, v;
  int64_t tri;

  PG_HD void init(const double* p) {
    valid = true, any_hit = false, d2 = INFINITY, u = v = 0.0, tri = -1;
    for (int k = 0; k < 3; k++) q[k] = p[k], point[k] = 0.0, valid = valid && fabs(p[k]) < INFINITY;
  }
  PG_HD bool done() const { return false; }
  PG_HD void triangle(const double* a, const double* b, const double* c, int64_t id) {
    double x[3], sv, sw;
    mq_closest_on_triangle(q, a, b, c, x, &sv, &sw);
    const double s = pg_dist2(q, x);
    if (!(s < d2 || (s == d2 && id < tri))) return;
    d2 = s, tri = id, u = sv, v = sw;
    for (int k = 0; k < 3; k++) point[k] = x[k];
  }
  // contract 7: a lower bound of every squared distance that a triangle inside the box can give
  PG_HD double key(const MqNode& n) const {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int k = 0; k < 3; k++) {
      const double below = n.lo[k] - q[k], above = q[k] - n.hi[k];
      double e = below > above ? below : above;
      const double big = fabs(n.lo[k]) > fabs(n.hi[k]) ? fabs(n.lo[k]) : fabs(n.hi[k]);
      e = e - big * kMqPointSlack;
      if (!(e > 0.0)) e = 0.0;
      s = s + e * e;
    }
    return s - s * kMqSquareSlack;
  }
  PG_HD bool box(const MqNode& n) const { return !(key(n) > d2); }
};

// ---- the walk ---------------------------------------------------------------------------------------------------------------------------------
// contract 8.  Depth first from the root; a leaf is tested where it is met; of two inner children that both pass, the one whose key() is
// smaller (the nearer one; the left one when equal) is entered first, and the one that waits is remembered by ONE bit of the trail at the
// level of its parent (and one bit that says which child it is), and found again by climbing the parent links.
// nodes, vertices, tri: the mesh's own; root: -1 for a mesh without a live triangle.
struct MqTrail {                                   // one bit a level, in two registers (an array under `level` would be scratch memory)
  uint64_t lo = 0, hi = 0;
  PG_HD bool test(int level) const { return ((level < 64 ? lo : hi) >> (level & 63)) & 1; }
  PG_HD void set(int level) {
    const uint64_t bit = 1ull << (level & 63);
    lo |= level < 64 ? bit : 0, hi |= level < 64 ? 0 : bit;
  }
  PG_HD void clear(int level) {
    const uint64_t bit = 1ull << (level & 63);
    lo &= ~(level < 64 ? bit : 0), hi &= ~(level < 64 ? 0 : bit);
  }
};

template <class Query>
PG_HD void mq_walk(const MqNode* nodes, int root, const double* vertices, const int64_t* tri, int64_t n, int64_t m, Query& Q) {
  if (root < 0) return;
  const double *a, *b, *c;
  auto leaf = [&](const MqNode& x) {
    const int64_t t = -1 - (int64_t)x.left;
    if (t < m && mq_triangle(vertices, tri, t, n, &a, &b, &c) == kMqLive) Q.triangle(a, b, c, t);
  };
  const int64_t node_count = 2 * m;
  MqNode top = nodes[root];
  if (!Q.box(top)) return;
  if (top.left < 0) {
    leaf(top);
    return;
  }
  MqTrail trail, swapped;
  int level = 0, cur = root, left = top.left, right = top.right;
  for (;;) {
    // (a table is trusted no further than its own size: a child outside it ends the walk)
    if (left < 0 || left >= node_count || right < 0 || right >= node_count || level >= kMqTrailBits - 1) return;
    const MqNode x = nodes[left], y = nodes[right];
    bool go_x = Q.box(x), go_y = Q.box(y);
    if (go_x && x.left < 0) {
      leaf(x), go_x = false;
      if (Q.done()) return;
      go_y = go_y && Q.box(y);
    }
    if (go_y && y.left < 0) {
      leaf(y), go_y = false;
      if (Q.done()) return;
    }
    if (go_x || go_y) {
      bool first_x = go_x;
      if (go_x && go_y) {
        trail.set(level);
        if (Q.key(y) < Q.key(x)) first_x = false, swapped.set(level);
      }
      cur = first_x ? left : right;
      left = first_x ? x.left : y.left, right = first_x ? x.right : y.right;
      level++;
      continue;
    }
    for (;;) {                                                            // climb to the deepest level where a child waits
      if (level == 0) return;
      cur = nodes[cur].parent;
      level--;
      if (cur < 0 || cur >= node_count) return;
      if (!trail.test(level)) continue;
      trail.clear(level);
      const bool was_swapped = swapped.test(level);
      swapped.clear(level);
      const int next = was_swapped ? nodes[cur].left : nodes[cur].right;
      if (next < 0 || next >= node_count) return;
      const MqNode z = nodes[next];
      if (z.left < 0 || !Q.box(z)) continue;
      cur = next, left = z.left, right = z.right, level++;
      break;
    }
  }
}

// every triangle in ascending order: the yardstick of the host entries
template <class Query>
PG_HD void mq_brute(const double* vertices, const int64_t* tri, int64_t n, int64_t m, Query& Q) {
  const double *a, *b, *c;
  for (int64_t t = 0; t < m && !Q.done(); t++)
    if (mq_triangle(vertices, tri, t, n, &a, &b, &c) == kMqLive) Q.triangle(a, b, c, t);
}

// the normal of the winner: cross(b - a, c - a) over its length
PG_HD void mq_normal(const double* vertices, const int64_t* tri, int64_t n, int64_t t, double* out) {
  mo_triangle_normal(vertices, tri, t, n, out);
  mo_normalize(out);
}
