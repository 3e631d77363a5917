// Ray casting and closest-point queries on stacked triangle meshes (Open3D's RaycastingScene: cast_rays, test_occlusions,
// compute_closest_points, compute_distance, and a depth rendering), up to SE3_PAIR_MAX_PAIRS meshes per call, over a bounding volume
// hierarchy that is built on the device.  se3et_amd/mesh_query.py is the front end; csrc/mesh_query_core.h holds the text that the kernels
// and the se3_debug_mesh_*_host entries share.
// (SE3_EXACT_FP: the file is built with contraction off, and the core fences itself as well.)
//
// Layout.  The meshes as csrc/mesh_ops.hip takes them: vertices (sum n, 3) float64, triangles (sum m, 3) int64 naming vertices by their
// number within their own mesh, the cuts as host offsets (B + 1); n, m < 2^31 per mesh.  nodes: 2 sum m nodes of 64 bytes, mesh b's from
// node 2 triangle_offsets[b] on.  counts (B, SE3_MESH_OPS_COUNT_WORDS) int64: status, live triangles, zero-area triangles, root.  Everything
// is float64 except the rendered depth.
//
// Contract.
//   1. The first rule is csrc/mesh_ops.hip's: mo_triangle is the only way from a triangle to vertex numbers.  Three kinds of triangle are
//      INERT: one that names a vertex outside [0, n) (status bit SE3_MESH_OPS_BAD_TRIANGLE), one with a vertex that is not finite (status
//      bit SE3_MESH_QUERY_NONFINITE_VERTEX; Python raises ValueError for either), and one whose cross(b - a, c - a) (mo_cross) is exactly
//      zero (counted in word 2, no error).  An inert triangle is in no leaf, is never hit and is never closest.  A mesh without a live
//      triangle has root -1: every ray misses, every query point gets distance inf and primitive -1.
//   2. Keys.  The centroid of a live triangle is ((a + b) + c) / 3 per axis.  Per mesh, lo and hi are the min and max of the live centroids
//      (the box reduction of block_ops.h; min and max are exact, so the order of the reduction does not matter).  The cell of an axis is
//      floor(((x - lo) / (hi - lo)) 2^21) kept inside [0, 2^21 - 1] (0 where hi == lo); the key interleaves the three cells, x highest, into
//      63 bits.  An inert triangle gets key -1.
//   3. The caller sorts each mesh's triangles by (key < 0, key), stable: the live triangles in key order, equal keys in triangle order, then
//      the inert ones.  (torch.sort in ops.py; everything that touches a float is HIP.)
//   4. Topology (Karras 2012), one thread per inner node.  delta(i, j) of two sorted places is the number of leading bits that their keys
//      share as 64-bit words, and 64 + the leading bits that i and j share as 64-bit words when the keys are equal; -1 when j is outside
//      [0, live).  The tree is a function of the sorted keys alone.  Inner node i of a mesh is its node i (the root is node 0), the leaf of
//      sorted place j is node m + j and holds -1 - (triangle number) in both child words; a mesh with ONE live triangle has the leaf m as its root.
//   5. Boxes.  A leaf's box is the min and max of its triangle's three vertices; an inner node's is the min and max of its children's,
//      computed by the second of its children's threads to arrive at the node's counter (the call clears the counters).  min and max are
//      exact, so the boxes do not depend on who arrives first: the build is bit-identical run to run, alone and in a batch.  (The first
//      arrival's box reaches the second through agent-scope stores and loads around the counter's atomic add, with a fence on each side:
//      the two threads may sit on chiplets whose L2 caches are not coherent.)
//   6. Ray against triangle: the watertight test of Woop, Benthin and Wald (2013).  kz = the axis of the largest |d| (the lowest such axis);
//      kx, ky the next two in cyclic order, swapped when d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].  A vertex p becomes
//      A = p - o, x = A[kx] - Sx A[kz], y = A[ky] - Sy A[kz], z = Sz A[kz].  U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax, every
//      product and difference rounded on its own (this is why contraction is off: the two sides of a shared edge compute exact negatives of
//      each other, so no ray slips between them).  A miss when some of U, V, W is negative and some positive, or when det = (U + V) + W is
//      zero.  Otherwise t = ((U Az + V Bz) + W Cz) / det, a hit when t_min <= t <= t_max.  Zeros count as inside: a ray through a shared edge
//      hits both neighbours.  Both faces are hit.  The winner of a ray is the smallest computed t, among equal t the lowest triangle number;
//      uvs = (V / det, W / det), the weights of the second and third vertex; the normal is cross(b - a, c - a) over its length (pg_sqrt).  A
//      ray whose origin or direction is not finite, or whose direction is zero, is a miss.  A miss holds t inf, primitive -1, uvs and normal 0.
//      The box of a ray.  Rounding is monotone: p -> fl(p - o) does not decrease in p, a product with a fixed factor is monotone, so the
//      x, y and z that THE TEXT ABOVE computes for any vertex inside a box lie between the values that the same operations give for the
//      box's ends (interval arithmetic with the triangle's own roundings; no real-number geometry enters).  A node is skipped
//        (a) when that interval of x or of y lies strictly on one side of zero: then Ax, Bx, Cx (or the ys) of every triangle below have one
//            strict sign, the ray's line does not pierce the triangle's projection, and U, V, W cannot agree in sign unless products that
//            differ exactly round to the same number (see Limits);
//        (b) when near - slack > min(best t, t_max) or far + slack < t_min, strictly, where [near, far] is the interval of z and slack =
//            2^-49 max(|near|, |far|).  The margin: with U, V, W of one sign, t is a weighted mean of Az, Bz, Cz computed with three rounded
//            products, two rounded sums, the two sums of det and one division: |t - mean| <= 7 u max|z| + O(u^2), u = 2^-53; the slack is
//            16 u max|z|.  A node at exactly the best t is visited, because a lower triangle number may tie.
//   7. Point against triangle: the region walk of Ericson, Real-Time Collision Detection 5.1.5, as mq_closest_on_triangle writes it out
//      (dots as (x x' + y y') + z z'); a vertex region returns the vertex itself.  d2 = pg_dist2(q, point); the winner is the smallest computed
//      d2, among equal d2 the lowest triangle number; the distance is pg_sqrt(d2).  A query point that is not finite gets NaN, NaN, -1, NaN, NaN.
//      The box of a point.  The returned point is a + v ab + w ac (or an edge's form) with computed weights in [0, 1] whose sum is at most
//      1 + 2 u: a convex combination up to at most 20 u of the largest |coordinate| of the box per axis.  So per axis e = max(lo - q, q - hi)
//      less 2^-48 max(|lo|, |hi|) (32 u), not below 0, bounds |q - point| from below, and (sum e^2)(1 - 2^-50) bounds the computed d2 (three
//      rounded squares and two sums: 4 u) from below.  A node is skipped only when that bound is strictly above the best d2.
//   8. The walk: one lane per ray or query point, depth first, no stack.  A leaf is tested where it is met.  When both children of a node
//      are inner nodes that pass their box test, the walk goes into the nearer one (the smaller near depth, or the smaller distance bound;
//      the left one when equal) and sets the bit of the node's LEVEL in a 128-bit trail, and in a second such word whether the child that
//      waits is the left one; at a dead end it climbs the parent links to the deepest level whose bit is set, clears it, tests the waiting
//      child's box again (the winner may have improved) and goes on there.  Depth bound: along a path from the root delta strictly grows, it takes the values
//      1 .. 63 while keys differ and 64 + 33 .. 64 + 63 behind equal keys (places are below 2^31), so a path has at most 63 + 31 = 94 inner
//      nodes and levels 0 .. 93 fit the trail at any shape of tree; the two trails are four registers, there is no per-lane array and no
//      scratch memory.  The order of the children cannot change the result under the rules of 6 and 7 (measured: the nearer child first
//      against the left child first gave the same bits and 0.88, 0.52 and 0.015 of the time: DESIGN.md).
//   9. Rendering.  A pixel's ray is rc_ray's of csrc/tsdf_raycast_core.h: origin the pose's translation, direction R (xr, yr, 1), so t IS the
//      depth along the camera's axis; t_min = depth_min, t_max = depth_max; point = origin + t dir (rc_point); the normal is the geometric
//      one (not turned towards the camera).  A pixel without a hit holds depth 0, NaN point and normal, primitive -1, mask 0.
//   Limits of the claim "the walk returns what the brute force over all triangles returns, bit for bit": it is proven for 6 (b) and 7 given
//   no overflow or underflow in the products; 6 (a) rests on the per-triangle test itself not reporting a hit for a triangle whose three
//   computed x (or y) are all strictly positive or all strictly negative, which exact arithmetic forbids and rounding allows only when a
//   triangle is seen exactly edge-on and two different products of an edge function round to one number.
//   Alone or in a batch, and from run to run, every output has the same bits: the only atomics are integer counts and arrival counters.
#include <math.h>
#include <string.h>

#include <vector>

#include "block_ops.h"
#include "common.h"
#include "mesh_query_core.h"
#include "tsdf_raycast_core.h"

namespace {

constexpr int kMqThreads = 256;
constexpr int kMqBoundsThreads = 256;
constexpr int kMqWalkThreads = 128;
constexpr int kMqRenderThreads = kRaycastTile * kRaycastTile;
constexpr int64_t kMqMaxRows = 1ll << 31;
constexpr int kMqCounts = SE3_MESH_OPS_COUNT_WORDS;
static_assert(kMqNodeBytes == SE3_MESH_QUERY_NODE_BYTES && kMqKeyBits == SE3_MESH_QUERY_KEY_BITS && kMqMaxDepth == SE3_MESH_QUERY_MAX_DEPTH &&
                  kMqTrailBits == SE3_MESH_QUERY_TRAIL_BITS,
              "mesh_query_core.h and include/se3et_hip.h name the same limits");
static_assert(kMqCounts == 4 && kRaycastTile == SE3_RAYCAST_TILE && kMqRenderThreads == 256, "four count words; a tile of 16 x 16 pixels");

struct MqCall {
  PairRows v, t;
  int64_t n_total, m_total;
};

int mq_call(const char* what, bool pointers, const int64_t* vertex_offsets, const int64_t* triangle_offsets, int num_meshes, MqCall* c) {
  SE3_REQUIRE(pointers && vertex_offsets && triangle_offsets, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(num_meshes >= 0 && num_meshes <= kPairMaxPairs, SE3_ERR_INVALID_ARG, "%s: %d meshes (at most %d)", what, num_meshes, kPairMaxPairs);
  SE3_REQUIRE(pg_fill_rows(&c->v, vertex_offsets, num_meshes) && pg_fill_rows(&c->t, triangle_offsets, num_meshes), SE3_ERR_INVALID_ARG,
              "%s: offsets must start at 0 and not decrease", what);
  for (int b = 0; b < num_meshes; b++)
    SE3_REQUIRE(c->v.start[b + 1] - c->v.start[b] < kMqMaxRows && c->t.start[b + 1] - c->t.start[b] < kMqMaxRows, SE3_ERR_UNSUPPORTED,
                "%s: mesh %d has 2^31 vertices or triangles or more", what, b);
  c->n_total = c->v.start[num_meshes], c->m_total = c->t.start[num_meshes];
  return SE3_OK;
}

inline unsigned mq_blocks(int64_t rows, int threads) { return (unsigned)se3_cdiv(rows, threads); }
inline size_t mq_atleast1(int64_t v) { return (size_t)(v > 0 ? v : 1); }

#define MQ_MEMSET(ptr, value, bytes, what)                                   \
  do {                                                                        \
    if (hipMemsetAsync(ptr, value, bytes, st) != hipSuccess) {                \
      se3_set_error("%s: hipMemsetAsync failed", what);                       \
      return SE3_ERR_LAUNCH;                                                  \
    }                                                                         \
  } while (0)

struct BvhLayout {
  double* boxes;       // [kPairMaxPairs][6]: lo and hi of the live centroids
  int* arrivals;       // [m_total]: the counter of inner node i of mesh b at triangle row start + i
};

size_t mq_bvh_carve(int64_t m_total, char* base, BvhLayout* L) {
  Se3Carver c(base);
  BvhLayout l;
  l.boxes = c.take<double>(6 * kPairMaxPairs);
  l.arrivals = c.take<int>(mq_atleast1(m_total));
  if (L) *L = l;
  return c.bytes();
}

// the status bit of an inert kind (0: none)
PG_HD int64_t mq_status_of(int kind) { return kind == kMqBad ? SE3_MESH_OPS_BAD_TRIANGLE : (kind == kMqNonfinite ? SE3_MESH_QUERY_NONFINITE_VERTEX : 0); }

// ---- the build ---------------------------------------------------------------------------------------------------------------------------------
// one workgroup per mesh: the kinds of its triangles and the box of the live centroids
__global__ __launch_bounds__(kMqBoundsThreads) void mesh_bvh_bounds_kernel(const double* __restrict__ vertices, const int64_t* __restrict__ tri, MqCall c,
                                                                           double* __restrict__ boxes, int64_t* __restrict__ counts) {
  __shared__ double sh[kMqBoundsThreads / 64];
  const int b = blockIdx.x;
  const int64_t v0 = c.v.start[b], n = c.v.start[b + 1] - v0, t0 = c.t.start[b], m = c.t.start[b + 1] - t0;
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  int64_t status = 0, live = 0, flat = 0;
  for (int64_t t = threadIdx.x; t < m; t += kMqBoundsThreads) {
    const double *p0, *p1, *p2;
    const int kind = mq_triangle(vertices + 3 * v0, tri + 3 * t0, t, n, &p0, &p1, &p2);
    status |= mq_status_of(kind), flat += kind == kMqFlat;
    if (kind != kMqLive) continue;
    double x[3];
    mq_centroid(p0, p1, p2, x);
    for (int k = 0; k < 3; k++) mn[k] = fmin(mn[k], x[k]), mx[k] = fmax(mx[k], x[k]);
    live++;
  }
  se3_block_bounds<double, kMqBoundsThreads>(mn, mx, sh);
  if (threadIdx.x == 0)
    for (int k = 0; k < 3; k++) boxes[6 * b + k] = mn[k], boxes[6 * b + 3 + k] = mx[k];
  if (status) atomicOr((unsigned long long*)(counts + kMqCounts * b), (unsigned long long)status);
  if (live) atomicAdd((unsigned long long*)(counts + kMqCounts * b + 1), (unsigned long long)live);
  if (flat) atomicAdd((unsigned long long*)(counts + kMqCounts * b + 2), (unsigned long long)flat);
}

__global__ __launch_bounds__(kMqThreads) void mesh_bvh_keys_kernel(const double* __restrict__ vertices, const int64_t* __restrict__ tri, MqCall c,
                                                                   const double* __restrict__ boxes, int64_t* __restrict__ keys) {
  const int64_t t = (int64_t)blockIdx.x * kMqThreads + threadIdx.x;
  if (t >= c.m_total) return;
  const int b = pg_pair_of_row(c.t, t);
  const double *p0, *p1, *p2;
  int64_t key = kMqInertKey;
  if (mq_triangle(vertices + 3 * c.v.start[b], tri + 3 * c.t.start[b], t - c.t.start[b], c.v.start[b + 1] - c.v.start[b], &p0, &p1, &p2) == kMqLive) {
    double x[3];
    mq_centroid(p0, p1, p2, x);
    key = mq_key(x, boxes + 6 * b, boxes + 6 * b + 3);
  }
  keys[t] = key;
}

// the live count of a mesh as the tree pass trusts it: within [0, m]
PG_HD int64_t mq_live(const int64_t* counts, int b, int64_t m) {
  const int64_t live = counts[kMqCounts * b + 1];
  return live < 0 ? 0 : (live > m ? m : live);
}
PG_HD int mq_root_of(int64_t live, int64_t m) { return live >= 2 ? 0 : (live == 1 ? (int)m : -1); }

// one thread per mesh: its root
__global__ void mesh_bvh_roots_kernel(MqCall c, MqNode* __restrict__ nodes, int64_t* __restrict__ counts) {
  const int b = threadIdx.x;
  if (b >= c.t.n) return;
  const int64_t t0 = c.t.start[b], m = c.t.start[b + 1] - t0;
  const int root = mq_root_of(mq_live(counts, b, m), m);
  counts[kMqCounts * b + 3] = root;
  if (root >= 0) nodes[2 * t0 + root].parent = -1;
}

// one thread per sorted place: the children of inner node i and their parent links
__global__ __launch_bounds__(kMqThreads) void mesh_bvh_topology_kernel(MqCall c, const int64_t* __restrict__ sorted_keys, MqNode* __restrict__ nodes,
                                                                       const int64_t* __restrict__ counts) {
  const int64_t t = (int64_t)blockIdx.x * kMqThreads + threadIdx.x;
  if (t >= c.m_total) return;
  const int b = pg_pair_of_row(c.t, t);
  const int64_t t0 = c.t.start[b], m = c.t.start[b + 1] - t0, i = t - t0, live = mq_live(counts, b, m);
  MqNode* N = nodes + 2 * t0;
  if (i >= live - 1) return;
  int left, right;
  mq_topology(sorted_keys + t0, live, m, i, &left, &right);
  N[i].left = left, N[i].right = right;
  N[left].parent = (int)i, N[right].parent = (int)i;
}

// one thread per sorted place: its leaf, then upwards as long as it is the second to arrive (contract 5)
__global__ __launch_bounds__(kMqThreads) void mesh_bvh_refit_kernel(const double* __restrict__ vertices, const int64_t* __restrict__ tri, MqCall c,
                                                                    const int64_t* __restrict__ order, MqNode* nodes, int* arrivals,
                                                                    const int64_t* __restrict__ counts) {
  const int64_t t = (int64_t)blockIdx.x * kMqThreads + threadIdx.x;
  if (t >= c.m_total) return;
  const int b = pg_pair_of_row(c.t, t);
  const int64_t t0 = c.t.start[b], m = c.t.start[b + 1] - t0, j = t - t0, live = mq_live(counts, b, m);
  if (j >= live) return;
  MqNode* N = nodes + 2 * t0;
  const int64_t id = order[t] - t0;
  const double *p0, *p1, *p2;
  if (id < 0 || id >= m || mq_triangle(vertices + 3 * c.v.start[b], tri + 3 * t0, id, c.v.start[b + 1] - c.v.start[b], &p0, &p1, &p2) != kMqLive)
    return;                                                               // (an order that is not the sort of this mesh's keys: its tree stays unfinished)
  MqNode mine;
  mq_leaf_box(p0, p1, p2, &mine);
  int self = (int)(m + j);
  for (int k = 0; k < 3; k++) {
    __hip_atomic_store(&N[self].lo[k], mine.lo[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&N[self].hi[k], mine.hi[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  N[self].left = N[self].right = (int)(-1 - id);
  int parent = N[self].parent;
  for (int level = 0; level <= kMqMaxDepth && parent >= 0 && parent < live - 1; level++) {
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int earlier = atomicAdd(arrivals + t0 + parent, 1);
    if (earlier == 0) return;
    __threadfence();
    const int left = N[parent].left, right = N[parent].right;
    const int other = left == self ? right : left;
    if (other < 0 || other >= 2 * m) return;
    for (int k = 0; k < 3; k++) {
      const double lo = __hip_atomic_load(&N[other].lo[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const double hi = __hip_atomic_load(&N[other].hi[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      mine.lo[k] = lo < mine.lo[k] ? lo : mine.lo[k], mine.hi[k] = hi > mine.hi[k] ? hi : mine.hi[k];
      __hip_atomic_store(&N[parent].lo[k], mine.lo[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&N[parent].hi[k], mine.hi[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    self = parent, parent = N[self].parent;
  }
}

// ---- the queries ---------------------------------------------------------------------------------------------------------------------------------
struct MqTree {
  const double* vertices;
  const int64_t* tri;
  const MqNode* nodes;
  const int64_t* counts;
};

// the walk of one query over mesh b (nothing for a mesh outside the call or a root outside its table)
template <class Query>
__device__ __forceinline__ void mq_query(const MqTree& T, const MqCall& c, int b, Query& Q) {
  if (b < 0 || b >= c.t.n || !Q.valid) return;
  const int64_t t0 = c.t.start[b], m = c.t.start[b + 1] - t0, v0 = c.v.start[b], root = T.counts[kMqCounts * b + 3];
  if (root < 0 || root >= 2 * m) return;
  mq_walk(T.nodes + 2 * t0, (int)root, T.vertices + 3 * v0, T.tri + 3 * t0, c.v.start[b + 1] - v0, m, Q);
}

struct RayOut {
  double* t;
  int64_t* ids;
  double *uvs, *normals;
  uint8_t* hit;
};

// vertices, tri, n: the mesh of the ray; a ray without a mesh has missed
PG_HD void mq_store_ray(const MqRay& Q, const double* vertices, const int64_t* tri, int64_t n, int64_t r, const RayOut& out) {
  const bool ok = Q.tri >= 0;
  double normal[3] = {0.0, 0.0, 0.0};
  if (ok && out.normals) mq_normal(vertices, tri, n, Q.tri, normal);
  if (out.hit) out.hit[r] = ok ? 1 : 0;
  if (out.t) out.t[r] = ok ? Q.t : (double)INFINITY;
  if (out.ids) out.ids[r] = ok ? Q.tri : -1;
  if (out.uvs) out.uvs[2 * r] = ok ? Q.u : 0.0, out.uvs[2 * r + 1] = ok ? Q.v : 0.0;
  if (out.normals)
    for (int k = 0; k < 3; k++) out.normals[3 * r + k] = normal[k];
}

__global__ __launch_bounds__(kMqWalkThreads) void mesh_cast_rays_kernel(MqTree T, MqCall c, const double* __restrict__ rays, const int* __restrict__ ray_meshes,
                                                                        int64_t num_rays, double t_min, double t_max, int any_hit, RayOut out) {
  const int64_t r = (int64_t)blockIdx.x * kMqWalkThreads + threadIdx.x;
  if (r >= num_rays) return;
  int b = ray_meshes[r];
  MqRay Q;
  Q.init(rays + 6 * r, t_min, t_max, any_hit != 0);
  mq_query(T, c, b, Q);
  if (b < 0 || b >= c.t.n) b = 0, Q.tri = -1;
  mq_store_ray(Q, T.vertices + 3 * c.v.start[b], T.tri + 3 * c.t.start[b], c.v.start[b + 1] - c.v.start[b], r, out);
}

struct RenderOut {
  float* depth;
  double *points, *normals;
  int64_t* ids;
  uint8_t* mask;
};

PG_HD void mq_store_pixel(const MqRay& Q, const RcRay& ray, const double* vertices, const int64_t* tri, int64_t n, int64_t pixel, const RenderOut& out) {
  const bool ok = Q.tri >= 0;
  double point[3] = {NAN, NAN, NAN}, normal[3] = {NAN, NAN, NAN};
  if (ok) rc_point(ray, Q.t, point);
  if (ok && out.normals) mq_normal(vertices, tri, n, Q.tri, normal);
  if (out.depth) out.depth[pixel] = ok ? (float)Q.t : 0.0f;
  if (out.mask) out.mask[pixel] = ok ? 1 : 0;
  if (out.ids) out.ids[pixel] = ok ? Q.tri : -1;
  for (int k = 0; k < 3; k++) {
    if (out.points) out.points[3 * pixel + k] = point[k];
    if (out.normals) out.normals[3 * pixel + k] = normal[k];
  }
}

// the ray of pixel (u, v) of a view as six words: rc_ray's with the world's origin
PG_HD RcRay mq_pixel_ray(const double* view, int u, int v, double* six) {
  const double zero[3] = {0.0, 0.0, 0.0};
  const RcRay ray = rc_ray(view, zero, u, v);
  for (int k = 0; k < 3; k++) six[k] = ray.e[k], six[3 + k] = ray.dir[k];
  return ray;
}

// a workgroup per tile of 16 x 16 pixels of one view, a wave per quadrant of 8 x 8 (csrc/tsdf_raycast.hip's cut)
__global__ __launch_bounds__(kMqRenderThreads) void mesh_render_kernel(MqTree T, MqCall c, const double* __restrict__ views, const int* __restrict__ view_meshes,
                                                                       int64_t first_view, int H, int W, double depth_min, double depth_max, RenderOut out) {
  const int tx = (W + kRaycastTile - 1) / kRaycastTile, ty = (H + kRaycastTile - 1) / kRaycastTile;
  const int64_t view = first_view + blockIdx.x / ((int64_t)tx * ty);
  const int in_view = (int)(blockIdx.x % ((int64_t)tx * ty));
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int u = (in_view % tx) * kRaycastTile + (wave & 1) * 8 + (lane & 7), v = (in_view / tx) * kRaycastTile + (wave >> 1) * 8 + (lane >> 3);
  if (u >= W || v >= H) return;
  int b = view_meshes[view];
  double six[6];
  const RcRay ray = mq_pixel_ray(views + view * kRaycastViewWords, u, v, six);
  MqRay Q;
  Q.init(six, depth_min, depth_max, false);
  mq_query(T, c, b, Q);
  if (b < 0 || b >= c.t.n) b = 0, Q.tri = -1;
  mq_store_pixel(Q, ray, T.vertices + 3 * c.v.start[b], T.tri + 3 * c.t.start[b], c.v.start[b + 1] - c.v.start[b], (view * H + v) * W + u, out);
}

struct PointOut {
  double *points, *distances;
  int64_t* ids;
  double *uvs, *normals;
};

PG_HD void mq_store_point(const MqPoint& Q, const double* vertices, const int64_t* tri, int64_t n, int64_t i, const PointOut& out) {
  const bool ok = Q.tri >= 0;
  double normal[3] = {NAN, NAN, NAN};
  if (ok && out.normals) mq_normal(vertices, tri, n, Q.tri, normal);
  if (out.distances) out.distances[i] = ok ? pg_sqrt(Q.d2) : (Q.valid ? (double)INFINITY : (double)NAN);
  if (out.ids) out.ids[i] = ok ? Q.tri : -1;
  if (out.uvs) out.uvs[2 * i] = ok ? Q.u : (double)NAN, out.uvs[2 * i + 1] = ok ? Q.v : (double)NAN;
  for (int k = 0; k < 3; k++) {
    if (out.points) out.points[3 * i + k] = ok ? Q.point[k] : (double)NAN;
    if (out.normals) out.normals[3 * i + k] = normal[k];
  }
}

__global__ __launch_bounds__(kMqWalkThreads) void mesh_closest_points_kernel(MqTree T, MqCall c, const double* __restrict__ queries,
                                                                             const int* __restrict__ query_meshes, int64_t num_queries, PointOut out) {
  const int64_t i = (int64_t)blockIdx.x * kMqWalkThreads + threadIdx.x;
  if (i >= num_queries) return;
  int b = query_meshes[i];
  MqPoint Q;
  Q.init(queries + 3 * i);
  mq_query(T, c, b, Q);
  if (b < 0 || b >= c.t.n) b = 0, Q.tri = -1;
  mq_store_point(Q, T.vertices + 3 * c.v.start[b], T.tri + 3 * c.t.start[b], c.v.start[b + 1] - c.v.start[b], i, out);
}

bool mq_render_args(const char* what, int64_t num_views, int H, int W, double depth_min, double depth_max) {
  if (num_views < 0 || H < 1 || H > kTsdfMaxImage || W < 1 || W > kTsdfMaxImage)
    return se3_set_error("%s: %lld views of %d x %d: each side must lie in [1, %d]", what, (long long)num_views, H, W, kTsdfMaxImage), false;
  if (!(isfinite(depth_min) && isfinite(depth_max) && depth_min > 0.0 && depth_max > depth_min))
    return se3_set_error("%s: depth_min %g, depth_max %g: 0 < depth_min < depth_max expected", what, depth_min, depth_max), false;
  return true;
}

bool mq_host_sizes(const char* what, int64_t n, int64_t m) {
  if (n >= 0 && n < kMqMaxRows && m >= 0 && m < kMqMaxRows) return true;
  se3_set_error("%s: %lld vertices, %lld triangles: each below 2^31", what, (long long)n, (long long)m);
  return false;
}

}  // namespace

// ================================================================ the entries ======================================================================
extern "C" size_t se3_mesh_bvh_workspace_bytes(int64_t m_total) { return m_total < 0 ? 0 : mq_bvh_carve(m_total, nullptr, nullptr); }

extern "C" int se3_mesh_bvh_stack(int pass, const double* vertices, const int64_t* triangles, const int64_t* vertex_offsets_host,
                                  const int64_t* triangle_offsets_host, int num_meshes, int64_t* keys, const int64_t* sorted_keys, const int64_t* order,
                                  void* out_nodes, int64_t* out_counts, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "mesh_bvh_stack";
  MqCall c;
  SE3_REQUIRE(pass == SE3_MESH_BVH_KEYS || pass == SE3_MESH_BVH_TREE, SE3_ERR_INVALID_ARG, "%s: pass %d", what, pass);
  const bool tree = pass == SE3_MESH_BVH_TREE;
  if (const int rc = mq_call(what, vertices && triangles && out_counts && workspace && (tree ? sorted_keys && order && out_nodes : keys != nullptr),
                             vertex_offsets_host, triangle_offsets_host, num_meshes, &c))
    return rc;
  SE3_REQUIRE(workspace_bytes >= se3_mesh_bvh_workspace_bytes(c.m_total), SE3_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what,
              workspace_bytes, se3_mesh_bvh_workspace_bytes(c.m_total));
  if (num_meshes == 0) return SE3_OK;
  hipStream_t st = (hipStream_t)stream;
  BvhLayout L;
  mq_bvh_carve(c.m_total, (char*)workspace, &L);
  if (!tree) {
    MQ_MEMSET(out_counts, 0, sizeof(int64_t) * kMqCounts * num_meshes, what);
    mesh_bvh_bounds_kernel<<<(unsigned)num_meshes, kMqBoundsThreads, 0, st>>>(vertices, triangles, c, L.boxes, out_counts);
    if (c.m_total > 0) mesh_bvh_keys_kernel<<<mq_blocks(c.m_total, kMqThreads), kMqThreads, 0, st>>>(vertices, triangles, c, L.boxes, keys);
    SE3_CHECK_LAUNCH(what);
    return SE3_OK;
  }
  MQ_MEMSET(out_nodes, 0, sizeof(MqNode) * 2 * mq_atleast1(c.m_total), what);
  MQ_MEMSET(L.arrivals, 0, sizeof(int) * mq_atleast1(c.m_total), what);
  mesh_bvh_roots_kernel<<<1, kPairMaxPairs, 0, st>>>(c, (MqNode*)out_nodes, out_counts);
  if (c.m_total > 0) {
    const unsigned blocks = mq_blocks(c.m_total, kMqThreads);
    mesh_bvh_topology_kernel<<<blocks, kMqThreads, 0, st>>>(c, sorted_keys, (MqNode*)out_nodes, out_counts);
    mesh_bvh_refit_kernel<<<blocks, kMqThreads, 0, st>>>(vertices, triangles, c, order, (MqNode*)out_nodes, L.arrivals, out_counts);
  }
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" int se3_mesh_cast_rays_stack(const double* vertices, const int64_t* triangles, const int64_t* vertex_offsets_host,
                                        const int64_t* triangle_offsets_host, int num_meshes, const void* nodes, const int64_t* tree_counts,
                                        const double* rays, const int* ray_meshes, int64_t num_rays, double t_min, double t_max, int any_hit,
                                        double* out_t, int64_t* out_ids, double* out_uvs, double* out_normals, uint8_t* out_hit, void* stream) {
  const char* what = "mesh_cast_rays_stack";
  MqCall c;
  if (const int rc = mq_call(what, vertices && triangles && nodes && tree_counts, vertex_offsets_host, triangle_offsets_host, num_meshes, &c)) return rc;
  SE3_REQUIRE(num_rays >= 0 && !isnan(t_min) && !isnan(t_max), SE3_ERR_INVALID_ARG, "%s: %lld rays, t in [%g, %g]", what, (long long)num_rays, t_min, t_max);
  SE3_REQUIRE(any_hit ? out_hit != nullptr : true, SE3_ERR_INVALID_ARG, "%s: any_hit writes out_hit", what);
  if (num_rays == 0) return SE3_OK;
  SE3_REQUIRE(rays && ray_meshes, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(num_rays < (1ll << 31) * kMqWalkThreads, SE3_ERR_UNSUPPORTED, "%s: %lld rays in one call", what, (long long)num_rays);
  const MqTree T{vertices, triangles, (const MqNode*)nodes, tree_counts};
  const RayOut out = any_hit ? RayOut{nullptr, nullptr, nullptr, nullptr, out_hit} : RayOut{out_t, out_ids, out_uvs, out_normals, nullptr};
  mesh_cast_rays_kernel<<<mq_blocks(num_rays, kMqWalkThreads), kMqWalkThreads, 0, (hipStream_t)stream>>>(T, c, rays, ray_meshes, num_rays, t_min, t_max,
            any_hit, out);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" int se3_mesh_render_stack(const double* vertices, const int64_t* triangles, const int64_t* vertex_offsets_host,
                                     const int64_t* triangle_offsets_host, int num_meshes, const void* nodes, const int64_t* tree_counts,
                                     const double* views, const int* view_meshes, int64_t num_views, int height, int width, double depth_min,
                                     double depth_max, float* out_depth, double* out_points, double* out_normals, int64_t* out_primitive_ids,
                                     uint8_t* out_mask, void* stream) {
  const char* what = "mesh_render_stack";
  MqCall c;
  if (const int rc = mq_call(what, vertices && triangles && nodes && tree_counts, vertex_offsets_host, triangle_offsets_host, num_meshes, &c)) return rc;
  if (!mq_render_args(what, num_views, height, width, depth_min, depth_max)) return SE3_ERR_INVALID_ARG;
  if (num_views == 0) return SE3_OK;
  SE3_REQUIRE(views && view_meshes, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  const MqTree T{vertices, triangles, (const MqNode*)nodes, tree_counts};
  const RenderOut out{out_depth, out_points, out_normals, out_primitive_ids, out_mask};
  const int64_t tiles = se3_cdiv(width, kRaycastTile) * se3_cdiv(height, kRaycastTile), per_launch = ((1ll << 31) - 1) / tiles;
  for (int64_t first = 0; first < num_views; first += per_launch) {
    const int64_t count = num_views - first < per_launch ? num_views - first : per_launch;
    mesh_render_kernel<<<(unsigned)(count * tiles), kMqRenderThreads, 0, (hipStream_t)stream>>>(T, c, views, view_meshes, first, height, width, depth_min,
              depth_max, out);
  }
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" int se3_mesh_closest_points_stack(const double* vertices, const int64_t* triangles, const int64_t* vertex_offsets_host,
                                             const int64_t* triangle_offsets_host, int num_meshes, const void* nodes, const int64_t* tree_counts,
                                             const double* queries, const int* query_meshes, int64_t num_queries, double* out_points,
                                             double* out_distances, int64_t* out_ids, double* out_uvs, double* out_normals, void* stream) {
  const char* what = "mesh_closest_points_stack";
  MqCall c;
  if (const int rc = mq_call(what, vertices && triangles && nodes && tree_counts, vertex_offsets_host, triangle_offsets_host, num_meshes, &c)) return rc;
  SE3_REQUIRE(num_queries >= 0 && num_queries < (1ll << 31) * kMqWalkThreads, SE3_ERR_INVALID_ARG, "%s: %lld query points", what, (long long)num_queries);
  if (num_queries == 0) return SE3_OK;
  SE3_REQUIRE(queries && query_meshes, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  const MqTree T{vertices, triangles, (const MqNode*)nodes, tree_counts};
  const PointOut out{out_points, out_distances, out_ids, out_uvs, out_normals};
  mesh_closest_points_kernel<<<mq_blocks(num_queries, kMqWalkThreads), kMqWalkThreads, 0, (hipStream_t)stream>>>(T, c, queries, query_meshes, num_queries,
            out);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

// ================================== the same text on host memory, one mesh, serially, no GPU (tests/test_mesh_query_cpu.py) =========================
// SE3_MESH_BVH_KEYS: keys (m) and out_counts (status, live, zero-area, root as it will be).  SE3_MESH_BVH_TREE: out_nodes (2 max(m, 1) nodes)
// from sorted_keys and order (m: the triangle of every sorted place) and the live count of out_counts, which the keys pass left there.
extern "C" int se3_debug_mesh_bvh_host(int pass, const double* vertices, const int64_t* triangles, int64_t n, int64_t m, int64_t* keys,
                                       const int64_t* sorted_keys, const int64_t* order, void* out_nodes, int64_t* out_counts) {
  const char* what = "debug_mesh_bvh_host";
  SE3_REQUIRE(pass == SE3_MESH_BVH_KEYS || pass == SE3_MESH_BVH_TREE, SE3_ERR_INVALID_ARG, "%s: pass %d", what, pass);
  const bool tree = pass == SE3_MESH_BVH_TREE;
  SE3_REQUIRE((vertices || n == 0) && (triangles || m == 0) && out_counts && (tree ? out_nodes && (m == 0 || (sorted_keys && order)) : keys || m == 0),
              SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  if (!mq_host_sizes(what, n, m)) return SE3_ERR_UNSUPPORTED;
  const double *p0, *p1, *p2;
  if (!tree) {
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, x[3];
    int64_t status = 0, live = 0, flat = 0;
    for (int64_t t = 0; t < m; t++) {
      const int kind = mq_triangle(vertices, triangles, t, n, &p0, &p1, &p2);
      status |= mq_status_of(kind), flat += kind == kMqFlat;
      if (kind != kMqLive) continue;
      mq_centroid(p0, p1, p2, x);
      for (int k = 0; k < 3; k++) mn[k] = fmin(mn[k], x[k]), mx[k] = fmax(mx[k], x[k]);
      live++;
    }
    for (int64_t t = 0; t < m; t++) {
      keys[t] = kMqInertKey;
      if (mq_triangle(vertices, triangles, t, n, &p0, &p1, &p2) != kMqLive) continue;
      mq_centroid(p0, p1, p2, x);
      keys[t] = mq_key(x, mn, mx);
    }
    out_counts[0] = status, out_counts[1] = live, out_counts[2] = flat, out_counts[3] = 0;
    return SE3_OK;
  }
  MqNode* N = (MqNode*)out_nodes;
  memset(N, 0, sizeof(MqNode) * 2 * mq_atleast1(m));
  const int64_t live = mq_live(out_counts, 0, m);
  const int root = mq_root_of(live, m);
  out_counts[3] = root;
  if (root >= 0) N[root].parent = -1;
  for (int64_t i = 0; i < live - 1; i++) {
    int left, right;
    mq_topology(sorted_keys, live, m, i, &left, &right);
    N[i].left = left, N[i].right = right;
    N[left].parent = (int)i, N[right].parent = (int)i;
  }
  std::vector<int> arrivals((size_t)mq_atleast1(m), 0);
  for (int64_t j = live - 1; j >= 0; j--) {                              // (descending: a node's second arrival is not always its right child)
    const int64_t id = order[j];
    if (id < 0 || id >= m || mq_triangle(vertices, triangles, id, n, &p0, &p1, &p2) != kMqLive) continue;
    int self = (int)(m + j);
    mq_leaf_box(p0, p1, p2, &N[self]);
    N[self].left = N[self].right = (int)(-1 - id);
    MqNode mine = N[self];
    int parent = N[self].parent;
    for (int level = 0; level <= kMqMaxDepth && parent >= 0 && parent < live - 1; level++) {
      if (arrivals[parent]++ == 0) break;
      const int other = N[parent].left == self ? N[parent].right : N[parent].left;
      if (other < 0 || other >= 2 * m) break;
      for (int k = 0; k < 3; k++) {
        mine.lo[k] = N[other].lo[k] < mine.lo[k] ? N[other].lo[k] : mine.lo[k], mine.hi[k] = N[other].hi[k] > mine.hi[k] ? N[other].hi[k] : mine.hi[k];
        N[parent].lo[k] = mine.lo[k], N[parent].hi[k] = mine.hi[k];
      }
      self = parent, parent = N[self].parent;
    }
  }
  return SE3_OK;
}

namespace {
int mq_cast_host(const char* what, const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const void* nodes, int64_t root,
                 const double* rays, int64_t num_rays, double t_min, double t_max, int any_hit, double* out_t, int64_t* out_ids, double* out_uvs,
                 double* out_normals, uint8_t* out_hit) {
  SE3_REQUIRE((vertices || n == 0) && (triangles || m == 0) && (rays || num_rays == 0) && num_rays >= 0 && (!any_hit || out_hit), SE3_ERR_INVALID_ARG,
              "%s: null pointer", what);
  if (!mq_host_sizes(what, n, m)) return SE3_ERR_UNSUPPORTED;
  SE3_REQUIRE(!nodes || (root >= -1 && root < 2 * m), SE3_ERR_INVALID_ARG, "%s: root %lld outside the table", what, (long long)root);
  const RayOut out = any_hit ? RayOut{nullptr, nullptr, nullptr, nullptr, out_hit} : RayOut{out_t, out_ids, out_uvs, out_normals, nullptr};
  for (int64_t r = 0; r < num_rays; r++) {
    MqRay Q;
    Q.init(rays + 6 * r, t_min, t_max, any_hit != 0);
    if (Q.valid && nodes) mq_walk((const MqNode*)nodes, (int)root, vertices, triangles, n, m, Q);
    else if (Q.valid) mq_brute(vertices, triangles, n, m, Q);
    mq_store_ray(Q, vertices, triangles, n, r, out);
  }
  return SE3_OK;
}

int mq_closest_host(const char* what, const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const void* nodes, int64_t root,
                    const double* queries, int64_t num_queries, double* out_points, double* out_distances, int64_t* out_ids, double* out_uvs,
                    double* out_normals) {
  SE3_REQUIRE((vertices || n == 0) && (triangles || m == 0) && (queries || num_queries == 0) && num_queries >= 0, SE3_ERR_INVALID_ARG, "%s: null pointer",
              what);
  if (!mq_host_sizes(what, n, m)) return SE3_ERR_UNSUPPORTED;
  SE3_REQUIRE(!nodes || (root >= -1 && root < 2 * m), SE3_ERR_INVALID_ARG, "%s: root %lld outside the table", what, (long long)root);
  const PointOut out{out_points, out_distances, out_ids, out_uvs, out_normals};
  for (int64_t i = 0; i < num_queries; i++) {
    MqPoint Q;
    Q.init(queries + 3 * i);
    if (Q.valid && nodes) mq_walk((const MqNode*)nodes, (int)root, vertices, triangles, n, m, Q);
    else if (Q.valid) mq_brute(vertices, triangles, n, m, Q);
    mq_store_point(Q, vertices, triangles, n, i, out);
  }
  return SE3_OK;
}
}  // namespace

// BRUTE FORCE over every triangle in ascending order with the per-triangle text and the tie rules: no tree.  The yardstick of the walk.
extern "C" int se3_debug_mesh_cast_rays_host(const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const double* rays, int64_t num_rays,
                                             double t_min, double t_max, int any_hit, double* out_t, int64_t* out_ids, double* out_uvs,
                                             double* out_normals, uint8_t* out_hit) {
  return mq_cast_host("debug_mesh_cast_rays_host", vertices, triangles, n, m, nullptr, -1, rays, num_rays, t_min, t_max, any_hit, out_t, out_ids, out_uvs,
                      out_normals, out_hit);
}

extern "C" int se3_debug_mesh_closest_points_host(const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const double* queries,
                                                  int64_t num_queries, double* out_points, double* out_distances, int64_t* out_ids, double* out_uvs,
                                                  double* out_normals) {
  return mq_closest_host("debug_mesh_closest_points_host", vertices, triangles, n, m, nullptr, -1, queries, num_queries, out_points, out_distances, out_ids,
                         out_uvs, out_normals);
}

// the kernels' walk (contract 8) over a tree of se3_debug_mesh_bvh_host, serially: what the device runs, for the tests without a GPU
extern "C" int se3_debug_mesh_walk_rays_host(const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const void* nodes, int64_t root,
                                             const double* rays, int64_t num_rays, double t_min, double t_max, int any_hit, double* out_t,
                                             int64_t* out_ids, double* out_uvs, double* out_normals, uint8_t* out_hit) {
  SE3_REQUIRE(nodes, SE3_ERR_INVALID_ARG, "debug_mesh_walk_rays_host: null pointer");
  return mq_cast_host("debug_mesh_walk_rays_host", vertices, triangles, n, m, nodes, root, rays, num_rays, t_min, t_max, any_hit, out_t, out_ids, out_uvs,
                      out_normals, out_hit);
}

extern "C" int se3_debug_mesh_walk_points_host(const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const void* nodes, int64_t root,
                                               const double* queries, int64_t num_queries, double* out_points, double* out_distances, int64_t* out_ids,
                                               double* out_uvs, double* out_normals) {
  SE3_REQUIRE(nodes, SE3_ERR_INVALID_ARG, "debug_mesh_walk_points_host: null pointer");
  return mq_closest_host("debug_mesh_walk_points_host", vertices, triangles, n, m, nodes, root, queries, num_queries, out_points, out_distances, out_ids,
                         out_uvs, out_normals);
}

// the kernel's ray of every pixel, then the brute-force cast
extern "C" int se3_debug_mesh_render_host(const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const double* views, int64_t num_views,
                                          int height, int width, double depth_min, double depth_max, float* out_depth, double* out_points,
                                          double* out_normals, int64_t* out_primitive_ids, uint8_t* out_mask) {
  const char* what = "debug_mesh_render_host";
  SE3_REQUIRE((vertices || n == 0) && (triangles || m == 0) && (views || num_views == 0), SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  if (!mq_host_sizes(what, n, m)) return SE3_ERR_UNSUPPORTED;
  if (!mq_render_args(what, num_views, height, width, depth_min, depth_max)) return SE3_ERR_INVALID_ARG;
  const RenderOut out{out_depth, out_points, out_normals, out_primitive_ids, out_mask};
  for (int64_t view = 0; view < num_views; view++)
    for (int v = 0; v < height; v++)
      for (int u = 0; u < width; u++) {
        double six[6];
        const RcRay ray = mq_pixel_ray(views + view * kRaycastViewWords, u, v, six);
        MqRay Q;
        Q.init(six, depth_min, depth_max, false);
        if (Q.valid) mq_brute(vertices, triangles, n, m, Q);
        mq_store_pixel(Q, ray, vertices, triangles, n, (view * height + v) * width + u, out);
      }
  return SE3_OK;
}
