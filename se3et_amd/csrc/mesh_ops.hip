// Mesh post-processing for stacked triangle meshes (Open3D's TriangleMesh tools that follow extract_triangle_mesh), up to SE3_PAIR_MAX_PAIRS
// meshes per call: the incidence tables, connected components, selection with compaction, normals, smoothing and (at the end of the file, with its own rules) vertex clustering.  se3et_amd/mesh.py is
// the front end; csrc/mesh_ops_core.h holds the text that the kernels and the se3_debug_mesh_*_host entries share.
// (SE3_EXACT_FP: the file is built with contraction off, and the core fences itself as well.)
//
// Layout.  vertices (sum n, 3) float64, triangles (sum m, 3) int64 naming vertices by their number within their own mesh, the meshes'
// cuts as host offsets (B + 1), attributes (sum n, 3) float64.  n, m < 2^31 per mesh.
//
// Contract.
//   0. A triangle that names a vertex outside [0, n) is never dereferenced (mo_triangle is the only way to a vertex number): it is
//      incident to nothing, belongs to a cluster of its own, has a zero normal and area and is never kept, and bit
//      SE3_MESH_OPS_BAD_TRIANGLE of its mesh's status word is set; the Python side raises ValueError.
//   1. Incidence.  Two CSR tables over the stacked vertices, offsets (sum n + 1) int64 into int rows of mesh-local numbers.  tri_rows: the
//      triangles that name the vertex, ascending, a degenerate (a, a, b) once under a.  nbr_rows: the distinct other vertices of those
//      triangles, ascending, an edge shared by two triangles giving one neighbour.  No valence limit: the rows are filled through integer
//      atomic cursors and then made canonical by an insertion sort in global memory, and the neighbours are found by comparing every
//      triangle of a row with the ones before it, so the cost of a row is QUADRATIC in the valence (6 on a marching-cubes mesh).
//   2. Components (cluster_connected_triangles).  Two triangles are adjacent iff they share an undirected edge {a, b} with a != b; a common
//      vertex alone does not connect.  Clusters are numbered 0 .. k - 1 in ascending order of their lowest triangle.  cluster_area: every
//      triangle's 0.5 |cross(v1 - v0, v2 - v0)|, the members of a cluster taken in ascending triangle order a[0], a[1], ..; lane l of 64
//      adds a[l], a[l + 64], .. in that order from 0.0, then the 64 lanes are added by the butterfly lane[l] += lane[l ^ o] for
//      o = 32, 16, 8, 4, 2, 1.  The host entry runs the same tree.
//   3. Selection (remove_triangles_by_mask + remove_unreferenced_vertices).  The kept triangles and the vertices they name, in their
//      original order, renumbered by the scan of block_ops.h; the old -> new vertex map holds -1 for a dropped vertex.
//   4. Normals.  Triangle: cross(v1 - v0, v2 - v0), optionally normalised.  Vertex: the sum of the un-normalised normals of its tri_row in
//      row order, normalised.  A zero (or non-finite) length gives (0, 0, 1).  A gather: no float atomics.
//   5. Smoothing.  s = the sum of the neighbour row in row order; simple: (x + s) / (len + 1); laplacian: x + lambda (s / len - x); taubin:
//      a laplacian step with lambda, then one with mu.  An empty row keeps x (Open3D's Laplacian divides by zero there).  Attributes are
//      filtered by the same rule; normals are not renormalised.  One launch per step over all meshes, ping-pong between the output and
//      the workspace, every step issued by the one call, nothing read back.
//   Alone or in a batch, and from run to run, every output has the same bits: the only atomics are integer counts, cursors whose order a
//   sort removes, and the forest of dbscan_core.h.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "mesh_ops_core.h"

namespace {

constexpr int kMoThreads = 256;
constexpr int kMoScanThreads = 1024;
constexpr int64_t kMoMaxRows = 1ll << 31;
constexpr int kMoCounts = SE3_MESH_OPS_COUNT_WORDS;
static_assert(kMoAreaLanes == SE3_MESH_OPS_AREA_LANES && kMoAreaLanes == SE3_WAVE, "the area tree is one wave wide");

struct MeshCall {
  PairRows v, t;                            // the meshes' vertex and triangle rows
  int64_t n_total, m_total;
};

int mo_call(const char* what, bool pointers, const int64_t* vertex_offsets, const int64_t* triangle_offsets, int num_meshes, MeshCall* c) {
  SE3_REQUIRE(pointers && vertex_offsets && triangle_offsets, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(num_meshes >= 0 && num_meshes <= kPairMaxPairs, SE3_ERR_INVALID_ARG, "%s: %d meshes (at most %d)", what, num_meshes, kPairMaxPairs);
  SE3_REQUIRE(pg_fill_rows(&c->v, vertex_offsets, num_meshes) && pg_fill_rows(&c->t, triangle_offsets, num_meshes), SE3_ERR_INVALID_ARG,
              "%s: offsets must start at 0 and not decrease", what);
  for (int b = 0; b < num_meshes; b++)
    SE3_REQUIRE(c->v.start[b + 1] - c->v.start[b] < kMoMaxRows && c->t.start[b + 1] - c->t.start[b] < kMoMaxRows, SE3_ERR_UNSUPPORTED,
                "%s: mesh %d has 2^31 vertices or triangles or more", what, b);
  c->n_total = c->v.start[num_meshes], c->m_total = c->t.start[num_meshes];
  return SE3_OK;
}

inline unsigned mo_blocks(int64_t rows) { return (unsigned)se3_cdiv(rows, kMoThreads); }
inline size_t mo_atleast1(int64_t v) { return (size_t)(v > 0 ? v : 1); }

#define MO_MEMSET(ptr, value, bytes, what)                                   \
  do {                                                                        \
    if (hipMemsetAsync(ptr, value, bytes, st) != hipSuccess) {                \
      se3_set_error("%s: hipMemsetAsync failed", what);                       \
      return SE3_ERR_LAUNCH;                                                  \
    }                                                                         \
  } while (0)

// ---- the prefix sums of the entries -----------------------------------------------------------------------------------------------------------------
// A scan of every mesh's rows of `a` in place (exclusive or inclusive) in three launches: every tile of kMoTile rows is scanned by one
// workgroup (se3_block_exclusive of block_ops.h, one row per thread, coalesced) and leaves its sum; one workgroup per mesh scans the
// mesh's tile sums (se3_block_scan) and writes the mesh's total into word `word` of its counts row (counts NULL: nowhere) and, for a single
// mesh, behind its rows (total_out); every row takes its tile's offset.  Integers: the result is the serial scan's.  tile_sums:
// mo_scan_tiles(rows) entries.
constexpr int kMoTile = 1024;
inline size_t mo_scan_tiles(int64_t rows) { return (size_t)se3_cdiv(rows > 0 ? rows : 0, kMoTile) + kPairMaxPairs; }

template <class T, bool EXCLUSIVE>
__global__ __launch_bounds__(kMoTile) void mesh_scan_tile_kernel(T* __restrict__ a, PairRows rows, PairRows tiles, T* __restrict__ tile_sums) {
  __shared__ T sh[kMoTile];
  const int64_t g = blockIdx.x;
  const int b = pg_pair_of_row(tiles, g);
  const int64_t i = rows.start[b] + (g - tiles.start[b]) * kMoTile + threadIdx.x;
  const bool in = i < rows.start[b + 1];
  const T v = in ? a[i] : 0;
  T total;
  const T before = se3_block_exclusive<T, kMoTile>(v, sh, &total);
  if (in) a[i] = EXCLUSIVE ? before : before + v;
  if (threadIdx.x == 0) tile_sums[g] = total;
}

template <class T>
__global__ __launch_bounds__(kMoScanThreads) void mesh_scan_sums_kernel(T* __restrict__ tile_sums, PairRows tiles, int64_t* __restrict__ counts, int word,
                                                                        T* __restrict__ total_out) {
  __shared__ T sh[kMoScanThreads];
  const int b = blockIdx.x;
  const T total = se3_block_scan<kSe3ScanExclusive, T, int64_t, kMoScanThreads>(tile_sums + tiles.start[b], tiles.start[b + 1] - tiles.start[b], sh);
  if (threadIdx.x == 0) {
    if (counts) counts[kMoCounts * b + word] = total;
    if (total_out) *total_out = total;
  }
}

template <class T>
__global__ __launch_bounds__(kMoTile) void mesh_scan_add_kernel(T* __restrict__ a, PairRows rows, PairRows tiles, const T* __restrict__ tile_sums) {
  const int64_t g = blockIdx.x;
  const int b = pg_pair_of_row(tiles, g);
  const int64_t i = rows.start[b] + (g - tiles.start[b]) * kMoTile + threadIdx.x;
  if (i < rows.start[b + 1]) a[i] += tile_sums[g];
}

template <class T, bool EXCLUSIVE>
void mo_scan_rows(T* a, const PairRows& rows, T* tile_sums, int64_t* counts, int word, T* total_out, hipStream_t st) {
  PairRows tiles;
  tiles.n = rows.n;
  tiles.start[0] = 0;
  for (int b = 0; b < kPairMaxPairs; b++) tiles.start[b + 1] = tiles.start[b] + (b < rows.n ? se3_cdiv(rows.start[b + 1] - rows.start[b], kMoTile) : 0);
  const unsigned blocks = (unsigned)tiles.start[rows.n];
  if (blocks) mesh_scan_tile_kernel<T, EXCLUSIVE><<<blocks, kMoTile, 0, st>>>(a, rows, tiles, tile_sums);
  mesh_scan_sums_kernel<T><<<(unsigned)rows.n, kMoScanThreads, 0, st>>>(tile_sums, tiles, counts, word, total_out);
  if (blocks) mesh_scan_add_kernel<T><<<blocks, kMoTile, 0, st>>>(a, rows, tiles, tile_sums);
}

// ---- incidence ---------------------------------------------------------------------------------------------------------------------------------
// one thread per triangle: the bounds rule, and one count under each distinct vertex
__global__ __launch_bounds__(kMoThreads) void mesh_incidence_count_kernel(const int64_t* __restrict__ tri, MeshCall c, int64_t* __restrict__ tri_offsets,
                                                                          int64_t* __restrict__ counts) {
  const int64_t t = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (t >= c.m_total) return;
  const int b = pg_pair_of_row(c.t, t);
  int w[3], d[3];
  if (!mo_triangle(tri, t, c.v.start[b + 1] - c.v.start[b], w)) {
    atomicOr((unsigned long long*)(counts + kMoCounts * b), (unsigned long long)SE3_MESH_OPS_BAD_TRIANGLE);
    return;
  }
  const int k = mo_distinct(w, d);
  for (int j = 0; j < k; j++) atomicAdd((unsigned long long*)(tri_offsets + c.v.start[b] + d[j]), 1ull);
}

__global__ __launch_bounds__(kMoThreads) void mesh_incidence_fill_kernel(const int64_t* __restrict__ tri, MeshCall c, const int64_t* __restrict__ tri_offsets,
                                                                         int* __restrict__ cursor, int* __restrict__ tri_rows) {
  const int64_t t = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (t >= c.m_total) return;
  const int b = pg_pair_of_row(c.t, t);
  int w[3], d[3];
  if (!mo_triangle(tri, t, c.v.start[b + 1] - c.v.start[b], w)) return;
  const int k = mo_distinct(w, d);
  for (int j = 0; j < k; j++) {
    const int64_t i = c.v.start[b] + d[j];
    const int64_t at = tri_offsets[i] + atomicAdd(cursor + i, 1);
    if (at < tri_offsets[i + 1]) tri_rows[at] = (int)(t - c.t.start[b]);          // (always, unless the triangles changed since the count)
  }
}

// one thread per vertex: its incident row in ascending order, then the number of its neighbours
__global__ __launch_bounds__(kMoThreads) void mesh_incidence_sort_kernel(const int64_t* __restrict__ tri, MeshCall c, const int64_t* __restrict__ tri_offsets,
                                                                         int* __restrict__ tri_rows, int64_t* __restrict__ nbr_offsets) {
  const int64_t i = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (i >= c.n_total) return;
  const int b = pg_pair_of_row(c.v, i);
  int* row = tri_rows + tri_offsets[i];
  const int64_t len = tri_offsets[i + 1] - tri_offsets[i];
  mo_sort_row(row, len);
  nbr_offsets[i] = mo_neighbors(tri + 3 * c.t.start[b], c.t.start[b + 1] - c.t.start[b], c.v.start[b + 1] - c.v.start[b], row, len, (int)(i - c.v.start[b]), nullptr, 0);
}

__global__ void mesh_incidence_totals_kernel(MeshCall c, const int64_t* __restrict__ tri_offsets, const int64_t* __restrict__ nbr_offsets,
                                             int64_t* __restrict__ counts) {
  const int b = threadIdx.x;
  if (b >= c.v.n) return;
  counts[kMoCounts * b + 1] = tri_offsets[c.v.start[b + 1]] - tri_offsets[c.v.start[b]];
  counts[kMoCounts * b + 2] = nbr_offsets[c.v.start[b + 1]] - nbr_offsets[c.v.start[b]];
}

__global__ __launch_bounds__(kMoThreads) void mesh_incidence_neighbors_kernel(const int64_t* __restrict__ tri, MeshCall c, const int64_t* __restrict__ tri_offsets,
                                                                              const int* __restrict__ tri_rows, const int64_t* __restrict__ nbr_offsets,
                                                                              int64_t capacity, int* __restrict__ nbr_rows) {
  const int64_t i = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (i >= c.n_total) return;
  const int b = pg_pair_of_row(c.v, i);
  const int64_t at = nbr_offsets[i], end = nbr_offsets[i + 1];
  if (at < 0 || end < at || end > capacity) return;
  mo_neighbors(tri + 3 * c.t.start[b], c.t.start[b + 1] - c.t.start[b], c.v.start[b + 1] - c.v.start[b], tri_rows + tri_offsets[i], tri_offsets[i + 1] - tri_offsets[i],
               (int)(i - c.v.start[b]), nbr_rows + at, end - at);
}

// ---- components --------------------------------------------------------------------------------------------------------------------------------
struct ComponentsLayout {
  int* parent;         // [m_total], mesh-local: the forest of dbscan_core.h over triangles
  int* rank;           // [m_total]: the flags "is its own root", then their exclusive scan per mesh
  int* root;           // [m_total]
  int* tile_sums;      // mo_scan_tiles(m_total)
};

size_t mo_components_carve(int64_t m_total, char* base, ComponentsLayout* L) {
  Se3Carver c(base);
  ComponentsLayout l;
  l.parent = c.take<int>(mo_atleast1(m_total));
  l.rank = c.take<int>(mo_atleast1(m_total));
  l.root = c.take<int>(mo_atleast1(m_total));
  l.tile_sums = c.take<int>(mo_scan_tiles(m_total));
  if (L) *L = l;
  return c.bytes();
}

__global__ __launch_bounds__(kMoThreads) void mesh_components_init_kernel(MeshCall c, ComponentsLayout L) {
  const int64_t t = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (t >= c.m_total) return;
  L.parent[t] = (int)(t - c.t.start[pg_pair_of_row(c.t, t)]);
}

__global__ __launch_bounds__(kMoThreads) void mesh_components_link_kernel(const int64_t* __restrict__ tri, MeshCall c, const int64_t* __restrict__ tri_offsets,
                                                                          const int* __restrict__ tri_rows, ComponentsLayout L, int64_t* __restrict__ counts) {
  const int64_t t = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (t >= c.m_total) return;
  const int b = pg_pair_of_row(c.t, t);
  const int64_t n = c.v.start[b + 1] - c.v.start[b];
  int w[3];
  if (!mo_triangle(tri, t, n, w)) atomicOr((unsigned long long*)(counts + kMoCounts * b), (unsigned long long)SE3_MESH_OPS_BAD_TRIANGLE);
  int* parent = L.parent + c.t.start[b];
  mo_link_triangle(
      tri + 3 * c.t.start[b], c.t.start[b + 1] - c.t.start[b], n, (int)(t - c.t.start[b]), tri_offsets + c.v.start[b], tri_rows,
      [&](int x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
      [&](int x, int v) { atomicMin(parent + x, v); }, [&](int a, int r) { return atomicCAS(parent + a, a, r); });
}

// (the forest is final: parent is read only here)
__global__ __launch_bounds__(kMoThreads) void mesh_components_flatten_kernel(MeshCall c, ComponentsLayout L) {
  const int64_t t = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (t >= c.m_total) return;
  const int b = pg_pair_of_row(c.t, t);
  const int* parent = L.parent + c.t.start[b];
  const int self = (int)(t - c.t.start[b]);
  int x = self;
  while (parent[x] != x) x = parent[x];
  L.root[t] = x;
  L.rank[t] = x == self ? 1 : 0;
}

// (the count of a cluster is one atomic per wave and cluster met in it, not one per triangle: a mesh is mostly one cluster, and millions of
// adds on one word ran 14 times slower than the rest of the entry)
__global__ __launch_bounds__(kMoThreads) void mesh_components_label_kernel(MeshCall c, ComponentsLayout L, int64_t* __restrict__ clusters,
                                                                           int64_t* __restrict__ cluster_n_triangles) {
  const int64_t t = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  bool pending = t < c.m_total;
  long long slot = -1;
  if (pending) {
    const int64_t s0 = c.t.start[pg_pair_of_row(c.t, t)];
    const int label = L.rank[s0 + L.root[t]];
    clusters[t] = label;
    slot = s0 + label;
  }
  for (;;) {
    const unsigned long long todo = __ballot(pending);
    if (!todo) break;
    const int leader = __ffsll((long long)todo) - 1;
    const long long lead = __shfl(slot, leader);
    const bool mine = pending && slot == lead;
    const unsigned long long group = __ballot(mine);
    if (se3_lane() == leader) atomicAdd((unsigned long long*)(cluster_n_triangles + lead), (unsigned long long)__popcll(group));
    if (mine) pending = false;
  }
}

// one thread per place of `order`: the area of the triangle that stands there (0 for a place that names no triangle of the call)
__global__ __launch_bounds__(kMoThreads) void mesh_area_gather_kernel(const double* __restrict__ vertices, const int64_t* __restrict__ tri, MeshCall c,
                                                                      const int64_t* __restrict__ order, double* __restrict__ sorted_area) {
  const int64_t i = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (i >= c.m_total) return;
  const int64_t t = order[i];
  double a = 0.0;
  if (t >= 0 && t < c.m_total) {
    const int b = pg_pair_of_row(c.t, t);
    a = mo_triangle_area(vertices + 3 * c.v.start[b], tri + 3 * c.t.start[b], t - c.t.start[b], c.v.start[b + 1] - c.v.start[b]);
  }
  sorted_area[i] = a;
}

// one wave per cluster slot: the tree of contract 2 over the slot's run of sorted_area
__global__ __launch_bounds__(kMoThreads) void mesh_area_sum_kernel(int64_t m_total, const int64_t* __restrict__ starts, const double* __restrict__ sorted_area,
                                                                   double* __restrict__ cluster_area) {
  const int64_t g = ((int64_t)blockIdx.x * kMoThreads + threadIdx.x) / SE3_WAVE;
  if (g >= m_total) return;                                                // (uniform over the wave)
  const int64_t a = starts[g], e = starts[g + 1];
  if (e <= a || a < 0 || e > m_total) return;
  double s = 0.0;
  int64_t i = a + se3_lane();
  for (; i + 7 * kMoAreaLanes < e; i += 8 * kMoAreaLanes) {               // eight loads in flight, added in the order of the contract
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; u++) x[u] = sorted_area[i + u * kMoAreaLanes];
#pragma unroll
    for (int u = 0; u < 8; u++) s += x[u];
  }
  for (; i < e; i += kMoAreaLanes) s += sorted_area[i];
  s = se3_wave_sum(s);
  if (se3_lane() == 0) cluster_area[g] = s;
}

// ---- selection -----------------------------------------------------------------------------------------------------------------------------------
struct SelectLayout {
  int* tri_scan;       // [m_total]: kept flags, then their inclusive scan per mesh
  int* vertex_scan;    // [n_total]: referenced flags, then their inclusive scan per mesh
  int* tile_sums;      // mo_scan_tiles(max(n_total, m_total))
};

size_t mo_select_carve(int64_t n_total, int64_t m_total, char* base, SelectLayout* L) {
  Se3Carver c(base);
  SelectLayout l;
  l.tri_scan = c.take<int>(mo_atleast1(m_total));
  l.vertex_scan = c.take<int>(mo_atleast1(n_total));
  l.tile_sums = c.take<int>(mo_scan_tiles(n_total > m_total ? n_total : m_total));
  if (L) *L = l;
  return c.bytes();
}

__global__ __launch_bounds__(kMoThreads) void mesh_select_mark_kernel(const int64_t* __restrict__ tri, const uint8_t* __restrict__ keep, MeshCall c,
                                                                      SelectLayout L, int64_t* __restrict__ counts) {
  const int64_t t = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (t >= c.m_total) return;
  const int b = pg_pair_of_row(c.t, t);
  int w[3];
  const bool valid = mo_triangle(tri, t, c.v.start[b + 1] - c.v.start[b], w);
  if (!valid) atomicOr((unsigned long long*)(counts + kMoCounts * b), (unsigned long long)SE3_MESH_OPS_BAD_TRIANGLE);
  const bool kept = valid && keep[t] != 0;
  L.tri_scan[t] = kept ? 1 : 0;
  if (kept)
    for (int j = 0; j < 3; j++) L.vertex_scan[c.v.start[b] + w[j]] = 1;          // (every writer stores the same word)
}

// the place of row i among the kept rows of its mesh, or -1: scan is the inclusive scan of the flags from row s0 on
__device__ __forceinline__ int mo_kept_place(const int* scan, int64_t s0, int64_t i) {
  const int before = i > s0 ? scan[i - 1] : 0;
  return scan[i] != before ? before : -1;
}

__global__ __launch_bounds__(kMoThreads) void mesh_select_map_kernel(MeshCall c, SelectLayout L, int64_t* __restrict__ vertex_map) {
  const int64_t i = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (i >= c.n_total) return;
  vertex_map[i] = mo_kept_place(L.vertex_scan, c.v.start[pg_pair_of_row(c.v, i)], i);
}

struct SelectArrays {
  const double* src[3];
  double* dst[3];
};

__global__ __launch_bounds__(kMoThreads) void mesh_select_vertices_kernel(MeshCall c, PairRows out_v, SelectLayout L, SelectArrays A) {
  const int64_t i = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (i >= c.n_total) return;
  const int b = pg_pair_of_row(c.v, i);
  const int place = mo_kept_place(L.vertex_scan, c.v.start[b], i);
  if (place < 0 || out_v.start[b] + place >= out_v.start[b + 1]) return;
  const int64_t row = out_v.start[b] + place;
  for (int a = 0; a < 3; a++)
    if (A.src[a])
      for (int d = 0; d < 3; d++) A.dst[a][3 * row + d] = A.src[a][3 * i + d];
}

__global__ __launch_bounds__(kMoThreads) void mesh_select_triangles_kernel(const int64_t* __restrict__ tri, MeshCall c, PairRows out_t, SelectLayout L,
                                                                           int64_t* __restrict__ out_triangles) {
  const int64_t t = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (t >= c.m_total) return;
  const int b = pg_pair_of_row(c.t, t);
  const int place = mo_kept_place(L.tri_scan, c.t.start[b], t);
  int w[3];
  if (place < 0 || out_t.start[b] + place >= out_t.start[b + 1] || !mo_triangle(tri, t, c.v.start[b + 1] - c.v.start[b], w)) return;
  const int64_t row = out_t.start[b] + place;
  for (int j = 0; j < 3; j++) out_triangles[3 * row + j] = mo_kept_place(L.vertex_scan, c.v.start[b], c.v.start[b] + w[j]);
}

// ---- normals --------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMoThreads) void mesh_triangle_normals_kernel(const double* __restrict__ vertices, const int64_t* __restrict__ tri, MeshCall c,
                                                                           int normalized, double* __restrict__ out, int64_t* __restrict__ counts) {
  const int64_t t = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (t >= c.m_total) return;
  const int b = pg_pair_of_row(c.t, t);
  double v[3];
  int w[3];
  if (counts && !mo_triangle(tri, t, c.v.start[b + 1] - c.v.start[b], w))
    atomicOr((unsigned long long*)(counts + kMoCounts * b), (unsigned long long)SE3_MESH_OPS_BAD_TRIANGLE);
  mo_triangle_normal(vertices + 3 * c.v.start[b], tri + 3 * c.t.start[b], t - c.t.start[b], c.v.start[b + 1] - c.v.start[b], v);
  if (normalized) mo_normalize(v);
  for (int d = 0; d < 3; d++) out[3 * t + d] = v[d];
}

__global__ __launch_bounds__(kMoThreads) void mesh_vertex_normals_kernel(const double* __restrict__ vertices, const int64_t* __restrict__ tri, MeshCall c,
                                                                         const int64_t* __restrict__ tri_offsets, const int* __restrict__ tri_rows,
                                                                         double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (i >= c.n_total) return;
  const int b = pg_pair_of_row(c.v, i);
  double v[3];
  mo_vertex_normal(vertices + 3 * c.v.start[b], tri + 3 * c.t.start[b], c.t.start[b + 1] - c.t.start[b], c.v.start[b + 1] - c.v.start[b], tri_rows + tri_offsets[i],
                   tri_offsets[i + 1] - tri_offsets[i], v);
  for (int d = 0; d < 3; d++) out[3 * i + d] = v[d];
}

// ---- smoothing --------------------------------------------------------------------------------------------------------------------------------------
struct SmoothArrays {
  const double* src[3];
  double* dst[3];
  int count;
};

// One step of every array for every vertex of the call: one lane per vertex, three components each.  (One lane per component, so that a
// wave's loads of a neighbour's 24 bytes sit in three adjacent lanes, gave the same bits and took 1.3 to 1.45 times as long:
// profiles/mesh_ops_probe.txt.)
__global__ __launch_bounds__(kMoThreads) void mesh_smooth_kernel(PairRows rows, int64_t n_total, const int64_t* __restrict__ nbr_offsets,
                                                                 const int* __restrict__ nbr_rows, int simple, double lambda, SmoothArrays A) {
  const int64_t i = (int64_t)blockIdx.x * kMoThreads + threadIdx.x;
  if (i >= n_total) return;
  const int b = pg_pair_of_row(rows, i);
  const int64_t s0 = rows.start[b];
  const int* row = nbr_rows + nbr_offsets[i];
  const int64_t len = nbr_offsets[i + 1] - nbr_offsets[i];
  for (int a = 0; a < A.count; a++) {
    double out[3];
    mo_smooth(A.src[a] + 3 * s0, rows.start[b + 1] - s0, (int)(i - s0), row, len, simple != 0, lambda, out);
    for (int d = 0; d < 3; d++) A.dst[a][3 * i + d] = out[d];
  }
}

bool mo_smooth_arguments(const char* what, int method, int iterations, double lambda, double mu) {
  if (method != SE3_MESH_SMOOTH_SIMPLE && method != SE3_MESH_SMOOTH_LAPLACIAN && method != SE3_MESH_SMOOTH_TAUBIN) {
    se3_set_error("%s: method %d is none of simple, laplacian, taubin", what, method);
    return false;
  }
  if (iterations < 0 || iterations > SE3_MESH_OPS_MAX_ITERATIONS || !isfinite(lambda) || !isfinite(mu)) {
    se3_set_error("%s: %d iterations (0 .. %d), lambda %g, mu %g", what, iterations, SE3_MESH_OPS_MAX_ITERATIONS, lambda, mu);
    return false;
  }
  return true;
}

}  // namespace

// ================================================================ the entries ======================================================================
extern "C" size_t se3_mesh_incidence_workspace_bytes(int64_t n_total) {
  return n_total < 0 ? 0 : se3_align256(sizeof(int) * mo_atleast1(n_total)) + se3_align256(sizeof(int64_t) * mo_scan_tiles(n_total));
}

extern "C" int se3_mesh_incidence_stack(const int64_t* triangles, const int64_t* vertex_offsets_host, const int64_t* triangle_offsets_host, int num_meshes,
                                        int64_t* tri_row_offsets, int* tri_rows, int64_t* nbr_row_offsets, int64_t nbr_capacity, int* nbr_rows,
                                        int64_t* out_counts, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "mesh_incidence_stack";
  MeshCall c;
  if (const int rc = mo_call(what, triangles && tri_row_offsets && tri_rows && nbr_row_offsets && out_counts && workspace, vertex_offsets_host,
                             triangle_offsets_host, num_meshes, &c))
    return rc;
  SE3_REQUIRE(workspace_bytes >= se3_mesh_incidence_workspace_bytes(c.n_total), SE3_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what,
              workspace_bytes, se3_mesh_incidence_workspace_bytes(c.n_total));
  SE3_REQUIRE(nbr_capacity >= 0, SE3_ERR_INVALID_ARG, "%s: capacity %lld", what, (long long)nbr_capacity);
  if (num_meshes == 0) return SE3_OK;
  hipStream_t st = (hipStream_t)stream;
  if (nbr_rows) {                                                          // the write pass
    if (c.n_total > 0)
      mesh_incidence_neighbors_kernel<<<mo_blocks(c.n_total), kMoThreads, 0, st>>>(triangles, c, tri_row_offsets, tri_rows, nbr_row_offsets, nbr_capacity,
                                                                                   nbr_rows);
    SE3_CHECK_LAUNCH(what);
    return SE3_OK;
  }
  int* cursor = (int*)workspace;
  int64_t* tile_sums = (int64_t*)((char*)workspace + se3_align256(sizeof(int) * mo_atleast1(c.n_total)));
  const PairRows all = pg_single_rows(c.n_total);
  MO_MEMSET(out_counts, 0, sizeof(int64_t) * kMoCounts * num_meshes, what);
  MO_MEMSET(tri_row_offsets, 0, sizeof(int64_t) * (c.n_total + 1), what);
  MO_MEMSET(nbr_row_offsets, 0, sizeof(int64_t) * (c.n_total + 1), what);
  MO_MEMSET(cursor, 0, sizeof(int) * mo_atleast1(c.n_total), what);
  if (c.m_total > 0) mesh_incidence_count_kernel<<<mo_blocks(c.m_total), kMoThreads, 0, st>>>(triangles, c, tri_row_offsets, out_counts);
  mo_scan_rows<int64_t, true>(tri_row_offsets, all, tile_sums, nullptr, 0, tri_row_offsets + c.n_total, st);
  if (c.m_total > 0) mesh_incidence_fill_kernel<<<mo_blocks(c.m_total), kMoThreads, 0, st>>>(triangles, c, tri_row_offsets, cursor, tri_rows);
  if (c.n_total > 0) mesh_incidence_sort_kernel<<<mo_blocks(c.n_total), kMoThreads, 0, st>>>(triangles, c, tri_row_offsets, tri_rows, nbr_row_offsets);
  mo_scan_rows<int64_t, true>(nbr_row_offsets, all, tile_sums, nullptr, 0, nbr_row_offsets + c.n_total, st);
  mesh_incidence_totals_kernel<<<1, kPairMaxPairs, 0, st>>>(c, tri_row_offsets, nbr_row_offsets, out_counts);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" size_t se3_mesh_components_workspace_bytes(int64_t m_total) { return m_total < 0 ? 0 : mo_components_carve(m_total, nullptr, nullptr); }

extern "C" int se3_mesh_components_stack(const int64_t* triangles, const int64_t* vertex_offsets_host, const int64_t* triangle_offsets_host, int num_meshes,
                                         const int64_t* tri_row_offsets, const int* tri_rows, int64_t* out_clusters, int64_t* out_cluster_n_triangles,
                                         int64_t* out_counts, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "mesh_components_stack";
  MeshCall c;
  if (const int rc = mo_call(what, triangles && tri_row_offsets && tri_rows && out_clusters && out_cluster_n_triangles && out_counts && workspace,
                             vertex_offsets_host, triangle_offsets_host, num_meshes, &c))
    return rc;
  SE3_REQUIRE(workspace_bytes >= se3_mesh_components_workspace_bytes(c.m_total), SE3_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what,
              workspace_bytes, se3_mesh_components_workspace_bytes(c.m_total));
  if (num_meshes == 0) return SE3_OK;
  hipStream_t st = (hipStream_t)stream;
  ComponentsLayout L;
  mo_components_carve(c.m_total, (char*)workspace, &L);
  MO_MEMSET(out_counts, 0, sizeof(int64_t) * kMoCounts * num_meshes, what);
  MO_MEMSET(out_cluster_n_triangles, 0, sizeof(int64_t) * mo_atleast1(c.m_total), what);
  const unsigned blocks = mo_blocks(c.m_total);
  if (c.m_total > 0) {
    mesh_components_init_kernel<<<blocks, kMoThreads, 0, st>>>(c, L);
    mesh_components_link_kernel<<<blocks, kMoThreads, 0, st>>>(triangles, c, tri_row_offsets, tri_rows, L, out_counts);
    mesh_components_flatten_kernel<<<blocks, kMoThreads, 0, st>>>(c, L);
  }
  mo_scan_rows<int, true>(L.rank, c.t, L.tile_sums, out_counts, 1, nullptr, st);
  if (c.m_total > 0) mesh_components_label_kernel<<<blocks, kMoThreads, 0, st>>>(c, L, out_clusters, out_cluster_n_triangles);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" size_t se3_mesh_cluster_area_workspace_bytes(int64_t m_total) {
  if (m_total < 0) return 0;
  Se3Carver c(nullptr);
  c.take<int64_t>((size_t)m_total + 1);
  c.take<double>(mo_atleast1(m_total));
  c.take<int64_t>(mo_scan_tiles(m_total));
  return c.bytes();
}

extern "C" int se3_mesh_cluster_area_stack(const double* vertices, const int64_t* triangles, const int64_t* vertex_offsets_host,
                                           const int64_t* triangle_offsets_host, int num_meshes, const int64_t* cluster_n_triangles, const int64_t* order,
                                           double* out_cluster_area, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "mesh_cluster_area_stack";
  MeshCall c;
  if (const int rc = mo_call(what, vertices && triangles && cluster_n_triangles && order && out_cluster_area && workspace, vertex_offsets_host,
                             triangle_offsets_host, num_meshes, &c))
    return rc;
  SE3_REQUIRE(workspace_bytes >= se3_mesh_cluster_area_workspace_bytes(c.m_total), SE3_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what,
              workspace_bytes, se3_mesh_cluster_area_workspace_bytes(c.m_total));
  SE3_REQUIRE(c.m_total < (1ll << 33), SE3_ERR_UNSUPPORTED, "%s: %lld triangles in one call", what, (long long)c.m_total);   // (one wave per slot)
  if (num_meshes == 0 || c.m_total == 0) return SE3_OK;
  hipStream_t st = (hipStream_t)stream;
  Se3Carver carve(workspace);
  int64_t* starts = carve.take<int64_t>((size_t)c.m_total + 1);
  double* sorted_area = carve.take<double>((size_t)c.m_total);
  int64_t* tile_sums = carve.take<int64_t>(mo_scan_tiles(c.m_total));
  if (hipMemcpyAsync(starts, cluster_n_triangles, sizeof(int64_t) * c.m_total, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    se3_set_error("%s: hipMemcpyAsync failed", what);
    return SE3_ERR_LAUNCH;
  }
  MO_MEMSET(out_cluster_area, 0, sizeof(double) * c.m_total, what);
  mo_scan_rows<int64_t, true>(starts, pg_single_rows(c.m_total), tile_sums, nullptr, 0, starts + c.m_total, st);
  mesh_area_gather_kernel<<<mo_blocks(c.m_total), kMoThreads, 0, st>>>(vertices, triangles, c, order, sorted_area);
  mesh_area_sum_kernel<<<mo_blocks(c.m_total * SE3_WAVE), kMoThreads, 0, st>>>(c.m_total, starts, sorted_area, out_cluster_area);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" size_t se3_mesh_select_workspace_bytes(int64_t n_total, int64_t m_total) {
  return n_total < 0 || m_total < 0 ? 0 : mo_select_carve(n_total, m_total, nullptr, nullptr);
}

extern "C" int se3_mesh_select_stack(const double* vertices, const double* normals, const double* colors, const int64_t* triangles, const uint8_t* keep,
                                     const int64_t* vertex_offsets_host, const int64_t* triangle_offsets_host, int num_meshes,
                                     const int64_t* out_vertex_offsets_host, const int64_t* out_triangle_offsets_host, double* out_vertices,
                                     double* out_normals, double* out_colors, int64_t* out_triangles, int64_t* out_vertex_map, int64_t* out_counts,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "mesh_select_stack";
  MeshCall c;
  if (const int rc = mo_call(what, vertices && triangles && keep && out_vertex_map && out_counts && workspace, vertex_offsets_host, triangle_offsets_host,
                             num_meshes, &c))
    return rc;
  SE3_REQUIRE(workspace_bytes >= se3_mesh_select_workspace_bytes(c.n_total, c.m_total), SE3_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what,
              workspace_bytes, se3_mesh_select_workspace_bytes(c.n_total, c.m_total));
  if (num_meshes == 0) return SE3_OK;
  hipStream_t st = (hipStream_t)stream;
  SelectLayout L;
  mo_select_carve(c.n_total, c.m_total, (char*)workspace, &L);
  if (!out_vertex_offsets_host) {                                          // the count pass
    MO_MEMSET(out_counts, 0, sizeof(int64_t) * kMoCounts * num_meshes, what);
    MO_MEMSET(L.vertex_scan, 0, sizeof(int) * mo_atleast1(c.n_total), what);
    if (c.m_total > 0) mesh_select_mark_kernel<<<mo_blocks(c.m_total), kMoThreads, 0, st>>>(triangles, keep, c, L, out_counts);
    mo_scan_rows<int, false>(L.vertex_scan, c.v, L.tile_sums, out_counts, 1, nullptr, st);
    mo_scan_rows<int, false>(L.tri_scan, c.t, L.tile_sums, out_counts, 2, nullptr, st);
    if (c.n_total > 0) mesh_select_map_kernel<<<mo_blocks(c.n_total), kMoThreads, 0, st>>>(c, L, out_vertex_map);
    SE3_CHECK_LAUNCH(what);
    return SE3_OK;
  }
  SE3_REQUIRE(out_triangle_offsets_host && out_vertices && out_triangles && (out_normals || !normals) && (out_colors || !colors), SE3_ERR_INVALID_ARG,
              "%s: null pointer in the write pass", what);
  PairRows out_v, out_t;
  SE3_REQUIRE(pg_fill_rows(&out_v, out_vertex_offsets_host, num_meshes) && pg_fill_rows(&out_t, out_triangle_offsets_host, num_meshes), SE3_ERR_INVALID_ARG,
              "%s: output offsets must start at 0 and not decrease", what);
  SelectArrays A = {{vertices, normals, colors}, {out_vertices, out_normals, out_colors}};
  if (c.n_total > 0) mesh_select_vertices_kernel<<<mo_blocks(c.n_total), kMoThreads, 0, st>>>(c, out_v, L, A);
  if (c.m_total > 0) mesh_select_triangles_kernel<<<mo_blocks(c.m_total), kMoThreads, 0, st>>>(triangles, c, out_t, L, out_triangles);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" int se3_mesh_normals_stack(const double* vertices, const int64_t* triangles, const int64_t* vertex_offsets_host,
                                      const int64_t* triangle_offsets_host, int num_meshes, const int64_t* tri_row_offsets, const int* tri_rows,
                                      int normalized, double* out_triangle_normals, double* out_vertex_normals, int64_t* out_counts, void* stream) {
  const char* what = "mesh_normals_stack";
  MeshCall c;
  if (const int rc = mo_call(what, vertices && triangles && (out_triangle_normals || out_vertex_normals) && (!out_vertex_normals || (tri_row_offsets && tri_rows)),
                             vertex_offsets_host, triangle_offsets_host, num_meshes, &c))
    return rc;
  if (num_meshes == 0) return SE3_OK;
  hipStream_t st = (hipStream_t)stream;
  if (out_counts) MO_MEMSET(out_counts, 0, sizeof(int64_t) * kMoCounts * num_meshes, what);
  if (out_triangle_normals && c.m_total > 0)
    mesh_triangle_normals_kernel<<<mo_blocks(c.m_total), kMoThreads, 0, st>>>(vertices, triangles, c, normalized, out_triangle_normals, out_counts);
  if (out_vertex_normals && c.n_total > 0)
    mesh_vertex_normals_kernel<<<mo_blocks(c.n_total), kMoThreads, 0, st>>>(vertices, triangles, c, tri_row_offsets, tri_rows, out_vertex_normals);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" size_t se3_mesh_smooth_workspace_bytes(int64_t n_total, int num_arrays) {
  return n_total < 0 || num_arrays < 1 || num_arrays > 3 ? 0 : se3_align256(sizeof(double) * 3 * mo_atleast1(n_total)) * (size_t)num_arrays;
}

extern "C" int se3_mesh_smooth_stack(const double* vertices, const double* normals, const double* colors, const int64_t* vertex_offsets_host, int num_meshes,
                                     const int64_t* nbr_row_offsets, const int* nbr_rows, int method, int iterations, double lambda, double mu,
                                     double* out_vertices, double* out_normals, double* out_colors, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "mesh_smooth_stack";
  SE3_REQUIRE(vertices && vertex_offsets_host && nbr_row_offsets && nbr_rows && out_vertices && workspace && (out_normals || !normals) &&
                  (out_colors || !colors),
              SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(num_meshes >= 0 && num_meshes <= kPairMaxPairs, SE3_ERR_INVALID_ARG, "%s: %d meshes (at most %d)", what, num_meshes, kPairMaxPairs);
  if (!mo_smooth_arguments(what, method, iterations, lambda, mu)) return SE3_ERR_INVALID_ARG;
  PairRows rows;
  SE3_REQUIRE(pg_fill_rows(&rows, vertex_offsets_host, num_meshes), SE3_ERR_INVALID_ARG, "%s: offsets must start at 0 and not decrease", what);
  const int64_t n_total = rows.start[num_meshes];
  const double* in[3] = {vertices, normals, colors};
  double* out[3] = {out_vertices, out_normals, out_colors};
  int arrays = 0;
  for (int a = 0; a < 3; a++)
    if (in[a]) in[arrays] = in[a], out[arrays] = out[a], arrays++;
  SE3_REQUIRE(workspace_bytes >= se3_mesh_smooth_workspace_bytes(n_total, arrays), SE3_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what,
              workspace_bytes, se3_mesh_smooth_workspace_bytes(n_total, arrays));
  if (n_total == 0) return SE3_OK;
  hipStream_t st = (hipStream_t)stream;
  const int steps = iterations * (method == SE3_MESH_SMOOTH_TAUBIN ? 2 : 1);
  const size_t bytes = sizeof(double) * 3 * (size_t)n_total;
  if (steps == 0) {
    for (int a = 0; a < arrays; a++)
      if (hipMemcpyAsync(out[a], in[a], bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        se3_set_error("%s: hipMemcpyAsync failed", what);
        return SE3_ERR_LAUNCH;
      }
    return SE3_OK;
  }
  // step s writes the output when an even number of steps follows it, else the workspace: the last step lands in the output
  SmoothArrays A;
  A.count = arrays;
  for (int s = 0; s < steps; s++) {
    const bool to_out = (steps - 1 - s) % 2 == 0;
    for (int a = 0; a < 3; a++) {
      double* tmp = a < arrays ? (double*)((char*)workspace + (size_t)a * se3_align256(bytes)) : nullptr;
      A.src[a] = a >= arrays ? nullptr : (s == 0 ? in[a] : (to_out ? tmp : out[a]));
      A.dst[a] = a >= arrays ? nullptr : (to_out ? out[a] : tmp);
    }
    const double step = method == SE3_MESH_SMOOTH_TAUBIN && s % 2 == 1 ? mu : lambda;
    mesh_smooth_kernel<<<mo_blocks(n_total), kMoThreads, 0, st>>>(rows, n_total, nbr_row_offsets, nbr_rows, method == SE3_MESH_SMOOTH_SIMPLE, step, A);
  }
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

// ================================== the same text on host memory, one mesh, serially, no GPU (tests/test_mesh_ops_cpu.py) ===========================
namespace {
bool mo_host_sizes(const char* what, int64_t n, int64_t m) {
  if (n >= 0 && n < kMoMaxRows && m >= 0 && m < kMoMaxRows) return true;
  se3_set_error("%s: %lld vertices, %lld triangles: each below 2^31", what, (long long)n, (long long)m);
  return false;
}
}  // namespace

// tri_row_offsets, nbr_row_offsets (n + 1); tri_rows (3 m); nbr_rows NULL: the counts alone.  out_counts: status, incidences, neighbours, 0.
extern "C" int se3_debug_mesh_incidence_host(const int64_t* triangles, int64_t n, int64_t m, int64_t* tri_row_offsets, int* tri_rows,
                                             int64_t* nbr_row_offsets, int64_t nbr_capacity, int* nbr_rows, int64_t* out_counts) {
  const char* what = "debug_mesh_incidence_host";
  SE3_REQUIRE((triangles || m == 0) && tri_row_offsets && tri_rows && nbr_row_offsets && out_counts, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  if (!mo_host_sizes(what, n, m)) return SE3_ERR_UNSUPPORTED;
  int64_t status = 0;
  std::vector<int> cursor((size_t)n, 0);
  for (int64_t i = 0; i <= n; i++) tri_row_offsets[i] = 0;
  int w[3], d[3];
  for (int64_t t = 0; t < m; t++) {
    if (!mo_triangle(triangles, t, n, w)) {
      status |= SE3_MESH_OPS_BAD_TRIANGLE;
      continue;
    }
    const int k = mo_distinct(w, d);
    for (int j = 0; j < k; j++) tri_row_offsets[d[j]]++;
  }
  int64_t run = 0;
  for (int64_t i = 0; i <= n; i++) {
    const int64_t count = tri_row_offsets[i];
    tri_row_offsets[i] = run;
    run += i < n ? count : 0;
  }
  for (int64_t t = m - 1; t >= 0; t--) {                                  // (descending: the sort below has work to do, as on the device)
    if (!mo_triangle(triangles, t, n, w)) continue;
    const int k = mo_distinct(w, d);
    for (int j = 0; j < k; j++) tri_rows[tri_row_offsets[d[j]] + cursor[d[j]]++] = (int)t;
  }
  run = 0;
  for (int64_t i = 0; i < n; i++) {
    int* row = tri_rows + tri_row_offsets[i];
    const int64_t len = tri_row_offsets[i + 1] - tri_row_offsets[i];
    mo_sort_row(row, len);
    nbr_row_offsets[i] = run;
    run += mo_neighbors(triangles, m, n, row, len, (int)i, nullptr, 0);
  }
  nbr_row_offsets[n] = run;
  out_counts[0] = status, out_counts[1] = tri_row_offsets[n], out_counts[2] = run, out_counts[3] = 0;
  if (nbr_rows)
    for (int64_t i = 0; i < n; i++) {
      const int64_t at = nbr_row_offsets[i], end = nbr_row_offsets[i + 1];
      if (end > nbr_capacity) continue;
      mo_neighbors(triangles, m, n, tri_rows + tri_row_offsets[i], tri_row_offsets[i + 1] - tri_row_offsets[i], (int)i, nbr_rows + at, end - at);
    }
  return SE3_OK;
}

// out_clusters (m); out_cluster_n_triangles, out_cluster_area (m: the first k are the clusters'); out_counts: status, k, 0, 0
extern "C" int se3_debug_mesh_components_host(const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const int64_t* tri_row_offsets,
                                              const int* tri_rows, int64_t* out_clusters, int64_t* out_cluster_n_triangles, double* out_cluster_area,
                                              int64_t* out_counts) {
  const char* what = "debug_mesh_components_host";
  SE3_REQUIRE((vertices || n == 0) && (triangles || m == 0) && tri_row_offsets && tri_rows && out_clusters && out_cluster_n_triangles && out_cluster_area &&
                  out_counts,
              SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  if (!mo_host_sizes(what, n, m)) return SE3_ERR_UNSUPPORTED;
  std::vector<int> parent((size_t)m), rank((size_t)m);
  int64_t status = 0;
  int w[3];
  for (int64_t t = 0; t < m; t++) parent[t] = (int)t;
  for (int64_t t = 0; t < m; t++) {
    if (!mo_triangle(triangles, t, n, w)) status |= SE3_MESH_OPS_BAD_TRIANGLE;
    mo_link_triangle(
        triangles, m, n, (int)t, tri_row_offsets, tri_rows, [&](int x) { return parent[x]; }, [&](int x, int v) { if (v < parent[x]) parent[x] = v; },
        [&](int a, int r) {
          const int old = parent[a];
          if (old == a) parent[a] = r;
          return old;
        });
  }
  int k = 0;
  for (int64_t t = 0; t < m; t++) {
    int x = (int)t;
    while (parent[x] != x) x = parent[x];
    rank[t] = k;
    k += x == (int)t ? 1 : 0;
  }
  std::vector<std::vector<double>> areas((size_t)k);
  for (int64_t t = 0; t < m; t++) {
    int x = (int)t;
    while (parent[x] != x) x = parent[x];
    out_clusters[t] = rank[x];
    areas[(size_t)rank[x]].push_back(mo_triangle_area(vertices, triangles, t, n));
    out_cluster_n_triangles[t] = 0, out_cluster_area[t] = 0.0;
  }
  for (int c = 0; c < k; c++) {
    out_cluster_n_triangles[c] = (int64_t)areas[(size_t)c].size();
    out_cluster_area[c] = mo_tree_sum_host(areas[(size_t)c].data(), (int64_t)areas[(size_t)c].size());
  }
  out_counts[0] = status, out_counts[1] = k, out_counts[2] = 0, out_counts[3] = 0;
  return SE3_OK;
}

// out_vertices NULL: the counts and the map alone.  out_counts: status, vertices kept, triangles kept, 0.
extern "C" int se3_debug_mesh_select_host(const double* vertices, const double* normals, const double* colors, const int64_t* triangles,
                                          const uint8_t* keep, int64_t n, int64_t m, int64_t vertex_capacity, int64_t triangle_capacity,
                                          double* out_vertices, double* out_normals, double* out_colors, int64_t* out_triangles, int64_t* out_vertex_map,
                                          int64_t* out_counts) {
  const char* what = "debug_mesh_select_host";
  SE3_REQUIRE((vertices || n == 0) && ((triangles && keep) || m == 0) && out_vertex_map && out_counts, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(!out_vertices || (out_triangles && (out_normals || !normals) && (out_colors || !colors)), SE3_ERR_INVALID_ARG,
              "%s: null pointer in the write pass", what);
  if (!mo_host_sizes(what, n, m)) return SE3_ERR_UNSUPPORTED;
  int64_t status = 0, kept_vertices = 0, kept_triangles = 0;
  int w[3];
  for (int64_t i = 0; i < n; i++) out_vertex_map[i] = 0;
  for (int64_t t = 0; t < m; t++) {
    const bool valid = mo_triangle(triangles, t, n, w);
    if (!valid) status |= SE3_MESH_OPS_BAD_TRIANGLE;
    if (valid && keep[t])
      for (int j = 0; j < 3; j++) out_vertex_map[w[j]] = 1;
  }
  for (int64_t i = 0; i < n; i++) out_vertex_map[i] = out_vertex_map[i] ? kept_vertices++ : -1;
  const double* src[3] = {vertices, normals, colors};
  double* dst[3] = {out_vertices, out_normals, out_colors};
  for (int64_t t = 0; t < m; t++) {
    if (!mo_triangle(triangles, t, n, w) || !keep[t]) continue;
    if (out_vertices && kept_triangles < triangle_capacity)
      for (int j = 0; j < 3; j++) out_triangles[3 * kept_triangles + j] = out_vertex_map[w[j]];
    kept_triangles++;
  }
  if (out_vertices)
    for (int64_t i = 0; i < n; i++) {
      const int64_t row = out_vertex_map[i];
      if (row < 0 || row >= vertex_capacity) continue;
      for (int a = 0; a < 3; a++)
        if (src[a])
          for (int d = 0; d < 3; d++) dst[a][3 * row + d] = src[a][3 * i + d];
    }
  out_counts[0] = status, out_counts[1] = kept_vertices, out_counts[2] = kept_triangles, out_counts[3] = 0;
  return SE3_OK;
}

extern "C" int se3_debug_mesh_normals_host(const double* vertices, const int64_t* triangles, int64_t n, int64_t m, const int64_t* tri_row_offsets,
                                           const int* tri_rows, int normalized, double* out_triangle_normals, double* out_vertex_normals) {
  const char* what = "debug_mesh_normals_host";
  SE3_REQUIRE((vertices || n == 0) && (triangles || m == 0) && (out_triangle_normals || out_vertex_normals) &&
                  (!out_vertex_normals || (tri_row_offsets && tri_rows)),
              SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  if (!mo_host_sizes(what, n, m)) return SE3_ERR_UNSUPPORTED;
  if (out_triangle_normals)
    for (int64_t t = 0; t < m; t++) {
      mo_triangle_normal(vertices, triangles, t, n, out_triangle_normals + 3 * t);
      if (normalized) mo_normalize(out_triangle_normals + 3 * t);
    }
  if (out_vertex_normals)
    for (int64_t i = 0; i < n; i++)
      mo_vertex_normal(vertices, triangles, m, n, tri_rows + tri_row_offsets[i], tri_row_offsets[i + 1] - tri_row_offsets[i], out_vertex_normals + 3 * i);
  return SE3_OK;
}

// one (n, 3) array, positions or an attribute, through the steps of se3_mesh_smooth_stack
extern "C" int se3_debug_mesh_smooth_host(const double* values, int64_t n, const int64_t* nbr_row_offsets, const int* nbr_rows, int method, int iterations,
                                          double lambda, double mu, double* out_values) {
  const char* what = "debug_mesh_smooth_host";
  SE3_REQUIRE(((values && out_values) || n == 0) && nbr_row_offsets && (nbr_rows || nbr_row_offsets[n > 0 ? n : 0] == 0), SE3_ERR_INVALID_ARG,
              "%s: null pointer", what);
  if (!mo_host_sizes(what, n, 0)) return SE3_ERR_UNSUPPORTED;
  if (!mo_smooth_arguments(what, method, iterations, lambda, mu)) return SE3_ERR_INVALID_ARG;
  std::vector<double> a(values, values + 3 * n), b((size_t)(3 * n));
  const int steps = iterations * (method == SE3_MESH_SMOOTH_TAUBIN ? 2 : 1);
  for (int s = 0; s < steps; s++) {
    const double step = method == SE3_MESH_SMOOTH_TAUBIN && s % 2 == 1 ? mu : lambda;
    for (int64_t i = 0; i < n; i++)
      mo_smooth(a.data(), n, (int)i, nbr_rows + nbr_row_offsets[i], nbr_row_offsets[i + 1] - nbr_row_offsets[i], method == SE3_MESH_SMOOTH_SIMPLE, step,
                b.data() + 3 * i);
    a.swap(b);
  }
  if (n > 0) memcpy(out_values, a.data(), sizeof(double) * 3 * (size_t)n);
  return SE3_OK;
}

// ================================================================ vertex clustering ===================================================================
// Open3D's simplify_vertex_clustering with contraction = Average (se3et_amd/mesh.py carries the same contract).
//   - per mesh o_d = min_d - voxel_size / 2 and cell_d = floor((v_d - o_d) / voxel_size), the text of csrc/voxel_key.h that voxel_down_sample
//     runs; a mesh is refused (a status bit) when a vertex or an attribute is not finite or an axis would need 2^21 cells or more.
//   - the vertices of a cell become one vertex: the mean of positions and attributes, summed in ascending vertex order, divided once.
//   - new vertices stand in ascending (x, y, z) cell order (Open3D's order is its hash map's).
//   - triangles are remapped; one with two equal new vertices is dropped; a survivor is rotated, not sorted, so that its lowest vertex comes
//     first; of equal triangles the first in the original order stays; survivors keep the original order.
// Both orders are sorts of integer keys, which the caller does between the passes (torch.sort, stable); the passes validate every place of
// an order before they read through it.
namespace {

constexpr int kMoClusterThreads = 256;

struct ClusterMeta {
  double org[3];
  int ok;
};

struct ClusterLayout {
  ClusterMeta* meta;   // [B]
  int* vertex_scan;    // [n_total]: "first of its cell" over the sorted places, then the inclusive scan per mesh
  int64_t* cell_start; // [n_total]: the sorted place where new vertex (mesh start + number) begins
  int* tri_scan;       // [m_total]: "stays" per triangle, then the inclusive scan per mesh
  int* tile_sums;      // mo_scan_tiles(max(n_total, m_total))
};

size_t mo_cluster_carve(int64_t n_total, int64_t m_total, char* base, ClusterLayout* L) {
  Se3Carver c(base);
  ClusterLayout l;
  l.meta = c.take<ClusterMeta>(kPairMaxPairs);
  l.vertex_scan = c.take<int>(mo_atleast1(n_total));
  l.cell_start = c.take<int64_t>(mo_atleast1(n_total));
  l.tri_scan = c.take<int>(mo_atleast1(m_total));
  l.tile_sums = c.take<int>(mo_scan_tiles(n_total > m_total ? n_total : m_total));
  if (L) *L = l;
  return c.bytes();
}

struct ClusterArrays {
  const double* src[3];
  double* dst[3];
};

__global__ __launch_bounds__(kMoClusterThreads) void mesh_cluster_bounds_kernel(ClusterArrays A, MeshCall c, double voxel_size, ClusterLayout L,
                                                                                int64_t* __restrict__ counts) {
  __shared__ double sh[kMoClusterThreads / 64];
  __shared__ int bad;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool finite = true;
  for (int64_t i = c.v.start[b] + threadIdx.x; i < c.v.start[b + 1]; i += kMoClusterThreads)
    for (int d = 0; d < 3; d++) {
      const double v = A.src[0][3 * i + d];
      finite = finite && isfinite(v) && (!A.src[1] || isfinite(A.src[1][3 * i + d])) && (!A.src[2] || isfinite(A.src[2][3 * i + d]));
      mn[d] = fmin(mn[d], v), mx[d] = fmax(mx[d], v);
    }
  if (!finite) bad = 1;                                                   // (every writer stores the same word)
  se3_block_bounds<double, kMoClusterThreads>(mn, mx, sh);
  if (threadIdx.x == 0) {
    int flags = bad ? SE3_MESH_OPS_NONFINITE : 0;
    for (int d = 0; d < 3; d++) {
      L.meta[b].org[d] = vd_origin(mn[d], voxel_size);
      if (c.v.start[b + 1] > c.v.start[b] && !flags && !vd_axis_ok(mx[d], L.meta[b].org[d], voxel_size)) flags |= SE3_MESH_OPS_TOO_MANY_CELLS;
    }
    L.meta[b].ok = flags == 0;
    if (flags) atomicOr((unsigned long long*)(counts + kMoCounts * b), (unsigned long long)flags);
  }
}

__global__ __launch_bounds__(kMoClusterThreads) void mesh_cluster_keys_kernel(const double* __restrict__ vertices, MeshCall c, double voxel_size,
                                                                              ClusterLayout L, int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kMoClusterThreads + threadIdx.x;
  if (i >= c.n_total) return;
  const ClusterMeta& m = L.meta[pg_pair_of_row(c.v, i)];
  keys[i] = m.ok ? vd_key_xyz(vertices + 3 * i, m.org, voxel_size) : 0;
}

__global__ __launch_bounds__(kMoClusterThreads) void mesh_cluster_first_kernel(MeshCall c, const int64_t* __restrict__ sorted_keys, ClusterLayout L) {
  const int64_t i = (int64_t)blockIdx.x * kMoClusterThreads + threadIdx.x;
  if (i >= c.n_total) return;
  L.vertex_scan[i] = i == c.v.start[pg_pair_of_row(c.v, i)] || sorted_keys[i] != sorted_keys[i - 1] ? 1 : 0;
}

__global__ __launch_bounds__(kMoClusterThreads) void mesh_cluster_map_kernel(MeshCall c, const int64_t* __restrict__ order, ClusterLayout L,
                                                                             int64_t* __restrict__ vertex_map) {
  const int64_t i = (int64_t)blockIdx.x * kMoClusterThreads + threadIdx.x;
  if (i >= c.n_total) return;
  const int b = pg_pair_of_row(c.v, i);
  const int64_t s0 = c.v.start[b], o = order[i];
  const int before = i > s0 ? L.vertex_scan[i - 1] : 0, number = L.vertex_scan[i] - 1;
  if (L.vertex_scan[i] != before) L.cell_start[s0 + number] = i;
  if (o >= s0 && o < c.v.start[b + 1]) vertex_map[o] = number;
}

__global__ __launch_bounds__(kMoClusterThreads) void mesh_cluster_remap_kernel(const int64_t* __restrict__ tri, MeshCall c, const int64_t* __restrict__ vertex_map,
                                                                               int64_t* __restrict__ rotated, int64_t* __restrict__ counts) {
  const int64_t t = (int64_t)blockIdx.x * kMoClusterThreads + threadIdx.x;
  if (t >= c.m_total) return;
  const int b = pg_pair_of_row(c.t, t);
  int w[3];
  int64_t r[3] = {-1, -1, -1};
  if (!mo_triangle(tri, t, c.v.start[b + 1] - c.v.start[b], w)) {
    atomicOr((unsigned long long*)(counts + kMoCounts * b), (unsigned long long)SE3_MESH_OPS_BAD_TRIANGLE);
  } else {
    const int64_t* map = vertex_map + c.v.start[b];
    if (map[w[0]] < 0 || map[w[1]] < 0 || map[w[2]] < 0 || !mo_rotate(map[w[0]], map[w[1]], map[w[2]], r)) r[0] = r[1] = r[2] = -1;
  }
  for (int j = 0; j < 3; j++) rotated[3 * t + j] = r[j];
}

// one thread per place of the triangle order: the triangle there stays iff it survived and the place before holds another triple
__global__ __launch_bounds__(kMoClusterThreads) void mesh_cluster_stay_kernel(MeshCall c, const int64_t* __restrict__ rotated, const int64_t* __restrict__ order,
                                                                              ClusterLayout L) {
  const int64_t j = (int64_t)blockIdx.x * kMoClusterThreads + threadIdx.x;
  if (j >= c.m_total) return;
  const int b = pg_pair_of_row(c.t, j);
  const int64_t s0 = c.t.start[b], s1 = c.t.start[b + 1], t = order[j];
  if (t < s0 || t >= s1 || rotated[3 * t] < 0) return;                     // (tri_scan was cleared)
  bool stays = true;
  if (j > s0) {
    const int64_t p = order[j - 1];
    stays = p < s0 || p >= s1 || rotated[3 * p] != rotated[3 * t] || rotated[3 * p + 1] != rotated[3 * t + 1] || rotated[3 * p + 2] != rotated[3 * t + 2];
  }
  if (stays) L.tri_scan[t] = 1;
}

__global__ __launch_bounds__(kMoClusterThreads) void mesh_cluster_vertices_kernel(MeshCall c, PairRows out_v, const int64_t* __restrict__ order, ClusterLayout L,
                                                                                  const int64_t* __restrict__ counts, ClusterArrays A) {
  const int64_t i = (int64_t)blockIdx.x * kMoClusterThreads + threadIdx.x;
  if (i >= c.n_total) return;
  const int b = pg_pair_of_row(c.v, i);
  const int64_t s0 = c.v.start[b], s1 = c.v.start[b + 1], number = i - s0, total = counts[kMoCounts * b + 1];
  if (number >= total || out_v.start[b] + number >= out_v.start[b + 1]) return;
  const int64_t begin = L.cell_start[i], end = number + 1 < total ? L.cell_start[i + 1] : s1;
  if (begin < s0 || end > s1 || end <= begin) return;
  const int64_t row = out_v.start[b] + number;
  for (int a = 0; a < 3; a++)
    if (A.src[a]) mo_cluster_mean(A.src[a] + 3 * s0, s1 - s0, order + begin, s0, end - begin, A.dst[a] + 3 * row);
}

__global__ __launch_bounds__(kMoClusterThreads) void mesh_cluster_triangles_kernel(MeshCall c, PairRows out_t, const int64_t* __restrict__ rotated, ClusterLayout L,
                                                                                   int64_t* __restrict__ out_triangles) {
  const int64_t t = (int64_t)blockIdx.x * kMoClusterThreads + threadIdx.x;
  if (t >= c.m_total) return;
  const int b = pg_pair_of_row(c.t, t);
  const int place = mo_kept_place(L.tri_scan, c.t.start[b], t);
  if (place < 0 || out_t.start[b] + place >= out_t.start[b + 1]) return;
  for (int j = 0; j < 3; j++) out_triangles[3 * (out_t.start[b] + place) + j] = rotated[3 * t + j];
}

}  // namespace

extern "C" size_t se3_mesh_cluster_vertices_workspace_bytes(int64_t n_total, int64_t m_total) {
  return n_total < 0 || m_total < 0 ? 0 : mo_cluster_carve(n_total, m_total, nullptr, nullptr);
}

extern "C" int se3_mesh_cluster_vertices_stack(int pass, const double* vertices, const double* normals, const double* colors, const int64_t* triangles,
                                               const int64_t* vertex_offsets_host, const int64_t* triangle_offsets_host, int num_meshes, double voxel_size,
                                               int64_t* keys, const int64_t* sorted_keys, const int64_t* vertex_order, int64_t* vertex_map,
                                               int64_t* rotated, const int64_t* triangle_order, const int64_t* out_vertex_offsets_host,
                                               const int64_t* out_triangle_offsets_host, double* out_vertices, double* out_normals, double* out_colors,
                                               int64_t* out_triangles, int64_t* out_counts, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "mesh_cluster_vertices_stack";
  MeshCall c;
  if (const int rc = mo_call(what, vertices && triangles && out_counts && workspace, vertex_offsets_host, triangle_offsets_host, num_meshes, &c)) return rc;
  SE3_REQUIRE(isfinite(voxel_size) && voxel_size > 0.0, SE3_ERR_INVALID_ARG, "%s: voxel size %g is not a positive finite number", what, voxel_size);
  SE3_REQUIRE(workspace_bytes >= se3_mesh_cluster_vertices_workspace_bytes(c.n_total, c.m_total), SE3_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed",
              what, workspace_bytes, se3_mesh_cluster_vertices_workspace_bytes(c.n_total, c.m_total));
  if (num_meshes == 0) return SE3_OK;
  hipStream_t st = (hipStream_t)stream;
  ClusterLayout L;
  mo_cluster_carve(c.n_total, c.m_total, (char*)workspace, &L);
  const unsigned vblocks = (unsigned)se3_cdiv(c.n_total, kMoClusterThreads), tblocks = (unsigned)se3_cdiv(c.m_total, kMoClusterThreads);
  if (pass == SE3_MESH_CLUSTER_KEYS) {
    SE3_REQUIRE(keys, SE3_ERR_INVALID_ARG, "%s: null pointer in the key pass", what);
    MO_MEMSET(out_counts, 0, sizeof(int64_t) * kMoCounts * num_meshes, what);
    ClusterArrays A = {{vertices, normals, colors}, {nullptr, nullptr, nullptr}};
    mesh_cluster_bounds_kernel<<<(unsigned)num_meshes, kMoClusterThreads, 0, st>>>(A, c, voxel_size, L, out_counts);
    if (c.n_total > 0) mesh_cluster_keys_kernel<<<vblocks, kMoClusterThreads, 0, st>>>(vertices, c, voxel_size, L, keys);
  } else if (pass == SE3_MESH_CLUSTER_VERTICES) {
    SE3_REQUIRE(sorted_keys && vertex_order && vertex_map && rotated, SE3_ERR_INVALID_ARG, "%s: null pointer in the vertex pass", what);
    MO_MEMSET(vertex_map, 0xff, sizeof(int64_t) * mo_atleast1(c.n_total), what);          // -1: a vertex that no place of the order names
    if (c.n_total > 0) mesh_cluster_first_kernel<<<vblocks, kMoClusterThreads, 0, st>>>(c, sorted_keys, L);
    mo_scan_rows<int, false>(L.vertex_scan, c.v, L.tile_sums, out_counts, 1, nullptr, st);
    if (c.n_total > 0) mesh_cluster_map_kernel<<<vblocks, kMoClusterThreads, 0, st>>>(c, vertex_order, L, vertex_map);
    if (c.m_total > 0) mesh_cluster_remap_kernel<<<tblocks, kMoClusterThreads, 0, st>>>(triangles, c, vertex_map, rotated, out_counts);
  } else if (pass == SE3_MESH_CLUSTER_TRIANGLES) {
    SE3_REQUIRE(rotated && triangle_order, SE3_ERR_INVALID_ARG, "%s: null pointer in the triangle pass", what);
    MO_MEMSET(L.tri_scan, 0, sizeof(int) * mo_atleast1(c.m_total), what);
    if (c.m_total > 0) mesh_cluster_stay_kernel<<<tblocks, kMoClusterThreads, 0, st>>>(c, rotated, triangle_order, L);
    mo_scan_rows<int, false>(L.tri_scan, c.t, L.tile_sums, out_counts, 2, nullptr, st);
  } else if (pass == SE3_MESH_CLUSTER_WRITE) {
    SE3_REQUIRE(vertex_order && rotated && out_vertex_offsets_host && out_triangle_offsets_host && out_vertices && out_triangles &&
                    (out_normals || !normals) && (out_colors || !colors),
                SE3_ERR_INVALID_ARG, "%s: null pointer in the write pass", what);
    PairRows out_v, out_t;
    SE3_REQUIRE(pg_fill_rows(&out_v, out_vertex_offsets_host, num_meshes) && pg_fill_rows(&out_t, out_triangle_offsets_host, num_meshes), SE3_ERR_INVALID_ARG,
                "%s: output offsets must start at 0 and not decrease", what);
    ClusterArrays A = {{vertices, normals, colors}, {out_vertices, out_normals, out_colors}};
    if (c.n_total > 0) mesh_cluster_vertices_kernel<<<vblocks, kMoClusterThreads, 0, st>>>(c, out_v, vertex_order, L, out_counts, A);
    if (c.m_total > 0) mesh_cluster_triangles_kernel<<<tblocks, kMoClusterThreads, 0, st>>>(c, out_t, rotated, L, out_triangles);
  } else {
    SE3_REQUIRE(false, SE3_ERR_INVALID_ARG, "%s: pass %d", what, pass);
  }
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

// out_vertices NULL: the counts and the map alone.  out_counts: status, new vertices, triangles that stay, 0.
extern "C" int se3_debug_mesh_cluster_vertices_host(const double* vertices, const double* normals, const double* colors, const int64_t* triangles, int64_t n,
                                                    int64_t m, double voxel_size, int64_t vertex_capacity, int64_t triangle_capacity, double* out_vertices,
                                                    double* out_normals, double* out_colors, int64_t* out_triangles, int64_t* out_vertex_map,
                                                    int64_t* out_counts) {
  const char* what = "debug_mesh_cluster_vertices_host";
  SE3_REQUIRE((vertices || n == 0) && (triangles || m == 0) && out_vertex_map && out_counts, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(!out_vertices || (out_triangles && (out_normals || !normals) && (out_colors || !colors)), SE3_ERR_INVALID_ARG,
              "%s: null pointer in the write pass", what);
  SE3_REQUIRE(isfinite(voxel_size) && voxel_size > 0.0, SE3_ERR_INVALID_ARG, "%s: voxel size %g is not a positive finite number", what, voxel_size);
  if (!mo_host_sizes(what, n, m)) return SE3_ERR_UNSUPPORTED;
  const double* src[3] = {vertices, normals, colors};
  double* dst[3] = {out_vertices, out_normals, out_colors};
  int64_t status = 0;
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, org[3];
  for (int64_t i = 0; i < 3 * n; i++) {
    for (int a = 0; a < 3; a++)
      if (src[a] && !isfinite(src[a][i])) status = SE3_MESH_OPS_NONFINITE;
    mn[i % 3] = fmin(mn[i % 3], vertices[i]), mx[i % 3] = fmax(mx[i % 3], vertices[i]);
  }
  for (int d = 0; d < 3; d++) {
    org[d] = vd_origin(mn[d], voxel_size);
    if (n > 0 && !status && !vd_axis_ok(mx[d], org[d], voxel_size)) status |= SE3_MESH_OPS_TOO_MANY_CELLS;
  }
  out_counts[0] = status, out_counts[1] = 0, out_counts[2] = 0, out_counts[3] = 0;
  for (int64_t i = 0; i < n; i++) out_vertex_map[i] = -1;
  if (status) return SE3_OK;
  std::vector<int64_t> keys((size_t)n), order((size_t)n), begin;
  for (int64_t i = 0; i < n; i++) keys[i] = vd_key_xyz(vertices + 3 * i, org, voxel_size), order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return keys[a] < keys[b]; });
  for (int64_t i = 0; i < n; i++) {
    if (i == 0 || keys[order[i]] != keys[order[i - 1]]) begin.push_back(i);
    out_vertex_map[order[i]] = (int64_t)begin.size() - 1;
  }
  const int64_t cells = (int64_t)begin.size();
  begin.push_back(n);
  std::vector<int64_t> rotated((size_t)(3 * m)), by_triple;
  int w[3];
  for (int64_t t = 0; t < m; t++) {
    int64_t* r = rotated.data() + 3 * t;
    r[0] = r[1] = r[2] = -1;
    if (!mo_triangle(triangles, t, n, w)) {
      status |= SE3_MESH_OPS_BAD_TRIANGLE;
      continue;
    }
    if (mo_rotate(out_vertex_map[w[0]], out_vertex_map[w[1]], out_vertex_map[w[2]], r)) by_triple.push_back(t);
    else r[0] = r[1] = r[2] = -1;
  }
  auto less = [&](int64_t a, int64_t b) {
    for (int j = 0; j < 3; j++)
      if (rotated[3 * a + j] != rotated[3 * b + j]) return rotated[3 * a + j] < rotated[3 * b + j];
    return false;
  };
  std::stable_sort(by_triple.begin(), by_triple.end(), less);
  std::vector<uint8_t> stays((size_t)m, 0);
  for (size_t j = 0; j < by_triple.size(); j++) stays[(size_t)by_triple[j]] = j == 0 || less(by_triple[j - 1], by_triple[j]);
  int64_t kept = 0;
  for (int64_t t = 0; t < m; t++) {
    if (!stays[(size_t)t]) continue;
    if (out_vertices && kept < triangle_capacity)
      for (int j = 0; j < 3; j++) out_triangles[3 * kept + j] = rotated[3 * t + j];
    kept++;
  }
  if (out_vertices)
    for (int64_t v = 0; v < cells && v < vertex_capacity; v++)
      for (int a = 0; a < 3; a++)
        if (src[a]) mo_cluster_mean(src[a], n, order.data() + begin[v], 0, begin[v + 1] - begin[v], dst[a] + 3 * v);
  out_counts[0] = status, out_counts[1] = cells, out_counts[2] = kept;
  return SE3_OK;
}
