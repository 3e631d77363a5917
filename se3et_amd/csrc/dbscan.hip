// DBSCAN clustering of stacked clouds (Open3D's cluster_dbscan, scikit-learn's DBSCAN) for up to SE3_PAIR_MAX_PAIRS clouds per call, on the
// float64 grid of csrc/pair_grid.h built over the clouds themselves with cell_hint = eps.  se3et_amd/segmentation.py carries the same
// contract; csrc/dbscan_core.h holds the shared text and the termination argument of the link loop.
// (SE3_EXACT_FP: the file is built with contraction off, and pg_dist2 fences itself as well.)
//
// Contract (the answer is integers and a pure function of the cloud).
//   1. j is a neighbour of i iff pg_dist2(p_i, p_j) < eps eps, strictly, i itself included: the ball query's own test, the one
//      remove_radius_outlier_clouds counts with.
//   2. i is a core row iff its neighbour count >= min_points.
//   3. Clusters are the connected components of the core rows under that relation, numbered 0, 1, .. in ascending order of each
//      component's lowest core row index.
//   4. A non-core row with at least one core neighbour gets the lowest label among its core neighbours; every other non-core row gets -1.
//   3 and 4 are what the index-order sweep with breadth-first expansion of Open3D and scikit-learn produces.  scikit-learn tests
//   d <= eps; a cloud with no pair distance at eps itself gets the same labels from both.
//
// Five launches, nothing read back, integer atomics only (the partition does not depend on their order):
//   dbscan_core_kernel     one thread per row: the ball count, the core byte, parent[i] = i.
//   dbscan_link_kernel     one thread per core row: walks its ball on the grid and unites itself with every core neighbour of a lower
//                          index (db_union: the larger root is hooked under the smaller by a compare-and-swap, paths are halved by an
//                          atomic minimum; no lock, no wait for another workgroup).  The walk visits the cells pg_ball_walk visits: a second
//                          walk instead of the (i, j) list of se3_pair_ball_fill_stack, which at ~20 neighbours would cost 320 bytes a row.
//   dbscan_flatten_kernel  one thread per row: a core row's root (the forest is final: read only) into an array of its own, and the flag
//                          "is its own root".
//   dbscan_rank_kernel     one workgroup per cloud: the exclusive scan of the flags in index order (se3_block_scan): a root's cluster
//                          number; the total is num_clusters.
//   dbscan_label_kernel    one thread per row: db_label_row.
#include <math.h>

#include <vector>

#include "common.h"
#include "dbscan_core.h"

namespace {

constexpr int kDbThreads = 256;
constexpr int kDbScanThreads = 1024;
constexpr int64_t kDbMaxRows = 1ll << 31;

struct DbLayout {
  uint8_t* core;      // [n_total]
  int* parent;        // [n_total], cloud-local: the forest of dbscan_core.h
  int* rank;          // [n_total]: the flags, then their exclusive scan per cloud
};

size_t db_carve(int64_t n_total, char* base, DbLayout* L) {
  Se3Carver c(base);
  const size_t n = (size_t)(n_total > 0 ? n_total : 1);
  DbLayout l;
  l.core = c.take<uint8_t>(n);
  l.parent = c.take<int>(n);
  l.rank = c.take<int>(n);
  if (L) *L = l;
  return c.bytes();
}

__global__ __launch_bounds__(kDbThreads) void dbscan_core_kernel(PairGridView g, const void* __restrict__ q, int elem, PairRows rows,
                                                                 int64_t n_total, double eps, int64_t min_points, DbLayout L) {
  const int64_t i = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
  if (i >= n_total) return;
  const int p = pg_pair_of_row(rows, i);
  double qv[3];
  pg_load3(q, elem, i, qv);
  L.core[i] = db_is_core(g, p, qv, eps, min_points) ? 1 : 0;
  L.parent[i] = (int)(i - rows.start[p]);
}

__global__ __launch_bounds__(kDbThreads) void dbscan_link_kernel(PairGridView g, const void* __restrict__ q, int elem, PairRows rows,
                                                                 int64_t n_total, double eps, DbLayout L) {
  const int64_t i = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
  if (i >= n_total || !L.core[i]) return;
  const int p = pg_pair_of_row(rows, i);
  const uint8_t* core = L.core + rows.start[p];
  int* parent = L.parent + rows.start[p];
  double qv[3];
  pg_load3(q, elem, i, qv);
  db_link_row(
      g, p, qv, eps, (int)(i - rows.start[p]), [&](int j) { return core[j] != 0; },
      [&](int x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
      [&](int x, int v) { atomicMin(parent + x, v); }, [&](int a, int b) { return atomicCAS(parent + a, a, b); });
}

// (the forest is final: parent is read only here; the roots go to an array of their own)
__global__ __launch_bounds__(kDbThreads) void dbscan_flatten_kernel(PairRows rows, int64_t n_total, DbLayout L, int* __restrict__ root) {
  const int64_t i = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
  if (i >= n_total) return;
  const int p = pg_pair_of_row(rows, i);
  const int* parent = L.parent + rows.start[p];
  const int self = (int)(i - rows.start[p]);
  int x = self;
  if (L.core[i])
    while (parent[x] != x) x = parent[x];
  root[i] = x;
  L.rank[i] = L.core[i] && x == self ? 1 : 0;
}

__global__ __launch_bounds__(kDbScanThreads) void dbscan_rank_kernel(PairRows rows, DbLayout L, int64_t* __restrict__ num_clusters) {
  __shared__ int sh[kDbScanThreads];
  const int p = blockIdx.x;
  const int64_t s0 = rows.start[p], n = rows.start[p + 1] - s0;
  const int total = se3_block_scan<kSe3ScanExclusive, int, int64_t, kDbScanThreads>(L.rank + s0, n, sh);
  if (threadIdx.x == 0) num_clusters[p] = total;
}

__global__ __launch_bounds__(kDbThreads) void dbscan_label_kernel(PairGridView g, const void* __restrict__ q, int elem, PairRows rows,
                                                                  int64_t n_total, double eps, DbLayout L, const int* __restrict__ root,
                                                                  int* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * kDbThreads + threadIdx.x;
  if (i >= n_total) return;
  const int p = pg_pair_of_row(rows, i);
  const int64_t s0 = rows.start[p];
  double qv[3];
  pg_load3(q, elem, i, qv);
  labels[i] = db_label_row(
      g, p, qv, eps, (int)(i - s0), [&](int j) { return L.core[s0 + j] != 0; }, [&](int j) { return L.rank[s0 + root[s0 + j]]; });
}

}  // namespace

extern "C" size_t se3_dbscan_workspace_bytes(int64_t n_total) {
  if (n_total < 0) return 0;
  return db_carve(n_total, nullptr, nullptr) + se3_align256(sizeof(int) * (size_t)(n_total > 0 ? n_total : 1));
}

extern "C" int se3_dbscan_stack(const void* grid_workspace, size_t grid_workspace_bytes, int64_t ns_total, const void* points, int elem,
                                const int64_t* offsets_host, int num_clouds, double eps, int64_t min_points, int* out_labels,
                                int64_t* out_num_clusters, void* workspace, size_t workspace_bytes, void* stream) {
  SE3_REQUIRE(isfinite(eps) && eps > 0.0, SE3_ERR_INVALID_ARG, "dbscan_stack: eps %g is not a positive finite number", eps);
  SE3_REQUIRE(min_points >= 1, SE3_ERR_INVALID_ARG, "dbscan_stack: min_points %lld is not >= 1", (long long)min_points);
  PairGridCall c;
  if (const int rc = pg_grid_call("dbscan_stack", "clouds", points && out_labels && out_num_clusters && workspace, grid_workspace,
                                  grid_workspace_bytes, ns_total, elem, offsets_host, num_clouds, kDbMaxRows, &c))
    return rc;
  SE3_REQUIRE(c.n_total == ns_total, SE3_ERR_INVALID_ARG, "dbscan_stack: the grid holds %lld rows, the clouds %lld: build it over the clouds themselves",
              (long long)ns_total, (long long)c.n_total);
  SE3_REQUIRE(workspace_bytes >= se3_dbscan_workspace_bytes(c.n_total), SE3_ERR_WORKSPACE, "dbscan_stack: workspace of %zu bytes, %zu needed",
              workspace_bytes, se3_dbscan_workspace_bytes(c.n_total));
  if (num_clouds == 0) return SE3_OK;
  DbLayout L;
  int* root = (int*)((char*)workspace + db_carve(c.n_total, (char*)workspace, &L));
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)se3_cdiv(c.n_total, kDbThreads);
  const PairGridView g = c.G.view();
  if (c.n_total > 0) {
    dbscan_core_kernel<<<blocks, kDbThreads, 0, st>>>(g, points, elem, c.rows, c.n_total, eps, min_points, L);
    dbscan_link_kernel<<<blocks, kDbThreads, 0, st>>>(g, points, elem, c.rows, c.n_total, eps, L);
    dbscan_flatten_kernel<<<blocks, kDbThreads, 0, st>>>(c.rows, c.n_total, L, root);
  }
  dbscan_rank_kernel<<<(unsigned)num_clouds, kDbScanThreads, 0, st>>>(c.rows, L, out_num_clusters);
  if (c.n_total > 0) dbscan_label_kernel<<<blocks, kDbThreads, 0, st>>>(g, points, elem, c.rows, c.n_total, eps, L, root, out_labels);
  SE3_CHECK_LAUNCH("dbscan_stack");
  return SE3_OK;
}

// ---- the same text on host memory, one cloud, no GPU (tests/test_segmentation_cpu.py) ---------------------------------------------------------
extern "C" int se3_debug_dbscan_host(const void* points, int64_t n, int elem, double eps, int64_t min_points, int* out_labels,
                                     int64_t* out_num_clusters) {
  SE3_REQUIRE(points && out_labels && out_num_clusters, SE3_ERR_INVALID_ARG, "debug_dbscan_host: null pointer");
  SE3_REQUIRE(n >= 0 && n < kDbMaxRows && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG, "debug_dbscan_host: n %lld, elem %d", (long long)n, elem);
  SE3_REQUIRE(isfinite(eps) && eps > 0.0, SE3_ERR_INVALID_ARG, "debug_dbscan_host: eps %g is not a positive finite number", eps);
  SE3_REQUIRE(min_points >= 1, SE3_ERR_INVALID_ARG, "debug_dbscan_host: min_points %lld is not >= 1", (long long)min_points);
  PairHostGrid H(points, n, elem, nullptr, eps);
  const PairGridView g = H.G.view();
  std::vector<uint8_t> core((size_t)n);
  std::vector<int> parent((size_t)n), rank((size_t)n);
  double qv[3];
  for (int64_t i = 0; i < n; i++) {
    pg_load3(points, elem, i, qv);
    core[i] = db_is_core(g, 0, qv, eps, min_points) ? 1 : 0;
    parent[i] = (int)i;
  }
  for (int64_t i = 0; i < n; i++) {
    if (!core[i]) continue;
    pg_load3(points, elem, i, qv);
    db_link_row(
        g, 0, qv, eps, (int)i, [&](int j) { return core[j] != 0; }, [&](int x) { return parent[x]; },
        [&](int x, int v) { if (v < parent[x]) parent[x] = v; },
        [&](int a, int b) {
          const int old = parent[a];
          if (old == a) parent[a] = b;
          return old;
        });
  }
  int run = 0;
  for (int64_t i = 0; i < n; i++) {
    int x = (int)i;
    if (core[i])
      while (parent[x] != x) x = parent[x];
    rank[i] = run;
    run += core[i] && x == (int)i ? 1 : 0;
  }
  for (int64_t i = 0; i < n; i++) {                           // (after the ranks: a root's parent word is its own index, so the walk is still valid)
    int x = (int)i;
    if (core[i])
      while (parent[x] != x) x = parent[x];
    parent[i] = x;
  }
  *out_num_clusters = run;
  for (int64_t i = 0; i < n; i++) {
    pg_load3(points, elem, i, qv);
    out_labels[i] = db_label_row(
        g, 0, qv, eps, (int)i, [&](int j) { return core[j] != 0; }, [&](int j) { return rank[parent[j]]; });
  }
  return SE3_OK;
}
