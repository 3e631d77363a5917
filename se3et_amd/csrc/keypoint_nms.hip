// Keypoint selection for stacked clouds: greedy radius non-maximum suppression in score order, the loop of the reference's
// sample_keypoints_with_nms / random_sample_keypoints_with_nms (geotransformer/utils/pointcloud.py:191-248), for up to SE3_PAIR_MAX_PAIRS
// clouds per call on the grid of csrc/pair_grid.h.  se3et_amd/keypoints.py carries the same contract.
// (SE3_EXACT_FP: the file is built with contraction off, and pg_dist2 fences itself as well.)
//
//   keypoint_rank_kernel     one thread per stacked row: rank[order[r]] = r, the inverse of the caller's order (entries outside the cloud
//                            are not written; the selection finds them).
//   keypoint_nms_kernel      one workgroup of 256 threads per cloud: the checks, then kp_tile_step for every tile of 256 ranks.
//   A call enqueues the two after the grid build (se3_pair_grid_build over the clouds themselves, identity transforms, cell_hint = radius);
//   nothing waits on the host.
//
// Contract.
//   Rank.  The total order is score descending, then cloud-local index ascending: equal scores keep the lower index first, -0.0 equals
//     0.0, infinities order as numbers, a NaN score refuses the cloud (the reference's np.argsort(scores)[::-1] leaves ties unspecified;
//     the rule is the project's, as in ransac.select_correspondences).  Ranking is the Python layer's: this file takes `order`, cloud-local
//     rank -> index, and refuses a cloud whose order is not a permutation of its rows (status bit 2).
//   Suppression.  In rank order a point is kept iff no already kept point lies at d^2 < r^2, d^2 = (dx dx + dy dy) + dz dz in float64,
//     unfused; float32 points are promoted on load; r^2 = r r in float64.  The test is strict: a pair at exactly r does not suppress, a
//     duplicate of a kept point does.
//   Output.  The kept points' cloud-local indices in rank order, int64.  With max_keep = K > 0 the first K of that list (the reference's
//     early break), fewer if fewer survive; K <= 0: the whole list.  n = 0 gives an empty list.
//   Refusals.  A non-finite point sets status bit 1; the cloud gives no rows and its count is MINUS its bits; the other clouds of the call
//     are unaffected.  radius must be positive and finite.
//   Determinism.  No atomics in the selection (the one integer atomicOr raises the call's status word for a refused cloud).  A tile's
//     outcome is a function of the cloud's points and order alone: a cloud's list is identical alone, anywhere in a batch, from run to
//     run, and between the device and se3_debug_keypoint_nms_host.
//
// The exact parallel form (kp_tile_step).  The ranks are walked in tiles of 256.  Thread t of the tile at rank a owns rank a + t and runs
// pg_ball_walk once for its point; for every hit j it looks up rank[j]:
//     rank[j] <  a            an earlier tile's point: if its kept byte is set, the thread's point is suppressed from outside;
//     rank[j] in [a, a + t)   bit rank[j] - a of the thread's own 256-bit row (8 KB of LDS for the tile; each thread writes its own row);
//     otherwise               a lower-ranked point (or the point itself): ignored.
//   After a barrier thread 0 resolves the tile in rank order, 256 dependent steps on four 64-bit words: rank i is kept iff it was not
//   suppressed from outside and (row[i] & kept_mask) == 0; the resolve ends at K.  The kept flags get their places from the shared block
//   scan, the kept indices are appended to the cloud's output segment and every rank's kept byte is written; a workgroup fence and barrier
//   order those writes before the next tile's reads.  The dependency depth is the tile count whatever the input: no fixed-point iteration,
//   no host loop, no captured graph, no cooperative launch.
//   Cost.  A radius far above the point spacing makes every walk long; in the extreme one ball holds the cloud and the walks are quadratic
//   on one workgroup: correct, slow.  One workgroup per cloud leaves most of the device idle for a single large cloud.
#include <math.h>

#include <vector>

#include "common.h"
#include "pair_grid.h"

namespace {

constexpr int kKpTile = 256;            // ranks per tile = threads per workgroup
constexpr int kKpNonFinite = 1;         // status bits
constexpr int kKpBadOrder = 2;

// one cloud of a call
struct KpCloud {
  const double* pts;            // (n, 3): the grid's `moved`, i.e. the points promoted to float64, in input order
  const int64_t* order;         // rank -> index
  int* rank;                    // index -> rank
  unsigned char* kept;          // per rank: 1 once kept, 0 once decided otherwise (written tile by tile)
  int64_t* out;
  int64_t n;
};

// the LDS of a tile (host: a plain struct)
struct KpTileShared {
  unsigned long long rows[kKpTile][4];
  unsigned long long mask[4];
  unsigned char outside[kKpTile];
  int nonfinite, bad_order;
};

// 0, or the bits that refuse the cloud.  Lanes [lane_begin, lane_end) of 256 take rows lane, lane + 256, ..
template <class Sync>
PG_HD int kp_cloud_check(const KpCloud& c, int lane_begin, int lane_end, KpTileShared* sh, Sync&& sync) {
  if (lane_begin == 0) sh->nonfinite = 0, sh->bad_order = 0;
  sync();
  for (int l = lane_begin; l < lane_end; l++)
    for (int64_t j = l; j < c.n; j += kKpTile) {
      if (!(fabs(c.pts[3 * j]) < INFINITY) || !(fabs(c.pts[3 * j + 1]) < INFINITY) || !(fabs(c.pts[3 * j + 2]) < INFINITY)) sh->nonfinite = 1;
      const int rk = c.rank[j];                                          // (every writer stores the same 1)
      if (rk < 0 || rk >= c.n || c.order[rk] != j) sh->bad_order = 1;    // order is onto, hence a permutation
    }
  sync();
  return (sh->nonfinite ? kKpNonFinite : 0) | (sh->bad_order ? kKpBadOrder : 0);
}

// One tile: ranks [a, a + 256) of cloud p, `kept_before` points kept by the earlier tiles, at most `room` more to keep (room >= 1).
// Returns the number kept in this tile, the same in every lane.  scan(lane, flag): the number of set flags in the lanes below, called
// once for every lane of the tile, in ascending lane order by a serial caller.
template <class Sync, class Scan>
PG_HD int kp_tile_step(const KpCloud& c, const PairGridView& g, int p, int64_t a, int64_t kept_before, int64_t room, double r, double r2,
                       int lane_begin, int lane_end, KpTileShared* sh, Sync&& sync, Scan&& scan) {
  const int m = c.n - a < kKpTile ? (int)(c.n - a) : kKpTile;
  // the walk and its three-way hit rule
  for (int t = lane_begin; t < lane_end; t++) {
    unsigned long long row[4] = {0, 0, 0, 0};
    bool outside = false;
    if (t < m) {
      const double* q = c.pts + 3 * c.order[a + t];
      pg_ball_walk(g, p, q, r, r2, [&](int j) {
        if (outside) return;
        const int64_t rk = c.rank[j];
        if (rk < a) {
          if (c.kept[rk]) outside = true;
        } else if (rk < a + t) {
          const int b = (int)(rk - a);
          for (int w = 0; w < 4; w++) row[w] |= (b >> 6) == w ? 1ull << (b & 63) : 0ull;
        }
      });
    }
    for (int w = 0; w < 4; w++) sh->rows[t][w] = row[w];
    sh->outside[t] = outside ? 1 : 0;
  }
  sync();
  // the resolve, in rank order
  if (lane_begin == 0) {
    unsigned long long k0 = 0, k1 = 0, k2 = 0, k3 = 0;
    int64_t kept = 0;
    for (int i = 0; i < m && kept < room; i++) {
      const unsigned long long* row = sh->rows[i];
      if (sh->outside[i] || ((row[0] & k0) | (row[1] & k1) | (row[2] & k2) | (row[3] & k3)) != 0) continue;
      const unsigned long long bit = 1ull << (i & 63);
      const int w = i >> 6;
      k0 |= w == 0 ? bit : 0ull, k1 |= w == 1 ? bit : 0ull, k2 |= w == 2 ? bit : 0ull, k3 |= w == 3 ? bit : 0ull;
      kept++;
    }
    sh->mask[0] = k0, sh->mask[1] = k1, sh->mask[2] = k2, sh->mask[3] = k3;
  }
  sync();
  // the append
  int total = 0;
  for (int w = 0; w < 4; w++) total += __builtin_popcountll(sh->mask[w]);
  for (int t = lane_begin; t < lane_end; t++) {
    const int flag = (int)((sh->mask[t >> 6] >> (t & 63)) & 1ull);
    const int place = scan(t, flag);
    if (t < m) {
      c.kept[a + t] = (unsigned char)flag;
      if (flag) c.out[kept_before + place] = c.order[a + t];
    }
  }
  sync();                                                                // (the kept bytes are ordered before the next tile's walks)
  return total;
}

// what the kernels get: the stacked arrays of a call
struct KpCall {
  const double* pts;            // the grid's `moved`
  const int64_t* order;
  int* rank;
  unsigned char* kept;
  int64_t* out;
  PairRows rows;
};

PG_HD KpCloud kp_cloud_of(const KpCall& k, int p) {
  const int64_t s0 = k.rows.start[p];
  return KpCloud{k.pts + 3 * s0, k.order + s0, k.rank + s0, k.kept + s0, k.out + s0, k.rows.start[p + 1] - s0};
}

struct KpLayout {
  int* rank;
  unsigned char* kept;
};

size_t kp_carve(int64_t n_total, char* base, KpLayout* L) {
  Se3Carver c(base);
  KpLayout l;
  l.rank = c.take<int>((size_t)(n_total > 0 ? n_total : 1));
  l.kept = c.take<unsigned char>((size_t)(n_total > 0 ? n_total : 1));
  if (L) *L = l;
  return c.bytes();
}

__global__ __launch_bounds__(256) void keypoint_rank_kernel(KpCall k, int64_t n_total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_total) return;
  const int p = pg_pair_of_row(k.rows, i);
  const int64_t s0 = k.rows.start[p], n = k.rows.start[p + 1] - s0, j = k.order[i];
  if (j >= 0 && j < n) k.rank[s0 + j] = (int)(i - s0);
}

__global__ __launch_bounds__(kKpTile) void keypoint_nms_kernel(PairGridView g, KpCall k, double r, double r2, int max_keep,
                                                               int* __restrict__ out_counts, int* __restrict__ status) {
  __shared__ KpTileShared sh;
  __shared__ int scan_sh[kKpTile];
  const int p = blockIdx.x, t = threadIdx.x;
  const KpCloud c = kp_cloud_of(k, p);
  const auto sync = [] {
    __threadfence_block();
    __syncthreads();
  };
  const int flags = kp_cloud_check(c, t, t + 1, &sh, sync);
  if (flags) {                                                           // (uniform over the workgroup)
    if (t == 0) {
      out_counts[p] = -flags;
      atomicOr(status, flags);
    }
    return;
  }
  const int64_t limit = max_keep > 0 ? (int64_t)max_keep : c.n;
  int64_t kept = 0;
  for (int64_t a = 0; a < c.n && kept < limit; a += kKpTile)
    kept += kp_tile_step(c, g, p, a, kept, limit - kept, r, r2, t, t + 1, &sh, sync, [&](int, int flag) {
      int total;
      return se3_block_exclusive<int, kKpTile>(flag, scan_sh, &total);
    });
  if (t == 0) out_counts[p] = (int)kept;
}

}  // namespace

extern "C" size_t se3_keypoint_nms_workspace_bytes(int64_t n_total, int num_clouds) {
  if (n_total < 0 || n_total >= (1ll << 31) || num_clouds < 0 || num_clouds > kPairMaxPairs) return 0;
  return kp_carve(n_total, nullptr, nullptr);
}

extern "C" int se3_keypoint_nms_stack(const void* grid_workspace, size_t grid_workspace_bytes, int64_t n_total, const int64_t* order,
                                      const int64_t* offsets_host, int num_clouds, double radius, int max_keep, int64_t* out_indices,
                                      int* out_counts, int* status, void* workspace, size_t workspace_bytes, void* stream) {
  SE3_REQUIRE(grid_workspace && order && offsets_host && out_indices && out_counts && status && workspace, SE3_ERR_INVALID_ARG,
              "keypoint_nms_stack: null pointer");
  SE3_REQUIRE(num_clouds >= 0 && num_clouds <= kPairMaxPairs && n_total >= 0 && n_total < (1ll << 31), SE3_ERR_INVALID_ARG,
              "keypoint_nms_stack: %d clouds (at most %d), %lld rows (below 2^31)", num_clouds, kPairMaxPairs, (long long)n_total);
  SE3_REQUIRE(isfinite(radius) && radius > 0.0, SE3_ERR_INVALID_ARG, "keypoint_nms_stack: radius %g is not a positive finite number", radius);
  KpCall k;
  SE3_REQUIRE(pg_fill_rows(&k.rows, offsets_host, num_clouds) && k.rows.start[num_clouds] == n_total, SE3_ERR_INVALID_ARG,
              "keypoint_nms_stack: offsets must start at 0, not decrease and end at n_total = %lld", (long long)n_total);
  PairGridCall c;                 // (the count and the offsets are worded by this entry, above: the call adds the grid workspace's check)
  if (const int rc = pg_grid_call("keypoint_nms_stack", "clouds", true, grid_workspace, grid_workspace_bytes, n_total, 0, offsets_host, num_clouds,
                                  1ll << 31, &c))
    return rc;
  const PairGridLayout& G = c.G;
  KpLayout L;
  SE3_REQUIRE(kp_carve(n_total, (char*)workspace, &L) <= workspace_bytes, SE3_ERR_WORKSPACE,
              "keypoint_nms_stack: workspace of %zu bytes is too small", workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  SE3_REQUIRE(hipMemsetAsync(status, 0, sizeof(int), st) == hipSuccess, SE3_ERR_LAUNCH, "keypoint_nms_stack: memset failed");
  if (num_clouds == 0) return SE3_OK;
  k.pts = G.moved, k.order = order, k.rank = L.rank, k.kept = L.kept, k.out = out_indices;
  if (n_total > 0) keypoint_rank_kernel<<<(unsigned)se3_cdiv(n_total, 256), 256, 0, st>>>(k, n_total);
  keypoint_nms_kernel<<<(unsigned)num_clouds, kKpTile, 0, st>>>(G.view(), k, radius, radius * radius, max_keep, out_counts, status);
  SE3_CHECK_LAUNCH("keypoint_nms_stack");
  return SE3_OK;
}

// ---- the same text on host memory, one cloud, no GPU (tests/test_keypoints_cpu.py) ----------------------------------------------------------
// *status: 0, or the bits of the device status word (then *out_count = 0).  out_indices: n entries.
extern "C" int se3_debug_keypoint_nms_host(const void* points, int64_t n, int elem, const int64_t* order, double radius, int max_keep,
                                           int64_t* out_indices, int64_t* out_count, int* status) {
  SE3_REQUIRE(points && order && out_indices && out_count && status, SE3_ERR_INVALID_ARG, "debug_keypoint_nms_host: null pointer");
  SE3_REQUIRE(n >= 0 && n < (1ll << 31) && (elem == 0 || elem == 1), SE3_ERR_INVALID_ARG, "debug_keypoint_nms_host: n %lld, elem %d",
              (long long)n, elem);
  SE3_REQUIRE(isfinite(radius) && radius > 0.0, SE3_ERR_INVALID_ARG, "debug_keypoint_nms_host: radius %g is not a positive finite number", radius);
  *out_count = 0, *status = 0;
  PairHostGrid H(points, n, elem, nullptr, radius);
  const PairGridLayout& G = H.G;
  std::vector<int> rank((size_t)n + 1, -1);
  std::vector<unsigned char> kept((size_t)n + 1);
  for (int64_t i = 0; i < n; i++)
    if (order[i] >= 0 && order[i] < n) rank[(size_t)order[i]] = (int)i;
  const KpCloud c{G.moved, order, rank.data(), kept.data(), out_indices, n};
  const PairGridView g = G.view();
  std::vector<KpTileShared> sh(1);
  const auto sync = [] {};
  *status = kp_cloud_check(c, 0, kKpTile, sh.data(), sync);
  if (*status) return SE3_OK;
  const int64_t limit = max_keep > 0 ? (int64_t)max_keep : n;
  int64_t total = 0;
  for (int64_t a = 0; a < n && total < limit; a += kKpTile) {
    int run = 0;
    total += kp_tile_step(c, g, 0, a, total, limit - total, radius, radius * radius, 0, kKpTile, sh.data(), sync, [&](int, int flag) {
      const int before = run;
      run += flag;
      return before;
    });
  }
  *out_count = total;
  return SE3_OK;
}
