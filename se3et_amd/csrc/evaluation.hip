// Registration evaluation for B stacked pairs (the reference's Evaluator, experiments/se3ete.3dmatch/loss.py:198-262 and
// experiments/se3eti.kitti/loss.py:94-151, fed by get_node_correspondences, geotransformer/modules/registration/matching.py:230-315).
//
//   se3_gt_node_overlaps_stack      ground-truth patch overlaps of every (ref node, src node) pair of every registration pair, dense, and
//                                   their compacted (C, 2) / (C,) lists in torch.nonzero's row-major order.  Three launches:
//                                     node_records_kernel   per node: position (src nodes under the pair's ground-truth transform) and
//                                                           patch radius = max norm of its masked knn points about it;
//                                     overlap_rows_kernel   one workgroup per ref node (4 waves): a lane per src node runs the enclosing-
//                                                           sphere prefilter, the wave then takes its candidates one by one -- a lane holds
//                                                           one ref patch point (two with K = 128), the src patch point of step j is read
//                                                           from its holder lane (v_readlane: a wave-uniform broadcast, no LDS traffic and
//                                                           no barrier), ref coverage is a per-lane flag, src coverage one ballot per step;
//                                                           writes the dense row and the row's count of overlap > 0;
//                                     compact_kernel        per pair: exclusive scan of the row counts, then every row's nonzero entries in
//                                                           column order (ballot + popcount of the lower lanes).
//   se3_registration_metrics_stack  PIR, IR, RRE, RTE, RMSE, RR of B pairs: one workgroup per pair, integer counts and a fixed-order f64 sum,
//                                   so a pair's row does not depend on the batch it shares.
//
// Arithmetic follows the reference's float32 expressions: squared distances (|x|^2 - 2 x.y) + |y|^2 clamped at 0 (common.h), the rigid
// transform as matmul(p, R^T) + t with the K = 3 products accumulated in ascending k, divisions and square roots correctly rounded.
// SE3_EXACT_FP (build.py: -ffp-contract=off) and SE3_NO_SLP_VECTORIZE (no packed-f32 arithmetic, tests/test_isa_hazard.py).
#define SE3_EXACT_FP 1
#include "common.h"

namespace {

constexpr int kMaxPairs = SE3_MAX_BATCH / 2;
constexpr int kWaves = 4;

struct EvalPairs {
  int64_t node_off[SE3_MAX_BATCH + 1];   // first stacked node of cloud c (cloud 2p = ref of pair p, 2p + 1 = src)
  int64_t dense_off[kMaxPairs + 1];      // first entry of pair p's (N_p, M_p) block in the dense overlaps (= its list capacity)
  int64_t row_off[kMaxPairs + 1];        // first global ref row of pair p (sum of N_q, q < p)
};

__device__ __forceinline__ void apply_rigid(const float* __restrict__ T, float x, float y, float z, float& ox, float& oy, float& oz) {
  // torch.matmul(points, R^T) + t: out_i = (x R_i0 (+) y R_i1 (+) z R_i2) + t_i, the k-sum fused in ascending order as the K = 3 GEMM
  ox = __builtin_fmaf(z, T[2], __builtin_fmaf(y, T[1], x * T[0])) + T[3];
  oy = __builtin_fmaf(z, T[6], __builtin_fmaf(y, T[5], x * T[4])) + T[7];
  oz = __builtin_fmaf(z, T[10], __builtin_fmaf(y, T[9], x * T[8])) + T[11];
}

__device__ __forceinline__ float norm3(float x, float y, float z) { return se3_exact_sqrt(se3_ref_sq_norm(x, y, z)); }

__device__ __forceinline__ int pair_of_row(const EvalPairs& P, int B, int64_t row) {
  int p = 0;
  while (p + 1 < B && row >= P.row_off[p + 1]) p++;
  return p;
}

// per node: (x, y, z, patch radius); src nodes and their patch points under the pair's ground-truth transform
__global__ __launch_bounds__(256) void node_records_kernel(const float* __restrict__ points_f, const float* __restrict__ points_c,
                                                           const int64_t* __restrict__ knn, const uint8_t* __restrict__ knn_masks,
                                                           const float* __restrict__ transforms, EvalPairs P, int num_clouds, int K,
                                                           float4* __restrict__ records) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= P.node_off[num_clouds]) return;
  int c = 0;
  while (c + 1 < num_clouds && n >= P.node_off[c + 1]) c++;
  const float* T = transforms + (c >> 1) * 16;
  const bool src = c & 1;
  float nx = points_c[3 * n], ny = points_c[3 * n + 1], nz = points_c[3 * n + 2];
  if (src) apply_rigid(T, nx, ny, nz, nx, ny, nz);
  float r = 0.f;
  for (int k = 0; k < K; k++) {
    if (!knn_masks[n * K + k]) continue;                         // masked entries count as 0 (masked_fill before the max)
    const int64_t i = knn[n * K + k];
    float x = points_f[3 * i], y = points_f[3 * i + 1], z = points_f[3 * i + 2];
    if (src) apply_rigid(T, x, y, z, x, y, z);
    r = fmaxf(r, norm3(x - nx, y - ny, z - nz));
  }
  records[n] = make_float4(nx, ny, nz, r);
}

template <int S>   // S = K / 64 patch points per lane
__global__ __launch_bounds__(256) void overlap_rows_kernel(const float* __restrict__ points_f, const float* __restrict__ points_c,
                                                           const int64_t* __restrict__ knn, const uint8_t* __restrict__ knn_masks,
                                                           const uint8_t* __restrict__ node_masks, const float* __restrict__ transforms,
                                                           const float4* __restrict__ records, EvalPairs P, int B, float pos_radius,
                                                           float pos_radius_sq, float* __restrict__ overlaps, int32_t* __restrict__ row_counts) {
  constexpr int K = 64 * S;
  __shared__ int wave_counts[kWaves];
  const int64_t row = blockIdx.x;
  const int p = pair_of_row(P, B, row);
  const int64_t r_local = row - P.row_off[p];
  const int64_t rn = P.node_off[2 * p] + r_local;                     // global ref node
  const int64_t sb = P.node_off[2 * p + 1];                           // first global src node
  const int64_t M = P.node_off[2 * p + 2] - sb;
  const float* T = transforms + p * 16;
  float* out_row = overlaps + P.dense_off[p] + r_local * M;
  const int lane = se3_lane(), wave = threadIdx.x / SE3_WAVE;

  // the ref patch: point lane + 64 s of node rn on this lane
  float px[S], py[S], pz[S], p2[S];
  bool pm[S];
  int n_ref = 0;
#pragma unroll
  for (int s = 0; s < S; s++) {
    const int k = lane + 64 * s;
    pm[s] = knn_masks[rn * K + k] != 0;
    px[s] = py[s] = pz[s] = p2[s] = 0.f;
    if (pm[s]) {
      const int64_t i = knn[rn * K + k];
      px[s] = points_f[3 * i], py[s] = points_f[3 * i + 1], pz[s] = points_f[3 * i + 2];
      p2[s] = se3_ref_sq_norm(px[s], py[s], pz[s]);
    }
    n_ref += __popcll(__ballot(pm[s]));
  }
  const float4 rrec = records[rn];
  const float rx = points_c[3 * rn], ry = points_c[3 * rn + 1], rz = points_c[3 * rn + 2];
  const float r2 = se3_ref_sq_norm(rx, ry, rz);
  const bool ref_on = node_masks[rn] != 0;

  int count = 0;
  for (int64_t s0 = (int64_t)wave * SE3_WAVE; s0 < M; s0 += kWaves * SE3_WAVE) {
    const int64_t s = s0 + lane;
    bool cand = false;
    if (s < M && ref_on && node_masks[sb + s]) {
      const float4 q = records[sb + s];
      const float d = se3_exact_sqrt(se3_ref_sq_dist(rx, ry, rz, r2, q.x, q.y, q.z, se3_ref_sq_norm(q.x, q.y, q.z)));
      cand = ((rrec.w + q.w) + pos_radius) - d > 0.f;               // enclosing spheres (grown by pos_radius) intersect
    }
    if (s < M && !cand) out_row[s] = 0.f;
    unsigned long long cmask = __ballot(cand);
    while (cmask) {
      const int j0 = __ffsll((long long)cmask) - 1;
      cmask &= cmask - 1;
      const int64_t sn = sb + s0 + j0;
      // the src patch under the transform, point lane + 64 s on this lane
      float qx[S], qy[S], qz[S], q2[S];
      unsigned long long qm[S];
      int n_src = 0;
#pragma unroll
      for (int t = 0; t < S; t++) {
        const int k = lane + 64 * t;
        const bool m = knn_masks[sn * K + k] != 0;
        qx[t] = qy[t] = qz[t] = q2[t] = 0.f;
        if (m) {
          const int64_t i = knn[sn * K + k];
          apply_rigid(T, points_f[3 * i], points_f[3 * i + 1], points_f[3 * i + 2], qx[t], qy[t], qz[t]);
          q2[t] = se3_ref_sq_norm(qx[t], qy[t], qz[t]);
        }
        qm[t] = __ballot(m);
        n_src += __popcll(qm[t]);
      }
      bool ref_cov[S];
#pragma unroll
      for (int s2 = 0; s2 < S; s2++) ref_cov[s2] = false;
      int src_cov = 0;
#pragma unroll
      for (int t = 0; t < S; t++) {
        unsigned long long live = qm[t];
        while (live) {                                                 // masked src points never match (the reference's 1e12 fill)
          const int j = __ffsll((long long)live) - 1;
          live &= live - 1;
          const float bx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qx[t]), j));
          const float by = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qy[t]), j));
          const float bz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qz[t]), j));
          const float b2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q2[t]), j));
          bool any = false;
#pragma unroll
          for (int s2 = 0; s2 < S; s2++) {
            const bool close = pm[s2] && se3_ref_sq_dist(px[s2], py[s2], pz[s2], p2[s2], bx, by, bz, b2) < pos_radius_sq;
            ref_cov[s2] |= close;
            any |= close;
          }
          src_cov += __ballot(any) != 0ull;
        }
      }
      int ref_covered = 0;
#pragma unroll
      for (int s2 = 0; s2 < S; s2++) ref_covered += __popcll(__ballot(ref_cov[s2]));
      // (count / masked count) per side in float32, then (ref + src) / 2 -- the reference's order
      const float ov = (se3_exact_div((float)ref_covered, (float)n_ref) + se3_exact_div((float)src_cov, (float)n_src)) / 2.f;
      if (lane == 0) out_row[s0 + j0] = ov;
      count += ov > 0.f;
    }
  }
  if (lane == 0) wave_counts[wave] = count;
  __syncthreads();
  if (threadIdx.x == 0) row_counts[row] = wave_counts[0] + wave_counts[1] + wave_counts[2] + wave_counts[3];
}

// per pair: row starts by an exclusive scan of the row counts (wave 0, 64 rows per step), then the nonzero entries of every row in column
// order; pair p's lists start at dense_off[p] (capacity N_p M_p), their length goes to pair_counts[p]
__global__ __launch_bounds__(256) void compact_kernel(const float* __restrict__ overlaps, const int32_t* __restrict__ row_counts, EvalPairs P,
                                                      int64_t* __restrict__ row_starts, int64_t* __restrict__ corr_indices,
                                                      float* __restrict__ corr_overlaps, int64_t* __restrict__ pair_counts) {
  const int p = blockIdx.x;
  const int64_t r0 = P.row_off[p], N = P.row_off[p + 1] - r0;
  const int64_t M = P.node_off[2 * p + 2] - P.node_off[2 * p + 1];
  const int lane = se3_lane(), wave = threadIdx.x / SE3_WAVE;
  if (wave == 0) {
    int64_t carry = 0;
    for (int64_t b = 0; b < N; b += SE3_WAVE) {
      const int64_t v = b + lane < N ? row_counts[r0 + b + lane] : 0;
      int64_t inc = v;
#pragma unroll
      for (int o = 1; o < SE3_WAVE; o <<= 1) {
        const int64_t u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
      }
      if (b + lane < N) row_starts[r0 + b + lane] = carry + inc - v;
      carry += __shfl(inc, SE3_WAVE - 1);
    }
    if (lane == 0) pair_counts[p] = carry;
  }
  __syncthreads();
  const float* dense = overlaps + P.dense_off[p];
  const int64_t base = P.dense_off[p];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t r = wave; r < N; r += kWaves) {
    int64_t pos = base + row_starts[r0 + r];
    for (int64_t b = 0; b < M; b += SE3_WAVE) {
      const int64_t s = b + lane;
      const float v = s < M ? dense[r * M + s] : 0.f;
      const unsigned long long m = __ballot(v > 0.f);
      if (v > 0.f) {
        const int64_t at = pos + __popcll(m & below);
        corr_indices[2 * at] = r;
        corr_indices[2 * at + 1] = s;
        corr_overlaps[at] = v;
      }
      pos += __popcll(m);
    }
  }
}

// one row of the per-pair table of se3_registration_metrics_stack (include/se3et_hip.h)
enum { kDense, kRows, kCols, kRefNode, kSrcNode, kNumPred, kRefCorr, kSrcCorr, kNumCorr, kEst, kGt, kSrcPts, kNumSrcPts, kTableWidth = 16 };

template <typename T>
__device__ __forceinline__ T block_sum(T v, T* scratch) {            // fixed order: wave trees, then the four wave sums in wave order
  v = se3_wave_sum(v);
  const int wave = threadIdx.x / SE3_WAVE;
  __syncthreads();
  if (se3_lane() == 0) scratch[wave] = v;
  __syncthreads();
  return ((scratch[0] + scratch[1]) + scratch[2]) + scratch[3];
}

__global__ __launch_bounds__(256) void metrics_kernel(const int64_t* __restrict__ table, float acceptance_overlap, float acceptance_radius,
                                                      float rmse_threshold, float rre_threshold, float rte_threshold, int kitti,
                                                      float* __restrict__ rows) {
  __shared__ long long iscratch[kWaves];
  __shared__ double dscratch[kWaves];
  const int64_t* row = table + blockIdx.x * kTableWidth;
  const float* dense = (const float*)row[kDense];
  const int64_t N = row[kRows], M = row[kCols];
  const float* Te = (const float*)row[kEst];
  const float* Tg = (const float*)row[kGt];
  const float nan = __int_as_float(0x7fc00000);

  // PIR: predicted node pairs whose ground-truth overlap exceeds acceptance_overlap (absent pairs have overlap 0); an index outside the
  // pair's nodes makes the row's PIR NaN instead of reading outside the block
  const int64_t* ri = (const int64_t*)row[kRefNode];
  const int64_t* si = (const int64_t*)row[kSrcNode];
  const int64_t n_pred = row[kNumPred];
  long long hit = 0, bad = 0;
  for (int64_t i = threadIdx.x; i < n_pred; i += blockDim.x) {
    const int64_t r = ri[i], s = si[i];
    if (r < 0 || r >= N || s < 0 || s >= M) {
      bad++;
      continue;
    }
    const float v = dense[r * M + s];
    hit += v > 0.f && v > acceptance_overlap;
  }
  hit = block_sum(hit, iscratch);
  bad = block_sum(bad, iscratch);

  // IR: correspondences with |ref - T_gt src| < acceptance_radius
  const float* rc = (const float*)row[kRefCorr];
  const float* sc = (const float*)row[kSrcCorr];
  const int64_t n_corr = row[kNumCorr];
  long long inl = 0;
  for (int64_t i = threadIdx.x; i < n_corr; i += blockDim.x) {
    float x, y, z;
    apply_rigid(Tg, sc[3 * i], sc[3 * i + 1], sc[3 * i + 2], x, y, z);
    inl += norm3(rc[3 * i] - x, rc[3 * i + 1] - y, rc[3 * i + 2] - z) < acceptance_radius;
  }
  inl = block_sum(inl, iscratch);

  // RMSE (3DMatch): mean over the stage-0 src points of |A p - p|, A = T_gt^-1 T_est (rigid inverse: R^T, -R^T t)
  double dist_sum = 0.0;
  const int64_t n_pts = row[kNumSrcPts];
  float A[12];
  {
    float Ri[9], ti[3];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) Ri[3 * i + j] = Tg[4 * j + i];
    for (int i = 0; i < 3; i++) ti[i] = -__builtin_fmaf(Ri[3 * i + 2], Tg[11], __builtin_fmaf(Ri[3 * i + 1], Tg[7], Ri[3 * i] * Tg[3]));
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 4; j++)
        A[4 * i + j] = __builtin_fmaf(Ri[3 * i + 2], Te[8 + j], __builtin_fmaf(Ri[3 * i + 1], Te[4 + j], Ri[3 * i] * Te[j]));
      A[4 * i + 3] += ti[i];
    }
  }
  if (!kitti) {
    const float* sp = (const float*)row[kSrcPts];
    for (int64_t i = threadIdx.x; i < n_pts; i += blockDim.x) {
      float x, y, z;
      const float px = sp[3 * i], py = sp[3 * i + 1], pz = sp[3 * i + 2];
      apply_rigid(A, px, py, pz, x, y, z);
      dist_sum += (double)norm3(x - px, y - py, z - pz);
    }
    dist_sum = block_sum(dist_sum, dscratch);
  }

  if (threadIdx.x != 0) return;
  // RRE = acos(clamp((tr(R_est^T R_gt) - 1) / 2, -1, 1)) in degrees; RTE = |t_gt - t_est|
  float tr = 0.f;
  for (int d = 0; d < 3; d++) {
    const float m = __builtin_fmaf(Te[8 + d], Tg[8 + d], __builtin_fmaf(Te[4 + d], Tg[4 + d], Te[d] * Tg[d]));
    tr = d == 0 ? m : tr + m;
  }
  const float x = fminf(fmaxf(0.5f * (tr - 1.f), -1.f), 1.f);
  const float rre = se3_exact_div(180.f * acosf(x), 3.14159265358979323846f);
  const float rte = norm3(Tg[3] - Te[3], Tg[7] - Te[7], Tg[11] - Te[11]);
  const float rmse = kitti ? nan : (n_pts > 0 ? (float)(dist_sum / (double)n_pts) : nan);
  float* out = rows + blockIdx.x * 6;
  out[0] = bad ? nan : (n_pred > 0 ? se3_exact_div((float)hit, (float)n_pred) : nan);
  out[1] = n_corr > 0 ? se3_exact_div((float)inl, (float)n_corr) : nan;
  out[2] = rre;
  out[3] = rte;
  out[4] = rmse;
  out[5] = (kitti ? (rre < rre_threshold && rte < rte_threshold) : (rmse < rmse_threshold)) ? 1.f : 0.f;
}

}  // namespace

extern "C" int se3_gt_node_overlaps_stack(const float* points_f, const float* points_c, const int64_t* node_lengths, int num_clouds,
                                          const int64_t* knn, const uint8_t* knn_masks, const uint8_t* node_masks, int K,
                                          const float* transforms, float pos_radius, float pos_radius_sq, void* workspace,
                                          float* overlaps, int64_t* corr_indices, float* corr_overlaps, int64_t* pair_counts, void* stream) {
  SE3_REQUIRE(points_f && points_c && node_lengths && knn && knn_masks && node_masks && transforms && workspace && overlaps && corr_indices &&
              corr_overlaps && pair_counts, SE3_ERR_INVALID_ARG, "gt_node_overlaps_stack: null pointer");
  SE3_REQUIRE(num_clouds >= 2 && num_clouds % 2 == 0 && num_clouds <= SE3_MAX_BATCH, SE3_ERR_UNSUPPORTED,
              "gt_node_overlaps_stack: %d clouds (an even number, at most %d)", num_clouds, SE3_MAX_BATCH);
  SE3_REQUIRE(K == 64 || K == 128, SE3_ERR_UNSUPPORTED, "gt_node_overlaps_stack: K = %d (64 or 128)", K);
  EvalPairs P;
  const int B = num_clouds / 2;
  P.node_off[0] = 0;
  for (int c = 0; c < num_clouds; c++) {
    SE3_REQUIRE(node_lengths[c] >= 0, SE3_ERR_INVALID_ARG, "gt_node_overlaps_stack: negative length");
    P.node_off[c + 1] = P.node_off[c] + node_lengths[c];
  }
  P.dense_off[0] = P.row_off[0] = 0;
  for (int p = 0; p < B; p++) {
    P.dense_off[p + 1] = P.dense_off[p] + node_lengths[2 * p] * node_lengths[2 * p + 1];
    P.row_off[p + 1] = P.row_off[p] + node_lengths[2 * p];
  }
  const int64_t nodes = P.node_off[num_clouds], rows = P.row_off[B];
  SE3_REQUIRE(rows < 2147483647, SE3_ERR_UNSUPPORTED, "gt_node_overlaps_stack: too many ref nodes");
  // workspace = se3_gt_node_overlaps_workspace_bytes(total nodes): records, row counts, row starts
  float4* records = (float4*)workspace;
  int64_t* row_starts = (int64_t*)(records + nodes);
  int32_t* row_counts = (int32_t*)(row_starts + nodes);
  hipStream_t st = (hipStream_t)stream;
  if (nodes > 0)
    node_records_kernel<<<(unsigned)se3_cdiv(nodes, 256), 256, 0, st>>>(points_f, points_c, knn, knn_masks, transforms, P, num_clouds, K, records);
  if (rows > 0) {
    if (K == 64)
      overlap_rows_kernel<1><<<(unsigned)rows, 256, 0, st>>>(points_f, points_c, knn, knn_masks, node_masks, transforms, records, P, B,
                                                             pos_radius, pos_radius_sq, overlaps, row_counts);
    else
      overlap_rows_kernel<2><<<(unsigned)rows, 256, 0, st>>>(points_f, points_c, knn, knn_masks, node_masks, transforms, records, P, B,
                                                             pos_radius, pos_radius_sq, overlaps, row_counts);
  }
  compact_kernel<<<(unsigned)B, 256, 0, st>>>(overlaps, row_counts, P, row_starts, corr_indices, corr_overlaps, pair_counts);
  SE3_CHECK_LAUNCH("gt_node_overlaps_stack");
  return SE3_OK;
}

extern "C" size_t se3_gt_node_overlaps_workspace_bytes(int64_t total_nodes) {
  return (size_t)(total_nodes > 0 ? total_nodes : 0) * (sizeof(float4) + sizeof(int64_t) + sizeof(int32_t));
}

extern "C" int se3_registration_metrics_stack(const int64_t* pair_table, int num_pairs, float acceptance_overlap, float acceptance_radius,
                                              float rmse_threshold, float rre_threshold, float rte_threshold, int kitti, float* rows,
                                              void* stream) {
  SE3_REQUIRE(pair_table && rows, SE3_ERR_INVALID_ARG, "registration_metrics_stack: null pointer");
  SE3_REQUIRE(num_pairs >= 0 && num_pairs <= 65535, SE3_ERR_UNSUPPORTED, "registration_metrics_stack: %d pairs", num_pairs);
  if (num_pairs == 0) return SE3_OK;
  metrics_kernel<<<(unsigned)num_pairs, 256, 0, (hipStream_t)stream>>>(pair_table, acceptance_overlap, acceptance_radius, rmse_threshold,
                                                                       rre_threshold, rte_threshold, kitti, rows);
  SE3_CHECK_LAUNCH("registration_metrics_stack");
  return SE3_OK;
}
