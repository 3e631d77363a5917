// RANSAC registration from correspondences for stacked pairs (the reference's registration_with_ransac_from_correspondences,
// geotransformer/utils/open3d.py:169-198: Open3D's registration_ransac_based_on_correspondence with TransformationEstimationPointToPoint(False),
// no checkers, RANSACConvergenceCriteria(num_iterations, num_iterations)).  Pair p uses the correspondences [offsets[p], offsets[p+1]) of the
// stacked src / ref arrays; n = their count, H = num_iterations hypotheses per pair.  The contract (restated from Open3D's
// pipelines/registration/Registration.cpp; se3et_amd/ransac.py carries the same text):
//   1. ransac_n < 3, n < ransac_n or distance_threshold <= 0: identity, fitness 0, RMSE 0.
//   2. Hypothesis h draws ransac_n pair-local indices uniformly with replacement:
//        idx_j = ((splitmix64(splitmix64(seed) + h * ransac_n + j) >> 32) * n) >> 32          (uint64 wrap-around)
//      splitmix64(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
//      return z ^ (z >> 31).  The stream depends on (seed, h, j, n) only, never on the pair's position in the batch.  (Or the indices come
//      from hypothesis_indices.)
//   3. Unweighted Kabsch in float64 (plain centroids, H = sum (s - s_)(r - r_)^T, reflection fixed), src -> ref; T rounded to float32.
//   4. i is an inlier iff |T s_i - r_i| < threshold, evaluated as d^2 < threshold^2 in float32 with d = R s + (t - r);
//      fitness = inliers / n, inlier_rmse = sqrt(sum_inliers d^2 / inliers) (0 without inliers).
//   5. Order: more inliers, then the smaller inlier error sum, then the lower h.  The initial best is the identity (fitness 0, RMSE 0),
//      so a hypothesis needs at least one inlier to win.
//   6. / 7. All H hypotheses are evaluated (no early exit); the winner's own fit is returned (no refit).
// Non-finite correspondences are never inliers; a hypothesis with a non-finite (or, given explicitly, out-of-range) sample has 0 inliers.
// Optional checkers (se3_ransac_correspondences_checked_stack; Open3D's CorrespondenceCheckerBasedOnEdgeLength / ...BasedOnDistance, which
// registration_with_ransac_from_feats of geotransformer/utils/open3d.py:133-166 passes).  A rejected hypothesis scores 0 inliers:
//   edge length   before the fit, over all pairs (a, b) of the sample, in float64: rejected if |s_a - s_b| < t |r_a - r_b| or
//                 |r_a - r_b| < t |s_a - s_b| (t = edge_length_similarity);
//   distance      after the fit: rejected if a sampled correspondence has d^2 > threshold^2 in the scoring arithmetic of 4.
// With both off the kernels are the instantiation without checker code: every output is bit-identical to the unchecked entry.
//
// Three launches, no host synchronisation:
//   ransac_fit_kernel     one thread per (pair, hypothesis): sample, float64 Kabsch (csrc/kabsch.h), 3x4 float32 transform to the workspace
//                         (NaN for an invalid hypothesis: it then scores 0 inliers).
//   ransac_score_kernel   one workgroup per (pair, 512 hypotheses): a lane holds two hypotheses' 3x4 transforms as packed pairs
//                         (v_pk_fma_f32), the pair's correspondences pass through LDS in chunks of 256 and are read at one address per
//                         wave (broadcast).  Counts are integers and each lane sums its hypotheses' d^2 serially in correspondence order:
//                         that is the fixed order that makes a pair's result independent of its batch and of the run.  Writes the
//                         workgroup's best candidate (and, on request, every hypothesis' count and error sum).
//   ransac_select_kernel  one wave per pair: the best of its workgroups' candidates under the total order of 5, then the outputs.
#include "common.h"
#include "kabsch.h"
#include "splitmix.h"          // splitmix64 and the draw of item 2, shared with csrc/fgr_core.h

namespace {

constexpr int kMaxSample = 16;
constexpr int kFitThreads = 128;
constexpr int kScoreThreads = 256;
constexpr int kTile = 2 * kScoreThreads;   // hypotheses per scoring workgroup (two per lane)
constexpr int kChunk = 256;                // correspondences per LDS stage

typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }   // v_pk_fma_f32

struct Candidate {                         // a workgroup's best hypothesis (count -1: none)
  int count;
  float err;
  int h;
  int pad;
};

// a beats b: more inliers, then the smaller error sum, then the lower hypothesis index
__device__ __forceinline__ bool beats(int ca, float ea, int ha, int cb, float eb, int hb) {
  return ca > cb || (ca == cb && (ea < eb || (ea == eb && ha < hb)));
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// CHECK: the optional checkers (edge_t > 0: edge length similarity; check_thr2 > 0: distance) and the `passed` flags (may be null)
template <bool CHECK>
__global__ __launch_bounds__(kFitThreads) void ransac_fit_kernel(const float* __restrict__ src, const float* __restrict__ ref,
                                                                 const int64_t* __restrict__ offsets, int H, int rn, uint64_t key,
                                                                 const int32_t* __restrict__ explicit_idx, int valid,
                                                                 float4* __restrict__ hyp, double edge_t, float check_thr2,
                                                                 uint8_t* __restrict__ passed) {
  const int p = blockIdx.y;
  const int h = blockIdx.x * kFitThreads + threadIdx.x;
  if (h >= H) return;
  const int64_t b0 = offsets[p], n = offsets[p + 1] - b0;
  float4* out = hyp + ((int64_t)p * H + h) * 3;
  bool ok = valid && n >= rn;
  // sample j of this hypothesis (recomputed in the second pass rather than held in a register array indexed at run time)
  auto index = [&](int j) -> int64_t {
    if (explicit_idx) return explicit_idx[((int64_t)p * H + h) * rn + j];
    return splitmix_draw(key, (uint64_t)h, (uint64_t)rn, (uint64_t)j, (uint64_t)n);
  };
  double sc[3] = {0, 0, 0}, rc[3] = {0, 0, 0};
  for (int j = 0; j < rn && ok; j++) {
    const int64_t i = index(j);
    ok = i >= 0 && i < n;                                   // (explicit indices: out of range makes the hypothesis invalid)
    if (!ok) break;
    const float* s = src + 3 * (b0 + i);
    const float* r = ref + 3 * (b0 + i);
    ok = finite3(s[0], s[1], s[2]) && finite3(r[0], r[1], r[2]);
    for (int d = 0; d < 3; d++) { sc[d] += s[d]; rc[d] += r[d]; }
  }
  if (CHECK && ok && edge_t > 0.0) {
    for (int a = 0; a < rn && ok; a++)
      for (int b = a + 1; b < rn && ok; b++) {
        const int64_t ia = index(a), ib = index(b);
        const float *sa = src + 3 * (b0 + ia), *sb = src + 3 * (b0 + ib), *ra = ref + 3 * (b0 + ia), *rb = ref + 3 * (b0 + ib);
        const double sx = (double)sa[0] - sb[0], sy = (double)sa[1] - sb[1], sz = (double)sa[2] - sb[2];
        const double rx = (double)ra[0] - rb[0], ry = (double)ra[1] - rb[1], rz = (double)ra[2] - rb[2];
        const double ds = sqrt((sx * sx + sy * sy) + sz * sz), dr = sqrt((rx * rx + ry * ry) + rz * rz);
        ok = !(ds < edge_t * dr || dr < edge_t * ds);
      }
  }
  if (!ok) {
    const float nan = __int_as_float(0x7fc00000);
    for (int k = 0; k < 3; k++) out[k] = make_float4(nan, nan, nan, nan);
    if (CHECK && passed) passed[(int64_t)p * H + h] = 0;
    return;
  }
  for (int d = 0; d < 3; d++) { sc[d] /= rn; rc[d] /= rn; }
  double Hm[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int j = 0; j < rn; j++) {
    const int64_t i = index(j);
    const float* s = src + 3 * (b0 + i);
    const float* r = ref + 3 * (b0 + i);
    const double ds[3] = {s[0] - sc[0], s[1] - sc[1], s[2] - sc[2]}, dr[3] = {r[0] - rc[0], r[1] - rc[1], r[2] - rc[2]};
    for (int a = 0; a < 3; a++)
      for (int c = 0; c < 3; c++) Hm[a][c] += ds[a] * dr[c];
  }
  float T[16];
  kabsch(Hm, sc, rc, T);
  if (CHECK && check_thr2 > 0.f) {
    for (int j = 0; j < rn && ok; j++) {                      // d = R s + (t - r) and d^2 as ransac_score_kernel forms them
      const int64_t i = index(j);
      const float* s = src + 3 * (b0 + i);
      const float* r = ref + 3 * (b0 + i);
      float d[3];
      for (int k = 0; k < 3; k++)
        d[k] = __builtin_fmaf(T[4 * k], s[0], __builtin_fmaf(T[4 * k + 1], s[1], __builtin_fmaf(T[4 * k + 2], s[2], T[4 * k + 3] - r[k])));
      const float d2 = __builtin_fmaf(d[2], d[2], __builtin_fmaf(d[1], d[1], d[0] * d[0]));
      ok = !(d2 > check_thr2);
    }
    if (!ok) {
      const float nan = __int_as_float(0x7fc00000);
      for (int k = 0; k < 16; k++) T[k] = nan;
    }
  }
  if (CHECK && passed) passed[(int64_t)p * H + h] = ok;
  for (int k = 0; k < 3; k++) out[k] = make_float4(T[4 * k], T[4 * k + 1], T[4 * k + 2], T[4 * k + 3]);
}

__global__ __launch_bounds__(kScoreThreads) void ransac_score_kernel(const float* __restrict__ src, const float* __restrict__ ref,
                                                                     const int64_t* __restrict__ offsets, int H, float thr2,
                                                                     const float4* __restrict__ hyp, int32_t* __restrict__ counts,
                                                                     float* __restrict__ err_sums, Candidate* __restrict__ cand) {
  __shared__ float4 s_lds[kChunk], r_lds[kChunk];
  __shared__ Candidate wave_best[kScoreThreads / SE3_WAVE];
  const int p = blockIdx.y;
  const int64_t b0 = offsets[p], n = offsets[p + 1] - b0;
  const int h0 = blockIdx.x * kTile + threadIdx.x, h1 = h0 + kScoreThreads;
  // the two hypotheses' rows as packed pairs (x: h0, y: h1); a hypothesis beyond H is NaN and never counts
  float a[12], b[12];
  {
    const float nan = __int_as_float(0x7fc00000);
    const float4* t0 = hyp + ((int64_t)p * H + h0) * 3;
    const float4* t1 = hyp + ((int64_t)p * H + h1) * 3;
    for (int k = 0; k < 3; k++) {
      const float4 u = h0 < H ? t0[k] : make_float4(nan, nan, nan, nan);
      const float4 v = h1 < H ? t1[k] : make_float4(nan, nan, nan, nan);
      a[4 * k] = u.x, a[4 * k + 1] = u.y, a[4 * k + 2] = u.z, a[4 * k + 3] = u.w;
      b[4 * k] = v.x, b[4 * k + 1] = v.y, b[4 * k + 2] = v.z, b[4 * k + 3] = v.w;
    }
  }
  f32x2 R[3][3], t[3];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) R[i][j] = f32x2{a[4 * i + j], b[4 * i + j]};
    t[i] = f32x2{a[4 * i + 3], b[4 * i + 3]};
  }
  int c0 = 0, c1 = 0;
  float e0 = 0.f, e1 = 0.f;
  for (int64_t base = 0; base < n; base += kChunk) {
    const int m = (int)(n - base < kChunk ? n - base : kChunk);
    __syncthreads();
    for (int i = threadIdx.x; i < m; i += kScoreThreads) {
      const int64_t g = b0 + base + i;
      s_lds[i] = make_float4(src[3 * g], src[3 * g + 1], src[3 * g + 2], 0.f);
      r_lds[i] = make_float4(ref[3 * g], ref[3 * g + 1], ref[3 * g + 2], 0.f);
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < m; i++) {
      const float4 s = s_lds[i], r = r_lds[i];          // one address per wave: an LDS broadcast
      const f32x2 sx = {s.x, s.x}, sy = {s.y, s.y}, sz = {s.z, s.z};
      const f32x2 dx = fma2(R[0][0], sx, fma2(R[0][1], sy, fma2(R[0][2], sz, t[0] - r.x)));   // R s + (t - r): 3 subs, 9 FMAs
      const f32x2 dy = fma2(R[1][0], sx, fma2(R[1][1], sy, fma2(R[1][2], sz, t[1] - r.y)));
      const f32x2 dz = fma2(R[2][0], sx, fma2(R[2][1], sy, fma2(R[2][2], sz, t[2] - r.z)));
      const f32x2 d2 = fma2(dz, dz, fma2(dy, dy, dx * dx));
      const bool in0 = d2.x < thr2, in1 = d2.y < thr2;   // false for NaN: non-finite correspondences and invalid hypotheses
      c0 += in0;
      c1 += in1;
      e0 += in0 ? d2.x : 0.f;                            // (+0 leaves the sum unchanged: the serial sum over the inliers)
      e1 += in1 ? d2.y : 0.f;
    }
  }
  if (counts) {
    if (h0 < H) counts[(int64_t)p * H + h0] = c0, err_sums[(int64_t)p * H + h0] = e0;
    if (h1 < H) counts[(int64_t)p * H + h1] = c1, err_sums[(int64_t)p * H + h1] = e1;
  }
  // the workgroup's best (count, err, h): lane, wave (xor tree), then the waves in order -- a total order, so any tree gives the same
  int bc = h0 < H ? c0 : -1, bh = h0;
  float be = e0;
  if (h1 < H && beats(c1, e1, h1, bc, be, bh)) bc = c1, be = e1, bh = h1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int oc = __shfl_xor(bc, o), oh = __shfl_xor(bh, o);
    const float oe = __shfl_xor(be, o);
    if (beats(oc, oe, oh, bc, be, bh)) bc = oc, be = oe, bh = oh;
  }
  if (se3_lane() == 0) wave_best[threadIdx.x / SE3_WAVE] = Candidate{bc, be, bh, 0};
  __syncthreads();
  if (threadIdx.x == 0) {
    Candidate best = wave_best[0];
    for (int w = 1; w < kScoreThreads / SE3_WAVE; w++) {
      const Candidate c = wave_best[w];
      if (beats(c.count, c.err, c.h, best.count, best.err, best.h)) best = c;
    }
    cand[(int64_t)p * gridDim.x + blockIdx.x] = best;
  }
}

// one wave per pair; num_blocks == 0: no hypotheses were scored (identity; per-hypothesis outputs, if any, are zeroed)
__global__ __launch_bounds__(SE3_WAVE) void ransac_select_kernel(const int64_t* __restrict__ offsets, int H, int num_blocks,
                                                                 const float4* __restrict__ hyp, const Candidate* __restrict__ cand,
                                                                 float* __restrict__ transforms, float* __restrict__ fitness,
                                                                 float* __restrict__ inlier_rmse, int32_t* __restrict__ best_hypothesis,
                                                                 int32_t* __restrict__ counts, float* __restrict__ err_sums,
                                                                 uint8_t* __restrict__ passed) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const int64_t n = offsets[p + 1] - offsets[p];
  if (num_blocks == 0 && counts)
    for (int64_t h = lane; h < H; h += SE3_WAVE) counts[(int64_t)p * H + h] = 0, err_sums[(int64_t)p * H + h] = 0.f;
  if (num_blocks == 0 && passed)
    for (int64_t h = lane; h < H; h += SE3_WAVE) passed[(int64_t)p * H + h] = 0;
  int bc = -1, bh = 0;
  float be = 0.f;
  for (int k = lane; k < num_blocks; k += SE3_WAVE) {
    const Candidate c = cand[(int64_t)p * num_blocks + k];
    if (beats(c.count, c.err, c.h, bc, be, bh)) bc = c.count, be = c.err, bh = c.h;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int oc = __shfl_xor(bc, o), oh = __shfl_xor(bh, o);
    const float oe = __shfl_xor(be, o);
    if (beats(oc, oe, oh, bc, be, bh)) bc = oc, be = oe, bh = oh;
  }
  if (lane != 0) return;
  float* T = transforms + 16 * p;
  if (bc > 0) {                                            // the identity (fitness 0, RMSE 0) beats every hypothesis without inliers
    const float4* w = hyp + ((int64_t)p * H + bh) * 3;
    for (int k = 0; k < 3; k++) {
      const float4 v = w[k];
      T[4 * k] = v.x, T[4 * k + 1] = v.y, T[4 * k + 2] = v.z, T[4 * k + 3] = v.w;
    }
    T[12] = 0.f, T[13] = 0.f, T[14] = 0.f, T[15] = 1.f;
    fitness[p] = (float)((double)bc / (double)n);
    inlier_rmse[p] = (float)sqrt((double)be / (double)bc);
    best_hypothesis[p] = bh;
  } else {
    for (int k = 0; k < 16; k++) T[k] = (k % 5 == 0) ? 1.f : 0.f;
    fitness[p] = 0.f;
    inlier_rmse[p] = 0.f;
    best_hypothesis[p] = -1;
  }
}

size_t hyp_bytes(int num_pairs, int H) { return (size_t)num_pairs * (size_t)H * 3 * sizeof(float4); }

}  // namespace

extern "C" size_t se3_ransac_correspondences_workspace_bytes(int num_pairs, int num_iterations) {
  if (num_pairs <= 0 || num_iterations <= 0) return 0;
  return hyp_bytes(num_pairs, num_iterations) + (size_t)num_pairs * se3_cdiv(num_iterations, kTile) * sizeof(Candidate);
}

namespace {
int ransac_stack(const char* what, const float* src_points, const float* ref_points, const int64_t* offsets, int num_pairs,
                 float distance_threshold, int ransac_n, int num_iterations, uint64_t seed, const int32_t* hypothesis_indices,
                 bool checked, double edge_length_similarity, int check_distance, void* workspace, size_t workspace_bytes, float* transforms,
                 float* fitness, float* inlier_rmse, int32_t* best_hypothesis, int32_t* counts, float* err_sums, uint8_t* passed,
                 void* stream) {
  SE3_REQUIRE(src_points && ref_points && offsets && transforms && fitness && inlier_rmse && best_hypothesis, SE3_ERR_INVALID_ARG,
              "%s: null pointer", what);
  SE3_REQUIRE((counts == nullptr) == (err_sums == nullptr), SE3_ERR_INVALID_ARG, "%s: counts and err_sums go together", what);
  SE3_REQUIRE(num_pairs >= 0 && num_pairs <= 65535 && num_iterations >= 0, SE3_ERR_INVALID_ARG, "%s: %d pairs, %d iterations", what,
              num_pairs, num_iterations);
  SE3_REQUIRE(ransac_n < 3 || ransac_n <= kMaxSample, SE3_ERR_UNSUPPORTED, "%s: ransac_n = %d (3 .. %d)", what, ransac_n, kMaxSample);
  SE3_REQUIRE(!checked || (edge_length_similarity >= 0.0 && edge_length_similarity <= 1.0), SE3_ERR_INVALID_ARG,
              "%s: edge_length_similarity = %g (0: off, up to 1)", what, edge_length_similarity);
  if (num_pairs == 0) return SE3_OK;
  const size_t need = se3_ransac_correspondences_workspace_bytes(num_pairs, num_iterations);
  SE3_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), SE3_ERR_INVALID_ARG, "%s: workspace of %zu bytes, %zu needed", what,
              workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const int H = num_iterations;
  const bool valid = ransac_n >= 3 && distance_threshold > 0.f && H > 0;   // (a NaN threshold is not > 0)
  float4* hyp = (float4*)workspace;
  Candidate* cand = valid ? (Candidate*)((char*)workspace + hyp_bytes(num_pairs, H)) : nullptr;
  const int blocks = valid ? (int)se3_cdiv(H, kTile) : 0;
  const float thr2 = distance_threshold * distance_threshold;
  if (valid) {
    const dim3 fit_grid((unsigned)se3_cdiv(H, kFitThreads), (unsigned)num_pairs);
    if (checked)
      ransac_fit_kernel<true><<<fit_grid, kFitThreads, 0, st>>>(src_points, ref_points, offsets, H, ransac_n, splitmix64(seed),
                                                                hypothesis_indices, 1, hyp, edge_length_similarity,
                                                                check_distance ? thr2 : 0.f, passed);
    else
      ransac_fit_kernel<false><<<fit_grid, kFitThreads, 0, st>>>(src_points, ref_points, offsets, H, ransac_n, splitmix64(seed),
                                                                 hypothesis_indices, 1, hyp, 0.0, 0.f, nullptr);
    ransac_score_kernel<<<dim3((unsigned)blocks, (unsigned)num_pairs), kScoreThreads, 0, st>>>(src_points, ref_points, offsets, H, thr2, hyp,
                                                                                              counts, err_sums, cand);
  }
  ransac_select_kernel<<<(unsigned)num_pairs, SE3_WAVE, 0, st>>>(offsets, H, blocks, hyp, cand, transforms, fitness, inlier_rmse,
                                                               best_hypothesis, counts, err_sums, passed);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}
}  // namespace

extern "C" int se3_ransac_correspondences_stack(const float* src_points, const float* ref_points, const int64_t* offsets, int num_pairs,
                                                float distance_threshold, int ransac_n, int num_iterations, uint64_t seed,
                                                const int32_t* hypothesis_indices, void* workspace, size_t workspace_bytes,
                                                float* transforms, float* fitness, float* inlier_rmse, int32_t* best_hypothesis,
                                                int32_t* counts, float* err_sums, void* stream) {
  return ransac_stack("ransac_correspondences_stack", src_points, ref_points, offsets, num_pairs, distance_threshold, ransac_n,
                      num_iterations, seed, hypothesis_indices, false, 0.0, 0, workspace, workspace_bytes, transforms, fitness, inlier_rmse,
                      best_hypothesis, counts, err_sums, nullptr, stream);
}

extern "C" int se3_ransac_correspondences_checked_stack(const float* src_points, const float* ref_points, const int64_t* offsets,
                                                        int num_pairs, float distance_threshold, int ransac_n, int num_iterations,
                                                        uint64_t seed, const int32_t* hypothesis_indices, double edge_length_similarity,
                                                        int check_distance, void* workspace, size_t workspace_bytes, float* transforms,
                                                        float* fitness, float* inlier_rmse, int32_t* best_hypothesis, int32_t* counts,
                                                        float* err_sums, uint8_t* passed, void* stream) {
  return ransac_stack("ransac_correspondences_checked_stack", src_points, ref_points, offsets, num_pairs, distance_threshold, ransac_n,
                      num_iterations, seed, hypothesis_indices, true, edge_length_similarity, check_distance, workspace, workspace_bytes,
                      transforms, fitness, inlier_rmse, best_hypothesis, counts, err_sums, passed, stream);
}
