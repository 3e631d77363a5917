// eval.py's benchmark metrics for stacked pairs (experiments/se3ete.3dmatch/eval.py:42-357, experiments/se3eti.kitti/eval.py:32-185):
// the per-pair correspondence and registration metrics of geotransformer/utils/registration.py and threedmatch/utils.py, and the
// per-scene / overall summaries eval.py prints.  Every kernel handles all P pairs (or G groups) of a call in one launch; nothing is read
// back to the host.  se3et_amd/benchmark.py carries the same contract.
//
//   bench_overlap_kernel     evaluate_correspondences' overlap (compute_overlap -> a cKDTree nearest neighbour in the reference): the
//                            fraction of ref_corr points whose nearest transformed src_corr point of the same pair is closer than r.
//                            Brute force, tiled: grid (query tile, pair), 512 queries per workgroup (two per lane, as packed float32
//                            pairs); the pair's transformed src points pass through LDS in chunks of kChunk, read at one address per
//                            wave (broadcast).  The predicate is "some j with d^2(i, j) < r^2", which equals min_j d < r, so a wave
//                            skips the rest of a chunk once all its lanes have a hit, and the workgroup stops once all its waves have.
//                            Tiles past a pair's own count return at once: the grid spans the largest pair the caller names.
//   bench_corr_kernel        one workgroup per pair: inlier count and residual sum in float64, then the pair's row.
//   bench_sparse_kernel      evaluate_sparse_correspondences (registration.py:253-280) with set semantics: one workgroup per pair sets
//                            bits of its (N x M) ground-truth and prediction bitmaps with atomicOr; the old bit tells a first setter,
//                            which gives distinct counts, and row / column bitmaps give the hit ratios.
//   bench_transform_kernel   compute_transform_error (threedmatch/utils.py:131-137) and compute_registration_error (registration.py:51-67),
//                            one thread per pair, float64.
//   bench_group_kernel       one workgroup per group (a 3DMatch scene, or all KITTI pairs): means, np.std and np.median of eval.py.
//   bench_overall_kernel     one thread: the overall row (3DMatch: the mean over scenes of each scene value, FMR_std = np.std of the
//                            scene FMRs; KITTI: the single group's row, FMR_std over pairs).
//
// Arithmetic contract (the overlap is the only test in float32):
//   overlap  T s = (fma(R[k][2], s.z, fma(R[k][1], s.y, R[k][0] * s.x)) + t[k])_k in float32 from the float32 transform;
//            d^2 = fma(dz, dz, fma(dy, dy, dx * dx)), d = q - T s, and r^2 = (float)((double)r * r), all float32.  The reference
//            transforms by a float32 GEMM and takes float64 distances, so only a point whose d^2 lies within float32 rounding of r^2
//            can be counted differently.  Non-finite points never hit.
//   IR, residual   per correspondence in float64 from the float32 inputs: d = ref - (R src + t), IR counts d^2 < r^2 (r^2 in float64);
//            the residual sums sqrt(d^2) -- each lane serially over a fixed stride, then a fixed tree.
//   sparse   integer counts; precision = pos / (pred + 1e-12), recall = pos / (gt + 1e-12), hit_ratio = 0.5 (rows_pos / (rows_gt + 1e-12)
//            + cols_pos / (cols_gt + 1e-12)), float64.  Node indices outside [0, N) x [0, M) are ignored.
//   transform   E = inv(T_gt) T_est (4x4 Gauss-Jordan with partial pivoting), q = nibabel's mat2quat(E[:3, :3]) (Bar-Itzhack: the
//            eigenvector of the largest eigenvalue of the symmetric 4x4 K, by 12 cyclic Jacobi sweeps, sign so that w >= 0),
//            err = ((e^T C) e) / C[0][0] with e = [t, q_x, q_y, q_z]; RRE = degrees(acos(clip(0.5 (tr(R_est^T R_gt) - 1), -1, 1))),
//            RTE = |t_gt - t_est|.  A pair without covariance gets err NaN.
//   summary  sums serially in pair order; empty sets give NaN (np.mean([]), np.median([])).
// Counts are integers and every sum has a fixed order, so a pair's row is bit-identical alone or in any batch, and from run to run.
#include <math.h>

#include "common.h"

namespace {

constexpr int kOvThreads = 256;
constexpr int kOvTile = 2 * kOvThreads;   // queries per overlap workgroup (two per lane)
constexpr int kChunk = 1024;              // transformed src points per LDS stage (16 KiB)
constexpr int kRowThreads = 256;
constexpr int kGroupThreads = 256;
constexpr int kMaxGroup = 4096;           // pairs per summary group (LDS-resident sort)
constexpr int kColumns = 14;              // PIR, PMR>0, PMR>=0.1, PMR>=0.3, PMR>=0.5, FMR, IR, OV, FMR_std, RR, mean/median RRE / RTE

typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }   // v_pk_fma_f32

__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7ff8000000000000ll); }

__global__ __launch_bounds__(kOvThreads) void bench_overlap_kernel(const float* __restrict__ ref, const float* __restrict__ src,
                                                                   const int64_t* __restrict__ offsets, const float* __restrict__ transforms,
                                                                   float r2, int32_t* __restrict__ hits) {
  __shared__ float4 pts[kChunk];
  const int p = blockIdx.y;
  const int64_t b0 = offsets[p], n = offsets[p + 1] - b0;
  const int64_t q0 = (int64_t)blockIdx.x * kOvTile;
  if (q0 >= n) return;                                     // (uniform over the workgroup)
  const float* T = transforms + 16 * p;
  float R[3][3], t[3];
  for (int k = 0; k < 3; k++) {
    for (int c = 0; c < 3; c++) R[k][c] = T[4 * k + c];
    t[k] = T[4 * k + 3];
  }
  const float nan = __int_as_float(0x7fc00000);
  const int64_t i0 = q0 + threadIdx.x, i1 = i0 + kOvThreads;
  f32x2 qx, qy, qz;
  qx.x = i0 < n ? ref[3 * (b0 + i0)] : nan, qy.x = i0 < n ? ref[3 * (b0 + i0) + 1] : nan, qz.x = i0 < n ? ref[3 * (b0 + i0) + 2] : nan;
  qx.y = i1 < n ? ref[3 * (b0 + i1)] : nan, qy.y = i1 < n ? ref[3 * (b0 + i1) + 1] : nan, qz.y = i1 < n ? ref[3 * (b0 + i1) + 2] : nan;
  // a query past n counts as done, so it never holds its wave back
  bool h0 = i0 >= n, h1 = i1 >= n;
  for (int64_t base = 0; base < n; base += kChunk) {
    const int m = (int)(n - base < kChunk ? n - base : kChunk);
    __syncthreads();
    for (int j = threadIdx.x; j < m; j += kOvThreads) {
      const float* s = src + 3 * (b0 + base + j);
      const float sx = s[0], sy = s[1], sz = s[2];
      float w[3];
      for (int k = 0; k < 3; k++) w[k] = __builtin_fmaf(R[k][2], sz, __builtin_fmaf(R[k][1], sy, R[k][0] * sx)) + t[k];
      pts[j] = make_float4(w[0], w[1], w[2], 0.f);
    }
    __syncthreads();
    for (int j0 = 0; j0 < m && !__all(h0 && h1); j0 += 64) {
      const int je = j0 + 64 < m ? j0 + 64 : m;
#pragma unroll 8
      for (int j = j0; j < je; j++) {
        const float4 s = pts[j];                           // one address per wave: an LDS broadcast
        const f32x2 dx = qx - s.x, dy = qy - s.y, dz = qz - s.z;
        const f32x2 d2 = fma2(dz, dz, fma2(dy, dy, dx * dx));
        h0 |= d2.x < r2;                                   // false for NaN
        h1 |= d2.y < r2;
      }
    }
    if (__syncthreads_and(h0 && h1)) break;
  }
  // one integer add per wave: counts do not depend on the order
  const unsigned long long b = __ballot(i0 < n && h0), c = __ballot(i1 < n && h1);
  if (se3_lane() == 0) {
    const int cnt = __popcll(b) + __popcll(c);
    if (cnt) atomicAdd(hits + p, cnt);
  }
}

// out (P, 4) float64: overlap, inlier_ratio, residual (means over n; NaN for n == 0), num_corr
__global__ __launch_bounds__(kRowThreads) void bench_corr_kernel(const float* __restrict__ ref, const float* __restrict__ src,
                                                                 const int64_t* __restrict__ offsets, const float* __restrict__ transforms,
                                                                 double rr2, int64_t max_count, const int32_t* __restrict__ hits,
                                                                 double* __restrict__ out) {
  __shared__ double s_sum[kRowThreads];
  __shared__ int s_cnt[kRowThreads];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t b0 = offsets[p], n = offsets[p + 1] - b0;
  const float* T = transforms + 16 * p;
  double R[3][3], t[3];
  for (int k = 0; k < 3; k++) {
    for (int c = 0; c < 3; c++) R[k][c] = T[4 * k + c];
    t[k] = T[4 * k + 3];
  }
  double sum = 0.0;
  int cnt = 0;
  for (int64_t i = tid; i < n; i += kRowThreads) {
    const float* s = src + 3 * (b0 + i);
    const float* r = ref + 3 * (b0 + i);
    double d2 = 0.0;
    for (int k = 0; k < 3; k++) {
      const double d = (double)r[k] - ((R[k][0] * s[0] + R[k][1] * s[1] + R[k][2] * s[2]) + t[k]);
      d2 += d * d;
    }
    cnt += d2 < rr2;
    sum += sqrt(d2);
  }
  s_sum[tid] = sum;
  s_cnt[tid] = cnt;
  __syncthreads();
  for (int o = kRowThreads / 2; o > 0; o >>= 1) {
    if (tid < o) s_sum[tid] += s_sum[tid + o], s_cnt[tid] += s_cnt[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    double* row = out + 4 * p;
    const double dn = (double)n;
    // a pair longer than the grid's tiles was not fully searched: its overlap is NaN rather than a partial count
    row[0] = n > max_count ? nan64() : (double)hits[p] / dn;
    row[1] = (double)s_cnt[0] / dn;
    row[2] = s_sum[0] / dn;
    row[3] = dn;
  }
}

// bitmap words of one pair: gt (N M), pred (N M), gt rows, pos rows (N), gt cols, pos cols (M); se3_benchmark_sparse_words
__host__ __device__ __forceinline__ int64_t nm_words(int64_t N, int64_t M) { return (N * M + 31) / 32; }

__device__ __forceinline__ bool set_bit(uint32_t* words, int64_t bit) {
  const uint32_t mask = 1u << (bit & 31);
  return !(atomicOr(words + (bit >> 5), mask) & mask);   // true: this call set it
}

__global__ __launch_bounds__(kRowThreads) void bench_sparse_kernel(const int64_t* __restrict__ ref_idx, const int64_t* __restrict__ src_idx,
                                                                   const int64_t* __restrict__ pred_offsets, const int64_t* __restrict__ gt_idx,
                                                                   const int64_t* __restrict__ gt_offsets, const int64_t* __restrict__ node_counts,
                                                                   const int64_t* __restrict__ word_offsets, uint32_t* __restrict__ bits,
                                                                   double* __restrict__ out) {
  __shared__ int s_cnt[6];   // gt, pred, pos, gt rows, pos rows, gt cols, (pos cols below)
  __shared__ int s_pos_cols;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t N = node_counts[2 * p], M = node_counts[2 * p + 1];
  uint32_t* gt = bits + word_offsets[p];
  uint32_t* pred = gt + nm_words(N, M);
  uint32_t* gt_rows = pred + nm_words(N, M);
  uint32_t* pos_rows = gt_rows + (N + 31) / 32;
  uint32_t* gt_cols = pos_rows + (N + 31) / 32;
  uint32_t* pos_cols = gt_cols + (M + 31) / 32;
  if (tid < 6) s_cnt[tid] = 0;
  if (tid == 0) s_pos_cols = 0;
  __syncthreads();
  for (int64_t k = gt_offsets[p] + tid; k < gt_offsets[p + 1]; k += kRowThreads) {
    const int64_t a = gt_idx[2 * k], b = gt_idx[2 * k + 1];
    if (a < 0 || a >= N || b < 0 || b >= M) continue;
    if (set_bit(gt, a * M + b)) atomicAdd(&s_cnt[0], 1);
    if (set_bit(gt_rows, a)) atomicAdd(&s_cnt[3], 1);
    if (set_bit(gt_cols, b)) atomicAdd(&s_cnt[5], 1);
  }
  __syncthreads();                                         // (the atomics above are complete: the gt bitmap is final)
  for (int64_t k = pred_offsets[p] + tid; k < pred_offsets[p + 1]; k += kRowThreads) {
    const int64_t a = ref_idx[k], b = src_idx[k];
    if (a < 0 || a >= N || b < 0 || b >= M) continue;
    const int64_t bit = a * M + b;
    if (!set_bit(pred, bit)) continue;                     // a duplicate: counted once
    atomicAdd(&s_cnt[1], 1);
    if (!(atomicOr(gt + (bit >> 5), 0u) & (1u << (bit & 31)))) continue;   // (an atomic read: L2, never a stale L1 line)
    atomicAdd(&s_cnt[2], 1);
    if (set_bit(pos_rows, a)) atomicAdd(&s_cnt[4], 1);
    if (set_bit(pos_cols, b)) atomicAdd(&s_pos_cols, 1);
  }
  __syncthreads();
  if (tid == 0) {
    double* row = out + 3 * p;
    const double pos = s_cnt[2];
    row[0] = pos / ((double)s_cnt[1] + 1e-12);
    row[1] = pos / ((double)s_cnt[0] + 1e-12);
    row[2] = 0.5 * ((double)s_cnt[4] / ((double)s_cnt[3] + 1e-12) + (double)s_pos_cols / ((double)s_cnt[5] + 1e-12));
  }
}

// inverse of a 4x4 matrix by Gauss-Jordan elimination with partial pivoting (false: singular)
__device__ bool invert4(const double* A, double* X) {
  double a[4][8];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) a[i][j] = A[4 * i + j], a[i][4 + j] = i == j ? 1.0 : 0.0;
  for (int c = 0; c < 4; c++) {
    int piv = c;
    for (int i = c + 1; i < 4; i++)
      if (fabs(a[i][c]) > fabs(a[piv][c])) piv = i;
    if (a[piv][c] == 0.0) return false;
    if (piv != c)
      for (int j = 0; j < 8; j++) {
        const double tmp = a[c][j];
        a[c][j] = a[piv][j], a[piv][j] = tmp;
      }
    const double inv = 1.0 / a[c][c];
    for (int j = 0; j < 8; j++) a[c][j] *= inv;
    for (int i = 0; i < 4; i++) {
      if (i == c) continue;
      const double f = a[i][c];
      for (int j = 0; j < 8; j++) a[i][j] -= f * a[c][j];
    }
  }
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) X[4 * i + j] = a[i][4 + j];
  return true;
}

// nibabel.quaternions.mat2quat: (w, x, y, z) of the largest eigenvalue's eigenvector of K (Bar-Itzhack 2000), w >= 0
__device__ void mat2quat(const double R[3][3], double q[4]) {
  // nibabel names the flat matrix Qxx, Qyx, Qzx, Qxy, Qyy, Qzy, Qxz, Qyz, Qzz (so Qyx = R[0][1])
  const double Qxx = R[0][0], Qyx = R[0][1], Qzx = R[0][2], Qxy = R[1][0], Qyy = R[1][1], Qzy = R[1][2], Qxz = R[2][0], Qyz = R[2][1],
               Qzz = R[2][2];
  double K[4][4];
  K[0][0] = Qxx - Qyy - Qzz;
  K[1][0] = Qyx + Qxy, K[1][1] = Qyy - Qxx - Qzz;
  K[2][0] = Qzx + Qxz, K[2][1] = Qzy + Qyz, K[2][2] = Qzz - Qxx - Qyy;
  K[3][0] = Qyz - Qzy, K[3][1] = Qzx - Qxz, K[3][2] = Qxy - Qyx, K[3][3] = Qxx + Qyy + Qzz;
  for (int i = 0; i < 4; i++) {
    for (int j = 0; j < i; j++) K[i][j] /= 3.0, K[j][i] = K[i][j];
    K[i][i] /= 3.0;
  }
  double V[4][4];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
  // cyclic Jacobi, a fixed number of sweeps (quadratic convergence: 12 sweeps are far past float64 accuracy for a 4x4)
  for (int sweep = 0; sweep < 12; sweep++)
    for (int p = 0; p < 3; p++)
      for (int r = p + 1; r < 4; r++) {
        const double apr = K[p][r];
        if (apr == 0.0) continue;
        const double theta = (K[r][r] - K[p][p]) / (2.0 * apr);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < 4; k++) {                      // K <- J^T K J
          const double kp = K[k][p], kr = K[k][r];
          K[k][p] = c * kp - s * kr, K[k][r] = s * kp + c * kr;
        }
        for (int k = 0; k < 4; k++) {
          const double kp = K[p][k], kr = K[r][k];
          K[p][k] = c * kp - s * kr, K[r][k] = s * kp + c * kr;
        }
        K[p][r] = K[r][p] = 0.0;
        for (int k = 0; k < 4; k++) {                      // V <- V J
          const double vp = V[k][p], vr = V[k][r];
          V[k][p] = c * vp - s * vr, V[k][r] = s * vp + c * vr;
        }
      }
  int best = 0;
  for (int i = 1; i < 4; i++)
    if (K[i][i] > K[best][best]) best = i;
  const double sg = V[3][best] < 0 ? -1.0 : 1.0;
  q[0] = sg * V[3][best], q[1] = sg * V[0][best], q[2] = sg * V[1][best], q[3] = sg * V[2][best];
}

// out (P, 3) float64: err (NaN without covariance), rre (degrees), rte
__global__ __launch_bounds__(64) void bench_transform_kernel(const double* __restrict__ gt, const double* __restrict__ est,
                                                             const double* __restrict__ cov, const int32_t* __restrict__ has_cov,
                                                             int num_pairs, double* __restrict__ out) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= num_pairs) return;
  const double* G = gt + 16 * p;
  const double* S = est + 16 * p;
  double* row = out + 3 * p;
  // compute_registration_error: x = 0.5 (trace(R_est^T R_gt) - 1)
  double tr = 0.0;
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) tr += S[4 * k + i] * G[4 * k + i];
  const double x = fmin(fmax(0.5 * (tr - 1.0), -1.0), 1.0);
  row[1] = 180.0 * acos(x) / M_PI;
  double dt2 = 0.0;
  for (int k = 0; k < 3; k++) dt2 += (G[4 * k + 3] - S[4 * k + 3]) * (G[4 * k + 3] - S[4 * k + 3]);
  row[2] = sqrt(dt2);
  if (!has_cov || !has_cov[p]) {
    row[0] = nan64();
    return;
  }
  double Gi[16];
  if (!invert4(G, Gi)) {
    row[0] = nan64();
    return;
  }
  double E[3][4];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) {
      double s = 0.0;
      for (int k = 0; k < 4; k++) s += Gi[4 * i + k] * S[4 * k + j];
      E[i][j] = s;
    }
  const double Rm[3][3] = {{E[0][0], E[0][1], E[0][2]}, {E[1][0], E[1][1], E[1][2]}, {E[2][0], E[2][1], E[2][2]}};
  double q[4];
  mat2quat(Rm, q);
  const double e[6] = {E[0][3], E[1][3], E[2][3], q[1], q[2], q[3]};
  const double* C = cov + 36 * p;
  double acc = 0.0;
  for (int j = 0; j < 6; j++) {                            // (e^T C) first, then with e: the order of er @ cov @ er^T
    double u = 0.0;
    for (int i = 0; i < 6; i++) u += e[i] * C[6 * i + j];
    acc += u * e[j];
  }
  row[0] = acc / C[0];
}

__device__ double median_sorted(const double* s, int k) { return k == 0 ? nan64() : 0.5 * (s[(k - 1) / 2] + s[k / 2]); }

// bitonic sort of s[0, k) in LDS (padded to a power of two with +inf), all threads of the workgroup
__device__ void lds_sort(double* s, int k) {
  int len = 1;
  while (len < k) len <<= 1;
  for (int i = k + threadIdx.x; i < len; i += kGroupThreads) s[i] = INFINITY;
  __syncthreads();
  for (int size = 2; size <= len; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < len; i += kGroupThreads) {
        const int j = i ^ stride;
        if (j > i) {
          const double a = s[i], b = s[j];
          if ((a > b) == ((i & size) == 0)) s[i] = b, s[j] = a;
        }
      }
      __syncthreads();
    }
}

// rows (P, 6) float64: precision, inlier_ratio, overlap, err, rre, rte; is_gt (P) int32 (3DMatch: the pair is a benchmark pair).
// group g owns pairs [group_offsets[g], group_offsets[g+1]); out (G, kColumns)
__global__ __launch_bounds__(kGroupThreads) void bench_group_kernel(const double* __restrict__ rows, const int32_t* __restrict__ is_gt,
                                                                    const int64_t* __restrict__ group_offsets, int kitti, double ir_thr,
                                                                    double err_thr, double rre_thr, double rte_thr,
                                                                    double* __restrict__ out) {
  __shared__ double s_val[kMaxGroup];
  __shared__ int s_k;
  const int g = blockIdx.x;
  const int64_t a = group_offsets[g], n = group_offsets[g + 1] - a;
  double* o = out + kColumns * g;
  if (n > kMaxGroup) {                                     // (refused on the host; never a partial answer)
    if (threadIdx.x < kColumns) o[threadIdx.x] = nan64();
    return;
  }
  auto accepted = [&](int64_t i) -> bool {
    const double* r = rows + 6 * i;
    return kitti ? (r[4] < rre_thr && r[5] < rte_thr) : (is_gt[i] && r[3] < err_thr);
  };
  if (threadIdx.x == 0) {
    const double dn = (double)n;
    double pir = 0, pmr0 = 0, pmr1 = 0, pmr3 = 0, pmr5 = 0, fmr = 0, ir = 0, ov = 0;
    double num_reg = 0, acc = 0, rre = 0, rte = 0;
    for (int64_t i = a; i < a + n; i++) {
      const double* r = rows + 6 * i;
      pir += r[0];
      pmr0 += r[0] > 0.0, pmr1 += r[0] >= 0.1, pmr3 += r[0] >= 0.3, pmr5 += r[0] >= 0.5;
      fmr += r[1] >= ir_thr;
      ir += r[1];
      ov += r[2];
      if (kitti || is_gt[i]) num_reg += 1.0;
      if (accepted(i)) acc += 1.0, rre += r[4], rte += r[5];
    }
    const double mfmr = fmr / dn;
    double var = 0.0;                                      // np.std of the 0/1 flags: sqrt(mean((x - mean)^2))
    for (int64_t i = a; i < a + n; i++) {
      const double d = (rows[6 * i + 1] >= ir_thr ? 1.0 : 0.0) - mfmr;
      var += d * d;
    }
    o[0] = pir / dn, o[1] = pmr0 / dn, o[2] = pmr1 / dn, o[3] = pmr3 / dn, o[4] = pmr5 / dn;
    o[5] = mfmr, o[6] = ir / dn, o[7] = ov / dn, o[8] = sqrt(var / dn);
    o[9] = acc / num_reg, o[10] = rre / acc, o[11] = rte / acc;
  }
  // medians over the accepted pairs
  for (int col = 4; col <= 5; col++) {
    __syncthreads();
    if (threadIdx.x == 0) {
      int k = 0;
      for (int64_t i = a; i < a + n; i++)
        if (accepted(i)) s_val[k++] = rows[6 * i + col];
      s_k = k;
    }
    __syncthreads();
    const int k = s_k;
    lds_sort(s_val, k);
    if (threadIdx.x == 0) o[col == 4 ? 12 : 13] = median_sorted(s_val, k);
  }
}

__global__ void bench_overall_kernel(const double* __restrict__ groups, int num_groups, int kitti, double* __restrict__ overall) {
  if (threadIdx.x != 0) return;
  if (kitti) {
    for (int c = 0; c < kColumns; c++) overall[c] = num_groups == 1 ? groups[c] : nan64();
    return;
  }
  const double dg = (double)num_groups;
  for (int c = 0; c < kColumns; c++) {
    double s = 0.0;
    for (int g = 0; g < num_groups; g++) s += groups[kColumns * g + c];
    overall[c] = s / dg;
  }
  double var = 0.0;                                        // FMR_std: np.std of the scenes' FMR
  for (int g = 0; g < num_groups; g++) {
    const double d = groups[kColumns * g + 5] - overall[5];
    var += d * d;
  }
  overall[8] = sqrt(var / dg);
}

}  // namespace

extern "C" size_t se3_benchmark_correspondences_workspace_bytes(int num_pairs) {
  return num_pairs <= 0 ? 0 : (size_t)num_pairs * sizeof(int32_t);
}

extern "C" int se3_benchmark_correspondences_stack(const float* ref_points, const float* src_points, const int64_t* offsets, int num_pairs,
                                                   int64_t max_count, const float* transforms, float positive_radius, void* workspace,
                                                   size_t workspace_bytes, double* out, void* stream) {
  SE3_REQUIRE(ref_points && src_points && offsets && transforms && out, SE3_ERR_INVALID_ARG, "benchmark_correspondences_stack: null pointer");
  SE3_REQUIRE(num_pairs >= 0 && num_pairs <= 65535 && max_count >= 0, SE3_ERR_INVALID_ARG,
              "benchmark_correspondences_stack: %d pairs, max_count %lld", num_pairs, (long long)max_count);
  if (num_pairs == 0) return SE3_OK;
  const size_t need = se3_benchmark_correspondences_workspace_bytes(num_pairs);
  SE3_REQUIRE(workspace && workspace_bytes >= need, SE3_ERR_INVALID_ARG, "benchmark_correspondences_stack: workspace of %zu bytes, %zu needed",
              workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  int32_t* hits = (int32_t*)workspace;
  const double r = positive_radius;
  const int64_t tiles = se3_cdiv(max_count, kOvTile);
  SE3_REQUIRE(tiles <= 0x7fffffff, SE3_ERR_UNSUPPORTED, "benchmark_correspondences_stack: max_count %lld", (long long)max_count);
  if (hipMemsetAsync(hits, 0, need, st) != hipSuccess) {
    se3_set_error("benchmark_correspondences_stack: hipMemsetAsync failed");
    return SE3_ERR_LAUNCH;
  }
  if (tiles > 0)
    bench_overlap_kernel<<<dim3((unsigned)tiles, (unsigned)num_pairs), kOvThreads, 0, st>>>(ref_points, src_points, offsets, transforms,
                                                                                            (float)(r * r), hits);
  bench_corr_kernel<<<(unsigned)num_pairs, kRowThreads, 0, st>>>(ref_points, src_points, offsets, transforms, r * r, max_count, hits, out);
  SE3_CHECK_LAUNCH("benchmark_correspondences_stack");
  return SE3_OK;
}

extern "C" int64_t se3_benchmark_sparse_words(int64_t num_ref_nodes, int64_t num_src_nodes) {
  if (num_ref_nodes < 0 || num_src_nodes < 0) return -1;
  return 2 * nm_words(num_ref_nodes, num_src_nodes) + 2 * ((num_ref_nodes + 31) / 32) + 2 * ((num_src_nodes + 31) / 32);
}

extern "C" size_t se3_benchmark_sparse_workspace_bytes(const int64_t* node_counts, int num_pairs) {
  if (!node_counts || num_pairs <= 0) return 0;
  int64_t words = 0;
  for (int p = 0; p < num_pairs; p++) words += se3_benchmark_sparse_words(node_counts[2 * p], node_counts[2 * p + 1]);
  return (size_t)words * sizeof(uint32_t);
}

extern "C" int se3_benchmark_sparse_stack(const int64_t* ref_node_indices, const int64_t* src_node_indices, const int64_t* pred_offsets,
                                          const int64_t* gt_node_corr_indices, const int64_t* gt_offsets, const int64_t* node_counts,
                                          const int64_t* word_offsets, int num_pairs, void* workspace, size_t workspace_bytes, double* out,
                                          void* stream) {
  SE3_REQUIRE(ref_node_indices && src_node_indices && pred_offsets && gt_node_corr_indices && gt_offsets && node_counts && word_offsets && out,
              SE3_ERR_INVALID_ARG, "benchmark_sparse_stack: null pointer");
  SE3_REQUIRE(num_pairs >= 0, SE3_ERR_INVALID_ARG, "benchmark_sparse_stack: %d pairs", num_pairs);
  if (num_pairs == 0) return SE3_OK;
  SE3_REQUIRE(workspace_bytes == 0 || workspace, SE3_ERR_INVALID_ARG, "benchmark_sparse_stack: null workspace");
  hipStream_t st = (hipStream_t)stream;
  if (workspace_bytes && hipMemsetAsync(workspace, 0, workspace_bytes, st) != hipSuccess) {
    se3_set_error("benchmark_sparse_stack: hipMemsetAsync failed");
    return SE3_ERR_LAUNCH;
  }
  bench_sparse_kernel<<<(unsigned)num_pairs, kRowThreads, 0, st>>>(ref_node_indices, src_node_indices, pred_offsets, gt_node_corr_indices,
                                                                   gt_offsets, node_counts, word_offsets, (uint32_t*)workspace, out);
  SE3_CHECK_LAUNCH("benchmark_sparse_stack");
  return SE3_OK;
}

extern "C" int se3_benchmark_transform_error_stack(const double* gt_transforms, const double* est_transforms, const double* covariances,
                                                   const int32_t* has_covariance, int num_pairs, double* out, void* stream) {
  SE3_REQUIRE(gt_transforms && est_transforms && out && (covariances || !has_covariance), SE3_ERR_INVALID_ARG,
              "benchmark_transform_error_stack: null pointer");
  SE3_REQUIRE(num_pairs >= 0, SE3_ERR_INVALID_ARG, "benchmark_transform_error_stack: %d pairs", num_pairs);
  if (num_pairs == 0) return SE3_OK;
  bench_transform_kernel<<<(unsigned)se3_cdiv(num_pairs, 64), 64, 0, (hipStream_t)stream>>>(gt_transforms, est_transforms, covariances,
                                                                                             has_covariance, num_pairs, out);
  SE3_CHECK_LAUNCH("benchmark_transform_error_stack");
  return SE3_OK;
}

extern "C" int se3_benchmark_summary(const double* rows, const int32_t* is_gt, const int64_t* group_offsets, int num_groups,
                                     int64_t max_group_pairs, int kitti, double inlier_ratio_threshold, double rmse_threshold,
                                     double rre_threshold, double rte_threshold, double* group_out, double* overall, void* stream) {
  SE3_REQUIRE(group_offsets && group_out && overall && (num_groups == 0 || rows) && (kitti || num_groups == 0 || is_gt), SE3_ERR_INVALID_ARG,
              "benchmark_summary: null pointer");
  SE3_REQUIRE(num_groups >= 0, SE3_ERR_INVALID_ARG, "benchmark_summary: %d groups", num_groups);
  SE3_REQUIRE(max_group_pairs <= kMaxGroup, SE3_ERR_UNSUPPORTED,
              "benchmark_summary: a group of %lld pairs (at most %d per group: split the groups)", (long long)max_group_pairs, kMaxGroup);
  SE3_REQUIRE(!kitti || num_groups == 1, SE3_ERR_INVALID_ARG, "benchmark_summary: KITTI takes all pairs as one group, got %d", num_groups);
  hipStream_t st = (hipStream_t)stream;
  if (num_groups > 0)
    bench_group_kernel<<<(unsigned)num_groups, kGroupThreads, 0, st>>>(rows, is_gt, group_offsets, kitti, inlier_ratio_threshold,
                                                                       rmse_threshold * rmse_threshold, rre_threshold, rte_threshold, group_out);
  bench_overall_kernel<<<1, 64, 0, st>>>(group_out, num_groups, kitti, overall);
  SE3_CHECK_LAUNCH("benchmark_summary");
  return SE3_OK;
}
