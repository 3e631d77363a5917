// RGB-D odometry (Open3D's legacy Odometry.cpp: ComputeRGBDOdometry with RGBDOdometryJacobianFromHybridTerm / ...FromColorTerm and
// CreateInformationMatrix) for up to SE3_PAIR_MAX_PAIRS frame pairs per call.  se3et_amd/odometry.py carries the same contract;
// csrc/rgbd_odometry_core.h holds the text that the kernels and se3_debug_rgbd_odometry_host share.
// (SE3_EXACT_FP: the file is built with contraction off, and every contract function fences itself as well.  SE3_NO_SLP_VECTORIZE: as in
// csrc/tsdf.hip, the float32 filter chains are kept out of packed arithmetic.)
//
// Contract: preparation, per frame.  All float32, every operation rounded on its own.
//   1. Depth: d = f32(raw) / f32(depth_scale); d > f32(depth_trunc) makes d = 0; then d <= f32(min_depth), d > f32(max_depth) and a
//      non-finite d become NaN.
//   2. Intensity: uint8 RGB ((0.2990f R + 0.5870f G) + 0.1140f B) / 255f; uint8 grey c / 255f; float32 alike without the division.
//   3. Both images pass Gaussian3: h(x, y) = (0.25f a + 0.5f b) + 0.25f c over in(x - 1, y), in(x, y), in(x + 1, y), then the same taps
//      over h(x, y - 1), h(x, y), h(x, y + 1); coordinates are clamped to the image.  A NaN depth spreads to its neighbours (Open3D's
//      behaviour).  The results are level 0.
//   4. Level l + 1 of floor(H / 2) x floor(W / 2): intensity is Gaussian3 of level l, then ((a + b) + (c + d)) 0.25f over the block
//      a = (2x, 2y), b = (2x + 1, 2y), c = (2x, 2y + 1), d = (2x + 1, 2y + 1); depth is that mean alone.  Intrinsics of level l: all four
//      values times 2^-l.
//   5. Sobel images of intensity and depth, per level, of every frame that is some pair's target: with e(x, y) = in(x + 1, y) - in(x - 1, y)
//      and s(x, y) = (in(x - 1, y) + 2f in(x, y)) + in(x + 1, y), dx = (e(x, y - 1) + 2f e(x, y)) + e(x, y + 1) and dy = s(x, y + 1) -
//      s(x, y - 1), clamped coordinates.  The factor 0.125 is applied where a gradient is used; a NaN depth gradient counts as 0 there.
//
// Contract: correspondences of a pair at level l under T = (R, t).  All float64.
//   1. M = K (R K^-1) and K t in the operation order of rg_camera (csrc/rgbd_odometry_core.h spells it out).
//   2. For source pixel (u, v), index s = v W + u, with non-NaN depth d: q_a = d ((M[a][0] u + M[a][1] v) + M[a][2]) + (K t)_a.  Skipped
//      unless q_z > 0.  u_t = floor(q_x / q_z + 0.5), v_t likewise; skipped when outside the image, when the target depth d_t there is NaN,
//      or when |q_z - d_t| > max_depth_diff.
//   3. A target pixel claimed by several source pixels keeps the one with the smallest hi32(q_z), the high 32 bits of q_z's float64
//      pattern (q_z cut to 20 mantissa bits), then the smallest s.
//
// Contract: intensity normalisation of a pair.  Over the correspondences at level 0 under the initial transform: a_s = 0.5 / (sum I_s / n),
// a_t = 0.5 / (sum I_t / n); n = 0 fails the pair (SE3_RGBD_EMPTY).  The factors multiply intensities and intensity gradients where read.
//
// Contract: one iteration.  For a correspondence (s, j): d the source depth, p = (d xr, d yr, d) with xr = (u - cx) / fx, yr = (v - cy) / fy;
// (x, y, z)_a = ((R[a][0] p_x + R[a][1] p_y) + R[a][2] p_z) + t_a.  For a gradient g: c0 = (g_x fx) / z, c1 = (g_y fy) / z,
// c2 = -((c0 x + c1 y) / z), row(g) = (y c2 - z c1, z c0 - x c2, x c1 - y c0, c0, c1, c2).
//   colour row   J = w_I row(a_t (0.125 S_I)),  r = w_I ((a_t I_t) - (a_s I_s))
//   depth row    J = w_D (row(0.125 S_D) + (-y, x, 0, 0, 0, -1)),  r = w_D (D_t - z)                    (method hybrid alone)
//   hybrid: w_D = sqrt(0.95), w_I = sqrt(0.05); colour: w_I = 1.  The 29 sums: the upper triangle of J^T J by rows, J^T r, r^2 (a pixel's
//   colour row before its depth row), the count.  (J^T J) x = -J^T r by icp_cholesky6; T <- M(x) T, M(x) = [Rz(x_2) Ry(x_1) Rx(x_0) | x_3..5]
//   with icp_sin / icp_cos.  A pair fails and stays frozen on a non-finite sum (SE3_RGBD_NONFINITE), fewer than 6 correspondences
//   (TOO_FEW), a refused pivot (SINGULAR), a rotation component of 1 rad or more (STEP_REFUSED).  A failed pair returns success 0, the
//   identity, a zero information matrix and count 0.  Every iteration of the schedule runs: there is no convergence test.
//
// Contract: information matrix.  Over the correspondences at level 0 under the final transform, p = d_t (xr, yr, 1) of the TARGET pixel:
// the sum of G^T G, G = [[0, p_z, -p_y, 1, 0, 0], [-p_z, 0, p_x, 0, 1, 0], [p_y, -p_x, 0, 0, 0, 1]], every entry ((g0 g0') + (g1 g1')) + (g2 g2').
//
// Sums.  Target pixels are cut into chunks of SE3_RGBD_CHUNK in index order; a chunk is summed in icp_sum's order (lane l of 256 adds
// pixels l, l + 256, .. ascending, then the halving tree), and a pair's chunk partials are folded in icp_sum's order over the chunks.
// The order depends on the level's image size alone.
//
// Departures from Open3D.  The tie rule of correspondences item 3 (Open3D's result under ties depends on its thread merge order) and
// its 20-bit q_z.  The intensity factors are applied where intensities are read (Open3D scales the images before it builds the
// pyramids; equal up to rounding); unscaled per-frame pyramids are what lets pairs share frames.  Sine and cosine are the library's
// series.  Refusals: Open3D has no pivot test and no step limit.  depth_trunc of the RGBD image and min_depth / max_depth of the option
// are one conversion.
//
// Determinism.  The z-buffer is a 64-bit unsigned minimum, which does not depend on arrival order; there are no float atomics.  A pair's
// result is bit-identical alone, anywhere in a batch, whether it shares frames or not, and from run to run.
//
// Launches, all on the caller's stream from one C call.
//   rgbd_gauss_kernel   one workgroup of 256 per tile of 32 x 16 Gaussian outputs: the tile and its halo are converted on load into LDS,
//                       the row pass and the column pass go through LDS, and for a pyramid step the 2 x 2 means are taken from LDS too.
//   rgbd_down_kernel    the depth's 2 x 2 mean.
//   rgbd_sobel_kernel   the same tile shape; both passes through LDS; frames that are no pair's target return at once.
//   rgbd_init_kernel    T <- T0.  The map is cleared to all ones once per call; every reader frees what it read.
//   rgbd_claim_kernel   one thread per source pixel: one no-return 64-bit atomic minimum per surviving pixel.
//   rgbd_sums_kernel    one workgroup per (chunk, pair): the 29 partials of the chunk.
//   rgbd_finish_kernel  one workgroup per pair: folds the partials, solves, updates T, writes the status.
//   The schedule: preparation (7 launches for 3 levels); init, clear; claim, sums, finish for the normalisation; claim, sums, finish
//   per iteration, coarsest level first; claim, sums, finish for the information matrix.
#include <math.h>

#include <vector>

#include "common.h"
#include "rgbd_odometry_core.h"

namespace {

constexpr int kRgbdThreads = 256;
constexpr int kTileW = 32, kTileH = 16;
static_assert(kRgbdThreads == kIcpLanes, "a workgroup is icp_sum's lanes");
static_assert(kRgbdMaxLevels == SE3_RGBD_MAX_LEVELS && kRgbdMaxImage == SE3_RGBD_MAX_IMAGE && kRgbdMinSide == SE3_RGBD_MIN_SIDE &&
                  kRgbdChunk == SE3_RGBD_CHUNK && kRgbdSums == SE3_RGBD_SUMS && kRgbdImages == SE3_RGBD_IMAGES,
              "rgbd_odometry_core.h and include/se3et_hip.h name the same limits");
static_assert(kRgbdHybrid == SE3_RGBD_HYBRID && kRgbdColor == SE3_RGBD_COLOR, "and the same methods");
static_assert(kRgbdMaxImage == SE3_TSDF_MAX_IMAGE, "image sides as in the TSDF limits");

// the raw images of a call
struct RgRaw {
  const void *depth, *color;
  int depth_elem, color_elem, channels;
  RgConvert cv;
};

enum { kGaussDepth = 0, kGaussColor = 1, kGaussStep = 2 };

// pixel (x, y), already clamped, of frame f of what the Gaussian kernel reads in `mode`
PG_HD float rg_source(const RgRaw& raw, const float* src, int mode, int64_t f, int H, int W, int x, int y) {
  const int64_t i = (f * H + y) * W + x;
  if (mode == kGaussDepth) return rg_depth(raw.depth, raw.depth_elem, i, raw.cv);
  if (mode == kGaussColor) return rg_intensity(raw.color, raw.color_elem, raw.channels, i);
  return src[(int64_t)y * W + x];
}

// mode kGaussDepth / kGaussColor: level 0 of image kRgD / kRgI from the raw images.  kGaussStep: intensity level l + 1 from level l.
__global__ __launch_bounds__(kRgbdThreads) void rgbd_gauss_kernel(RgPyramid py, RgRaw raw, int mode, int l) {
  __shared__ float in[kTileH + 2][kTileW + 2];
  __shared__ float hp[kTileH + 2][kTileW];
  __shared__ float g[kTileH][kTileW];
  const int64_t f = blockIdx.y;
  const int H = py.H[l], W = py.W[l];
  const int tx = (W + kTileW - 1) / kTileW;
  const int x0 = (blockIdx.x % tx) * kTileW, y0 = (blockIdx.x / tx) * kTileH;
  const float* src = mode == kGaussStep ? rg_image(py, kRgI, f, l) : nullptr;
  for (int i = threadIdx.x; i < (kTileH + 2) * (kTileW + 2); i += kRgbdThreads) {
    const int r = i / (kTileW + 2), c = i % (kTileW + 2);
    in[r][c] = rg_source(raw, src, mode, f, H, W, rg_clamp(x0 - 1 + c, W), rg_clamp(y0 - 1 + r, H));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (kTileH + 2) * kTileW; i += kRgbdThreads) {
    const int r = i / kTileW, c = i % kTileW;
    hp[r][c] = rg_blur3(in[r][c], in[r][c + 1], in[r][c + 2]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTileH * kTileW; i += kRgbdThreads) {
    const int r = i / kTileW, c = i % kTileW;
    const float v = rg_blur3(hp[r][c], hp[r + 1][c], hp[r + 2][c]);
    if (mode == kGaussStep) {
      g[r][c] = v;
    } else if (x0 + c < W && y0 + r < H) {
      rg_image(py, mode == kGaussDepth ? kRgD : kRgI, f, 0)[(int64_t)(y0 + r) * W + x0 + c] = v;
    }
  }
  if (mode != kGaussStep) return;                                       // (uniform over the workgroup)
  __syncthreads();
  const int Hn = py.H[l + 1], Wn = py.W[l + 1];
  if (threadIdx.x < (kTileH / 2) * (kTileW / 2)) {
    const int c = threadIdx.x % (kTileW / 2), r = threadIdx.x / (kTileW / 2);
    const int x = x0 / 2 + c, y = y0 / 2 + r;
    if (x < Wn && y < Hn)
      rg_image(py, kRgI, f, l + 1)[(int64_t)y * Wn + x] = rg_mean4(g[2 * r][2 * c], g[2 * r][2 * c + 1], g[2 * r + 1][2 * c], g[2 * r + 1][2 * c + 1]);
  }
}

// depth level l + 1 from level l
__global__ __launch_bounds__(kRgbdThreads) void rgbd_down_kernel(RgPyramid py, int l) {
  const int64_t f = blockIdx.y;
  const int W = py.W[l], Hn = py.H[l + 1], Wn = py.W[l + 1];
  const int64_t i = (int64_t)blockIdx.x * kRgbdThreads + threadIdx.x;
  if (i >= (int64_t)Hn * Wn) return;
  const int x = (int)(i % Wn), y = (int)(i / Wn);
  const float* src = rg_image(py, kRgD, f, l) + (int64_t)(2 * y) * W + 2 * x;
  rg_image(py, kRgD, f, l + 1)[i] = rg_mean4(src[0], src[1], src[W], src[W + 1]);
}

// the Sobel images of image `blockIdx.z` (kRgI or kRgD) at level l of every target frame
__global__ __launch_bounds__(kRgbdThreads) void rgbd_sobel_kernel(RgPyramid py, const uint8_t* __restrict__ target, int l) {
  __shared__ float in[kTileH + 2][kTileW + 2];
  __shared__ float e[kTileH + 2][kTileW];
  __shared__ float s[kTileH + 2][kTileW];
  const int64_t f = blockIdx.y;
  if (!target[f]) return;                                               // (uniform over the workgroup)
  const int kind = blockIdx.z;
  const int H = py.H[l], W = py.W[l];
  const int tx = (W + kTileW - 1) / kTileW;
  const int x0 = (blockIdx.x % tx) * kTileW, y0 = (blockIdx.x / tx) * kTileH;
  const float* src = rg_image(py, kind, f, l);
  for (int i = threadIdx.x; i < (kTileH + 2) * (kTileW + 2); i += kRgbdThreads) {
    const int r = i / (kTileW + 2), c = i % (kTileW + 2);
    in[r][c] = src[(int64_t)rg_clamp(y0 - 1 + r, H) * W + rg_clamp(x0 - 1 + c, W)];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (kTileH + 2) * kTileW; i += kRgbdThreads) {
    const int r = i / kTileW, c = i % kTileW;
    e[r][c] = rg_sobel_diff(in[r][c], in[r][c + 2]);
    s[r][c] = rg_sobel_smooth(in[r][c], in[r][c + 1], in[r][c + 2]);
  }
  __syncthreads();
  float* dx = rg_image(py, kind == kRgI ? kRgIx : kRgDx, f, l);
  float* dy = rg_image(py, kind == kRgI ? kRgIy : kRgDy, f, l);
  for (int i = threadIdx.x; i < kTileH * kTileW; i += kRgbdThreads) {
    const int r = i / kTileW, c = i % kTileW;
    if (x0 + c >= W || y0 + r >= H) continue;
    const int64_t at = (int64_t)(y0 + r) * W + x0 + c;
    dx[at] = rg_sobel_smooth(e[r][c], e[r + 1][c], e[r + 2][c]);
    dy[at] = rg_sobel_diff(s[r][c], s[r + 2][c]);
  }
}

// what the pair kernels share: the pyramids, the pairs, the running state and the results, the map and the partials
struct RgCall {
  RgPyramid py;
  RgPairs pairs;
  double *T, *scale, *information, *partials;
  int *status, *done;
  int64_t* count;
  uint8_t* success;
  uint64_t* map;            // (P, H W) of level 0; level l uses the first H_l W_l entries of a pair's row
  int64_t map_stride;       // H W of level 0
  int max_chunks;           // chunks of level 0: the stride of a pair's partials
  int method;
  double max_depth_diff;
};

PG_HD RgState rg_state(const RgCall& c, int p) {
  RgState st;
  st.T = c.T + 16 * p, st.scale = c.scale + 2 * p, st.status = c.status + p, st.done = c.done + p;
  st.information = c.information + 36 * p, st.count = c.count + p, st.success = c.success + p;
  return st;
}

__global__ void rgbd_init_kernel(RgCall c, const double* __restrict__ T0, int P) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < P) rg_pair_init(rg_state(c, p), T0 + 16 * p, c.pairs.K[p]);
}

__global__ __launch_bounds__(kRgbdThreads) void rgbd_claim_kernel(RgCall c, int l) {
  __shared__ double cam[12];
  const int p = blockIdx.y;
  if (c.done[p]) return;                                                // (uniform over the workgroup)
  const RgLevel v = rg_level(c.py, c.pairs, p, l);
  if (threadIdx.x == 0) rg_camera(v.K, c.T + 16 * p, cam);
  __syncthreads();
  const int64_t s = (int64_t)blockIdx.x * kRgbdThreads + threadIdx.x;
  if (s >= (int64_t)v.H * v.W) return;
  int j;
  uint64_t key;
  if (rg_claim(v, cam, (int)s, c.max_depth_diff, &j, &key)) atomicMin((unsigned long long*)(c.map + p * c.map_stride + j), (unsigned long long)key);
}

__global__ __launch_bounds__(kRgbdThreads) void rgbd_sums_kernel(RgCall c, int l, int what) {
  __shared__ double sh[kRgbdSums * kIcpLanes];
  const int p = blockIdx.y, chunk = blockIdx.x;
  if (c.done[p]) return;                                                // (uniform over the workgroup)
  const RgLevel v = rg_level(c.py, c.pairs, p, l);
  double out[kRgbdSums];
  rg_chunk_sums(v, c.T + 16 * p, c.scale + 2 * p, c.method, what, c.map + p * c.map_stride, chunk, (int)threadIdx.x, (int)threadIdx.x + 1, sh,
                [] { __syncthreads(); }, out);
  if (threadIdx.x == 0)
    for (int k = 0; k < kRgbdSums; k++) c.partials[((int64_t)p * c.max_chunks + chunk) * kRgbdSums + k] = out[k];
}

__global__ __launch_bounds__(kRgbdThreads) void rgbd_finish_kernel(RgCall c, int what, int chunks) {
  __shared__ double sh[kRgbdSums * kIcpLanes];
  const int p = blockIdx.x;
  rg_pair_finish(rg_state(c, p), what, c.partials + (int64_t)p * c.max_chunks * kRgbdSums, chunks, (int)threadIdx.x, (int)threadIdx.x + 1, sh,
                 [] { __syncthreads(); }, nullptr);
}

int rg_chunks(int H, int W) { return (int)se3_cdiv((int64_t)H * W, kRgbdChunk); }

bool rgbd_args(const char* what, int depth_elem, int color_elem, int channels, int64_t F, int H, int W, int P, const int* pairs,
               const double* K, int method, const int* iterations, int levels, double depth_scale, double depth_trunc, double min_depth,
               double max_depth, double max_depth_diff) {
  if ((depth_elem != 0 && depth_elem != 1) || (color_elem != 1 && color_elem != 2) || (channels != 1 && channels != 3))
    return se3_set_error("%s: depth_elem %d, color_elem %d, %d channels", what, depth_elem, color_elem, channels), false;
  if (F < 0 || F >= (1ll << 31) || P < 0 || P > kPairMaxPairs)
    return se3_set_error("%s: %lld frames, %d pairs (at most %d per call)", what, (long long)F, P, kPairMaxPairs), false;
  if (levels < 1 || levels > kRgbdMaxLevels) return se3_set_error("%s: %d pyramid levels not in [1, %d]", what, levels, kRgbdMaxLevels), false;
  if (H < 1 || W < 1 || H > kRgbdMaxImage || W > kRgbdMaxImage || (H >> (levels - 1)) < kRgbdMinSide || (W >> (levels - 1)) < kRgbdMinSide)
    return se3_set_error("%s: images of %d x %d with %d levels (each side at most %d, and at least %d at the coarsest level)", what, H, W, levels,
                         kRgbdMaxImage, kRgbdMinSide),
           false;
  if (method != kRgbdHybrid && method != kRgbdColor) return se3_set_error("%s: method %d", what, method), false;
  if (!iterations || (P > 0 && (!pairs || !K))) return se3_set_error("%s: null pointer", what), false;
  for (int l = 0; l < levels; l++)
    if (iterations[l] < 0 || iterations[l] > SE3_RGBD_MAX_ITERATIONS)
      return se3_set_error("%s: %d iterations at a level (in [0, %d])", what, iterations[l], SE3_RGBD_MAX_ITERATIONS), false;
  for (int p = 0; p < P; p++) {
    if (pairs[2 * p] < 0 || pairs[2 * p] >= F || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= F)
      return se3_set_error("%s: pair %d names frames (%d, %d) of %lld", what, p, pairs[2 * p], pairs[2 * p + 1], (long long)F), false;
    if (!(K[4 * p] > 0.0 && K[4 * p + 1] > 0.0 && isfinite(K[4 * p]) && isfinite(K[4 * p + 1]) && isfinite(K[4 * p + 2]) && isfinite(K[4 * p + 3])))
      return se3_set_error("%s: the intrinsics of pair %d are not finite with positive focal lengths", what, p), false;
  }
  if (!(isfinite(depth_scale) && depth_scale > 0.0 && isfinite(depth_trunc) && depth_trunc > 0.0))
    return se3_set_error("%s: depth_scale %g and depth_trunc %g must be positive and finite", what, depth_scale, depth_trunc), false;
  if (!(isfinite(min_depth) && min_depth >= 0.0 && isfinite(max_depth) && max_depth > min_depth && isfinite(max_depth_diff) && max_depth_diff >= 0.0))
    return se3_set_error("%s: 0 <= min_depth %g < max_depth %g and max_depth_diff %g >= 0 must be finite", what, min_depth, max_depth,
                         max_depth_diff),
           false;
  return true;
}

RgPairs rg_pairs(const int* pairs, const double* K, int P) {
  RgPairs out = {};
  for (int p = 0; p < P; p++) {
    out.src[p] = pairs[2 * p], out.tgt[p] = pairs[2 * p + 1];
    for (int k = 0; k < 4; k++) out.K[p][k] = K[4 * p + k];
  }
  return out;
}

size_t rg_align(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t se3_rgbd_frames_workspace_bytes(int64_t num_frames, int height, int width, int num_levels) {
  if (num_frames < 0 || height < 1 || width < 1 || height > kRgbdMaxImage || width > kRgbdMaxImage || num_levels < 1 || num_levels > kRgbdMaxLevels)
    return 0;
  const RgPyramid py = rg_pyramid(nullptr, num_frames, height, width, num_levels);
  return rg_align((size_t)kRgbdImages * (size_t)num_frames * (size_t)py.S * sizeof(float)) + 256;
}

extern "C" size_t se3_rgbd_pairs_workspace_bytes(int num_pairs, int height, int width) {
  if (num_pairs < 0 || num_pairs > kPairMaxPairs || height < 1 || width < 1 || height > kRgbdMaxImage || width > kRgbdMaxImage) return 0;
  const size_t P = (size_t)num_pairs;
  return rg_align(P * (size_t)height * width * sizeof(uint64_t)) + rg_align(P * rg_chunks(height, width) * kRgbdSums * sizeof(double)) +
         rg_align(P * 2 * sizeof(double)) + rg_align(P * sizeof(int)) + 256;
}

extern "C" int se3_rgbd_odometry_stack(const void* depths, int depth_elem, const void* colors, int color_elem, int color_channels,
                                       int64_t num_frames, int height, int width, const uint8_t* target_flags, int prepare,
                                       const int* pairs_host, const double* intrinsics_host, int num_pairs, const double* init_transforms,
                                       int method, const int* iterations_host, int num_levels, double depth_scale, double depth_trunc,
                                       double min_depth, double max_depth, double max_depth_diff, double* out_transforms,
                                       uint8_t* out_success, int* out_status, double* out_information, int64_t* out_count,
                                       void* frames_workspace, size_t frames_workspace_bytes, void* pairs_workspace,
                                       size_t pairs_workspace_bytes, void* stream) {
  const char* what = "rgbd_odometry_stack";
  if (!rgbd_args(what, depth_elem, color_elem, color_channels, num_frames, height, width, num_pairs, pairs_host, intrinsics_host, method,
                 iterations_host, num_levels, depth_scale, depth_trunc, min_depth, max_depth, max_depth_diff))
    return SE3_ERR_INVALID_ARG;
  const int P = num_pairs, H = height, W = width;
  const int64_t F = num_frames;
  if (F == 0) return SE3_OK;
  SE3_REQUIRE(frames_workspace && frames_workspace_bytes >= se3_rgbd_frames_workspace_bytes(F, H, W, num_levels), SE3_ERR_WORKSPACE,
              "%s: the frames' workspace is too small", what);
  SE3_REQUIRE(!prepare || (depths && colors && target_flags), SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  hipStream_t st = (hipStream_t)stream;
  RgCall c = {};
  c.py = rg_pyramid((float*)(((uintptr_t)frames_workspace + 255) & ~(uintptr_t)255), F, H, W, num_levels);
  if (prepare) {
    RgRaw raw = {depths, colors, depth_elem, color_elem, color_channels, rg_convert(depth_scale, depth_trunc, min_depth, max_depth)};
    for (int mode = kGaussDepth; mode <= kGaussColor; mode++)
      rgbd_gauss_kernel<<<dim3((unsigned)(se3_cdiv(W, kTileW) * se3_cdiv(H, kTileH)), (unsigned)F), kRgbdThreads, 0, st>>>(c.py, raw, mode, 0);
    for (int l = 0; l + 1 < num_levels; l++) {
      rgbd_gauss_kernel<<<dim3((unsigned)(se3_cdiv(c.py.W[l], kTileW) * se3_cdiv(c.py.H[l], kTileH)), (unsigned)F), kRgbdThreads, 0, st>>>(
          c.py, raw, kGaussStep, l);
      rgbd_down_kernel<<<dim3((unsigned)se3_cdiv((int64_t)c.py.H[l + 1] * c.py.W[l + 1], kRgbdThreads), (unsigned)F), kRgbdThreads, 0, st>>>(c.py, l);
    }
    for (int l = 0; l < num_levels; l++)
      rgbd_sobel_kernel<<<dim3((unsigned)(se3_cdiv(c.py.W[l], kTileW) * se3_cdiv(c.py.H[l], kTileH)), (unsigned)F, 2), kRgbdThreads, 0, st>>>(
          c.py, target_flags, l);
    SE3_CHECK_LAUNCH(what);
  }
  if (P == 0) return SE3_OK;
  SE3_REQUIRE(init_transforms && out_transforms && out_success && out_status && out_information && out_count, SE3_ERR_INVALID_ARG,
              "%s: null pointer", what);
  SE3_REQUIRE(pairs_workspace && pairs_workspace_bytes >= se3_rgbd_pairs_workspace_bytes(P, H, W), SE3_ERR_WORKSPACE,
              "%s: the pairs' workspace is too small", what);
  c.pairs = rg_pairs(pairs_host, intrinsics_host, P);
  c.map_stride = (int64_t)H * W, c.max_chunks = rg_chunks(H, W), c.method = method, c.max_depth_diff = max_depth_diff;
  char* at = (char*)(((uintptr_t)pairs_workspace + 255) & ~(uintptr_t)255);
  const size_t map_bytes = (size_t)P * H * W * sizeof(uint64_t);
  c.map = (uint64_t*)at, at += rg_align(map_bytes);
  c.partials = (double*)at, at += rg_align((size_t)P * c.max_chunks * kRgbdSums * sizeof(double));
  c.scale = (double*)at, at += rg_align((size_t)P * 2 * sizeof(double));
  c.done = (int*)at;
  c.T = out_transforms, c.status = out_status, c.information = out_information, c.count = out_count, c.success = out_success;
  rgbd_init_kernel<<<1, kPairMaxPairs, 0, st>>>(c, init_transforms, P);
  if (hipMemsetAsync(c.map, 0xff, map_bytes, st) != hipSuccess) return se3_set_error("%s: clearing the map failed", what), SE3_ERR_LAUNCH;
  auto pass = [&](int l, int sums) {
    const int chunks = rg_chunks(c.py.H[l], c.py.W[l]);
    rgbd_claim_kernel<<<dim3((unsigned)se3_cdiv((int64_t)c.py.H[l] * c.py.W[l], kRgbdThreads), (unsigned)P), kRgbdThreads, 0, st>>>(c, l);
    rgbd_sums_kernel<<<dim3((unsigned)chunks, (unsigned)P), kRgbdThreads, 0, st>>>(c, l, sums);
    rgbd_finish_kernel<<<(unsigned)P, kRgbdThreads, 0, st>>>(c, sums, chunks);
  };
  pass(0, kRgbdSumNorm);
  for (int l = num_levels - 1; l >= 0; l--)
    for (int it = 0; it < iterations_host[num_levels - 1 - l]; it++) pass(l, kRgbdSumStep);
  pass(0, kRgbdSumInfo);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

// ---- the same text on host memory, no GPU, serially (tests/test_rgbd_odometry_cpu.py) -------------------------------------------------------
namespace {

void rg_host_prepare(const RgPyramid& py, const RgRaw& raw, const uint8_t* target) {
  std::vector<float> hp, g;
  for (int64_t f = 0; f < py.F; f++) {
    for (int l = 0; l < py.levels; l++) {
      const int H = py.H[l], W = py.W[l];
      hp.assign((size_t)H * W, 0.0f), g.assign((size_t)H * W, 0.0f);
      // Gaussian3 of: the raw depth and the raw colour at level 0 (the results are level 0), the intensity of level l for the step to l + 1
      for (int mode = l == 0 ? kGaussDepth : kGaussStep; mode <= kGaussStep; mode++) {
        if (mode == kGaussStep && l + 1 >= py.levels) break;
        const float* src = mode == kGaussStep ? rg_image(py, kRgI, f, l) : nullptr;
        for (int y = 0; y < H; y++)
          for (int x = 0; x < W; x++)
            hp[(size_t)y * W + x] = rg_blur3(rg_source(raw, src, mode, f, H, W, rg_clamp(x - 1, W), y), rg_source(raw, src, mode, f, H, W, x, y),
                                             rg_source(raw, src, mode, f, H, W, rg_clamp(x + 1, W), y));
        float* out = mode == kGaussStep ? g.data() : rg_image(py, mode == kGaussDepth ? kRgD : kRgI, f, 0);
        for (int y = 0; y < H; y++)
          for (int x = 0; x < W; x++)
            out[(size_t)y * W + x] = rg_blur3(hp[(size_t)rg_clamp(y - 1, H) * W + x], hp[(size_t)y * W + x], hp[(size_t)rg_clamp(y + 1, H) * W + x]);
      }
      if (l + 1 < py.levels) {
        const int Hn = py.H[l + 1], Wn = py.W[l + 1];
        const float* d = rg_image(py, kRgD, f, l);
        for (int y = 0; y < Hn; y++)
          for (int x = 0; x < Wn; x++) {
            const size_t a = (size_t)(2 * y) * W + 2 * x;
            rg_image(py, kRgI, f, l + 1)[(size_t)y * Wn + x] = rg_mean4(g[a], g[a + 1], g[a + W], g[a + W + 1]);
            rg_image(py, kRgD, f, l + 1)[(size_t)y * Wn + x] = rg_mean4(d[a], d[a + 1], d[a + W], d[a + W + 1]);
          }
      }
    }
    if (!target[f]) continue;
    for (int l = 0; l < py.levels; l++)
      for (int kind = kRgI; kind <= kRgD; kind++) {
        const int H = py.H[l], W = py.W[l];
        const float* in = rg_image(py, kind, f, l);
        float *dx = rg_image(py, kind == kRgI ? kRgIx : kRgDx, f, l), *dy = rg_image(py, kind == kRgI ? kRgIy : kRgDy, f, l);
        auto e = [&](int x, int y) { return rg_sobel_diff(in[(size_t)y * W + rg_clamp(x - 1, W)], in[(size_t)y * W + rg_clamp(x + 1, W)]); };
        auto s = [&](int x, int y) {
          return rg_sobel_smooth(in[(size_t)y * W + rg_clamp(x - 1, W)], in[(size_t)y * W + x], in[(size_t)y * W + rg_clamp(x + 1, W)]);
        };
        for (int y = 0; y < H; y++)
          for (int x = 0; x < W; x++) {
            const int ym = rg_clamp(y - 1, H), yp = rg_clamp(y + 1, H);
            dx[(size_t)y * W + x] = rg_sobel_smooth(e(x, ym), e(x, y), e(x, yp));
            dy[(size_t)y * W + x] = rg_sobel_diff(s(x, ym), s(x, yp));
          }
      }
  }
}

}  // namespace

extern "C" int se3_debug_rgbd_odometry_host(const void* depths, int depth_elem, const void* colors, int color_elem, int color_channels,
                                            int64_t num_frames, int height, int width, const uint8_t* target_flags, const int* pairs,
                                            const double* intrinsics, int num_pairs, const double* init_transforms, int method,
                                            const int* iterations, int num_levels, double depth_scale, double depth_trunc, double min_depth,
                                            double max_depth, double max_depth_diff, int stop, int stop_level, double* out_transforms,
                                            uint8_t* out_success, int* out_status, double* out_information, int64_t* out_count,
                                            float* out_pyramids, uint64_t* out_map, double* out_sums, double* out_scales) {
  const char* what = "debug_rgbd_odometry_host";
  if (!rgbd_args(what, depth_elem, color_elem, color_channels, num_frames, height, width, num_pairs, pairs, intrinsics, method, iterations,
                 num_levels, depth_scale, depth_trunc, min_depth, max_depth, max_depth_diff))
    return SE3_ERR_INVALID_ARG;
  SE3_REQUIRE(stop >= SE3_RGBD_STOP_NONE && stop <= SE3_RGBD_STOP_EVALUATED && stop_level >= 0 && stop_level < num_levels, SE3_ERR_INVALID_ARG,
              "%s: stop %d at level %d of %d", what, stop, stop_level, num_levels);
  const int P = num_pairs, H = height, W = width;
  const int64_t F = num_frames;
  SE3_REQUIRE(F == 0 || (depths && colors && target_flags), SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  RgPyramid py = rg_pyramid(nullptr, F, H, W, num_levels);
  std::vector<float> images((size_t)kRgbdImages * F * py.S, 0.0f);
  py.base = out_pyramids ? out_pyramids : images.data();
  const RgRaw raw = {depths, colors, depth_elem, color_elem, color_channels, rg_convert(depth_scale, depth_trunc, min_depth, max_depth)};
  rg_host_prepare(py, raw, target_flags);
  if (stop == SE3_RGBD_STOP_PREPARED || P == 0) return SE3_OK;
  SE3_REQUIRE(init_transforms && out_transforms && out_success && out_status && out_information && out_count, SE3_ERR_INVALID_ARG,
              "%s: null pointer", what);
  const RgPairs table = rg_pairs(pairs, intrinsics, P);
  const int max_chunks = rg_chunks(H, W);
  std::vector<uint64_t> map((size_t)H * W);
  std::vector<double> partials((size_t)max_chunks * kRgbdSums), sh((size_t)kRgbdSums * kIcpLanes);
  auto nothing = [] {};
  for (int p = 0; p < P; p++) {
    double scale[2];
    int done;
    RgState state = {out_transforms + 16 * p, scale, out_status + p, &done, out_information + 36 * p, out_count + p, out_success + p};
    rg_pair_init(state, init_transforms + 16 * p, table.K[p]);
    map.assign(map.size(), kRgbdFree);
    auto claim = [&](int l) {
      if (done) return;
      const RgLevel v = rg_level(py, table, p, l);
      double cam[12];
      rg_camera(v.K, state.T, cam);
      for (int s = 0; s < v.H * v.W; s++) {
        int j;
        uint64_t key;
        if (rg_claim(v, cam, s, max_depth_diff, &j, &key) && key < map[j]) map[j] = key;
      }
    };
    auto pass = [&](int l, int sums) {
      claim(l);
      const RgLevel v = rg_level(py, table, p, l);
      const int chunks = rg_chunks(v.H, v.W);
      if (!done)
        for (int chunk = 0; chunk < chunks; chunk++)
          rg_chunk_sums(v, state.T, scale, method, sums, map.data(), chunk, 0, kIcpLanes, sh.data(), nothing, partials.data() + (size_t)chunk * kRgbdSums);
      rg_pair_finish(state, sums, partials.data(), chunks, 0, kIcpLanes, sh.data(), nothing, out_sums ? out_sums + (size_t)kRgbdSums * p : nullptr);
    };
    if (stop == SE3_RGBD_STOP_CLAIMED) {
      claim(stop_level);
      if (out_map)
        for (size_t j = 0; j < map.size(); j++) out_map[(size_t)p * H * W + j] = map[j];
      continue;
    }
    pass(0, kRgbdSumNorm);
    if (stop == SE3_RGBD_STOP_EVALUATED) {
      pass(stop_level, kRgbdSumStep);
    } else {
      for (int l = num_levels - 1; l >= 0; l--)
        for (int it = 0; it < iterations[num_levels - 1 - l]; it++) pass(l, kRgbdSumStep);
      pass(0, kRgbdSumInfo);
    }
    if (out_scales) out_scales[2 * p] = scale[0], out_scales[2 * p + 1] = scale[1];
  }
  return SE3_OK;
}
