// TSDF fusion of depth frames into uniform volumes (Open3D's UniformTSDFVolume: integrate and extract_point_cloud) for up to
// SE3_PAIR_MAX_PAIRS volumes per call, and depth images as clouds (the reference's convert_depth_mat_to_points, Open3D's
// create_from_depth_image).  se3et_amd/tsdf.py carries the same contract; csrc/tsdf_core.h holds the text that the kernels and the
// se3_debug_tsdf_integrate_host / se3_debug_tsdf_extract_host / se3_debug_depth_points_host entries share.
// (SE3_EXACT_FP: the file is built with contraction off, and every contract function fences itself as well.  SE3_NO_SLP_VECTORIZE: the
// vectoriser packed the x and y chains of the projection into v_pk_*_f32 with an op_sel read of a fresh packed result, the shape that
// tests/test_isa_hazard.py keeps out of the library; the kernel is bound by its gathers, so it does without packed arithmetic.)
//
// State.  A volume is R^3 voxels of length vl with its corner at origin o (float64).  Voxel [x, y, z] (Open3D's IndexOf) sits at
// (x R + y) R + z: tsdf and weight (V, R, R, R) float32, zeros at the start, colour (V, 3, R, R, R) float32, planar, z fastest.
//
// Contract: integration.  All float32, every operation rounded on its own (no contraction; `/` and sqrtf rounded to nearest, hipcc's
// default).  A volume takes its frames in ascending order.  For voxel (x, y, z) and one frame with extrinsic E (world to camera, rounded
// to float32), intrinsics (fx, fy, cx, cy) as float32, an image of H x W:
//   1. World position: w_a = f32((vl / 2 + vl i_a) + o_a), evaluated in float64 with that one final rounding.
//   2. Camera position: c_a = ((E[a][0] w_x + E[a][1] w_y) + E[a][2] w_z) + E[a][3], evaluated directly for every voxel, never
//      incrementally along z.  The frame is skipped unless c_z > 0.
//   3. Pixel: u_f = ((c_x fx) / c_z + cx) + 0.5f, v_f likewise with fy, cy.  Skipped unless u_f >= 0.0001f, u_f < f32(W) - 0.0001f and the
//      same for v_f with H.  u = (int)u_f, v = (int)v_f.
//   4. Depth: d = f32(raw) / f32(depth_scale); d >= f32(depth_trunc) makes d = 0; skipped unless d > 0 (a NaN is skipped this way).
//   5. Signed distance: m = sqrtf((xr xr + yr yr) + 1) with xr = (f32(u) - cx) / fx, yr = (f32(v) - cy) / fy; sdf = (d - c_z) m; skipped
//      unless sdf > -trunc, trunc = f32(sdf_trunc).
//   6. Truncation: t = min(1, sdf (1f / trunc)).
//   7. Update: tsdf = (tsdf w + t) / (w + 1); each colour channel likewise with its pixel's value, a uint8 colour loaded as
//      f32(c) / 255f, a float32 colour as it is; then w = w + 1.
//
// Contract: extraction.  All float64.  Output order is ascending (x, y, z, axis), Open3D's loop order.
//   1. A voxel is usable iff w != 0, t < 0.98f and t >= -0.98f (float32 tests).
//   2. For x, y, z in [1, R - 1) and each axis i with idx_i + 1 < R - 1: a point is emitted when the voxel and its neighbour at idx + e_i
//      are both usable and their tsdf values f0, f1 are non-zero with opposite signs.
//   3. p0_a = vl / 2 + vl idx_a, p1_i = p0_i + vl, r0 = |f0|, r1 = |f1|, p_i = ((p0_i r1) + (p1_i r0)) / (r0 + r1), p_a = p0_a on the other
//      two axes.  The returned point is p + origin.  A colour channel is ((c0 r1) + (c1 r0)) / (r0 + r1).
//   4. Normal: n_i = T(p + h e_i) - T(p - h e_i), h = 0.99 vl, p without the origin.  T(q): g_a = q_a / vl - 0.5, i_a = floor(g_a),
//      r_a = g_a - i_a, s_a = 1 - r_a, f[dx][dy][dz] the stored tsdf of voxel (i_x + dx, i_y + dy, i_z + dz), and
//        T = s_x (s_y (s_z f000 + r_z f001) + r_y (s_z f010 + r_z f011)) + r_x (s_y (s_z f100 + r_z f101) + r_y (s_z f110 + r_z f111)),
//      every product and sum rounded on its own.  T reads the stored tsdf of every voxel, observed or not (an unobserved one holds 0:
//      Open3D's quirk).  n is divided by sqrt((n_x^2 + n_y^2) + n_z^2) (pg_sqrt) when that is positive and returned as it is otherwise.
//      The reads are inside the volume by construction: p_a lies between the centres of voxels idx_a and idx_a + 1 <= R - 2 with
//      idx_a >= 1, so p_a / vl - 0.5 is in [1, R - 2] and, h being 0.99 vl, g_a is in [0.01, R - 1.01]; float64 rounding moves g_a by
//      less than R 2^-50 <= 2^-40, so floor(g_a) is in [0, R - 2] and the far corner of the stencil is at most R - 1.
//
// Contract: depth images as clouds.  All float64, output in row-major pixel order.  z = raw / scaling_factor; z > distance_limit makes
// z = 0; x = ((u - cx) z) / fx, y = ((v - cy) z) / fy.
//   SE3_DEPTH_REFERENCE   the reference function, quirks included: v = (row W + u) / W, a true quotient, so the row is fractional; a pixel
//                         is kept iff raw > 0, so one beyond the limit stays as a (0, 0, 0) row.
//   SE3_DEPTH_OPEN3D      v = row; a pixel is kept iff raw > 0 and not z > distance_limit (create_from_depth_image, identity extrinsic).
//
// Departures from Open3D.  The surface test of extraction item 2 is a sign test, not the float product f0 f1 < 0 (which underflows to 0
// for two tiny values).  Colours are stored in [0, 1] (Open3D stores 0 .. 255 and divides on extraction).  Weights have no cap.  Depth
// is converted per gather, never as a float image; create_from_depth_image's float32 depth image is float64 arithmetic here.  With
// float32 depth the reference convention divides in float64 (numpy would divide a float32 array in float32).
//
// Determinism.  Every voxel is independent and there are no atomics: a volume's state and clouds are bit-identical alone, anywhere in a
// batch, from run to run, and whether its frames arrive in one call or split over several (the running average only ever sees a
// voxel's own frame sequence).
//
// Launches.
//   tsdf_integrate_kernel   one workgroup of 256 threads per tile of 64 z x 4 y voxels of one x and one volume: lanes run along z, so a
//                           wave reads and writes contiguous rows of the planes.  A thread keeps its voxel's tsdf, weight and colour in
//                           registers across all frames of the call; the volume is read once and written once, and only where a frame
//                           touched it.  The frame table (SE3_TSDF_FRAME_WORDS float32 a frame) passes through LDS in tiles of
//                           SE3_TSDF_FRAME_TILE frames and is read at one address per wave.  Depth and colour pixels are gathers,
//                           converted on load.  Voxel indices are 64-bit.  A volume without frames returns before it reads anything.
//   tsdf_count_kernel / tsdf_write_kernel   one workgroup of 256 threads per row (volume, x, y): the lanes take z in chunks of 256; the
//                           count pass sums the row's points, se3_exclusive_scan_i64 turns the counts into offsets, the write pass
//                           places every chunk's points with se3_block_exclusive, in (z, axis) order.
//   depth_count_kernel / depth_write_kernel   the same shape over the rows of the images.
#include <math.h>

#include <vector>

#include "common.h"
#include "tsdf_core.h"

namespace {

constexpr int kTsdfThreads = 256;
constexpr int kTsdfTileZ = 64, kTsdfTileY = kTsdfThreads / kTsdfTileZ;
static_assert(kTsdfMinResolution == SE3_TSDF_MIN_RESOLUTION && kTsdfMaxResolution == SE3_TSDF_MAX_RESOLUTION &&
                  kTsdfMaxImage == SE3_TSDF_MAX_IMAGE && kTsdfMaxTruncVoxels == SE3_TSDF_MAX_TRUNC_VOXELS &&
                  kTsdfFrameTile == SE3_TSDF_FRAME_TILE && kTsdfFrameWords == SE3_TSDF_FRAME_WORDS,
              "tsdf_core.h and include/se3et_hip.h name the same limits");
static_assert(kDepthReference == SE3_DEPTH_REFERENCE && kDepthOpen3d == SE3_DEPTH_OPEN3D, "and the same conventions");
static_assert(kTsdfTileZ == SE3_WAVE, "a wave is one row of z");

__global__ __launch_bounds__(kTsdfThreads) void tsdf_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                                      float* __restrict__ color, int R, double vl,
                                                                      const double* __restrict__ origins, TsImages im,
                                                                      const float* __restrict__ frames, PairRows frame_rows) {
  __shared__ float table[kTsdfFrameTile * kTsdfFrameWords];
  const int vol = blockIdx.y;
  const int64_t f0 = frame_rows.start[vol], f1 = frame_rows.start[vol + 1];
  if (f0 >= f1) return;                                                 // (uniform over the workgroup)
  const int zt = (R + kTsdfTileZ - 1) / kTsdfTileZ, yt = (R + kTsdfTileY - 1) / kTsdfTileY;
  const int zb = blockIdx.x % zt, yb = (blockIdx.x / zt) % yt, x = blockIdx.x / (zt * yt);
  const int z = zb * kTsdfTileZ + (threadIdx.x & (kTsdfTileZ - 1)), y = yb * kTsdfTileY + (threadIdx.x >> 6);
  const bool inside = x < R && y < R && z < R;                          // (no early return: every thread meets the barriers)
  const int64_t cube = (int64_t)R * R * R, at = (int64_t)vol * cube + ts_index(R, x, y, z), cat = (int64_t)vol * 3 * cube + ts_index(R, x, y, z);
  float t = 0.0f, w = 0.0f, c[3] = {0.0f, 0.0f, 0.0f}, wx = 0.0f, wy = 0.0f, wz = 0.0f;
  if (inside) {
    t = tsdf[at], w = weight[at];
    if (color)
      for (int k = 0; k < 3; k++) c[k] = color[cat + k * cube];
    wx = ts_world(vl, x, origins[3 * vol]), wy = ts_world(vl, y, origins[3 * vol + 1]), wz = ts_world(vl, z, origins[3 * vol + 2]);
  }
  bool touched = false;
  for (int64_t base = f0; base < f1; base += kTsdfFrameTile) {
    const int m = (int)(f1 - base < kTsdfFrameTile ? f1 - base : kTsdfFrameTile);
    __syncthreads();
    for (int i = threadIdx.x; i < m * kTsdfFrameWords; i += kTsdfThreads) table[i] = frames[base * kTsdfFrameWords + i];
    __syncthreads();
    if (inside)
      for (int i = 0; i < m; i++) touched |= ts_integrate(table + i * kTsdfFrameWords, im, base + i, wx, wy, wz, &t, &w, c);
  }
  if (touched) {
    tsdf[at] = t, weight[at] = w;
    if (color)
      for (int k = 0; k < 3; k++) color[cat + k * cube] = c[k];
  }
}

PG_HD TsVolume ts_volume(const float* tsdf, const float* weight, const float* color, int vol, int R, double vl, const double* origins) {
  const int64_t cube = (int64_t)R * R * R;
  TsVolume V;
  V.tsdf = tsdf + vol * cube, V.weight = weight + vol * cube, V.color = color ? color + vol * 3 * cube : nullptr;
  V.R = R, V.vl = vl;
  for (int a = 0; a < 3; a++) V.origin[a] = origins ? origins[3 * vol + a] : 0.0;
  return V;
}

PG_HD int ts_popcount3(int mask) { return (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1); }

// counts[row] = the points of row (vol, x, y), row = (vol R + x) R + y
__global__ __launch_bounds__(kTsdfThreads) void tsdf_count_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, int R,
                                                                  int64_t* __restrict__ counts) {
  __shared__ int sh[kTsdfThreads];
  const int64_t row = blockIdx.x;
  const int y = (int)(row % R), x = (int)((row / R) % R), vol = (int)(row / ((int64_t)R * R));
  const TsVolume V = ts_volume(tsdf, weight, nullptr, vol, R, 0.0, nullptr);
  int n = 0, total;
  for (int z = threadIdx.x; z < R; z += kTsdfThreads) n += ts_popcount3(ts_edges(V, x, y, z));
  se3_block_exclusive<int, kTsdfThreads>(n, sh, &total);
  if (threadIdx.x == 0) counts[row] = total;
}

__global__ __launch_bounds__(kTsdfThreads) void tsdf_write_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                  const float* __restrict__ color, int R, double vl,
                                                                  const double* __restrict__ origins, const int64_t* __restrict__ offsets,
                                                                  int64_t capacity, double* __restrict__ out_points,
                                                                  double* __restrict__ out_normals, double* __restrict__ out_colors) {
  __shared__ int sh[kTsdfThreads];
  const int64_t row = blockIdx.x;
  if (offsets[row + 1] == offsets[row]) return;                         // (uniform over the workgroup)
  const int y = (int)(row % R), x = (int)((row / R) % R), vol = (int)(row / ((int64_t)R * R));
  const TsVolume V = ts_volume(tsdf, weight, color, vol, R, vl, origins);
  int64_t base = offsets[row];
  for (int z0 = 0; z0 < R; z0 += kTsdfThreads) {
    const int z = z0 + threadIdx.x;
    const int mask = z < R ? ts_edges(V, x, y, z) : 0;
    int total;
    int64_t out = base + se3_block_exclusive<int, kTsdfThreads>(ts_popcount3(mask), sh, &total);
    for (int axis = 0; axis < 3; axis++) {
      if (!(mask >> axis & 1)) continue;
      double p[3], n[3], c[3];
      ts_emit(V, x, y, z, axis, p, n, c);
      if (out < capacity)
        for (int a = 0; a < 3; a++) {
          out_points[3 * out + a] = p[a], out_normals[3 * out + a] = n[a];
          if (color) out_colors[3 * out + a] = c[a];
        }
      out++;
    }
    base += total;
  }
}

// counts[row] = the kept pixels of row `row` of the stacked images (row = image H + v)
__global__ __launch_bounds__(kTsdfThreads) void depth_count_kernel(const void* __restrict__ depth, int elem, int W, double scaling, double limit,
                                                                   int convention, int64_t* __restrict__ counts) {
  __shared__ int sh[kTsdfThreads];
  const int64_t row = blockIdx.x;
  int n = 0, total;
  for (int u = threadIdx.x; u < W; u += kTsdfThreads) n += dp_keep(dp_raw(depth, elem, row * W + u), scaling, limit, convention) ? 1 : 0;
  se3_block_exclusive<int, kTsdfThreads>(n, sh, &total);
  if (threadIdx.x == 0) counts[row] = total;
}

__global__ __launch_bounds__(kTsdfThreads) void depth_write_kernel(const void* __restrict__ depth, int elem, int H, int W,
                                                                   const double* __restrict__ intrinsics, double scaling, double limit,
                                                                   int convention, const int64_t* __restrict__ offsets, int64_t capacity,
                                                                   double* __restrict__ out_points) {
  __shared__ int sh[kTsdfThreads];
  const int64_t row = blockIdx.x;
  if (offsets[row + 1] == offsets[row]) return;                         // (uniform over the workgroup)
  const int64_t image = row / H;
  const int v = (int)(row % H);
  int64_t base = offsets[row];
  for (int u0 = 0; u0 < W; u0 += kTsdfThreads) {
    const int u = u0 + threadIdx.x;
    const double raw = u < W ? dp_raw(depth, elem, row * W + u) : 0.0;
    const bool keep = u < W && dp_keep(raw, scaling, limit, convention);
    int total;
    const int64_t out = base + se3_block_exclusive<int, kTsdfThreads>(keep ? 1 : 0, sh, &total);
    if (keep && out < capacity) {
      double p[3];
      dp_point(raw, v, u, W, intrinsics + 4 * image, scaling, limit, convention, p);
      for (int a = 0; a < 3; a++) out_points[3 * out + a] = p[a];
    }
    base += total;
  }
}

bool tsdf_volume_args(const char* what, int R, double vl) {
  if (R < kTsdfMinResolution || R > kTsdfMaxResolution)
    return se3_set_error("%s: resolution %d not in [%d, %d]", what, R, kTsdfMinResolution, kTsdfMaxResolution), false;
  if (!(isfinite(vl) && vl > 0.0)) return se3_set_error("%s: voxel_length %g is not a positive finite number", what, vl), false;
  return true;
}

bool tsdf_integrate_args(const char* what, bool has_color, int R, double vl, double trunc, int depth_elem, const void* colors, int color_elem,
                         int H, int W, double depth_scale, double depth_trunc) {
  if (!tsdf_volume_args(what, R, vl)) return false;
  if (!(isfinite(trunc) && trunc > 0.0 && trunc <= kTsdfMaxTruncVoxels * vl && (float)trunc > 0.0f))
    return se3_set_error("%s: sdf_trunc %g not in (0, %d voxel lengths]", what, trunc, kTsdfMaxTruncVoxels), false;
  if (H < 1 || W < 1 || H > kTsdfMaxImage || W > kTsdfMaxImage)
    return se3_set_error("%s: images of %d x %d (each side in [1, %d])", what, H, W, kTsdfMaxImage), false;
  if ((depth_elem != 0 && depth_elem != 1) || color_elem < 0 || color_elem > 2 || (color_elem != 0) != (colors != nullptr) ||
      (color_elem != 0) != has_color)
    return se3_set_error("%s: depth_elem %d, color_elem %d: colours go with a volume that has colour, and only with one", what, depth_elem,
                         color_elem),
           false;
  if (!(isfinite(depth_scale) && depth_scale > 0.0 && isfinite(depth_trunc) && depth_trunc > 0.0))
    return se3_set_error("%s: depth_scale %g and depth_trunc %g must be positive and finite", what, depth_scale, depth_trunc), false;
  return true;
}

bool depth_points_args(const char* what, int elem, int H, int W, double scaling, double limit, int convention) {
  if ((elem != 0 && elem != 1) || (convention != kDepthReference && convention != kDepthOpen3d))
    return se3_set_error("%s: depth_elem %d, convention %d", what, elem, convention), false;
  if (H < 1 || W < 1 || H > kTsdfMaxImage || W > kTsdfMaxImage)
    return se3_set_error("%s: images of %d x %d (each side in [1, %d])", what, H, W, kTsdfMaxImage), false;
  if (!(isfinite(scaling) && scaling > 0.0) || isnan(limit))
    return se3_set_error("%s: scaling_factor %g must be positive and finite, distance_limit %g a number", what, scaling, limit), false;
  return true;
}

}  // namespace

extern "C" int se3_tsdf_integrate_stack(float* tsdf, float* weight, float* color, int num_volumes, int resolution, double voxel_length,
                                        double sdf_trunc, const double* origins, const void* depths, int depth_elem, const void* colors,
                                        int color_elem, int height, int width, const float* frames, const int64_t* frame_offsets_host,
                                        double depth_scale, double depth_trunc, void* stream) {
  const char* what = "tsdf_integrate_stack";
  SE3_REQUIRE(tsdf && weight && origins && frame_offsets_host, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(num_volumes >= 0 && num_volumes <= kPairMaxPairs, SE3_ERR_INVALID_ARG, "%s: %d volumes (at most %d)", what, num_volumes,
              kPairMaxPairs);
  if (!tsdf_integrate_args(what, color != nullptr, resolution, voxel_length, sdf_trunc, depth_elem, colors, color_elem, height, width,
                           depth_scale, depth_trunc))
    return SE3_ERR_INVALID_ARG;
  PairRows rows;
  SE3_REQUIRE(pg_fill_rows(&rows, frame_offsets_host, num_volumes), SE3_ERR_INVALID_ARG, "%s: frame offsets must start at 0 and not decrease",
              what);
  const int64_t F = rows.start[num_volumes];
  SE3_REQUIRE(F < (1ll << 31), SE3_ERR_UNSUPPORTED, "%s: %lld frames in one call (below 2^31)", what, (long long)F);
  if (num_volumes == 0 || F == 0) return SE3_OK;
  SE3_REQUIRE(depths && frames, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  const int R = resolution;
  const int64_t tiles = se3_cdiv(R, kTsdfTileZ) * se3_cdiv(R, kTsdfTileY) * R;
  const TsImages im = ts_images(depths, depth_elem, colors, color_elem, height, width, depth_scale, depth_trunc, sdf_trunc);
  tsdf_integrate_kernel<<<dim3((unsigned)tiles, (unsigned)num_volumes), kTsdfThreads, 0, (hipStream_t)stream>>>(
      tsdf, weight, color, R, voxel_length, origins, im, frames, rows);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" int se3_tsdf_extract_stack(const float* tsdf, const float* weight, const float* color, int num_volumes, int resolution,
                                      double voxel_length, const double* origins, int64_t* row_offsets, int64_t capacity, double* out_points,
                                      double* out_normals, double* out_colors, void* stream) {
  const char* what = "tsdf_extract_stack";
  SE3_REQUIRE(tsdf && weight && row_offsets, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(num_volumes >= 0 && num_volumes <= kPairMaxPairs, SE3_ERR_INVALID_ARG, "%s: %d volumes (at most %d)", what, num_volumes,
              kPairMaxPairs);
  if (!tsdf_volume_args(what, resolution, voxel_length)) return SE3_ERR_INVALID_ARG;
  const int R = resolution;
  const int64_t nrows = (int64_t)num_volumes * R * R;
  hipStream_t st = (hipStream_t)stream;
  if (!out_points) {
    if (nrows > 0) tsdf_count_kernel<<<(unsigned)nrows, kTsdfThreads, 0, st>>>(tsdf, weight, R, row_offsets);
    se3_exclusive_scan_i64(row_offsets, nrows, st);
  } else {
    SE3_REQUIRE(origins && out_normals && (out_colors != nullptr) == (color != nullptr) && capacity >= 0, SE3_ERR_INVALID_ARG,
                "%s: the write pass needs origins, normals and, exactly with colour, colours", what);
    if (nrows > 0 && capacity > 0)
      tsdf_write_kernel<<<(unsigned)nrows, kTsdfThreads, 0, st>>>(tsdf, weight, color, R, voxel_length, origins, row_offsets, capacity,
                                                                  out_points, out_normals, out_colors);
  }
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" int se3_depth_points_stack(const void* depths, int depth_elem, int64_t num_images, int height, int width, const double* intrinsics,
                                      double scaling_factor, double distance_limit, int convention, int64_t* row_offsets, int64_t capacity,
                                      double* out_points, void* stream) {
  const char* what = "depth_points_stack";
  SE3_REQUIRE(row_offsets && num_images >= 0, SE3_ERR_INVALID_ARG, "%s: null pointer or a negative image count", what);
  if (!depth_points_args(what, depth_elem, height, width, scaling_factor, distance_limit, convention)) return SE3_ERR_INVALID_ARG;
  const int64_t nrows = num_images * height;
  SE3_REQUIRE(nrows < (1ll << 31), SE3_ERR_UNSUPPORTED, "%s: %lld image rows in one call (below 2^31)", what, (long long)nrows);
  SE3_REQUIRE(nrows == 0 || depths, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  hipStream_t st = (hipStream_t)stream;
  if (!out_points) {
    if (nrows > 0)
      depth_count_kernel<<<(unsigned)nrows, kTsdfThreads, 0, st>>>(depths, depth_elem, width, scaling_factor, distance_limit, convention,
                                                                   row_offsets);
    se3_exclusive_scan_i64(row_offsets, nrows, st);
  } else {
    SE3_REQUIRE(intrinsics && capacity >= 0, SE3_ERR_INVALID_ARG, "%s: the write pass needs the intrinsics", what);
    if (nrows > 0 && capacity > 0)
      depth_write_kernel<<<(unsigned)nrows, kTsdfThreads, 0, st>>>(depths, depth_elem, height, width, intrinsics, scaling_factor,
                                                                   distance_limit, convention, row_offsets, capacity, out_points);
  }
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

// ---- the same text on host memory, one volume / one image, no GPU (tests/test_tsdf_cpu.py) --------------------------------------------------
extern "C" int se3_debug_tsdf_integrate_host(float* tsdf, float* weight, float* color, int resolution, double voxel_length, double sdf_trunc,
                                             const double* origin, const void* depths, int depth_elem, const void* colors, int color_elem,
                                             int64_t num_frames, int height, int width, const float* frames, double depth_scale,
                                             double depth_trunc) {
  const char* what = "debug_tsdf_integrate_host";
  SE3_REQUIRE(tsdf && weight && origin && num_frames >= 0 && (num_frames == 0 || (depths && frames)), SE3_ERR_INVALID_ARG,
              "%s: null pointer or a negative frame count", what);
  if (!tsdf_integrate_args(what, color != nullptr, resolution, voxel_length, sdf_trunc, depth_elem, colors, color_elem, height, width,
                           depth_scale, depth_trunc))
    return SE3_ERR_INVALID_ARG;
  const int R = resolution;
  const int64_t cube = (int64_t)R * R * R;
  const TsImages im = ts_images(depths, depth_elem, colors, color_elem, height, width, depth_scale, depth_trunc, sdf_trunc);
  for (int x = 0; x < R; x++)
    for (int y = 0; y < R; y++)
      for (int z = 0; z < R; z++) {
        const int64_t at = ts_index(R, x, y, z);
        float t = tsdf[at], w = weight[at], c[3] = {0.0f, 0.0f, 0.0f};
        if (color)
          for (int k = 0; k < 3; k++) c[k] = color[k * cube + at];
        const float wx = ts_world(voxel_length, x, origin[0]), wy = ts_world(voxel_length, y, origin[1]), wz = ts_world(voxel_length, z, origin[2]);
        bool touched = false;
        for (int64_t f = 0; f < num_frames; f++) touched |= ts_integrate(frames + f * kTsdfFrameWords, im, f, wx, wy, wz, &t, &w, c);
        if (!touched) continue;
        tsdf[at] = t, weight[at] = w;
        if (color)
          for (int k = 0; k < 3; k++) color[k * cube + at] = c[k];
      }
  return SE3_OK;
}

extern "C" int se3_debug_tsdf_extract_host(const float* tsdf, const float* weight, const float* color, int resolution, double voxel_length,
                                           const double* origin, int64_t capacity, double* out_points, double* out_normals, double* out_colors,
                                           int64_t* out_count) {
  const char* what = "debug_tsdf_extract_host";
  SE3_REQUIRE(tsdf && weight && origin && out_count, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(!out_points || (out_normals && (out_colors != nullptr) == (color != nullptr) && capacity >= 0), SE3_ERR_INVALID_ARG,
              "%s: points need normals and, exactly with colour, colours", what);
  if (!tsdf_volume_args(what, resolution, voxel_length)) return SE3_ERR_INVALID_ARG;
  const int R = resolution;
  const TsVolume V = ts_volume(tsdf, weight, color, 0, R, voxel_length, origin);
  int64_t n = 0;
  for (int x = 0; x < R; x++)
    for (int y = 0; y < R; y++)
      for (int z = 0; z < R; z++) {
        const int mask = ts_edges(V, x, y, z);
        for (int axis = 0; axis < 3; axis++) {
          if (!(mask >> axis & 1)) continue;
          if (out_points && n < capacity) {
            double c[3];
            ts_emit(V, x, y, z, axis, out_points + 3 * n, out_normals + 3 * n, color ? out_colors + 3 * n : c);
          }
          n++;
        }
      }
  *out_count = n;
  return SE3_OK;
}

extern "C" int se3_debug_depth_points_host(const void* depth, int depth_elem, int height, int width, const double* intrinsics,
                                           double scaling_factor, double distance_limit, int convention, int64_t capacity, double* out_points,
                                           int64_t* out_count) {
  const char* what = "debug_depth_points_host";
  SE3_REQUIRE(depth && intrinsics && out_count && capacity >= 0, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  if (!depth_points_args(what, depth_elem, height, width, scaling_factor, distance_limit, convention)) return SE3_ERR_INVALID_ARG;
  int64_t n = 0;
  for (int v = 0; v < height; v++)
    for (int u = 0; u < width; u++) {
      const double raw = dp_raw(depth, depth_elem, (int64_t)v * width + u);
      if (!dp_keep(raw, scaling_factor, distance_limit, convention)) continue;
      if (out_points && n < capacity) dp_point(raw, v, u, width, intrinsics, scaling_factor, distance_limit, convention, out_points + 3 * n);
      n++;
    }
  *out_count = n;
  return SE3_OK;
}
