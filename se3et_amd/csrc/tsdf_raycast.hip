// Ray casting of the uniform and the block-sparse TSDF volumes (Open3D's VoxelBlockGrid.ray_cast, KinectFusion's model rendering) for up to
// SE3_PAIR_MAX_PAIRS volumes per call: depth, point, normal, colour and hit maps of the fused model from any camera, one ray per lane, no
// atomics, nothing read back.  se3et_amd/tsdf.py and se3et_amd/tsdf_sparse.py carry the same contract; csrc/tsdf_raycast_core.h holds the
// per-ray text that the kernels and the se3_debug_tsdf_raycast_host / se3_debug_stsdf_raycast_host entries share, and T, ts_index and the
// normal are those of csrc/tsdf_core.h (ts_cell, ts_mix, ts_trilinear, ts_gradient: ts_emit computes what it computed, bit for bit).
// (SE3_EXACT_FP: the file is built with contraction off, and every contract function fences itself as well.)
//
// Contract.  All float64, every operation rounded on its own, unless said otherwise.  A view has an extrinsic E (world to camera), its
// inverse P computed on the host in float64 (camera_poses) and intrinsics (fx, fy, cx, cy); a volume has voxel length vl, sdf_trunc and
// an origin o (0 for a sparse volume).
//   1. Ray.  For pixel (u, v): xr = (u - cx) / fx, yr = (v - cy) / fy, dir_a = (P[a][0] xr + P[a][1] yr) + P[a][2], e_a = P[a][3] - o_a,
//      q_a(s) = e_a + s dir_a: s is camera depth.  m = sqrt((xr xr + yr yr) + 1) turns a Euclidean step into a step of s.
//   2. Interval, uniform volume.  Starting from [depth_min, depth_max], each axis intersects the interval with the ray's stay in the slab
//      [1.5 vl, (R - 1.5) vl], both ends computed once as 1.5 vl and (f64(R) - 1.5) vl: t = (end - e_a) / dir_a for both ends, the smaller
//      raises the lower end, the larger lowers the upper end.  An axis with dir_a == 0 divides nothing: it leaves the interval alone when
//      e_a lies in the slab and empties it otherwise.  An empty interval (not lo <= hi) is no hit.
//      A sample is read only where the three computed q_a themselves lie in the slab (a slab end that rounding moved by an ulp may not: it
//      is an unobserved sample).  For such a q, q_a / vl - 0.5 is in [1, R - 2] up to one rounding, so the nearest voxel floor(q_a / vl) is
//      in [1, R - 2], T's g_a is in [1 - 2^-50, R - 2 + R 2^-50] with floor in [0, R - 2] and a far corner of at most R - 1, and the
//      normal's g_a -+ 0.99 is in [0.01 - 2^-50, R - 1.01 + R 2^-50]: the same floors.  This is the argument of extraction item 4.
//      The refined s* lies in [s0, s1] (item 5), and q_a(s) is monotone in s as computed (a rounded product and a rounded sum are both
//      monotone), so q_a(s*) lies between q_a(s0) and q_a(s1), which were both tested: q(s*) is in the slab as well.
//   3. Interval, sparse volume: [depth_min, depth_max].  The global voxel index is i_a = floor(q_a / vl), tested as a float64 against
//      [-2^22, 2^22) before it becomes a 64-bit integer; the block is i_a >> 4, the local voxel i_a & 15.  A block coordinate outside the
//      key's range is an absent block.  T and the normal use g_a = q_a / vl - 0.5 in global coordinates and read their eight corners
//      through the directory; a corner in an absent block reads 0 (contract C, item 6).  A storage index is slot 4096 + a 12-bit local index
//      with the slot tested against the storage, so every read is inside it whatever the directory holds.
//   4. March.  s starts at the interval's lower end.  The sample at s is the nearest voxel's stored (f, w); it is observed iff
//      w >= f32(weight_threshold).  Observed: s advances by max(vl, f64(f) sdf_trunc) / m.  Unobserved: by vl / m.  Absent block: to the
//      ray's exit from the block, the smallest (face_a - e_a) / dir_a over the axes with dir_a != 0, face_a = L (b_a + 1) for dir_a > 0
//      and L b_a otherwise, b_a = floor(i_a / 16), and at least by vl / m; the sample counts as unobserved.  A crossing is an observed
//      sample with f <= 0 whose predecessor on the ray was observed with f > 0: a ray that starts on the negative side has no hit until
//      it has seen a positive observed sample, and no crossing is taken across an unobserved sample.  Marching ends at the first crossing
//      or when s > the upper end.  Every step advances s by vl / m at least, so a ray takes at most (hi - lo) / (vl / m) + 1 samples; the
//      loop counts them against that number + 1, which ends a ray whose s is so large that s + vl / m == s.  The calls refuse
//      (depth_max - depth_min) / vl > SE3_RAYCAST_MAX_STEPS.
//   5. Refinement.  At the crossing between s0 and s1: F0 = T(q(s0)), F1 = T(q(s1)), stored values, observed or not.  If F0 > 0 and
//      F1 <= 0 those are used, otherwise the two nearest-voxel values f64(f0), f64(f1).  s* = ((s1 F0) - (s0 F1)) / (F0 - F1), then
//      limited to [s0, s1], which only rounding can leave.
//   6. Outputs at s*.  depth = f32(s*); point = q(s*) + o; normal = extraction item 4 at q(s*) (h = 0.99 vl, divided by its length when
//      that is positive): it points to the positive side, towards the camera; a colour channel is T's sum over that colour plane's eight
//      corners with T's weights, rounded once to float32.  A pixel without a hit holds depth 0, a NaN point and normal, colour 0, mask 0.
//   7. Determinism.  No atomics, every pixel independent: a view is bit-identical alone, anywhere in a batch, across chunks, run to run.
//   8. Departures from Open3D.  No range map: every ray marches from depth_min.  The step is Euclidean (Open3D advances the ray parameter
//      by the sdf itself).  Refinement interpolates the trilinear field, not the two samples.  The uniform volume is cast inside its inner
//      box.  Observed is a threshold on the stored weight.  Colours are in [0, 1].
//
// Launch.  One kernel per volume type, a workgroup per tile of 16 x 16 pixels of one view, a lane per pixel: a wave is a quadrant of 8 x 8
// pixels, so its rays stay close in the volume and its gathers share L2 lines (16 x 4 pixels a wave measured 4 to 6 % slower).  The view's 16 words and the volume's constants are uniform over the
// workgroup (scalar loads).  The sparse directory lookup is a binary search over the keys behind a one-block cache per lane.  No LDS.
#include <math.h>

#include "common.h"
#include "tsdf_raycast_core.h"

namespace {

constexpr int kRaycastThreads = kRaycastTile * kRaycastTile;
static_assert(kRaycastTile == 16 && kRaycastThreads == 256, "rc_pixel cuts a tile of 16 x 16 into four waves of 8 x 8");
static_assert(kRaycastViewWords == SE3_RAYCAST_VIEW_WORDS && kRaycastTile == SE3_RAYCAST_TILE && kRaycastMaxSteps == SE3_RAYCAST_MAX_STEPS,
              "tsdf_raycast_core.h and include/se3et_hip.h name the same limits");

struct RcMaps {
  float* depth;
  double *points, *normals;
  float* colors;
  uint8_t* mask;
};

// the pixel of this lane, false outside the image; tile = the workgroup's index among the launch's tiles
__device__ __forceinline__ bool rc_pixel(int64_t tile, int H, int W, int64_t* view, int* u, int* v) {
  const int tx = (W + kRaycastTile - 1) / kRaycastTile, ty = (H + kRaycastTile - 1) / kRaycastTile;
  *view = tile / ((int64_t)tx * ty);
  const int in_view = (int)(tile % ((int64_t)tx * ty));
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;          // a wave is a quadrant of 8 x 8 pixels of the tile
  *u = (in_view % tx) * kRaycastTile + (wave & 1) * 8 + (lane & 7);
  *v = (in_view / tx) * kRaycastTile + (wave >> 1) * 8 + (lane >> 3);
  return *u < W && *v < H;
}

__global__ __launch_bounds__(kRaycastThreads) void tsdf_raycast_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                       const float* __restrict__ color, int num_volumes, int R, double vl,
                                                                       const double* __restrict__ origins, const double* __restrict__ views,
                                                                       const int* __restrict__ view_volumes, int64_t first_view, int H, int W,
                                                                       RcCall call, RcMaps out) {
  int64_t view;
  int u, v;
  if (!rc_pixel(blockIdx.x, H, W, &view, &u, &v)) return;
  view += first_view;
  const int64_t pixel = (view * H + v) * W + u;
  const int vol = view_volumes[view];
  RcHit hit;
  bool ok = false;
  if (vol >= 0 && vol < num_volumes) {                                  // (uniform over the workgroup)
    RcDense field = rc_dense(tsdf, weight, color, vol, R, vl, origins);
    const RcRay ray = rc_ray(views + view * kRaycastViewWords, field.V.origin, u, v);
    ok = rc_cast(field, ray, call, field.V.origin, out.normals != nullptr, out.colors != nullptr, &hit);
  }
  rc_store(ok, hit, pixel, out.depth, out.points, out.normals, out.colors, out.mask);
}

__global__ __launch_bounds__(kRaycastThreads) void stsdf_raycast_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                        const float* __restrict__ color, const int64_t* __restrict__ keys,
                                                                        const int* __restrict__ slots, int64_t num_blocks, int64_t num_slots,
                                                                        int num_volumes, double vl, const double* __restrict__ views,
                                                                        const int* __restrict__ view_volumes, int64_t first_view, int H, int W,
                                                                        RcCall call, RcMaps out) {
  int64_t view;
  int u, v;
  if (!rc_pixel(blockIdx.x, H, W, &view, &u, &v)) return;
  view += first_view;
  const int64_t pixel = (view * H + v) * W + u;
  const int vol = view_volumes[view];
  RcHit hit;
  bool ok = false;
  if (vol >= 0 && vol < num_volumes) {
    const double zero[3] = {0.0, 0.0, 0.0};
    RcSparse field = rc_sparse(tsdf, weight, color, keys, slots, num_blocks, num_slots, vol, vl);
    const RcRay ray = rc_ray(views + view * kRaycastViewWords, zero, u, v);
    ok = rc_cast(field, ray, call, zero, out.normals != nullptr, out.colors != nullptr, &hit);
  }
  rc_store(ok, hit, pixel, out.depth, out.points, out.normals, out.colors, out.mask);
}

// what both entries refuse; true: the call is fine
bool raycast_args(const char* what, double vl, double sdf_trunc, int64_t num_views, int H, int W, double depth_min, double depth_max,
                  double weight_threshold, const float* color, const float* out_colors) {
  if (!(isfinite(vl) && vl > 0.0)) return se3_set_error("%s: voxel_length %g is not a positive finite number", what, vl), false;
  if (!(isfinite(sdf_trunc) && sdf_trunc > 0.0)) return se3_set_error("%s: sdf_trunc %g is not a positive finite number", what, sdf_trunc), false;
  if (num_views < 0 || H < 1 || H > kTsdfMaxImage || W < 1 || W > kTsdfMaxImage)
    return se3_set_error("%s: %lld views of %d x %d: each side must lie in [1, %d]", what, (long long)num_views, H, W, kTsdfMaxImage), false;
  if (!(isfinite(depth_min) && isfinite(depth_max) && depth_min > 0.0 && depth_max > depth_min))
    return se3_set_error("%s: depth_min %g, depth_max %g: 0 < depth_min < depth_max expected", what, depth_min, depth_max), false;
  if (!((depth_max - depth_min) / vl <= (double)kRaycastMaxSteps))
    return se3_set_error("%s: (depth_max - depth_min) / voxel_length is %g (at most %d)", what, (depth_max - depth_min) / vl, kRaycastMaxSteps), false;
  if (isnan(weight_threshold)) return se3_set_error("%s: weight_threshold is not a number", what), false;
  if (out_colors && !color) return se3_set_error("%s: a colour map of a volume without colour", what), false;
  return true;
}

RcCall raycast_call(double depth_min, double depth_max, double sdf_trunc, double weight_threshold) {
  RcCall call;
  call.depth_min = depth_min, call.depth_max = depth_max, call.trunc = sdf_trunc, call.threshold = (float)weight_threshold;
  return call;
}

// the launches of one call: at most 2^31 - 1 tiles each
template <class Launch>
void raycast_launches(int64_t num_views, int H, int W, Launch launch) {
  const int64_t tiles = se3_cdiv(W, kRaycastTile) * se3_cdiv(H, kRaycastTile), per_launch = ((1ll << 31) - 1) / tiles;
  for (int64_t first = 0; first < num_views; first += per_launch) {
    const int64_t n = num_views - first < per_launch ? num_views - first : per_launch;
    launch(first, (unsigned)(n * tiles));
  }
}

template <class Field>
void raycast_host(Field& field, const double* origin, const double* views, int64_t num_views, int H, int W, const RcCall& call, const RcMaps& out) {
  for (int64_t view = 0; view < num_views; view++)
    for (int v = 0; v < H; v++)
      for (int u = 0; u < W; u++) {
        RcHit hit;
        const RcRay ray = rc_ray(views + view * kRaycastViewWords, origin, u, v);
        const bool ok = rc_cast(field, ray, call, origin, out.normals != nullptr, out.colors != nullptr, &hit);
        rc_store(ok, hit, (view * H + v) * W + u, out.depth, out.points, out.normals, out.colors, out.mask);
      }
}

}  // namespace

extern "C" int se3_tsdf_raycast_stack(const float* tsdf, const float* weight, const float* color, int num_volumes, int resolution,
                                      double voxel_length, double sdf_trunc, const double* origins, const double* views,
                                      const int* view_volumes, int64_t num_views, int height, int width, double depth_min, double depth_max,
                                      double weight_threshold, float* out_depth, double* out_points, double* out_normals, float* out_colors,
                                      uint8_t* out_mask, void* stream) {
  const char* what = "tsdf_raycast_stack";
  SE3_REQUIRE(num_volumes >= 0 && num_volumes <= kPairMaxPairs, SE3_ERR_INVALID_ARG, "%s: %d volumes (at most %d)", what, num_volumes,
              kPairMaxPairs);
  SE3_REQUIRE(resolution >= kTsdfMinResolution && resolution <= kTsdfMaxResolution, SE3_ERR_INVALID_ARG, "%s: resolution %d not in [%d, %d]", what,
              resolution, kTsdfMinResolution, kTsdfMaxResolution);
  if (!raycast_args(what, voxel_length, sdf_trunc, num_views, height, width, depth_min, depth_max, weight_threshold, color, out_colors))
    return SE3_ERR_INVALID_ARG;
  if (num_views == 0) return SE3_OK;
  SE3_REQUIRE(views && view_volumes && (num_volumes == 0 || (tsdf && weight && origins)), SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  const RcCall call = raycast_call(depth_min, depth_max, sdf_trunc, weight_threshold);
  const RcMaps out{out_depth, out_points, out_normals, out_colors, out_mask};
  raycast_launches(num_views, height, width, [&](int64_t first, unsigned tiles) {
    tsdf_raycast_kernel<<<tiles, kRaycastThreads, 0, (hipStream_t)stream>>>(tsdf, weight, color, num_volumes, resolution, voxel_length, origins, views,
                                                                           view_volumes, first, height, width, call, out);
  });
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" int se3_stsdf_raycast_stack(const float* tsdf, const float* weight, const float* color, const int64_t* keys, const int* slots,
                                       int64_t num_blocks, int64_t num_slots, int num_volumes, double voxel_length, double sdf_trunc,
                                       const double* views, const int* view_volumes, int64_t num_views, int height, int width,
                                       double depth_min, double depth_max, double weight_threshold, float* out_depth, double* out_points,
                                       double* out_normals, float* out_colors, uint8_t* out_mask, void* stream) {
  const char* what = "stsdf_raycast_stack";
  SE3_REQUIRE(num_volumes >= 0 && num_volumes <= kPairMaxPairs, SE3_ERR_INVALID_ARG, "%s: %d volumes (at most %d)", what, num_volumes,
              kPairMaxPairs);
  SE3_REQUIRE(num_blocks >= 0 && num_slots >= 0, SE3_ERR_INVALID_ARG, "%s: a negative block or slot count", what);
  if (!raycast_args(what, voxel_length, sdf_trunc, num_views, height, width, depth_min, depth_max, weight_threshold, color, out_colors))
    return SE3_ERR_INVALID_ARG;
  if (num_views == 0) return SE3_OK;
  SE3_REQUIRE(views && view_volumes && (num_blocks == 0 || (tsdf && weight && keys && slots)), SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  const RcCall call = raycast_call(depth_min, depth_max, sdf_trunc, weight_threshold);
  const RcMaps out{out_depth, out_points, out_normals, out_colors, out_mask};
  raycast_launches(num_views, height, width, [&](int64_t first, unsigned tiles) {
    stsdf_raycast_kernel<<<tiles, kRaycastThreads, 0, (hipStream_t)stream>>>(tsdf, weight, color, keys, slots, num_blocks, num_slots, num_volumes,
                                                                            voxel_length, views, view_volumes, first, height, width, call, out);
  });
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

// ---- the same text on host memory, serially, no GPU (tests/test_raycast_cpu.py): one volume, every pointer a host pointer -----------------------
extern "C" int se3_debug_tsdf_raycast_host(const float* tsdf, const float* weight, const float* color, int resolution, double voxel_length,
                                           double sdf_trunc, const double* origin, const double* views, int64_t num_views, int height,
                                           int width, double depth_min, double depth_max, double weight_threshold, float* out_depth,
                                           double* out_points, double* out_normals, float* out_colors, uint8_t* out_mask) {
  const char* what = "debug_tsdf_raycast_host";
  SE3_REQUIRE(tsdf && weight && origin && (views || num_views == 0), SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  SE3_REQUIRE(resolution >= kTsdfMinResolution && resolution <= kTsdfMaxResolution, SE3_ERR_INVALID_ARG, "%s: resolution %d not in [%d, %d]", what,
              resolution, kTsdfMinResolution, kTsdfMaxResolution);
  if (!raycast_args(what, voxel_length, sdf_trunc, num_views, height, width, depth_min, depth_max, weight_threshold, color, out_colors))
    return SE3_ERR_INVALID_ARG;
  RcDense field = rc_dense(tsdf, weight, color, 0, resolution, voxel_length, origin);
  raycast_host(field, field.V.origin, views, num_views, height, width, raycast_call(depth_min, depth_max, sdf_trunc, weight_threshold),
               RcMaps{out_depth, out_points, out_normals, out_colors, out_mask});
  return SE3_OK;
}

extern "C" int se3_debug_stsdf_raycast_host(const float* tsdf, const float* weight, const float* color, const int64_t* keys, const int* slots,
                                            int64_t num_blocks, int64_t num_slots, int volume, double voxel_length, double sdf_trunc,
                                            const double* views, int64_t num_views, int height, int width, double depth_min,
                                            double depth_max, double weight_threshold, float* out_depth, double* out_points,
                                            double* out_normals, float* out_colors, uint8_t* out_mask) {
  const char* what = "debug_stsdf_raycast_host";
  SE3_REQUIRE(num_blocks >= 0 && num_slots >= 0 && (num_blocks == 0 || (tsdf && weight && keys && slots)) && (views || num_views == 0),
              SE3_ERR_INVALID_ARG, "%s: null pointer or a negative count", what);
  SE3_REQUIRE(volume >= 0 && volume < kPairMaxPairs, SE3_ERR_INVALID_ARG, "%s: volume %d not in [0, %d)", what, volume, kPairMaxPairs);
  if (!raycast_args(what, voxel_length, sdf_trunc, num_views, height, width, depth_min, depth_max, weight_threshold, color, out_colors))
    return SE3_ERR_INVALID_ARG;
  const double zero[3] = {0.0, 0.0, 0.0};
  RcSparse field = rc_sparse(tsdf, weight, color, keys, slots, num_blocks, num_slots, volume, voxel_length);
  raycast_host(field, zero, views, num_views, height, width, raycast_call(depth_min, depth_max, sdf_trunc, weight_threshold),
               RcMaps{out_depth, out_points, out_normals, out_colors, out_mask});
  return SE3_OK;
}
