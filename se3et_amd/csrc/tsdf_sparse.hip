// Block-sparse TSDF volumes (Open3D's ScalableTSDFVolume: integrate and extract_point_cloud) for up to SE3_PAIR_MAX_PAIRS volumes per
// object: blocks of 16^3 voxels that exist only where a frame saw a surface, integration over the touched blocks, extraction across block
// faces.  se3et_amd/tsdf_sparse.py carries the same contract; csrc/tsdf_sparse_core.h holds the text that the kernels and the
// se3_debug_stsdf_touch_host / se3_debug_stsdf_integrate_host / se3_debug_stsdf_extract_host entries share, and csrc/tsdf_core.h, unchanged,
// everything per voxel.
// (SE3_EXACT_FP: the file is built with contraction off, and every contract function fences itself as well.  SE3_NO_SLP_VECTORIZE: the
// hazard note at the top of csrc/tsdf.hip holds here, the integration kernel inlines the same ts_integrate.)
//
// State.  A block is 16^3 voxels of length vl; block (v, b) of volume v has its corner at o_a = L f64(b_a), L = 16 vl, and is a uniform
// volume of resolution 16 there: local voxel [x, y, z] at (x 16 + y) 16 + z.  The storage is tsdf, weight (S, 16, 16, 16) float32 and colour
// (S, 3, 16, 16, 16) float32 in slots; the directory is the blocks' keys, ascending, with each block's slot.  The key packs 5 bits of
// volume above 3 x 19 bits of b_a + 2^18 into a non-negative int64, so key order is (volume, bx, by, bz) lexicographic.
//
// Contract A: allocation.  Float64 unless said.  Frame f of volume v has extrinsic E (world to camera) and camera pose P, its inverse,
// computed once on the host in float64 and passed in with the float64 intrinsics (fx, fy, cx, cy).
//   1. Sampled pixels are rows i and columns j that are multiples of `stride`.
//   2. d = f32(raw) / f32(depth_scale) in float32; d >= f32(depth_trunc) makes d = 0; the pixel is skipped unless d > 0: item 4 of the
//      uniform integration, so allocation and integration agree on which pixels exist.
//   3. z = f64(d), x = ((j - cx) z) / fx, y = ((i - cy) z) / fy.
//   4. q_a = ((P[a][0] x + P[a][1] y) + P[a][2] z) + P[a][3].  A pixel with a non-finite q is skipped.
//   5. lo_a = floor((q_a - sdf_trunc) / L), hi_a = floor((q_a + sdf_trunc) / L).  Frame f touches every block (v, b) with lo <= b <= hi.
//      sdf_trunc is at most L, so a pixel touches 27 blocks or fewer (64 where the two quotients round apart; the loops take the range
//      as it comes).
//   6. A touched coordinate outside [-2^18, 2^18) is reported with its frame, and the caller refuses the call before any state changes.
// A block exists from the first call in which a frame touches it, starts as zeros and never disappears.
//
// Contract B: integration.  Block (v, b) integrates exactly the frames that touch it, in ascending frame order, as the uniform contract
// (csrc/tsdf.hip, items 1 to 7) does for a volume of resolution 16 with origin o: its tsdf, weight and colour are bit-identical to that
// uniform volume's given that frame subset.  The running average of a voxel only ever sees the voxel's own frame sequence, so the result
// does not depend on how the frames are split over calls, on the other volumes of the batch, or on when the storage grew.
//
// Contract C: extraction.  Float64.
//   1. Output order is ascending key, then (x, y, z, axis) inside a block.
//   2. Usability and the sign test are ts_usable and the test of ts_edges.  There is no border exclusion.
//   3. The neighbour of local voxel idx along axis i is idx + e_i in the same block, and voxel idx_i = 0 of block b + e_i when idx_i = 15.
//      An absent block gives no point.
//   4. Point, colour and normal follow items 3 and 4 of the uniform extraction in block-local coordinates: p0_a = vl / 2 + vl idx_a, and
//      the returned point is p + o.
//   5. T(q) has g_a = q_a / vl - 0.5.  p_a lies between the centres of local voxels idx_a >= 0 and idx_a + 1 <= 16, so p_a / vl - 0.5 is
//      in [0, 16] and, h being 0.99 vl, g_a is in [-0.99, 16.99]; float64 rounding moves g_a by less than 2^-40, so floor(g_a) is in
//      [-1, 16] and the far corner of the stencil is at most 17: every read falls in the block or one of its 26 neighbours (sts_at maps
//      an index in [-1, 17] to a neighbour and a local index in [0, 16), and answers "absent" for anything else).
//   6. A corner in an absent block reads 0, like an unobserved voxel.
//
// Departures from Open3D.  Open3D allocates per call from a hash map, so its unit order depends on the order of insertion; here the
// order is the key order and the order of the records is irrelevant.  Allocation and integration share one depth rule (item 2).  Weights
// have no cap, colours are stored in [0, 1], the surface test is a sign test: as in csrc/tsdf.hip.
//
// Determinism.  No atomics anywhere.  The touch records of a call are a set: which workgroup emits a record, and how often, does not
// reach the result, because the caller sorts them and drops duplicates.  Every voxel is independent.
//
// Launches.
//   stsdf_touch_kernel      one workgroup of 256 threads per tile of 16 x 16 sampled pixels of one frame, a thread per pixel.  The
//                           threads' block ranges go to LDS; a thread emits a block unless the pixel to its left or above it in the tile
//                           touches it too (that pixel, or one further on, emits it: induction over the tile), which removes most of
//                           what neighbouring pixels share before anything is written.  Count, se3_exclusive_scan_i64, write; records
//                           come out in frame order, so a stable sort by key leaves each block's frames ascending.
//   stsdf_neighbors_kernel  a thread per (block, neighbour): binary search in the sorted keys.
//   stsdf_integrate_kernel  one workgroup of 256 threads per (touched block, x): lanes run along z then y, so a wave covers 64 contiguous
//                           floats of the block.  A thread keeps its voxel's state in registers across the block's frames; the rows
//                           of the frame table pass through LDS in tiles of SE3_TSDF_FRAME_TILE, gathered by the block's frame list
//                           (CSR); the state is written only where a frame touched it.
//   stsdf_count_kernel / stsdf_write_kernel   one workgroup of 256 threads per (block, x), a thread per (y, z): se3_block_exclusive
//                           places a workgroup's points in (y, z, axis) order, se3_exclusive_scan_i64 the workgroups'.
#include <math.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "common.h"
#include "tsdf_sparse_core.h"

namespace {

constexpr int kStsThreads = 256;
constexpr int kStsTile = 16;                                            // sampled pixels per tile side
static_assert(kStsdfBlock == SE3_STSDF_BLOCK && kStsdfCoordBits == SE3_STSDF_COORD_BITS && kStsdfMaxTruncVoxels == SE3_STSDF_MAX_TRUNC_VOXELS &&
                  kStsdfMaxStride == SE3_STSDF_MAX_STRIDE && kStsdfPoseWords == SE3_STSDF_POSE_WORDS,
              "tsdf_sparse_core.h and include/se3et_hip.h name the same limits");
static_assert(kTsdfFrameTile == SE3_TSDF_FRAME_TILE && kTsdfFrameWords == SE3_TSDF_FRAME_WORDS, "the frame table of csrc/tsdf.hip");
static_assert(kStsThreads == kStsdfBlock * kStsdfBlock && kStsThreads == kStsTile * kStsTile, "a thread per (y, z) and per pixel of a tile");
static_assert(4 * kStsdfBlock == SE3_WAVE, "a wave is four rows of z");

__device__ __forceinline__ bool sts_box_has(const int* box, int bx, int by, int bz) {
  return box[0] <= bx && bx <= box[3] && box[1] <= by && by <= box[4] && box[2] <= bz && bz <= box[5];
}

// WRITE false: counts[group] = the records of the group, bad[frame] = 1 where a pixel of the frame touches a coordinate out of range.
// WRITE true: the records at counts[group] (the exclusive offsets by then), nothing at or past `capacity`.
template <bool WRITE>
__global__ __launch_bounds__(kStsThreads) void stsdf_touch_kernel(StsTouch T, const double* __restrict__ poses, PairRows frame_rows, int tiles_y,
                                                                  int tiles_x, int* __restrict__ bad, int64_t* __restrict__ counts,
                                                                  int64_t capacity, int64_t* __restrict__ out_keys,
                                                                  int* __restrict__ out_frames) {
  __shared__ int box[kStsThreads][6];
  __shared__ int sh[kStsThreads];
  const int t = threadIdx.x;
  const int64_t group = blockIdx.x;
  const int tx = (int)(group % tiles_x), ty = (int)((group / tiles_x) % tiles_y);
  const int64_t frame = group / ((int64_t)tiles_x * tiles_y);
  const int rows = (T.H + T.stride - 1) / T.stride, cols = (T.W + T.stride - 1) / T.stride;
  const int r = ty * kStsTile + (t >> 4), c = tx * kStsTile + (t & (kStsTile - 1));
  int mine[6] = {1, 0, 0, 0, 0, 0};                                     // (lo, hi): empty
  if (r < rows && c < cols) {                                           // (no early return: every thread meets the barriers)
    double lo[3], hi[3];
    if (sts_pixel_range(T, poses + frame * kStsdfPoseWords, frame, r * T.stride, c * T.stride, lo, hi)) {
      if (sts_range_ok(lo, hi)) {
        for (int a = 0; a < 3; a++) mine[a] = (int)lo[a], mine[3 + a] = (int)hi[a];
      } else if (!WRITE) {
        bad[frame] = 1;                                                 // (every writer stores the same value)
      }
    }
  }
  for (int a = 0; a < 6; a++) box[t][a] = mine[a];
  __syncthreads();
  const int* left = (t & (kStsTile - 1)) ? box[t - 1] : nullptr;
  const int* up = (t >> 4) ? box[t - kStsTile] : nullptr;
  int n = 0, total;
  for (int bx = mine[0]; bx <= mine[3]; bx++)
    for (int by = mine[1]; by <= mine[4]; by++)
      for (int bz = mine[2]; bz <= mine[5]; bz++)
        n += !((left && sts_box_has(left, bx, by, bz)) || (up && sts_box_has(up, bx, by, bz)));
  const int first = se3_block_exclusive<int, kStsThreads>(n, sh, &total);
  if (!WRITE) {
    if (t == 0) counts[group] = total;
    return;
  }
  const int vol = pg_pair_of_row(frame_rows, frame);
  int64_t out = counts[group] + first;
  for (int bx = mine[0]; bx <= mine[3]; bx++)
    for (int by = mine[1]; by <= mine[4]; by++)
      for (int bz = mine[2]; bz <= mine[5]; bz++) {
        if ((left && sts_box_has(left, bx, by, bz)) || (up && sts_box_has(up, bx, by, bz))) continue;
        if (out < capacity) out_keys[out] = sts_key(vol, bx, by, bz), out_frames[out] = (int)frame;
        out++;
      }
}

__global__ __launch_bounds__(kStsThreads) void stsdf_neighbors_kernel(const int64_t* __restrict__ keys, const int* __restrict__ slots, int64_t n,
                                                                      int* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kStsThreads + threadIdx.x;
  if (i >= n * 27) return;
  out[i] = sts_neighbor(keys, slots, n, i / 27, (int)(i % 27));
}

// workgroup (block, x) of the touched blocks: keys, slots (num_blocks), the frames of block i at ids[csr[i], csr[i + 1]), ascending
__global__ __launch_bounds__(kStsThreads) void stsdf_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                                      float* __restrict__ color, int64_t num_slots,
                                                                      const int64_t* __restrict__ keys, const int* __restrict__ slots,
                                                                      const int64_t* __restrict__ csr, const int* __restrict__ ids,
                                                                      int64_t num_frames, double vl, TsImages im,
                                                                      const float* __restrict__ frames) {
  __shared__ float table[kTsdfFrameTile * kTsdfFrameWords];
  __shared__ int frame_of[kTsdfFrameTile];
  const int64_t blk = blockIdx.x / kStsdfBlock;
  const int x = blockIdx.x % kStsdfBlock, y = threadIdx.x >> 4, z = threadIdx.x & (kStsdfBlock - 1);
  const int64_t slot = slots[blk], f0 = csr[blk], f1 = csr[blk + 1];
  if (slot < 0 || slot >= num_slots || f0 >= f1) return;                // (uniform over the workgroup; a slot outside the storage is never written)
  int b[3];
  sts_key_coords(keys[blk], b);
  const double L = sts_block_length(vl);
  const int64_t at = slot * kStsdfBlockVoxels + ts_index(kStsdfBlock, x, y, z);
  float t = tsdf[at], w = weight[at], c[3] = {0.0f, 0.0f, 0.0f};
  if (color)
    for (int k = 0; k < 3; k++) c[k] = color[sts_color_at(at, k)];
  const float wx = ts_world(vl, x, sts_origin(L, b[0])), wy = ts_world(vl, y, sts_origin(L, b[1])), wz = ts_world(vl, z, sts_origin(L, b[2]));
  bool touched = false;
  for (int64_t base = f0; base < f1; base += kTsdfFrameTile) {
    const int m = (int)(f1 - base < kTsdfFrameTile ? f1 - base : kTsdfFrameTile);
    __syncthreads();
    for (int i = threadIdx.x; i < m * kTsdfFrameWords; i += kStsThreads) {
      const int f = ids[base + i / kTsdfFrameWords];
      const bool known = f >= 0 && f < num_frames;                      // (a frame outside the call's images is not read)
      table[i] = known ? frames[(int64_t)f * kTsdfFrameWords + i % kTsdfFrameWords] : 0.0f;
      if (i % kTsdfFrameWords == 0) frame_of[i / kTsdfFrameWords] = known ? f : -1;
    }
    __syncthreads();
    for (int i = 0; i < m; i++)
      if (frame_of[i] >= 0) touched |= ts_integrate(table + i * kTsdfFrameWords, im, frame_of[i], wx, wy, wz, &t, &w, c);
  }
  if (touched) {
    tsdf[at] = t, weight[at] = w;
    if (color)
      for (int k = 0; k < 3; k++) color[sts_color_at(at, k)] = c[k];
  }
}

PG_HD StsBlock sts_block(const float* tsdf, const float* weight, const float* color, int64_t key, const int* nb, double vl) {
  StsBlock B;
  B.tsdf = tsdf, B.weight = weight, B.color = color, B.nb = nb, B.vl = vl;
  int b[3];
  sts_key_coords(key, b);
  const double L = sts_block_length(vl);
  for (int a = 0; a < 3; a++) B.origin[a] = sts_origin(L, b[a]);
  return B;
}

PG_HD int sts_popcount3(int mask) { return (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1); }

// WRITE false: counts[group] = the points of group (block, x) = block 16 + x.  WRITE true: the points at counts[group] (offsets by then).
template <bool WRITE>
__global__ __launch_bounds__(kStsThreads) void stsdf_extract_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                    const float* __restrict__ color, const int64_t* __restrict__ keys,
                                                                    const int* __restrict__ neighbors, double vl, int64_t* __restrict__ counts,
                                                                    int64_t capacity, double* __restrict__ out_points,
                                                                    double* __restrict__ out_normals, double* __restrict__ out_colors) {
  __shared__ int sh[kStsThreads];
  const int64_t group = blockIdx.x, blk = group / kStsdfBlock;
  if (WRITE && counts[group + 1] == counts[group]) return;              // (uniform over the workgroup)
  const int x = (int)(group % kStsdfBlock), y = threadIdx.x >> 4, z = threadIdx.x & (kStsdfBlock - 1);
  const StsBlock B = sts_block(tsdf, weight, color, keys[blk], neighbors + blk * 27, vl);
  const int mask = sts_edges(B, x, y, z);
  int total;
  const int first = se3_block_exclusive<int, kStsThreads>(sts_popcount3(mask), sh, &total);
  if (!WRITE) {
    if (threadIdx.x == 0) counts[group] = total;
    return;
  }
  int64_t out = counts[group] + first;
  for (int axis = 0; axis < 3; axis++) {
    if (!(mask >> axis & 1)) continue;
    double p[3], n[3], c[3];
    sts_emit(B, x, y, z, axis, p, n, c);
    if (out < capacity)
      for (int a = 0; a < 3; a++) {
        out_points[3 * out + a] = p[a], out_normals[3 * out + a] = n[a];
        if (color) out_colors[3 * out + a] = c[a];
      }
    out++;
  }
}

bool stsdf_volume_args(const char* what, double vl, double trunc) {
  if (!(isfinite(vl) && vl > 0.0)) return se3_set_error("%s: voxel_length %g is not a positive finite number", what, vl), false;
  if (!(isfinite(trunc) && trunc > 0.0 && trunc <= kStsdfMaxTruncVoxels * vl && (float)trunc > 0.0f))
    return se3_set_error("%s: sdf_trunc %g not in (0, %d voxel lengths]", what, trunc, kStsdfMaxTruncVoxels), false;
  return true;
}

bool stsdf_image_args(const char* what, int depth_elem, int H, int W, double depth_scale, double depth_trunc) {
  if (H < 1 || W < 1 || H > kTsdfMaxImage || W > kTsdfMaxImage)
    return se3_set_error("%s: images of %d x %d (each side in [1, %d])", what, H, W, kTsdfMaxImage), false;
  if (depth_elem != 0 && depth_elem != 1) return se3_set_error("%s: depth_elem %d", what, depth_elem), false;
  if (!(isfinite(depth_scale) && depth_scale > 0.0 && isfinite(depth_trunc) && depth_trunc > 0.0))
    return se3_set_error("%s: depth_scale %g and depth_trunc %g must be positive and finite", what, depth_scale, depth_trunc), false;
  return true;
}

bool stsdf_color_args(const char* what, bool has_color, const void* colors, int color_elem) {
  if (color_elem < 0 || color_elem > 2 || (color_elem != 0) != (colors != nullptr) || (color_elem != 0) != has_color)
    return se3_set_error("%s: color_elem %d: colours go with a volume that has colour, and only with one", what, color_elem), false;
  return true;
}

bool stsdf_touch_args(const char* what, int depth_elem, int64_t F, int H, int W, int num_volumes, double vl, double trunc, int stride,
                      double depth_scale, double depth_trunc) {
  if (!stsdf_volume_args(what, vl, trunc) || !stsdf_image_args(what, depth_elem, H, W, depth_scale, depth_trunc)) return false;
  if (stride < 1 || stride > kStsdfMaxStride) return se3_set_error("%s: stride %d not in [1, %d]", what, stride, kStsdfMaxStride), false;
  if (F < 0 || num_volumes < 0 || num_volumes > kPairMaxPairs)
    return se3_set_error("%s: %lld frames, %d volumes (at most %d)", what, (long long)F, num_volumes, kPairMaxPairs), false;
  return true;
}

int64_t stsdf_tiles(int side, int stride) { return se3_cdiv(se3_cdiv(side, stride), kStsTile); }

}  // namespace

extern "C" int64_t se3_stsdf_touch_groups(int64_t num_frames, int height, int width, int stride) {
  if (num_frames < 0 || height < 1 || width < 1 || stride < 1) return 0;
  return num_frames * stsdf_tiles(height, stride) * stsdf_tiles(width, stride);
}

extern "C" int se3_stsdf_touch_stack(const void* depths, int depth_elem, int64_t num_frames, int height, int width, const double* poses,
                                     const int64_t* frame_offsets_host, int num_volumes, double voxel_length, double sdf_trunc, int stride,
                                     double depth_scale, double depth_trunc, int64_t* group_offsets, int* bad_frames, int64_t capacity,
                                     int64_t* out_keys, int* out_frames, void* stream) {
  const char* what = "stsdf_touch_stack";
  SE3_REQUIRE(frame_offsets_host && group_offsets, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  if (!stsdf_touch_args(what, depth_elem, num_frames, height, width, num_volumes, voxel_length, sdf_trunc, stride, depth_scale, depth_trunc))
    return SE3_ERR_INVALID_ARG;
  PairRows rows;
  SE3_REQUIRE(pg_fill_rows(&rows, frame_offsets_host, num_volumes) && rows.start[num_volumes] == num_frames, SE3_ERR_INVALID_ARG,
              "%s: frame offsets must start at 0, not decrease and end at the %lld frames", what, (long long)num_frames);
  const int64_t groups = se3_stsdf_touch_groups(num_frames, height, width, stride);
  SE3_REQUIRE(groups < (1ll << 31), SE3_ERR_UNSUPPORTED, "%s: %lld pixel tiles in one call (below 2^31)", what, (long long)groups);
  SE3_REQUIRE(groups == 0 || (depths && poses), SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  hipStream_t st = (hipStream_t)stream;
  const StsTouch T = sts_touch(depths, depth_elem, height, width, stride, voxel_length, sdf_trunc, depth_scale, depth_trunc);
  const int ty = (int)stsdf_tiles(height, stride), tx = (int)stsdf_tiles(width, stride);
  if (!out_keys) {
    SE3_REQUIRE(groups == 0 || bad_frames, SE3_ERR_INVALID_ARG, "%s: the count pass needs the frames' flags", what);
    if (groups > 0)
      stsdf_touch_kernel<false><<<(unsigned)groups, kStsThreads, 0, st>>>(T, poses, rows, ty, tx, bad_frames, group_offsets, 0, nullptr, nullptr);
    se3_exclusive_scan_i64(group_offsets, groups, st);
  } else {
    SE3_REQUIRE(out_frames && capacity >= 0, SE3_ERR_INVALID_ARG, "%s: the write pass needs the frames of the records", what);
    if (groups > 0 && capacity > 0)
      stsdf_touch_kernel<true><<<(unsigned)groups, kStsThreads, 0, st>>>(T, poses, rows, ty, tx, nullptr, group_offsets, capacity, out_keys,
                                                                         out_frames);
  }
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" int se3_stsdf_neighbors(const int64_t* keys, const int* slots, int64_t num_blocks, int* out_neighbors, void* stream) {
  const char* what = "stsdf_neighbors";
  SE3_REQUIRE(num_blocks >= 0 && num_blocks < (1ll << 31) / 27, SE3_ERR_UNSUPPORTED, "%s: %lld blocks (below 2^31 / 27)", what,
              (long long)num_blocks);
  if (num_blocks == 0) return SE3_OK;
  SE3_REQUIRE(keys && slots && out_neighbors, SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  stsdf_neighbors_kernel<<<(unsigned)se3_cdiv(num_blocks * 27, kStsThreads), kStsThreads, 0, (hipStream_t)stream>>>(keys, slots, num_blocks,
                                                                                                                 out_neighbors);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" int se3_stsdf_integrate_stack(float* tsdf, float* weight, float* color, int64_t num_slots, const int64_t* block_keys,
                                         const int* block_slots, int64_t num_blocks, const int64_t* block_frame_offsets,
                                         const int* block_frames, double voxel_length, double sdf_trunc, const void* depths, int depth_elem,
                                         const void* colors, int color_elem, int64_t num_frames, int height, int width, const float* frames,
                                         double depth_scale, double depth_trunc, void* stream) {
  const char* what = "stsdf_integrate_stack";
  SE3_REQUIRE(num_slots >= 0 && num_blocks >= 0 && num_frames >= 0, SE3_ERR_INVALID_ARG, "%s: a negative count", what);
  if (!stsdf_volume_args(what, voxel_length, sdf_trunc) || !stsdf_image_args(what, depth_elem, height, width, depth_scale, depth_trunc) ||
      !stsdf_color_args(what, color != nullptr, colors, color_elem))
    return SE3_ERR_INVALID_ARG;
  SE3_REQUIRE(num_frames < (1ll << 31) && num_blocks < (1ll << 31) / kStsdfBlock && num_slots < (1ll << 31), SE3_ERR_UNSUPPORTED,
              "%s: %lld frames, %lld blocks, %lld slots in one call", what, (long long)num_frames, (long long)num_blocks, (long long)num_slots);
  if (num_blocks == 0 || num_frames == 0) return SE3_OK;
  SE3_REQUIRE(tsdf && weight && block_keys && block_slots && block_frame_offsets && block_frames && depths && frames, SE3_ERR_INVALID_ARG,
              "%s: null pointer", what);
  const TsImages im = ts_images(depths, depth_elem, colors, color_elem, height, width, depth_scale, depth_trunc, sdf_trunc);
  stsdf_integrate_kernel<<<(unsigned)(num_blocks * kStsdfBlock), kStsThreads, 0, (hipStream_t)stream>>>(
      tsdf, weight, color, num_slots, block_keys, block_slots, block_frame_offsets, block_frames, num_frames, voxel_length, im, frames);
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

extern "C" int se3_stsdf_extract_stack(const float* tsdf, const float* weight, const float* color, const int64_t* keys, const int* neighbors,
                                       int64_t num_blocks, double voxel_length, int64_t* group_offsets, int64_t capacity, double* out_points,
                                       double* out_normals, double* out_colors, void* stream) {
  const char* what = "stsdf_extract_stack";
  SE3_REQUIRE(group_offsets && num_blocks >= 0, SE3_ERR_INVALID_ARG, "%s: null pointer or a negative block count", what);
  SE3_REQUIRE(num_blocks < (1ll << 31) / kStsdfBlock, SE3_ERR_UNSUPPORTED, "%s: %lld blocks (below 2^31 / 16)", what, (long long)num_blocks);
  SE3_REQUIRE(isfinite(voxel_length) && voxel_length > 0.0, SE3_ERR_INVALID_ARG, "%s: voxel_length %g is not a positive finite number", what,
              voxel_length);
  SE3_REQUIRE(num_blocks == 0 || (tsdf && weight && keys && neighbors), SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  const int64_t groups = num_blocks * kStsdfBlock;
  hipStream_t st = (hipStream_t)stream;
  if (!out_points) {
    if (groups > 0)
      stsdf_extract_kernel<false><<<(unsigned)groups, kStsThreads, 0, st>>>(tsdf, weight, nullptr, keys, neighbors, voxel_length, group_offsets, 0,
                                                                           nullptr, nullptr, nullptr);
    se3_exclusive_scan_i64(group_offsets, groups, st);
  } else {
    SE3_REQUIRE(out_normals && (out_colors != nullptr) == (color != nullptr) && capacity >= 0, SE3_ERR_INVALID_ARG,
                "%s: the write pass needs normals and, exactly with colour, colours", what);
    if (groups > 0 && capacity > 0)
      stsdf_extract_kernel<true><<<(unsigned)groups, kStsThreads, 0, st>>>(tsdf, weight, color, keys, neighbors, voxel_length, group_offsets,
                                                                          capacity, out_points, out_normals, out_colors);
  }
  SE3_CHECK_LAUNCH(what);
  return SE3_OK;
}

// ---- the same text on host memory, serially, no GPU (tests/test_tsdf_sparse_cpu.py) ----------------------------------------------------------
// The records of the frames, sorted by (key, frame) without duplicates: the form the device's records take after the caller's sort.
// *out_bad_frame: the first frame with a touched coordinate out of range, or -1; with one, nothing else is returned.
extern "C" int se3_debug_stsdf_touch_host(const void* depths, int depth_elem, int64_t num_frames, int height, int width, const double* poses,
                                          const int64_t* frame_offsets, int num_volumes, double voxel_length, double sdf_trunc, int stride,
                                          double depth_scale, double depth_trunc, int64_t capacity, int64_t* out_keys, int* out_frames,
                                          int64_t* out_count, int64_t* out_bad_frame) {
  const char* what = "debug_stsdf_touch_host";
  SE3_REQUIRE(frame_offsets && out_count && out_bad_frame && (num_frames <= 0 || (depths && poses)), SE3_ERR_INVALID_ARG, "%s: null pointer", what);
  if (!stsdf_touch_args(what, depth_elem, num_frames, height, width, num_volumes, voxel_length, sdf_trunc, stride, depth_scale, depth_trunc))
    return SE3_ERR_INVALID_ARG;
  PairRows rows;
  SE3_REQUIRE(pg_fill_rows(&rows, frame_offsets, num_volumes) && rows.start[num_volumes] == num_frames && num_frames < (1ll << 31),
              SE3_ERR_INVALID_ARG, "%s: frame offsets must start at 0, not decrease and end at the %lld frames", what, (long long)num_frames);
  SE3_REQUIRE(!out_keys || (out_frames && capacity >= 0), SE3_ERR_INVALID_ARG, "%s: keys come with frames", what);
  const StsTouch T = sts_touch(depths, depth_elem, height, width, stride, voxel_length, sdf_trunc, depth_scale, depth_trunc);
  std::vector<std::pair<int64_t, int>> records;
  *out_count = 0, *out_bad_frame = -1;
  for (int64_t f = 0; f < num_frames; f++) {
    const int vol = pg_pair_of_row(rows, f);
    for (int i = 0; i < height; i += stride)
      for (int j = 0; j < width; j += stride) {
        double lo[3], hi[3];
        if (!sts_pixel_range(T, poses + f * kStsdfPoseWords, f, i, j, lo, hi)) continue;
        if (!sts_range_ok(lo, hi)) {
          *out_bad_frame = f;
          return SE3_OK;
        }
        for (int bx = (int)lo[0]; bx <= (int)hi[0]; bx++)
          for (int by = (int)lo[1]; by <= (int)hi[1]; by++)
            for (int bz = (int)lo[2]; bz <= (int)hi[2]; bz++) records.emplace_back(sts_key(vol, bx, by, bz), (int)f);
      }
    std::sort(records.begin(), records.end());                          // (per frame, so that the list stays as short as the result)
    records.erase(std::unique(records.begin(), records.end()), records.end());
  }
  *out_count = (int64_t)records.size();
  if (out_keys)
    for (int64_t r = 0; r < *out_count && r < capacity; r++) out_keys[r] = records[r].first, out_frames[r] = records[r].second;
  return SE3_OK;
}

extern "C" int se3_debug_stsdf_integrate_host(float* tsdf, float* weight, float* color, int64_t num_slots, const int64_t* block_keys,
                                              const int* block_slots, int64_t num_blocks, const int64_t* block_frame_offsets,
                                              const int* block_frames, double voxel_length, double sdf_trunc, const void* depths,
                                              int depth_elem, const void* colors, int color_elem, int64_t num_frames, int height, int width,
                                              const float* frames, double depth_scale, double depth_trunc) {
  const char* what = "debug_stsdf_integrate_host";
  SE3_REQUIRE(num_slots >= 0 && num_blocks >= 0 && num_frames >= 0, SE3_ERR_INVALID_ARG, "%s: a negative count", what);
  if (!stsdf_volume_args(what, voxel_length, sdf_trunc) || !stsdf_image_args(what, depth_elem, height, width, depth_scale, depth_trunc) ||
      !stsdf_color_args(what, color != nullptr, colors, color_elem))
    return SE3_ERR_INVALID_ARG;
  if (num_blocks == 0 || num_frames == 0) return SE3_OK;
  SE3_REQUIRE(tsdf && weight && block_keys && block_slots && block_frame_offsets && block_frames && depths && frames, SE3_ERR_INVALID_ARG,
              "%s: null pointer", what);
  const TsImages im = ts_images(depths, depth_elem, colors, color_elem, height, width, depth_scale, depth_trunc, sdf_trunc);
  const double L = sts_block_length(voxel_length);
  for (int64_t blk = 0; blk < num_blocks; blk++) {
    const int64_t slot = block_slots[blk];
    SE3_REQUIRE(slot >= 0 && slot < num_slots, SE3_ERR_INVALID_ARG, "%s: block %lld has slot %lld of %lld", what, (long long)blk, (long long)slot,
                (long long)num_slots);
    int b[3];
    sts_key_coords(block_keys[blk], b);
    for (int x = 0; x < kStsdfBlock; x++)
      for (int y = 0; y < kStsdfBlock; y++)
        for (int z = 0; z < kStsdfBlock; z++) {
          const int64_t at = slot * kStsdfBlockVoxels + ts_index(kStsdfBlock, x, y, z);
          float t = tsdf[at], w = weight[at], c[3] = {0.0f, 0.0f, 0.0f};
          if (color)
            for (int k = 0; k < 3; k++) c[k] = color[sts_color_at(at, k)];
          const float wx = ts_world(voxel_length, x, sts_origin(L, b[0])), wy = ts_world(voxel_length, y, sts_origin(L, b[1])),
                      wz = ts_world(voxel_length, z, sts_origin(L, b[2]));
          bool touched = false;
          for (int64_t r = block_frame_offsets[blk]; r < block_frame_offsets[blk + 1]; r++) {
            const int f = block_frames[r];
            if (f >= 0 && f < num_frames) touched |= ts_integrate(frames + (int64_t)f * kTsdfFrameWords, im, f, wx, wy, wz, &t, &w, c);
          }
          if (!touched) continue;
          tsdf[at] = t, weight[at] = w;
          if (color)
            for (int k = 0; k < 3; k++) color[sts_color_at(at, k)] = c[k];
        }
  }
  return SE3_OK;
}

extern "C" int se3_debug_stsdf_extract_host(const float* tsdf, const float* weight, const float* color, const int64_t* keys, const int* slots,
                                            int64_t num_blocks, double voxel_length, int64_t capacity, double* out_points, double* out_normals,
                                            double* out_colors, int64_t* out_block_offsets) {
  const char* what = "debug_stsdf_extract_host";
  SE3_REQUIRE(out_block_offsets && num_blocks >= 0 && (num_blocks == 0 || (tsdf && weight && keys && slots)), SE3_ERR_INVALID_ARG,
              "%s: null pointer or a negative block count", what);
  SE3_REQUIRE(!out_points || (out_normals && (out_colors != nullptr) == (color != nullptr) && capacity >= 0), SE3_ERR_INVALID_ARG,
              "%s: points need normals and, exactly with colour, colours", what);
  SE3_REQUIRE(isfinite(voxel_length) && voxel_length > 0.0, SE3_ERR_INVALID_ARG, "%s: voxel_length %g is not a positive finite number", what,
              voxel_length);
  int64_t n = 0;
  for (int64_t blk = 0; blk < num_blocks; blk++) {
    int nb[27];
    for (int k = 0; k < 27; k++) nb[k] = sts_neighbor(keys, slots, num_blocks, blk, k);
    const StsBlock B = sts_block(tsdf, weight, color, keys[blk], nb, voxel_length);
    out_block_offsets[blk] = n;
    for (int x = 0; x < kStsdfBlock; x++)
      for (int y = 0; y < kStsdfBlock; y++)
        for (int z = 0; z < kStsdfBlock; z++) {
          const int mask = sts_edges(B, x, y, z);
          for (int axis = 0; axis < 3; axis++) {
            if (!(mask >> axis & 1)) continue;
            if (out_points && n < capacity) {
              double c[3];
              sts_emit(B, x, y, z, axis, out_points + 3 * n, out_normals + 3 * n, color ? out_colors + 3 * n : c);
            }
            n++;
          }
        }
  }
  out_block_offsets[num_blocks] = n;
  return SE3_OK;
}
