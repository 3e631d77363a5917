// The text of block-sparse TSDF volumes that is not per voxel (csrc/tsdf_sparse.hip carries the contract): a block's key, a pixel's range of
// touched blocks, the lookup in the sorted directory and a block's 27 neighbours, and extraction that reads through that neighbour table.
// Everything per voxel -- ts_world, ts_integrate, ts_usable -- is csrc/tsdf_core.h as it stands; a block is a uniform volume of resolution
// kStsdfBlock at its corner.  __host__ __device__ text that the kernels and the se3_debug_stsdf_*_host entries both run; allocation and
// extraction are float64, contraction off in every function.
#pragma once
#include "tsdf_core.h"

constexpr int kStsdfBlock = 16;                // SE3_STSDF_BLOCK: voxels per block side
constexpr int kStsdfCoordBits = 19;            // SE3_STSDF_COORD_BITS: a block coordinate lies in [-2^18, 2^18)
constexpr int kStsdfMaxTruncVoxels = 16;       // SE3_STSDF_MAX_TRUNC_VOXELS: sdf_trunc is at most one block
constexpr int kStsdfMaxStride = 64;            // SE3_STSDF_MAX_STRIDE
constexpr int kStsdfPoseWords = 16;            // SE3_STSDF_POSE_WORDS: P[3][4] by rows, fx, fy, cx, cy (float64)
constexpr int kStsdfBlockVoxels = kStsdfBlock * kStsdfBlock * kStsdfBlock;
constexpr int kStsdfBias = 1 << (kStsdfCoordBits - 1);
constexpr int kStsdfVolumeShift = 3 * kStsdfCoordBits;
static_assert((kPairMaxPairs - 1) < (1 << (63 - kStsdfVolumeShift)), "the volume fits above the coordinates of a non-negative int64");
static_assert(kStsdfBlockVoxels == 4096 && kStsdfMaxTruncVoxels <= kStsdfBlock, "a truncation of at most one block");

// ---- keys -------------------------------------------------------------------------------------------------------------------------------
// (volume, bx, by, bz) -> volume above three biased coordinates: int64 order is (volume, bx, by, bz) lexicographic
PG_HD int64_t sts_key(int vol, int bx, int by, int bz) {
  return ((int64_t)vol << kStsdfVolumeShift) | ((int64_t)(bx + kStsdfBias) << (2 * kStsdfCoordBits)) |
         ((int64_t)(by + kStsdfBias) << kStsdfCoordBits) | (int64_t)(bz + kStsdfBias);
}
PG_HD int sts_key_volume(int64_t key) { return (int)(key >> kStsdfVolumeShift); }
PG_HD void sts_key_coords(int64_t key, int* b) {
  const int64_t mask = ((int64_t)1 << kStsdfCoordBits) - 1;
  b[0] = (int)((key >> (2 * kStsdfCoordBits)) & mask) - kStsdfBias;
  b[1] = (int)((key >> kStsdfCoordBits) & mask) - kStsdfBias;
  b[2] = (int)(key & mask) - kStsdfBias;
}
PG_HD bool sts_coord_ok(int b) { return b >= -kStsdfBias && b < kStsdfBias; }
// L = 16 vl, and the corner of block b along one axis: o = L f64(b)
PG_HD double sts_block_length(double vl) {
#pragma clang fp contract(off)
  return (double)kStsdfBlock * vl;
}
PG_HD double sts_origin(double L, int b) {
#pragma clang fp contract(off)
  return L * (double)b;
}

// ---- allocation: contract A ---------------------------------------------------------------------------------------------------------------
struct StsTouch {
  const void* depth;        // (F, H, W) uint16 (depth_elem 0) or float32 (1)
  int depth_elem, H, W, stride;
  float scale, depth_trunc;          // f32(depth_scale), f32(depth_trunc): integration item 4
  double trunc, L;
};

PG_HD StsTouch sts_touch(const void* depth, int depth_elem, int H, int W, int stride, double vl, double sdf_trunc, double depth_scale,
                         double depth_trunc) {
  StsTouch T;
  T.depth = depth, T.depth_elem = depth_elem, T.H = H, T.W = W, T.stride = stride;
  T.scale = (float)depth_scale, T.depth_trunc = (float)depth_trunc, T.trunc = sdf_trunc, T.L = sts_block_length(vl);
  return T;
}

// items 2 to 5 for pixel (i, j) of image `frame`: pose = the frame's kStsdfPoseWords words.  False: the pixel is skipped.  lo, hi: the
// floors as float64, so that a range outside the coordinates is seen before any conversion to int (sts_range_ok).
PG_HD bool sts_pixel_range(const StsTouch& T, const double* pose, int64_t frame, int i, int j, double* lo, double* hi) {
#pragma clang fp contract(off)
  const int64_t pixel = (frame * T.H + i) * T.W + j;
  const float raw = T.depth_elem ? ((const float*)T.depth)[pixel] : (float)((const uint16_t*)T.depth)[pixel];
  float d = ts_div(raw, T.scale);
  if (d >= T.depth_trunc) d = 0.0f;
  if (!(d > 0.0f)) return false;
  const double z = (double)d;
  const double fx = pose[12], fy = pose[13], cx = pose[14], cy = pose[15];
  const double xz = ((double)j - cx) * z, yz = ((double)i - cy) * z;
  const double x = xz / fx, y = yz / fy;
  for (int a = 0; a < 3; a++) {
    const double px = pose[4 * a] * x, py = pose[4 * a + 1] * y, pz = pose[4 * a + 2] * z;
    const double s = px + py;
    const double t = s + pz;
    const double q = t + pose[4 * a + 3];
    if (!(fabs(q) < INFINITY)) return false;
    const double below = q - T.trunc, above = q + T.trunc;
    lo[a] = floor(below / T.L), hi[a] = floor(above / T.L);
  }
  return true;
}
// item 6: every touched coordinate inside [-2^18, 2^18)
PG_HD bool sts_range_ok(const double* lo, const double* hi) {
  bool ok = true;
  for (int a = 0; a < 3; a++) ok = ok && lo[a] >= (double)-kStsdfBias && hi[a] < (double)kStsdfBias;
  return ok;
}

// ---- the directory --------------------------------------------------------------------------------------------------------------------------
// the position of `key` in keys[0, n), ascending, or -1
PG_HD int64_t sts_find(const int64_t* keys, int64_t n, int64_t key) {
  int64_t a = 0, b = n;
  while (a < b) {
    const int64_t m = a + (b - a) / 2;
    if (keys[m] < key) a = m + 1;
    else b = m;
  }
  return a < n && keys[a] == key ? a : -1;
}
// the storage slot of neighbour k = (dx + 1) 9 + (dy + 1) 3 + (dz + 1) of the block at position `at` of the directory, -1 where absent
PG_HD int sts_neighbor(const int64_t* keys, const int* slots, int64_t n, int64_t at, int k) {
  if (k == 13) return slots[at];
  int b[3];
  sts_key_coords(keys[at], b);
  const int x = b[0] + k / 9 - 1, y = b[1] + (k / 3) % 3 - 1, z = b[2] + k % 3 - 1;
  if (!(sts_coord_ok(x) && sts_coord_ok(y) && sts_coord_ok(z))) return -1;
  const int64_t pos = sts_find(keys, n, sts_key(sts_key_volume(keys[at]), x, y, z));
  return pos < 0 ? -1 : slots[pos];
}

// ---- extraction: contract C -----------------------------------------------------------------------------------------------------------------
// one block with its neighbourhood.  tsdf, weight: the storage (S, 16, 16, 16); color: (S, 3, 16, 16, 16) or NULL; nb: the block's 27 slots.
struct StsBlock {
  const float *tsdf, *weight, *color;
  const int* nb;
  double vl, origin[3];
};

// where voxel (x, y, z) of the neighbourhood lies in the storage, each index in [-1, 17] (item 5): slot 4096 + the local index, or -1 in
// an absent block (and for an index outside that range, which no caller asks for)
PG_HD int64_t sts_at(const int* nb, int x, int y, int z) {
  const int cx = x < 0 ? 0 : (x >= kStsdfBlock ? 2 : 1), cy = y < 0 ? 0 : (y >= kStsdfBlock ? 2 : 1), cz = z < 0 ? 0 : (z >= kStsdfBlock ? 2 : 1);
  const int lx = x - kStsdfBlock * (cx - 1), ly = y - kStsdfBlock * (cy - 1), lz = z - kStsdfBlock * (cz - 1);
  if ((unsigned)lx >= (unsigned)kStsdfBlock || (unsigned)ly >= (unsigned)kStsdfBlock || (unsigned)lz >= (unsigned)kStsdfBlock) return -1;
  const int slot = nb[(cx * 3 + cy) * 3 + cz];
  return slot < 0 ? -1 : (int64_t)slot * kStsdfBlockVoxels + ts_index(kStsdfBlock, lx, ly, lz);
}
// item 6: the stored tsdf, 0 in an absent block
PG_HD float sts_tsdf(const StsBlock& B, int x, int y, int z) {
  const int64_t at = sts_at(B.nb, x, y, z);
  return at < 0 ? 0.0f : B.tsdf[at];
}
PG_HD int64_t sts_color_at(int64_t at, int k) {
  return ((at / kStsdfBlockVoxels) * 3 + k) * kStsdfBlockVoxels + at % kStsdfBlockVoxels;
}

// the axes (bit i) along which local voxel (x, y, z) emits a point: items 2 and 3, ts_usable and the test of ts_edges without its border
PG_HD int sts_edges(const StsBlock& B, int x, int y, int z) {
  const int64_t at = sts_at(B.nb, x, y, z);
  if (at < 0) return 0;
  const float f0 = B.tsdf[at];
  if (!ts_usable(B.weight[at], f0) || f0 == 0.0f) return 0;
  int mask = 0;
  for (int i = 0; i < 3; i++) {
    const int64_t to = sts_at(B.nb, x + (i == 0), y + (i == 1), z + (i == 2));
    if (to < 0) continue;
    const float f1 = B.tsdf[to];
    if (ts_usable(B.weight[to], f1) && f1 != 0.0f && (f0 < 0.0f) != (f1 < 0.0f)) mask |= 1 << i;
  }
  return mask;
}

// T(q) of ts_trilinear in block-local coordinates, the eight reads through the neighbour table
PG_HD double sts_trilinear(const StsBlock& B, const double* q) {
#pragma clang fp contract(off)
  int i[3];
  double r[3], s[3];
  for (int a = 0; a < 3; a++) {
    const double g = q[a] / B.vl - 0.5;
    const double fl = floor(g);
    i[a] = (int)fl, r[a] = g - fl, s[a] = 1.0 - r[a];
  }
  const double a00 = s[2] * (double)sts_tsdf(B, i[0], i[1], i[2]), b00 = r[2] * (double)sts_tsdf(B, i[0], i[1], i[2] + 1);
  const double a01 = s[2] * (double)sts_tsdf(B, i[0], i[1] + 1, i[2]), b01 = r[2] * (double)sts_tsdf(B, i[0], i[1] + 1, i[2] + 1);
  const double a10 = s[2] * (double)sts_tsdf(B, i[0] + 1, i[1], i[2]), b10 = r[2] * (double)sts_tsdf(B, i[0] + 1, i[1], i[2] + 1);
  const double a11 = s[2] * (double)sts_tsdf(B, i[0] + 1, i[1] + 1, i[2]), b11 = r[2] * (double)sts_tsdf(B, i[0] + 1, i[1] + 1, i[2] + 1);
  const double z00 = a00 + b00, z01 = a01 + b01, z10 = a10 + b10, z11 = a11 + b11;
  const double c0 = s[1] * z00, d0 = r[1] * z01, c1 = s[1] * z10, d1 = r[1] * z11;
  const double y0 = c0 + d0, y1 = c1 + d1;
  const double e0 = s[0] * y0, e1 = r[0] * y1;
  return e0 + e1;
}

// item 4 for the edge of local voxel (x, y, z) along `axis` (which sts_edges admitted): ts_emit in block-local coordinates
PG_HD void sts_emit(const StsBlock& B, int x, int y, int z, int axis, double* point, double* normal, double* color) {
#pragma clang fp contract(off)
  const int idx[3] = {x, y, z};
  const int64_t at = sts_at(B.nb, x, y, z), to = sts_at(B.nb, x + (axis == 0), y + (axis == 1), z + (axis == 2));
  const double r0 = fabs((double)B.tsdf[at]), r1 = fabs((double)B.tsdf[to]);
  const double sum = r0 + r1;
  double p[3];
  for (int a = 0; a < 3; a++) {
    const double scaled = B.vl * (double)idx[a];
    p[a] = B.vl / 2.0 + scaled;
  }
  const double p1 = p[axis] + B.vl;
  const double m0 = p[axis] * r1, m1 = p1 * r0;
  p[axis] = (m0 + m1) / sum;
  for (int a = 0; a < 3; a++) point[a] = p[a] + B.origin[a];
  if (B.color)
    for (int k = 0; k < 3; k++) {
      const double k0 = (double)B.color[sts_color_at(at, k)] * r1, k1 = (double)B.color[sts_color_at(to, k)] * r0;
      color[k] = (k0 + k1) / sum;
    }
  const double h = 0.99 * B.vl;
  double n[3];
  for (int a = 0; a < 3; a++) {
    double hi[3] = {p[0], p[1], p[2]}, lo[3] = {p[0], p[1], p[2]};
    hi[a] = p[a] + h, lo[a] = p[a] - h;
    const double th = sts_trilinear(B, hi), tl = sts_trilinear(B, lo);
    n[a] = th - tl;
  }
  const double xx = n[0] * n[0], yy = n[1] * n[1], zz = n[2] * n[2];
  const double xy = xx + yy;
  const double len = pg_sqrt(xy + zz);
  const bool unit = len > 0.0;
  for (int a = 0; a < 3; a++) normal[a] = unit ? n[a] / len : n[a];
}
