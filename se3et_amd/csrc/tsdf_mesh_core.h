// The per-cube text of triangle mesh extraction (csrc/tsdf_mesh.hip carries the contract): a voxel's two bits, a cube's index, the three
// edges a voxel owns that carry a vertex, and the owner of a cube edge.  __host__ __device__ templates over a bit reader B -- B::at(x, y, z)
// answers the bits of a voxel, 0 for one that does not exist -- so that the kernels read rows staged in LDS and the se3_debug_*_mesh_host
// entries read the volume itself through the same text.  A vertex's point, normal and colour are ts_emit / sts_emit, unchanged.
#pragma once
#include "mesh_table.h"
#include "tsdf_sparse_core.h"

constexpr int kMeshTableWidth = 16;            // SE3_MESH_TABLE_WIDTH: entries of a table row, -1 terminated
constexpr int kMeshMaxTriangles = 5;           // SE3_MESH_MAX_TRIANGLES: of one cube
constexpr int kMeshNoLimit = 1 << 30;          // a cube range for volumes without a border (the sparse ones)

// bit 0: observed (weight != 0); bit 1: negative (t < 0.0f, so an exact zero is positive)
PG_HD int tm_bits(float w, float t) { return (w != 0.0f ? 1 : 0) | (t < 0.0f ? 2 : 0); }
PG_HD int tm_popcount3(int mask) { return (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1); }

// corner c of a cube as offsets: c0 (0,0,0) c1 (1,0,0) c2 (1,1,0) c3 (0,1,0), c4 .. c7 the same at z + 1
PG_HD int tm_corner_x(int c) { return ((c + 1) >> 1) & 1; }
PG_HD int tm_corner_y(int c) { return (c >> 1) & 1; }
PG_HD int tm_corner_z(int c) { return (c >> 2) & 1; }
// edge e: its owner (the first corner of the pair) and its axis (the direction to the second): e0 (0,1) e1 (1,2) e2 (3,2) e3 (0,3),
// e4 .. e7 the same at z + 1, e8 (0,4) e9 (1,5) e10 (2,6) e11 (3,7)
PG_HD int tm_edge_owner(int e) { return (int)((0x321047540310ull >> (4 * e)) & 15); }
PG_HD int tm_edge_axis(int e) { return e >= 8 ? 2 : (e & 1); }

// the index of the cube with min corner (x, y, z): bit c set iff corner c is negative.  -1: the cube is not taken, because its min corner
// lies outside [lo, hi]^3 or a corner is unobserved.
template <class B>
PG_HD int tm_cube_index(const B& b, int lo, int hi, int x, int y, int z) {
  if (x < lo || y < lo || z < lo || x > hi || y > hi || z > hi) return -1;
  int index = 0, seen = 1;
  for (int c = 0; c < 8; c++) {
    const int v = b.at(x + tm_corner_x(c), y + tm_corner_y(c), z + tm_corner_z(c));
    seen &= v, index |= ((v >> 1) & 1) << c;
  }
  return seen ? index : -1;
}

// the axes (bit i) along which voxel (x, y, z) owns a vertex: the edge to idx + e_i changes sign and lies in at least one taken cube
template <class B>
PG_HD int tm_vertex_mask(const B& b, int lo, int hi, int x, int y, int z) {
  const int v0 = b.at(x, y, z);
  if (!(v0 & 1)) return 0;
  int mask = 0;
  for (int a = 0; a < 3; a++) {
    const int v1 = b.at(x + (a == 0), y + (a == 1), z + (a == 2));
    if (!(v1 & 1) || !((v0 ^ v1) & 2)) continue;
    bool taken = false;
    for (int k = 0; k < 4 && !taken; k++) {                             // the four cubes around the edge
      int m[3] = {x, y, z};
      m[(a + 1) % 3] -= k & 1, m[(a + 2) % 3] -= k >> 1;
      taken = tm_cube_index(b, lo, hi, m[0], m[1], m[2]) >= 0;
    }
    if (taken) mask |= 1 << a;
  }
  return mask;
}

// the vertices that voxel's mask places before the one on `axis`
PG_HD int tm_rank(int mask, int axis) { return tm_popcount3(mask & ((1 << axis) - 1)); }

// the first position of keys[0, n), ascending, that holds `key` or more
PG_HD int64_t tm_lower_bound(const int64_t* keys, int64_t n, int64_t key) {
  int64_t a = 0, b = n;
  while (a < b) {
    const int64_t m = a + (b - a) / 2;
    if (keys[m] < key) a = m + 1;
    else b = m;
  }
  return a;
}

// ---- bit readers on the volumes themselves (the host entries) ---------------------------------------------------------------------------------
struct TmVolumeBits {
  TsVolume V;
  PG_HD int at(int x, int y, int z) const {
    if ((unsigned)x >= (unsigned)V.R || (unsigned)y >= (unsigned)V.R || (unsigned)z >= (unsigned)V.R) return 0;
    const int64_t i = ts_index(V.R, x, y, z);
    return tm_bits(V.weight[i], V.tsdf[i]);
  }
};
struct TmBlockBits {                           // block-local indices in [-1, 17]; a voxel of an absent block is unobserved
  StsBlock B;
  PG_HD int at(int x, int y, int z) const {
    const int64_t i = sts_at(B.nb, x, y, z);
    return i < 0 ? 0 : tm_bits(B.weight[i], B.tsdf[i]);
  }
};
