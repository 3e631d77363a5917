// Open3D's voxel arithmetic, once: the origin of a cloud's voxel grid, the extent check and the cell of a point, as the __host__ __device__
// text that csrc/voxel_downsample.hip (voxel_down_sample) and csrc/mesh_ops.hip (simplify_vertex_clustering) both run.
//   origin o_d = min_d - 0.5 voxel_size; cell i_d = floor((p_d - o_d) / voxel_size): a true division, no reciprocal multiply; an axis may
//   hold fewer than 2^21 cells, so that three indices make a 63-bit key.
#pragma once
#include <math.h>

#include "stack_rows.h"

constexpr double kVoxelAxisCap = 2097152.0;          // 2^21 voxels per axis: three indices make a 63-bit key

PG_HD double vd_origin(double mn, double voxel_size) { return mn - 0.5 * voxel_size; }
PG_HD bool vd_axis_ok(double mx, double org, double voxel_size) { return (mx - org) / voxel_size < kVoxelAxisCap; }
PG_HD unsigned long long vd_cell(double p, double org, double voxel_size) { return (unsigned long long)(long long)floor((p - org) / voxel_size); }
// the table key of voxel_downsample.hip: x in the low bits
PG_HD unsigned long long vd_key(const double* p, const double* org, double voxel_size) {
  unsigned long long key = 0;
  for (int d = 0; d < 3; d++) key |= vd_cell(p[d], org[d], voxel_size) << (21 * d);
  return key;
}
// the same three indices with x in the high bits: integer order is ascending (x, y, z) cell order
PG_HD long long vd_key_xyz(const double* p, const double* org, double voxel_size) {
  return (long long)(vd_cell(p[0], org[0], voxel_size) << 42 | vd_cell(p[1], org[1], voxel_size) << 21 | vd_cell(p[2], org[2], voxel_size));
}
