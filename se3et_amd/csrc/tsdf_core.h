// The per-voxel and per-pixel arithmetic of TSDF fusion and of depth images as clouds (csrc/tsdf.hip carries the contract): a voxel's world
// position, one frame's update of a voxel, the surface test of a voxel edge, the point, colour and normal of an edge, and a pixel's point.
// __host__ __device__ text that the kernels and the se3_debug_tsdf_* / se3_debug_depth_points_host entries both run; integration is
// float32, extraction and the depth points float64, contraction off in every function.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pair_grid.h"

constexpr int kTsdfMinResolution = 4;          // SE3_TSDF_MIN_RESOLUTION
constexpr int kTsdfMaxResolution = 1024;       // SE3_TSDF_MAX_RESOLUTION
constexpr int kTsdfMaxImage = 8192;            // SE3_TSDF_MAX_IMAGE
constexpr int kTsdfMaxTruncVoxels = 64;        // SE3_TSDF_MAX_TRUNC_VOXELS
constexpr int kTsdfFrameTile = 64;             // SE3_TSDF_FRAME_TILE
constexpr int kTsdfFrameWords = 16;            // SE3_TSDF_FRAME_WORDS: E[3][4] by rows, fx, fy, cx, cy
constexpr int kDepthReference = 0, kDepthOpen3d = 1;          // enum se3_depth_convention

// float32 division and square root, rounded to nearest: hipcc's default for `/` and sqrtf on the device, IEEE on the host
PG_HD float ts_div(float a, float b) { return a / b; }
PG_HD float ts_sqrt(float a) { return sqrtf(a); }

// what every frame of a call shares
struct TsImages {
  const void* depth;        // (F, H, W) uint16 (depth_elem 0) or float32 (1)
  const void* color;        // (F, H, W, 3) uint8 (color_elem 1) or float32 (2); color_elem 0: none
  int depth_elem, color_elem, H, W;
  float u_max, v_max;       // f32(W) - 0.0001f, f32(H) - 0.0001f
  float scale, depth_trunc, trunc, inv_trunc;          // f32(depth_scale), f32(depth_trunc), f32(sdf_trunc), 1f / trunc
};

PG_HD TsImages ts_images(const void* depth, int depth_elem, const void* color, int color_elem, int H, int W, double depth_scale,
                         double depth_trunc, double sdf_trunc) {
#pragma clang fp contract(off)
  TsImages im;
  im.depth = depth, im.color = color, im.depth_elem = depth_elem, im.color_elem = color_elem, im.H = H, im.W = W;
  im.u_max = (float)W - 0.0001f, im.v_max = (float)H - 0.0001f;
  im.scale = (float)depth_scale, im.depth_trunc = (float)depth_trunc, im.trunc = (float)sdf_trunc;
  im.inv_trunc = ts_div(1.0f, im.trunc);
  return im;
}

// item 1: w_a = f32((vl / 2 + vl i_a) + o_a), in float64 with one final rounding
PG_HD float ts_world(double vl, int i, double o) {
#pragma clang fp contract(off)
  const double half = vl / 2.0, step = vl * (double)i;
  const double local = half + step;
  return (float)(local + o);
}

// items 2 to 7 for one voxel and one frame: fr = the frame's kTsdfFrameWords words, frame = its index among the call's images.  t, w and
// (with colour) c[3] are the voxel's running state; true when the frame updated it.
PG_HD bool ts_integrate(const float* fr, const TsImages& im, int64_t frame, float wx, float wy, float wz, float* t, float* w, float* c) {
#pragma clang fp contract(off)
  float cam[3];
  for (int a = 0; a < 3; a++) {
    const float ex = fr[4 * a] * wx, ey = fr[4 * a + 1] * wy, ez = fr[4 * a + 2] * wz;
    const float s = ex + ey;
    const float q = s + ez;
    cam[a] = q + fr[4 * a + 3];
  }
  if (!(cam[2] > 0.0f)) return false;
  const float fx = fr[12], fy = fr[13], cx = fr[14], cy = fr[15];
  const float px = cam[0] * fx, py = cam[1] * fy;
  const float qx = ts_div(px, cam[2]), qy = ts_div(py, cam[2]);
  const float sx = qx + cx, sy = qy + cy;
  const float uf = sx + 0.5f, vf = sy + 0.5f;
  if (!(uf >= 0.0001f && uf < im.u_max && vf >= 0.0001f && vf < im.v_max)) return false;
  const int u = (int)uf, v = (int)vf;
  const int64_t pixel = (frame * im.H + v) * im.W + u;
  const float raw = im.depth_elem ? ((const float*)im.depth)[pixel] : (float)((const uint16_t*)im.depth)[pixel];
  float d = ts_div(raw, im.scale);
  if (d >= im.depth_trunc) d = 0.0f;
  if (!(d > 0.0f)) return false;
  const float du = (float)u - cx, dv = (float)v - cy;
  const float xr = ts_div(du, fx), yr = ts_div(dv, fy);
  const float xx = xr * xr, yy = yr * yr;
  const float rr = xx + yy;
  const float m = ts_sqrt(rr + 1.0f);
  const float along = d - cam[2];
  const float sdf = along * m;
  if (!(sdf > -im.trunc)) return false;
  const float scaled = sdf * im.inv_trunc;
  const float tn = scaled < 1.0f ? scaled : 1.0f;
  const float w0 = *w, w1 = w0 + 1.0f;
  const float tw = *t * w0;
  *t = ts_div(tw + tn, w1);
  if (im.color_elem) {
    for (int k = 0; k < 3; k++) {
      const float rgb = im.color_elem == 1 ? ts_div((float)((const uint8_t*)im.color)[3 * pixel + k], 255.0f) : ((const float*)im.color)[3 * pixel + k];
      const float cw = c[k] * w0;
      c[k] = ts_div(cw + rgb, w1);
    }
  }
  *w = w1;
  return true;
}

// ---- extraction --------------------------------------------------------------------------------------------------------------------------
// one volume's state
struct TsVolume {
  const float *tsdf, *weight, *color;          // color NULL: none; channel k at color + k R^3
  int R;
  double vl, origin[3];
};

PG_HD int64_t ts_index(int R, int x, int y, int z) { return ((int64_t)x * R + y) * R + z; }
PG_HD bool ts_usable(float w, float t) { return w != 0.0f && t < 0.98f && t >= -0.98f; }

// the axes (bit i) along which voxel (x, y, z) emits a point: items 1 and 2
PG_HD int ts_edges(const TsVolume& V, int x, int y, int z) {
  const int R = V.R;
  if (x < 1 || y < 1 || z < 1 || x >= R - 1 || y >= R - 1 || z >= R - 1) return 0;
  const int64_t at = ts_index(R, x, y, z);
  const float f0 = V.tsdf[at];
  if (!ts_usable(V.weight[at], f0) || f0 == 0.0f) return 0;
  const int idx[3] = {x, y, z};
  const int64_t stride[3] = {(int64_t)R * R, R, 1};
  int mask = 0;
  for (int i = 0; i < 3; i++) {
    if (!(idx[i] + 1 < R - 1)) continue;
    const float f1 = V.tsdf[at + stride[i]];
    if (ts_usable(V.weight[at + stride[i]], f1) && f1 != 0.0f && (f0 < 0.0f) != (f1 < 0.0f)) mask |= 1 << i;
  }
  return mask;
}

// one axis of T's cell at q: g = q / vl - 0.5, fl = floor(g) (kept as float64: the caller knows its range), r = g - fl, s = 1 - r
PG_HD void ts_cell(double vl, double q, double* fl, double* r, double* s) {
#pragma clang fp contract(off)
  const double g = q / vl - 0.5;
  *fl = floor(g), *r = g - *fl, *s = 1.0 - *r;
}
// T's sum over the eight corner values f[dx][dy][dz], z innermost, every product and sum rounded on its own
PG_HD double ts_mix(const double* r, const double* s, float f000, float f001, float f010, float f011, float f100, float f101, float f110,
                    float f111) {
#pragma clang fp contract(off)
  const double a00 = s[2] * (double)f000, b00 = r[2] * (double)f001;
  const double a01 = s[2] * (double)f010, b01 = r[2] * (double)f011;
  const double a10 = s[2] * (double)f100, b10 = r[2] * (double)f101;
  const double a11 = s[2] * (double)f110, b11 = r[2] * (double)f111;
  const double z00 = a00 + b00, z01 = a01 + b01, z10 = a10 + b10, z11 = a11 + b11;
  const double c0 = s[1] * z00, d0 = r[1] * z01, c1 = s[1] * z10, d1 = r[1] * z11;
  const double y0 = c0 + d0, y1 = c1 + d1;
  const double e0 = s[0] * y0, e1 = r[0] * y1;
  return e0 + e1;
}

// T(q): the trilinear interpolation of the stored tsdf at g = q / vl - 0.5, z innermost.  The eight reads lie inside the volume for every
// q that ts_emit asks for (the argument is with the contract, item 4 of the extraction).
PG_HD double ts_trilinear(const TsVolume& V, const double* q) {
#pragma clang fp contract(off)
  int i[3];
  double r[3], s[3];
  for (int a = 0; a < 3; a++) {
    double fl;
    ts_cell(V.vl, q[a], &fl, &r[a], &s[a]);
    i[a] = (int)fl;
  }
  const float* f = V.tsdf + ts_index(V.R, i[0], i[1], i[2]);
  const int64_t sx = (int64_t)V.R * V.R, sy = V.R;
  return ts_mix(r, s, f[0], f[1], f[sy], f[sy + 1], f[sx], f[sx + 1], f[sx + sy], f[sx + sy + 1]);
}

// item 4 of the extraction at p (without the origin) for any field T: n_a = T(p + h e_a) - T(p - h e_a), h = 0.99 vl, divided by its
// length when that is positive.  ts_emit and the ray casting of csrc/tsdf_raycast_core.h share it.
template <class Field>
PG_HD void ts_gradient(const Field& T, double vl, const double* p, double* normal) {
#pragma clang fp contract(off)
  const double h = 0.99 * vl;
  double n[3];
  for (int a = 0; a < 3; a++) {
    double hi[3] = {p[0], p[1], p[2]}, lo[3] = {p[0], p[1], p[2]};
    hi[a] = p[a] + h, lo[a] = p[a] - h;
    const double th = T(hi), tl = T(lo);
    n[a] = th - tl;
  }
  const double xx = n[0] * n[0], yy = n[1] * n[1], zz = n[2] * n[2];
  const double xy = xx + yy;
  const double len = pg_sqrt(xy + zz);
  const bool unit = len > 0.0;
  for (int a = 0; a < 3; a++) normal[a] = unit ? n[a] / len : n[a];
}
struct TsField {
  const TsVolume& V;
  PG_HD double operator()(const double* q) const { return ts_trilinear(V, q); }
};

// items 3 and 4 for the edge of voxel (x, y, z) along `axis`: the point (origin added), its normal and, where V.color, its colour
PG_HD void ts_emit(const TsVolume& V, int x, int y, int z, int axis, double* point, double* normal, double* color) {
#pragma clang fp contract(off)
  const int R = V.R;
  const int idx[3] = {x, y, z};
  const int64_t at = ts_index(R, x, y, z), step = axis == 0 ? (int64_t)R * R : (axis == 1 ? R : 1), cube = (int64_t)R * R * R;
  const double r0 = fabs((double)V.tsdf[at]), r1 = fabs((double)V.tsdf[at + step]);
  const double sum = r0 + r1;
  double p[3];
  for (int a = 0; a < 3; a++) {
    const double scaled = V.vl * (double)idx[a];
    p[a] = V.vl / 2.0 + scaled;
  }
  const double p1 = p[axis] + V.vl;
  const double m0 = p[axis] * r1, m1 = p1 * r0;
  p[axis] = (m0 + m1) / sum;
  for (int a = 0; a < 3; a++) point[a] = p[a] + V.origin[a];
  if (V.color)
    for (int k = 0; k < 3; k++) {
      const double k0 = (double)V.color[k * cube + at] * r1, k1 = (double)V.color[k * cube + at + step] * r0;
      color[k] = (k0 + k1) / sum;
    }
  ts_gradient(TsField{V}, V.vl, p, normal);
}

// ---- depth images as clouds ----------------------------------------------------------------------------------------------------------------
PG_HD double dp_raw(const void* depth, int elem, int64_t pixel) {
  return elem ? (double)((const float*)depth)[pixel] : (double)((const uint16_t*)depth)[pixel];
}
// is the pixel a row of the output?
PG_HD bool dp_keep(double raw, double scaling, double limit, int convention) {
#pragma clang fp contract(off)
  if (!(raw > 0.0)) return false;
  return convention == kDepthReference || !(raw / scaling > limit);
}
// the pixel's point.  K = (fx, fy, cx, cy).  Reference: the row is the true quotient (row W + u) / W and a far pixel is (0, 0, 0).
PG_HD void dp_point(double raw, int row, int u, int W, const double* K, double scaling, double limit, int convention, double* out) {
#pragma clang fp contract(off)
  double z = raw / scaling;
  if (z > limit) z = 0.0;
  const double v = convention == kDepthReference ? (double)((int64_t)row * W + u) / (double)W : (double)row;
  const double xu = ((double)u - K[2]) * z, yv = (v - K[3]) * z;
  out[0] = xu / K[0], out[1] = yv / K[1], out[2] = z;
}
