// The per-pixel and per-pair arithmetic of RGB-D odometry (csrc/rgbd_odometry.hip carries the contract): the conversion of a raw depth and
// colour pixel, the taps of the Gaussian, the 2 x 2 mean and the Sobel filter, the warp of a source pixel with its z-buffer key, the terms
// of the three kinds of sum over a pair's correspondences, the fold of a chunk and of a pair's chunks, and the solve with its update.
// __host__ __device__ text that the kernels and se3_debug_rgbd_odometry_host both run; preparation is float32, everything after it
// float64, contraction off in every function.  The sums, the Cholesky solve, the sine, the cosine and the composition are icp_core.h's.
#pragma once
#include <math.h>
#include <stdint.h>

#include "icp_core.h"

constexpr int kRgbdMaxLevels = 4;              // SE3_RGBD_MAX_LEVELS
constexpr int kRgbdMaxImage = 8192;            // SE3_RGBD_MAX_IMAGE
constexpr int kRgbdMinSide = 3;                // SE3_RGBD_MIN_SIDE: the smallest side of the coarsest level
constexpr int kRgbdChunk = 2048;               // SE3_RGBD_CHUNK: target pixels per accumulation chunk
constexpr int kRgbdSums = 29;                  // SE3_RGBD_SUMS: 21 of J^T J, 6 of J^T r, the squared residual, the count
constexpr int kRgbdImages = 6;                 // SE3_RGBD_IMAGES: intensity, depth, and the Sobel images Ix, Iy, Dx, Dy
constexpr int kRgbdHybrid = 0, kRgbdColor = 1;                                  // enum se3_rgbd_method
constexpr int kRgbdSumNorm = 0, kRgbdSumStep = 1, kRgbdSumInfo = 2;             // what a sum over the correspondences collects
constexpr uint64_t kRgbdFree = ~0ull;          // a target pixel that no source pixel has claimed
constexpr double kRgbdWeightDepth = 0.9746794344808963;                         // sqrt(0.95), correctly rounded
constexpr double kRgbdWeightColor = 0.22360679774997896;                        // sqrt(0.05), correctly rounded
enum { kRgI = 0, kRgD = 1, kRgIx = 2, kRgIy = 3, kRgDx = 4, kRgDy = 5 };

// ---- preparation: float32 ------------------------------------------------------------------------------------------------------------------
struct RgConvert {
  float scale, trunc, min_depth, max_depth;    // f32 of depth_scale, depth_trunc, min_depth, max_depth
};

PG_HD RgConvert rg_convert(double depth_scale, double depth_trunc, double min_depth, double max_depth) {
  RgConvert c;
  c.scale = (float)depth_scale, c.trunc = (float)depth_trunc, c.min_depth = (float)min_depth, c.max_depth = (float)max_depth;
  return c;
}

// d = f32(raw) / scale; d > trunc makes d = 0; d <= min_depth, d > max_depth and a non-finite d become NaN
PG_HD float rg_depth(const void* depth, int elem, int64_t i, const RgConvert& c) {
#pragma clang fp contract(off)
  const float raw = elem ? ((const float*)depth)[i] : (float)((const uint16_t*)depth)[i];
  float d = raw / c.scale;
  if (d > c.trunc) d = 0.0f;
  if (d <= c.min_depth || d > c.max_depth || !isfinite(d)) d = NAN;
  return d;
}

// color_elem 1: uint8, 2: float32; channels 3 or 1
PG_HD float rg_intensity(const void* color, int elem, int channels, int64_t i) {
#pragma clang fp contract(off)
  if (channels == 1) return elem == 1 ? (float)((const uint8_t*)color)[i] / 255.0f : ((const float*)color)[i];
  float r, g, b;
  if (elem == 1) {
    const uint8_t* p = (const uint8_t*)color + 3 * i;
    r = (float)p[0], g = (float)p[1], b = (float)p[2];
  } else {
    const float* p = (const float*)color + 3 * i;
    r = p[0], g = p[1], b = p[2];
  }
  const float wr = 0.2990f * r, wg = 0.5870f * g, wb = 0.1140f * b;
  const float rg = wr + wg;
  const float s = rg + wb;
  return elem == 1 ? s / 255.0f : s;
}

PG_HD float rg_blur3(float a, float b, float c) {
#pragma clang fp contract(off)
  const float x = 0.25f * a, y = 0.5f * b, z = 0.25f * c;
  const float s = x + y;
  return s + z;
}
PG_HD float rg_mean4(float a, float b, float c, float d) {
#pragma clang fp contract(off)
  const float top = a + b, bottom = c + d;
  const float s = top + bottom;
  return s * 0.25f;
}
PG_HD float rg_sobel_diff(float a, float c) { return c - a; }
PG_HD float rg_sobel_smooth(float a, float b, float c) {
#pragma clang fp contract(off)
  const float twice = 2.0f * b;
  const float s = a + twice;
  return s + c;
}
PG_HD int rg_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// the pyramids of all frames of a call: image `kind` of frame f at level l starts at base + (kind F + f) S + off[l]
struct RgPyramid {
  float* base;
  int64_t F, S, off[kRgbdMaxLevels];
  int levels, H[kRgbdMaxLevels], W[kRgbdMaxLevels];
};

PG_HD RgPyramid rg_pyramid(float* base, int64_t F, int H, int W, int levels) {
  RgPyramid py;
  py.base = base, py.F = F, py.levels = levels, py.S = 0;
  for (int l = 0; l < kRgbdMaxLevels; l++) {
    py.H[l] = l < levels ? H >> l : 0, py.W[l] = l < levels ? W >> l : 0;
    py.off[l] = py.S;
    py.S += (int64_t)py.H[l] * py.W[l];
  }
  return py;
}
PG_HD float* rg_image(const RgPyramid& py, int kind, int64_t f, int l) { return py.base + ((int64_t)kind * py.F + f) * py.S + py.off[l]; }

// ---- correspondences: float64 --------------------------------------------------------------------------------------------------------------
// the pairs of a call, by value: frames and the level-0 intrinsics (fx, fy, cx, cy)
struct RgPairs {
  int src[kPairMaxPairs], tgt[kPairMaxPairs];
  double K[kPairMaxPairs][4];
};

// one pair at one level
struct RgLevel {
  const float* im[2][kRgbdImages];             // [0]: the source frame's images, [1]: the target frame's
  int H, W;
  double K[4];                                 // the level's intrinsics: all four times 2^-l
};

PG_HD RgLevel rg_level(const RgPyramid& py, const RgPairs& pairs, int p, int l) {
#pragma clang fp contract(off)
  RgLevel v;
  for (int k = 0; k < kRgbdImages; k++) v.im[0][k] = rg_image(py, k, pairs.src[p], l), v.im[1][k] = rg_image(py, k, pairs.tgt[p], l);
  v.H = py.H[l], v.W = py.W[l];
  const double s = 1.0 / (double)(1 << l);
  for (int k = 0; k < 4; k++) v.K[k] = pairs.K[p][k] * s;
  return v;
}

// M = K (R K^-1) and K t, in this order: A = R K^-1 with A[a][0] = R[a][0] (1 / fx), A[a][1] = R[a][1] (1 / fy),
// A[a][2] = (R[a][0] (-(cx / fx)) + R[a][1] (-(cy / fy))) + R[a][2]; M[0][b] = fx A[0][b] + cx A[2][b], M[1][b] = fy A[1][b] + cy A[2][b],
// M[2][b] = A[2][b]; Kt = (fx t_x + cx t_z, fy t_y + cy t_z, t_z).  cam[0 .. 8] = M by rows, cam[9 .. 11] = Kt.
PG_HD void rg_camera(const double* K, const double* T, double* cam) {
#pragma clang fp contract(off)
  const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  const double ifx = 1.0 / fx, ify = 1.0 / fy, kx = -(cx / fx), ky = -(cy / fy);
  double A[3][3];
  for (int a = 0; a < 3; a++) {
    A[a][0] = T[4 * a] * ifx, A[a][1] = T[4 * a + 1] * ify;
    const double x = T[4 * a] * kx, y = T[4 * a + 1] * ky;
    const double s = x + y;
    A[a][2] = s + T[4 * a + 2];
  }
  for (int b = 0; b < 3; b++) {
    const double x0 = fx * A[0][b], x2 = cx * A[2][b], y1 = fy * A[1][b], y2 = cy * A[2][b];
    cam[b] = x0 + x2, cam[3 + b] = y1 + y2, cam[6 + b] = A[2][b];
  }
  const double tx = fx * T[3], tz = cx * T[11], ty = fy * T[7], tw = cy * T[11];
  cam[9] = tx + tz, cam[10] = ty + tw, cam[11] = T[11];
}

// Source pixel (u, v) with depth d: q_a = d ((M[a][0] u + M[a][1] v) + M[a][2]) + Kt[a]; kept iff q_z > 0 and the rounded landing
// (floor(q_x / q_z + 0.5), floor(q_y / q_z + 0.5)) lies in the image.  True: *j = the target pixel, *qz = q_z.
PG_HD bool rg_warp(const double* cam, int u, int v, double d, int H, int W, int* j, double* qz) {
#pragma clang fp contract(off)
  double q[3];
  for (int a = 0; a < 3; a++) {
    const double x = cam[3 * a] * (double)u, y = cam[3 * a + 1] * (double)v;
    const double s = x + y;
    const double r = s + cam[3 * a + 2];
    const double m = d * r;
    q[a] = m + cam[9 + a];
  }
  if (!(q[2] > 0.0)) return false;
  const double xu = q[0] / q[2], yv = q[1] / q[2];
  const double ut = floor(xu + 0.5), vt = floor(yv + 0.5);
  if (!(ut >= 0.0 && ut < (double)W && vt >= 0.0 && vt < (double)H)) return false;           // (a NaN fails here)
  *j = (int)vt * W + (int)ut, *qz = q[2];
  return true;
}

// The claim of source pixel s on target pixel j: kept iff the source depth and the target depth are numbers and |q_z - d_t| <=
// max_depth_diff.  The key orders by the high 32 bits of q_z's float64 pattern (q_z > 0: the pattern is monotone), then by s.
PG_HD bool rg_claim(const RgLevel& v, const double* cam, int s, double max_depth_diff, int* j, uint64_t* key) {
#pragma clang fp contract(off)
  const float ds = v.im[0][kRgD][s];
  if (isnan(ds)) return false;
  double qz;
  if (!rg_warp(cam, s % v.W, s / v.W, (double)ds, v.H, v.W, j, &qz)) return false;
  const float dt = v.im[1][kRgD][*j];
  if (isnan(dt)) return false;
  const double diff = fabs(qz - (double)dt);
  if (diff > max_depth_diff || isnan(diff)) return false;
  union { double f; uint64_t u; } bits;
  bits.f = qz;
  *key = (bits.u & 0xffffffff00000000ull) | (uint64_t)(uint32_t)s;
  return true;
}

// ---- the sums over a pair's correspondences -----------------------------------------------------------------------------------------------
// row(g) of the contract for the point (x, y, z) and the gradient (gx, gy), already scaled
PG_HD void rg_row(double gx, double gy, double fx, double fy, double x, double y, double z, double* J) {
#pragma clang fp contract(off)
  const double gfx = gx * fx, gfy = gy * fy;
  const double c0 = gfx / z, c1 = gfy / z;
  const double ax = c0 * x, ay = c1 * y;
  const double c2 = -((ax + ay) / z);
  const double yc2 = y * c2, zc1 = z * c1, zc0 = z * c0, xc2 = x * c2, xc1 = x * c1, yc0 = y * c0;
  J[0] = yc2 - zc1, J[1] = zc0 - xc2, J[2] = xc1 - yc0, J[3] = c0, J[4] = c1, J[5] = c2;
}

PG_HD void rg_add_row(const double* J, double r, double* acc) {
#pragma clang fp contract(off)
  for (int a = 0, e = 0; a < 6; a++)
    for (int b = a; b < 6; b++, e++) {
      const double m = J[a] * J[b];
      acc[e] += m;
    }
  for (int a = 0; a < 6; a++) {
    const double m = J[a] * r;
    acc[21 + a] += m;
  }
  const double rr = r * r;
  acc[27] += rr;
}

// what the correspondence (source pixel s, target pixel j) adds to the sums of `what`.  scale = (a_s, a_t).
PG_HD void rg_term(const RgLevel& v, const double* T, const double* scale, int method, int what, int s, int j, double* acc) {
#pragma clang fp contract(off)
  acc[28] += 1.0;
  const double fx = v.K[0], fy = v.K[1], cx = v.K[2], cy = v.K[3];
  if (what == kRgbdSumNorm) {
    acc[0] += (double)v.im[0][kRgI][s], acc[1] += (double)v.im[1][kRgI][j];
    return;
  }
  if (what == kRgbdSumInfo) {
    const double d = (double)v.im[1][kRgD][j];
    const double xr = ((double)(j % v.W) - cx) / fx, yr = ((double)(j / v.W) - cy) / fy;
    const double px = d * xr, py = d * yr, pz = d;
    const double G[3][6] = {{0.0, pz, -py, 1.0, 0.0, 0.0}, {-pz, 0.0, px, 0.0, 1.0, 0.0}, {py, -px, 0.0, 0.0, 0.0, 1.0}};
    for (int a = 0, e = 0; a < 6; a++)
      for (int b = a; b < 6; b++, e++) {
        const double m0 = G[0][a] * G[0][b], m1 = G[1][a] * G[1][b], m2 = G[2][a] * G[2][b];
        const double m01 = m0 + m1;
        acc[e] += m01 + m2;
      }
    return;
  }
  const double d = (double)v.im[0][kRgD][s];
  const double xr = ((double)(s % v.W) - cx) / fx, yr = ((double)(s / v.W) - cy) / fy;
  const double p[3] = {d * xr, d * yr, d};
  double m[3];
  for (int a = 0; a < 3; a++) {
    const double x = T[4 * a] * p[0], y = T[4 * a + 1] * p[1], z = T[4 * a + 2] * p[2];
    const double xy = x + y;
    const double xyz = xy + z;
    m[a] = xyz + T[4 * a + 3];
  }
  const double wi = method == kRgbdColor ? 1.0 : kRgbdWeightColor;
  double J[6];
  {
    const double sx = 0.125 * (double)v.im[1][kRgIx][j], sy = 0.125 * (double)v.im[1][kRgIy][j];
    rg_row(scale[1] * sx, scale[1] * sy, fx, fy, m[0], m[1], m[2], J);
    for (int a = 0; a < 6; a++) J[a] = wi * J[a];
    const double it = scale[1] * (double)v.im[1][kRgI][j], is = scale[0] * (double)v.im[0][kRgI][s];
    const double diff = it - is;
    rg_add_row(J, wi * diff, acc);
  }
  if (method == kRgbdHybrid) {
    const float fdx = v.im[1][kRgDx][j], fdy = v.im[1][kRgDy][j];
    const double sx = isnan(fdx) ? 0.0 : 0.125 * (double)fdx, sy = isnan(fdy) ? 0.0 : 0.125 * (double)fdy;
    rg_row(sx, sy, fx, fy, m[0], m[1], m[2], J);
    J[0] = J[0] - m[1], J[1] = J[1] + m[0], J[5] = J[5] - 1.0;
    for (int a = 0; a < 6; a++) J[a] = kRgbdWeightDepth * J[a];
    const double diff = (double)v.im[1][kRgD][j] - m[2];
    rg_add_row(J, kRgbdWeightDepth * diff, acc);
  }
}

// Chunk `chunk` of the pair's map at this level: the kRgbdSums partial sums of its kRgbdChunk target pixels in icp_sum's order (lane l adds
// pixels l, l + 256, .. of the chunk, then the halving tree).  Every entry that is read is set free again for the next pass.
template <class Barrier>
PG_HD void rg_chunk_sums(const RgLevel& v, const double* T, const double* scale, int method, int what, uint64_t* map, int chunk,
                         int lane_begin, int lane_end, double* sh, Barrier&& barrier, double* out) {
  const int64_t first = (int64_t)chunk * kRgbdChunk, pixels = (int64_t)v.H * v.W;
  const int64_t n = pixels - first < kRgbdChunk ? pixels - first : kRgbdChunk;
  icp_sum<kRgbdSums>(n, lane_begin, lane_end,
                     [&](int64_t i, double* acc) {
                       const int64_t j = first + i;
                       const uint64_t entry = map[j];
                       if (entry == kRgbdFree) return;
                       map[j] = kRgbdFree;
                       rg_term(v, T, scale, method, what, (int)(uint32_t)entry, (int)j, acc);
                     },
                     sh, barrier, out);
}

// one pair's running state and results; every pointer already points at the pair's own entry
struct RgState {
  double* T;                // (4, 4): the running transform, the result at the end
  double* scale;            // (2): a_s, a_t
  int* status;
  int* done;                // 1: failed and frozen
  double* information;      // (6, 6)
  int64_t* count;
  uint8_t* success;
};

// Before the first pass: T <- T0, everything else cleared; a non-finite T0 or intrinsic fails the pair at once.
PG_HD void rg_pair_init(const RgState& st, const double* T0, const double* K) {
  bool bad = false;
  for (int k = 0; k < 12; k++) bad = bad || !isfinite(T0[k]);
  for (int k = 0; k < 4; k++) bad = bad || !isfinite(K[k]);
  for (int k = 0; k < 16; k++) st.T[k] = k < 12 ? T0[k] : (k == 15 ? 1.0 : 0.0);
  st.scale[0] = 1.0, st.scale[1] = 1.0;
  *st.status = bad ? SE3_RGBD_NONFINITE : 0, *st.done = bad ? 1 : 0;
  for (int k = 0; k < 36; k++) st.information[k] = 0.0;
  *st.count = 0, *st.success = 0;
}

// The fold of a pair's `chunks` partials (icp_sum's order over the chunks: it depends on the level's image size alone) and what follows:
//   kRgbdSumNorm   a_s = 0.5 / (sum I_s / n), a_t likewise; no correspondence fails the pair
//   kRgbdSumStep   the tests of the contract, the solve and T <- M(x) T
//   kRgbdSumInfo   the information matrix and the count; a failed pair gets the identity, a zero matrix and success 0
// Uniform over the lanes; lane 0 writes.  sums_out: NULL, or kRgbdSums doubles that receive the folded sums (the host entry's window).
template <class Barrier>
PG_HD void rg_pair_finish(const RgState& st, int what, const double* partials, int chunks, int lane_begin, int lane_end, double* sh,
                          Barrier&& barrier, double* sums_out) {
#pragma clang fp contract(off)
  const bool done = *st.done != 0;
  double T[16];
  for (int k = 0; k < 16; k++) T[k] = st.T[k];
  int status = *st.status;
  barrier();                                                             // (every lane has read the state lane 0 writes below)
  if (done) {
    if (what == kRgbdSumInfo && lane_begin == 0) {
      icp_identity(st.T);
      for (int k = 0; k < 36; k++) st.information[k] = 0.0;
      *st.count = 0, *st.success = 0;
    }
    return;
  }
  double s[kRgbdSums];
  icp_sum<kRgbdSums>(chunks, lane_begin, lane_end,
                     [&](int64_t i, double* acc) {
                       for (int c = 0; c < kRgbdSums; c++) acc[c] += partials[i * kRgbdSums + c];
                     },
                     sh, barrier, s);
  if (sums_out && lane_begin == 0)
    for (int c = 0; c < kRgbdSums; c++) sums_out[c] = s[c];
  bool finite = true;
  for (int c = 0; c < kRgbdSums; c++) finite = finite && isfinite(s[c]);
  const double n = s[28];
  bool failed = false;
  double Tn[16], scale[2] = {1.0, 1.0};
  if (!finite) {
    status |= SE3_RGBD_NONFINITE, failed = true;
  } else if (what == kRgbdSumNorm) {
    if (!(n > 0.0)) {
      status |= SE3_RGBD_EMPTY, failed = true;
    } else {
      const double ms = s[0] / n, mt = s[1] / n;
      scale[0] = 0.5 / ms, scale[1] = 0.5 / mt;
      if (!isfinite(scale[0]) || !isfinite(scale[1])) status |= SE3_RGBD_NONFINITE, failed = true;
    }
  } else if (what == kRgbdSumStep) {
    double rhs[6], x[6], U[16];
    for (int a = 0; a < 6; a++) rhs[a] = -s[21 + a];
    if (n < 6.0) {
      status |= SE3_RGBD_TOO_FEW, failed = true;
    } else if (!icp_cholesky6(s, rhs, x)) {
      status |= SE3_RGBD_SINGULAR, failed = true;
    } else if (!(fabs(x[0]) < kIcpMaxAngle) || !(fabs(x[1]) < kIcpMaxAngle) || !(fabs(x[2]) < kIcpMaxAngle)) {
      status |= SE3_RGBD_STEP_REFUSED, failed = true;
    } else {
      icp_vector6_to_matrix(x, U);
      icp_compose(U, T, Tn);
    }
  }
  if (lane_begin != 0) return;
  *st.status = status;
  if (failed) {
    *st.done = 1;
    if (what == kRgbdSumInfo) {
      icp_identity(st.T);
      *st.count = 0, *st.success = 0;
    }
    return;
  }
  if (what == kRgbdSumNorm) st.scale[0] = scale[0], st.scale[1] = scale[1];
  if (what == kRgbdSumStep)
    for (int k = 0; k < 16; k++) st.T[k] = Tn[k];
  if (what == kRgbdSumInfo) {
    for (int a = 0, e = 0; a < 6; a++)
      for (int b = a; b < 6; b++, e++) st.information[6 * a + b] = st.information[6 * b + a] = s[e];
    *st.count = (int64_t)n, *st.success = 1;
  }
}
