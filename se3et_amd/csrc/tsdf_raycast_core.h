// The per-ray text of ray casting the uniform and the block-sparse TSDF volumes (csrc/tsdf_raycast.hip carries the contract): a pixel's ray,
// its interval, the march, the refinement and the maps at the hit.  One text for both volume types: a volume type is a `field` that knows
// how to sample the nearest voxel, how to read T and a colour plane at a point, and where the march may go.  T's arithmetic (ts_cell,
// ts_mix, ts_trilinear), ts_index and the normal (ts_gradient) are csrc/tsdf_core.h's; the directory is csrc/tsdf_sparse_core.h's.
// __host__ __device__ text that the kernels and the se3_debug_*_raycast_host entries both run; float64, contraction off in every function.
#pragma once
#include "tsdf_sparse_core.h"

constexpr int kRaycastViewWords = kStsdfPoseWords;      // SE3_RAYCAST_VIEW_WORDS: P[3][4] by rows, fx, fy, cx, cy (float64)
constexpr int kRaycastTile = 16;                        // SE3_RAYCAST_TILE: a workgroup is a tile of 16 x 16 pixels
constexpr int kRaycastMaxSteps = 1 << 20;               // SE3_RAYCAST_MAX_STEPS: (depth_max - depth_min) / vl at most

// what every ray of a call shares
struct RcCall {
  double depth_min, depth_max, trunc;         // trunc = sdf_trunc
  float threshold;                            // f32(weight_threshold)
};

// item 1: q_a(s) = e_a + s dir_a, m
struct RcRay {
  double e[3], dir[3], m;
};

PG_HD RcRay rc_ray(const double* view, const double* origin, int u, int v) {
#pragma clang fp contract(off)
  RcRay ray;
  const double fx = view[12], fy = view[13], cx = view[14], cy = view[15];
  const double du = (double)u - cx, dv = (double)v - cy;
  const double xr = du / fx, yr = dv / fy;
  for (int a = 0; a < 3; a++) {
    const double px = view[4 * a] * xr, py = view[4 * a + 1] * yr;
    const double sum = px + py;
    ray.dir[a] = sum + view[4 * a + 2];
    ray.e[a] = view[4 * a + 3] - origin[a];
  }
  const double xx = xr * xr, yy = yr * yr;
  const double rr = xx + yy;
  ray.m = pg_sqrt(rr + 1.0);
  return ray;
}

PG_HD void rc_point(const RcRay& ray, double s, double* q) {
#pragma clang fp contract(off)
  for (int a = 0; a < 3; a++) {
    const double along = s * ray.dir[a];
    q[a] = ray.e[a] + along;
  }
}

// the intersection of [*lo, *hi] with the ray's stay inside the slab [a, b] of one axis (items 2 and 4); false: empty
PG_HD bool rc_slab(double e, double dir, double a, double b, double* lo, double* hi) {
#pragma clang fp contract(off)
  if (dir == 0.0) return e >= a && e <= b;
  const double da = a - e, db = b - e;
  const double ta = da / dir, tb = db / dir;
  const double t0 = ta < tb ? ta : tb, t1 = ta < tb ? tb : ta;
  if (t0 > *lo) *lo = t0;
  if (t1 < *hi) *hi = t1;
  return *lo <= *hi;
}

enum { kRcOutside = 0, kRcVoxel = 1, kRcAbsent = 2 };

// ---- the uniform volume as a field -----------------------------------------------------------------------------------------------------------
struct RcDense {
  TsVolume V;
  double box_lo, box_hi;                      // 1.5 vl and (R - 1.5) vl: item 2

  PG_HD double vl() const { return V.vl; }
  PG_HD bool color() const { return V.color != nullptr; }
  // item 2: false for an empty interval
  PG_HD bool interval(const RcRay& ray, double* lo, double* hi) const {
    for (int a = 0; a < 3; a++)
      if (!rc_slab(ray.e[a], ray.dir[a], box_lo, box_hi, lo, hi)) return false;
    return *lo <= *hi;
  }
  // the nearest voxel of q.  Only a q whose three computed coordinates lie in [box_lo, box_hi] is read: then q_a / vl is in
  // [1.5 (1 - 2^-52), (R - 1.5) (1 + 2^-52)] and its floor in [1, R - 2] (a slab end that rounding moved by an ulp is the one q that is not).
  PG_HD int sample(const RcRay&, double, const double* q, float* f, float* w, double*) {
#pragma clang fp contract(off)
    int i[3];
    for (int a = 0; a < 3; a++) {
      if (!(q[a] >= box_lo && q[a] <= box_hi)) return kRcOutside;
      i[a] = (int)floor(q[a] / V.vl);
    }
    const int64_t at = ts_index(V.R, i[0], i[1], i[2]);
    *f = V.tsdf[at], *w = V.weight[at];
    return kRcVoxel;
  }
  // T and the colour planes at a q inside the box, or within 0.99 vl of one along one axis: extraction item 4's argument
  PG_HD double plane(const double* q, int k) {
    if (k == 0) return ts_trilinear(V, q);
    TsVolume C = V;
    C.tsdf = V.color + (int64_t)(k - 1) * V.R * V.R * V.R;
    return ts_trilinear(C, q);
  }
};

PG_HD RcDense rc_dense(const float* tsdf, const float* weight, const float* color, int vol, int R, double vl, const double* origins) {
#pragma clang fp contract(off)
  const int64_t cube = (int64_t)R * R * R;
  RcDense D;
  D.V.tsdf = tsdf + vol * cube, D.V.weight = weight + vol * cube, D.V.color = color ? color + vol * 3 * cube : nullptr;
  D.V.R = R, D.V.vl = vl;
  for (int a = 0; a < 3; a++) D.V.origin[a] = origins[3 * vol + a];
  D.box_lo = 1.5 * vl, D.box_hi = ((double)R - 1.5) * vl;
  return D;
}

// ---- the block-sparse volume as a field ------------------------------------------------------------------------------------------------------
struct RcSparse {
  const float *tsdf, *weight, *colors;        // the storage
  const int64_t* keys;
  const int* slots;
  int64_t num_blocks, num_slots;
  int vol;
  double voxel, L;
  int cached[3], cached_slot;                 // the one-block cache: the block looked up last and its slot (-1: absent)
  bool cache_valid;

  PG_HD double vl() const { return voxel; }
  PG_HD bool color() const { return colors != nullptr; }
  PG_HD bool interval(const RcRay&, double*, double*) const { return true; }          // item 3: [depth_min, depth_max]

  // the slot of block b, -1 where absent.  A slot outside the storage counts as absent, so no directory can make a read leave it.
  PG_HD int slot_of(int bx, int by, int bz) {
    if (cache_valid && bx == cached[0] && by == cached[1] && bz == cached[2]) return cached_slot;
    const int64_t at = sts_find(keys, num_blocks, sts_key(vol, bx, by, bz));
    int slot = at < 0 ? -1 : slots[at];
    if (slot < 0 || slot >= num_slots) slot = -1;
    cached[0] = bx, cached[1] = by, cached[2] = bz, cached_slot = slot, cache_valid = true;
    return slot;
  }
  // where global voxel (x, y, z) lies in the storage, -1 in an absent block or outside the key's range.  The local index is three times
  // four bits, so the result is in [0, 4096 num_slots).
  PG_HD int64_t voxel_at(int64_t x, int64_t y, int64_t z) {
    const int64_t bx = x >> 4, by = y >> 4, bz = z >> 4;
    if (bx < -kStsdfBias || bx >= kStsdfBias || by < -kStsdfBias || by >= kStsdfBias || bz < -kStsdfBias || bz >= kStsdfBias) return -1;
    const int slot = slot_of((int)bx, (int)by, (int)bz);
    return slot < 0 ? -1 : (int64_t)slot * kStsdfBlockVoxels + ts_index(kStsdfBlock, (int)(x & 15), (int)(y & 15), (int)(z & 15));
  }
  // item 3: the nearest voxel; in an absent block *next is the ray's exit from it (item 4)
  PG_HD int sample(const RcRay& ray, double s, const double* q, float* f, float* w, double* next) {
#pragma clang fp contract(off)
    double fl[3];
    bool range = true;
    const double side = (double)(kStsdfBias * kStsdfBlock);              // 2^22 voxels each way
    for (int a = 0; a < 3; a++) {
      fl[a] = floor(q[a] / voxel);
      range = range && fl[a] >= -side && fl[a] < side;                   // (false for a NaN)
    }
    const int64_t at = range ? voxel_at((int64_t)fl[0], (int64_t)fl[1], (int64_t)fl[2]) : -1;
    if (at >= 0) {
      *f = tsdf[at], *w = weight[at];
      return kRcVoxel;
    }
    double exit = INFINITY;
    for (int a = 0; a < 3; a++) {
      if (ray.dir[a] == 0.0) continue;
      const double b = floor(fl[a] / (double)kStsdfBlock);
      const double face = ray.dir[a] > 0.0 ? L * (b + 1.0) : L * b;
      const double t = (face - ray.e[a]) / ray.dir[a];
      if (t < exit) exit = t;
    }
    *next = exit;
    (void)s;
    return kRcAbsent;
  }
  PG_HD float corner(int k, int64_t x, int64_t y, int64_t z) {
    const int64_t at = voxel_at(x, y, z);
    if (at < 0) return 0.0f;
    return k == 0 ? tsdf[at] : colors[sts_color_at(at, k - 1)];
  }
  // T and the colour planes in global coordinates, the corners through the directory, 0 in an absent block (contract C, item 6)
  PG_HD double plane(const double* q, int k) {
#pragma clang fp contract(off)
    int64_t i[3];
    double r[3], s[3];
    const double side = (double)(kStsdfBias * kStsdfBlock) + 2.0;
    for (int a = 0; a < 3; a++) {
      double fl;
      ts_cell(voxel, q[a], &fl, &r[a], &s[a]);
      if (!(fl >= -side && fl < side)) return 0.0;                       // every corner outside the key's range
      i[a] = (int64_t)fl;
    }
    const int64_t x = i[0], y = i[1], z = i[2];
    return ts_mix(r, s, corner(k, x, y, z), corner(k, x, y, z + 1), corner(k, x, y + 1, z), corner(k, x, y + 1, z + 1), corner(k, x + 1, y, z),
                  corner(k, x + 1, y, z + 1), corner(k, x + 1, y + 1, z), corner(k, x + 1, y + 1, z + 1));
  }
};

PG_HD RcSparse rc_sparse(const float* tsdf, const float* weight, const float* color, const int64_t* keys, const int* slots, int64_t num_blocks,
                         int64_t num_slots, int vol, double vl) {
  RcSparse S;
  S.tsdf = tsdf, S.weight = weight, S.colors = color, S.keys = keys, S.slots = slots, S.num_blocks = num_blocks, S.num_slots = num_slots;
  S.vol = vol, S.voxel = vl, S.L = sts_block_length(vl);
  S.cached[0] = S.cached[1] = S.cached[2] = 0, S.cached_slot = -1, S.cache_valid = false;
  return S;
}

// ---- the march ---------------------------------------------------------------------------------------------------------------------------------
struct RcHit {
  double s, point[3], normal[3];
  float color[3];
};

template <class Field>
struct RcPlane {
  Field& field;
  PG_HD double operator()(const double* q) const { return field.plane(q, 0); }
};

// items 5 and 6 for the crossing between (s0, f0) and (s1, f1)
template <class Field>
PG_HD void rc_refine(Field& field, const RcRay& ray, const double* origin, double s0, float f0, double s1, float f1, bool want_normal,
                     bool want_color, RcHit* hit) {
#pragma clang fp contract(off)
  double q0[3], q1[3], q[3];
  rc_point(ray, s0, q0), rc_point(ray, s1, q1);
  double F0 = field.plane(q0, 0), F1 = field.plane(q1, 0);
  if (!(F0 > 0.0 && F1 <= 0.0)) F0 = (double)f0, F1 = (double)f1;
  const double a = s1 * F0, b = s0 * F1;
  const double num = a - b, den = F0 - F1;
  double s = num / den;
  if (s < s0) s = s0;                                                   // (rounding alone can leave [s0, s1]: the contract, item 5)
  if (s > s1) s = s1;
  hit->s = s;
  rc_point(ray, s, q);
  for (int k = 0; k < 3; k++) hit->point[k] = q[k] + origin[k];
  if (want_normal) ts_gradient(RcPlane<Field>{field}, field.vl(), q, hit->normal);
  if (want_color)
    for (int k = 0; k < 3; k++) hit->color[k] = (float)field.plane(q, k + 1);
}

// items 2 to 6 for one ray; false: no hit
template <class Field>
PG_HD bool rc_cast(Field& field, const RcRay& ray, const RcCall& call, const double* origin, bool want_normal, bool want_color, RcHit* hit) {
#pragma clang fp contract(off)
  double lo = call.depth_min, hi = call.depth_max;
  if (!field.interval(ray, &lo, &hi)) return false;
  const double vl = field.vl();
  const double unit = vl / ray.m;
  const double limit = (hi - lo) / unit + 2.0;                          // each step advances s by unit at least: item 4
  double s = lo, s_prev = 0.0;
  float f_prev = 0.0f;
  bool positive = false;                                                // the predecessor was observed with f > 0
  for (double n = 0.0; n < limit && s <= hi; n += 1.0) {
    double q[3], next = 0.0;
    float f = 0.0f, w = 0.0f;
    rc_point(ray, s, q);
    const int kind = field.sample(ray, s, q, &f, &w, &next);
    if (kind == kRcVoxel && w >= call.threshold) {
      if (f <= 0.0f && positive) {
        rc_refine(field, ray, origin, s_prev, f_prev, s, f, want_normal, want_color, hit);
        return true;
      }
      positive = f > 0.0f, s_prev = s, f_prev = f;
      const double along = (double)f * call.trunc;
      const double step = along > vl ? along : vl;
      s = s + step / ray.m;
    } else {
      positive = false;
      const double ahead = s + unit;
      s = kind == kRcAbsent && next > ahead ? next : ahead;
    }
  }
  return false;
}

// what a pixel without a hit holds
PG_HD void rc_store(bool ok, const RcHit& hit, int64_t pixel, float* depth, double* points, double* normals, float* colors, uint8_t* mask) {
  if (depth) depth[pixel] = ok ? (float)hit.s : 0.0f;
  if (mask) mask[pixel] = ok ? 1 : 0;
  for (int k = 0; k < 3; k++) {
    if (points) points[3 * pixel + k] = ok ? hit.point[k] : (double)NAN;
    if (normals) normals[3 * pixel + k] = ok ? hit.normal[k] : (double)NAN;
    if (colors) colors[3 * pixel + k] = ok ? hit.color[k] : 0.0f;
  }
}
