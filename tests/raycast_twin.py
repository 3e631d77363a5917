"""A float64 restatement of the ray casting contract (se3et_amd/tsdf.py, se3et_amd/tsdf_sparse.py, csrc/tsdf_raycast.hip), one ray at a
time in plain Python floats (IEEE doubles: every product and sum rounds on its own).  Written from the contract text; nothing here is
shared with the library.

A model is Dense(state, vl, origin) over a tsdf_twin state, or Sparse(blocks, volume, vl) over a dict (volume, bx, by, bz) -> state of
resolution 16.  cast(model, views, H, W, ...) returns the five maps.  `mistake` models a kernel bug (tests/test_raycast_cpu.py checks
that the cases notice each): 'step' (the step of s not divided by m), 'unobserved' (a crossing taken across an unobserved sample), 'corner'
(the far corner of a stencil read from the block of the near corner)."""
import math

import numpy as np

F32 = np.float32
BLOCK, BIAS = 16, 1 << 18
MAPS = ('depth', 'points', 'normals', 'color', 'mask')


def _mix(r, s, f):
    """T's sum over f[dx][dy][dz]"""
    z = [[s[2] * float(f[dx][dy][0]) + r[2] * float(f[dx][dy][1]) for dy in (0, 1)] for dx in (0, 1)]
    y = [s[1] * z[dx][0] + r[1] * z[dx][1] for dx in (0, 1)]
    return s[0] * y[0] + r[0] * y[1]


def _cell(vl, q):
    i, r, s = [], [], []
    for a in range(3):
        g = q[a] / vl - 0.5
        fl = math.floor(g)
        i.append(fl), r.append(g - fl), s.append(1.0 - (g - fl))
    return i, r, s


class Dense:
    def __init__(self, state, vl, origin):
        self.state, self.vl, self.origin = state, float(vl), [float(x) for x in origin]
        self.R = state['tsdf'].shape[0]
        self.lo, self.hi = 1.5 * self.vl, (float(self.R) - 1.5) * self.vl
        self.color = state['color'] is not None

    def interval(self, ray, lo, hi):
        for a in range(3):
            e, d = ray['e'][a], ray['dir'][a]
            if d == 0.0:
                if not (self.lo <= e <= self.hi):
                    return None
                continue
            ta, tb = (self.lo - e) / d, (self.hi - e) / d
            lo, hi = max(lo, min(ta, tb)), min(hi, max(ta, tb))
            if not lo <= hi:
                return None
        return lo, hi

    def sample(self, ray, q):
        """('voxel', f, w), or ('outside',)"""
        if not all(self.lo <= x <= self.hi for x in q):
            return ('outside',)
        i = tuple(math.floor(x / self.vl) for x in q)
        assert all(1 <= k <= self.R - 2 for k in i)
        return 'voxel', self.state['tsdf'][i], self.state['weight'][i]

    def plane(self, q, k, mistake=None):
        i, r, s = _cell(self.vl, q)
        assert all(0 <= k_ <= self.R - 2 for k_ in i), (i, self.R)
        vol = self.state['tsdf'] if k == 0 else self.state['color'][k - 1]
        return _mix(r, s, vol[i[0]:i[0] + 2, i[1]:i[1] + 2, i[2]:i[2] + 2])


class Sparse:
    def __init__(self, blocks, volume, vl, color):
        self.blocks, self.volume, self.vl, self.origin = blocks, int(volume), float(vl), [0.0, 0.0, 0.0]
        self.L = 16.0 * self.vl
        self.color = bool(color)

    def interval(self, ray, lo, hi):
        return lo, hi

    def _block(self, b):
        if not all(-BIAS <= x < BIAS for x in b):
            return None
        return self.blocks.get((self.volume,) + tuple(int(x) for x in b))

    def sample(self, ray, q):
        """('voxel', f, w), or ('absent', the ray's exit from the block)"""
        i = [math.floor(x / self.vl) for x in q]
        blk = self._block([x // BLOCK for x in i])
        if blk is not None:
            at = tuple(int(x) % BLOCK for x in i)
            return 'voxel', blk['tsdf'][at], blk['weight'][at]
        out = math.inf
        for a in range(3):
            d = ray['dir'][a]
            if d == 0.0:
                continue
            b = float(math.floor(float(i[a]) / 16.0))
            face = self.L * (b + 1.0) if d > 0.0 else self.L * b
            out = min(out, (face - ray['e'][a]) / d)
        return 'absent', out

    def _corner(self, k, idx, near, mistake):
        b = [x // BLOCK for x in idx]
        if mistake == 'corner':
            b = [x // BLOCK for x in near]
        blk = self._block(b)
        if blk is None:
            return 0.0
        at = tuple(x % BLOCK for x in idx)
        return blk['tsdf'][at] if k == 0 else blk['color'][k - 1][at]

    def plane(self, q, k, mistake=None):
        i, r, s = _cell(self.vl, q)
        f = [[[self._corner(k, (i[0] + dx, i[1] + dy, i[2] + dz), i, mistake) for dz in (0, 1)] for dy in (0, 1)] for dx in (0, 1)]
        return _mix(r, s, f)


def ray_of(view, origin, u, v):
    P, (fx, fy, cx, cy) = view[:12].reshape(3, 4), view[12:]
    xr, yr = (float(u) - cx) / fx, (float(v) - cy) / fy
    return dict(dir=[float((P[a][0] * xr + P[a][1] * yr) + P[a][2]) for a in range(3)], e=[float(P[a][3] - origin[a]) for a in range(3)],
                m=math.sqrt((xr * xr + yr * yr) + 1.0))


def point(ray, s):
    return [ray['e'][a] + s * ray['dir'][a] for a in range(3)]


def normal_at(model, q, mistake=None):
    h = 0.99 * model.vl
    n = []
    for a in range(3):
        hi, lo = list(q), list(q)
        hi[a], lo[a] = q[a] + h, q[a] - h
        n.append(model.plane(hi, 0, mistake) - model.plane(lo, 0, mistake))
    length = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    return [x / length for x in n] if length > 0.0 else n


def cast_ray(model, ray, depth_min, depth_max, threshold, trunc, mistake=None):
    """None, or (s*, point, normal, colour or None)"""
    iv = model.interval(ray, float(depth_min), float(depth_max))
    if iv is None:
        return None
    lo, hi = iv
    vl, m = model.vl, ray['m']
    unit = vl / m
    limit = (hi - lo) / unit + 2.0
    s, before, n = lo, None, 0.0                                        # before: (s, f) of an observed positive predecessor
    while n < limit and s <= hi:
        n += 1.0
        got = model.sample(ray, point(ray, s))
        if got[0] == 'voxel' and got[2] >= F32(threshold):
            f = got[1]
            if f <= 0 and before is not None:
                return refine(model, ray, before[0], before[1], s, f, mistake)
            before = (s, f) if f > 0 else None
            step = max(vl, float(f) * trunc)
            s = s + (step if mistake == 'step' else step / m)
        else:
            if mistake != 'unobserved':
                before = None
            ahead = s + (vl if mistake == 'step' else unit)
            s = got[1] if got[0] == 'absent' and got[1] > ahead else ahead
    return None


def refine(model, ray, s0, f0, s1, f1, mistake=None):
    F0, F1 = model.plane(point(ray, s0), 0, mistake), model.plane(point(ray, s1), 0, mistake)
    if not (F0 > 0.0 and F1 <= 0.0):
        F0, F1 = float(f0), float(f1)
    s = ((s1 * F0) - (s0 * F1)) / (F0 - F1)
    s = min(max(s, s0), s1)
    q = point(ray, s)
    color = [F32(model.plane(q, k + 1, mistake)) for k in range(3)] if model.color else None
    return s, [q[a] + model.origin[a] for a in range(3)], normal_at(model, q, mistake), color


def cast(model, views, H, W, depth_min=0.1, depth_max=3.0, threshold=1.0, trunc=None, mistake=None):
    """the maps of the views (F, 16): {'depth', 'points', 'normals', 'color' (None without colour), 'mask'}"""
    views = np.asarray(views, np.float64).reshape(-1, 16)
    F = len(views)
    out = dict(depth=np.zeros((F, H, W), F32), points=np.full((F, H, W, 3), np.nan), normals=np.full((F, H, W, 3), np.nan),
               color=np.zeros((F, H, W, 3), F32) if model.color else None, mask=np.zeros((F, H, W), bool))
    for f in range(F):
        for v in range(H):
            for u in range(W):
                hit = cast_ray(model, ray_of(views[f], model.origin, u, v), depth_min, depth_max, threshold, float(trunc), mistake)
                if hit is None:
                    continue
                out['depth'][f, v, u], out['points'][f, v, u], out['normals'][f, v, u], out['mask'][f, v, u] = F32(hit[0]), hit[1], hit[2], True
                if model.color:
                    out['color'][f, v, u] = hit[3]
    return out
