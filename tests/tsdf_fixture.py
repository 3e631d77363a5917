"""The cases of the TSDF tests (tests/test_tsdf_cpu.py, tests/test_gpu_tsdf.py): rendered analytic spheres, the deliberate edge cases, the
crafted extraction states, the depth images, and the callers of the library's host entries.  The twin's results are computed once per
case and shared (lru_cache); callers must not write into them.

Sizes: resolutions 13 and 33 (neither a multiple of a tile of 64 z x 4 y), images of 32 x 24 and 31 x 17, 0, 1, 3 and 65 frames (one more
than a table tile of 64), uint16 and float32 depth, colour off, uint8 and float32."""
import ctypes
import functools

import numpy as np

import tsdf_twin as twin

F32 = np.float32
FRAME_TILE = 64

# the twin's worst radial error on the sphere cases, in voxel lengths, measured on the CPU with sphere_error(name) on the committed twin
# (tests/test_tsdf_cpu.py prints the figure again and checks it); the bound of the test is twice this.  Three poses, a truncation of two
# voxel lengths: 203 points at resolution 16 with 32 x 24 images, 841 at 32 with 64 x 48.  The median error is 0.09 voxel lengths; the worst
# points sit at the silhouettes, where a neighbouring ray misses the sphere.
SPHERE_TWIN_ERROR = {'sphere16': 0.5056, 'sphere32': 0.3753}
SPHERES = {'sphere16': dict(R=16, W=32, H=24), 'sphere32': dict(R=32, W=64, H=48)}
SPHERE_CENTER, SPHERE_RADIUS, SPHERE_SIDE = np.array([0.5, 0.5, 0.5]), 0.3, 1.0


def look_at(eye, target=SPHERE_CENTER, up=(0.0, -1.0, 0.0)):
    """world-to-camera (4, 4) float64 of a camera at eye looking at target (z forward, x right, y down)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(-np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    E = np.eye(4)
    E[:3, :3] = np.stack([x, y, z])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def render_sphere(E, K, H, W, center=SPHERE_CENTER, radius=SPHERE_RADIUS):
    """depth along the camera's z in metres (H, W) float64, 0 where the ray misses, and the hit points' unit normals as colours"""
    fx, fy, cx, cy = K
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    c = E[:3, :3] @ np.asarray(center) + E[:3, 3]
    a, b, cc = (d * d).sum(-1), -2.0 * (d @ c), c @ c - radius * radius
    disc = b * b - 4 * a * cc
    lam = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0)
    lam = np.where(lam > 0, lam, 0.0)
    n = (lam[..., None] * d - c) / radius
    return lam, np.where(lam[..., None] > 0, 0.5 + 0.5 * n, 0.0)


def _orbit(F, distance=1.4):
    ang = 2.0 * np.pi * np.arange(F) / max(F, 1) * 0.35 - 0.5
    return [look_at(SPHERE_CENTER + distance * np.array([np.sin(a), 0.25 * np.cos(3 * a), -np.cos(a)])) for a in ang]


def _scene(R, H, W, F, depth='uint16', color=None, origin=(0.0, 0.0, 0.0), trunc_voxels=3.0, mangle=False):
    """F rendered frames of the sphere into a volume of side SPHERE_SIDE at `origin` (the sphere moves with it)"""
    vl = SPHERE_SIDE / R
    K = np.array([0.9 * W, 0.95 * W, W / 2.0 - 0.3, H / 2.0 + 0.2])
    poses = _orbit(F)
    origin = np.asarray(origin, np.float64)
    shift = np.eye(4)
    shift[:3, 3] = -origin
    lam, cols = [], []
    for E in poses:
        a, b = render_sphere(E, K, H, W)
        lam.append(a), cols.append(b)
    lam = np.array(lam).reshape(F, H, W)
    mm = lam * 1000.0
    depths = np.round(mm).astype(np.uint16) if depth == 'uint16' else mm.astype(F32)
    if mangle:                                                          # zeros, NaNs and depths at and beyond depth_trunc among the hits
        flat = depths.reshape(-1)
        hits = np.flatnonzero(flat > 0)
        flat[hits[0::7]] = 0
        flat[hits[1::7]] = np.nan if depth != 'uint16' else 0
        flat[hits[2::7]] = 3000                                        # exactly depth_trunc: zeroed
        flat[hits[3::7]] = 4000
    colors = None
    if color is not None:
        cols = np.array(cols).reshape(F, H, W, 3)
        colors = np.round(cols * 255).astype(np.uint8) if color == 'uint8' else cols.astype(F32)
    return dict(R=R, vl=vl, trunc=trunc_voxels * vl, origin=origin, depths=np.ascontiguousarray(depths), colors=colors,
                table=twin.frame_table(np.array([E @ shift for E in poses]).reshape(F, 4, 4), K), depth_scale=1000.0, depth_trunc=3.0)


def _axis_case():
    """Unit voxels at integer world positions (origin -0.5), one camera along +z through voxel column (6, 6): c_z = z - 2, the principal
    point on pixel (10, 8), depth 1 everywhere.  Column (6, 6) has m = 1, so sdf = 1 - c_z exactly: voxel z = 3 gets tsdf 0, z = 4 gets
    -0.5, z = 5 has sdf = -trunc exactly and is skipped, z <= 2 is not in front of the camera."""
    E = np.eye(4)
    E[:3, 3] = [-6.0, -6.0, -2.0]
    return dict(R=13, vl=1.0, trunc=2.0, origin=np.array([-0.5, -0.5, -0.5]), depths=np.full((1, 24, 32), 1000, np.uint16), colors=None,
                table=twin.frame_table(E[None], [1.0, 1.0, 10.0, 8.0]), depth_scale=1000.0, depth_trunc=3.0)


def edge_pixel_frames():
    """Four frames over the voxels of _axis_case's grid with c_z = 1 on the plane z = 0, fx = 1, c_x = x: u_f = (x + cx) + 0.5.
    Frame 0: voxel x = 0 lands on the smallest u_f >= 0.0001f (pixel 0, admitted); frame 1: one step of 2^-25 below, under 0.0001f (refused); frame 2:
    voxel x = 12 lands one step below f32(32) - 0.0001f (pixel 31, admitted); frame 3: exactly on it (refused).  Frame k's image holds
    depth in column 0 (k < 2) or 31 alone.  Returns the case and the four u_f, which are asserted here."""
    lo = F32(0.0001)
    first = F32(np.ceil(float(lo) * 2.0 ** 25) / 2.0 ** 25)            # u_f = 0.5 - |cx| is a multiple of 2^-25
    hi = F32(32) - F32(0.0001)
    last = np.nextafter(hi, F32(0))
    below = first - F32(2.0 ** -25)                                     # the next u_f down that x = 0 can reach
    cxs = [first - F32(0.5), below - F32(0.5), F32(float(last) - 12.5), F32(float(hi) - 12.5)]
    want = [first, below, last, hi]
    got = [(F32(0) + cxs[0]) + F32(0.5), (F32(0) + cxs[1]) + F32(0.5), (F32(12) + cxs[2]) + F32(0.5), (F32(12) + cxs[3]) + F32(0.5)]
    assert [float(g) for g in got] == [float(w) for w in want] and first >= lo > want[1] and last < hi
    E = np.eye(4)
    E[:3, 3] = [0.0, 0.0, 1.0]
    depths = np.zeros((4, 24, 32), np.uint16)
    depths[:2, :, 0] = 1500
    depths[2:, :, 31] = 1500
    K = np.array([[1.0, 1.0, float(cx), 5.0] for cx in cxs])
    case = dict(R=13, vl=1.0, trunc=2.0, origin=np.array([-0.5, -0.5, -0.5]), depths=depths, colors=None,
                table=twin.frame_table(np.repeat(E[None], 4, 0), K), depth_scale=1000.0, depth_trunc=3.0)
    return case, want


@functools.lru_cache(maxsize=None)
def cases():
    behind = _scene(13, 24, 32, 1)
    flip = np.diag([-1.0, 1.0, -1.0, 1.0])                              # the same camera turned round: the volume is behind it
    behind['table'] = twin.frame_table((flip @ _orbit(1)[0])[None], behind['table'][0, 12:])
    c = {
        'r13_u16_f3': _scene(13, 24, 32, 3),
        'r33_f32_u8color_f3_origin': _scene(33, 17, 31, 3, 'float32', 'uint8', origin=(0.25, -1.0, 2.0)),
        'r13_f0': _scene(13, 24, 32, 0),
        'r13_f0_color': _scene(13, 24, 32, 0, 'uint16', 'uint8'),
        'r13_f32color_f1': _scene(13, 17, 31, 1, 'uint16', 'float32'),
        'r13_u8color_f65': _scene(13, 24, 32, 65, 'uint16', 'uint8', trunc_voxels=2.0),
        'r13_f32_f65_31x17': _scene(13, 17, 31, 65, 'float32'),
        'r33_u16_f3': _scene(33, 24, 32, 3),
        'r13_behind': behind,
        'r13_mangled_f32': _scene(13, 24, 32, 3, 'float32', mangle=True),
        'r13_mangled_u16': _scene(13, 24, 32, 3, 'uint16', 'uint8', mangle=True),
        'axis': _axis_case(),
        'edge_pixels': edge_pixel_frames()[0],
    }
    for name, s in SPHERES.items():
        c[name] = _scene(s['R'], s['H'], s['W'], 3, trunc_voxels=2.0)
    return c


def crafted_states():
    """Extraction states written by hand (the state is plain tensors): name -> (state, vl, origin)."""
    def blank(color=False):
        return twin.new_state(13, color)

    def put(s, idx, t, w=1.0):
        s['tsdf'][idx], s['weight'][idx] = F32(t), F32(w)
    out = {}
    s = blank()                                                         # a lone edge: every other voxel of its normal's stencils is unobserved (0);
    put(s, (3, 3, 3), 0.5), put(s, (4, 3, 3), -0.5)                     # the gradient is exactly zero along y and z
    put(s, (8, 8, 8), 0.25), put(s, (8, 9, 8), -0.75), put(s, (8, 8, 9), -0.125)
    out['lone_edges'] = (s, 0.05, np.zeros(3))
    s = blank()                                                         # +-0.98f: +0.98f is not usable, -0.98f is, and so is one step below +0.98f
    put(s, (3, 3, 3), F32(0.98)), put(s, (4, 3, 3), -0.5)
    put(s, (3, 6, 3), F32(-0.98)), put(s, (4, 6, 3), 0.5)
    put(s, (3, 9, 3), np.nextafter(F32(0.98), F32(0))), put(s, (4, 9, 3), -0.5)
    put(s, (7, 3, 3), np.nextafter(F32(-0.98), F32(-1))), put(s, (8, 3, 3), 0.5)
    out['at_098'] = (s, 0.05, np.array([1.0, 2.0, 3.0]))
    s = blank()                                                         # zeros: 0 and -0 next to a negative and a positive value give no point;
    put(s, (3, 3, 3), 0.0), put(s, (4, 3, 3), -0.5)                     # tiny values whose float product underflows do
    put(s, (3, 6, 3), -0.0), put(s, (4, 6, 3), 0.5)
    put(s, (3, 9, 3), 1e-30), put(s, (4, 9, 3), -1e-30)
    put(s, (7, 7, 7), 0.5, 0.0), put(s, (8, 7, 7), -0.5)                # weight 0: not usable, though its tsdf is read by the normals nearby
    put(s, (8, 8, 7), 0.5)
    out['zeros'] = (s, 0.05, np.zeros(3))
    s = blank()                                                         # the last admissible index: idx + 1 < R - 1
    for x in (10, 11):
        put(s, (x, 5, 5), 0.5), put(s, (x, 5, 6), -0.5)
    put(s, (11, 5, 5), 0.5), put(s, (12, 5, 5), -0.5)                   # x + 1 = 12 = R - 1: no point along x
    put(s, (1, 1, 1), 0.5), put(s, (0, 1, 1), -0.5), put(s, (1, 1, 2), -0.25)
    out['borders'] = (s, 0.05, np.zeros(3))
    s = blank(True)                                                     # a NaN in an unobserved voxel of a stencil: the normal is returned unnormalised
    put(s, (5, 5, 5), 0.5), put(s, (6, 5, 5), -0.25)
    s['tsdf'][6, 6, 5] = np.nan
    s['color'][:, 5, 5, 5], s['color'][:, 6, 5, 5] = [0.25, 0.5, 1.0], [1.0, 0.125, 0.0]
    out['nan_stencil'] = (s, 0.05, np.zeros(3))
    return out


# ---- the library's host entries ---------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _elems(depths, colors):
    return (0 if depths.dtype == np.uint16 else 1), (0 if colors is None else (1 if colors.dtype == np.uint8 else 2))


def host_integrate(case, state=None, frames=slice(None)):
    """se3_debug_tsdf_integrate_host on the case's frames[frames], from `state` (None: a new one); returns the state"""
    from se3et_amd import _lib
    color = case['colors'] is not None
    state = twin.new_state(case['R'], color) if state is None else state
    d = np.ascontiguousarray(case['depths'][frames])
    c = np.ascontiguousarray(case['colors'][frames]) if color else None
    t = np.ascontiguousarray(case['table'][frames])
    de, ce = _elems(d, c)
    o = np.ascontiguousarray(case['origin'], dtype=np.float64)
    _lib.check(_lib.lib().se3_debug_tsdf_integrate_host(_ptr(state['tsdf']), _ptr(state['weight']), _ptr(state['color']), case['R'], case['vl'],
                                                        case['trunc'], _ptr(o), _ptr(d), de, _ptr(c), ce, d.shape[0], d.shape[1], d.shape[2],
                                                        _ptr(t), case['depth_scale'], case['depth_trunc']), 'se3_debug_tsdf_integrate_host')
    return state


def host_extract(state, vl, origin):
    from se3et_amd import _lib
    R = state['tsdf'].shape[0]
    o = np.ascontiguousarray(origin, dtype=np.float64)
    n = ctypes.c_int64(-1)
    args = (_ptr(state['tsdf']), _ptr(state['weight']), _ptr(state['color']), R, float(vl), _ptr(o))
    _lib.check(_lib.lib().se3_debug_tsdf_extract_host(*args, 0, None, None, None, ctypes.byref(n)), 'se3_debug_tsdf_extract_host')
    out = [np.full((n.value, 3), np.nan) for _ in range(3 if state['color'] is not None else 2)]
    m = ctypes.c_int64(-1)
    if n.value:
        _lib.check(_lib.lib().se3_debug_tsdf_extract_host(*args, n.value, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]) if len(out) == 3 else None,
                                                          ctypes.byref(m)), 'se3_debug_tsdf_extract_host')
        assert m.value == n.value
    return out[0], out[1], out[2] if len(out) == 3 else None


def host_depth_points(depth, K, scaling_factor=1000.0, distance_limit=6.0, convention='reference'):
    from se3et_amd import _lib, ops
    d = np.ascontiguousarray(depth)
    k = np.ascontiguousarray(K, dtype=np.float64)
    conv = ops.DEPTH_CONVENTIONS[convention]
    n = ctypes.c_int64(-1)
    args = (_ptr(d), 0 if d.dtype == np.uint16 else 1, d.shape[0], d.shape[1], _ptr(k), float(scaling_factor), float(distance_limit), conv)
    _lib.check(_lib.lib().se3_debug_depth_points_host(*args, 0, None, ctypes.byref(n)), 'se3_debug_depth_points_host')
    out = np.full((n.value, 3), np.nan)
    if n.value:
        _lib.check(_lib.lib().se3_debug_depth_points_host(*args, n.value, _ptr(out), ctypes.byref(n)), 'se3_debug_depth_points_host')
    return out


# ---- references, computed once --------------------------------------------------------------------------------------------------------------
def _frozen(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def twin_state(name):
    c = cases()[name]
    s = twin.integrate(twin.new_state(c['R'], c['colors'] is not None), c['vl'], c['trunc'], c['origin'], c['depths'], c['table'], c['colors'],
                       c['depth_scale'], c['depth_trunc'])
    return {k: _frozen(v) for k, v in s.items()}


@functools.lru_cache(maxsize=None)
def twin_cloud(name):
    c = cases()[name]
    return tuple(_frozen(x) for x in twin.extract(twin_state(name), c['vl'], c['origin']))


@functools.lru_cache(maxsize=None)
def host_state(name):
    return {k: _frozen(v) for k, v in host_integrate(cases()[name]).items()}


@functools.lru_cache(maxsize=None)
def host_cloud(name):
    c = cases()[name]
    return tuple(_frozen(x) for x in host_extract(host_state(name), c['vl'], c['origin']))


def sphere_error(points, vl):
    """the worst radial error of points against the analytic sphere, in voxel lengths"""
    return float(np.max(np.abs(np.linalg.norm(points - SPHERE_CENTER, axis=1) - SPHERE_RADIUS))) / vl


def depth_image(dtype=np.uint16):
    """(24, 32): a slanted plane in mm with zeros, pixels beyond 6 m and (float32) a NaN; non-square intrinsics as (fx, fy, cx, cy)"""
    v, u = np.meshgrid(np.arange(24), np.arange(32), indexing='ij')
    d = (800 + 37 * u + 91 * v + (u * v) % 13).astype(np.float64)
    d[(u + 2 * v) % 5 == 0] = 0
    d = np.where((3 * u + v) % 11 == 0, 6000.0 + 17 * ((u + v) % 9), d)          # 6000 is not beyond the limit, 6017 is
    d = d.astype(dtype)
    if dtype != np.uint16:
        d += F32(0.25)
        d[(u + 2 * v) % 5 == 0] = 0
        d[7, 9] = np.nan
    return d, np.array([585.0, 577.5, 15.25, 11.75])


def same(got, want):
    """equal values (a NaN equals a NaN) and equal sign bits"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True) and \
        np.array_equal(np.signbit(got), np.signbit(want))
