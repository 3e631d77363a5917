"""The cases of the RGB-D odometry tests (tests/test_rgbd_odometry_cpu.py, tests/test_gpu_rgbd_odometry.py): an analytic scene rendered by
ray casting, the crafted inputs, and the callers of the library's host entry.  The twin's and the host entry's results are computed once
per case and shared (lru_cache); callers must not write into them.

The scene, in the frame of the first camera (z forward, x right, y down): a sphere of radius 0.45 at (0.1, 0, 1.6) in front of the tilted
plane n . p = 2.3, n the unit vector along (0.15, -0.1, 1), both carrying the world-space texture
0.5 + 0.2 sin(17 x + 1) cos(15 y) + 0.15 sin(19 z + 13 x) + 0.1 cos(21 y - 4 z).  Depth is rounded to millimetres, colour to uint8.

Sizes: 32 x 24 (three levels: 16 x 12, 8 x 6), 31 x 17 (odd sides down the pyramid: 15 x 8, 7 x 4), 683 x 3 = one accumulation chunk of
2048 target pixels plus one, and 160 x 120 for the recovered motion."""
import ctypes
import functools

import numpy as np

import rgbd_odometry_twin as twin

F32 = np.float32
SPHERE_CENTER, SPHERE_RADIUS = np.array([0.1, 0.0, 1.6]), 0.45
PLANE_NORMAL, PLANE_OFFSET = np.array([0.15, -0.1, 1.0]) / np.linalg.norm([0.15, -0.1, 1.0]), 2.3
CONVERT = dict(depth_scale=1000.0, depth_trunc=3.0, min_depth=0.0, max_depth=4.0)

# The twin's own error on the committed scene at 160 x 120 against the applied motion of 1.0 degree and 31.6 mm, measured on the CPU with
# motion_error(twin result) on the committed twin (tests/test_rgbd_odometry_cpu.py prints the figures again and checks them): (degrees,
# millimetres).  The bound of the recovered-motion tests is twice this; the condition is that each is below a quarter of the motion.
MOTION_TWIN_ERROR = {'hybrid': (0.09424, 1.5840), 'color': (0.06414, 3.2119)}
# The same for the chained odometry poses of the 6-frame orbit (frame k against frame 0, the worst over k): (degrees, millimetres).
ORBIT_TWIN_ERROR = (0.33511, 5.7971)


def texture(p):
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return 0.5 + 0.2 * np.sin(17 * x + 1) * np.cos(15 * y) + 0.15 * np.sin(19 * z + 13 * x) + 0.1 * np.cos(21 * y - 4 * z)


def rigid(axis, degrees, translation):
    """world-to-camera (4, 4) of a camera turned by `degrees` about `axis` and moved by `translation`"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.radians(degrees)
    X = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + np.sin(t) * X + (1 - np.cos(t)) * X @ X
    E[:3, 3] = translation
    return E


MOTION = rigid((0.2, 1.0, 0.1), 1.0, (0.03, 0.01, 0.0))                 # 1 degree and 31.6 mm: the first camera's frame to the second's


def intrinsics(H, W):
    return np.array([0.94 * W, 0.94 * W, W / 2.0 - 0.5, H / 2.0 - 0.5])


def render(E, K, H, W):
    """(depth along the camera's z in metres (H, W) float64, texture (H, W) float64 in [0.05, 0.95]) of the scene seen through the
    world-to-camera transform E: every ray hits the plane, the sphere in front of it where it is met"""
    fx, fy, cx, cy = K
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    R, t = E[:3, :3], E[:3, 3]
    o = -R.T @ t
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ R                         # R^T applied to every camera ray
    oc = o - SPHERE_CENTER
    a, b, c = (d * d).sum(-1), 2.0 * (d @ oc), oc @ oc - SPHERE_RADIUS ** 2
    disc = b * b - 4 * a * c
    lam_sphere = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
    lam_sphere = np.where(lam_sphere > 0, lam_sphere, np.inf)
    lam_plane = (PLANE_OFFSET - PLANE_NORMAL @ o) / (d @ PLANE_NORMAL)
    lam = np.minimum(lam_sphere, lam_plane)
    return lam, texture(o + lam[..., None] * d)


def frames(poses, H, W, depth='uint16', color='u8rgb'):
    """(depths (F, H, W), colors (F, H, W, 3) or (F, H, W)) of the scene through the poses, in the given forms"""
    K = intrinsics(H, W)
    lam, tex = zip(*[render(E, K, H, W) for E in poses])
    mm = np.round(np.array(lam) * 1000.0)
    depths = mm.astype(np.uint16) if depth == 'uint16' else mm.astype(F32)
    grey = np.round(np.array(tex) * 255.0)
    rgb = np.round(np.stack([np.array(tex), 0.8 * np.array(tex) + 0.1, 0.6 * np.array(tex) + 0.2], -1) * 255.0)
    colors = {'u8rgb': rgb.astype(np.uint8), 'u8grey': grey.astype(np.uint8), 'f32rgb': (rgb / 255.0).astype(F32),
              'f32grey': (grey / 255.0).astype(F32)}[color]
    return np.ascontiguousarray(depths), np.ascontiguousarray(colors)


def _case(H, W, method, iterations, depth='uint16', color='u8rgb', poses=None, pairs=((0, 1),), T0=None, **options):
    poses = [np.eye(4), MOTION] if poses is None else poses
    d, c = frames(poses, H, W, depth, color)
    P = len(pairs)
    return dict(depths=d, colors=c, K=intrinsics(H, W), pairs=[tuple(p) for p in pairs], T0=np.tile(np.eye(4), (P, 1, 1)) if T0 is None else T0,
                method=method, iterations=tuple(iterations), max_depth_diff=0.03, poses=poses, **dict(CONVERT, **options))


def orbit_poses(F=6):
    """F cameras on a short arc about the scene: neighbours differ by about 1 degree and 3 cm"""
    return [rigid((0.2, 1.0, 0.1), 1.0 * k, (0.03 * k, 0.01 * k, 0.002 * k * k)) for k in range(F)]


def _flat(H, W, F, value, K=None, **kw):
    """F frames of constant depth `value[f]` in metres (float32, depth_scale 1) with a smooth float32 grey ramp"""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    depths = np.stack([np.full((H, W), x, F32) if np.isscalar(x) else np.asarray(x, F32) for x in value])
    colors = np.stack([(0.3 + 0.01 * u + 0.02 * v + 0.05 * f).astype(F32) for f in range(F)])
    case = dict(depths=depths, colors=colors, K=np.array([32.0, 32.0, 16.0, 12.0]) if K is None else K, pairs=[(0, 1)], T0=np.eye(4)[None].copy(),
                method='hybrid', iterations=(2,), max_depth_diff=0.03, depth_scale=1.0, depth_trunc=3.0, min_depth=0.0, max_depth=4.0, poses=None)
    case.update(kw)
    return case


def _shifted(tx=0.0, tz=0.0):
    T = np.eye(4)[None].copy()
    T[0, 0, 3], T[0, 2, 3] = tx, tz
    return T


@functools.lru_cache(maxsize=None)
def cases():
    H, W = 24, 32
    step = np.where(np.arange(W)[None, :] < W // 2, 1.0, 2.0) * np.ones((H, 1))
    hole = _case(24, 32, 'hybrid', (2, 2, 2))
    hole['depths'] = hole['depths'].copy()
    hole['depths'][1, 8:13, 10:16] = 0                                  # a hole in the target: NaN depth gradients around it
    zero = _case(24, 32, 'hybrid', (2, 2, 2))
    zero['depths'] = zero['depths'].copy()
    zero['depths'][0] = 0                                               # an all-zero source frame
    c = {
        '32x24_hybrid_u16_u8rgb_l3': _case(24, 32, 'hybrid', (3, 2, 2)),
        '31x17_hybrid_f32_u8grey_l3': _case(17, 31, 'hybrid', (2, 2, 2), 'float32', 'u8grey'),
        '31x17_color_u16_f32rgb_l1': _case(17, 31, 'color', (3,), 'uint16', 'f32rgb'),
        '32x24_color_f32_f32grey_l2': _case(24, 32, 'color', (2, 2), 'float32', 'f32grey'),
        '683x3_hybrid_chunk_plus_one_l1': _case(3, 683, 'hybrid', (2,)),
        '32x24_orbit_shared_l2': _case(24, 32, 'hybrid', (2, 2), poses=orbit_poses(4), pairs=((0, 1), (1, 2), (2, 3), (0, 2), (3, 1))),
        'hole_in_target': hole,
        'zero_source': zero,
        # depth 1 and 2 side by side, moved 4 and 2 pixels to the right: the near half covers the far one (different depths on one pixel)
        'collide_different': _flat(H, W, 2, [step, 2.0], T0=_shifted(tx=4.0 / 32.0), max_depth_diff=5.0),
        # depth 1 seen from 1 further back: the image shrinks to half, two source pixels per target pixel with q_z = 2 exactly
        'collide_equal': _flat(H, W, 2, [1.0, 2.0], T0=_shifted(tz=1.0)),
        # q_x / q_z = u - 0.5 exactly: source column 0 lands on u_t = floor(-0.5 + 0.5) = 0, inside
        'edge_low': _flat(H, W, 2, [1.0, 1.0], T0=_shifted(tx=-1.0 / 64.0)),
        # q_x / q_z = u + 0.5 exactly: source column W - 1 lands on floor(W - 0.5 + 0.5) = W, outside
        'edge_high': _flat(H, W, 2, [1.0, 1.0], T0=_shifted(tx=1.0 / 64.0)),
        # |q_z - d_t| = 0.25 exactly: kept at max_depth_diff 0.25, dropped one step below
        'diff_at_limit': _flat(H, W, 2, [1.0, 1.5], T0=_shifted(tz=0.25), max_depth_diff=0.25),
        'diff_below_limit': _flat(H, W, 2, [1.0, 1.5], T0=_shifted(tz=0.25), max_depth_diff=float(np.nextafter(0.25, 0.0))),
    }
    return c


EXACT_CASES = ['32x24_hybrid_u16_u8rgb_l3', '31x17_hybrid_f32_u8grey_l3', '31x17_color_u16_f32rgb_l1', '32x24_color_f32_f32grey_l2',
               '683x3_hybrid_chunk_plus_one_l1', '32x24_orbit_shared_l2', 'hole_in_target', 'zero_source', 'collide_different', 'collide_equal']
CRAFTED_MAPS = ['collide_different', 'collide_equal', 'edge_low', 'edge_high', 'diff_at_limit', 'diff_below_limit']


@functools.lru_cache(maxsize=None)
def motion_case(method):
    return _case(120, 160, method, (20, 10, 5))


@functools.lru_cache(maxsize=None)
def orbit_case():
    return _case(120, 160, 'hybrid', (20, 10, 5), poses=orbit_poses(6), pairs=tuple((i, i + 1) for i in range(5)))


def motion_error(T, truth):
    """(degrees, millimetres) between a recovered transform and the true one"""
    D = np.asarray(T) @ np.linalg.inv(truth)
    return float(np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))), float(np.linalg.norm(D[:3, 3])) * 1000.0


def truth_of(case, pair):
    s, t = pair
    return case['poses'][t] @ np.linalg.inv(case['poses'][s])


# ---- the twin, once per case ----------------------------------------------------------------------------------------------------------------------
def _frozen(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    return x


def convert_options(case):
    return {k: case[k] for k in CONVERT}


def twin_pyramids_of(case):
    targets = {t for _s, t in case['pairs']}
    levels = len(case['iterations'])
    return [[{k: _frozen(v) for k, v in lv.items()} for lv in twin.prepare_frame(case['depths'][f], case['colors'][f], levels, f in targets,
                                                                              **convert_options(case))] for f in range(len(case['depths']))]


def twin_results_of(case):
    py = twin_pyramids_of(case)
    return [twin.odometry(py[s], py[t], case['K'].tolist(), case['T0'][p], case['method'], case['iterations'], case['max_depth_diff'])
            for p, (s, t) in enumerate(case['pairs'])]


@functools.lru_cache(maxsize=None)
def twin_pyramids(name):
    return twin_pyramids_of(cases()[name])


@functools.lru_cache(maxsize=None)
def twin_results(name):
    return twin_results_of(cases()[name])


# ---- the library's host entry ---------------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def level_shapes(H, W, levels):
    return [(H >> l, W >> l) for l in range(levels)]


def host_run(case, stop='none', stop_level=0):
    """se3_debug_rgbd_odometry_host on a case.  Returns a dict: transforms, success, status, information, correspondences, and the windows
    pyramids (per frame a list of levels of dicts I, D, Ix, Iy, Dx, Dy), maps (P, H W) uint64, sums (P, 29), scales (P, 2)."""
    from se3et_amd import _lib, ops
    d, c = np.ascontiguousarray(case['depths']), np.ascontiguousarray(case['colors'])
    F, H, W = d.shape
    P, L = len(case['pairs']), len(case['iterations'])
    flags = np.zeros(F, np.uint8)
    for _s, t in case['pairs']:
        if 0 <= t < F:                                                  # (a frame outside is the entry's to refuse)
            flags[t] = 1
    pairs = np.ascontiguousarray(np.array(case['pairs'], np.int32).reshape(-1, 2))
    K = np.ascontiguousarray(np.tile(np.asarray(case['K'], np.float64), (P, 1)))
    T0 = np.ascontiguousarray(case['T0'], dtype=np.float64)
    its = np.ascontiguousarray(np.array(case['iterations'], np.int32))
    S = sum(h * w for h, w in level_shapes(H, W, L))
    out = dict(transforms=np.full((P, 4, 4), np.nan), success=np.full(P, 7, np.uint8), status=np.full(P, -1, np.int32),
               information=np.full((P, 6, 6), np.nan), correspondences=np.full(P, -1, np.int64))
    images, maps = np.zeros((twin.IMAGES, F, S), F32), np.full((P, H * W), twin.FREE, np.uint64)
    sums, scales = np.full((P, twin.SUMS), np.nan), np.full((P, 2), np.nan)
    _lib.check(_lib.lib().se3_debug_rgbd_odometry_host(
        _ptr(d), 0 if d.dtype == np.uint16 else 1, _ptr(c), 1 if c.dtype == np.uint8 else 2, 3 if c.ndim == 4 else 1, F, H, W, _ptr(flags), _ptr(pairs),
        _ptr(K), P, _ptr(T0), ops.RGBD_METHODS[case['method']], _ptr(its), L, case['depth_scale'], case['depth_trunc'], case['min_depth'],
        case['max_depth'], case['max_depth_diff'], ops.RGBD_STOPS[stop], stop_level, _ptr(out['transforms']), _ptr(out['success']),
        _ptr(out['status']), _ptr(out['information']), _ptr(out['correspondences']), _ptr(images), _ptr(maps), _ptr(sums), _ptr(scales)),
        'se3_debug_rgbd_odometry_host')
    pyramids, off = [[] for _ in range(F)], 0
    for h, w in level_shapes(H, W, L):
        for f in range(F):
            pyramids[f].append({k: images[i, f, off:off + h * w].reshape(h, w) for i, k in enumerate(('I', 'D', 'Ix', 'Iy', 'Dx', 'Dy'))})
        off += h * w
    out.update(pyramids=pyramids, maps=maps, sums=sums, scales=scales)
    return out


@functools.lru_cache(maxsize=None)
def host_results(name):
    return {k: _frozen(v) for k, v in host_run(cases()[name]).items()}


def same(got, want):
    """equal values (a NaN equals a NaN) and equal sign bits"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True) and \
        np.array_equal(np.signbit(got), np.signbit(want))
