"""The cases of the ray casting tests (tests/test_raycast_cpu.py, tests/test_gpu_raycast.py, tests/test_gpu_tracking.py): states written
straight into .tsdf and .weight (the sphere, the random and the exact-zero states of tests/mesh_fixture.py, the 32^3 agreement state of
tests/tsdf_sparse_fixture.py, planes through 2 x 2 x 2 sparse blocks), the cameras, and the callers of the library's host entries.  The
twin's and the host entries' results are computed once per case and shared (lru_cache); callers must not write into them.

Sizes: resolutions 5 (the inner box is two voxels wide), 9, 11, 24 and 32; images of 1 x 1 and 17 x 19 (two tiles each way, both partial);
voxel lengths that are powers of two where a ray has to run exactly along a voxel boundary."""
import functools

import numpy as np

import mesh_fixture as M
import raycast_twin as twin
import tsdf_fixture as U
import tsdf_sparse_fixture as S
import tsdf_sparse_twin as sparse
import tsdf_twin as uniform

F32 = np.float32
_ptr = U._ptr
MAP_NAMES = twin.MAPS
H2, W2 = 17, 19

# The twin's worst hit-depth error on the analytic sphere (case 'sphere_outside': 19 x 17 rays from outside the volume), against the exact
# intersection of each ray with the sphere, in voxel lengths of camera depth, over the pixels that both hit; measured on the CPU on the
# committed twin on 2026-10-21 (tests/test_raycast_cpu.py prints the figure again and checks it).  The host entry is held to twice this.
# The state is the exact distance over three voxel lengths rounded to float32, so the error is that of the trilinear field of a curved
# distance: the median is 0.083 voxel lengths; the worst six (1.08 to 2.39) are rays that graze the silhouette, where depth changes fastest
# with the field and the bracket of two nearest-voxel samples is widest.  123 pixels.
SPHERE_TWIN_ERROR = 2.3943
# The round trip (case 'round_trip': the analytic scene of tests/rgbd_odometry_fixture.py at 32 x 24 integrated from its first pose into a
# sparse volume of 1 / 32 m voxels (sdf_trunc of four, stride 1) and ray-cast at that pose, host entries throughout): the twin's worst |rendered - input| depth over the
# pixels where both exist, in metres, and the share of the pixels with valid input depth that the twin hits.  Measured on 2026-10-21.
# All 768 pixels have input depth and all are hit; the worst pixel (0.63 voxel lengths) lies on the sphere's silhouette.
ROUND_TRIP_TWIN_ERROR = 0.019670
ROUND_TRIP_TWIN_SHARE = 1.0
# The tracker on the 6-frame orbit of tests/rgbd_odometry_fixture.py at 32 x 24 through the host entries (ray cast, odometry, integration):
# the worst pose error against the ground truth over the frames, (degrees, millimetres), with the settings of TRACK below.  Measured on
# 2026-10-21; per frame (0.46, 11.4), (1.22, 17.6), (1.56, 15.5), (0.37, 21.8), (0.97, 23.7): it does not grow along the orbit.
TRACKING_HOST_ERROR = (1.5585, 23.661)


def intrinsics(H, W):
    return np.array([0.9 * W, 0.95 * W, W / 2.0 - 0.3, H / 2.0 + 0.2])


def views_of(extrinsics, K):
    return sparse.pose_table(np.asarray(extrinsics, np.float64).reshape(-1, 4, 4), K)


def axis_view(eye, toward):
    """a camera at `eye` whose z axis is the unit vector `toward` (an axis of the world), x and y the next two axes: P has exact zeros"""
    z = np.asarray(toward, np.float64)
    a = int(np.argmax(np.abs(z)))
    x, y = np.zeros(3), np.zeros(3)
    x[(a + 1) % 3], y[(a + 2) % 3] = 1.0, z[a]
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return np.linalg.inv(P)


def plane_state(R, normal, offset, trunc=3.0, color=False, band=None):
    """tsdf = clip((n . centre - offset) / trunc) in voxel lengths, every voxel observed (band: only those within `band` of the plane)"""
    x, y, z = M._centres(R)
    d = normal[0] * x + normal[1] * y + normal[2] * z - offset
    s = M._state(d, trunc, color)
    if band is not None:
        s['weight'][...] = (np.abs(d) < band).astype(F32)
    return s


def _dense(state, vl, origin, E, H, W, depth_min=0.1, depth_max=3.0, threshold=1.0, trunc_voxels=3.0, K=None):
    K = intrinsics(H, W) if K is None else np.asarray(K, np.float64)
    return dict(kind='dense', state=state, vl=vl, origin=np.asarray(origin, np.float64), color=state['color'] is not None, E=np.asarray(E).reshape(-1, 4, 4),
                K=K, views=views_of(E, K), H=H, W=W, depth_min=depth_min, depth_max=depth_max, threshold=threshold, trunc=trunc_voxels * vl)


def _sparse(blocks, vl, color, E, H, W, volume=0, depth_min=0.1, depth_max=3.0, threshold=1.0, trunc_voxels=3.0, K=None):
    K = intrinsics(H, W) if K is None else np.asarray(K, np.float64)
    return dict(kind='sparse', blocks=blocks, vl=vl, volume=volume, color=color, E=np.asarray(E).reshape(-1, 4, 4), K=K, views=views_of(E, K), H=H, W=W,
                depth_min=depth_min, depth_max=depth_max, threshold=threshold, trunc=trunc_voxels * vl)


ONE = [20.0, 20.0, 0.0, 0.0]                                            # a 1 x 1 image whose one ray is the camera's z axis


def sphere_world():
    state, vl, origin = M.analytic('sphere')
    return origin + vl * np.array(M.SPHERE['center']), vl * M.SPHERE['radius']


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    # ---- uniform volumes
    vl = 0.0625
    up = plane_state(5, (0, 0, 1), 2.7, color=True)                      # positive above z = 2.7 voxels: voxel 3 positive, voxel 2 negative
    o5 = np.array([1.0, 2.0, 3.0])
    c['r5_1x1_axis'] = _dense(up, vl, o5, axis_view(o5 + vl * np.array([2.5, 2.5, 3.4]), (0, 0, -1)), 1, 1, K=ONE, depth_min=0.001)      # dir_x = dir_y = 0, inside
    c['r5_zero_dir_outside'] = _dense(up, vl, o5, axis_view(o5 + vl * np.array([1.25, 2.5, 3.4]), (0, 0, -1)), 1, 1, K=ONE, depth_min=0.001)   # e_x left of the slab
    c['r5_17x19'] = _dense(up, vl, o5, U.look_at(o5 + vl * np.array([2.4, 2.6, 3.45]), o5 + vl * np.array([2.5, 2.5, 0.0])), H2, W2, depth_min=0.001)
    flat = plane_state(9, (0, 0, 1), 4.0)
    # the ray runs along x = 3 vl and y = 5 vl exactly: q_a / vl is integral at every sample
    c['r9_voxel_boundary'] = _dense(flat, vl, np.zeros(3), axis_view(vl * np.array([3.0, 5.0, 7.0]), (0, 0, -1)), 1, 1, K=ONE)
    zero, zvl, zo = M.dense_states()['r9_exact_zero']                   # z = 3 holds exactly 0.0f, below it negative
    c['r9_exact_zero'] = _dense(zero, vl, zo, axis_view(vl * np.array([4.5, 4.5, 7.0]), (0, 0, -1)), 1, 1, K=ONE, depth_min=0.5 * vl)
    c['r9_exact_zero_17x19'] = _dense(zero, vl, zo, U.look_at(vl * np.array([4.4, 4.6, 7.2]), vl * np.array([4.5, 4.5, 0.0])), H2, W2)
    gap = plane_state(9, (0, 0, 1), 4.0)
    gap['weight'][:, :, 4] = 0                                          # the last positive layer unobserved: no crossing may be taken across it
    c['r9_unobserved_between'] = _dense(gap, vl, np.zeros(3), axis_view(vl * np.array([4.5, 4.5, 7.0]), (0, 0, -1)), 1, 1, K=ONE, depth_min=0.5 * vl)
    c['r9_unobserved_between_17x19'] = _dense(gap, vl, np.zeros(3), U.look_at(vl * np.array([4.4, 4.6, 7.2]), vl * np.array([4.5, 4.5, 0.0])), H2, W2)
    c['r9_depth_min_behind'] = _dense(flat, vl, np.zeros(3), axis_view(vl * np.array([4.5, 4.5, 7.0]), (0, 0, -1)), 1, 1, K=ONE, depth_min=3.5 * vl)
    c['r9_depth_max_in_front'] = _dense(flat, vl, np.zeros(3), axis_view(vl * np.array([4.5, 4.5, 7.0]), (0, 0, -1)), 1, 1, K=ONE, depth_min=0.01,
                                        depth_max=2.5 * vl)
    pit = M._state(np.full((9, 9, 9), 1.5))                             # +0.5 everywhere but one voxel: T stays positive beside its centre
    pit['tsdf'][4, 4, 4] = -0.1
    c['r9_bracket_fails'] = _dense(pit, vl, np.zeros(3), axis_view(vl * np.array([4.1, 4.1, 7.75]), (0, 0, -1)), 1, 1, K=ONE, depth_min=0.5 * vl)
    holes = M.random_state(9, 2, False)                                 # weights 0 .. 3
    inside = U.look_at(0.04 * np.array([4.3, 4.6, 4.4]), 0.04 * np.array([9.0, 2.0, 1.0]))
    for t in (0.5, 2.0, 4.0):
        c['r9_random_inside_w%g' % t] = _dense(holes, 0.04, np.zeros(3), inside, H2, W2, depth_min=0.01, threshold=t)
    r11, vl11, o11 = M.dense_states()['r11_color_holes']
    mid = o11 + vl11 * 5.5
    c['r11_color_outside_in'] = _dense(r11, vl11, o11, [U.look_at(mid + np.array([0.3, -0.2, -0.5]), mid), U.look_at(mid + np.array([-0.4, 0.1, 0.3]), mid)],
                                       H2, W2)
    c['r11_looking_away'] = _dense(r11, vl11, o11, U.look_at(mid + np.array([0.3, -0.2, -0.5]), mid + np.array([0.6, -0.4, -1.0])), H2, W2)
    ball, bvl, bo = M.analytic('sphere')
    centre, _ = sphere_world()
    c['sphere_outside'] = _dense(ball, bvl, bo, U.look_at(centre + np.array([0.15, -0.2, -0.85]), centre), H2, W2)
    torus, tvl, to = M.analytic('torus')
    c['torus_inside'] = _dense(torus, tvl, to, U.look_at(np.array([0.49, 0.51, 0.485]), np.array([0.9, 0.6, 0.45])), H2, W2, depth_min=0.02)
    # ---- sparse volumes: vl = 1 / 32, a block is 0.5 m
    svl = 1.0 / 32
    # through the shared corner of 2 x 2 x 2 blocks; a truncation of 12 voxel lengths, so that no value in the band is clipped and T is linear
    diag = plane_state(32, np.ones(3) / np.sqrt(3.0), 48.0 / np.sqrt(3.0), trunc=12.0, color=True, band=9.0)
    eye = np.array([0.31, 0.29, 0.3])
    at_corner = [U.look_at(eye, np.zeros(3)), axis_view([0.25, 0.0, 0.0], (-1, 0, 0)), U.look_at([0.3, 0.3, 0.0], np.zeros(3))]
    # the blocks sit at (-1 .. 0)^3, so the shared corner is the world's origin: crossings on the faces, the edges (the third view looks
    # along the plane z = 0, a block face) and, for the second view's central ray, exactly at the corner
    c['sparse_corner'] = _sparse(M.split_blocks(diag, corner=(-1, -1, -1)), svl, True, at_corner, H2, W2, trunc_voxels=12.0)
    c['sparse_corner_1x1'] = _sparse(M.split_blocks(diag, corner=(-1, -1, -1)), svl, True, axis_view([0.25, 0.0, 0.0], (-1, 0, 0)), 1, 1, K=ONE, trunc_voxels=12.0)
    c['sparse_corner_diagonal_1x1'] = _sparse(M.split_blocks(diag, corner=(-1, -1, -1)), svl, True, U.look_at([0.3, 0.3, 0.3], np.zeros(3)), 1, 1, K=ONE,
                                              trunc_voxels=12.0)
    # the block on the camera's side of the corner absent: the central rays reach the surface without a positive sample
    c['sparse_absent_between'] = _sparse(M.split_blocks(diag, corner=(-1, -1, -1), drop=((1, 1, 1),)), svl, True, at_corner[0], H2, W2, trunc_voxels=12.0)
    c['sparse_absent_only'] = _sparse(M.split_blocks(diag, corner=(-1, -1, -1)), svl, True, at_corner[0], H2, W2, volume=1, trunc_voxels=12.0)
    c['sparse_looking_away'] = _sparse(M.split_blocks(diag, corner=(-1, -1, -1)), svl, True, U.look_at(eye, 2.0 * eye), H2, W2, trunc_voxels=12.0)
    ball_blocks, _, _, _ = M.sparse_states()['corner_sphere']           # blocks at (-1, 3, -2) + (0 .. 1)^3
    bc = svl * (np.array([-16.0, 48.0, -32.0]) + np.array([15.7, 16.4, 16.1]))
    c['sparse_sphere_negative_coords'] = _sparse(ball_blocks, svl, True, [U.look_at(bc + np.array([0.4, 0.3, -0.5]), bc), U.look_at(bc + np.array([-0.5, 0.1, 0.2]), bc)],
                                                 H2, W2, threshold=2.0)
    edge = uniform.new_state(16, False)                                 # the last block of the key's range along x: positive towards the camera
    x, y, z = M._centres(16)
    edge['tsdf'][...] = np.clip((8.0 - x) / 3.0, -1, 1).astype(F32)
    edge['weight'][...] = (y < 8).astype(F32)                           # the rays above pass the block unobserved and leave the key's range
    last = sparse.BIAS - 1
    c['sparse_key_range'] = _sparse({(0, last, 0, 0): edge}, svl, False, axis_view([0.5 * last - 0.4, 0.25, 0.25], (1, 0, 0)), H2, W2)
    s32, b32 = S.agreement_state()
    pose = U.look_at(np.array([0.5, 0.45, 0.75]), np.array([0.5, 0.45, 0.1]))
    c['agreement_dense'] = _dense(s32, S.VL, np.zeros(3), pose, H2, W2, depth_max=0.6)
    c['agreement_sparse'] = _sparse(b32, S.VL, True, pose, H2, W2, depth_max=0.6)
    for t in (2.0, 3.0, 3.5):                                           # the stored weights are 1 + (x + y) % 3: columns of voxels drop out
        c['agreement_dense_w%g' % t] = _dense(s32, S.VL, np.zeros(3), pose, H2, W2, depth_max=0.6, threshold=t)
    return c


DENSE_CASES = [n for n, c in cases().items() if c['kind'] == 'dense']
SPARSE_CASES = [n for n, c in cases().items() if c['kind'] == 'sparse']


def model_of(case):
    if case['kind'] == 'dense':
        return twin.Dense(case['state'], case['vl'], case['origin'])
    return twin.Sparse(case['blocks'], case['volume'], case['vl'], case['color'])


def twin_cast(case, mistake=None):
    return twin.cast(model_of(case), case['views'], case['H'], case['W'], case['depth_min'], case['depth_max'], case['threshold'], case['trunc'], mistake)


# ---- the library's host entries ---------------------------------------------------------------------------------------------------------------
def _outputs(F, H, W, color, maps):
    out = dict(depth=np.full((F, H, W), -1, F32), points=np.full((F, H, W, 3), 7.0), normals=np.full((F, H, W, 3), 7.0),
               color=np.full((F, H, W, 3), -1, F32) if color else None, mask=np.full((F, H, W), 9, np.uint8))
    return {k: (v if k in maps else None) for k, v in out.items()}


def _finish(out):
    if out['mask'] is not None:
        assert set(np.unique(out['mask'])) <= {0, 1}
        out['mask'] = out['mask'].astype(bool)
    return out


def host_cast_dense(state, vl, origin, trunc, views, H, W, depth_min=0.1, depth_max=3.0, threshold=1.0, maps=MAP_NAMES):
    """se3_debug_tsdf_raycast_host: the dict of maps (None for one that was not asked for)"""
    from se3et_amd import _lib
    views = np.ascontiguousarray(views, np.float64).reshape(-1, 16)
    out = _outputs(len(views), H, W, state['color'] is not None, maps)
    o = np.ascontiguousarray(origin, np.float64)
    _lib.check(_lib.lib().se3_debug_tsdf_raycast_host(_ptr(state['tsdf']), _ptr(state['weight']), _ptr(state['color']), state['tsdf'].shape[0], float(vl),
                                                      float(trunc), _ptr(o), _ptr(views), len(views), H, W, float(depth_min), float(depth_max),
                                                      float(threshold), *[_ptr(out[k]) for k in MAP_NAMES]), 'se3_debug_tsdf_raycast_host')
    return _finish(out)


def host_cast_sparse(volumes, volume, vl, trunc, views, H, W, depth_min=0.1, depth_max=3.0, threshold=1.0, maps=MAP_NAMES):
    """se3_debug_stsdf_raycast_host over a tsdf_sparse_fixture.HostVolumes"""
    from se3et_amd import _lib
    views = np.ascontiguousarray(views, np.float64).reshape(-1, 16)
    out = _outputs(len(views), H, W, volumes.color, maps)
    _lib.check(_lib.lib().se3_debug_stsdf_raycast_host(_ptr(volumes.tsdf), _ptr(volumes.weight), _ptr(volumes.colors), _ptr(volumes.keys),
                                                       _ptr(volumes.slots), len(volumes.keys), len(volumes.tsdf), int(volume), float(vl), float(trunc),
                                                       _ptr(views), len(views), H, W, float(depth_min), float(depth_max), float(threshold),
                                                       *[_ptr(out[k]) for k in MAP_NAMES]), 'se3_debug_stsdf_raycast_host')
    return _finish(out)


def host_cast(case, maps=MAP_NAMES):
    args = (case['vl'], case['trunc'], case['views'], case['H'], case['W'], case['depth_min'], case['depth_max'], case['threshold'], maps)
    if case['kind'] == 'dense':
        return host_cast_dense(case['state'], case['vl'], case['origin'], *args[1:])
    return host_cast_sparse(S.HostVolumes(case['color']).put(case['blocks']), case['volume'], *args)


def _frozen(maps):
    for x in maps.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def twin_maps(name):
    return _frozen(twin_cast(cases()[name]))


@functools.lru_cache(maxsize=None)
def host_maps(name):
    return _frozen(host_cast(cases()[name]))


def same_maps(a, b, names=MAP_NAMES):
    """the named maps equal bit for bit (NaNs at the same places)"""
    return all((a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and a[k].dtype == b[k].dtype and U.same(a[k], b[k])) for k in names)


def sphere_depth_error(case, maps):
    """(the worst |depth - exact| over the pixels that hit and that the exact ray meets, in voxel lengths; the number of such pixels)"""
    centre, radius = sphere_world()
    worst, n = 0.0, 0
    for f, view in enumerate(case['views']):
        for v in range(case['H']):
            for u in range(case['W']):
                if not maps['mask'][f, v, u]:
                    continue
                ray = twin.ray_of(view, np.zeros(3), u, v)
                d, e = np.array(ray['dir']), np.array(ray['e']) - centre
                a, b, cc = d @ d, 2.0 * (d @ e), e @ e - radius * radius
                disc = b * b - 4 * a * cc
                if disc <= 0:
                    continue
                exact = (-b - np.sqrt(disc)) / (2 * a)
                worst, n = max(worst, abs(float(maps['depth'][f, v, u]) - exact) / case['vl']), n + 1
    return worst, n


# ---- the round trip and the tracker through the host entries ------------------------------------------------------------------------------------
# two pyramid levels: at 32 x 24 a third one is 8 x 6 pixels, and the recipe left the orbit at frame 4 with it (37 degrees)
TRACK = dict(H=24, W=32, vl=1.0 / 32, trunc=4.0 / 32, stride=1, iterations=(10, 5), max_depth_diff=0.1)


def _rigid_inverse(T):
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = T[:3, :3].T, -(T[:3, :3].T @ T[:3, 3])
    return out


@functools.lru_cache(maxsize=None)
def orbit_frames():
    """(depths (6, 24, 32) uint16, colors (6, 24, 32, 3) uint8, K, the true camera-to-world poses) of tests/rgbd_odometry_fixture.py's orbit"""
    import rgbd_odometry_fixture as O
    E = O.orbit_poses(6)
    d, c = O.frames(E, TRACK['H'], TRACK['W'])
    return d, c, O.intrinsics(TRACK['H'], TRACK['W']), [np.linalg.inv(e) for e in E]


def _integrate_host(volumes, depth, color, pose, K):
    E = _rigid_inverse(pose)[None]
    return volumes.integrate(S._case(depth[None], color[None], E, K, TRACK['trunc'], TRACK['stride'], vl=TRACK['vl']))


def _cast_host(volumes, pose, K, maps=('depth', 'color')):
    return host_cast_sparse(volumes, 0, TRACK['vl'], TRACK['trunc'], views_of(_rigid_inverse(pose)[None], K), TRACK['H'], TRACK['W'], maps=maps)


@functools.lru_cache(maxsize=None)
def round_trip():
    """(the frame's depth in metres (24, 32) float32, the host entries' rendering, the twin's rendering) of orbit frame 0 at its own pose"""
    d, c, K, truth = orbit_frames()
    volumes = _integrate_host(S.HostVolumes(True), d[0], c[0], truth[0], K)
    got = _cast_host(volumes, truth[0], K, MAP_NAMES)
    want = twin.cast(twin.Sparse(volumes.blocks(), 0, TRACK['vl'], True), views_of(_rigid_inverse(truth[0])[None], K), TRACK['H'], TRACK['W'], trunc=TRACK['trunc'])
    return d[0].astype(F32) / F32(1000.0), _frozen(got), _frozen(want)


def round_trip_error(depth, maps):
    """(the worst |rendered - input| over the pixels where both exist, in metres; the share of the pixels with input depth that are hit)"""
    valid = (depth > 0) & (depth < 3.0)
    both = valid & maps['mask'][0]
    return float(np.abs(maps['depth'][0][both].astype(np.float64) - depth[both]).max()), float(both.sum()) / float(valid.sum())


def track_host():
    """the recipe of se3et_amd.tracking.track_and_integrate_rgbd on the orbit through the host entries: (poses, success)"""
    import rgbd_odometry_fixture as O
    d, c, K, truth = orbit_frames()
    volumes, pose, poses, success = S.HostVolumes(True), truth[0].copy(), [], []
    for k in range(len(d)):
        ok = True
        if k:
            model = _cast_host(volumes, pose, K)
            case = dict(depths=np.stack([d[k].astype(F32) / F32(1000.0), model['depth'][0]]), colors=np.stack([c[k].astype(F32) / F32(255.0), model['color'][0]]),
                        K=K, pairs=[(0, 1)], T0=np.eye(4)[None].copy(), method='hybrid', iterations=TRACK['iterations'], max_depth_diff=TRACK['max_depth_diff'],
                        depth_scale=1.0, depth_trunc=3.0, min_depth=0.0, max_depth=4.0)
            found = O.host_run(case)
            ok = bool(found['success'][0])
            if ok:
                pose = pose @ found['transforms'][0]
        if ok:
            _integrate_host(volumes, d[k], c[k], pose, K)
        poses.append(pose.copy()), success.append(ok)
    return poses, success


def pose_error(poses, truth):
    """the worst (degrees, millimetres) of the poses against the true ones"""
    import rgbd_odometry_fixture as O
    errs = [O.motion_error(p, t) for p, t in zip(poses, truth)]
    return max(e[0] for e in errs), max(e[1] for e in errs)
