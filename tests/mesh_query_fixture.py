"""The named cases of the mesh query tests (tests/test_mesh_query_cpu.py, tests/test_gpu_mesh_query.py), the rays and query points cast
against them, and the callers of the library's se3_debug_mesh_*_host entries.  A case is (vertices (n, 3) float64, triangles (m, 3)
int64); results are computed once per case and shared (lru_cache); callers must not write into them.

Sizes: small, because small is where this goes wrong: 1, 2, 12, 100, 200 and 320 triangles, a chain of 74 whose tree is more than 64 levels
deep, the marching-cubes sphere of mesh_ops_fixture (about 1 500), and the four meshes that hold an inert triangle or none at all."""
import functools

import numpy as np

import mesh_ops_fixture
import mesh_query_twin as twin
import tsdf_fixture as U

_ptr = U._ptr
NODE = np.dtype([('lo', '<f8', (3,)), ('hi', '<f8', (3,)), ('left', '<i4'), ('right', '<i4'), ('parent', '<i4'), ('pad', '<i4')])
assert NODE.itemsize == 64
KEYS, TREE = 0, 1


def _tris(rows):
    return np.array(rows, np.int64).reshape(-1, 3)


def _cube():
    """[0.25, 1]^3, twelve triangles: every box of a face has zero thickness; dyadic, so a ray inside a face's plane computes exact zeros"""
    v = np.array([[x, y, z] for x in (0.25, 1.0) for y in (0.25, 1.0) for z in (0.25, 1.0)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, _tris([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])


def _icosphere(levels=2):
    """320 triangles, scaled unevenly and moved off the origin"""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p) / np.linalg.norm(p) for p in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in t:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = out
    return np.array(v) * np.array([1.0, 0.7, 1.3]) + np.array([3.1, -2.2, 0.4]), _tris(t)


ICOSPHERE_CENTER = np.array([3.1, -2.2, 0.4])


def _chain():
    """Centroids whose Morton cells are 0 (eight of them, spread inside the first cell), one single bit 2^j on one axis (63 of them) and the
    far corner of each axis (3): the radix tree peels one key bit a level, so the eight of cell 0 hang more than 64 levels deep, in a subtree
    that splits by position.  Every triangle is tiny (1e-9) around its centroid."""
    cell = 2.0 ** -21
    centres = [np.array([0.05 + 0.1 * (i & 1), 0.05 + 0.1 * (i >> 1 & 1), 0.05 + 0.1 * (i >> 2 & 1)]) * cell for i in range(8)]
    for axis in range(3):
        for j in range(21):
            c = np.full(3, 0.5 * cell)
            c[axis] = (2.0 ** j + 0.5) * cell
            centres.append(c)
        c = np.full(3, 0.5 * cell)
        c[axis] = 1.0
        centres.append(c)
    d = 1e-9
    offsets = np.array([[d, 0, 0], [0, d, 0], [-d, -d, 0.5 * d]])
    v = np.concatenate([c + offsets for c in centres])
    return v, np.arange(3 * len(centres), dtype=np.int64).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(5)
    one = (np.array([[0.1, 0.2, 0.3], [1.3, 0.1, 0.5], [0.4, 1.1, 0.2]]), _tris([(0, 1, 2)]))
    pair_v = np.array([[0.0, 0.0, 0.1], [1.0, 0.1, 0.2], [0.1, 1.0, 0.0], [1.1, 1.2, 0.4]])
    fan = mesh_ops_fixture.cases()['fan_100']
    sv, st, _, _ = mesh_ops_fixture.sphere()
    tri3 = rng.uniform(-1, 1, (3, 3))
    good = rng.uniform(-1, 1, (6, 3))
    nan_v = good.copy()
    nan_v[4, 1] = np.nan
    out = {
        'one': one,
        'edge_pair': (pair_v, _tris([(1, 3, 2), (0, 1, 2)])),              # the edge {1, 2} is shared; the higher centroid has the lower number
        'fan_100': (fan[0].copy(), fan[1].copy()),
        'cube': _cube(),
        'icosphere': _icosphere(),
        'chain': _chain(),
        'coincident_200': (tri3, np.tile(_tris([(0, 1, 2)]), (200, 1))),
        'mc_sphere': (sv.copy(), st.copy()),
        'bad_triangle': (good, _tris([(0, 1, 2), (1, 2, 6), (3, 4, 5), (2, -1, 3)])),
        'nan_vertex': (nan_v, _tris([(0, 1, 2), (3, 4, 5), (2, 3, 5)])),
        'zero_area': (np.concatenate([good[:4], good[:1] + 2 * (good[1:2] - good[:1])]), _tris([(0, 1, 2), (0, 1, 4), (3, 3, 1), (1, 2, 3)])),
        'no_triangles': (good, _tris([])),
    }
    for v, t in out.values():
        v.setflags(write=False), t.setflags(write=False)
    return out


RAISING = ('bad_triangle', 'nan_vertex')               # the cases for which Python raises ValueError


def _extent(v, t):
    live = twin.kinds(v, t) == twin.LIVE
    p = v[t[live]].reshape(-1, 3) if live.any() else np.zeros((1, 3))
    return p.min(0), p.max(0), live


@functools.lru_cache(maxsize=None)
def rays(name):
    """(R, 6): origins inside, outside, on a vertex and 1e6 extents away; aimed at centroids, vertices and edge points of seeded triangles;
    directions of length 1e-30 and 1e30, a zero direction, a NaN direction, a NaN origin; for the cube also the rays of its degenerate
    positions"""
    v, t = cases()[name]
    lo, hi, live = _extent(v, t)
    centre, ext = (lo + hi) / 2, max(float((hi - lo).max()), 1e-3)
    rng = np.random.default_rng(len(name) * 7 + len(t))
    numbers = np.nonzero(live)[0]
    targets = [centre]
    for k in (rng.choice(numbers, min(6, len(numbers)), replace=False) if len(numbers) else []):
        a, b, c = v[t[k]]
        targets += [(a + b + c) / 3, a, (a + b) / 2, b + (c - b) * 0.25, a + (c - a) / 3]
    away = rng.normal(size=3)
    away /= np.linalg.norm(away)
    origins = [centre + 0.013 * ext * rng.normal(size=3), centre + 2.0 * ext * away, centre + 1e6 * ext * away]
    if len(numbers):
        origins.append(v[t[numbers[0], 0]].copy())
    out = []
    for o in origins:
        for p in targets:
            d = p - o
            if np.any(d != 0):
                out.append(np.concatenate([o, d]))
    base = np.array(out[:len(targets)])
    extra = [np.concatenate([r[:3], r[3:] * 1e-30]) for r in base[:4]] + [np.concatenate([r[:3], r[3:] * 1e30]) for r in base[:4]]
    extra += [np.concatenate([base[0][:3], np.zeros(3)]), np.concatenate([base[0][:3], [np.nan, 1.0, 0.0]]),
              np.concatenate([[np.inf, 0.0, 0.0], base[0][3:]])]
    if name == 'cube':
        extra += _cube_rays()
    if name == 'chain':
        extra += [np.concatenate([v[t[k]].mean(0) + np.array([1e-9, -2e-9, 3e-8]), [-1e-9, 2e-9, -3e-8]]) for k in range(8)]
    return np.array(out + extra)


def _cube_rays():
    """inside a face's plane, along an edge, through a corner, with one, two and three zero direction components, and seeded axis-aligned rays
    from origins that are not dyadic (their hits sit at a depth that every vertex of the face shares)"""
    r = [
        (-1.0, 0.5, 1.0, 1.0, 0.0, 0.0), (-1.0, 0.5, 1.0, 1.0, 0.25, 0.0),         # inside the plane z = 1 of a face
        (-1.0, 1.0, 1.0, 1.0, 0.0, 0.0), (0.25, 0.25, -1.0, 0.0, 0.0, 1.0),         # along an edge
        (-0.5, -0.5, -0.5, 1.0, 1.0, 1.0), (2.0, 2.0, 2.0, -1.0, -1.0, -1.0),       # through two corners, no zero component
        (0.5, 0.5, -1.0, 0.0, 0.0, 2.0), (0.625, 0.625, 3.0, 0.0, 0.0, -1.0),       # two zero components; the second through a face's diagonal
        (0.5, -1.0, -1.0, 0.0, 1.0, 1.0), (-1.0, 0.5, 0.5, 1.0, 0.0, 0.25),         # one zero component
        (0.5, 0.5, 0.5, 0.0, 0.0, 1.0), (0.5, 0.5, 0.5, 1.0, 0.0, 0.0),             # from the centre
    ]
    rng = np.random.default_rng(77)
    for _ in range(48):
        axis, sign = int(rng.integers(3)), (1.0, -1.0)[int(rng.integers(2))]
        o = rng.uniform(0.3, 0.95, 3)
        o[axis] = 0.625 - sign * rng.uniform(1.0, 3.0)
        d = np.zeros(3)
        d[axis] = sign * rng.uniform(0.5, 2.0)
        r.append(tuple(o) + tuple(d))
    for _ in range(16):                                                     # along x through the diagonal y = z of the face x = 0.25: a tie
        s_ = rng.uniform(0.3, 0.95)
        r.append((0.25 - rng.uniform(1.0, 3.0), s_, s_, rng.uniform(0.5, 2.0), 0.0, 0.0))
    return [np.array(x) for x in r]


@functools.lru_cache(maxsize=None)
def queries(name):
    """(Q, 3): on a vertex, on an edge, on a face, at the centre, 1e6 extents away, seeded points around the mesh, a NaN"""
    v, t = cases()[name]
    lo, hi, live = _extent(v, t)
    centre, ext = (lo + hi) / 2, max(float((hi - lo).max()), 1e-3)
    rng = np.random.default_rng(len(name) * 11 + len(t))
    numbers = np.nonzero(live)[0]
    out = [centre, centre + 1e6 * ext * np.array([0.3, -0.8, 0.52]), np.array([np.nan, 0.0, 0.0])]
    for k in (rng.choice(numbers, min(5, len(numbers)), replace=False) if len(numbers) else []):
        a, b, c = v[t[k]]
        out += [a, (a + b) / 2, (a + b + c) / 3, b + (c - b) * 0.25, (a + b + c) / 3 + 0.01 * ext * rng.normal(size=3)]
    out += list(centre + ext * rng.uniform(-1, 1, (12, 3)))
    if name == 'chain':                                                     # the eight triangles at the bottom of the chain, each from close by
        out += [v[t[k]].mean(0) + np.array([0.0, 0.0, 2e-9]) for k in range(8)]
    return np.array(out)


# ---- the library's host entries -----------------------------------------------------------------------------------------------------------------------
def _lib():
    from se3et_amd import _lib as L
    return L, L.lib()


def _mesh(v, t):
    return np.ascontiguousarray(v, np.float64), np.ascontiguousarray(t, np.int64)


def sort_order(keys):
    """contract 3: stable by (key < 0, key)"""
    o = np.argsort(keys, kind='stable')
    return o[np.argsort(keys[o] < 0, kind='stable')]


def host_bvh(vertices, tri, order=None):
    """se3_debug_mesh_bvh_host, both passes with the sort between: (nodes (2 max(m, 1),) NODE, counts (4,), keys (m,), order (m,))"""
    L, lib = _lib()
    v, t = _mesh(vertices, tri)
    n, m = len(v), len(t)
    keys, counts = np.full(m, -7, np.int64), np.full(4, -7, np.int64)
    L.check(lib.se3_debug_mesh_bvh_host(KEYS, _ptr(v), _ptr(t), n, m, _ptr(keys), None, None, None, _ptr(counts)), 'bvh_host')
    order = sort_order(keys) if order is None else order
    order = np.ascontiguousarray(order, np.int64)
    sorted_keys = np.ascontiguousarray(keys[order])
    nodes = np.full(2 * max(m, 1) * 8, -7, np.int64).view(NODE)
    L.check(lib.se3_debug_mesh_bvh_host(TREE, _ptr(v), _ptr(t), n, m, None, _ptr(sorted_keys), _ptr(order), _ptr(nodes), _ptr(counts)), 'bvh_host')
    return nodes, counts, keys, order


def _ray_outputs(R):
    return np.full(R, -7.0), np.full(R, -7, np.int64), np.full((R, 2), -7.0), np.full((R, 3), -7.0)


def host_cast(vertices, tri, rays_, t_min=0.0, t_max=np.inf, tree=None):
    """se3_debug_mesh_cast_rays_host (brute force), or with tree=(nodes, counts) se3_debug_mesh_walk_rays_host: (t, ids, uvs, normals, hit)"""
    L, lib = _lib()
    v, t = _mesh(vertices, tri)
    r = np.ascontiguousarray(rays_, np.float64).reshape(-1, 6)
    R = len(r)
    out, hit = _ray_outputs(R), np.full(R, 7, np.uint8)
    head = (_ptr(v), _ptr(t), len(v), len(t)) + (() if tree is None else (_ptr(tree[0]), int(tree[1][3])))
    fn = lib.se3_debug_mesh_cast_rays_host if tree is None else lib.se3_debug_mesh_walk_rays_host
    L.check(fn(*head, _ptr(r), R, float(t_min), float(t_max), 0, *(_ptr(x) for x in out), None), 'cast_rays_host')
    L.check(fn(*head, _ptr(r), R, float(t_min), float(t_max), 1, None, None, None, None, _ptr(hit)), 'cast_rays_host')
    return out + (hit,)


def host_closest(vertices, tri, queries_, tree=None):
    """se3_debug_mesh_closest_points_host (brute force) or se3_debug_mesh_walk_points_host: (points, distances, ids, uvs, normals)"""
    L, lib = _lib()
    v, t = _mesh(vertices, tri)
    q = np.ascontiguousarray(queries_, np.float64).reshape(-1, 3)
    Q = len(q)
    out = np.full((Q, 3), -7.0), np.full(Q, -7.0), np.full(Q, -7, np.int64), np.full((Q, 2), -7.0), np.full((Q, 3), -7.0)
    head = (_ptr(v), _ptr(t), len(v), len(t)) + (() if tree is None else (_ptr(tree[0]), int(tree[1][3])))
    fn = lib.se3_debug_mesh_closest_points_host if tree is None else lib.se3_debug_mesh_walk_points_host
    L.check(fn(*head, _ptr(q), Q, *(_ptr(x) for x in out)), 'closest_points_host')
    return out


def host_render(vertices, tri, views, H, W, depth_min, depth_max):
    """se3_debug_mesh_render_host: (depth, points, normals, primitive_ids, mask)"""
    L, lib = _lib()
    v, t = _mesh(vertices, tri)
    views = np.ascontiguousarray(views, np.float64).reshape(-1, 16)
    F = len(views)
    out = (np.full((F, H, W), -7, np.float32), np.full((F, H, W, 3), -7.0), np.full((F, H, W, 3), -7.0), np.full((F, H, W), -7, np.int64),
           np.full((F, H, W), 7, np.uint8))
    L.check(lib.se3_debug_mesh_render_host(_ptr(v), _ptr(t), len(v), len(t), _ptr(views), F, H, W, float(depth_min), float(depth_max),
                                           *(_ptr(x) for x in out)), 'render_host')
    return out


def same(a, b):
    """bit for bit (NaN equals NaN, -0.0 differs from 0.0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def host_tree(name):
    return host_bvh(*cases()[name])


@functools.lru_cache(maxsize=None)
def host_brute(name):
    """the brute-force host results of a case: (cast, closest)"""
    v, t = cases()[name]
    return host_cast(v, t, rays(name)), host_closest(v, t, queries(name))


def depth_of(nodes, root):
    """the number of inner nodes on the longest path from the root"""
    if root < 0 or nodes[root]['left'] < 0:
        return 0
    best, stack = 0, [(root, 1)]
    while stack:
        i, d = stack.pop()
        best = max(best, d)
        for c in (int(nodes[i]['left']), int(nodes[i]['right'])):
            if nodes[c]['left'] >= 0:
                stack.append((c, d + 1))
    return best


def views_of(eyes, target, fx, fy, cx, cy):
    """(F, 16) views looking from eyes at target: the camera-to-world pose by rows, then the intrinsics"""
    rows = []
    for eye in eyes:
        E = U.look_at(np.asarray(eye, np.float64), np.asarray(target, np.float64))
        P = np.linalg.inv(E)
        rows.append(np.concatenate([P[:3, :].reshape(-1), [fx, fy, cx, cy]]))
    return np.array(rows)


# ---- end to end: the analytic sphere of mesh_fixture as a volume and as its own mesh ----------------------------------------------------------------
# The largest |depth of the ray-cast volume - depth of the rendered mesh| over the pixels where both hit and the mesh's normal is within 60
# degrees of the ray, measured on the CPU with the two host entries se3_debug_tsdf_raycast_host and se3_debug_mesh_render_host
# (tests/test_mesh_query_cpu.py::test_sphere_volume_against_its_mesh prints it again and checks it): 1.0252 voxel lengths over 932 pixels (the volume's
# ray caster marches by nearest-voxel samples and refines between two of them; the mesh is flat between marching-cubes vertices).  Both
# are float64 and deterministic; the GPU test asserts twice this figure, a factor that covers other views of the same sphere only.
END_TO_END = dict(H=24, W=32, depth_min=0.1, depth_max=3.0, trunc_voxels=3.0, eyes=((1.0, -0.5, 1.7), (0.3, -0.8, 2.9), (1.1, 0.3, 2.4)))
END_TO_END_HOST_ERROR = 1.0252          # voxel lengths
END_TO_END_FACTOR = 2.0


def end_to_end_views():
    import mesh_fixture
    import raycast_fixture
    state, vl, origin = mesh_fixture.analytic('sphere')
    centre = origin + vl * np.array(mesh_fixture.SPHERE['center'])
    E = np.stack([U.look_at(np.array(eye), centre) for eye in END_TO_END['eyes']])
    K = raycast_fixture.intrinsics(END_TO_END['H'], END_TO_END['W'])
    return E, K, raycast_fixture.views_of(E, K)


def end_to_end_difference(volume_depth, mesh_depth, mesh_normals, mesh_mask, views):
    """(the largest depth difference in voxel lengths over the compared pixels, how many pixels are compared)"""
    import mesh_fixture
    _, vl, _ = mesh_fixture.analytic('sphere')
    H, W = END_TO_END['H'], END_TO_END['W']
    worst, count = 0.0, 0
    for f, view in enumerate(np.asarray(views).reshape(-1, 16)):
        P, (fx, fy, cx, cy) = view[:12].reshape(3, 4), view[12:]
        u, v = np.meshgrid(np.arange(W), np.arange(H))
        d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, float)], -1) @ P[:, :3].T
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        with np.errstate(invalid='ignore'):
            steep = np.abs((mesh_normals[f] * d).sum(-1)) >= 0.5
        both = (volume_depth[f] > 0) & mesh_mask[f].astype(bool) & steep
        count += int(both.sum())
        if both.any():
            worst = max(worst, float(np.abs(volume_depth[f].astype(np.float64) - mesh_depth[f].astype(np.float64))[both].max()) / vl)
    return worst, count


@functools.lru_cache(maxsize=None)
def end_to_end_host():
    """the two host entries on the sphere: (difference in voxel lengths, pixels compared, the mesh (vertices, triangles))"""
    import mesh_fixture
    import raycast_fixture
    state, vl, origin = mesh_fixture.analytic('sphere')
    _, _, views = end_to_end_views()
    c = END_TO_END
    volume = raycast_fixture.host_cast_dense(state, vl, origin, c['trunc_voxels'] * vl, views, c['H'], c['W'], c['depth_min'], c['depth_max'], 1.0,
                                             maps=('depth', 'mask'))
    v, t, _, _ = mesh_fixture.host_mesh(state, vl, origin)
    depth, _, normals, _, mask = host_render(v, t, views, c['H'], c['W'], c['depth_min'], c['depth_max'])
    return end_to_end_difference(volume['depth'], depth, normals, mask, views) + ((v, t),)
