"""The named cases of the mesh post-processing tests (tests/test_mesh_ops_cpu.py, tests/test_gpu_mesh_ops.py) and the callers of the library's
se3_debug_mesh_*_host entries.  A case is (vertices (n, 3) float64, triangles (m, 3) int64); results are computed once per case and shared
(lru_cache); callers must not write into them.

Sizes: a handful of triangles for the crafted cases, a fan of 100 (a valence above one wave), a strip of 4 096 shuffled triangles (union
chains across workgroups, several chunks of the scans), the small sphere of mesh_fixture (about 1 500 triangles)."""
import functools

import numpy as np

import mesh_fixture
import mesh_ops_twin as twin
import tsdf_fixture as U

_ptr = U._ptr
METHODS = ('simple', 'laplacian', 'taubin')


def _points(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3))


def _tris(rows):
    return np.array(rows, np.int64).reshape(-1, 3)


def _strip(m, seed):
    """a strip of m triangles over m + 2 vertices, orientation alternating so that it is consistent, in a shuffled order"""
    rng = np.random.default_rng(seed)
    i = np.arange(m)
    tri = np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], 1), np.stack([i + 1, i, i + 2], 1))
    v = np.stack([(np.arange(m + 2) // 2) * 0.1, (np.arange(m + 2) % 2) * 0.1, 0.01 * np.sin(np.arange(m + 2))], 1)
    return v + rng.uniform(-0.01, 0.01, v.shape), tri[rng.permutation(m)]


def _grid(k, h):
    """(k + 1)^2 vertices in the plane z = 0.5 at spacing h, every cell cut by the same diagonal"""
    ij = np.stack(np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing='ij'), -1).reshape(-1, 2)
    v = np.concatenate([ij * h, np.full((len(ij), 1), 0.5)], 1)
    at = lambda i, j: i * (k + 1) + j
    tri = []
    for i in range(k):
        for j in range(k):
            tri += [(at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1))]
    return v, _tris(tri)


@functools.lru_cache(maxsize=None)
def sphere():
    """the mesh of mesh_fixture.small_sphere_state through the library's marching cubes on the host: (vertices, triangles, vl, origin)"""
    vl, origin = 1.0 / 32, np.array([0.25, -0.5, 1.0])
    v, t, _, _ = mesh_fixture.host_mesh(mesh_fixture.small_sphere_state(False), vl, origin)
    return v, t, vl, origin


# How much five Taubin iterations may add to mesh_fixture.sphere_error of the fused sphere, in voxel lengths: the twin's own growth,
# measured on the CPU by tests/test_mesh_ops_cpu.py::test_twin_taubin_on_the_fused_sphere (which prints it again): 0.0159, rounded up.
TAUBIN_SPHERE_GROWTH = 0.016


def fused_state():
    """the analytic sphere of mesh_fixture (R = 24) with a separate blob of 2^3 voxels in a corner: (state, vl, origin)"""
    s, vl, origin = mesh_fixture.analytic('sphere')
    s = {k: None if x is None else x.copy() for k, x in s.items()}
    s['tsdf'][2:4, 2:4, 2:4] = -0.5
    return s, vl, origin


@functools.lru_cache(maxsize=None)
def fused_sphere():
    """its mesh through the library's marching cubes on the host: (vertices, triangles, vl, origin)"""
    s, vl, origin = fused_state()
    v, t, _, _ = mesh_fixture.host_mesh(s, vl, origin)
    return v, t, vl, origin


SPHERE_CENTER, SPHERE_RADIUS = np.array([15.7, 16.4, 16.1]), 6.3            # of small_sphere_state, in voxel lengths


@functools.lru_cache(maxsize=None)
def cases():
    tet = [(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)]
    fan = 100
    out = {
        # components
        'two_tets_one_vertex': (_points(7, 1), _tris(tet + [tuple(v + 3 for v in t) for t in tet])),           # vertex 3 is in both
        'edge_pair_same': (_points(4, 2), _tris([(0, 1, 2), (1, 0, 3)])),            # consistently oriented: the edge runs both ways
        'edge_pair_opposite': (_points(4, 3), _tris([(0, 1, 2), (0, 1, 3)])),        # the shared edge runs the same way in both
        'three_on_edge': (_points(5, 4), _tris([(0, 1, 2), (0, 1, 3), (1, 0, 4)])),
        'duplicate_triangle': (_points(4, 5), _tris([(0, 1, 2), (1, 2, 3), (0, 1, 2)])),
        'degenerate': (_points(4, 6), _tris([(0, 0, 1), (0, 1, 2), (3, 3, 3)])),
        'interleaved': (_points(9, 7), _tris([(0, 1, 2), (3, 4, 5), (2, 1, 6), (5, 4, 7), (6, 1, 8)])),
        'strip_4096': _strip(4096, 8),
        'no_triangles': (_points(5, 9), _tris([])),
        'nothing': (np.zeros((0, 3)), _tris([])),
        # incidence and smoothing
        'isolated_vertex': (_points(5, 10), _tris([(0, 1, 2), (2, 1, 3)])),
        'one_neighbor': (_points(2, 11), _tris([(0, 0, 1)])),
        'fan_100': (np.concatenate([_points(1, 12) * 0.1, np.stack([np.cos(np.arange(fan) * 2 * np.pi / fan), np.sin(np.arange(fan) * 2 * np.pi / fan),
                                                                   0.1 * np.cos(np.arange(fan))], 1)]),
                    _tris([(0, 1 + i, 1 + (i + 1) % fan) for i in range(fan)])),
        'grid_dyadic': _grid(8, 0.25),
    }
    v, t, _, _ = sphere()
    out['sphere'] = (v, t)
    for v, t in out.values():
        v.setflags(write=False), t.setflags(write=False)
    return out


BAD = {                                                                     # a triangle out of range: vertex n, vertex -1
    'bad_n': (_points(4, 20), _tris([(0, 1, 2), (1, 2, 4), (2, 1, 3)])),
    'bad_minus_one': (_points(4, 21), _tris([(0, 1, 2), (-1, 2, 3), (2, 1, 3)])),
}


def attributes(n, seed):
    """normals and colours of a case: any values, they are filtered like positions"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)), rng.uniform(0, 1, (n, 3))


def keep_masks(m, seed):
    """name -> keep bytes: all, none, one of many, a random half (vertices shared by kept and dropped triangles)"""
    rng = np.random.default_rng(seed)
    one = np.zeros(m, np.uint8)
    one[m // 2:m // 2 + 1] = 1
    return {'all': np.ones(m, np.uint8), 'none': np.zeros(m, np.uint8), 'one': one, 'half': (rng.uniform(size=m) < 0.5).astype(np.uint8)}


# ---- the library's host entries -----------------------------------------------------------------------------------------------------------------------
def _lib():
    from se3et_amd import _lib as L
    return L, L.lib()


def host_incidence(tri, n):
    """se3_debug_mesh_incidence_host: (tri_offsets, tri_rows, nbr_offsets, nbr_rows, status)"""
    L, lib = _lib()
    tri = np.ascontiguousarray(tri, np.int64)
    m = len(tri)
    toff, noff = np.full(n + 1, -1, np.int64), np.full(n + 1, -1, np.int64)
    trows, counts = np.full(3 * m + 1, -1, np.int32), np.full(4, -1, np.int64)
    L.check(lib.se3_debug_mesh_incidence_host(_ptr(tri), n, m, _ptr(toff), _ptr(trows), _ptr(noff), 0, None, _ptr(counts)), 'incidence_host')
    nrows = np.full(int(counts[2]) + 1, -1, np.int32)
    L.check(lib.se3_debug_mesh_incidence_host(_ptr(tri), n, m, _ptr(toff), _ptr(trows), _ptr(noff), int(counts[2]), _ptr(nrows), _ptr(counts)),
            'incidence_host')
    assert trows[int(counts[1])] == -1 and nrows[-1] == -1 and toff[n] == counts[1] and noff[n] == counts[2]
    return toff, trows[:int(counts[1])], noff, nrows[:-1], int(counts[0])


def host_components(vertices, tri):
    """se3_debug_mesh_components_host: (labels, n_triangles (k,), area (k,), status)"""
    L, lib = _lib()
    v, tri = np.ascontiguousarray(vertices, np.float64), np.ascontiguousarray(tri, np.int64)
    n, m = len(v), len(tri)
    toff, trows, _, _, _ = host_incidence(tri, n)
    trows = np.ascontiguousarray(np.concatenate([trows, np.zeros(1, np.int32)]))
    labels, count, area, counts = np.full(m + 1, -7, np.int64), np.full(m + 1, -7, np.int64), np.full(m + 1, np.nan), np.full(4, -1, np.int64)
    L.check(lib.se3_debug_mesh_components_host(_ptr(v), _ptr(tri), n, m, _ptr(toff), _ptr(trows), _ptr(labels), _ptr(count), _ptr(area), _ptr(counts)),
            'components_host')
    k = int(counts[1])
    assert labels[m] == -7 and count[m] == -7 and not count[k:m].any() and not area[k:m].any()
    return labels[:m], count[:k], area[:k], int(counts[0])


def host_select(vertices, tri, keep, normals=None, colors=None):
    """se3_debug_mesh_select_host: (vertices, triangles, normals, colors, vertex_map, status)"""
    L, lib = _lib()
    v, tri, keep = np.ascontiguousarray(vertices, np.float64), np.ascontiguousarray(tri, np.int64), np.ascontiguousarray(keep, np.uint8)
    n, m = len(v), len(tri)
    vmap, counts = np.full(n + 1, -7, np.int64), np.full(4, -1, np.int64)
    head = (_ptr(v), _ptr(normals), _ptr(colors), _ptr(tri), _ptr(keep), n, m)
    L.check(lib.se3_debug_mesh_select_host(*head, 0, 0, None, None, None, None, _ptr(vmap), _ptr(counts)), 'select_host')
    nv, nt = int(counts[1]), int(counts[2])
    out = [None if x is None else np.full((nv + 1, 3), np.nan) for x in (v, normals, colors)]
    otri = np.full((nt + 1, 3), -7, np.int64)
    L.check(lib.se3_debug_mesh_select_host(*head, nv, nt, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(otri), _ptr(vmap), _ptr(counts)), 'select_host')
    assert vmap[n] == -7 and (otri[nt] == -7).all() and all(x is None or np.isnan(x[nv]).all() for x in out)
    return out[0][:nv], otri[:nt], None if out[1] is None else out[1][:nv], None if out[2] is None else out[2][:nv], vmap[:n], int(counts[0])


def host_normals(vertices, tri, normalized=True):
    """se3_debug_mesh_normals_host: (triangle normals, vertex normals)"""
    L, lib = _lib()
    v, tri = np.ascontiguousarray(vertices, np.float64), np.ascontiguousarray(tri, np.int64)
    n, m = len(v), len(tri)
    toff, trows, _, _, _ = host_incidence(tri, n)
    trows = np.ascontiguousarray(np.concatenate([trows, np.zeros(1, np.int32)]))
    tn, vn = np.full((m + 1, 3), np.nan), np.full((n + 1, 3), np.nan)
    L.check(lib.se3_debug_mesh_normals_host(_ptr(v), _ptr(tri), n, m, _ptr(toff), _ptr(trows), int(normalized), _ptr(tn), _ptr(vn)), 'normals_host')
    assert np.isnan(tn[m]).all() and np.isnan(vn[n]).all()
    return tn[:m], vn[:n]


def host_smooth(values, tri, method, iterations, lam=0.5, mu=-0.53):
    """se3_debug_mesh_smooth_host over the neighbour table of the host incidence"""
    L, lib = _lib()
    from se3et_amd import ops
    x = np.ascontiguousarray(values, np.float64)
    n = len(x)
    _, _, noff, nrows, _ = host_incidence(tri, n)
    nrows = np.ascontiguousarray(np.concatenate([nrows, np.zeros(1, np.int32)]))
    out = np.full((n + 1, 3), np.nan)
    L.check(lib.se3_debug_mesh_smooth_host(_ptr(x), n, _ptr(noff), _ptr(nrows), ops.MESH_SMOOTH_METHODS[method], iterations, lam, mu, _ptr(out)), 'smooth_host')
    assert np.isnan(out[n]).all()
    return out[:n]


def same(a, b):
    """equal bit for bit (floats), equal (integers)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- references, computed once ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def twin_incidence(name):
    v, t = cases()[name]
    return twin.incidence(t, len(v))


@functools.lru_cache(maxsize=None)
def twin_components(name):
    v, t = cases()[name]
    return twin.components(v, t, len(v))


@functools.lru_cache(maxsize=None)
def host_case(name, what):
    v, t = cases()[name]
    return {'incidence': lambda: host_incidence(t, len(v)), 'components': lambda: host_components(v, t), 'normals': lambda: host_normals(v, t),
            'normals_raw': lambda: host_normals(v, t, False)}[what]()


# ---- vertex clustering --------------------------------------------------------------------------------------------------------------------------------
def _cells(rows, h, seed):
    """one vertex per row (i, j, k) somewhere inside cell (i, j, k) of a grid of spacing h whose first cell starts at -h / 2 (vertex 0 sits
    at the origin: the minimum, so the grid's origin is -h / 2 exactly)"""
    rng = np.random.default_rng(seed)
    v = (np.array(rows, np.float64) + rng.uniform(-0.4, 0.4, (len(rows), 3))) * h
    v[0] = 0.0
    return np.maximum(v, 0.0)


@functools.lru_cache(maxsize=None)
def cluster_cases():
    """name -> (vertices, triangles, voxel_size)"""
    C = cases()
    rng = np.random.default_rng(31)
    neg = rng.uniform(-3.0, -1.0, (60, 3))
    # cells A = (0, 0, 0), B = (1, 0, 0), C = (1, 2, 0), D = (2, 0, 1), two vertices in each of A, B, C: a 0, 1; b 2, 3; c 4, 5; d 6
    abcd = _cells([(0, 0, 0), (0, 0, 0), (1, 0, 0), (1, 0, 0), (1, 2, 0), (1, 2, 0), (2, 0, 1)], 0.5, 32)
    face = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.249, 0.3, 0.0], [0.75, 0.75, 0.25], [1.0, 0.1, 0.7]])     # origin -0.25: x = 0.25 is the face of cell 1
    out = {
        'larger_than_mesh': (C['fan_100'][0], C['fan_100'][1], 10.0),                       # one vertex, no triangles
        'on_cell_face': (face, _tris([(0, 1, 2), (1, 3, 4), (2, 1, 3), (0, 2, 4)]), 0.5),
        'negative': (neg, rng.integers(0, 60, (200, 3)), 0.4),
        'collapse_to_edge': (abcd, _tris([(0, 1, 2), (0, 2, 4), (2, 3, 6)]), 0.5),          # (a, a, b) and (b, b, d) collapse
        'equal_and_mirror': (abcd, _tris([(0, 2, 4), (3, 5, 1), (1, 4, 2), (6, 0, 3), (5, 0, 2)]), 0.5),
        'sphere': (C['sphere'][0], C['sphere'][1], 2.5 / 32),
        'grid': (C['grid_dyadic'][0], C['grid_dyadic'][1], 0.5),
        'strip': (C['strip_4096'][0], C['strip_4096'][1], 0.35),
        'no_triangles': (C['no_triangles'][0], C['no_triangles'][1], 0.5),
        'nothing': (C['nothing'][0], C['nothing'][1], 0.5),
    }
    for v, t, _ in out.values():
        v.setflags(write=False), t.setflags(write=False)
    return out


def host_cluster(vertices, tri, voxel_size, normals=None, colors=None):
    """se3_debug_mesh_cluster_vertices_host: (vertices, triangles, normals, colors, vertex_map, status)"""
    L, lib = _lib()
    v, tri = np.ascontiguousarray(vertices, np.float64), np.ascontiguousarray(tri, np.int64)
    n, m = len(v), len(tri)
    vmap, counts = np.full(n + 1, -7, np.int64), np.full(4, -1, np.int64)
    head = (_ptr(v), _ptr(normals), _ptr(colors), _ptr(tri), n, m, float(voxel_size))
    L.check(lib.se3_debug_mesh_cluster_vertices_host(*head, 0, 0, None, None, None, None, _ptr(vmap), _ptr(counts)), 'cluster_vertices_host')
    nv, nt = int(counts[1]), int(counts[2])
    out = [None if x is None else np.full((nv + 1, 3), np.nan) for x in (v, normals, colors)]
    otri = np.full((nt + 1, 3), -7, np.int64)
    L.check(lib.se3_debug_mesh_cluster_vertices_host(*head, nv, nt, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(otri), _ptr(vmap), _ptr(counts)),
            'cluster_vertices_host')
    assert vmap[n] == -7 and (otri[nt] == -7).all() and all(x is None or np.isnan(x[nv]).all() for x in out) and (int(counts[1]), int(counts[2])) == (nv, nt)
    return out[0][:nv], otri[:nt], None if out[1] is None else out[1][:nv], None if out[2] is None else out[2][:nv], vmap[:n], int(counts[0])
