"""The cases of the triangle mesh tests (tests/test_mesh_cpu.py, tests/test_gpu_mesh.py): analytic states written straight into .tsdf and
.weight (no rendering), random and crafted states for the bit-for-bit comparisons, and the callers of the library's host entries.  The
twin's and the host entries' results are computed once per case and shared (lru_cache); callers must not write into them.

Sizes: resolutions 4 (exactly one cube), 5, 9 and 11 (several workgroups, nothing a multiple of anything), 24 and 32 for the analytic
surfaces, 260 for a row longer than one chunk of 256 lanes; blocks of 16^3 in 2 x 2 x 2 arrangements for the sparse volumes."""
import ctypes
import functools

import numpy as np

import mesh_twin as twin
import tsdf_fixture as U
import tsdf_sparse_fixture as S
import tsdf_sparse_twin as sparse
import tsdf_twin as uniform

F32 = np.float32
_ptr = U._ptr

# the twin's worst distance of a mesh vertex from the analytic sphere, in voxel lengths, measured on the CPU with sphere_error on the committed
# twin (tests/test_mesh_cpu.py prints the figure again and checks it); the bound of the test is twice this.  The state is the exact distance
# divided by a truncation of three voxel lengths and rounded to float32, so the error is that of interpolating a sphere's distance
# linearly along one edge: about (vl / 2)^2 / (2 radius) = 0.017 voxel lengths at a radius of 7.2.
SPHERE_TWIN_ERROR = 0.0168


# ---- analytic states -----------------------------------------------------------------------------------------------------------------------------
def _centres(R):
    i = np.arange(R) + 0.5
    return np.meshgrid(i, i, i, indexing='ij')


def _state(dist, trunc=3.0, color=False):
    """a state from a signed distance in voxel lengths: tsdf = clip(dist / trunc), every voxel observed"""
    R = dist.shape[0]
    s = uniform.new_state(R, color)
    s['tsdf'][...] = np.clip(dist / trunc, -1, 1).astype(F32)
    s['weight'][...] = 1
    if color:
        x, y, z = _centres(R)
        s['color'][...] = (np.stack([x, y, (x + z) / 2]) / R).astype(F32)
    return s


SPHERE = dict(R=24, center=(11.7, 12.2, 11.9), radius=7.2)


@functools.lru_cache(maxsize=None)
def analytic(name):
    """name -> (state, vl, origin); distances in voxel lengths, vl = 1 / 24 or 1 / 32"""
    if name == 'sphere':
        x, y, z = _centres(SPHERE['R'])
        c = SPHERE['center']
        return _state(np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - SPHERE['radius']), 1.0 / 24, np.array([0.5, -1.0, 2.0])
    if name == 'torus':
        x, y, z = _centres(32)
        ring = np.sqrt((x - 15.8) ** 2 + (y - 16.3) ** 2) - 8.6
        return _state(np.sqrt(ring ** 2 + (z - 15.6) ** 2) - 3.7), 1.0 / 32, np.zeros(3)
    if name == 'two_spheres':
        x, y, z = _centres(32)
        a = np.sqrt((x - 8.3) ** 2 + (y - 9.1) ** 2 + (z - 8.7) ** 2) - 5.2
        b = np.sqrt((x - 21.6) ** 2 + (y - 20.9) ** 2 + (z - 22.2) ** 2) - 6.1
        return _state(np.minimum(a, b)), 1.0 / 32, np.zeros(3)
    if name == 'half_observed':                                          # the sphere with the half-space x >= 12 unobserved
        s, vl, o = analytic('sphere')
        s = {k: v.copy() for k, v in s.items() if v is not None}
        s['color'] = None
        s['weight'][12:] = 0
        return s, vl, o
    raise KeyError(name)


def sphere_error(vertices, vl, origin):
    """the worst distance of the vertices from the analytic sphere, in voxel lengths"""
    local = (vertices - origin) / vl
    return float(np.max(np.abs(np.linalg.norm(local - np.array(SPHERE['center']), axis=1) - SPHERE['radius'])))


# ---- states for the bit-for-bit comparisons --------------------------------------------------------------------------------------------------
def random_state(R, seed, color, holes=True):
    """smooth random values (so that surfaces are sheets, not noise) with exact zeros, -0, values at +-1 and unobserved voxels among them"""
    rng = np.random.default_rng(seed)
    x, y, z = _centres(R)
    f = sum(rng.normal() * np.sin(rng.uniform(0.3, 1.1) * x + rng.uniform(0.3, 1.1) * y + rng.uniform(0.3, 1.1) * z + rng.uniform(0, 6)) for _ in range(4))
    s = uniform.new_state(R, color)
    s['tsdf'][...] = np.clip(f / 2, -1, 1).astype(F32)
    flat = s['tsdf'].reshape(-1)
    pick = rng.permutation(flat.size)
    flat[pick[:R]] = 0.0
    flat[pick[R:2 * R]] = -0.0
    s['weight'][...] = rng.integers(1, 4, (R, R, R))
    if holes:
        s['weight'].reshape(-1)[pick[2 * R:2 * R + R * R // 2]] = 0
    if color:
        s['color'][...] = rng.uniform(0, 1, (3, R, R, R)).astype(F32)
    return s


def one_cube(case, color=False):
    """R = 4: exactly one cube, at (1, 1, 1), with cube index `case`"""
    s = uniform.new_state(4, color)
    s['tsdf'][...] = 0.5
    s['weight'][...] = 1
    for c in range(8):
        if case >> c & 1:
            s['tsdf'][tuple(1 + twin.CORNERS[c])] = -0.25 - c / 16.0
    if color:
        s['color'][...] = np.linspace(0, 1, 3 * 64, dtype=F32).reshape(3, 4, 4, 4)
    return s


@functools.lru_cache(maxsize=None)
def dense_states():
    """name -> (state, vl, origin)"""
    out = {
        'r5_color': (random_state(5, 1, True, holes=False), 0.05, np.array([1.0, 2.0, 3.0])),
        'r9_holes': (random_state(9, 2, False), 0.04, np.zeros(3)),
        'r11_color_holes': (random_state(11, 3, True), 0.03, np.array([-0.25, 0.5, 0.0])),
        'r9_flat': (_state(np.full((9, 9, 9), 1.0)), 0.05, np.zeros(3)),                 # no surface at all
        'r4_case_105': (one_cube(105), 0.1, np.zeros(3)),
    }
    s = _state(_centres(9)[2] - 3.5)                                   # a plane through voxel centres: z = 3 holds exactly 0.0f and is positive
    assert s['tsdf'][4, 4, 3] == 0 and s['tsdf'][4, 4, 2] < 0
    out['r9_exact_zero'] = (s, 0.05, np.zeros(3))
    return out


def sheet_state():
    """R = 260: a tilted sheet through z = 255 / 256, where a row is longer than one chunk of 256 lanes, observed only near the sheet"""
    R = 260
    x, y, z = _centres(R)
    d = (z - 256.4) + 1.5 * (x - 130) / 130 + 0.8 * (y - 130) / 130      # crossings from z = 254 to z = 258 in voxel indices
    s = uniform.new_state(R, False)
    s['tsdf'][...] = np.clip(d / 3, -1, 1).astype(F32)
    s['weight'][...] = (np.abs(d) < 4).astype(F32)
    return s, 0.01, np.zeros(3)


def agreement_state():
    """every weight != 0, no exact zero, |t| < 0.98: the mesh's vertices are the rows of the point extraction"""
    x, y, z = _centres(12)
    d = np.sqrt((x - 5.7) ** 2 + (y - 6.2) ** 2 + (z - 6.4) ** 2) - 3.9
    s = _state(d, trunc=12.0, color=True)
    assert np.all(np.abs(s['tsdf']) < F32(0.98)) and np.all(s['tsdf'] != 0)
    return s, 0.05, np.array([0.1, 0.2, 0.3])


# ---- sparse states ----------------------------------------------------------------------------------------------------------------------------
def split_blocks(state, volume=0, corner=(0, 0, 0), drop=()):
    """a uniform state of resolution 16 n as n^3 blocks at block corner `corner`, without the blocks in `drop` (offsets from the corner)"""
    n = state['tsdf'].shape[0] // 16
    blocks = {}
    for bx in range(n):
        for by in range(n):
            for bz in range(n):
                if (bx, by, bz) in drop:
                    continue
                cut = (slice(16 * bx, 16 * bx + 16), slice(16 * by, 16 * by + 16), slice(16 * bz, 16 * bz + 16))
                blocks[(volume, corner[0] + bx, corner[1] + by, corner[2] + bz)] = dict(
                    tsdf=state['tsdf'][cut].copy(), weight=state['weight'][cut].copy(),
                    color=None if state['color'] is None else state['color'][(slice(None),) + cut].copy())
    return blocks


def small_sphere_state(color=True):
    """R = 32: a sphere of radius 6.3 around the shared corner of the 2 x 2 x 2 blocks, observed within 13 voxels of it and so clear of the outer shell"""
    x, y, z = _centres(32)
    r = np.sqrt((x - 15.7) ** 2 + (y - 16.4) ** 2 + (z - 16.1) ** 2)
    s = _state(r - 6.3, color=color)
    s['weight'][...] = (r < 13).astype(F32) * 2
    return s


@functools.lru_cache(maxsize=None)
def sparse_states():
    """name -> (blocks, vl, num_volumes, color)"""
    ball = small_sphere_state()
    out = {
        # the surface passes through the faces, the edges and the shared corner of 2 x 2 x 2 blocks, at a corner with negative coordinates
        'corner_sphere': (split_blocks(ball, corner=(-1, 3, -2)), 1.0 / 32, 1, True),
        # one of the eight blocks absent: a hole
        'absent_block': (split_blocks(ball, corner=(0, 0, 0), drop=((1, 0, 1),)), 1.0 / 32, 1, True),
    }
    two = split_blocks(random_state(16, 5, False), volume=0, corner=(2, -3, 1))
    two.update(split_blocks(small_sphere_state(False), volume=2, corner=(0, 0, 0)))
    out['two_volumes'] = (two, 0.02, 3, False)                          # volume 1 has no blocks
    return out


# ---- the library's host entries ---------------------------------------------------------------------------------------------------------------
def host_table():
    from se3et_amd import _lib, ops
    rows, counts = np.full((256, ops.MESH_LIMITS['table_width']), 99, np.int8), np.full((256,), -1, np.int32)
    _lib.check(_lib.lib().se3_debug_mesh_table(_ptr(rows), _ptr(counts)), 'se3_debug_mesh_table')
    return rows, counts


def host_mesh(state, vl, origin):
    """se3_debug_tsdf_mesh_host: (vertices, triangles, normals, colors or None)"""
    from se3et_amd import _lib
    R = state['tsdf'].shape[0]
    o = np.ascontiguousarray(origin, dtype=np.float64)
    counts = np.full((2,), -1, np.int64)
    args = (_ptr(state['tsdf']), _ptr(state['weight']), _ptr(state['color']), R, float(vl), _ptr(o))
    _lib.check(_lib.lib().se3_debug_tsdf_mesh_host(*args, 0, 0, None, None, None, None, _ptr(counts)), 'se3_debug_tsdf_mesh_host')
    nv, nt = int(counts[0]), int(counts[1])
    out = [np.full((nv, 3), np.nan) for _ in range(3 if state['color'] is not None else 2)]
    tri = np.full((nt, 3), -1, np.int64)
    if nv:
        _lib.check(_lib.lib().se3_debug_tsdf_mesh_host(*args, nv, nt, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]) if len(out) == 3 else None, _ptr(tri),
                                                       _ptr(counts)), 'se3_debug_tsdf_mesh_host')
        assert (int(counts[0]), int(counts[1])) == (nv, nt)
    return out[0], tri, out[1], out[2] if len(out) == 3 else None


def host_mesh_sparse(blocks, vl, num_volumes, color):
    """se3_debug_stsdf_mesh_host: per volume (vertices, triangles, normals, colors or None)"""
    from se3et_amd import _lib
    H = S.HostVolumes(color).put(blocks)
    B = len(H.keys)
    off = np.full((2, B + 1), -1, np.int64)
    args = (_ptr(H.tsdf), _ptr(H.weight), _ptr(H.colors), _ptr(H.keys), _ptr(H.slots), B, float(vl))
    _lib.check(_lib.lib().se3_debug_stsdf_mesh_host(*args, 0, 0, None, None, None, None, _ptr(off)), 'se3_debug_stsdf_mesh_host')
    nv, nt = int(off[0, -1]), int(off[1, -1])
    out = [np.full((nv, 3), np.nan) for _ in range(3 if color else 2)]
    tri = np.full((nt, 3), -1, np.int64)
    if nv:
        _lib.check(_lib.lib().se3_debug_stsdf_mesh_host(*args, nv, nt, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]) if color else None, _ptr(tri), _ptr(off)),
                   'se3_debug_stsdf_mesh_host')
    cuts = np.searchsorted(H.keys, [v << (3 * sparse.COORD_BITS) for v in range(num_volumes + 1)])
    vc, tc = off[0][cuts], off[1][cuts]
    return [(out[0][vc[v]:vc[v + 1]], tri[tc[v]:tc[v + 1]], out[1][vc[v]:vc[v + 1]], out[2][vc[v]:vc[v + 1]] if color else None)
            for v in range(num_volumes)]


# ---- references, computed once --------------------------------------------------------------------------------------------------------------
def _frozen(mesh):
    for x in mesh:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return tuple(mesh)


@functools.lru_cache(maxsize=None)
def twin_mesh(kind, name):
    state, vl, origin = (analytic if kind == 'analytic' else lambda n: dense_states()[n])(name)
    return _frozen(twin.mesh_dense(state, vl, origin))


@functools.lru_cache(maxsize=None)
def host_dense(kind, name):
    state, vl, origin = {'analytic': analytic, 'dense': lambda n: dense_states()[n], 'sheet': lambda n: sheet_state(),
                         'agreement': lambda n: agreement_state()}[kind](name)
    return _frozen(host_mesh(state, vl, origin))


@functools.lru_cache(maxsize=None)
def host_sparse(name):
    blocks, vl, V, color = sparse_states()[name]
    return [_frozen(m) for m in host_mesh_sparse(blocks, vl, V, color)]


def same_mesh(a, b):
    """vertices, normals and colours equal bit for bit, triangles equal"""
    return len(a) == len(b) == 4 and all((p is None and q is None) or (p is not None and q is not None and U.same(p, q)) for p, q in zip(a, b))


def euler(mesh):
    """V - E + F of (vertices, triangles, ..)"""
    t = mesh[1]
    edges = np.unique(np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1), axis=0)
    return len(mesh[0]) - len(edges) + len(t)
