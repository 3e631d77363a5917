"""The cases of the block-sparse TSDF tests (tests/test_tsdf_sparse_cpu.py, tests/test_gpu_tsdf_sparse.py): rendered spheres cut by the
block faces, the deliberate allocation cases, extraction states written by hand into blocks, and the callers of the library's host
entries.  The twin's results are computed once per case and shared (lru_cache); callers must not write into them.

Sizes: vl = 1 / 32, so a block is 0.5 m and the sphere of tests/tsdf_fixture.py (centre 0.5, radius 0.3) is cut by the block faces through
its centre; images of 32 x 24 and 31 x 17; strides 1, 4 and 5 (5 divides neither image); 0, 1, 2, 3 and 65 frames (one more than a table
tile of 64); uint16 and float32 depth; colour off, uint8 and float32."""
import ctypes
import functools

import numpy as np

import tsdf_fixture as U
import tsdf_sparse_twin as twin
import tsdf_twin as uniform

F32 = np.float32
VL = 1.0 / 32.0
SHIFT = (-0.7, -1.2, -0.3)

# the twin's worst radial error on the sphere cases, in voxel lengths, measured on the CPU with U.sphere_error on the committed twin
# (tests/test_tsdf_sparse_cpu.py prints the figure again and checks it); the bound of the test is twice this.  Three poses, 32 x 24 images,
# stride 1, a truncation of two voxel lengths: 867 points at the origin, 846 in the shifted scene.  The worst points sit at the silhouettes,
# where a neighbouring ray misses the sphere, and a pixel is 1.5 voxel lengths wide at the sphere's distance.
SPHERE_TWIN_ERROR = {'sphere': 0.6550, 'sphere_shifted': 0.6607}


def _orbit(F, center, distance=1.4):
    ang = 2.0 * np.pi * np.arange(F) / max(F, 1) * 0.35 - 0.5
    return [U.look_at(center + distance * np.array([np.sin(a), 0.25 * np.cos(3 * a), -np.cos(a)]), center) for a in ang]


def _scene(H, W, F, depth='uint16', color=None, shift=(0.0, 0.0, 0.0), trunc_voxels=3.0, stride=4, mangle=False, counts=None, apart=False):
    """F rendered frames of the sphere moved by `shift`; apart: every frame after the first sees a second sphere, 2 m along x"""
    K = np.array([0.9 * W, 0.95 * W, W / 2.0 - 0.3, H / 2.0 + 0.2])
    center = U.SPHERE_CENTER + np.asarray(shift, np.float64)
    E, lam, cols = [], [], []
    for k, pose in enumerate(_orbit(F, center)):
        c = center + np.array([2.0, 0.0, 0.0]) if apart and k else center
        e = U.look_at(np.linalg.inv(pose)[:3, 3] + (c - center), c)
        a, b = U.render_sphere(e, K, H, W, center=c)
        E.append(e), lam.append(a), cols.append(b)
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
    E = np.array(E).reshape(F, 4, 4)
    return _case(depths, colors, E, K, trunc_voxels * VL, stride, counts, center=center)


def _case(depths, colors, E, K, trunc, stride, counts=None, vl=VL, center=None):
    F = len(depths)
    return dict(vl=vl, trunc=trunc, stride=stride, depths=np.ascontiguousarray(depths), colors=colors, E=E, K=np.asarray(K, np.float64),
                table=uniform.frame_table(E, K) if F else np.zeros((0, 16), F32), poses=twin.pose_table(E, K) if F else np.zeros((0, 16)),
                counts=[F] if counts is None else list(counts), depth_scale=1000.0, depth_trunc=3.0, center=center)


def face_case():
    """Identity pose, fx = fy = 1, the principal point on pixel (0, 0), which alone has depth: q = (0, 0, d).  L = 0.5.
    Frame 0: d = 1 m, sdf_trunc = L (16 voxels): q_z - trunc = 0.5 and q_z + trunc = 1.5 lie exactly on block faces, and so do
    q_x -+ trunc = -+0.5: the pixel touches the 27 blocks [-1, 1] x [-1, 1] x [1, 3]."""
    depths = np.zeros((1, 24, 32), np.uint16)
    depths[0, 0, 0] = 1000
    return _case(depths, None, np.eye(4)[None], [1.0, 1.0, 0.0, 0.0], 16 * VL, 4)


def face_case_quarter():
    """The same pixel at d = 0.75 m with sdf_trunc = 0.25 m: q_z -+ trunc = 0.5 and 1.0, both on faces: bz in [1, 2]; bx, by in [-1, 0]"""
    depths = np.zeros((1, 24, 32), np.uint16)
    depths[0, 0, 0] = 750
    return _case(depths, None, np.eye(4)[None], [1.0, 1.0, 0.0, 0.0], 8 * VL, 4)


def range_case(x):
    """face_case_quarter's pixel with the camera at (x, 0, 0): x = 131071.8 puts q_x + trunc past 2^18 blocks of 0.5 m, 131071.7 does not;
    frame 0 is harmless, frame 1 is the one at x"""
    depths = np.zeros((2, 24, 32), np.uint16)
    depths[:, 0, 0] = 750
    E = np.stack([np.eye(4), np.eye(4)])
    E[1, 0, 3] = -x
    return _case(depths, None, E, [1.0, 1.0, 0.0, 0.0], 8 * VL, 4)


@functools.lru_cache(maxsize=None)
def cases():
    c = {
        'u16_f3_s4': _scene(24, 32, 3),
        'u16_f3_s1': _scene(24, 32, 3, stride=1),
        'f32_u8color_f3_s1_31x17': _scene(17, 31, 3, 'float32', 'uint8', stride=1),
        'u16_f32color_f1_s5': _scene(24, 32, 1, 'uint16', 'float32', stride=5),
        'f32_f3_s5_31x17': _scene(17, 31, 3, 'float32', stride=5),
        'shifted_u16_f3_s4': _scene(24, 32, 3, shift=SHIFT),
        'trunc16_u8color_f2_s4': _scene(24, 32, 2, 'uint16', 'uint8', trunc_voxels=16.0),
        'apart_u16_f2_s1': _scene(24, 32, 2, stride=1, apart=True),
        'u8color_f65_s4': _scene(24, 32, 65, 'uint16', 'uint8', trunc_voxels=2.0),
        'mangled_f32_s1': _scene(24, 32, 3, 'float32', stride=1, mangle=True),
        'mangled_u16_color_s1': _scene(24, 32, 3, 'uint16', 'uint8', stride=1, mangle=True),
        'f0': _scene(24, 32, 0),
        'two_volumes_s1': _scene(24, 32, 3, stride=1, counts=[2, 1]),
        'face': face_case(),
        'face_quarter': face_case_quarter(),
        'sphere': _scene(24, 32, 3, stride=1, trunc_voxels=2.0),
        'sphere_shifted': _scene(24, 32, 3, stride=1, trunc_voxels=2.0, shift=SHIFT),
    }
    return c


# ---- extraction states written by hand ---------------------------------------------------------------------------------------------------------
def _blank(color=False):
    return uniform.new_state(twin.BLOCK, color)


def _put(s, idx, t, w=1.0):
    s['tsdf'][idx], s['weight'][idx] = F32(t), F32(w)


def crafted_blocks():
    """name -> (blocks, vl, color): blocks is {(volume, bx, by, bz): state}"""
    out = {}
    # an edge crossing a block face along each axis, between block (-1, 0, 2) and its three face neighbours
    b = {(0, -1, 0, 2): _blank(), (0, 0, 0, 2): _blank(), (0, -1, 1, 2): _blank(), (0, -1, 0, 3): _blank()}
    _put(b[(0, -1, 0, 2)], (15, 5, 5), 0.5), _put(b[(0, 0, 0, 2)], (0, 5, 5), -0.25)
    _put(b[(0, -1, 0, 2)], (7, 15, 9), -0.5), _put(b[(0, -1, 1, 2)], (7, 0, 9), 0.75)
    _put(b[(0, -1, 0, 2)], (3, 4, 15), 0.125), _put(b[(0, -1, 0, 3)], (3, 4, 0), -0.5)
    out['faces'] = (b, VL, False)
    # the face neighbour absent: no point along x from voxel 15; the edge along z beside it has a stencil that reaches x = 16: reads 0
    b = {(0, 0, 0, 0): _blank()}
    _put(b[(0, 0, 0, 0)], (15, 5, 5), 0.5), _put(b[(0, 0, 0, 0)], (15, 5, 6), -0.5)
    out['absent_face'] = (b, VL, False)
    # a normal's stencil reaching the diagonal block (1, 1, 0): absent, then present with values there
    # (the edge crosses the face at x = 15.5, so the stencil along y weighs voxel (16, 16, 7) by 0.5 x 0.99)
    for name in ('diagonal_absent', 'diagonal_present'):
        b = {(0, 0, 0, 0): _blank(), (0, 1, 0, 0): _blank()}
        _put(b[(0, 0, 0, 0)], (15, 15, 7), 0.5), _put(b[(0, 1, 0, 0)], (0, 15, 7), -0.5)
        if name == 'diagonal_present':
            b[(0, 1, 1, 0)] = _blank()
            b[(0, 1, 1, 0)]['tsdf'][0, 0, 6:9] = [0.25, 0.75, -0.125]  # unobserved (weight 0), read by the stencil all the same
        out[name] = (b, VL, False)
    # local index 0: the stencil reads block b - e
    b = {(1, 1, 0, 0): _blank(True), (1, 0, 0, 0): _blank(True), (0, 1, 0, 0): _blank(True)}
    _put(b[(1, 1, 0, 0)], (0, 5, 5), 0.5), _put(b[(1, 1, 0, 0)], (0, 5, 6), -0.5)
    _put(b[(1, 0, 0, 0)], (15, 5, 5), 0.25), _put(b[(1, 0, 0, 0)], (15, 5, 6), 0.75)             # (and an edge across the face, with colours)
    b[(1, 1, 0, 0)]['color'][:, 0, 5, 5], b[(1, 0, 0, 0)]['color'][:, 15, 5, 5] = [0.25, 0.5, 1.0], [1.0, 0.125, 0.0]
    b[(1, 1, 0, 0)]['color'][:, 0, 5, 6], b[(1, 0, 0, 0)]['color'][:, 15, 5, 6] = [0.5, 0.5, 0.0], [0.0, 1.0, 0.75]
    _put(b[(0, 1, 0, 0)], (0, 5, 5), 0.5), _put(b[(0, 1, 0, 0)], (0, 5, 6), -0.5)                # the same block coordinate in volume 0: block b - e absent
    out['local_zero'] = (b, VL, True)
    # the states of tsdf_fixture.crafted_states in the corner of a block: +-0.98f, zeros, tiny opposite signs, weight 0, a NaN in a stencil
    for name, (state, vl, _) in U.crafted_states().items():
        s = _blank(state['color'] is not None)
        for k in ('tsdf', 'weight'):
            s[k][:13, :13, :13] = state[k]
        if s['color'] is not None:
            s['color'][:, :13, :13, :13] = state['color']
        out['uniform_' + name] = ({(0, 2, -3, 1): s}, vl, s['color'] is not None)
    return out


def agreement_state():
    """A hand-written state on 32^3 voxels -- a sphere's truncated distance, cut by the volume's border, observed everywhere, with
    colours -- as a uniform state and as the same numbers in 2 x 2 x 2 blocks of volume 0"""
    i = (np.arange(32) + 0.5) * VL
    x, y, z = np.meshgrid(i, i, i, indexing='ij')
    dist = np.sqrt((x - 0.5) ** 2 + (y - 0.45) ** 2 + (z - 0.1) ** 2) - 0.3
    s = uniform.new_state(32, True)
    s['tsdf'][...] = np.clip(dist / (3 * VL), -1, 1).astype(F32)
    s['weight'][...] = 1 + ((np.arange(32)[:, None, None] + np.arange(32)[None, :, None]) % 3)
    s['color'][...] = np.stack([x, y, (x + z) / 2]).astype(F32)
    blocks = {}
    for bx in range(2):
        for by in range(2):
            for bz in range(2):
                cut = (slice(16 * bx, 16 * bx + 16), slice(16 * by, 16 * by + 16), slice(16 * bz, 16 * bz + 16))
                blocks[(0, bx, by, bz)] = dict(tsdf=s['tsdf'][cut].copy(), weight=s['weight'][cut].copy(), color=s['color'][(slice(None),) + cut].copy())
    return s, blocks


# ---- the library's host entries ---------------------------------------------------------------------------------------------------------------
_ptr, _elems = U._ptr, U._elems


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def host_touch(case, frames=slice(None), counts=None):
    """se3_debug_stsdf_touch_host: ((n,) int64 keys, (n,) int32 frames, bad_frame)"""
    from se3et_amd import _lib
    d, p = np.ascontiguousarray(case['depths'][frames]), np.ascontiguousarray(case['poses'][frames])
    off = _offsets(case['counts'] if counts is None else counts)
    n, bad = ctypes.c_int64(-1), ctypes.c_int64(-2)
    args = (_ptr(d), 0 if d.dtype == np.uint16 else 1, d.shape[0], d.shape[1], d.shape[2], _ptr(p), _ptr(off), len(off) - 1, case['vl'], case['trunc'],
            case['stride'], case['depth_scale'], case['depth_trunc'])
    _lib.check(_lib.lib().se3_debug_stsdf_touch_host(*args, 0, None, None, ctypes.byref(n), ctypes.byref(bad)), 'se3_debug_stsdf_touch_host')
    keys, fr = np.full((n.value,), -1, np.int64), np.full((n.value,), -1, np.int32)
    if n.value:
        _lib.check(_lib.lib().se3_debug_stsdf_touch_host(*args, n.value, _ptr(keys), _ptr(fr), ctypes.byref(n), ctypes.byref(bad)),
                   'se3_debug_stsdf_touch_host')
    return keys, fr, bad.value


class HostVolumes:
    """The directory and the storage on host memory, driven like se3et_amd.tsdf_sparse.SparseTSDFVolumes but through the host entries:
    slots in the order of allocation, the directory in key order."""

    def __init__(self, color):
        self.color = color
        self.keys, self.slots = np.zeros((0,), np.int64), np.zeros((0,), np.int32)
        self.tsdf, self.weight = np.zeros((0, 16, 16, 16), F32), np.zeros((0, 16, 16, 16), F32)
        self.colors = np.zeros((0, 3, 16, 16, 16), F32) if color else None

    def add(self, keys):
        fresh = np.setdiff1d(keys, self.keys)
        n, used = len(fresh), len(self.keys)
        grow = lambda a: np.concatenate([a, np.zeros((n,) + a.shape[1:], F32)])
        self.tsdf, self.weight = grow(self.tsdf), grow(self.weight)
        if self.color:
            self.colors = grow(self.colors)
        allkeys, allslots = np.concatenate([self.keys, fresh]), np.concatenate([self.slots, np.arange(used, used + n, dtype=np.int32)])
        order = np.argsort(allkeys, kind='stable')
        self.keys, self.slots = allkeys[order], allslots[order]
        return self.slots[np.searchsorted(self.keys, keys)]

    def integrate(self, case, frames=slice(None), counts=None):
        from se3et_amd import _lib
        keys, fr, bad = host_touch(case, frames, counts)
        assert bad == -1
        d, t = np.ascontiguousarray(case['depths'][frames]), np.ascontiguousarray(case['table'][frames])
        c = np.ascontiguousarray(case['colors'][frames]) if self.color else None
        touched, per_block = np.unique(keys, return_counts=True)
        csr = _offsets(per_block)
        slots = np.ascontiguousarray(self.add(touched))
        de, ce = _elems(d, c)
        _lib.check(_lib.lib().se3_debug_stsdf_integrate_host(_ptr(self.tsdf), _ptr(self.weight), _ptr(self.colors), len(self.tsdf), _ptr(touched),
                                                             _ptr(slots), len(touched), _ptr(csr), _ptr(fr), case['vl'], case['trunc'], _ptr(d), de,
                                                             _ptr(c), ce, d.shape[0], d.shape[1], d.shape[2], _ptr(t), case['depth_scale'],
                                                             case['depth_trunc']), 'se3_debug_stsdf_integrate_host')
        return self

    def put(self, blocks):
        """blocks written by hand: {coord: state}"""
        keys = np.array(sorted(twin.key_of(c) for c in blocks), np.int64)
        self.add(keys)
        for coord, s in blocks.items():
            slot = self.slots[np.searchsorted(self.keys, twin.key_of(coord))]
            self.tsdf[slot], self.weight[slot] = s['tsdf'], s['weight']
            if self.color:
                self.colors[slot] = s['color']
        return self

    def blocks(self):
        """{coord: state}, the form of the twin"""
        return {twin.coord_of(k): dict(tsdf=self.tsdf[s], weight=self.weight[s], color=self.colors[s] if self.color else None)
                for k, s in zip(self.keys, self.slots)}

    def extract(self, vl, num_volumes):
        """se3_debug_stsdf_extract_host: per volume (points, normals, colors or None)"""
        from se3et_amd import _lib
        B = len(self.keys)
        off = np.full((B + 1,), -1, np.int64)
        args = (_ptr(self.tsdf), _ptr(self.weight), _ptr(self.colors), _ptr(self.keys), _ptr(self.slots), B, float(vl))
        _lib.check(_lib.lib().se3_debug_stsdf_extract_host(*args, 0, None, None, None, _ptr(off)), 'se3_debug_stsdf_extract_host')
        n = int(off[-1])
        out = [np.full((n, 3), np.nan) for _ in range(3 if self.color else 2)]
        if n:
            _lib.check(_lib.lib().se3_debug_stsdf_extract_host(*args, n, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]) if self.color else None, _ptr(off)),
                       'se3_debug_stsdf_extract_host')
            assert int(off[-1]) == n
        cuts = off[np.searchsorted(self.keys, [v << (3 * twin.COORD_BITS) for v in range(num_volumes + 1)])]
        return [tuple(x[cuts[v]:cuts[v + 1]] for x in out) + (() if self.color else (None,)) for v in range(num_volumes)]


# ---- references, computed once --------------------------------------------------------------------------------------------------------------
def _frozen(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def twin_records(name):
    c = cases()[name]
    return twin.touch(c['depths'], c['poses'], c['counts'], c['vl'], c['trunc'], c['stride'], c['depth_scale'], c['depth_trunc'])


@functools.lru_cache(maxsize=None)
def twin_blocks(name):
    c = cases()[name]
    return twin.integrate({}, c['colors'] is not None, c['vl'], c['trunc'], c['depths'], c['table'], c['poses'], c['counts'], c['stride'], c['colors'],
                          c['depth_scale'], c['depth_trunc'])


@functools.lru_cache(maxsize=None)
def twin_clouds(name):
    c = cases()[name]
    return twin.extract(twin_blocks(name), c['vl'], len(c['counts']), c['colors'] is not None)


@functools.lru_cache(maxsize=None)
def host_volumes(name):
    c = cases()[name]
    return HostVolumes(c['colors'] is not None).integrate(c)


@functools.lru_cache(maxsize=None)
def host_clouds(name):
    c = cases()[name]
    return host_volumes(name).extract(c['vl'], len(c['counts']))


def same_blocks(a, b):
    """two {coord: state} with equal coordinates and bit-equal states"""
    return sorted(a) == sorted(b) and all((a[k][f] is None and b[k][f] is None) or U.same(a[k][f], b[k][f]) for k in a for f in ('tsdf', 'weight', 'color'))


def same_clouds(a, b):
    return len(a) == len(b) and all(len(x) == len(y) == 3 and all((p is None and q is None) or U.same(p, q) for p, q in zip(x, y)) for x, y in zip(a, b))
