"""Shared inputs, edge cases and demands of the scan-preparation tests (tests/test_scan_prep_cpu.py, tests/test_gpu_scan_prep.py).

Inputs: se3et_amd.synthetic.box_surface at seed 1 -- `micro` (600 points), `c1_2k` (2000), and `c3_4k` twice: `c3_1500`, the first 1500
of its 4000 points, and `c3_gen1500`, 1500 points drawn with its box and jitter (the generator's stream depends on the count, so these are
two clouds).  With the twin (tests/scan_prep_twin.py): every row has a relative eigenvalue gap (l1 - l0) / l2 >= 0.044 (>= 0.118 without
`c3_1500`), no row has a distance tie at the 33rd place, and voxel sizes 0.05 / 0.1 / 2.5 / 2.5 give 385 / 574 / 270 / 272 voxels with at
most 6 / 9 / 15 / 13 members (test_fixture_facts pins these).

Demands on the normals (k = 33), against the twin:
  - every covariance entry within 4 m 2^-53 trace(C): both sides add the same m terms, each bounded by the trace;
  - every normal unit to 4 2^-53, measured exactly (fractions): three squares, two sums, a root and a division round the length by less
    than 2.25 units of 2^-53;
  - direction: 1 - |n . n_twin| <= (K 2^-53 l2 / (l1 - l0))^2 / 2 -- Davis-Kahan for a backward-stable solver whose backward error is
    K 2^-53 |C|.  The left side is far below the resolution of a float64 dot product near 1, so it is measured through the sine:
    |n x n_twin| <= K 2^-53 l2 / (l1 - l0), the same demand (1 - cos = sin^2 / (1 + cos)).  K cannot be derived without fixing the
    solver: the largest value observed for the host entry against the twin on the fixture clouds is recorded in
    profiles/scan_prep_probe.txt (tools/scan_prep_probe.py measures it); DIRECTION_K is 8 times that, rounded up to a power of two (the
    margin covers the second solver in the comparison, numpy's);
  - rows with (l1 - l0) / l2 < 1e-6 are excluded from the direction check only (at most 1 % of a case; the fixture clouds exclude none)."""
import ctypes
import functools
from fractions import Fraction

import numpy as np

import scan_prep_twin as twin

U = 2.0 ** -53
KNN = 33
DIRECTION_K = 64.0            # 8 x the largest observed K (4.18: profiles/scan_prep_probe.txt), rounded up to a power of two
GAP_FLOOR = 1e-6
VOXEL_SIZES = {'micro': 0.05, 'c1_2k': 0.1, 'c3_1500': 2.5, 'c3_gen1500': 2.5}
VOXEL_FACTS = {'micro': (385, 6), 'c1_2k': (574, 9), 'c3_1500': (270, 15), 'c3_gen1500': (272, 13)}
GAP_FACTS = {'micro': 0.118, 'c1_2k': 0.118, 'c3_1500': 0.044, 'c3_gen1500': 0.118}
CLOUDS = ('micro', 'c1_2k', 'c3_1500', 'c3_gen1500')


@functools.lru_cache(None)
def cloud(name):
    from se3et_amd.synthetic import PAIR_PRESETS, box_surface
    preset, drawn, rows = {'micro': ('micro', 600, 600), 'c1_2k': ('c1_2k', 2000, 2000), 'c3_1500': ('c3_4k', 4000, 1500),
                           'c3_gen1500': ('c3_4k', 1500, 1500)}[name]
    _, dims, jitter = PAIR_PRESETS[preset]
    pts = np.ascontiguousarray(box_surface(drawn, dims, 1, jitter)[:rows])
    pts.setflags(write=False)
    return pts


@functools.lru_cache(None)
def fake_normals(name):
    """Some (n, 3) values to average: deterministic, not unit."""
    g = np.random.default_rng(7)
    a = g.standard_normal(cloud(name).shape).astype(cloud(name).dtype)
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def twin_knn(name, k=64):
    """The twin's 64 neighbours of every row of a named cloud, once: a prefix of a row is the row of a smaller k."""
    idx, d2 = twin.knn(cloud(name), k)
    idx.setflags(write=False), d2.setflags(write=False)
    return idx, d2


@functools.lru_cache(None)
def twin_normals(name):
    """-> (C, m, normals, eigenvalues) of the twin at k = 33"""
    idx = twin_knn(name)[0][:, :KNN]
    C, m = twin.covariances(cloud(name), idx)
    n, w = twin.normals_from(C, m)
    return C, m, n, w


def edge_clouds():
    """name -> (points float64, what the normals check may demand: 'direction' | 'fallback' | 'unit' | 'plane')"""
    g = np.random.default_rng(11)
    lattice = np.stack(np.meshgrid(np.arange(6.0), np.arange(6.0), np.arange(6.0), indexing='ij'), -1).reshape(-1, 3)
    dup = g.uniform(-1, 1, (150, 3))
    planar = np.concatenate([g.uniform(-1, 1, (300, 2)), np.zeros((300, 1))], 1)
    line = np.outer(g.uniform(-2, 2, 80), np.array([1.0, 2.0, -0.5]))
    cell = 0.05
    clusters = np.concatenate([g.uniform(0, cell, (10, 3)), g.uniform(0, 10 * cell, (500, 3)) + 40 * cell * np.array([1.0, 1.0, 1.0])], 0)
    return {
        'n0': (np.zeros((0, 3)), 'fallback'),
        'n1': (np.array([[0.3, -0.2, 0.9]]), 'fallback'),
        'n2': (np.array([[0.3, -0.2, 0.9], [0.1, 0.4, -0.5]]), 'fallback'),
        'n20': (g.uniform(-1, 1, (20, 3)), 'direction'),
        'identical': (np.tile(np.array([[0.25, -0.5, 0.125]]), (40, 1)), 'fallback'),
        'duplicated': (np.concatenate([dup, dup[::3]], 0), 'direction'),
        'lattice': (lattice, 'unit'),
        'clusters': (clusters, 'direction'),
        'planar': (planar, 'plane'),
        'collinear': (line, 'unit'),
        'negative': (g.uniform(-5, -1, (200, 3)), 'direction'),
    }


def face_cloud(voxel_size=0.25):
    """Points exactly on voxel faces: coordinates o_d + j voxel_size with power-of-two values (min = -2, o = -2.125: every quotient is exact)."""
    g = np.random.default_rng(5)
    j = g.integers(0, 9, (400, 3)).astype(np.float64)
    pts = (-2.0 - 0.5 * voxel_size) + (j + 1.0) * voxel_size
    pts[0] = -2.0                                   # the minimum on every axis: the origin is -2.125
    return pts, voxel_size


# ---- the library's host entries (the __host__ __device__ text of the kernels, no GPU) -----------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _lib():
    from se3et_amd import _lib as L
    return L


def host_voxel(points, voxel_size, normals=None):
    """-> (means, normal means or None, status)"""
    L = _lib()
    p = np.ascontiguousarray(points).reshape(-1, 3)
    nr = None if normals is None else np.ascontiguousarray(normals, p.dtype).reshape(-1, 3)
    out = np.full((max(len(p), 1), 3), -7.0)
    out_n = None if nr is None else np.full((max(len(p), 1), 3), -7.0)
    count, status = np.zeros(1, np.int64), np.zeros(1, np.int32)
    L.check(L.lib().se3_debug_voxel_downsample_host(_ptr(p), len(p), int(p.dtype == np.float64), _ptr(nr), float(voxel_size), _ptr(out), _ptr(out_n),
                                                    _ptr(count), _ptr(status)), 'se3_debug_voxel_downsample_host')
    m = int(count[0])
    return out[:m], (None if out_n is None else out_n[:m]), int(status[0])


def host_knn(support, k, queries=None, dtype=np.float64):
    L = _lib()
    s = np.ascontiguousarray(support, dtype).reshape(-1, 3)
    q = s if queries is None else np.ascontiguousarray(queries, dtype).reshape(-1, 3)
    idx, d2 = np.full((len(q), k), -7, np.int64), np.full((len(q), k), -7.0)
    L.check(L.lib().se3_debug_knn_host(_ptr(q), len(q), _ptr(s), len(s), int(dtype == np.float64), k, _ptr(idx), _ptr(d2)), 'se3_debug_knn_host')
    return idx, d2


def host_normals(points, k=KNN, viewpoint=None):
    L = _lib()
    p = np.ascontiguousarray(points).reshape(-1, 3)
    n, C = np.full((len(p), 3), -7.0), np.full((len(p), 6), -7.0)
    view = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float64)
    L.check(L.lib().se3_debug_knn_normals_host(_ptr(p), len(p), int(p.dtype == np.float64), k, _ptr(view), _ptr(n), _ptr(C)),
            'se3_debug_knn_normals_host')
    return n, C


def voxel_edge_cases():
    g = np.random.default_rng(3)
    face, face_v = face_cloud()
    own = np.stack(np.meshgrid(np.arange(20.0), np.arange(10.0), np.arange(10.0), indexing='ij'), -1).reshape(-1, 3) * 0.5
    return {
        'n0': (np.zeros((0, 3)), 0.1, 0), 'n1': (np.array([[0.3, -0.2, 0.9]]), 0.1, 1),
        'n2': (np.array([[0.3, -0.2, 0.9], [0.31, -0.21, 0.91]]), 0.1, None),
        'identical': (np.tile(np.array([[0.25, -0.5, 0.125]]), (40, 1)), 0.05, 1),
        'faces': (face, face_v, None),
        'negative': (g.uniform(-5, -1, (200, 3)), 0.3, None),
        'one_voxel_600': (cloud('micro').astype(np.float64), 10.0, 1),
        'own_voxels_2000': (own[g.permutation(len(own))], 0.25, 2000),
        'members_64_65_300': (np.concatenate([g.uniform(0.0, 0.4, (64, 3)), g.uniform(2.0, 2.4, (65, 3)), g.uniform(4.0, 4.4, (300, 3))])[g.permutation(429)],
                              1.0, 3),          # (around the library's switch from one thread per voxel to a workgroup: 64 members)
    }


# ---- demands --------------------------------------------------------------------------------------------------------------------------------
def assert_unit(n):
    assert np.isfinite(n).all()
    lo, hi = (1 - Fraction(4) * Fraction(U)) ** 2, (1 + Fraction(4) * Fraction(U)) ** 2
    for row in n:
        s = sum(Fraction(float(v)) ** 2 for v in row)
        assert lo <= s <= hi, 'length^2 - 1 = %g' % float(s - 1)


def assert_covariances(C, tC, m):
    trace = tC[:, 0] + tC[:, 3] + tC[:, 5]
    assert (np.abs(C - tC) <= 4 * m * U * trace[:, None]).all()


def direction_K(n, tn, w):
    """The K each row would need: |n x tn| (l1 - l0) / (2^-53 l2); rows below the gap floor give 0.  -> (K per row, excluded)"""
    with np.errstate(invalid='ignore', divide='ignore'):
        gap = (w[:, 1] - w[:, 0]) / w[:, 2]
        excluded = ~(gap >= GAP_FLOOR)
        K = np.linalg.norm(np.cross(n, tn), axis=1) * gap / U
    K[excluded] = 0.0
    return K, excluded


def assert_directions(n, tn, w, max_excluded=0.01):
    K, excluded = direction_K(n, tn, w)
    assert excluded.sum() <= max_excluded * len(n), '%d rows below the gap floor' % excluded.sum()
    assert (K <= DIRECTION_K).all(), 'K = %g' % K.max()
    return K.max() if len(K) else 0.0


def chamfer_float32_bound(raw, ref, src, gt_transform, transform):
    """Per pair the bound of the reference's float32 metric against the exact one: per point sqrt(11 2^-22 (|x|^2 + |y|^2)) at its nearest
    neighbour -- the (C + 8) 2^-22 bound of INTEGRATION.md "Feature-space matching" at C = 3 through |sqrt(a + e) - sqrt(a)| <= sqrt|e| --
    averaged as the metric averages.  (x, y: the two points of the nearest pair, in the frame the reference measures them in.)"""
    out = []
    for b in range(len(raw)):
        r, q, s = (np.asarray(a[b]).astype(np.float64) for a in (raw, ref, src))
        T, G = np.asarray(transform[b], np.float64), np.asarray(gt_transform[b], np.float64)
        total = 0.0
        for queries, support in ((twin._apply(T, s), r), (q, twin._apply(T @ np.linalg.inv(G), r))):
            idx = twin.knn(support, 1, queries)[0][:, 0]
            total += np.sqrt(11 * 2.0 ** -22 * ((queries ** 2).sum(1) + (support[idx] ** 2).sum(1))).mean()
        out.append(total)
    return np.array(out)
