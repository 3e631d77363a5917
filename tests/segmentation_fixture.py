"""Synthetic inputs of the segmentation tests (nothing is taken from any dataset): the plane cases and DBSCAN clouds that
tests/test_segmentation_cpu.py and tests/test_gpu_segmentation.py share, the references of tests/segmentation_twin.py computed once, the
conditions that make the compared integers well-defined across summation orders (asserted here: a fixture that does not meet them fails),
and the library's host entries (the __host__ __device__ text of the kernels, no GPU)."""
import ctypes
import functools

import numpy as np

import segmentation_twin as twin

TILE, SEGMENT = 128, 1024            # SE3_PLANE_TILE, SE3_PLANE_SEGMENT (test_segmentation_cpu.py checks them against the header)
MARGIN = 1e-9                        # no |dist| this close to the threshold; no equal-count error sums this close (relative); no pair
GAP = 1e-6                           # distance this close to eps (relative); no eigenvector fit with its two smallest eigenvalues this close


def slab(n, seed, outliers=0.3, noise=0.01):
    """A noisy tilted plane patch among uniform outliers, shuffled."""
    rng = np.random.default_rng(seed)
    m = int(n * (1 - outliers))
    uv = rng.uniform(-1, 1, (m, 2))
    normal = np.array([0.3, -0.2, 0.93])
    normal /= np.linalg.norm(normal)
    e1 = np.cross(normal, [1.0, 0, 0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(normal, e1)
    p = uv[:, :1] * e1 + uv[:, 1:] * e2 + rng.normal(0, noise, (m, 1)) * normal + np.array([0.5, -0.25, 1.0])
    q = rng.uniform(-1, 1, (n - m, 3)) + np.array([0.5, -0.25, 1.0])
    return rng.permutation(np.concatenate([p, q]))


def _coplanar():
    g = np.arange(8) / 8.0
    x, y = np.meshgrid(g[:5], g)
    return np.stack([x.ravel(), y.ravel(), np.full(x.size, 0.25)], 1)


def _collinear():
    return np.arange(20.0)[:, None] * np.array([[0.125, 0.25, 0.5]])


def _seed_for(n, ransac_n, want):
    """The lowest seed whose hypothesis 0 draws the rows `want` (a set) of n."""
    for seed in range(100000):
        if set(twin.sample_indices(seed, n, 1, ransac_n)[0].tolist()) == set(want):
            return seed
    raise AssertionError('no seed found')


EDGE = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [0.5, 0.5, 0.25]])          # row 3 is exactly 0.5 from z = 0


@functools.lru_cache(None)
def planes():
    """name -> (points, distance_threshold, ransac_n, num_iterations, seed, deliberate ties)"""
    c = {'slab': (slab(300, 1), 0.03, 3, 100, 0, False),
         'rn4': (slab(300, 2), 0.03, 4, 64, 1, False),
         'rn16': (slab(300, 3), 0.03, 16, 64, 2, False),
         'h1': (slab(200, 4, outliers=0.0), 0.03, 3, 1, 1, False),
         'h1_none': (slab(200, 4, outliers=0.0), 0.03, 3, 1, 3, True),          # (its one sample draws a row twice)
         'coplanar': (_coplanar(), 0.5, 3, 20, 0, True),
         'coplanar4': (_coplanar(), 0.5, 4, 20, 0, True),
         'collinear': (_collinear(), 0.5, 3, 20, 0, True),
         'n2': (slab(2, 5), 0.03, 3, 10, 0, True),
         'n3': (np.array([[0.0, 0, 0.5], [1, 0, 0.5], [0, 1, 0.5]]), 0.03, 3, 10, _seed_for(3, 3, {0, 1, 2}), True),
         'n0': (np.zeros((0, 3)), 0.03, 3, 4, 0, True)}
    for k, H in (('tile_m1', TILE - 1), ('tile', TILE), ('tile_p1', TILE + 1)):
        c[k] = (slab(200, 7), 0.03, 3, H, 4, False)
    for k, n in (('seg_m1', SEGMENT - 1), ('seg', SEGMENT), ('seg_p1', SEGMENT + 1), ('seg2_p1', 2 * SEGMENT + 1)):
        c[k] = (slab(n, 8 + n), 0.03, 3, 16, 5, False)
    return c


@functools.lru_cache(None)
def plane_reference(name):
    """The twin's answer for a plane case, with the fixture's conditions asserted."""
    p, thr, rn, H, seed, ties = planes()[name]
    ref = twin.segment_plane(p, thr, rn, H, seed)
    if not ties:
        assert ref['status'] == twin.OK, name
        assert ref['margin'] > MARGIN, (name, ref['margin'])
        assert ref['tie'] > MARGIN, (name, ref['tie'])
        assert ref['gap'] > GAP, (name, ref['gap'])
    return ref


@functools.lru_cache(None)
def plane_tolerance(name):
    """16 times the twin's own spread between two formulations, at least 1e-13, per quantity."""
    p, thr, rn, H, seed, _ = planes()[name]
    spread = twin.plane_spread(p, thr, rn, H, seed)
    return {k: max(16 * v, 1e-13) for k, v in spread.items()}, spread


def _blobs():
    rng = np.random.default_rng(11)
    centres = np.array([[0.0, 0, 0], [2, 0.5, 0], [0.5, 2, 1]])
    p = np.concatenate([c + rng.normal(0, 0.15, (110, 3)) for c in centres] + [rng.uniform(-1, 3, (70, 3))])
    return rng.permutation(p)


def _line(xs):
    return np.stack([np.asarray(xs, np.float64), np.zeros(len(xs)), np.zeros(len(xs))], 1)


_A, _B, _BORDER = [0.0, 0.3, 0.6, 0.9], [2.7, 3.0, 3.3, 3.6], [1.8]          # eps 1, min_points 4: 1.8 is a border row of both


def _star():
    leaves = np.array([[0.9, 0, 0], [-0.45, 0.78, 0], [-0.45, -0.78, 0]]) + np.array([10.0, 0, 0])
    return np.concatenate([leaves, _line(_A), np.array([[10.0, 0, 0]])])


def _chain(order):
    x = 0.9 * 0.05 * np.arange(2049)
    rng = np.random.default_rng(12)
    return _line(x[::-1] if order == 'reversed' else rng.permutation(x))


def _wide():
    rng = np.random.default_rng(13)
    return np.stack([rng.uniform(0, 20, 1500), rng.uniform(0, 0.05, 1500), rng.uniform(0, 0.05, 1500)], 1)


@functools.lru_cache(None)
def clouds():
    """name -> (points, eps, min_points)"""
    rng = np.random.default_rng(14)
    dup = np.concatenate([np.zeros((6, 3)), np.full((2, 3), 0.05), np.full((1, 3), 5.0), np.zeros((3, 3))])
    return {'blobs': (_blobs(), 0.3, 5),
            'n0': (np.zeros((0, 3)), 0.5, 1),
            'n1_own': (np.array([[1.0, 2, 3]]), 0.5, 1),
            'n1_noise': (np.array([[1.0, 2, 3]]), 0.5, 2),
            'all_noise': (rng.uniform(0, 10, (50, 3)), 0.2, 3),
            'duplicates': (dup, 0.1, 4),
            'border_between': (_line(_A + _B + _BORDER), 1.0, 4),
            'border_first': (_line(_BORDER + _B + _A), 1.0, 4),
            'last_core': (_star(), 1.0, 4),
            'chain_reversed': (_chain('reversed'), 0.05, 2),
            'chain_shuffled': (_chain('shuffled'), 0.05, 2),
            'wide': (_wide(), 0.1, 5)}


@functools.lru_cache(None)
def cloud_reference(name):
    p, eps, min_points = clouds()[name]
    return twin.cluster_dbscan(p, eps, min_points)


def sklearn_comparable(name):
    """No pair distance lies within 1e-9 eps of eps: scikit-learn's d <= eps and the contract's d < eps are the same question."""
    p, eps, _ = clouds()[name]
    return twin.eps_margin(p, eps) > MARGIN


# ---- the library's host entries ----------------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_plane(points, thr, ransac_n=3, num_iterations=100, seed=0):
    """se3_debug_plane_host: the dict of the twin's keys (mask as bool)."""
    from se3et_amd import _lib as L
    p = np.ascontiguousarray(points)
    assert p.dtype in (np.float32, np.float64)
    n, H = len(p), int(num_iterations)
    plane, mask = np.full(4, -7.0), np.full(max(n, 1), 7, np.uint8)
    count, status, best = (np.full(1, -7, np.int32) for _ in range(3))
    fitness, rmse = np.full(1, -7.0), np.full(1, -7.0)
    hc, he = np.full(H, -7, np.int32), np.full(H, -7.0)
    L.check(L.lib().se3_debug_plane_host(_ptr(p if n else np.zeros((1, 3), p.dtype)), n, int(p.dtype == np.float64), float(thr), int(ransac_n), H,
                                         int(seed), _ptr(plane), _ptr(mask), _ptr(count), _ptr(fitness), _ptr(rmse), _ptr(status), _ptr(best),
                                         _ptr(hc), _ptr(he)), 'se3_debug_plane_host')
    return dict(plane=plane, mask=mask[:n].astype(bool), count=int(count[0]), fitness=float(fitness[0]), inlier_rmse=float(rmse[0]),
                status=int(status[0]), best_hypothesis=int(best[0]), hyp_counts=hc, hyp_errs=he)


def host_dbscan(points, eps, min_points):
    """se3_debug_dbscan_host: (labels (n,) int32, num_clusters)"""
    from se3et_amd import _lib as L
    p = np.ascontiguousarray(points)
    assert p.dtype in (np.float32, np.float64)
    n = len(p)
    labels, num = np.full(max(n, 1), -7, np.int32), np.full(1, -7, np.int64)
    L.check(L.lib().se3_debug_dbscan_host(_ptr(p if n else np.zeros((1, 3), p.dtype)), n, int(p.dtype == np.float64), float(eps), int(min_points),
                                          _ptr(labels), _ptr(num)), 'se3_debug_dbscan_host')
    return labels[:n], int(num[0])
