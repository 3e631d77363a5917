"""The cases of the outlier-removal tests (tests/test_outlier_cpu.py, tests/test_gpu_outliers.py), and the calls of the library's host entries.

Clouds: name -> (points, nb_neighbors, std_ratio, nb_points, radius).
  scan         the surface patch of tests/iss_fixture.py (2000 points) with 40 stray points, default_rng(3), uniform in the unit box.
  edge clouds  n = 0, 1, 2; R - 1, R, R + 1 rows for R = 4 (knn_distance_kernel: one wave per row) and R = 256 (the mask kernel, and the
               lanes of the fixed-shape sum); one far stray point; a cloud of nb_neighbors - 1 points; duplicates (a_i = 0: never kept).
FACTS pins, per cloud, the rows each filter keeps and the rows the twin flags; the fixtures are chosen so that it flags none."""
import ctypes
import functools

import numpy as np

import iss_fixture as I
import outlier_twin as twin

U = 2.0 ** -53
R_ROWS, R_MASK = 4, 256
NB, RATIO = 20, 2.0

# cloud -> (kept by the statistical filter, kept by the radius filter, flagged rows)
FACTS = {'scan': (2010, 1881, 0), 'n0': (0, 0, 0), 'n1': (0, 0, 0), 'n2': (0, 0, 0), 'n3': (3, 0, 0), 'n4': (4, 0, 0), 'n5': (5, 3, 0),
         'n255': (216, 142, 0), 'n256': (213, 151, 0), 'n257': (218, 163, 0), 'stray': (60, 60, 0), 'below_nb': (16, 12, 0),
         'duplicates': (27, 28, 0), 'knn_1': (0, 50, 0), 'knn_64': (104, 58, 0)}


@functools.lru_cache(None)
def clouds():
    g = np.random.default_rng(3)
    out = {'scan': (np.concatenate([I.patch(2000, 0), g.uniform(0, 1, (40, 3))])[g.permutation(2040)], NB, RATIO, 8, 0.05)}
    for n in (0, 1, 2, R_ROWS - 1, R_ROWS, R_ROWS + 1):
        out['n%d' % n] = (g.uniform(0, 0.3, (n, 3)), NB, RATIO, 2, 0.2)
    for n in (R_MASK - 1, R_MASK, R_MASK + 1):
        out['n%d' % n] = (g.uniform(0, 1, (n, 3)), NB, 1.0, 6, 0.2)
    out['stray'] = (np.concatenate([g.uniform(0, 0.2, (60, 3)), [[5.0, 5.0, 5.0]]]), NB, RATIO, 3, 0.1)
    out['below_nb'] = (g.uniform(0, 0.2, (NB - 1, 3)), NB, 1.0, 3, 0.1)
    dup = g.uniform(0, 0.2, (30, 3))
    out['duplicates'] = (np.concatenate([dup, np.tile(dup[:1], (NB + 4, 1))]), NB, RATIO, NB, 0.05)
    out['knn_1'] = (g.uniform(0, 0.2, (50, 3)), 1, RATIO, 0, 0.05)                       # the row itself alone: a_i = 0, nothing kept
    out['knn_64'] = (g.uniform(0, 0.2, (150, 3)), 64, 0.5, 40, 0.1)
    for v in out.values():
        v[0].setflags(write=False)
    return out


@functools.lru_cache(None)
def reference(name):
    p, nb, ratio, nb_points, r = clouds()[name]
    return twin.statistical(p, nb, ratio), twin.radius(p, nb_points, r)


def facts(name):
    s, r = reference(name)
    return (int(s['keep'].sum()), int(r['keep'].sum()), int(s['flagged'].sum()))


# ---- the library's host entries (the __host__ __device__ text of the kernels, no GPU) --------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_statistical(points, nb_neighbors=NB, std_ratio=RATIO):
    """se3_debug_knn_distance_host and se3_debug_distance_stats_host: {'a' (n,), 'stats' (4: mean, std, thr, resolution), 'keep' (n,) bool}"""
    from se3et_amd import _lib as L
    p = np.ascontiguousarray(points).reshape(-1, 3)
    assert p.dtype in (np.float32, np.float64)
    n = len(p)
    a, stats, mask = np.full(max(n, 1), -7.0), np.full(4, -7.0), np.full(max(n, 1), 7, np.uint8)
    L.check(L.lib().se3_debug_knn_distance_host(_ptr(p if n else np.zeros((1, 3), p.dtype)), n, int(p.dtype == np.float64), int(nb_neighbors), -1,
                                                _ptr(a)), 'se3_debug_knn_distance_host')
    L.check(L.lib().se3_debug_distance_stats_host(_ptr(a), n, float(std_ratio), _ptr(stats), _ptr(mask)), 'se3_debug_distance_stats_host')
    return {'a': a[:n], 'stats': stats, 'keep': mask[:n].astype(bool)}


def host_radius(points, nb_points, radius):
    """The ball counts of se3_debug_pair_ball_host and the filter's test on them: {'counts' (n,), 'keep' (n,) bool}"""
    from se3et_amd import _lib as L
    p = np.ascontiguousarray(points).reshape(-1, 3)
    n = len(p)
    q = p if n else np.zeros((1, 3), p.dtype)
    eye, counts, total = np.eye(4), np.zeros(max(n, 1), np.int64), np.zeros(1, np.int64)
    L.check(L.lib().se3_debug_pair_ball_host(_ptr(q), n, _ptr(q), n, int(p.dtype == np.float64), _ptr(eye), float(radius), _ptr(counts), None, 0,
                                             _ptr(total)), 'se3_debug_pair_ball_host')
    return {'counts': counts[:n], 'keep': counts[:n] > int(nb_points)}
