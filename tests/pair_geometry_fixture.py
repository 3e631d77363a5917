"""Shared by tests/test_pair_geometry_cpu.py and tests/test_gpu_pair_geometry.py: the fixture tests/golden/pair_geometry.npz (written by
tests/golden/generate_pair_geometry_golden.py from the reference's own functions), the demands made on an implementation against it, and
the edge cases.  The bounds are derived here, per case, from the inputs and the number format -- never from what an implementation gives:
  distances     16 * 2^-52 * max|coordinate| absolute: the rounding of the transform (three products and three sums per coordinate, of
                values no larger than a few times the largest coordinate) carried through the difference and the root;
  covariance    n * 2^-52 * sum|terms| entrywise: the bound of summing n float64 terms in any order;
  everything else is an integer or a ratio of integers and must be equal."""
import functools
import os

import numpy as np

import pair_geometry_twin as twin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pair_geometry.npz')
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def inputs(name):
    return twin.case_inputs(name)


@functools.lru_cache(maxsize=None)
def twin_scan(name):
    """The twin's (distances, indices, correspondences at the case's matching radius), computed once per process."""
    ref, src, T = inputs(name)
    return twin.scan(ref, src, T.astype(np.float64), twin.CASES[name][0])


def distance_bound(name):
    ref, src, T = inputs(name)
    moved = twin.transform_points(src, T.astype(np.float64))
    return 16 * EPS * max(float(np.abs(ref).max()), float(np.abs(src).max()), float(np.abs(moved).max()))


def check_nearest(name, dist, idx):
    g = golden()
    dist, idx = np.asarray(dist), np.asarray(idx)
    assert dist.dtype == np.float64 and idx.dtype == np.int64
    assert np.array_equal(idx, g[name + '/nn_idx'].astype(np.int64)), '%s: nearest-neighbour indices differ' % name
    err, bound = float(np.abs(dist - g[name + '/nn_dist']).max()), distance_bound(name)
    print('%s: nearest-neighbour distance error %.3e (bound %.3e)' % (name, err, bound))
    assert err <= bound


def check_overlaps(name, overlaps):
    g = golden()
    overlaps = np.asarray(overlaps)
    assert overlaps.dtype == np.float64
    assert np.array_equal(overlaps, g[name + '/overlaps']), '%s: overlaps %r, fixture %r' % (name, overlaps, g[name + '/overlaps'])


def check_correspondences(name, corr):
    g = golden()
    corr = np.asarray(corr)
    n_ref = len(inputs(name)[0])
    assert corr.dtype == np.int64 and corr.ndim == 2 and corr.shape[1] == 2
    assert len(corr) == int(g[name + '/corr_total'])
    assert np.array_equal(np.bincount(corr[:, 0], minlength=n_ref), g[name + '/corr_counts'].astype(np.int64))
    assert twin.checksum(corr) == g[name + '/corr_checksum']
    assert np.array_equal(corr[:64], g[name + '/corr_head']) and np.array_equal(corr[-64:], g[name + '/corr_tail'])


def check_info(name, k, overlap, cov, absolute):
    """Record k (the k-th voxel size of the case) against the fixture; `absolute`: the twin's sum of |terms| of the same selection."""
    g = golden()
    assert np.float64(overlap) == g[name + '/info_overlap'][k]
    n = min(int(g[name + '/info_selected'][k]), 5000)
    cov = np.asarray(cov)
    assert cov.dtype == np.float64 and cov.shape == (6, 6)
    bound = n * EPS * absolute
    err = np.abs(cov - g[name + '/info_cov'][k])
    print('%s voxel %g: %d points, covariance error / bound at most %.3e' % (name, g[name + '/voxel_sizes'][k], n,
                                                                               float((err / np.maximum(bound, 1e-300)).max())))
    assert cov[0, 0] == n and np.all(err <= bound)


def edge_cases():
    """name -> (q, s, transform, radius): float32-exact values, so that the transform's products are exact in float64."""
    g = np.random.default_rng(77)
    T = np.eye(4)
    T[:3, :3] = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = [0.25, -0.5, 1.0]
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)          # noqa: E731
    cloud = f32(g.uniform(-1, 1, (400, 3)))
    dup = np.concatenate([cloud[:50], cloud[:50], cloud[25:75]])
    return {
        'far_outside': (f32(g.uniform(-1, 1, (64, 3)) + [500.0, -300.0, 40.0]), cloud, T, 0.2),
        'far_outside_one_axis': (f32(g.uniform(-1, 1, (64, 3)) * [1, 1, 0] + [0.0, 0.0, 900.0]), cloud, np.eye(4), 0.2),
        'one_support_point': (cloud[:40], cloud[7:8], T, 1.5),
        'empty_support': (cloud[:10], np.zeros((0, 3)), T, 0.5),
        'empty_query': (np.zeros((0, 3)), cloud, T, 0.5),
        'duplicated_support': (f32(cloud[:60] @ T[:3, :3].T + T[:3, 3]), dup, T, 0.3),
        'radius_below_every_distance': (f32(cloud[:30] + 10.0), cloud, np.eye(4), 1e-3),
        'one_cell': (f32(g.uniform(0, 1e-3, (50, 3))), f32(g.uniform(0, 1e-3, (80, 3))), np.eye(4), 1.0),
        'planar_support': (cloud[:80], f32(cloud * [1, 1, 0]), T, 0.4),
    }


def check_edge(name, case, dist, idx, corr):
    """An implementation's answers on an edge case against the twin, exactly (same arithmetic, same tie rule)."""
    q, s, T, r = case
    td, ti, tc = twin.scan(q, s, T, r)
    assert np.array_equal(np.asarray(idx), ti), name
    assert np.array_equal(np.asarray(dist), td), name
    corr = np.asarray(corr)
    assert corr.dtype == np.int64 and corr.shape == tc.shape and np.array_equal(corr, tc), name
    if name == 'empty_support':
        assert np.all(np.isinf(dist)) and np.all(np.asarray(idx) == -1) and corr.shape == (0, 2)
    if name == 'radius_below_every_distance':
        assert corr.shape == (0, 2)
    if name == 'duplicated_support':
        assert np.all(np.asarray(idx)[:50] < 50)          # the first copy of a duplicated point wins
    if name == 'one_cell':
        assert len(corr) == len(q) * len(s)
