"""Outlier removal without a GPU: se3_debug_knn_distance_host and se3_debug_distance_stats_host (the text of csrc/outliers.hip,
csrc/outliers_core.h and csrc/fixed_sum.h on host memory), and the ball counts of se3_debug_pair_ball_host that the radius filter is made
of, against the numpy twin (tests/outlier_twin.py) on the clouds of tests/outlier_fixture.py, for float32 and float64 inputs.

The row values a_i and the ball counts are exact and demanded equal.  mean, std and thr must agree with the twin's fsum values to
(n + 16) 2^-53 relative (NaN where the formulas give NaN, on both sides).  The statistical masks are demanded equal on every row the twin
does not flag (|a_i - thr| <= 2 (n + 16) 2^-53 thr); at most 1 % of a cloud's rows may be flagged, and test_fixture_facts pins that the
fixtures have none."""
import numpy as np
import pytest

import outlier_fixture as F
import outlier_twin as twin

CLOUDS = F.clouds()
DTYPES = (np.float64, np.float32)


def test_fixture_facts():
    for name in CLOUDS:
        assert F.facts(name) == F.FACTS[name], name
        assert F.FACTS[name][2] == 0
    assert {F.R_ROWS - 1, F.R_ROWS, F.R_ROWS + 1, F.R_MASK - 1, F.R_MASK, F.R_MASK + 1, 0, 1, 2, F.NB - 1} <= {len(v[0]) for v in CLOUDS.values()}


def _agree(got, want, tolerance):
    return (np.isnan(got) and np.isnan(want)) or abs(got - want) <= tolerance * abs(want)


@pytest.mark.parametrize('dtype', DTYPES, ids=['float64', 'float32'])
@pytest.mark.parametrize('name', list(CLOUDS))
def test_statistical_host_entries_against_the_twin(name, dtype):
    p, nb, ratio, _, _ = CLOUDS[name]
    p = p.astype(dtype)
    ref = F.reference(name)[0] if dtype == np.float64 else twin.statistical(p, nb, ratio)
    got = F.host_statistical(p, nb, ratio)
    assert np.array_equal(got['a'], ref['a'])
    for k, key in enumerate(('mean', 'std', 'thr')):
        print('%s: %s %.17g, twin %.17g' % (name, key, got['stats'][k], ref[key]))
        assert _agree(got['stats'][k], ref[key], ref['tolerance']), key
    assert ref['flagged'].sum() <= 0.01 * len(p)
    sound = ~ref['flagged']
    assert np.array_equal(got['keep'][sound], ref['keep'][sound])
    assert not got['keep'][got['a'] <= 0].any()


@pytest.mark.parametrize('dtype', DTYPES, ids=['float64', 'float32'])
@pytest.mark.parametrize('name', list(CLOUDS))
def test_radius_filter_against_the_twin(name, dtype):
    p, _, _, nb_points, r = CLOUDS[name]
    p = p.astype(dtype)
    ref, got = twin.radius(p, nb_points, r), F.host_radius(p, nb_points, r)
    assert np.array_equal(got['counts'], ref['counts']) and np.array_equal(got['keep'], ref['keep'])


def test_open3d_quirks():
    """n < 2 keeps nothing; a far stray point is dropped and nothing else; fewer points than nb_neighbors: m = n; nb_neighbors or more
    duplicates have a_i = 0 and are dropped; nb_neighbors = 1 keeps nothing (every a_i is 0)."""
    for name in ('n0', 'n1', 'knn_1'):
        assert not F.host_statistical(*CLOUDS[name][:3])['keep'].any(), name
    got = F.host_statistical(*CLOUDS['stray'][:3])
    assert got['keep'].tolist() == [True] * 60 + [False]
    p, nb, ratio = CLOUDS['below_nb'][:3]
    got = F.host_statistical(p, nb, ratio)
    assert np.array_equal(got['a'], F.host_statistical(p, len(p), ratio)['a']) and np.array_equal(got['a'], twin.row_means(p, len(p)))
    got = F.host_statistical(*CLOUDS['duplicates'][:3])
    assert (got['a'][30:] == 0).all() and got['a'][0] == 0 and (got['a'][1:30] > 0).all() and not got['keep'][30:].any() and not got['keep'][0]
    # the radius filter's two strict tests: a point at exactly the radius is not counted, and count == nb_points is not kept
    q = np.array([[0.0, 0, 0], [0.25, 0, 0], [0.25, 0, 0], [0, 0.125, 0]])
    assert F.host_radius(q, 2, 0.25)['counts'].tolist() == [2, 2, 2, 2] and not F.host_radius(q, 2, 0.25)['keep'].any()
    assert F.host_radius(q, 1, 0.25)['keep'].all()


def test_host_entry_refusals():
    from se3et_amd import _lib as L
    p = np.ascontiguousarray(CLOUDS['n5'][0])
    a, stats = np.zeros(5), np.zeros(4)
    lib = L.lib()
    assert lib.se3_debug_knn_distance_host(F._ptr(p), 5, 1, 0, -1, F._ptr(a)) != 0 and b'debug_knn_distance_host' in lib.se3_last_error()
    assert lib.se3_debug_knn_distance_host(F._ptr(p), 5, 1, 65, -1, F._ptr(a)) != 0
    assert lib.se3_debug_knn_distance_host(F._ptr(p), 5, 1, 2, 2, F._ptr(a)) != 0
    for ratio in (0.0, -1.0, np.inf, np.nan):
        assert lib.se3_debug_distance_stats_host(F._ptr(a), 5, ratio, F._ptr(stats), None) != 0
    assert lib.se3_distance_stats_stack(None, None, 0, 1.0, None, None, None) != 0


def test_refusals_before_any_launch():
    import torch
    from se3et_amd.scan_prep import remove_radius_outlier_clouds, remove_statistical_outlier_clouds
    p = torch.zeros(4, 3)
    for nb in (0, 65, 2.5, -1):
        with pytest.raises(ValueError, match='nb_neighbors'):
            remove_statistical_outlier_clouds([p], nb)
    for ratio in (0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match='std_ratio'):
            remove_statistical_outlier_clouds([p], 20, ratio)
    for nb in (-1, 1.5):
        with pytest.raises(ValueError, match='nb_points'):
            remove_radius_outlier_clouds([p], nb, 0.1)
    for r in (0, -0.1, np.inf, np.nan):
        with pytest.raises(ValueError, match='radius'):
            remove_radius_outlier_clouds([p], 3, r)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        remove_statistical_outlier_clouds([p])
    with pytest.raises(RuntimeError, match='GPU tensor'):
        remove_radius_outlier_clouds([p], 3, 0.1)
