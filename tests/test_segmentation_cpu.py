"""Plane segmentation and DBSCAN without a GPU: se3_debug_plane_host and se3_debug_dbscan_host (the text of csrc/plane_core.h and
csrc/dbscan_core.h on host memory) against the numpy twins (tests/segmentation_twin.py) on the cases of tests/segmentation_fixture.py.

Plane: the winning hypothesis, the per-hypothesis counts, the inlier sets and the status are integers and demanded equal; the fixture
asserts the margins that make them well-defined.  Plane coefficients, fitness and inlier_rmse must agree within 16 times the twin's own
spread between two formulations (eigh against Jacobi, sums ascending against descending), and at least 1e-13.  DBSCAN: labels equal the
twin's, and scikit-learn's where no pair distance is within 1e-9 eps of eps."""
import numpy as np
import pytest

import segmentation_fixture as F
import segmentation_twin as twin

PLANES = F.planes()
CLOUDS = F.clouds()


def test_limits_are_the_headers():
    from se3et_amd import _lib, ops
    assert _lib.ENUMS['se3_plane_status'] == {'SE3_PLANE_OK': twin.OK, 'SE3_PLANE_TOO_FEW': twin.TOO_FEW, 'SE3_PLANE_NONE': twin.NONE}
    assert (ops.PLANE_TILE, ops.PLANE_SEGMENT, ops.PLANE_MAX_SAMPLE) == (F.TILE, F.SEGMENT, 16)
    for name in ('se3_plane_segment_stack', 'se3_plane_segment_workspace_bytes', 'se3_dbscan_stack', 'se3_dbscan_workspace_bytes',
                 'se3_debug_plane_host', 'se3_debug_dbscan_host'):
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES, name
    assert {len(v[0]) for v in PLANES.values()} >= {0, 2, 3, F.SEGMENT - 1, F.SEGMENT, F.SEGMENT + 1, 2 * F.SEGMENT + 1}
    assert {v[3] for v in PLANES.values()} >= {1, F.TILE - 1, F.TILE, F.TILE + 1} and {v[2] for v in PLANES.values()} >= {3, 4, 16}


@pytest.mark.parametrize('name', list(PLANES))
def test_plane_host_entry_against_the_twin(name):
    p, thr, rn, H, seed, _ = PLANES[name]
    ref, got = F.plane_reference(name), F.host_plane(p, thr, rn, H, seed)
    tol, spread = F.plane_tolerance(name)
    print('%s: status %d, h %d, count %d; twin spread %r' % (name, got['status'], got['best_hypothesis'], got['count'], spread))
    assert got['status'] == ref['status'] and got['best_hypothesis'] == ref['best_hypothesis'] and got['count'] == ref['count']
    assert np.array_equal(got['hyp_counts'], ref['hyp_counts'])
    assert np.array_equal(got['mask'], ref['mask'])
    for key in ('plane', 'fitness', 'inlier_rmse'):
        print('  %s: %r, twin %r, allowed %.3g' % (key, got[key], ref[key], tol[key]))
        assert np.max(np.abs(np.asarray(got[key]) - np.asarray(ref[key]))) <= tol[key], key
    if ref['status'] == twin.OK:
        e = ref['hyp_errs']
        assert np.all(np.abs(got['hyp_errs'] - e) <= 1e-10 * e + 1e-30)


def test_plane_float32_points_are_promoted():
    p, thr, rn, H, seed, _ = PLANES['slab']
    p32 = p.astype(np.float32)
    a, b = F.host_plane(p32, thr, rn, H, seed), F.host_plane(p32.astype(np.float64), thr, rn, H, seed)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_plane_deliberate_cases():
    from se3et_amd.ransac import sample_indices
    # exactly coplanar on z = 0.25: every valid hypothesis ties on the count and on error 0, so the lowest valid h wins
    p, thr, rn, H, seed, _ = PLANES['coplanar']
    got = F.host_plane(p, thr, rn, H, seed)
    idx = sample_indices(seed, len(p), H, rn)
    valid = [bool(np.any(np.cross(p[i[1]] - p[i[0]], p[i[2]] - p[i[0]]))) for i in idx]
    assert got['best_hypothesis'] == valid.index(True) and got['status'] == twin.OK and got['count'] == len(p) and got['mask'].all()
    assert np.array_equal(got['hyp_counts'], np.where(valid, len(p), 0)) and not got['hyp_errs'].any()
    assert got['plane'].tolist() == [0.0, 0.0, 1.0, -0.25] and got['inlier_rmse'] == 0.0 and got['fitness'] == 1.0
    # collinear rows: no plane
    p, thr, rn, H, seed, _ = PLANES['collinear']
    got = F.host_plane(p, thr, rn, H, seed)
    assert got['status'] == twin.NONE and got['best_hypothesis'] == -1 and not got['mask'].any() and not got['plane'].any()
    assert not got['hyp_counts'].any()
    # too few rows; exactly ransac_n rows
    assert F.host_plane(*PLANES['n2'][:5])['status'] == twin.TOO_FEW and F.host_plane(*PLANES['n0'][:5])['status'] == twin.TOO_FEW
    got = F.host_plane(*PLANES['n3'][:5])
    assert got['status'] == twin.OK and got['best_hypothesis'] == 0 and got['count'] == 3 and got['fitness'] == 1.0
    # a row exactly distance_threshold = 0.5 from the hypothesis plane z = 0 is not an inlier
    seed = F._seed_for(len(F.EDGE), 3, {0, 1, 2})
    got = F.host_plane(F.EDGE, 0.5, 3, 1, seed)
    assert got['hyp_counts'].tolist() == [4] and got['hyp_errs'].tolist() == [0.0625]
    assert F.host_plane(F.EDGE, np.nextafter(0.5, 1), 3, 1, seed)['hyp_counts'].tolist() == [5]


def test_plane_host_entry_refusals():
    from se3et_amd import _lib as L
    lib = L.lib()
    p = np.ascontiguousarray(PLANES['slab'][0])
    o = [F._ptr(np.zeros(len(p) * 8)) for _ in range(7)]
    for thr, rn, H in ((0.0, 3, 10), (-1.0, 3, 10), (np.inf, 3, 10), (np.nan, 3, 10), (0.1, 2, 10), (0.1, 17, 10), (0.1, 3, 0)):
        assert lib.se3_debug_plane_host(F._ptr(p), len(p), 1, thr, rn, H, 0, *o, None, None) != 0
        assert b'debug_plane_host' in lib.se3_last_error()
    assert lib.se3_plane_segment_stack(None, 1, None, 0, 0.1, 3, 10, 0, *[None] * 10, 0, None) != 0
    assert lib.se3_dbscan_stack(None, 0, 0, None, 1, None, 0, 0.1, 1, None, None, None, 0, None) != 0
    for eps, mp in ((0.0, 1), (np.nan, 1), (np.inf, 1), (0.1, 0)):
        assert lib.se3_debug_dbscan_host(F._ptr(p), len(p), 1, eps, mp, o[0], o[1]) != 0 and b'debug_dbscan_host' in lib.se3_last_error()


def test_refusals_before_any_launch():
    import torch
    from se3et_amd.segmentation import cluster_dbscan_clouds, segment_plane_clouds, segment_planes_clouds
    p = torch.zeros(4, 3)
    for thr in (0, -0.1, np.inf, np.nan):
        with pytest.raises(ValueError, match='segment_plane_clouds: distance_threshold'):
            segment_plane_clouds([p], thr)
    for rn in (2, 17, 3.5):
        with pytest.raises(ValueError, match='segment_plane_clouds: ransac_n'):
            segment_plane_clouds([p], 0.1, rn)
    with pytest.raises(ValueError, match='segment_plane_clouds: num_iterations'):
        segment_plane_clouds([p], 0.1, 3, 0)
    with pytest.raises(ValueError, match='segment_planes_clouds: max_planes'):
        segment_planes_clouds([p], 0.1, 0)
    for eps in (0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match='cluster_dbscan_clouds: eps'):
            cluster_dbscan_clouds([p], eps, 3)
    for mp in (0, 2.5):
        with pytest.raises(ValueError, match='cluster_dbscan_clouds: min_points'):
            cluster_dbscan_clouds([p], 0.1, mp)
    from se3et_amd.fpfh import global_registration_pairs
    for planes in (-1, 1.5):
        with pytest.raises(ValueError, match='global_registration_pairs: remove_planes'):
            global_registration_pairs([p], [p], 0.1, remove_planes=planes)
    for size in (0, 2.5):
        with pytest.raises(ValueError, match='global_registration_pairs: keep_clusters'):
            global_registration_pairs([p], [p], 0.1, keep_clusters=size)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        segment_plane_clouds([p], 0.1)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        cluster_dbscan_clouds([p], 0.1, 3)


@pytest.mark.parametrize('dtype', (np.float64, np.float32), ids=['float64', 'float32'])
@pytest.mark.parametrize('name', list(CLOUDS))
def test_dbscan_host_entry_against_the_twin(name, dtype):
    p, eps, min_points = CLOUDS[name]
    p = p.astype(dtype)
    labels, num = F.cloud_reference(name) if dtype == np.float64 else twin.cluster_dbscan(p, eps, min_points)
    got, got_num = F.host_dbscan(p, eps, min_points)
    print('%s: %d rows, %d clusters, %d noise' % (name, len(p), got_num, int((got == -1).sum())))
    assert got_num == num and np.array_equal(got, labels)


@pytest.mark.parametrize('name', [k for k, v in CLOUDS.items() if len(v[0])])          # (scikit-learn refuses an empty array)
def test_dbscan_against_scikit_learn(name):
    cluster = pytest.importorskip('sklearn.cluster')
    p, eps, min_points = CLOUDS[name]
    assert F.sklearn_comparable(name), name
    want = cluster.DBSCAN(eps=eps, min_samples=min_points).fit(p).labels_
    got, _ = F.host_dbscan(p, eps, min_points)
    assert np.array_equal(got, want)


def test_dbscan_deliberate_cases():
    # the strict edge: two rows exactly eps = 0.5 apart on an axis are not neighbours
    two = np.array([[0.0, 0, 0], [0.5, 0, 0]])
    assert F.host_dbscan(two, 0.5, 2)[0].tolist() == [-1, -1] and F.host_dbscan(two, 0.5, 1)[0].tolist() == [0, 1]
    assert F.host_dbscan(two, np.nextafter(0.5, 1), 2)[0].tolist() == [0, 0]
    assert F.host_dbscan(*CLOUDS['n0'])[1] == 0
    assert F.host_dbscan(*CLOUDS['n1_own'])[0].tolist() == [0] and F.host_dbscan(*CLOUDS['n1_noise'])[0].tolist() == [-1]
    labels, num = F.host_dbscan(*CLOUDS['all_noise'])
    assert num == 0 and (labels == -1).all()
    labels, num = F.host_dbscan(*CLOUDS['duplicates'])
    assert labels.tolist() == [0] * 8 + [-1] + [0] * 3 and num == 1
    # a border row between two clusters gets the lower label, also when its index is lower than both clusters' seeds
    assert F.host_dbscan(*CLOUDS['border_between'])[0].tolist() == [0] * 4 + [1] * 4 + [0]
    assert F.host_dbscan(*CLOUDS['border_first'])[0].tolist() == [0] + [0] * 4 + [1] * 4
    # a cluster whose lowest (and only) core row is the cloud's last row
    assert F.host_dbscan(*CLOUDS['last_core'])[0].tolist() == [1] * 3 + [0] * 4 + [1]
    for name in ('chain_reversed', 'chain_shuffled'):
        labels, num = F.host_dbscan(*CLOUDS[name])
        assert num == 1 and not labels.any() and len(labels) == 2049
    p, eps, _ = CLOUDS['wide']
    assert np.ptp(p[:, 0]) > 64 * eps
