"""Keypoint selection without a GPU: the numpy twin (tests/keypoint_twin.py) against the reference's recorded outputs
(tests/golden/keypoints.npz), and se3_debug_keypoint_nms_host (the tile step of csrc/keypoint_nms.hip on host memory) against the twin on
the fixture and on every edge cloud of tests/keypoint_fixture.py.  Every comparison is of integer index lists, for equality."""
import os

import numpy as np
import pytest

import keypoint_fixture as F
import keypoint_twin as twin

EDGES = F.edge_cases()


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'keypoints.npz'))


def _case(golden, name):
    return golden[name + '/points'], golden[name + '/feats'], golden[name + '/scores']


@pytest.mark.parametrize('case', F.GOLDEN_CASES, ids=[c[0] for c in F.GOLDEN_CASES])
def test_twin_equals_the_reference(golden, case):
    name, n, radius, K = case
    points, feats, scores = _case(golden, name)
    assert points.shape == (n, 3) and points.dtype == np.float64
    for fn, idx in (('sample_keypoints_with_scores', twin.topk(scores, K)), ('sample_keypoints_with_nms', twin.nms(points, scores, radius, K))):
        assert np.array_equal(golden['%s/%s/points' % (name, fn)], points[idx]), fn
        assert np.array_equal(golden['%s/%s/feats' % (name, fn)], feats[idx]), fn
    # the random form: the full NMS, then the reference's draw over the survivors
    kept = twin.nms(points, scores, radius)
    assert len(kept) > K
    np.random.seed(F.GOLDEN_SEED)
    idx = np.random.choice(kept, K, replace=False, p=scores[kept] / np.sum(scores[kept]))
    assert np.array_equal(golden[name + '/random_sample_keypoints_with_nms/points'], points[idx])
    assert np.array_equal(golden[name + '/random_sample_keypoints_with_nms/feats'], feats[idx])


@pytest.mark.parametrize('case', F.GOLDEN_CASES, ids=[c[0] for c in F.GOLDEN_CASES])
def test_host_entry_equals_the_twin_on_the_fixture(golden, case):
    name, n, radius, K = case
    points, _, scores = _case(golden, name)
    order = twin.rank_order(scores)
    for k in (None, K):
        got, status = F.host_nms(points, order, radius, k)
        assert status == 0 and np.array_equal(got, twin.nms_from_order(points, order, radius, k))


@pytest.mark.parametrize('case', EDGES, ids=[c[0] for c in EDGES])
def test_host_entry_equals_the_twin_on_the_edges(case):
    _, points, scores, radius = case
    order = twin.rank_order(scores)
    full = twin.nms_from_order(points, order, radius)
    for k in (None, 1, max(len(full), 1), len(full) + 3):
        got, status = F.host_nms(points, order, radius, k)
        assert status == 0 and np.array_equal(got, twin.nms_from_order(points, order, radius, k)), k


def test_known_answers():
    by_name = {c[0]: c for c in EDGES}
    for name, want in (('exactly_r', [0, 1]), ('one_ulp_inside', [1]), ('empty', [])):
        _, p, s, r = by_name[name]
        assert twin.nms(p, s, r).tolist() == want, name
    for ascending in (False, True):
        _, p, s, r = by_name['chain_ascending' if ascending else 'chain_descending']
        assert twin.nms(p, s, r).tolist() == (list(range(599, 0, -2)) if ascending else list(range(0, 600, 2)))
    for first in (254, 255):
        p, s, r, shuffle = F.three_point(first)
        order = twin.rank_order(s)
        assert shuffle[order[first:first + 3]].tolist() == [first, first + 1, first + 2]          # A, B, C sit at those ranks
        kept = shuffle[twin.nms(p, s, r)].tolist()
        assert first in kept and first + 1 not in kept and first + 2 in kept and len(kept) == len(s) - 1
    _, p, s, r = by_name['one_ball']
    assert twin.nms(p, s, r).tolist() == [int(np.argmax(s))]
    _, p, s, r = by_name['equal_scores']
    assert twin.rank_order(s).tolist() == list(range(300))                                    # the lower index first
    _, p, s, r = by_name['signed_zeros']
    assert twin.rank_order(s).tolist() == [5] + [i for i in range(300) if i not in (5, 6)] + [6]
    _, p, s, r = by_name['duplicates']
    kept = twin.nms(p, s, r)
    assert len(np.unique(p[kept], axis=0)) == len(kept) and len(kept) <= 40


def test_host_entry_refusals():
    p = np.random.default_rng(0).uniform(0, 1, (20, 3))
    order = np.arange(20)
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[7, 1] = bad
        got, status = F.host_nms(q, order, 0.1)
        assert status == 1 and len(got) == 0
    for wrong in (np.zeros(20), np.arange(1, 21), np.arange(-1, 19)):                          # not a permutation
        got, status = F.host_nms(p, wrong, 0.1)
        assert status == 2 and len(got) == 0
    for radius in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(RuntimeError, match='radius'):
            F.host_nms(p, order, radius)
    with pytest.raises(ValueError):
        twin.rank_order([1.0, np.nan])


@pytest.mark.parametrize('case', F.GOLDEN_CASES, ids=[c[0] for c in F.GOLDEN_CASES])
def test_host_side_dropins_equal_the_reference(golden, case):
    """The two forms that are a draw alone, and the guard of all five: with num_points <= num_keypoints the input comes back untouched."""
    from se3et_amd import keypoints as kp
    name, n, radius, K = case
    points, feats, scores = _case(golden, name)
    for fn, args in (('random_sample_keypoints', (points, feats, K)), ('random_sample_keypoints_with_scores', (points, feats, scores, K))):
        np.random.seed(F.GOLDEN_SEED)
        got = getattr(kp, fn)(*args)
        assert np.array_equal(got[0], golden['%s/%s/points' % (name, fn)]) and np.array_equal(got[1], golden['%s/%s/feats' % (name, fn)])
    for fn in F.GOLDEN_FUNCTIONS:
        for k in (n, n + 1):
            args = [points, feats] + ([scores] if 'scores' in fn or 'nms' in fn else []) + [k] + ([radius] if 'nms' in fn else [])
            got = getattr(kp, fn)(*args)
            assert got[0] is points and got[1] is feats, fn


def test_dropins_are_aliased():
    import sys
    from se3et_amd import dropin, keypoints as kp
    assert 'geotransformer.utils.pointcloud' in dropin.install_aliases()
    import geotransformer.utils.pointcloud as P
    assert sys.modules['geotransformer.utils.pointcloud'] is P
    assert dropin.KEYPOINT_NAMES == F.GOLDEN_FUNCTIONS
    for fn in F.GOLDEN_FUNCTIONS:
        assert getattr(P, fn) is getattr(kp, fn)


def test_refusals_before_any_launch():
    import torch
    from se3et_amd.keypoints import gather_keypoints, nms_keypoints_clouds, random_sample_keypoints_with_scores, topk_keypoints_clouds
    p, s = torch.zeros(4, 3), torch.zeros(4)
    for radius in (0, -0.1, np.inf, np.nan):
        with pytest.raises(ValueError, match='radius'):
            nms_keypoints_clouds([p], [s], radius)
    for K in (0, -3, 2.5):
        with pytest.raises(ValueError, match='num_keypoints'):
            nms_keypoints_clouds([p], [s], 0.1, K)
        with pytest.raises(ValueError, match='num_keypoints'):
            topk_keypoints_clouds([s], K)
    with pytest.raises(ValueError, match='one scores tensor per cloud'):
        nms_keypoints_clouds([p, p], [s], 0.1)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        nms_keypoints_clouds([p], [s], 0.1)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        topk_keypoints_clouds([s], 2)
    with pytest.raises(RuntimeError, match='tensor on the device'):
        nms_keypoints_clouds([p.numpy()], [s], 0.1)
    with pytest.raises(ValueError, match='one tensor per cloud'):
        gather_keypoints([torch.zeros(2, dtype=torch.int64)], [p, p])
    idx = [torch.tensor([2, 0]), torch.tensor([1])]
    pts = [torch.arange(12.).reshape(4, 3), torch.arange(6.).reshape(2, 3)]
    assert [t.tolist() for t in gather_keypoints(idx, pts)] == [[[6., 7., 8.], [0., 1., 2.]], [[3., 4., 5.]]]
    feats = np.zeros((4, 2), np.float32)
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='finite and non-negative'):
            random_sample_keypoints_with_scores(p.numpy(), feats, np.array([1.0, bad, 1.0, 1.0]), 2)
