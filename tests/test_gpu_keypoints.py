"""Keypoint selection on the device (se3et_amd/keypoints.py, csrc/keypoint_nms.hip) against the library's host entry -- the same tile step
on host memory, which tests/test_keypoints_cpu.py pins to the numpy twin -- and against the reference's recorded outputs
(tests/golden/keypoints.npz).  Every comparison is of integer index lists (or of the rows they select), for equality."""
import os

import numpy as np
import pytest
import torch

import keypoint_fixture as F
import keypoint_twin as twin

pytestmark = pytest.mark.gpu

EDGES = F.edge_cases()
DEV = 'cuda'


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device_nms(points, scores, radius, K=None):
    from se3et_amd.keypoints import nms_keypoints_clouds
    out = nms_keypoints_clouds([_gpu(points)], [_gpu(scores)], radius, K)
    assert len(out) == 1 and out[0].dtype == torch.int64 and out[0].is_cuda
    return out[0].cpu().numpy()


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'keypoints.npz'))


@pytest.mark.parametrize('case', EDGES, ids=[c[0] for c in EDGES])
def test_device_equals_the_host_entry(case):
    """Tile edges in float32 and float64, chains across tile boundaries, the strict threshold, ties and duplicates, the grid shapes: K =
    None, 1, the survivor count and above it."""
    _, points, scores, radius = case
    order = twin.rank_order(scores)
    full, status = F.host_nms(points, order, radius)
    assert status == 0
    for k in (None, 1, max(len(full), 1), len(full) + 3):
        want, _ = F.host_nms(points, order, radius, k)
        assert np.array_equal(_device_nms(points, scores, radius, k), want), k


def test_known_answers():
    by_name = {c[0]: c for c in EDGES}
    for name, want in (('exactly_r', [0, 1]), ('one_ulp_inside', [1]), ('empty', [])):
        _, p, s, r = by_name[name]
        assert _device_nms(p, s, r).tolist() == want, name
    _, p, s, r = by_name['chain_descending']
    assert _device_nms(p, s, r).tolist() == list(range(0, 600, 2))
    _, p, s, r = by_name['chain_ascending']
    assert _device_nms(p, s, r).tolist() == list(range(599, 0, -2))
    for first in (254, 255):
        p, s, r, shuffle = F.three_point(first)
        kept = shuffle[_device_nms(p, s, r)].tolist()
        assert first in kept and first + 1 not in kept and first + 2 in kept and len(kept) == len(s) - 1
    _, p, s, r = by_name['one_ball']
    assert _device_nms(p, s, r).tolist() == [int(np.argmax(s))]


def test_ranking_ties():
    """Identical scores keep the lower index first; -0.0 equals 0.0; infinities order as numbers."""
    from se3et_amd.keypoints import topk_keypoints_clouds
    by_name = {c[0]: c for c in EDGES}
    names = ('equal_scores', 'few_score_levels', 'signed_zeros', 'infinite_scores', 'duplicates')
    scores = [by_name[n][2] for n in names] + [by_name['signed_zeros'][2].astype(np.float32)]
    for K in (None, 1, 17):
        got = topk_keypoints_clouds([_gpu(s) for s in scores], K)
        for s, g in zip(scores, got):
            assert g.dtype == torch.int64 and np.array_equal(g.cpu().numpy(), twin.topk(s, K))


def test_batch_of_33_equals_the_single_calls():
    """33 clouds cross the chunk of 32; n = 0, n = 1, float32 and float64 clouds side by side; every list equals the one from a call with
    that cloud alone, and two runs agree."""
    from se3et_amd.keypoints import gather_keypoints, nms_keypoints_clouds
    sizes = [0, 1, 300, 257] + [40 + 23 * i for i in range(28)] + [513]
    assert len(sizes) == 33
    radius, K = 0.08, 60
    clouds = [F.random_cloud(n, 500 + i, np.float32 if i % 2 else np.float64)[:2] for i, n in enumerate(sizes)]
    pts, scs = [_gpu(p) for p, _ in clouds], [_gpu(s.astype(np.float32) if i % 3 == 0 else s) for i, (_, s) in enumerate(clouds)]
    first = nms_keypoints_clouds(pts, scs, radius, K)
    second = nms_keypoints_clouds(pts, scs, radius, K)
    assert len(first) == 33 and first[0].numel() == 0 and first[1].tolist() == [0]
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), i
        alone = nms_keypoints_clouds([pts[i]], [scs[i]], radius, K)[0]
        assert torch.equal(a, alone), i
        want, _ = F.host_nms(clouds[i][0], twin.rank_order(scs[i].cpu().numpy()), radius, K)
        assert np.array_equal(a.cpu().numpy(), want), i
    kp, ks = gather_keypoints(first, pts, scs)
    assert all(torch.equal(k, p[i]) and torch.equal(v, s[i]) for k, v, p, s, i in zip(kp, ks, pts, scs, first))
    assert nms_keypoints_clouds([], [], radius) == []


def _rows_equal(got, want_points, want_feats):
    assert np.array_equal(got[0], want_points) and np.array_equal(got[1], want_feats)


@pytest.mark.parametrize('case', F.GOLDEN_CASES, ids=[c[0] for c in F.GOLDEN_CASES])
def test_dropins_return_the_references_rows(golden, case):
    from se3et_amd import keypoints as kp
    name, n, radius, K = case
    points, feats, scores = golden[name + '/points'], golden[name + '/feats'], golden[name + '/scores']
    for fn in F.GOLDEN_FUNCTIONS:
        args = [points, feats] + ([scores] if 'scores' in fn or 'nms' in fn else []) + [K] + ([radius] if 'nms' in fn else [])
        np.random.seed(F.GOLDEN_SEED)
        _rows_equal(getattr(kp, fn)(*args), golden['%s/%s/points' % (name, fn)], golden['%s/%s/feats' % (name, fn)])
        for k in (n, n + 1):                                            # the reference's guard: the input comes back untouched
            args[-2 if 'nms' in fn else -1] = k
            got = getattr(kp, fn)(*args)
            assert got[0] is points and got[1] is feats, fn


def test_dropins_are_aliased():
    import sys
    from se3et_amd import dropin, keypoints as kp
    dropin.install_aliases()
    import geotransformer.utils.pointcloud as P
    assert sys.modules['geotransformer.utils.pointcloud'] is P
    for fn in F.GOLDEN_FUNCTIONS:
        assert getattr(P, fn) is getattr(kp, fn)


def test_refusals():
    from se3et_amd.keypoints import (nms_keypoints_clouds, random_sample_keypoints_with_nms, random_sample_keypoints_with_scores,
                                     topk_keypoints_clouds)
    p, s, r = F.random_cloud(50, 1)
    good_p, good_s = _gpu(p), _gpu(s)
    for bad in (np.nan, np.inf):
        q = p.copy()
        q[9, 2] = bad
        with pytest.raises(ValueError, match='cloud 1: a point is not finite'):
            nms_keypoints_clouds([good_p, _gpu(q), good_p], [good_s] * 3, r)
    t = s.copy()
    t[4] = np.nan
    with pytest.raises(ValueError, match='cloud 2: a score is NaN'):
        nms_keypoints_clouds([good_p] * 3, [good_s, good_s, _gpu(t)], r)
    with pytest.raises(ValueError, match='cloud 0: a score is NaN'):
        topk_keypoints_clouds([_gpu(t)], 5)
    for radius in (0, -0.1, np.inf, np.nan):
        with pytest.raises(ValueError, match='radius'):
            nms_keypoints_clouds([good_p], [good_s], radius)
    for K in (0, -3, 2.5):
        with pytest.raises(ValueError, match='num_keypoints'):
            nms_keypoints_clouds([good_p], [good_s], r, K)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        nms_keypoints_clouds([torch.from_numpy(p)], [good_s], r)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        nms_keypoints_clouds([good_p], [torch.from_numpy(s)], r)
    with pytest.raises(RuntimeError):
        nms_keypoints_clouds([p], [good_s], r)
    with pytest.raises(ValueError, match='one scores tensor per cloud'):
        nms_keypoints_clouds([good_p, good_p], [good_s], r)
    with pytest.raises(ValueError, match='scores'):
        nms_keypoints_clouds([good_p], [good_s[:-1]], r)
    feats = np.zeros((50, 2), np.float32)
    for bad in (-1.0, np.nan, np.inf):
        t = s.copy()
        t[0] = bad
        with pytest.raises(ValueError):
            random_sample_keypoints_with_scores(p, feats, t, 10)
    t = s.copy()
    t[0] = -1.0
    with pytest.raises(ValueError):
        random_sample_keypoints_with_nms(p, feats, t, 3, 1e-3)
