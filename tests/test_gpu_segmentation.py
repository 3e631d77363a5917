"""Plane segmentation and DBSCAN on the device (se3et_amd/segmentation.py, csrc/plane.hip, csrc/dbscan.hip) against the library's host
entries -- the same text on host memory, which tests/test_segmentation_cpu.py pins to the numpy twins -- bit for bit, on every case of
tests/segmentation_fixture.py; a cloud alone, at positions 0 and 31 of a batch and through the chunking at 33 clouds; from run to run;
the plane peeling, the two new arguments of global_registration_pairs and the numpy drop-ins."""
import numpy as np
import pytest
import torch

import segmentation_fixture as F

pytestmark = pytest.mark.gpu

PLANES = F.planes()
CLOUDS = F.clouds()
DEV = 'cuda'
STATS = ('status', 'best_hypothesis', 'count', 'fitness', 'inlier_rmse')


def _gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(want))


def _plane_matches_host(out, c, want):
    """cloud c of a plane_segment_stack / segment_plane_clouds result against the host entry's dict, bit for bit"""
    planes, inliers, stats = out
    assert _same(planes[c].cpu().numpy(), want['plane'])
    assert np.array_equal(inliers[c].cpu().numpy(), np.flatnonzero(want['mask']))
    assert [int(stats[k][c]) for k in STATS[:3]] == [want[k] for k in STATS[:3]]
    assert _same(float(stats['fitness'][c]), want['fitness']) and _same(float(stats['inlier_rmse'][c]), want['inlier_rmse'])


@pytest.mark.parametrize('dtype', (np.float64, np.float32), ids=['float64', 'float32'])
@pytest.mark.parametrize('name', list(PLANES))
def test_plane_device_equals_the_host_entry(name, dtype):
    from se3et_amd import ops
    from se3et_amd.segmentation import segment_plane_clouds
    p, thr, rn, H, seed, _ = PLANES[name]
    p = p.astype(dtype)
    want = F.host_plane(p, thr, rn, H, seed)
    t = _gpu(p)
    out = segment_plane_clouds([t], thr, rn, H, seed=seed, return_stats=True)
    assert out[0].dtype == torch.float64 and tuple(out[0].shape) == (1, 4) and out[1][0].dtype == torch.int64 and out[1][0].is_cuda
    _plane_matches_host(out, 0, want)
    raw = ops.plane_segment_stack(t, [len(p)], thr, rn, H, seed, per_hypothesis=True)
    assert np.array_equal(raw['hyp_counts'][0].cpu().numpy(), want['hyp_counts']) and _same(raw['hyp_errs'][0].cpu().numpy(), want['hyp_errs'])
    assert np.array_equal(raw['mask'].cpu().numpy().astype(bool), want['mask'])


def test_plane_threshold_edge_on_the_device():
    from se3et_amd import ops
    seed = F._seed_for(len(F.EDGE), 3, {0, 1, 2})
    raw = ops.plane_segment_stack(_gpu(F.EDGE), [5], 0.5, 3, 1, seed, per_hypothesis=True)
    assert raw['hyp_counts'].cpu().tolist() == [[4]] and raw['hyp_errs'].cpu().tolist() == [[0.0625]]


@pytest.mark.parametrize('dtype', (np.float64, np.float32), ids=['float64', 'float32'])
@pytest.mark.parametrize('name', list(CLOUDS))
def test_dbscan_device_equals_the_host_entry(name, dtype):
    from se3et_amd.segmentation import cluster_dbscan_clouds
    p, eps, min_points = CLOUDS[name]
    p = p.astype(dtype)
    want, want_num = F.host_dbscan(p, eps, min_points)
    labels, num = cluster_dbscan_clouds([_gpu(p)], eps, min_points)
    assert labels[0].dtype == torch.int32 and labels[0].is_cuda and num.dtype == torch.int64 and tuple(num.shape) == (1,)
    assert np.array_equal(labels[0].cpu().numpy(), want) and int(num[0]) == want_num


def _batch():
    """33 clouds of different lengths, an empty one among them, float32 and float64 mixed; cloud 0 is cloud 31 again"""
    clouds = [F.slab(90 + 41 * i, 100 + i) for i in range(33)]
    clouds[5] = np.zeros((0, 3))
    clouds[7] = clouds[7][:2]
    clouds[12] = F.slab(2 * F.SEGMENT + 1, 99)
    clouds[31] = clouds[0]
    return [p.astype(np.float32 if i % 2 and i != 31 else np.float64) for i, p in enumerate(clouds)]


def test_plane_batch_of_33_equals_the_single_calls():
    from se3et_amd.segmentation import segment_plane_clouds
    clouds = _batch()
    pts = [_gpu(p) for p in clouds]
    args = (0.03, 4, F.TILE + 1)
    first, second = segment_plane_clouds(pts, *args, seed=9, return_stats=True), segment_plane_clouds(pts, *args, seed=9, return_stats=True)
    assert tuple(first[0].shape) == (33, 4) and len(first[1]) == 33
    assert _same(first[0].cpu().numpy(), second[0].cpu().numpy()) and all(torch.equal(a, b) for a, b in zip(first[1], second[1]))
    assert all(_same(first[2][k].cpu().numpy(), second[2][k].cpu().numpy()) for k in STATS)
    for i in (0, 5, 7, 12, 31, 32):
        alone = segment_plane_clouds([pts[i]], *args, seed=9, return_stats=True)
        assert _same(first[0][i].cpu().numpy(), alone[0][0].cpu().numpy()) and torch.equal(first[1][i], alone[1][0]), i
        assert all(_same(first[2][k][i].cpu().numpy(), alone[2][k][0].cpu().numpy()) for k in STATS), i
        _plane_matches_host(first, i, F.host_plane(clouds[i], *args, seed=9))
    assert _same(first[0][0].cpu().numpy(), first[0][31].cpu().numpy()) and torch.equal(first[1][0], first[1][31])
    assert first[2]['status'].cpu().tolist()[5] == 2 and first[2]['status'].cpu().tolist()[7] == 2
    planes, inliers = segment_plane_clouds([], 0.03)
    assert tuple(planes.shape) == (0, 4) and inliers == []


def test_dbscan_batch_of_33_equals_the_single_calls():
    from se3et_amd.segmentation import cluster_dbscan_clouds
    clouds = _batch()
    clouds[12] = CLOUDS['chain_shuffled'][0]
    pts = [_gpu(p) for p in clouds]
    first, second = cluster_dbscan_clouds(pts, 0.05, 2), cluster_dbscan_clouds(pts, 0.05, 2)
    assert len(first[0]) == 33 and tuple(first[1].shape) == (33,)
    assert all(torch.equal(a, b) for a, b in zip(first[0], second[0])) and torch.equal(first[1], second[1])
    for i in (0, 5, 7, 12, 31, 32):
        alone = cluster_dbscan_clouds([pts[i]], 0.05, 2)
        assert torch.equal(first[0][i], alone[0][0]) and int(first[1][i]) == int(alone[1][0]), i
        want, want_num = F.host_dbscan(clouds[i], 0.05, 2)
        assert np.array_equal(first[0][i].cpu().numpy(), want) and int(first[1][i]) == want_num, i
    assert torch.equal(first[0][0], first[0][31]) and int(first[1][12]) == 1
    labels, num = cluster_dbscan_clouds([], 0.05, 2)
    assert labels == [] and tuple(num.shape) == (0,)


def _corner(rng):
    floor = np.stack([rng.uniform(0, 1, 350), rng.uniform(0, 1, 350), rng.normal(0, 0.002, 350)], 1)
    wall = np.stack([rng.normal(0, 0.002, 250), rng.uniform(0, 1, 250), rng.uniform(0.05, 1, 250)], 1)
    return rng.permutation(np.concatenate([floor, wall]))


def test_segment_planes_peels_a_two_plane_corner():
    from se3et_amd.segmentation import segment_planes_clouds
    p = _corner(np.random.default_rng(21))
    labels, planes, counts = segment_planes_clouds([_gpu(p), _gpu(p[:2])], 0.01, 3, num_iterations=200)
    assert tuple(planes.shape) == (2, 3, 4) and tuple(counts.shape) == (2, 3) and labels[0].dtype == torch.int32
    lab, cnt, pl = labels[0].cpu().numpy(), counts[0].cpu().tolist(), planes[0].cpu().numpy()
    assert cnt[0] >= cnt[1] > 200 and cnt[2] == 0 and cnt[0] + cnt[1] == 600 and not pl[2].any()
    assert set(lab.tolist()) == {0, 1} and [(lab == k).sum() for k in (0, 1)] == cnt[:2]
    assert np.abs(pl[0] - [0, 0, 1, 0]).max() < 0.01 and np.abs(pl[1] - [1, 0, 0, 0]).max() < 0.01
    for k in (0, 1):
        assert (np.abs(p[lab == k] @ pl[k][:3] + pl[k][3]) < 0.01).all()
    assert labels[1].cpu().tolist() == [-1, -1] and counts[1].cpu().tolist() == [0, 0, 0]


def _equal(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    return a == b


def _scene(rng):
    """a floor under a bumpy surface, and its moved copy"""
    floor = np.stack([rng.uniform(0, 2, 2500), rng.uniform(0, 2, 2500), rng.normal(0, 0.003, 2500)], 1)
    xy = rng.uniform(0.2, 1.8, (2500, 2))
    bumps = np.concatenate([xy, 0.6 + 0.25 * np.sin(5 * xy[:, :1]) * np.cos(4 * xy[:, 1:]) + 0.1 * xy[:, :1] ** 2], 1)
    ref = np.concatenate([floor, bumps])
    a = 0.3
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    return _gpu(((ref[rng.permutation(len(ref))[:4500]] - [0.1, 0.2, 0.05]) @ R).astype(np.float32)), _gpu(ref.astype(np.float32))


def test_global_registration_with_the_segmentation_arguments():
    from se3et_amd.fpfh import global_registration_pairs
    src, ref = _scene(np.random.default_rng(22))
    kw = dict(voxel_size=0.08, num_iterations=1000, seed=0)
    default = global_registration_pairs([src], [ref], **kw)
    explicit = global_registration_pairs([src], [ref], remove_planes=0, plane_options=None, keep_clusters=None, dbscan_options=None, **kw)
    assert set(default) == {'transforms', 'coarse_transforms', 'ransac_transforms', 'src_points', 'ref_points', 'src_normals', 'ref_normals',
                            'src_feats', 'ref_feats', 'ransac', 'fgr', 'icp'}
    assert _equal(default, explicit)
    out = global_registration_pairs([src], [ref], remove_planes=1, plane_options=dict(distance_threshold=0.03, num_iterations=200),
                                    keep_clusters=20, **kw)
    assert set(out) == set(default) | {side + key for side in ('src_', 'ref_') for key in ('segment_rows', 'plane_labels', 'planes', 'cluster_labels')}
    for side in ('src_', 'ref_'):
        down, rows, lab = default[side + 'points'][0], out[side + 'segment_rows'][0], out[side + 'plane_labels'][0]
        assert lab.shape[0] == down.shape[0] and int((lab == 0).sum()) > 100 and tuple(out[side + 'planes'].shape) == (1, 1, 4)
        assert torch.equal(out[side + 'points'][0], down[rows]) and bool((lab[rows] == -1).all()) and 50 < rows.shape[0] < down.shape[0]
        plane = out[side + 'planes'][0, 0]
        assert bool(((out[side + 'points'][0].to(torch.float64) @ plane[:3] + plane[3]).abs() >= 0.03).all())
        assert out[side + 'normals'][0].shape[0] == rows.shape[0] and out[side + 'feats'][0].shape[0] == rows.shape[0]
        assert out[side + 'cluster_labels'][0].shape[0] == int((lab == -1).sum())
    assert bool(torch.isfinite(out['transforms']).all())


def test_numpy_drop_ins_and_refusals():
    from se3et_amd.segmentation import cluster_dbscan, cluster_dbscan_clouds, segment_plane, segment_plane_clouds
    p, thr, rn, H, seed, _ = PLANES['slab']
    want = F.host_plane(p, thr, rn, H, seed)
    plane, inliers = segment_plane(p, thr, rn, H, seed=seed)
    assert plane.shape == (4,) and plane.dtype == np.float64 and inliers.dtype == np.int64 and inliers.ndim == 1
    assert _same(plane, want['plane']) and np.array_equal(inliers, np.flatnonzero(want['mask']))
    q, eps, min_points = CLOUDS['blobs']
    labels = cluster_dbscan(q, eps, min_points)
    assert labels.shape == (len(q),) and labels.dtype == np.int32 and np.array_equal(labels, F.host_dbscan(q, eps, min_points)[0])
    bad = p.copy()
    bad[9, 2] = np.nan
    with pytest.raises(ValueError, match='segment_plane_clouds: cloud 1: a point is not finite'):
        segment_plane_clouds([_gpu(p), _gpu(bad)], thr)
    with pytest.raises(ValueError, match='cluster_dbscan_clouds: cloud 33: a point is not finite'):
        cluster_dbscan_clouds([_gpu(p[:5])] * 33 + [_gpu(bad)], 0.1, 3)
