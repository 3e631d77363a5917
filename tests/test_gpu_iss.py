"""ISS keypoints on the device (se3et_amd/iss.py, csrc/iss.hip) against the library's host entry -- the same text on host memory, which
tests/test_iss_cpu.py pins to the numpy twin -- bit for bit: saliencies, keypoint lists and the model resolution, for float32 and float64
inputs.  The clouds of tests/iss_fixture.py have R - 1, R and R + 1 rows for both kernels' rows per workgroup (4 and 256), rows with 1 to
301 members (the tile of 64 of the saliency kernel), and the exact edges of the memberships."""
import numpy as np
import pytest
import torch

import fpfh_fixture as FP
import iss_fixture as F

pytestmark = pytest.mark.gpu

CLOUDS = F.edge_clouds()
DTYPES = (np.float64, np.float32)
DEV = 'cuda'


def _gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _assert_equals_host(points, rs, rn, **kwargs):
    from se3et_amd.iss import iss_keypoints_clouds, model_resolution_clouds
    want = F.host_iss(points, rs, rn, **kwargs)
    keys, sal = iss_keypoints_clouds([_gpu(points)], rs, rn, return_saliency=True, **kwargs)
    assert len(keys) == 1 and keys[0].dtype == torch.int64 and keys[0].is_cuda and sal[0].dtype == torch.float64
    assert np.array_equal(sal[0].cpu().numpy(), want['saliency'])
    assert np.array_equal(keys[0].cpu().numpy(), np.flatnonzero(want['keypoint']))
    res = model_resolution_clouds([_gpu(points)])
    assert tuple(res.shape) == (1,) and res.dtype == torch.float64 and res.is_cuda and float(res[0]) == F.host_resolution(points)


@pytest.mark.parametrize('dtype', DTYPES, ids=['float64', 'float32'])
@pytest.mark.parametrize('name', list(CLOUDS))
def test_device_equals_the_host_entry(name, dtype):
    p, rs, rn = CLOUDS[name]
    _assert_equals_host(p.astype(dtype), rs, rn)


def test_other_parameters():
    p, rs, rn = CLOUDS['patch']
    _assert_equals_host(p, rs, rn, gamma_21=0.8, gamma_32=0.5, min_neighbors=12)
    _assert_equals_host(p, rn, rs, min_neighbors=1)                          # a non_max radius above the salient one


def _batch():
    """33 small clouds (the chunk boundary at 32), float32 and float64 side by side: the edge clouds at radii (0.25, 0.2), with n = 0, 1, 2
    and R - 1, R, R + 1 rows among them."""
    names = [n for n, v in CLOUDS.items() if v[1:] == (0.25, 0.2)]
    g = np.random.default_rng(3)
    clouds = [CLOUDS[n][0] for n in names]
    while len(clouds) < 33:
        clouds.append(g.uniform(0, 0.6, (20 + 7 * len(clouds), 3)))
    assert len(clouds) == 33 and {'clusters', 'planar', 'n0', 'n1', 'n2', 'n3', 'n4', 'n5'} <= set(names)
    return [p.astype(np.float32 if i % 2 else np.float64) for i, p in enumerate(clouds)]


@pytest.mark.parametrize('radii', [(0.25, 0.2), (0.0, 0.0), (0.0, 0.2)], ids=['given', 'default', 'mixed'])
def test_batch_of_33_equals_the_single_calls(radii):
    from se3et_amd.iss import iss_keypoints_clouds
    clouds = _batch()
    pts = [_gpu(p) for p in clouds]
    first, second = iss_keypoints_clouds(pts, *radii, return_saliency=True), iss_keypoints_clouds(pts, *radii, return_saliency=True)
    assert len(first[0]) == len(first[1]) == 33
    for i, p in enumerate(clouds):
        alone = iss_keypoints_clouds([pts[i]], *radii, return_saliency=True)
        for k in (0, 1):
            assert torch.equal(first[k][i], second[k][i]), i                                 # two runs are identical
            assert torch.equal(first[k][i], alone[k][0]), i                                  # alone
        if radii == (0.25, 0.2):
            want = F.host_iss(p, *radii)
            assert np.array_equal(first[1][i].cpu().numpy(), want['saliency']) and np.array_equal(first[0][i].cpu().numpy(),
                                                                                                   np.flatnonzero(want['keypoint'])), i
    assert iss_keypoints_clouds([]) == []


def test_default_radii_are_six_and_four_resolutions():
    from se3et_amd.iss import iss_keypoints_clouds, model_resolution_clouds
    names = ('patch', 'clusters', 'n257', 'copies', 'n1')
    pts = [_gpu(CLOUDS[n][0]) for n in names]
    res = model_resolution_clouds(pts).cpu().tolist()
    keys, sal = iss_keypoints_clouds(pts, return_saliency=True)
    assert sum(len(k) for k in keys) > 0
    for i, n in enumerate(names):
        assert res[i] == F.host_resolution(CLOUDS[n][0]), n
        if res[i] == 0:
            assert len(keys[i]) == 0 and not sal[i].any()
            continue
        k1, s1 = iss_keypoints_clouds([pts[i]], 6.0 * res[i], 4.0 * res[i], return_saliency=True)
        assert torch.equal(keys[i], k1[0]) and torch.equal(sal[i], s1[0]), n
        want = F.host_iss(CLOUDS[n][0], 6.0 * res[i], 4.0 * res[i])
        assert np.array_equal(sal[i].cpu().numpy(), want['saliency']) and np.array_equal(keys[i].cpu().numpy(), np.flatnonzero(want['keypoint'])), n


def test_small_list_budget_changes_no_bit(monkeypatch):
    """A list budget far below the lists' size cuts the chunk into row slices; float32 beside float64."""
    from se3et_amd import iss
    pts = [_gpu(CLOUDS['patch'][0]), _gpu(CLOUDS['clusters'][0].astype(np.float32)), _gpu(CLOUDS['n257'][0])]
    whole = iss.iss_keypoints_clouds(pts, 0.1, 0.08, return_saliency=True)
    monkeypatch.setattr(iss, 'PAIR_BUDGET', 20000)
    cut = iss.iss_keypoints_clouds(pts, 0.1, 0.08, return_saliency=True)
    assert sum(len(s) for s in whole[1]) > 0
    for i in range(3):
        assert torch.equal(cut[0][i], whole[0][i]) and torch.equal(cut[1][i], whole[1][i]), i
    want = F.host_iss(CLOUDS['patch'][0], 0.1, 0.08)
    assert np.array_equal(cut[1][0].cpu().numpy(), want['saliency'])


def test_numpy_wrapper():
    from se3et_amd.iss import compute_iss_keypoints
    p, rs, rn = CLOUDS['patch']
    got = compute_iss_keypoints(p, rs, rn)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, p[F.host_iss(p, rs, rn)['keypoint']])


def test_refusals():
    from se3et_amd.iss import iss_keypoints_clouds
    good = _gpu(CLOUDS['n257'][0])
    for bad in (np.nan, np.inf):
        q = CLOUDS['n257'][0].copy()
        q[9, 2] = bad
        for radii in ((0.25, 0.15), (0.0, 0.0)):
            with pytest.raises(ValueError, match='cloud 1: a point'):
                iss_keypoints_clouds([good, _gpu(q), good], *radii)
    with pytest.raises(ValueError, match='cloud 33'):                                      # the index counts across chunks
        q = CLOUDS['n257'][0].copy()
        q[0, 0] = np.nan
        iss_keypoints_clouds([good[:5]] * 33 + [_gpu(q)], 0.25, 0.15)
    with pytest.raises(ValueError, match='salient_radius'):
        iss_keypoints_clouds([good], -0.1)
    with pytest.raises(ValueError, match='gamma_21'):
        iss_keypoints_clouds([good], gamma_21=0.0)
    with pytest.raises(ValueError, match='min_neighbors'):
        iss_keypoints_clouds([good], min_neighbors=0)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        iss_keypoints_clouds([torch.from_numpy(CLOUDS['n257'][0])], 0.25, 0.15)


def _errors(T, Rm, t):
    T = T.cpu().numpy().astype(np.float64)                                                 # ref ~ T src: the inverse of the motion
    rre = np.degrees(np.arccos(np.clip((np.trace(T[:3, :3] @ Rm) - 1.0) / 2.0, -1.0, 1.0)))
    return rre, np.linalg.norm(T[:3, 3] - (-Rm.T @ t))


ISS_OPTIONS = {'salient_radius': 0.25, 'non_max_radius': 0.15}


def test_global_registration_from_iss_keypoints():
    """global_registration_pairs on the FPFH test's pair (the surface cloud and its moved, permuted copy, voxel size 0.1, seed 0, ICP) with
    keypoints='iss': the coarse method sees the keypoint rows alone, and the result meets the tolerance of the plain call's test (RRE
    below 15 degrees, RTE below 0.3).  The plain call's dict has the keys it had, and the whole-cloud outputs of the call with a detector
    equal the plain call's bit for bit."""
    from se3et_amd.fpfh import global_registration_pairs
    p, _ = FP.cloud('surface')
    mp, _, _, Rm, t = FP.moved_surface()
    v = 0.1
    plain = global_registration_pairs([_gpu(mp)], [_gpu(p)], v, icp_distance=1.5 * v, seed=0)
    assert not {'src_keypoints', 'ref_keypoints', 'src_kept', 'ref_kept'} & set(plain)          # the plain call's dict is what it was
    rre, rte = _errors(plain['transforms'][0], Rm, t)
    assert rre < 15.0 and rte < 0.3
    out = global_registration_pairs([_gpu(mp)], [_gpu(p)], v, icp_distance=1.5 * v, seed=0, keypoints='iss', iss_options=ISS_OPTIONS)
    ks, kr = out['src_keypoints'][0], out['ref_keypoints'][0]
    print('keypoints: %d of %d src rows, %d of %d ref rows' % (len(ks), len(out['src_points'][0]), len(kr), len(out['ref_points'][0])))
    for key in ('src_points', 'ref_points', 'src_normals', 'ref_normals', 'src_feats', 'ref_feats'):          # the whole clouds, as before
        assert torch.equal(out[key][0], plain[key][0]), key
    assert 3 <= len(ks) < len(out['src_points'][0]) and 3 <= len(kr) < len(out['ref_points'][0])
    table = out['ransac']['correspondences'][0]
    assert 0 < len(table) <= len(ks) and int(table[:, 0].max()) < len(ks) and int(table[:, 1].max()) < len(kr)
    assert out['icp'] is not None and out['src_kept'] is None
    for key in ('coarse_transforms', 'transforms'):
        rre, rte = _errors(out[key][0], Rm, t)
        print('%s: RRE %.4f deg, RTE %.5f' % (key, rre, rte))
    assert rre < 15.0 and rte < 0.3


def test_global_registration_with_outlier_removal():
    """The same pair with 25 stray points added to each raw cloud: the statistical filter drops them before the voxel grid."""
    from se3et_amd.fpfh import global_registration_pairs
    p, _ = FP.cloud('surface')
    mp, _, _, Rm, t = FP.moved_surface()
    g = np.random.default_rng(9)
    stray = g.uniform(-1, 1, (25, 3)) * np.array([1.0, 1.0, 0.3]) + np.array([0, 0, 1.5])       # a slab well above the surface
    src, ref = np.concatenate([mp, stray @ Rm.T + t]), np.concatenate([p, stray])
    v = 0.1
    out = global_registration_pairs([_gpu(src)], [_gpu(ref)], v, icp_distance=1.5 * v, seed=0, keypoints='iss', iss_options=ISS_OPTIONS,
                                    outlier_removal=('statistical', 20, 2.0))
    for kept, n in ((out['src_kept'][0], len(mp)), (out['ref_kept'][0], len(p))):
        assert not bool((kept >= n).any()) and len(kept) > 0.95 * n                           # every stray point is gone
    rre, rte = _errors(out['transforms'][0], Rm, t)
    print('with outlier removal: RRE %.4f deg, RTE %.5f' % (rre, rte))
    assert rre < 15.0 and rte < 0.3
    radius = global_registration_pairs([_gpu(src)], [_gpu(ref)], v, seed=0, outlier_removal=('radius', 4, 0.15))
    assert not bool((radius['src_kept'][0] >= len(mp)).any()) and radius['src_keypoints'] is None


def test_ball_query_with_a_radius_per_cloud():
    """The ball query's entries with one radius per cloud (the default radii of a batch): every cloud's counts and lists equal those of
    the one-radius call on that cloud alone, a radius of 0 (no member) among them."""
    from se3et_amd import ops
    from se3et_amd.stacking import identities, lengths, stack
    clouds = [_gpu(p) for p in _batch()[:7]]
    radii = [0.1, 0.25, 0.0, 0.3, 0.2, 0.15, 0.05]
    p, pl = stack(clouds), lengths(clouds)
    grid = ops.pair_grid_build(p, pl, identities(len(pl)), max(radii))
    ro = ops.pair_ball_count_stack(grid, p, pl, radii)
    pairs = ops.pair_ball_fill_stack(grid, p, pl, radii, ro, int(ro[-1]))
    counts, at = (ro[1:] - ro[:-1]).cpu(), 0
    assert int(ro[-1]) > sum(pl)
    for c, (q, r) in enumerate(zip(clouds, radii)):
        g1 = ops.pair_grid_build(q, [pl[c]], identities(1), r)
        ro1 = ops.pair_ball_count_stack(g1, q, [pl[c]], r)
        want = ops.pair_ball_fill_stack(g1, q, [pl[c]], r, ro1, int(ro1[-1]))
        rows = slice(sum(pl[:c]), sum(pl[:c + 1]))
        assert torch.equal(counts[rows], (ro1[1:] - ro1[:-1]).cpu()), c
        assert torch.equal(pairs[at:at + len(want)], want), c
        at += len(want)
    assert at == len(pairs)
    with pytest.raises(RuntimeError, match='radius'):
        ops.pair_ball_count_stack(grid, p, pl, radii[:-1] + [-1.0])
    with pytest.raises(RuntimeError, match='one radius per pair'):
        ops.pair_ball_count_stack(grid, p, pl, radii[:-1])
