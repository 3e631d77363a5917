"""Robust loss kernels and generalized ICP on the device (csrc/icp.hip, se3et_amd/icp.py) against se3_debug_icp_weighted_host, the same
text on host memory, BIT FOR BIT, at the shapes of tests/test_gpu_icp.py: the source row counts straddle a wave (64 lanes, one wave per row
in the nearest-neighbour kernel) and the reduction's lane width (kIcpLanes = 256 in csrc/icp_core.h), against 300 reference rows."""
import numpy as np
import pytest
import torch

import icp_fixture as F
import icp_robust_fixture as R
from icp_twin import EMPTY, TOO_FEW

pytestmark = pytest.mark.gpu

ESTIMATORS = ('point_to_point', 'point_to_plane', 'generalized')
LANES = 256          # kIcpLanes
KEYS = ('transforms', 'fitness', 'inlier_rmse', 'iterations', 'converged', 'status')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(pairs, mode, loss, loss_k=None, max_iteration=30):
    """icp_pairs / generalized_icp_pairs over pairs = [(src, ref, normals, T0, r, src_normals)] (one r for the call) -> per pair dict of
    numpy results."""
    from se3et_amd.icp import generalized_icp_pairs, icp_pairs
    srcs, refs, T0 = [_dev(p[0]) for p in pairs], [_dev(p[1]) for p in pairs], np.stack([p[3] for p in pairs])
    nrm, snr = [_dev(p[2]) for p in pairs], [_dev(p[5]) for p in pairs]
    if mode == 'generalized':
        out = generalized_icp_pairs(srcs, refs, T0, pairs[0][4], snr, nrm, loss=loss, loss_k=loss_k, max_iteration=max_iteration,
                                    return_correspondences=True)
    else:
        out = icp_pairs(srcs, refs, T0, pairs[0][4], mode, nrm, max_iteration=max_iteration, return_correspondences=True, loss=loss, loss_k=loss_k)
    host = {k: out[k].cpu().numpy() for k in KEYS}
    return [dict({k: host[k][i] for k in KEYS}, correspondences=out['correspondences'][i].cpu().numpy()) for i in range(len(pairs))]


def _same(got, want):
    """every bit of two per-pair results (NaN transforms compare by their bits too)"""
    for k in KEYS + ('correspondences',):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def _named(h):
    return {'transforms': h['transform'], 'fitness': np.float64(h['fitness']), 'inlier_rmse': np.float64(h['rmse']),
            'iterations': np.int32(h['iterations']), 'converged': np.int32(h['converged']), 'status': np.int32(h['status']),
            'correspondences': h['correspondences']}


def _host(p, mode, loss, loss_k=None, max_iteration=30):
    return _named(R.host_weighted_icp(p[0], p[1], p[3], p[4], mode, p[2], p[5], loss, 1.0 if loss_k is None else loss_k,
                                      max_iteration=max_iteration))


def _sheet(seed, nsrc, dtype, nref=300, r=0.15):
    ref, nrm, src, gt, T0 = F._pair(seed, nref, nsrc, 0.0)
    return tuple(np.ascontiguousarray(a.astype(dtype)) for a in (src, ref, nrm)) + (T0, r, np.ascontiguousarray(
        R.source_normals(src, gt).astype(dtype)))


SIZES = (63, 64, 65, LANES - 1, LANES, LANES + 1)


def _width(mode, loss):
    """The fixture's width of a loss; for generalized ICP in units of its Mahalanobis residual, which for an offset along the normal is
    1 / sqrt(2 epsilon) times the Euclidean one (M^-1 has the eigenvalue 1 / (2 epsilon) there, epsilon = 1e-3)."""
    return R.LOSS_K[loss] / np.sqrt(2e-3) if mode == 'generalized' else R.LOSS_K[loss]


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('loss', ['huber', 'tukey'])
@pytest.mark.parametrize('mode', ESTIMATORS)
def test_device_equals_the_weighted_host_entry_bit_for_bit(mode, loss, dtype):
    pairs = [_sheet(1 + i, n, dtype) for i, n in enumerate(SIZES)]
    got = _run(pairs, mode, loss, _width(mode, loss))
    for n, p, g in zip(SIZES, pairs, got):
        want = _host(p, mode, loss, _width(mode, loss))
        assert want['iterations'] >= 3 and want['fitness'] == 1.0, n                      # (a run of real updates)
        _same(g, want)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('loss', [None, 'l2'])
def test_generalized_without_a_robust_loss_equals_the_host_entry_bit_for_bit(loss, dtype):
    pairs = [_sheet(1 + i, n, dtype) for i, n in enumerate(SIZES)]
    got = _run(pairs, 'generalized', loss)
    for n, p, g in zip(SIZES, pairs, got):
        want = _host(p, 'generalized', loss)
        assert want['converged'] == 1 and want['iterations'] >= 3 and want['fitness'] == 1.0, n
        _same(g, want)


def _six(dtype='float64'):
    """test_gpu_icp._six with source normals: pairs that stop at different evaluations of a call with max_iteration = 8: converged at
    k = 1 (an exact T0), still moving at 8, two correspondences (the identity update), an empty source, and two ordinary ones."""
    ref, nrm, _src, gt, _T0 = F._pair(7, 300, 100, 0.0)
    inv = np.linalg.inv(gt)
    cast = lambda *arrays: tuple(np.ascontiguousarray(a.astype(dtype)) for a in arrays)
    exact = cast(ref[:100] @ inv[:3, :3].T + inv[:3, 3], ref, nrm) + (gt, 0.15) + cast(nrm[:100] @ gt[:3, :3])
    slow = _sheet(3, 65, dtype)
    few = _sheet(4, 120, dtype)
    far = few[0].copy()
    far[2:] += (np.linalg.inv(few[3])[:3, :3] @ np.array([0.0, 0.0, 7.0])).astype(dtype)          # all rows but two end far above the sheet
    few = (far,) + few[1:]
    empty = _sheet(5, 80, dtype)
    empty = (empty[0][:0],) + empty[1:5] + (empty[5][:0],)
    return [exact, slow, few, empty, _sheet(1, 257, dtype), _sheet(2, 190, dtype, nref=260)]


def test_six_unequal_pairs_equal_themselves_alone_and_a_second_run():
    mode, loss, k = 'generalized', 'cauchy', R.LOSS_K['cauchy']
    pairs = _six()
    first = _run(pairs, mode, loss, k, max_iteration=8)
    second = _run(pairs, mode, loss, k, max_iteration=8)
    for p, a, b in zip(pairs, first, second):
        _same(a, b)
        _same(a, _run([p], mode, loss, k, max_iteration=8)[0])
        _same(a, _host(p, mode, loss, k, max_iteration=8))
    exact, slow, few, empty, one, two = first
    assert (exact['iterations'], exact['converged'], exact['status']) == (1, 1, 0)
    assert (slow['iterations'], slow['converged'], slow['status']) == (8, 0, 0)
    assert (few['iterations'], few['converged'], few['status'], few['fitness']) == (1, 1, TOO_FEW, 2 / 120)
    assert (empty['iterations'], empty['converged'], empty['status'], empty['fitness']) == (1, 1, EMPTY, 0.0)
    for o in (one, two):
        assert o['status'] == 0 and o['iterations'] > 1 and o['fitness'] == 1.0


def test_a_non_finite_source_normal_refuses_its_pair_alone():
    from se3et_amd import ops
    from se3et_amd.icp import generalized_icp_pairs
    pairs = [_sheet(1, 65, 'float64'), _sheet(2, 64, 'float64'), _sheet(3, 63, 'float64')]
    bad = pairs[1][5].copy()
    bad[5, 1] = np.nan
    snr = [_dev(pairs[0][5]), _dev(bad), _dev(pairs[2][5])]
    with pytest.raises(ValueError, match='generalized_icp_pairs: pair 1'):
        generalized_icp_pairs([_dev(p[0]) for p in pairs], [_dev(p[1]) for p in pairs], np.stack([p[3] for p in pairs]), 0.15, snr,
                              [_dev(p[2]) for p in pairs], loss='huber', loss_k=0.01)
    # the stacked call below the raising wrapper: the refused pair's status and NaN transform, the other two as if alone
    grid = ops.pair_grid_build(torch.cat([_dev(p[1]) for p in pairs]), [300] * 3, torch.eye(4, dtype=torch.float64).repeat(3, 1, 1), 0.15)
    out = ops.icp_weighted_stack(grid, torch.cat([_dev(p[0]) for p in pairs]), [65, 64, 63], _dev(np.stack([p[3] for p in pairs])), 0.15,
                                 'generalized', torch.cat([_dev(p[2]) for p in pairs]), torch.cat(snr), 'huber', 0.01, return_correspondences=True)
    assert out['status'].cpu().tolist() == [0, ops.ICP_STATUS['nonfinite'], 0]
    assert bool(torch.isnan(out['transforms'][1]).all()) and bool((out['correspondences'][65:129] == -1).all())
    for i, rows in ((0, slice(0, 65)), (2, slice(129, 192))):
        want = _host(pairs[i], 'generalized', 'huber', 0.01)
        got = dict({k: out[k][i].cpu().numpy() for k in KEYS}, correspondences=out['correspondences'][rows].cpu().numpy())
        _same(got, want)


@pytest.mark.parametrize('mode', ESTIMATORS[:2])
def test_no_loss_on_the_device_is_the_old_host_entry_bit_for_bit(mode):
    """icp_pairs(..., loss=None): the kernels of before the losses, after they were made one instantiation of four."""
    sizes = (65, LANES + 1)
    pairs = [_sheet(1 + i, n, 'float64') for i, n in enumerate(sizes)]
    got = _run(pairs, mode, None)
    for p, g in zip(pairs, got):
        want = _named(F.host_icp(p[0], p[1], p[3], p[4], mode, p[2]))
        assert want['converged'] == 1 and want['iterations'] >= 3
        _same(g, want)


def test_registration_generalized_icp_numpy_round_trip():
    from se3et_amd.icp import registration_generalized_icp
    src, ref, nrm, T0, r, snr = _sheet(2, 200, 'float64')
    got = registration_generalized_icp(src, ref, T0, r, snr, nrm, loss='huber', loss_k=0.01)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (4, 4)
    assert got.tobytes() == R.host_weighted_icp(src, ref, T0, r, 'generalized', nrm, snr, 'huber', 0.01)['transform'].tobytes()


def test_global_registration_refines_with_generalized_icp():
    """The pipeline hands generalized_icp_pairs the clouds, the normals of both and the RANSAC transforms it returns."""
    from se3et_amd.fpfh import global_registration_pairs
    from se3et_amd.icp import generalized_icp_pairs
    from se3et_amd.synthetic import make_pair
    pairs = [make_pair('micro', i) for i in range(2)]
    out = global_registration_pairs([_dev(p[1]) for p in pairs], [_dev(p[0]) for p in pairs], 0.05, num_iterations=4000, icp_distance=0.075,
                                    icp_estimation='generalized', icp_loss='huber', icp_loss_k=0.5, seed=0)
    direct = generalized_icp_pairs(out['src_points'], out['ref_points'], out['ransac_transforms'], 0.075, out['src_normals'], out['ref_normals'],
                                   loss='huber', loss_k=0.5)
    assert sorted(out['icp']) == sorted(direct) == sorted(KEYS)
    for k in KEYS:
        assert out['icp'][k].dtype == direct[k].dtype and torch.equal(out['icp'][k].view(torch.uint8), direct[k].view(torch.uint8)), k
    assert torch.equal(out['transforms'], out['icp']['transforms']) and tuple(out['transforms'].shape) == (2, 4, 4)
    assert bool((out['icp']['iterations'] >= 1).all())


def test_tukey_point_to_plane_ends_nearer_the_ground_truth_on_the_outlier_family():
    from se3et_amd.icp import icp_pairs
    ref, nrm, src, _snr, gt, T0, _rows = R.outlier_pair(1)
    args = ([_dev(src)], [_dev(ref)], T0[None], 0.15, 'point_to_plane', [_dev(nrm)])
    plain = R.errors(icp_pairs(*args)['transforms'][0].cpu().numpy(), gt)
    robust = R.errors(icp_pairs(*args, loss='tukey', loss_k=0.02)['transforms'][0].cpu().numpy(), gt)
    print('rotation %.2e -> %.2e rad, translation %.2e -> %.2e' % (plain[0], robust[0], plain[1], robust[1]))
    assert robust[0] < plain[0] and robust[1] < plain[1]
