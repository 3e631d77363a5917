"""ICP refinement on the device (csrc/icp.hip, se3et_amd/icp.py) against se3_debug_icp_host, the same text on host memory, BIT FOR BIT,
at the smallest shapes at which the kernels can go wrong: the source row counts straddle a wave (64 lanes, one wave per row in the
nearest-neighbour kernel, four rows per workgroup) and the reduction's lane width (kIcpLanes = 256 in csrc/icp_core.h: lane l sums rows
l, l + 256, ..), against 300 reference rows."""
import numpy as np
import pytest
import torch

import icp_fixture as F
from icp_twin import EMPTY, TOO_FEW

pytestmark = pytest.mark.gpu

MODES = ('point_to_point', 'point_to_plane')
LANES = 256          # kIcpLanes
KEYS = ('transforms', 'fitness', 'inlier_rmse', 'iterations', 'converged', 'status')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(pairs, mode, max_iteration=30, T0=None):
    """icp_pairs over pairs = [(src, ref, normals, T0, r)] (one r for the call) -> per pair dict of numpy results."""
    from se3et_amd.icp import icp_pairs
    out = icp_pairs([_dev(p[0]) for p in pairs], [_dev(p[1]) for p in pairs], np.stack([p[3] for p in pairs]) if T0 is None else T0,
                    pairs[0][4], mode, [_dev(p[2]) for p in pairs], max_iteration=max_iteration, return_correspondences=True)
    host = {k: out[k].cpu().numpy() for k in KEYS}
    return [dict({k: host[k][i] for k in KEYS}, correspondences=out['correspondences'][i].cpu().numpy()) for i in range(len(pairs))]


def _same(got, want):
    """every bit of two per-pair results (NaN transforms compare by their bits too)"""
    for k in KEYS + ('correspondences',):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def _host(p, mode, max_iteration=30):
    h = F.host_icp(p[0], p[1], p[3], p[4], mode, p[2], max_iteration=max_iteration)
    return {'transforms': h['transform'], 'fitness': np.float64(h['fitness']), 'inlier_rmse': np.float64(h['rmse']),
            'iterations': np.int32(h['iterations']), 'converged': np.int32(h['converged']), 'status': np.int32(h['status']),
            'correspondences': h['correspondences']}


def _sheet(seed, nsrc, dtype, nref=300, r=0.15):
    ref, nrm, src, _gt, T0 = F._pair(seed, nref, nsrc, 0.0)
    return tuple(np.ascontiguousarray(a.astype(dtype)) for a in (src, ref, nrm)) + (T0, r)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('mode', MODES)
def test_device_equals_the_host_entry_bit_for_bit(mode, dtype):
    sizes = (63, 64, 65, LANES - 1, LANES, LANES + 1)
    pairs = [_sheet(1 + i, n, dtype) for i, n in enumerate(sizes)]
    got = _run(pairs, mode)
    for n, p, g in zip(sizes, pairs, got):
        want = _host(p, mode)
        assert want['converged'] == 1 and want['iterations'] >= 3 and want['fitness'] == 1.0, n       # (a run of real updates)
        _same(g, want)


def _six(dtype='float64'):
    """Pairs that stop at different evaluations of a call with max_iteration = 8: converged at k = 1 (an exact T0), still moving at 8,
    two correspondences (the identity update), an empty source, and two ordinary ones."""
    ref, nrm, _src, gt, _T0 = F._pair(7, 300, 100, 0.0)
    inv = np.linalg.inv(gt)
    exact = tuple(np.ascontiguousarray(a.astype(dtype)) for a in (ref[:100] @ inv[:3, :3].T + inv[:3, 3], ref, nrm)) + (gt, 0.15)
    slow = _sheet(3, 65, dtype)
    few = _sheet(4, 120, dtype)
    far = few[0].copy()
    T = few[3]
    far[2:] += (np.linalg.inv(T)[:3, :3] @ np.array([0.0, 0.0, 7.0])).astype(dtype)          # all rows but two end far above the sheet
    few = (far,) + few[1:]
    empty = _sheet(5, 80, dtype)
    empty = (empty[0][:0],) + empty[1:]
    return [exact, slow, few, empty, _sheet(1, 257, dtype), _sheet(2, 190, dtype, nref=260)]


@pytest.mark.parametrize('mode', MODES)
def test_six_unequal_pairs_equal_themselves_alone_and_a_second_run(mode):
    pairs = _six()
    first = _run(pairs, mode, max_iteration=8)
    second = _run(pairs, mode, max_iteration=8)
    for p, a, b in zip(pairs, first, second):
        _same(a, b)
        _same(a, _run([p], mode, max_iteration=8)[0])
        _same(a, _host(p, mode, max_iteration=8))
    exact, slow, few, empty, one, two = first
    assert (exact['iterations'], exact['converged'], exact['status']) == (1, 1, 0)
    if mode == 'point_to_point':
        assert (slow['iterations'], slow['converged'], slow['status']) == (8, 0, 0)
    assert (few['iterations'], few['converged'], few['status'], few['fitness']) == (1, 1, TOO_FEW, 2 / 120)
    assert (empty['iterations'], empty['converged'], empty['status'], empty['fitness']) == (1, 1, EMPTY, 0.0)
    for o in (one, two):
        assert o['converged'] == 1 and o['status'] == 0 and 1 < o['iterations'] < 8


def test_a_refused_pair_leaves_the_others_of_its_call_alone():
    from se3et_amd import ops
    from se3et_amd.icp import icp_pairs
    pairs = [_sheet(1, 65, 'float64'), _sheet(2, 64, 'float64'), _sheet(3, 63, 'float64')]
    bad = pairs[1][0].copy()
    bad[5, 1] = np.nan
    with pytest.raises(ValueError, match='pair 1'):
        icp_pairs([_dev(p[0]) for p in pairs[:1]] + [_dev(bad)] + [_dev(pairs[2][0])], [_dev(p[1]) for p in pairs],
                  np.stack([p[3] for p in pairs]), 0.15)
    # the stacked call below the raising wrapper: the refused pair's status and NaN transform, the other two as if alone
    src = torch.cat([_dev(pairs[0][0]), _dev(bad), _dev(pairs[2][0])])
    ref = torch.cat([_dev(p[1]) for p in pairs])
    grid = ops.pair_grid_build(ref, [300] * 3, torch.eye(4, dtype=torch.float64).repeat(3, 1, 1), 0.15)
    out = ops.icp_stack(grid, src, [65, 64, 63], _dev(np.stack([p[3] for p in pairs])), 0.15, 'point_to_point', return_correspondences=True)
    assert out['status'].cpu().tolist() == [0, ops.ICP_STATUS['nonfinite'], 0]
    assert bool(torch.isnan(out['transforms'][1]).all()) and bool((out['correspondences'][65:129] == -1).all())
    for i in (0, 2):
        want = _host(pairs[i], 'point_to_point')
        assert out['transforms'][i].cpu().numpy().tobytes() == want['transforms'].tobytes()


def _rotation_error_deg(A, B):
    R = A[:3, :3].T @ B[:3, :3]
    return np.rad2deg(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))


def test_refine_pairs_on_synthetic_output_dicts():
    """Two pairs of se3et_amd.synthetic's smallest preset, independently sampled clouds of one box, with the known transform turned by
    2 degrees about the reference cloud's centre (a registration error pivots about the scene; about the world origin it would leave
    1 mm of translation error, below what 600 points with 5 mm of jitter can resolve).  Point-to-plane: the estimator for independent
    samples of a surface, and the path that estimates the normals on the device."""
    from se3et_amd.icp import icp_pairs, refine_pairs
    from se3et_amd.synthetic import make_pair
    outs, gts, inits = [], [], []
    for i in range(2):
        ref, src, T = make_pair('micro', i)
        T = T.astype(np.float64)
        c = ref.mean(0).astype(np.float64)
        P = F.rigid(np.random.default_rng(100 + i), 2.0, 0.0)
        P[:3, 3] = c - P[:3, :3] @ c
        outs.append({'ref_points_f': _dev(ref), 'src_points_f': _dev(src)})
        gts.append(T)
        inits.append(P @ T)
    init = _dev(np.stack(inits).astype(np.float32))
    refined = refine_pairs(outs, init, 0.1, estimation='point_to_plane')
    assert refined.dtype == torch.float32 and tuple(refined.shape) == (2, 4, 4) and refined.is_cuda
    direct = icp_pairs([o['src_points_f'] for o in outs], [o['ref_points_f'] for o in outs], init, 0.1, 'point_to_plane')
    assert torch.equal(refined, direct['transforms'].to(torch.float32))
    for T, T0, got in zip(gts, np.stack(inits).astype(np.float32).astype(np.float64), refined.cpu().numpy().astype(np.float64)):
        rre0, rte0 = _rotation_error_deg(T0, T), np.linalg.norm(T0[:3, 3] - T[:3, 3])
        rre1, rte1 = _rotation_error_deg(got, T), np.linalg.norm(got[:3, 3] - T[:3, 3])
        print('RRE %.3f -> %.3f deg, RTE %.4f -> %.4f m' % (rre0, rre1, rte0, rte1))
        assert rre1 <= rre0 and rte1 <= rte0


@pytest.mark.parametrize('mode', MODES)
def test_registration_icp_numpy_round_trip(mode):
    from se3et_amd.icp import registration_icp
    src, ref, nrm, T0, r = _sheet(2, 200, 'float64')
    got = registration_icp(src, ref, T0, r, mode, nrm)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (4, 4)
    assert got.tobytes() == F.host_icp(src, ref, T0, r, mode, nrm)['transform'].tobytes()
    if mode == 'point_to_point':                           # init = None is the identity
        moved = np.ascontiguousarray(src @ T0[:3, :3].T + T0[:3, 3])
        assert registration_icp(moved, ref, None, r).tobytes() == F.host_icp(moved, ref, np.eye(4), r, mode)['transform'].tobytes()


def test_a_float32_device_init_is_taken_on_the_device():
    from se3et_amd.icp import icp_pairs
    pairs = [_sheet(1, 65, 'float32'), _sheet(2, 64, 'float32')]
    T32 = np.stack([p[3] for p in pairs]).astype(np.float32)
    args = ([_dev(p[0]) for p in pairs], [_dev(p[1]) for p in pairs])
    on_device = icp_pairs(*args, _dev(T32), 0.15)                                    # a float32 tensor on the device
    from_host = icp_pairs(*args, T32.astype(np.float64), 0.15)                       # the same values as float64 host arrays
    listed = icp_pairs(*args, [_dev(T32[0]), T32[1]], 0.15)                          # a list mixing device tensors and arrays
    for k in KEYS:
        assert torch.equal(on_device[k], from_host[k]), k
    assert torch.equal(listed['transforms'], from_host['transforms'])
