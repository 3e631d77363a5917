"""Colour gradients, coloured ICP and the multi-scale schedule on the device (csrc/color_gradient.hip, csrc/icp.hip, se3et_amd/icp.py)
against se3_debug_color_gradient_host and se3_debug_icp_colored_host, the same text on host memory, BIT FOR BIT: the gradients at cloud
sizes round K = 30 and over more than one workgroup, the loop at source row counts that straddle a wave and the reduction's lane width
(kIcpLanes = 256) against 300 reference rows; then the properties of a batch and the schedule's chain."""
import numpy as np
import pytest
import torch

import colored_icp_fixture as X
import icp_fixture as F
from icp_robust_fixture import LOSS_K
from icp_twin import EMPTY, NONFINITE, SINGULAR, TOO_FEW

pytestmark = pytest.mark.gpu

LANES = 256          # kIcpLanes
SIZES = (63, 64, 65, LANES - 1, LANES, LANES + 1)
KEYS = ('transforms', 'fitness', 'inlier_rmse', 'iterations', 'converged', 'status')
GRADIENT_RADIUS = 0.15          # of the 300-row references: about the reach of a row's 30 nearest


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
    return a.dtype, a.shape, a.tobytes()


def _sheet(seed, nsrc, dtype, nref=300, r=0.15):
    """(src, ref, normals, T0, r, src colours, ref colours) of a textured sheet pair."""
    ref, nrm, src, gt, T0 = F._pair(seed, nref, nsrc, 0.0)
    on_sheet = src @ gt[:3, :3].T + gt[:3, 3]
    cast = lambda a: np.ascontiguousarray(a.astype(dtype))
    return (cast(src), cast(ref), cast(nrm), T0, r, cast(X.texture(on_sheet[:, 0], on_sheet[:, 1])), cast(X.texture(ref[:, 0], ref[:, 1])))


def _run(pairs, loss=None, loss_k=None, max_iteration=30, lam=0.968):
    """colored_icp_pairs over pairs of _sheet (one r for the call) -> per pair dict of numpy results."""
    from se3et_amd.icp import colored_icp_pairs
    out = colored_icp_pairs([_dev(p[0]) for p in pairs], [_dev(p[1]) for p in pairs], np.stack([p[3] for p in pairs]), pairs[0][4],
                            [_dev(p[5]) for p in pairs], [_dev(p[6]) for p in pairs], [_dev(p[2]) for p in pairs], lam, GRADIENT_RADIUS,
                            loss=loss, loss_k=loss_k, max_iteration=max_iteration, return_correspondences=True)
    host = {k: out[k].cpu().numpy() for k in KEYS}
    return [dict({k: host[k][i] for k in KEYS}, correspondences=out['correspondences'][i].cpu().numpy()) for i in range(len(pairs))]


def _host(p, loss=None, loss_k=None, max_iteration=30, lam=0.968):
    g, status = X.host_gradients(p[1], p[2], p[6], GRADIENT_RADIUS)
    assert status == 0
    h = X.host_colored_icp(p[0], p[1], p[3], p[4], p[2], p[5], p[6], g, lam, loss, 1.0 if loss_k is None else loss_k, max_iteration=max_iteration)
    return {'transforms': h['transform'], 'fitness': np.float64(h['fitness']), 'inlier_rmse': np.float64(h['rmse']),
            'iterations': np.int32(h['iterations']), 'converged': np.int32(h['converged']), 'status': np.int32(h['status']),
            'correspondences': h['correspondences']}


def _same(got, want):
    """every bit of two per-pair results (NaN transforms compare by their bits too)"""
    for k in KEYS + ('correspondences',):
        assert _bits(got[k]) == _bits(want[k]), k


def _gradients(clouds, radius):
    from se3et_amd.icp import color_gradient_clouds
    return color_gradient_clouds([_dev(c[0]) for c in clouds], [_dev(c[1]) for c in clouds], [_dev(c[2]) for c in clouds], radius)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_device_gradients_equal_the_host_entry_bit_for_bit(dtype):
    sized = [X.small_cloud(n, dtype) for n in X.CLOUD_SIZES]
    calls = [(sized, 2.0)] + [([X.small_cloud(kind, dtype)], X.small_cloud(kind, dtype)[3]) for kind in ('duplicates', 'sparse')]
    c = X.inputs('sheet2048', dtype)                                   # eight workgroups of the gradient kernel
    calls.append(([(c['ref'], c['normals'], c['ref_colors'])], c['gradient_radius']))
    for clouds, radius in calls:
        for cloud, got in zip(clouds, _gradients(clouds, radius)):
            want, status = X.host_gradients(cloud[0], cloud[1], cloud[2], radius)
            assert status == 0 and _bits(got) == _bits(want), (len(cloud[0]), radius)
    sparse = X.small_cloud('sparse', dtype)
    g = _gradients([sparse], sparse[3])[0].cpu().numpy()
    zero = (g == 0.0).all(1)
    assert zero.sum() >= 1 and (~zero).sum() >= 1


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('loss', [None, 'huber', 'tukey'])
def test_device_equals_the_coloured_host_entry_bit_for_bit(loss, dtype):
    k = None if loss is None else LOSS_K[loss]
    pairs = [_sheet(1 + i, n, dtype) for i, n in enumerate(SIZES)]
    got = _run(pairs, loss, k)
    for n, p, g in zip(SIZES, pairs, got):
        want = _host(p, loss, k)
        assert want['iterations'] >= 2 and want['fitness'] == 1.0 and want['status'] == 0, n          # (a run of real updates)
        _same(g, want)


def _six(dtype='float64'):
    """Pairs that stop at different evaluations of a call with max_iteration = 8: converged at k = 1 (an exact T0), still moving at 8, two
    correspondences (the identity update), an empty source, and two ordinary ones of other sizes."""
    ref, nrm, _src, gt, _T0 = F._pair(7, 300, 100, 0.0)
    inv = np.linalg.inv(gt)
    cast = lambda *arrays: tuple(np.ascontiguousarray(a.astype(dtype)) for a in arrays)
    rcol = X.texture(ref[:, 0], ref[:, 1])
    exact = cast(ref[:100] @ inv[:3, :3].T + inv[:3, 3], ref, nrm) + (gt, 0.15) + cast(rcol[:100], rcol)
    slow = _sheet(3, 65, dtype)
    few = _sheet(4, 120, dtype)
    far = few[0].copy()
    far[2:] += (np.linalg.inv(few[3])[:3, :3] @ np.array([0.0, 0.0, 7.0])).astype(dtype)          # all rows but two end far above the sheet
    few = (far,) + few[1:]
    empty = _sheet(5, 80, dtype)
    empty = (empty[0][:0],) + empty[1:5] + (empty[5][:0], empty[6])
    return [exact, slow, few, empty, _sheet(1, 257, dtype), _sheet(2, 190, dtype, nref=260)]


def test_six_unequal_pairs_equal_themselves_alone_and_a_second_run():
    pairs = _six()
    first = _run(pairs, 'huber', LOSS_K['huber'], max_iteration=8)
    second = _run(pairs, 'huber', LOSS_K['huber'], max_iteration=8)
    for p, a, b in zip(pairs, first, second):
        _same(a, b)
        _same(a, _run([p], 'huber', LOSS_K['huber'], max_iteration=8)[0])
        if len(p[0]):
            _same(a, _host(p, 'huber', LOSS_K['huber'], max_iteration=8))
    exact, slow, few, empty, one, two = first
    assert (exact['iterations'], exact['converged']) == (1, 1)
    assert slow['iterations'] >= 2
    assert few['status'] == TOO_FEW and few['fitness'] == 2 / 120
    assert empty['status'] == EMPTY and empty['fitness'] == 0.0 and len(empty['correspondences']) == 0
    assert one['status'] == 0 and two['status'] == 0


def test_six_unequal_clouds_have_the_gradients_they_have_alone_and_in_a_second_run():
    clouds = [X.small_cloud(n, 'float32') for n in X.CLOUD_SIZES]
    first, second = _gradients(clouds, 2.0), _gradients(clouds, 2.0)
    for cloud, a, b in zip(clouds, first, second):
        assert _bits(a) == _bits(b) and _bits(a) == _bits(_gradients([cloud], 2.0)[0])


def test_thirty_three_small_pairs_cross_the_chunk_boundary():
    pairs = [_sheet(20 + i, 40 + i % 3, 'float64', nref=60) for i in range(33)]
    got = _run(pairs, max_iteration=6)
    assert len(got) == 33
    for p, g in zip(pairs, got):
        _same(g, _host(p, max_iteration=6))
    for i in (0, 31, 32):
        _same(got[i], _run([pairs[i]], max_iteration=6)[0])
    clouds = [(p[1], p[2], p[6]) for p in pairs]
    for cloud, g in zip(clouds, _gradients(clouds, GRADIENT_RADIUS)):
        assert _bits(g) == _bits(X.host_gradients(cloud[0], cloud[1], cloud[2], GRADIENT_RADIUS)[0])


def _ops_run(pairs):
    """The coloured entry through ops alone (icp.colored_icp_pairs raises on a refusal): the stacked results and the gradient words."""
    from se3et_amd import ops
    from se3et_amd.stacking import identities
    cat = lambda i: torch.cat([_dev(p[i]) for p in pairs])
    sl, ql, P = [len(p[0]) for p in pairs], [len(p[1]) for p in pairs], len(pairs)
    s, q, nr, sc, rc = cat(0), cat(1), cat(2), cat(5), cat(6)
    idx, d2 = ops.knn_stack(ops.pair_grid_build(q, ql, identities(P), 0.0), q, ql, 30)
    g, words = ops.color_gradient_stack(q, nr, rc, ql, idx, d2, GRADIENT_RADIUS)
    grid = ops.pair_grid_build(q, ql, identities(P), pairs[0][4])
    out = ops.icp_colored_stack(grid, s, sl, _dev(np.stack([p[3] for p in pairs])), pairs[0][4], nr, sc, rc, g, max_iteration=8,
                                return_correspondences=True)
    host = {k: out[k].cpu().numpy() for k in KEYS}
    corr = torch.split(out['correspondences'], sl)
    return [dict({k: host[k][i] for k in KEYS}, correspondences=corr[i].cpu().numpy()) for i in range(P)], words.cpu().tolist()


@pytest.mark.parametrize('which', [5, 6])
def test_a_non_finite_colour_refuses_its_pair_alone(which):
    pairs = [_sheet(1, 65, 'float32'), _sheet(2, 130, 'float32'), _sheet(3, 257, 'float32', nref=280)]
    clean, words = _ops_run(pairs)
    assert words == [0, 0, 0, 0] and all(c['status'] == 0 for c in clean)
    bad = list(pairs[1])
    bad[which] = bad[which].copy()
    bad[which][11, 2] = np.nan
    got, words = _ops_run([pairs[0], tuple(bad), pairs[2]])
    assert words == ([0, 1, 0, 1] if which == 6 else [0, 0, 0, 0])      # (the gradient call reads the reference colours alone)
    _same(got[0], clean[0])
    _same(got[2], clean[2])
    assert got[1]['status'] == NONFINITE and got[1]['iterations'] == 0 and got[1]['converged'] == 0
    assert np.isnan(got[1]['transforms']).all() and (got[1]['correspondences'] == -1).all()
    from se3et_amd.icp import color_gradient_clouds, colored_icp_pairs
    with pytest.raises(ValueError, match='colored_icp_pairs: pair 1: a point, normal, colour, gradient or initial transform is not finite'):
        _run([pairs[0], tuple(bad), pairs[2]])
    if which == 6:
        with pytest.raises(ValueError, match='color_gradient_clouds: cloud 1: a point, normal or colour is not finite'):
            _gradients([(p[1], p[2], p[6]) for p in (pairs[0], tuple(bad), pairs[2])], GRADIENT_RADIUS)


def _textured_pair(n=2000, seed=31):
    """(src, ref, src colours, ref colours, T0) on the device, float32: two independent samples of the textured sheet."""
    rng = np.random.default_rng(seed)
    ref, _ = F.sheet(rng, n)
    on_ref, _ = F.sheet(rng, n)
    gt = F.rigid(rng, 25.0, 0.5)
    inv = np.linalg.inv(gt)
    src = on_ref @ inv[:3, :3].T + inv[:3, 3]
    f32 = lambda a: _dev(a.astype(np.float32))
    return (f32(src), f32(ref), f32(X.texture(on_ref[:, 0], on_ref[:, 1])), f32(X.texture(ref[:, 0], ref[:, 1])),
            _dev(F.rigid(rng, 4.0, 0.03) @ gt)[None])


VOXELS, DISTANCES, ITERATIONS = [0.08, 0.04, None], [0.16, 0.08, 0.05], [20, 15, 10]


@pytest.mark.parametrize('estimation', ['colored', 'point_to_plane'])
def test_the_schedule_is_the_chain_of_its_calls_bit_for_bit(estimation):
    from se3et_amd import icp
    from se3et_amd.scan_prep import estimate_normals_clouds, voxel_downsample_clouds
    src, ref, scol, rcol, T0 = _textured_pair()
    colours = dict(src_colors_list=[scol], ref_colors_list=[rcol]) if estimation == 'colored' else {}
    out = icp.multiscale_icp_pairs([src], [ref], T0, VOXELS, DISTANCES, ITERATIONS, estimation, **colours)
    assert len(out['per_scale']) == 3 and _bits(out['transforms']) == _bits(out['per_scale'][-1]['transforms'])
    T, rows = T0, []
    for s, (v, r, it) in enumerate(zip(VOXELS, DISTANCES, ITERATIONS)):
        if v is None:
            p, q, pc, qc = [src], [ref], [scol], [rcol]
        else:
            (p, pc), (q, qc) = voxel_downsample_clouds([src], v, [scol]), voxel_downsample_clouds([ref], v, [rcol])
        rows.append(len(q[0]))
        nrm = estimate_normals_clouds(q, 30)
        if estimation == 'colored':
            want = icp.colored_icp_pairs(p, q, T, r, pc, qc, nrm, max_iteration=it)
        else:
            want = icp.icp_pairs(p, q, T, r, 'point_to_plane', nrm, max_iteration=it)
        for k in KEYS:
            assert _bits(out['per_scale'][s][k]) == _bits(want[k]), (s, k)
        assert int(want['status'][0]) == 0 and float(want['fitness'][0]) > 0.9
        T = want['transforms']
    assert rows[0] < rows[1] < rows[2] == 2000
    for k in KEYS:
        assert _bits(out[k]) == _bits(out['per_scale'][-1][k])


@pytest.mark.parametrize('estimation', ['colored', 'point_to_plane', 'generalized', 'point_to_point'])
def test_one_scale_of_none_is_the_plain_call(estimation):
    from se3et_amd import icp
    from se3et_amd.scan_prep import estimate_normals_clouds
    src, ref, scol, rcol, T0 = _textured_pair(600, 32)
    colours = dict(src_colors_list=[scol], ref_colors_list=[rcol]) if estimation == 'colored' else {}
    out = icp.multiscale_icp_pairs([src], [ref], T0, [None], [0.1], [12], estimation, **colours)
    if estimation == 'colored':
        want = icp.colored_icp_pairs([src], [ref], T0, 0.1, [scol], [rcol], normal_knn=30, max_iteration=12)
    elif estimation == 'generalized':
        want = icp.generalized_icp_pairs([src], [ref], T0, 0.1, normal_knn=30, max_iteration=12)
    else:
        nrm = estimate_normals_clouds([ref], 30) if estimation == 'point_to_plane' else None
        want = icp.icp_pairs([src], [ref], T0, 0.1, estimation, nrm, max_iteration=12)
    for k in KEYS:
        assert _bits(out[k]) == _bits(want[k]), k
    assert int(out['iterations'][0]) >= 2 and len(out['per_scale']) == 1


def test_colour_registers_the_flat_sheet_on_the_device():
    from se3et_amd import icp
    c = X.inputs('flat', 'float64')
    start = X.in_plane_error(c['T0'], c)
    args = ([_dev(c['src'])], [_dev(c['ref'])], c['T0'][None], c['r'])
    plane = icp.icp_pairs(*args, 'point_to_plane', [_dev(c['normals'])])
    assert int(plane['status'][0]) & SINGULAR or X.in_plane_error(plane['transforms'][0].cpu().numpy(), c) > 0.5 * start
    got = icp.colored_icp_pairs(*args, [_dev(c['src_colors'])], [_dev(c['ref_colors'])], [_dev(c['normals'])], gradient_radius=c['gradient_radius'])
    assert int(got['status'][0]) == 0 and int(got['converged'][0]) == 1
    assert X.in_plane_error(got['transforms'][0].cpu().numpy(), c) < 0.1 * start
    coarse = icp.multiscale_icp_pairs(args[0], args[1], args[2], [0.06, None], [0.2, 0.1], [30, 30], 'colored',
                                      src_colors_list=[_dev(c['src_colors'])], ref_colors_list=[_dev(c['ref_colors'])])
    assert X.in_plane_error(coarse['transforms'][0].cpu().numpy(), c) < 0.1 * start


def test_numpy_round_trips():
    from se3et_amd import icp
    src, ref, scol, rcol, T0 = _textured_pair(500, 33)
    host = lambda t: t.cpu().numpy()
    T = icp.registration_colored_icp(host(src), host(ref), host(scol), host(rcol), host(T0[0]), 0.1, max_iteration=10)
    want = icp.colored_icp_pairs([src], [ref], T0, 0.1, [scol], [rcol], max_iteration=10)
    assert T.dtype == np.float64 and T.shape == (4, 4) and _bits(T) == _bits(want['transforms'][0])
    T = icp.registration_multiscale_icp(host(src), host(ref), [0.08, None], [0.16, 0.08], [10, 10], host(T0[0]), 'colored', host(scol), host(rcol))
    want = icp.multiscale_icp_pairs([src], [ref], T0, [0.08, None], [0.16, 0.08], [10, 10], 'colored', [scol], [rcol])
    assert T.dtype == np.float64 and T.shape == (4, 4) and _bits(T) == _bits(want['transforms'][0])
    T = icp.registration_multiscale_icp(host(src), host(ref), [0.08, None], [0.16, 0.08], [10, 10], host(T0[0]))
    want = icp.multiscale_icp_pairs([src], [ref], T0, [0.08, None], [0.16, 0.08], [10, 10])
    assert _bits(T) == _bits(want['transforms'][0])
