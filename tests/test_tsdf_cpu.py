"""TSDF fusion without a GPU: se3_debug_tsdf_integrate_host, se3_debug_tsdf_extract_host and se3_debug_depth_points_host (the text of
csrc/tsdf_core.h on host memory) against the numpy twin (tests/tsdf_twin.py), bit for bit (values and sign bits), on every case of
tests/tsdf_fixture.py; the deliberate edge cases; the rendered sphere; frames split over two calls; the reference's depth-to-points
function through tests/golden/depth_points.npz; the limits and the refusals of se3et_amd/tsdf.py.

A zero gradient is held per component: a lone edge has a gradient of exactly 0 across its axis.  Along its axis the two stencils always
see the edge's own two values with opposite signs, so the whole gradient cannot vanish; the branch that returns an unnormalised normal
is reached through a NaN in an unobserved voxel of the stencil instead (crafted state 'nan_stencil').

The sphere bound is twice the twin's own worst radial error on that case (tsdf_fixture.SPHERE_TWIN_ERROR, measured on the CPU on the
committed twin: 0.5056 voxel lengths at resolution 16 with 32 x 24 images, 0.3753 at 32 with 64 x 48, three poses each)."""
import os

import numpy as np
import pytest

import tsdf_fixture as F
import tsdf_twin as twin

CASES = F.cases()
CRAFTED = F.crafted_states()
STATE_KEYS = ('tsdf', 'weight', 'color')


def _same_state(a, b):
    return all((a[k] is None and b[k] is None) or F.same(a[k], b[k]) for k in STATE_KEYS)


def _same_cloud(a, b):
    return all((x is None and y is None) or F.same(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3


def test_limits_are_the_headers():
    from se3et_amd import _lib, ops
    assert _lib.ENUMS['se3_tsdf_limit'] == {'SE3_TSDF_MIN_RESOLUTION': 4, 'SE3_TSDF_MAX_RESOLUTION': 1024, 'SE3_TSDF_MAX_IMAGE': 8192,
                                            'SE3_TSDF_MAX_TRUNC_VOXELS': 64, 'SE3_TSDF_FRAME_TILE': F.FRAME_TILE,
                                            'SE3_TSDF_FRAME_WORDS': twin.FRAME_WORDS}
    assert ops.TSDF_LIMITS == {k[len('SE3_TSDF_'):].lower(): v for k, v in _lib.ENUMS['se3_tsdf_limit'].items()}
    assert ops.DEPTH_CONVENTIONS == {'reference': 0, 'open3d': 1}
    for name in ('se3_tsdf_integrate_stack', 'se3_tsdf_extract_stack', 'se3_depth_points_stack', 'se3_debug_tsdf_integrate_host',
                 'se3_debug_tsdf_extract_host', 'se3_debug_depth_points_host'):
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES, name
    # the sizes the issue asks for are among the cases
    assert {c['R'] for c in CASES.values()} >= {13, 33}
    assert {c['depths'].shape[1:] for c in CASES.values()} >= {(24, 32), (17, 31)}
    assert {c['depths'].shape[0] for c in CASES.values()} >= {0, 1, 3, F.FRAME_TILE + 1}
    assert {c['depths'].dtype for c in CASES.values()} == {np.dtype(np.uint16), np.dtype(np.float32)}
    assert {None if c['colors'] is None else c['colors'].dtype for c in CASES.values()} == {None, np.dtype(np.uint8), np.dtype(np.float32)}


@pytest.mark.parametrize('name', list(CASES))
def test_host_entries_against_the_twin(name):
    c = CASES[name]
    want, got = F.twin_state(name), F.host_state(name)
    print('%s: %d voxels touched, weight up to %g' % (name, int((want['weight'] > 0).sum()), float(want['weight'].max())))
    assert _same_state(got, want)
    wp, gp = F.twin_cloud(name), F.host_cloud(name)
    print('   %d points' % len(wp[0]))
    assert _same_cloud(gp, wp)
    assert (wp[2] is not None) == (c['colors'] is not None)


@pytest.mark.parametrize('name', list(CRAFTED))
def test_extraction_of_crafted_states(name):
    state, vl, origin = CRAFTED[name]
    want, got = twin.extract(state, vl, origin), F.host_extract(state, vl, origin)
    print('%s: %d points' % (name, len(want[0])))
    assert _same_cloud(got, want)


def test_the_cases_are_not_empty():
    assert len(F.twin_cloud('r13_u16_f3')[0]) > 50 and len(F.twin_cloud('r33_f32_u8color_f3_origin')[0]) > 300
    assert len(F.twin_cloud('r13_u8color_f65')[0]) > 50 and F.twin_state('r13_u8color_f65')['weight'].max() > 40
    for name in ('r13_f0', 'r13_f0_color', 'r13_behind'):
        s = F.twin_state(name)
        assert not s['tsdf'].any() and not s['weight'].any() and len(F.twin_cloud(name)[0]) == 0
    c = F.twin_cloud('r33_f32_u8color_f3_origin')[2]
    assert c.min() >= 0 and c.max() <= 1 and c.std() > 0.05


def test_deliberate_integration_cases():
    # depth 0, NaN and >= depth_trunc are skipped: the mangled images touch fewer voxels than the clean ones, and only where a pixel is valid
    assert 0 < (F.twin_state('r13_mangled_f32')['weight'] > 0).sum() < (F.twin_state('r13_u16_f3')['weight'] > 0).sum()
    assert np.isnan(CASES['r13_mangled_f32']['depths']).any() and (CASES['r13_mangled_f32']['depths'] == 3000).any()
    assert np.isfinite(F.twin_state('r13_mangled_f32')['tsdf']).all()
    # the axis column: tsdf exactly 0 at z = 3, -0.5 at z = 4, sdf exactly -trunc at z = 5 (skipped), nothing at or behind the camera
    s = F.host_state('axis')
    assert s['weight'][6, 6].tolist() == [0, 0, 0, 1, 1] + [0] * 8
    assert s['tsdf'][6, 6, 3] == 0 and s['tsdf'][6, 6, 4] == np.float32(-0.5) and s['tsdf'][6, 6, 5] == 0
    assert len(F.host_cloud('axis')[0]) == len(F.twin_cloud('axis')[0])
    # a zero next to a negative value gives no point along z there
    pts = F.host_cloud('axis')[0]
    assert not np.any((np.abs(pts[:, 0] - 6.0) < 1e-9) & (np.abs(pts[:, 1] - 6.0) < 1e-9) & (pts[:, 2] > 3.0) & (pts[:, 2] < 4.0))
    # the first and the last admissible pixel, each frame on its own
    case, uf = F.edge_pixel_frames()
    weights = [F.host_integrate(case, frames=slice(k, k + 1))['weight'] for k in range(4)]
    twins = [twin.integrate(twin.new_state(13, False), 1.0, 2.0, case['origin'], case['depths'][k:k + 1], case['table'][k:k + 1])['weight']
             for k in range(4)]
    print('u_f of the four frames: %r' % [float(x) for x in uf])
    assert all(F.same(a, b) for a, b in zip(weights, twins))
    assert weights[0][0, :, 0].all() and not weights[1][0, :, 0].any()             # x = 0, z = 0: pixel 0 admitted, then refused
    assert weights[2][12, :, 0].all() and not weights[3][12, :, 0].any()           # x = 12, z = 0: pixel 31 admitted, then refused


def test_deliberate_extraction_cases():
    pts, nrm, _ = F.host_extract(*CRAFTED['lone_edges'])
    assert len(pts) == 3
    assert nrm[0, 0] < 0 and not nrm[0, 1:].any() and abs(nrm[0, 0]) == 1.0       # the gradient is exactly zero along y and z
    pts, _, _ = F.host_extract(*CRAFTED['at_098'])
    # +0.98f and one step below -0.98f are not usable; -0.98f and one step below +0.98f are
    assert len(pts) == 2 and sorted(np.round((pts[:, 1] - 2.0) / 0.05 - 0.5).astype(int).tolist()) == [6, 9]
    pts, _, _ = F.host_extract(*CRAFTED['zeros'])
    assert len(pts) == 2 and sorted(np.round(pts[:, 1] / 0.05 - 0.5).astype(int).tolist()) == [8, 9]
    pts, _, _ = F.host_extract(*CRAFTED['borders'])
    cells = pts / 0.05 - 0.5                                            # along z only: nothing towards x = R - 1, nothing from x = 0
    assert np.round(cells[:, :2]).astype(int).tolist() == [[1, 1], [10, 5], [11, 5]] and np.all(np.abs(cells[:, 2] - np.round(cells[:, 2])) > 0.1)
    pts, nrm, col = F.host_extract(*CRAFTED['nan_stencil'])
    assert len(pts) == 1 and np.isnan(nrm).any() and np.isfinite(pts).all()
    assert col[0].tolist() == [(0.25 * 0.25 + 1.0 * 0.5) / 0.75, (0.5 * 0.25 + 0.125 * 0.5) / 0.75, (1.0 * 0.25 + 0.0 * 0.5) / 0.75]


@pytest.mark.parametrize('name', list(F.SPHERES))
def test_rendered_sphere(name):
    c = CASES[name]
    twin_error = F.sphere_error(F.twin_cloud(name)[0], c['vl'])
    pts, nrm, _ = F.host_cloud(name)
    got = F.sphere_error(pts, c['vl'])
    print('%s: %d points, worst radial error %.4f voxel lengths (twin, now: %.4f; recorded: %.4f)' % (name, len(pts), got, twin_error,
                                                                                                       F.SPHERE_TWIN_ERROR[name]))
    assert abs(twin_error - F.SPHERE_TWIN_ERROR[name]) < 5e-4          # the recorded figure is the committed twin's
    assert len(pts) > 100 and got <= 2.0 * F.SPHERE_TWIN_ERROR[name]
    outward = np.einsum('ij,ij->i', nrm, (pts - F.SPHERE_CENTER) / F.SPHERE_RADIUS)
    print('   normals against the radial direction: median %.3f' % float(np.median(outward)))
    assert np.median(outward) > 0.9


@pytest.mark.parametrize('name,cut', [('r13_u16_f3', 1), ('r13_u8color_f65', 64), ('r13_f32_f65_31x17', 17), ('r13_f32color_f1', 0)])
def test_frames_split_over_two_calls(name, cut):
    c = CASES[name]
    s = F.host_integrate(c, frames=slice(0, cut))
    s = F.host_integrate(c, state=s, frames=slice(cut, None))
    assert _same_state(s, F.host_state(name))


def test_depth_points_reference_convention_against_the_golden_file():
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'depth_points.npz'))
    depth, K3 = g['depth'], g['intrinsics']
    K = np.array([K3[0, 0], K3[1, 1], K3[0, 2], K3[1, 2]])
    d, k = F.depth_image(np.uint16)
    assert np.array_equal(depth, d) and np.array_equal(K, k) and depth.shape == (24, 32) and K[0] != K[1]
    for tag in ('default', 'near'):
        (scale, limit), want = g[tag + '_params'], g[tag + '_points']
        got = F.host_depth_points(depth, K, scale, limit, 'reference')
        zero_rows, rows = int((~want.any(1)).sum()), want[:, 1] * K[1] / np.where(want[:, 2] > 0, want[:, 2], 1) + K[3]
        print('%s: %d points, %d zero rows, %d fractional rows' % (tag, len(want), zero_rows, int((np.abs(rows - np.round(rows)) > 1e-3).sum())))
        assert zero_rows > 0 and (np.abs(rows - np.round(rows)) > 1e-3).sum() > 100          # both quirks are in the file
        assert F.same(got, want)
        assert F.same(twin.depth_points(depth, K, scale, limit, 'reference'), want)


@pytest.mark.parametrize('dtype', (np.uint16, np.float32), ids=['uint16', 'float32'])
@pytest.mark.parametrize('convention', ('reference', 'open3d'))
def test_depth_points_against_the_twin(convention, dtype):
    depth, K = F.depth_image(dtype)
    for scale, limit in ((1000.0, 6.0), (500.0, 3.5)):
        want = twin.depth_points(depth, K, scale, limit, convention)
        assert F.same(F.host_depth_points(depth, K, scale, limit, convention), want)
        if convention == 'open3d':
            assert want[:, 2].min() > 0 and want[:, 2].max() <= limit and len(want) < len(twin.depth_points(depth, K, scale, limit))


def test_refusals_fire_before_any_launch():
    """Every refusal is a ValueError from the Python side's own checks: they are reached here without a GPU, on CPU tensors, where a
    call that passed them would end at the 'no CPU implementation' RuntimeError instead."""
    import torch
    from se3et_amd import ops
    from se3et_amd.tsdf import TSDFVolumes, depth_to_points_clouds, fuse_depth_frames
    lim = ops.TSDF_LIMITS
    for R in (lim['min_resolution'] - 1, lim['max_resolution'] + 1, 13.5):
        with pytest.raises(ValueError, match='resolution'):
            TSDFVolumes(1, R, 0.01, 0.04, device='cpu')
    for trunc in (0.0, -1.0, float('nan'), float('inf'), 0.01 * lim['max_trunc_voxels'] * 1.01):
        with pytest.raises(ValueError, match='sdf_trunc'):
            TSDFVolumes(1, 13, 0.01, trunc, device='cpu')
    with pytest.raises(ValueError, match='voxel_length'):
        TSDFVolumes(1, 13, 0.0, 0.04, device='cpu')
    with pytest.raises(ValueError, match='origins'):
        TSDFVolumes(2, 13, 0.01, 0.04, origins=np.zeros((1, 3)), device='cpu')
    vol, colvol = TSDFVolumes(1, 13, 0.01, 0.04, device='cpu'), TSDFVolumes(1, 13, 0.01, 0.04, color=True, device='cpu')
    two = TSDFVolumes(2, 13, 0.01, 0.04, device='cpu')
    depths, K, E = torch.zeros((3, 24, 32), dtype=torch.float32), [30.0, 30.0, 16.0, 12.0], torch.eye(4, dtype=torch.float64).repeat(3, 1, 1)
    with pytest.raises(ValueError, match='each side'):
        vol.integrate(torch.zeros((1, 1, lim['max_image'] + 1), dtype=torch.uint16), K, E[:1])
    with pytest.raises(ValueError, match='each side'):
        vol.integrate(torch.zeros((1, 0, 32), dtype=torch.float32), K, E[:1])
    bad = E.clone()
    bad[1, 0, 3] = float('nan')
    with pytest.raises(ValueError, match='not finite'):
        vol.integrate(depths, K, bad)
    bad[1, 0, 3] = 1e39                                                 # finite in float64, not in float32
    with pytest.raises(ValueError, match='not finite'):
        vol.integrate(depths, K, bad)
    with pytest.raises(ValueError, match='not finite'):
        vol.integrate(depths, [30.0, float('inf'), 16.0, 12.0], E)
    with pytest.raises(ValueError, match='one \\(4, 4\\) transform per pair'):
        vol.integrate(depths, K, E[:2])
    for counts in ([2], [4], [3, 0], [-1]):
        with pytest.raises(ValueError, match='frame_counts'):
            vol.integrate(depths, K, E, frame_counts=counts)
    with pytest.raises(ValueError, match='frame_counts'):
        two.integrate(depths, K, E)                                     # no default for two volumes
    with pytest.raises(ValueError, match='frame_counts'):
        two.integrate(depths, K, E, frame_counts=[1, 1])
    colors = torch.zeros((3, 24, 32, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match='colour'):
        vol.integrate(depths, K, E, colors=colors)
    with pytest.raises(ValueError, match='colour'):
        colvol.integrate(depths, K, E)
    with pytest.raises(ValueError, match='do not match'):
        colvol.integrate(depths, K, E, colors=colors[:, :, :31])
    with pytest.raises(ValueError, match='intrinsics'):
        vol.integrate(depths, [1.0, 2.0, 3.0], E)
    for key in ('depth_scale', 'depth_trunc'):
        with pytest.raises(ValueError, match=key):
            vol.integrate(depths, K, E, **{key: 0.0})
    with pytest.raises(ValueError, match='convention'):
        depth_to_points_clouds(depths, K, convention='opencv')
    with pytest.raises(ValueError, match='scaling_factor'):
        depth_to_points_clouds(depths, K, scaling_factor=0.0)
    with pytest.raises(ValueError, match='one entry per fragment'):
        fuse_depth_frames([depths], K, [E, E], 13, 0.01, 0.04, device='cpu')
    # what passes every check ends at the device check, not in a kernel: nothing has been written
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        vol.integrate(depths, K, E)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        depth_to_points_clouds(depths, K)
    assert not vol.tsdf.any() and not vol.weight.any()
    # the library refuses on its own as well, through the host entries
    c = dict(CASES['r13_u16_f3'])
    for key, value in (('R', 3), ('trunc', 0.0), ('trunc', 65 * c['vl']), ('vl', float('nan'))):
        with pytest.raises(RuntimeError, match='code'):
            F.host_integrate({**c, key: value})
