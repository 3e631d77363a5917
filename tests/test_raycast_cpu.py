"""Ray casting without a GPU: se3_debug_tsdf_raycast_host and se3_debug_stsdf_raycast_host (the text of csrc/tsdf_raycast_core.h with
csrc/tsdf_core.h and csrc/tsdf_sparse_core.h on host memory) against the float64 twin (tests/raycast_twin.py), bit for bit on every map,
over the cases of tests/raycast_fixture.py; what each crafted case is there for, checked on the twin; the analytic sphere; the power of
the cases against three modelled kernel mistakes; the sparse volume against the dense one; the round trip and the tracker through the
host entries (the figures that tests/test_gpu_raycast.py and tests/test_gpu_tracking.py hold the device to); what the calls refuse.

The sphere bound is twice the twin's own worst hit-depth error against the exact ray-sphere intersection (raycast_fixture.SPHERE_TWIN_ERROR,
measured on the CPU on the committed twin: 2.3943 voxel lengths at a grazing ray, median 0.083, 123 pixels)."""
import numpy as np
import pytest

import raycast_fixture as R
import raycast_twin as twin

CASES = R.cases()


def test_limits_and_entries_are_the_headers():
    from se3et_amd import _lib, ops
    assert _lib.ENUMS['se3_raycast_limit'] == {'SE3_RAYCAST_VIEW_WORDS': 16, 'SE3_RAYCAST_TILE': 16, 'SE3_RAYCAST_MAX_STEPS': 1 << 20}
    assert ops.RAYCAST_LIMITS == {'view_words': 16, 'tile': 16, 'max_steps': 1 << 20} and tuple(ops.RAYCAST_MAPS) == twin.MAPS
    for name in ('se3_tsdf_raycast_stack', 'se3_stsdf_raycast_stack', 'se3_debug_tsdf_raycast_host', 'se3_debug_stsdf_raycast_host'):
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES, name


@pytest.mark.parametrize('name', list(CASES))
def test_the_host_entry_equals_the_twin(name):
    got, want = R.host_maps(name), R.twin_maps(name)
    for k in R.MAP_NAMES:
        assert R.same_maps(got, want, (k,)), k
    hit = want['mask']
    assert np.all(want['depth'][~hit] == 0) and np.all(np.isnan(want['points'][~hit])) and np.all(np.isnan(want['normals'][~hit]))
    assert np.all(want['depth'][hit] > 0) and np.all(np.isfinite(want['points'][hit])) and np.all(np.isfinite(want['normals'][hit]))
    if want['color'] is not None:
        assert np.all(want['color'][~hit] == 0)


def test_every_subset_of_the_maps_gives_the_same_values():
    for name in ('r11_color_outside_in', 'sparse_corner'):
        full = R.host_maps(name)
        for mask in range(1, 32):
            maps = tuple(k for i, k in enumerate(R.MAP_NAMES) if mask >> i & 1)
            got = R.host_cast(CASES[name], maps)
            assert all(got[k] is None for k in R.MAP_NAMES if k not in maps) and R.same_maps(got, full, maps), maps


# ---- what the crafted cases are there for -------------------------------------------------------------------------------------------------------
def _hits(name):
    return int(R.twin_maps(name)['mask'].sum())


def test_what_the_dense_cases_exercise():
    vl = 0.0625
    assert _hits('r5_1x1_axis') == 1 and _hits('r5_17x19') == 17 * 19          # R = 5: the inner box is two voxels wide and enough
    c = CASES['r5_1x1_axis']
    ray = twin.ray_of(c['views'][0], c['origin'], 0, 0)
    assert ray['dir'][0] == 0.0 and ray['dir'][1] == 0.0 and ray['m'] == 1.0
    assert _hits('r5_zero_dir_outside') == 0
    ray = twin.ray_of(CASES['r5_zero_dir_outside']['views'][0], c['origin'], 0, 0)
    assert ray['dir'][0] == 0.0 and ray['e'][0] == 1.25 * vl < 1.5 * vl        # outside the slab of an axis that the ray never crosses
    c = CASES['r9_voxel_boundary']
    ray = twin.ray_of(c['views'][0], c['origin'], 0, 0)
    assert _hits('r9_voxel_boundary') == 1 and twin.point(ray, 0.3)[0] / vl == 3.0 and twin.point(ray, 0.3)[1] / vl == 5.0
    # the exact zero is the crossing sample (f <= 0 after a positive one): 1.0f at z = 6.5, a step of three voxel lengths, 0.0f at z = 3.5,
    # where T is 0 as well: s* is that sample
    c, m = CASES['r9_exact_zero'], R.twin_maps('r9_exact_zero')
    ray = twin.ray_of(c['views'][0], c['origin'], 0, 0)
    found = R.model_of(c).sample(ray, twin.point(ray, 3.5 * vl))
    assert found[1] == 0.0 and not np.signbit(found[1]) and found[2] == 1.0
    assert m['mask'][0, 0, 0] and m['depth'][0, 0, 0] == np.float32(3.5 * vl) and m['points'][0, 0, 0, 2] == 3.5 * vl
    assert _hits('r9_exact_zero_17x19') == 17 * 19
    assert _hits('r9_unobserved_between') == 0 and _hits('r9_unobserved_between_17x19') == 0
    assert _hits('r9_depth_min_behind') == 0 and _hits('r9_depth_max_in_front') == 0 and _hits('r11_looking_away') == 0
    assert 0 < _hits('r11_color_outside_in') < 2 * 17 * 19 and R.twin_maps('r11_color_outside_in')['mask'][1].any()
    assert _hits('agreement_dense') > _hits('agreement_dense_w2') > _hits('agreement_dense_w3') > _hits('agreement_dense_w3.5') == 0
    assert _hits('r9_random_inside_w0.5') > 0 and _hits('torus_inside') > 200


def test_the_same_cases_hit_with_the_limits_moved():
    """depth_min behind the surface and depth_max in front of it are what empties the two cases: with the default limits both hit"""
    for name in ('r9_depth_min_behind', 'r9_depth_max_in_front'):
        c = dict(CASES[name], depth_min=0.01, depth_max=3.0)
        assert R.twin_cast(c)['mask'].all() and R.host_cast(c)['mask'].all()


def test_the_trilinear_bracket_fails_and_the_nearest_values_refine():
    c = CASES['r9_bracket_fails']
    model, ray = R.model_of(c), twin.ray_of(c['views'][0], c['origin'], 0, 0)
    s0, s1 = 2.0 * c['vl'], 3.5 * c['vl']                               # the samples at z = 5.75 and 4.25 voxel lengths
    assert model.sample(ray, twin.point(ray, s0))[1] > 0 and model.sample(ray, twin.point(ray, s1))[1] == np.float32(-0.1)
    assert model.plane(twin.point(ray, s1), 0) > 0                       # T is positive beside the one negative voxel: no bracket
    want = ((s1 * 0.5) - (s0 * float(np.float32(-0.1)))) / (0.5 - float(np.float32(-0.1)))
    m = R.twin_maps('r9_bracket_fails')
    assert m['mask'][0, 0, 0] and m['depth'][0, 0, 0] == np.float32(want)


def test_what_the_sparse_cases_exercise():
    m = R.twin_maps('sparse_corner')
    pts = m['points'][m['mask']]
    assert all((pts[:, a] > 0).any() and (pts[:, a] < 0).any() for a in range(3))      # hits on every side of the three block faces
    one = R.twin_maps('sparse_corner_1x1')
    vl = CASES['sparse_corner']['vl']
    # along the edge y = z = 0 that four blocks share, less than two voxel lengths from the corner (the nearest voxels sit half a voxel
    # length beside the ray, so their sign changes a sample later than T's: another failed bracket)
    assert one['mask'][0, 0, 0] and abs(one['points'][0, 0, 0, 0]) < 2 * vl and np.all(one['points'][0, 0, 0, 1:] == 0)
    diagonal = R.twin_maps('sparse_corner_diagonal_1x1')                 # the crossing at the shared corner of the eight blocks
    assert diagonal['mask'][0, 0, 0] and np.all(np.abs(diagonal['points'][0, 0, 0]) < 1e-6 * vl)
    near = np.abs(pts) < vl                                             # stencils that straddle a face, an edge (two faces), the corner
    assert all(near[:, a].any() for a in range(3)) and all((near[:, a] & near[:, b]).any() for a, b in ((0, 1), (0, 2), (1, 2))) and near.all(1).any()
    assert min(k[1] for k in CASES['sparse_corner']['blocks']) < 0                       # negative block coordinates
    assert 0 < _hits('sparse_absent_between') < int(m['mask'][0].sum())
    assert (m['mask'][0] & ~R.twin_maps('sparse_absent_between')['mask'][0]).any()          # rays that reach the surface out of the absent block
    assert _hits('sparse_absent_only') == 0 and _hits('sparse_looking_away') == 0
    assert min(min(k[1:]) for k in CASES['sparse_sphere_negative_coords']['blocks']) < 0 and _hits('sparse_sphere_negative_coords') > 100
    k = R.twin_maps('sparse_key_range')['mask'][0]
    assert k.any() and not k.all()                                      # half of the rays pass the last block unobserved and leave the key's range
    c = CASES['sparse_key_range']
    ray = twin.ray_of(c['views'][0], np.zeros(3), 0, 0)
    assert twin.point(ray, c['depth_max'])[0] / c['vl'] >= 16 * twin.BIAS


def test_sparse_equals_dense_bit_for_bit():
    assert R.same_maps(R.host_maps('agreement_sparse'), R.host_maps('agreement_dense')) and _hits('agreement_dense') > 200
    c = CASES['agreement_dense']
    far = R.twin_maps('agreement_dense')['points'][R.twin_maps('agreement_dense')['mask']]
    assert far.min() > 1.5 * c['vl'] and far.max() < (32 - 1.5) * c['vl']


# ---- the analytic anchor ---------------------------------------------------------------------------------------------------------------------------
def test_the_sphere_is_hit_where_it_is():
    c = CASES['sphere_outside']
    twin_error, n = R.sphere_depth_error(c, R.twin_maps('sphere_outside'))
    host_error, _ = R.sphere_depth_error(c, R.host_maps('sphere_outside'))
    print('sphere: twin %.4f, host entry %.4f voxel lengths over %d pixels' % (twin_error, host_error, n))
    assert n == 123 and abs(twin_error - R.SPHERE_TWIN_ERROR) < 1e-4
    assert host_error <= 2 * R.SPHERE_TWIN_ERROR
    m = R.twin_maps('sphere_outside')
    centre, radius = R.sphere_world()
    out = (m['points'][m['mask']] - centre) / radius
    assert np.all(np.sum(out * m['normals'][m['mask']], 1) > 0.9)       # unit normals, outwards: towards the positive side
    assert np.allclose(np.linalg.norm(m['normals'][m['mask']], axis=1), 1.0, atol=1e-12)


# ---- the power of the cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mistake', ['step', 'unobserved', 'corner'])
def test_a_modelled_kernel_mistake_changes_a_case(mistake):
    """'step': the step of s not divided by m; 'unobserved': a crossing taken across an unobserved sample; 'corner': the far corner of a
    stencil read from the near corner's block"""
    changed = [name for name in CASES if not R.same_maps(R.twin_cast(CASES[name], mistake), R.twin_maps(name))]
    print(mistake, changed)
    assert changed
    if mistake == 'unobserved':
        assert 'r9_unobserved_between' in changed
    if mistake == 'corner':
        assert all(CASES[name]['kind'] == 'sparse' for name in changed) and 'sparse_corner_diagonal_1x1' in changed
    if mistake == 'step':
        assert 'sphere_outside' in changed


# ---- the round trip and the tracker through the host entries -----------------------------------------------------------------------------------------
def test_round_trip_through_the_host_entries():
    depth, got, want = R.round_trip()
    assert R.same_maps(got, want)
    error, share = R.round_trip_error(depth, want)
    print('round trip: the twin is %.6f m off at worst and hits %.4f of the valid pixels' % (error, share))
    assert abs(error - R.ROUND_TRIP_TWIN_ERROR) < 1e-6 and share == R.ROUND_TRIP_TWIN_SHARE >= 0.8
    host_error, host_share = R.round_trip_error(depth, got)
    assert host_error <= 2 * R.ROUND_TRIP_TWIN_ERROR and host_share >= R.ROUND_TRIP_TWIN_SHARE


def test_tracking_through_the_host_entries():
    poses, ok = R.track_host()
    degrees, mm = R.pose_error(poses, R.orbit_frames()[3])
    print('tracking through the host entries: %.4f degrees, %.3f mm at worst' % (degrees, mm))
    assert all(ok) and abs(degrees - R.TRACKING_HOST_ERROR[0]) < 1e-3 and abs(mm - R.TRACKING_HOST_ERROR[1]) < 1e-2


# ---- what the entries refuse ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('change', [dict(H=0), dict(W=8193), dict(depth_min=0.0), dict(depth_min=-1.0), dict(depth_max=0.1), dict(depth_max=np.inf),
                                    dict(depth_max=0.1 + 0.0625 * (1 << 20) * 1.01), dict(threshold=np.nan), dict(vl=0.0)])
def test_the_host_entry_refuses(change):
    with pytest.raises(RuntimeError):
        R.host_cast(dict(CASES['r9_voxel_boundary'], **change))
    with pytest.raises(RuntimeError):
        R.host_cast(dict(CASES['sparse_corner_1x1'], **change))


def test_a_colour_map_needs_colour():
    with pytest.raises(RuntimeError):
        _color_of_plain()


def _color_of_plain():
    from se3et_amd import _lib
    c = CASES['r9_voxel_boundary']
    s, out = c['state'], np.zeros((1, 1, 1, 3), np.float32)
    o = np.zeros(3)
    _lib.check(_lib.lib().se3_debug_tsdf_raycast_host(R._ptr(s['tsdf']), R._ptr(s['weight']), None, 9, c['vl'], c['trunc'], R._ptr(o), R._ptr(c['views']), 1, 1, 1,
                                                      0.1, 3.0, 1.0, None, None, None, R._ptr(out), None), 'se3_debug_tsdf_raycast_host')
