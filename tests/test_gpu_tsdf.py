"""TSDF fusion on the device (se3et_amd/tsdf.py, csrc/tsdf.hip) against the library's host entries -- the same text on host memory, which
tests/test_tsdf_cpu.py pins to the numpy twin -- bit for bit, on every case of tests/tsdf_fixture.py in both depth dtypes; a volume alone, at positions 0 and
31 of a batch of 32 and through the chunking at 33 volumes, with mixed frame counts and images; frames split over two calls; from run to
run; an untouched volume; fuse_depth_frames into voxel_downsample_clouds; depth images as clouds in both conventions."""
import numpy as np
import pytest
import torch

import tsdf_fixture as F

pytestmark = pytest.mark.gpu

CASES = F.cases()
CRAFTED = F.crafted_states()
DEV = 'cuda'
KEYS = ('tsdf', 'weight', 'color')


def _gpu(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _volumes(cases, color=None):
    from se3et_amd.tsdf import TSDFVolumes
    c = cases[0]
    assert all((x['R'], x['vl'], x['trunc']) == (c['R'], c['vl'], c['trunc']) for x in cases)
    color = (c['colors'] is not None) if color is None else color
    return TSDFVolumes(len(cases), c['R'], c['vl'], c['trunc'], origins=np.array([x['origin'] for x in cases]), color=color, device=DEV)


def _integrate(vol, cases, frames=slice(None)):
    """the cases' frames[frames], one case per volume, in one integrate call; extrinsics and intrinsics come back out of the float32 table"""
    tables = [x['table'][frames] for x in cases]
    E = np.zeros((sum(len(t) for t in tables), 4, 4))
    table = np.concatenate(tables)
    E[:, :3, :], E[:, 3, 3] = table[:, :12].reshape(-1, 3, 4), 1.0
    colors = None if vol.color is None else _gpu(np.concatenate([x['colors'][frames] for x in cases]))
    vol.integrate(_gpu(np.concatenate([x['depths'][frames] for x in cases])), table[:, 12:].astype(np.float64), E, [len(t) for t in tables], colors,
                  cases[0]['depth_scale'], cases[0]['depth_trunc'])
    return vol


def _state(vol, v):
    return {'tsdf': vol.tsdf[v].cpu().numpy(), 'weight': vol.weight[v].cpu().numpy(), 'color': None if vol.color is None else vol.color[v].cpu().numpy()}


def _same_state(a, b):
    return all((a[k] is None and b[k] is None) or F.same(a[k], b[k]) for k in KEYS)


def _cloud(clouds, v):
    return tuple(None if x[v] is None else x[v].cpu().numpy() for x in clouds)


def _same_cloud(a, b):
    return len(a) == len(b) == 3 and all((x is None and y is None) or F.same(x, y) for x, y in zip(a, b))


def _with_depth(case, dtype):
    """the case with its depth images as dtype: uint16 becomes float32 exactly; float32 is rounded, a NaN becoming 0"""
    d = case['depths']
    if d.dtype == dtype:
        return case
    with np.errstate(invalid='ignore'):
        d = d.astype(np.float32) if dtype == np.float32 else np.where(np.isnan(d), 0, np.round(d)).astype(np.uint16)
    return dict(case, depths=np.ascontiguousarray(d))


@pytest.mark.parametrize('dtype', (np.uint16, np.float32), ids=['uint16', 'float32'])
@pytest.mark.parametrize('name', list(CASES))
def test_device_equals_the_host_entries(name, dtype):
    c = _with_depth(CASES[name], dtype)
    own = c is CASES[name]                                              # the case's own dtype: the shared host results
    want = F.host_state(name) if own else F.host_integrate(c)
    vol = _integrate(_volumes([c]), [c])
    assert vol.tsdf.dtype == torch.float32 and vol.tsdf.is_cuda and tuple(vol.tsdf.shape) == (1,) + (c['R'],) * 3
    assert _same_state(_state(vol, 0), want)
    clouds = vol.extract_point_clouds()
    assert all(x.dtype == torch.float64 and x.is_cuda and x.shape[1] == 3 for x in clouds[0] + clouds[1])
    assert _same_cloud(_cloud(clouds, 0), F.host_cloud(name) if own else F.host_extract(want, c['vl'], c['origin']))


@pytest.mark.parametrize('name', list(CRAFTED))
def test_extraction_of_crafted_states_on_the_device(name):
    from se3et_amd.tsdf import TSDFVolumes
    state, vl, origin = CRAFTED[name]
    vol = TSDFVolumes(1, 13, vl, 2 * vl, origins=origin[None], color=state['color'] is not None, device=DEV)
    vol.tsdf.copy_(_gpu(state['tsdf'])[None]), vol.weight.copy_(_gpu(state['weight'])[None])
    if vol.color is not None:
        vol.color.copy_(_gpu(state['color'])[None])
    assert _same_cloud(_cloud(vol.extract_point_clouds(), 0), F.host_extract(state, vl, origin))


BATCH = ('r13_u16_f3', 'r13_f0', 'r13_u8color_f65', 'r13_mangled_u16', 'r13_behind')          # uint16 depth, 32 x 24, resolution 13, two truncations


def _batch_cases(n):
    """n volumes over the uint16 cases of one size: mixed frame counts (0, 1, 3 and 65 among them) and images; colour dropped, and the
    truncation of the first"""
    pool = [dict(CASES[k], colors=None, trunc=CASES[BATCH[0]]['trunc']) for k in BATCH]
    pool.append(dict(pool[2], depths=pool[2]['depths'][5:6], table=pool[2]['table'][5:6]))
    return [dict(pool[i % len(pool)], origin=np.array([0.001 * (i // len(pool)), 0.0, 0.0])) for i in range(n)]


@pytest.fixture(scope='module')
def alone():
    """each distinct volume of the batches on its own: its state and cloud"""
    out = {}
    for i, c in enumerate(_batch_cases(12)):
        vol = _integrate(_volumes([c]), [c])
        out[i] = (_state(vol, 0), _cloud(vol.extract_point_clouds(), 0))
    return out


@pytest.mark.parametrize('n', (32, 33))
def test_a_volume_is_the_same_alone_and_in_a_batch(alone, n):
    cases = _batch_cases(n)
    assert {len(c['table']) for c in cases} >= {0, 1, 3, 65}
    vol = _integrate(_volumes(cases), cases)
    clouds = vol.extract_point_clouds()
    assert len(clouds[0]) == n
    for v in sorted({0, 1, 5, 6, 11, 31, n - 1}):                       # positions 0 and 31, the volume after the chunk boundary, one without frames
        i = v % 6 + 6 * min(v // 6, 1)
        if v // 6 > 1:                                                  # a later origin: the same case alone, at that origin
            one = _integrate(_volumes([cases[v]]), [cases[v]])
            want = (_state(one, 0), _cloud(one.extract_point_clouds(), 0))
        else:
            want = alone[i]
        assert _same_state(_state(vol, v), want[0]), v
        assert _same_cloud(_cloud(clouds, v), want[1]), v
    assert not vol.weight[1].any() and clouds[0][1].shape == (0, 3)


@pytest.mark.parametrize('name,cut', [('r13_u8color_f65', 64), ('r13_f32_f65_31x17', 17), ('r33_f32_u8color_f3_origin', 1)])
def test_a_second_integrate_call_equals_one_call(name, cut):
    c = CASES[name]
    vol = _volumes([c])
    _integrate(vol, [c], slice(0, cut))
    _integrate(vol, [c], slice(cut, None))
    assert _same_state(_state(vol, 0), F.host_state(name))


def test_two_runs_are_bit_identical():
    cases = _batch_cases(7)
    runs = []
    for _ in range(2):
        vol = _integrate(_volumes(cases), cases)
        clouds = vol.extract_point_clouds()
        runs.append(([_state(vol, v) for v in range(7)], [_cloud(clouds, v) for v in range(7)]))
    assert all(_same_state(a, b) for a, b in zip(runs[0][0], runs[1][0])) and all(_same_cloud(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_an_untouched_volume_gives_empty_clouds():
    from se3et_amd.tsdf import TSDFVolumes
    for color in (False, True):
        pts, nrm, col = TSDFVolumes(2, 13, 0.01, 0.04, color=color, device=DEV).extract_point_clouds()
        assert len(pts) == len(nrm) == len(col) == 2
        for v in range(2):
            assert tuple(pts[v].shape) == tuple(nrm[v].shape) == (0, 3) and pts[v].dtype == torch.float64 and pts[v].is_cuda
            assert (col[v] is None) if not color else (tuple(col[v].shape) == (0, 3) and col[v].is_cuda)
    assert TSDFVolumes(0, 13, 0.01, 0.04, device=DEV).extract_point_clouds() == ([], [], [])


def test_fuse_depth_frames_feeds_the_scan_preparation():
    from se3et_amd.scan_prep import voxel_downsample_clouds
    from se3et_amd.tsdf import fuse_depth_frames
    names = ('r13_mangled_u16', 'r13_u8color_f65')
    cs = [dict(CASES[k], trunc=CASES[names[0]]['trunc']) for k in names]
    E = []
    for c in cs:
        e = np.zeros((len(c['table']), 4, 4))
        e[:, :3, :], e[:, 3, 3] = c['table'][:, :12].reshape(-1, 3, 4), 1.0
        E.append(e)
    K = [c['table'][:, 12:].astype(np.float64) for c in cs]
    pts, nrm, col = fuse_depth_frames([_gpu(c['depths']) for c in cs], K, E, 13, cs[0]['vl'], cs[0]['trunc'],
                                      colors_list=[_gpu(c['colors']) for c in cs])
    assert len(pts) == len(nrm) == len(col) == 2
    for v, c in enumerate(cs):
        want = F.host_extract(F.host_integrate(c), c['vl'], c['origin'])
        assert all(x[v].dtype == torch.float64 and x[v].is_cuda and tuple(x[v].shape) == (len(want[0]), 3) for x in (pts, nrm, col))
        assert _same_cloud((pts[v].cpu().numpy(), nrm[v].cpu().numpy(), col[v].cpu().numpy()), want)
    assert fuse_depth_frames([_gpu(c['depths']) for c in cs], K[0][0], E, 13, cs[0]['vl'], cs[0]['trunc'])[2] is None
    down = voxel_downsample_clouds(pts, 2.5 * cs[0]['vl'], nrm)
    assert len(down[0]) == 2 and all(0 < len(d) < len(p) for d, p in zip(down[0], pts))


@pytest.mark.parametrize('dtype', (np.uint16, np.float32), ids=['uint16', 'float32'])
@pytest.mark.parametrize('convention', ('reference', 'open3d'))
def test_depth_points_equal_the_host_entry(convention, dtype):
    from se3et_amd.tsdf import convert_depth_mat_to_points, depth_to_points_clouds
    depth, K = F.depth_image(dtype)
    wide = np.tile(depth, (1, 9))[:, :257]                              # a row longer than a workgroup
    blank = np.zeros_like(depth)
    for scale, limit in ((1000.0, 6.0), (500.0, 3.5)):
        got = depth_to_points_clouds(_gpu(np.stack([depth, blank, depth[::-1].copy()])), np.stack([K, K, K + 0.5]), scale, limit, convention)
        assert len(got) == 3 and all(g.dtype == torch.float64 and g.is_cuda for g in got) and tuple(got[1].shape) == (0, 3)
        assert F.same(got[0].cpu().numpy(), F.host_depth_points(depth, K, scale, limit, convention))
        assert F.same(got[2].cpu().numpy(), F.host_depth_points(depth[::-1].copy(), K + 0.5, scale, limit, convention))
        got = depth_to_points_clouds([_gpu(wide)], K, scale, limit, convention)
        assert F.same(got[0].cpu().numpy(), F.host_depth_points(wide, K, scale, limit, convention))
    K3 = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    assert F.same(convert_depth_mat_to_points(depth, K3), F.host_depth_points(depth, K, convention='reference'))
