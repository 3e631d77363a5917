"""GPU: the neighbour-limit calibration on the device -- the count-only radius search (exhaustive and grid kernel, each forced) against the
host entry and the numpy twin, the stacked histograms against every pair alone, and data.calibrate_neighbors_stack_mode against the
reference's own results (tests/golden/calibration.npz).  Everything is an integer: every comparison is whole-array equality."""
import warnings

import numpy as np
import pytest
import torch

import calibration_twin as twin
from calibration_fixture import CASES, OVER_64, dataset, direct_cases, expected

pytestmark = pytest.mark.gpu


def _t(a, dt):
    return torch.from_numpy(np.array(a)).to(dt).contiguous()


def _device_call(c, grid):
    """grid False: the exhaustive kernel; True: the grid kernel over a RadiusGrid built for the support, whatever its size."""
    from se3et_amd import ops
    q, s = _t(c['q'], torch.float32).cuda(), _t(c['s'], torch.float32).cuda()
    if c['q'] is c['s']:
        q = s
    ql, sl = _t(c['q_lengths'], torch.int64), _t(c['s_lengths'], torch.int64)
    start = {k: _t(c[k], torch.int32).cuda() for k in ('hist', 'dropped', 'max_count') if k in c}
    hist = start.get('hist', torch.zeros((c['num_slots'], c['hist_n']), dtype=torch.int32, device='cuda'))
    g = ops.RadiusGrid(s, sl, c['radius']) if grid else False
    out = ops.radius_count_hist(q, s, ql, sl, c['radius'], c['hist_n'], c['slots'], hist=hist, grid=g, dropped=start.get('dropped'),
                                max_count=start.get('max_count'))
    return [o.cpu().numpy() for o in out]


def _host_call(c):
    from se3et_amd import ext
    start = {k: _t(c[k], torch.int32).clone() for k in ('hist', 'dropped', 'max_count') if k in c}
    hist = start.get('hist', torch.zeros((c['num_slots'], c['hist_n']), dtype=torch.int32))
    out = ext.radius_count_hist(_t(c['q'], torch.float32), _t(c['s'], torch.float32), _t(c['q_lengths'], torch.int64), _t(c['s_lengths'], torch.int64),
                                c['radius'], c['hist_n'], c['slots'], hist=hist, dropped=start.get('dropped'), max_count=start.get('max_count'))
    return [o.numpy() for o in out]


def _check_all_ways(c, context):
    want = twin.count_hist(c['q'], c['s'], c['q_lengths'], c['s_lengths'], c['radius'], c['hist_n'], c['slots'], c['num_slots'],
                           c.get('hist'), c.get('dropped'), c.get('max_count'))
    for way, got in (('host', _host_call(c)), ('exhaustive', _device_call(c, False)), ('grid', _device_call(c, True))):
        for what, g, w in zip(('hist', 'dropped', 'max_count'), got, want):
            np.testing.assert_array_equal(g, w, err_msg='%s: %s %s' % (context, way, what))
    return want


@pytest.mark.parametrize('name', list(direct_cases()))
def test_count_search_direct_calls(name):
    _check_all_ways(direct_cases()[name], name)


@pytest.mark.parametrize('preset,case', [('c2_5k', 'c2'), ('c3_4k', 'kitti')])
def test_count_search_on_every_stage(preset, case):
    from se3et_amd import data
    from se3et_amd.synthetic import make_pair
    params = CASES[case][0]
    ref, src, _ = make_pair(preset, 0)
    pts = torch.from_numpy(np.concatenate([ref, src])).cuda()
    points, lengths = data.stage_clouds(pts, torch.tensor([len(ref), len(src)]), params['num_stages'], params['voxel_size'])
    hist_n, radius = data.calibration_hist_n(params['voxel_size'], params['search_radius']), params['search_radius']
    _, _, fixture = expected(case)
    for i in range(params['num_stages']):
        p = points[i].cpu().numpy()
        c = dict(q=p, s=p, q_lengths=lengths[i].tolist(), s_lengths=lengths[i].tolist(), radius=radius, hist_n=hist_n, slots=[0, 0], num_slots=1)
        want = _check_all_ways(c, '%s stage %d' % (preset, i))
        np.testing.assert_array_equal(want[0][0], fixture[0, i])           # (and the twin equals the reference)
        radius *= 2


def _stack(items):
    clouds = [torch.from_numpy(it[k]) for it in items for k in ('ref_points', 'src_points')]
    return torch.cat(clouds).cuda(), torch.tensor([c.shape[0] for c in clouds])


def _histograms(items, params):
    from se3et_amd import data
    pts, ln = _stack(items)
    return [t.numpy() for t in data.neighbor_histograms(pts, ln, params['num_stages'], params['voxel_size'], params['search_radius'])]


def test_stacked_histograms_equal_every_pair_alone_and_the_reference():
    params = CASES['c2_all'][0]
    items = dataset('c2_all')
    _, _, fixture = expected('c2_all')
    alone = [_histograms([it], params) for it in items]
    for a, f in zip(alone, fixture):
        np.testing.assert_array_equal(a[0][0], f)
        assert a[0].dtype == np.int32 and a[0].shape == (1, 4, 180) and a[1].shape == (1, 4) and a[2].shape == (1, 4)
    for n in (1, 2, 8, 16):
        group = [items[i % 8] for i in range(n)]
        hist, dropped, mc = _histograms(group, params)
        assert hist.shape == (n, 4, 180)
        for p in range(n):
            for got, want in zip((hist, dropped, mc), alone[p % 8]):
                np.testing.assert_array_equal(got[p], want[0], err_msg='%d stacked, pair %d' % (n, p))


def test_stacked_histograms_keep_the_dropped_rows_apart():
    """The dense pair (a third of its stage-0 rows beyond the last bin) stacked between ordinary ones."""
    params = CASES['dense'][0]
    group = [dataset('c1')[0], dataset('dense')[0], dataset('c1')[1]]
    hist, dropped, mc = _histograms(group, params)
    np.testing.assert_array_equal(hist[1], expected('dense')[2][0])
    np.testing.assert_array_equal(hist[0], expected('c1')[2][0])
    np.testing.assert_array_equal(hist[2], expected('c1')[2][1])
    assert dropped[:, 0].tolist() == [0, 13312, 0] and mc[1, 0] >= 180 and mc[0, 0] < 180


@pytest.mark.parametrize('name', list(CASES))
def test_device_calibration_equals_the_reference(name):
    from se3et_amd import data
    params, kwargs, _, _ = CASES[name]
    limits, pairs_used, hist = expected(name)
    items = dataset(name)
    for ppc in (1, 4, 16):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            got, details = data.calibrate_neighbors_stack_mode(items, data.registration_collate_fn_stack_mode, **params, **kwargs,
                                                               pairs_per_call=ppc, return_details=True)
        np.testing.assert_array_equal(got, limits, err_msg='pairs_per_call %d' % ppc)
        assert details['pairs_used'] == pairs_used
        np.testing.assert_array_equal(details['histograms'], hist)
        over = [w for w in caught if 'SE3_MAX_NEIGHBOR_LIMIT' in str(w.message)]
        assert len(over) == (1 if name in OVER_64 else 0)
    plain = data.calibrate_neighbors_stack_mode(items, None, **params, **kwargs) if name not in OVER_64 else None
    if plain is not None:
        assert isinstance(plain, np.ndarray) and plain.tolist() == limits.tolist()


def test_two_runs_and_a_side_stream_give_identical_tensors():
    params = CASES['c2'][0]
    items = dataset('c2')[:4]
    first = _histograms(items, params)
    for a, b in zip(first, _histograms(items, params)):
        np.testing.assert_array_equal(a, b)
    # the same on a side stream while the default stream is busy with count searches of its own (queued, not waited for)
    from se3et_amd import data, ops
    pts, ln = _stack(items)
    busy_pts, busy_ln = _stack(dataset('cap')[:1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    busy = [ops.radius_count_hist(busy_pts, busy_pts, busy_ln, busy_ln, 0.0625, 180, [0, 0], grid=False) for _ in range(4)]
    with torch.cuda.stream(side):
        got = [t.numpy() for t in data.neighbor_histograms(pts, ln, params['num_stages'], params['voxel_size'], params['search_radius'])]
    busy.append(ops.radius_count_hist(busy_pts, busy_pts, busy_ln, busy_ln, 0.0625, 180, [0, 0]))
    torch.cuda.synchronize()
    for a, b in zip(first, got):
        np.testing.assert_array_equal(a, b)
    for other in busy:
        np.testing.assert_array_equal(other[0][0].cpu().numpy(), expected('cap')[2][0, 0])
