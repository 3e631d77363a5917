"""GPU: grid subsampling and the radius search (csrc/grid_subsample.hip, csrc/radius_neighbors.hip) at their geometric edges -- the seeded
cases of precompute_edge_fixture.py (wrapped voxel indices, voxel counts on the bucket-growth steps of the order emulation, capped and
flat search grids, distances equal to the radius, the tile sizes of the exhaustive kernel, 32 stacked clouds with empty ones, far /
infinite / NaN queries ...) against the C oracle, which tests/test_precompute_edges_cpu.py pins to the reference's own binary on the same
cases.  The contract is bit-exact: points, normals, emission order, counts and indices are compared for equality (neighbour tables up to
the order of EXACTLY tied distances, helpers.assert_neighbors_equal)."""
import numpy as np
import pytest
import torch

import precompute_edge_fixture as F
from helpers import assert_neighbors_equal

pytestmark = pytest.mark.gpu

SPARE_ROWS = 37                     # rows behind the clouds of a chain on device lengths (they belong to no cloud)
_cache = {}


def _t(a, dtype=None):
    return torch.from_numpy(np.array(a)) if dtype is None else torch.tensor(list(a), dtype=dtype)


def _oracle_chain(name):
    """[(input of stage k, oracle's output of stage k)] of a grid case; computed once."""
    if ('grid', name) not in _cache:
        from oracle import native
        case = F.grid_cases()[name]
        cur = (_t(case['points']), _t(case['lengths'], torch.int64), _t(case['normals']))
        stages = []
        for k in range(F.CHAIN_STAGES):
            p, l, n = native.grid_subsample(cur[0], cur[1], cur[2], case['voxel'] * 2 ** k)
            stages.append((cur, (p, l, n)))
            cur = (p, l, n)
        _cache['grid', name] = stages
    return _cache['grid', name]


def _oracle_radius(name, case=None, limit=None):
    key = ('radius', name, limit)
    if key not in _cache:
        from oracle import native
        case = case or F.radius_cases()[name]
        _cache[key] = native.radius_search(_t(case['q']), _t(case['s']), _t(case['q_lengths'], torch.int64), _t(case['s_lengths'], torch.int64),
                                           case['radius'], case['limit'] if limit is None else limit)
    return _cache[key]


def _assert_stage(got, want, context):
    (gp, gn, gl), (sp, sl, sn) = got, want
    assert gl.cpu().tolist() == sl.tolist(), '%s: counts' % context
    m = int(sl.sum())
    assert torch.equal(gp[:m].cpu(), sp), '%s: points differ (selection or emission order)' % context
    assert torch.equal(gn[:m].cpu(), sn), '%s: normals' % context


@pytest.mark.parametrize('name', list(F.grid_cases()))
def test_grid_subsample_on_host_lengths_equals_the_oracle(name):
    """Every stage of the chain on its own, fed with the oracle's previous stage and lengths known on the host."""
    from se3et_amd import ops
    voxel = F.grid_cases()[name]['voxel']
    for k, ((p, l, n), want) in enumerate(_oracle_chain(name)):
        got = ops.grid_subsample(p.cuda(), l, n.cuda(), voxel * 2 ** k)
        assert got[0].shape[0] == p.shape[0]
        _assert_stage(got, want, '%s stage %d' % (name, k))


@pytest.mark.parametrize('name', list(F.grid_cases()))
def test_grid_subsample_chain_on_device_lengths_equals_the_oracle(name):
    """Three stages back to back on device lengths (no host synchronisation in between), spare rows behind the clouds."""
    from se3et_amd import ops
    case = F.grid_cases()[name]
    spare = torch.full((SPARE_ROWS, 3), 1e30)
    gp, gn = torch.cat((_t(case['points']), spare)).cuda(), torch.cat((_t(case['normals']), spare)).cuda()
    gl = _t(case['lengths'], torch.int64).cuda()
    got = []
    for k in range(F.CHAIN_STAGES):
        gp, gn, gl = ops.grid_subsample(gp, gl, gn, case['voxel'] * 2 ** k)
        assert gp.shape[0] == len(case['points']) + SPARE_ROWS
        got.append((gp, gn, gl))
    for k, (g, (_, want)) in enumerate(zip(got, _oracle_chain(name))):
        _assert_stage(g, want, '%s stage %d' % (name, k))


def _search_three_ways(case):
    """-> {'exhaustive' | 'grid': (table (Nq, limit), per-cloud max_count list), 'default': table (Nq, width)} on the device."""
    from se3et_amd import ops
    from se3et_amd.modules.ops import radius_search
    q, s = _t(case['q']).cuda(), _t(case['s']).cuda()
    ql, sl = _t(case['q_lengths'], torch.int64), _t(case['s_lengths'], torch.int64)
    out = {}
    old, ops.GRID_SEARCH_MIN_SUPPORT = ops.GRID_SEARCH_MIN_SUPPORT, 10 ** 12
    try:
        t, mc = ops.radius_neighbors(q, s, ql, sl, case['radius'], case['limit'])
    finally:
        ops.GRID_SEARCH_MIN_SUPPORT = old
    out['exhaustive'] = (t.cpu(), mc.cpu().tolist())
    t, mc = ops.RadiusGrid(s, sl, case['radius']).search(q, ql, case['limit'])
    out['grid'] = (t.cpu(), mc.cpu().tolist())
    out['default'] = radius_search(q, s, ql, sl, case['radius'], case['limit']).cpu()
    return out


def _cloud_maxima(counts, q_lengths):
    return [int(c.max()) if len(c) else 0 for c in F.split(counts, q_lengths)]


@pytest.mark.parametrize('name', list(F.radius_cases()))
def test_radius_search_three_ways_equals_the_oracle(name):
    case = F.radius_cases()[name]
    want, ns = _oracle_radius(name), len(case['s'])
    counts = (_oracle_radius(name, limit=0) < ns).sum(1).numpy()
    got = _search_three_ways(case)
    (te, me), (tg, mg) = got['exhaustive'], got['grid']
    assert me == mg == _cloud_maxima(counts, case['q_lengths']), 'per-cloud largest in-radius counts'
    assert torch.equal(tg, te), 'grid kernel and exhaustive kernel differ'
    width = min(case['limit'], max(me))
    assert width == want.shape[1]
    assert bool((te[:, width:] == ns).all()), 'columns past the largest count must be padding'
    q, s = _t(case['q']), _t(case['s'])
    with np.errstate(invalid='ignore'):
        assert_neighbors_equal(te[:, :width], want, q, s, name + ' exhaustive')
        assert_neighbors_equal(tg[:, :width], want, q, s, name + ' grid')
        assert_neighbors_equal(got['default'], want, q, s, name + ' default path')
    # the padding index is the STACKED support total, and rows keep to the support of their own cloud
    starts = np.concatenate([[0], np.cumsum(case['s_lengths'])])
    for b, rows in enumerate(F.split(np.arange(len(case['q'])), case['q_lengths'])):
        for t in (te, tg, got['default']):
            r = t[rows]
            assert bool((((r >= starts[b]) & (r < starts[b + 1])) | (r == ns)).all()), '%s: cloud %d reaches into another support' % (name, b)


def test_awkward_queries_get_padding_and_disturb_no_other_row():
    """Rows one cell outside the support box, on its corner, far away (1e6, +-1e30), infinite and NaN behind an ordinary cloud: the far,
    infinite and NaN rows hold padding only, every other row is what it is without them."""
    case = F.radius_cases()['awkward']
    base, keep = F.without_awkward_rows(case)
    got, alone = _search_three_ways(case), _search_three_ways(base)
    ns = len(case['s'])
    for form in ('exhaustive', 'grid', 'default'):
        t, a = (got[form][0], alone[form][0]) if form != 'default' else (got[form], alone[form])
        assert bool((t[case['awkward_rows']] == ns).all()), form
        assert torch.equal(t[keep], a), form
        if form != 'default':
            assert got[form][1] == alone[form][1], form


@pytest.mark.parametrize('name', list(F.radius_cases()))
def test_count_only_search_equals_the_oracle_histogram(name):
    """ops.radius_count_hist (exhaustive and grid kernel) against the histogram of the oracle's full-width search, with the last bin below
    and above the largest count; neighbouring clouds add into different histogram rows."""
    from se3et_amd import ops
    case = F.radius_cases()[name]
    counts = (_oracle_radius(name, limit=0) < len(case['s'])).sum(1).numpy()
    batch = len(case['q_lengths'])
    slots = [b % 2 for b in range(batch)]
    per_cloud = F.split(counts, case['q_lengths'])
    q, s = _t(case['q']).cuda(), _t(case['s']).cuda()
    ql, sl = _t(case['q_lengths'], torch.int64), _t(case['s_lengths'], torch.int64)
    grid = ops.RadiusGrid(s, sl, case['radius'])
    largest = int(counts.max())
    for hist_n in (max(1, largest // 2), largest + 3):
        want_hist = np.zeros((max(slots) + 1, hist_n), np.int64)
        want_dropped = np.zeros(max(slots) + 1, np.int64)
        for b, c in enumerate(per_cloud):
            want_hist[slots[b]] += np.bincount(c[c < hist_n], minlength=hist_n)
            want_dropped[slots[b]] += int((c >= hist_n).sum())
        for g in (False, grid):
            hist, dropped, mc = ops.radius_count_hist(q, s, ql, sl, case['radius'], hist_n, slots, grid=g)
            context = '%s hist_n %d %s' % (name, hist_n, 'grid' if g else 'exhaustive')
            np.testing.assert_array_equal(hist.cpu().numpy(), want_hist, err_msg=context)
            np.testing.assert_array_equal(dropped.cpu().numpy(), want_dropped, err_msg=context)
            assert mc.cpu().tolist() == _cloud_maxima(counts, case['q_lengths']), context
