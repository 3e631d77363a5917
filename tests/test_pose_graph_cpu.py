"""Multiway registration without a GPU: se3_debug_pair_information_host and se3_debug_pose_graph_host (the text of
csrc/pose_graph_core.h on host memory, run serially over the kernels' lanes) against the independent float64 twin
tests/pose_graph_twin.py on the seeded graphs of tests/pose_graph_fixture.py, and on known-answer, degenerate and edge cases.

Margins.  The library may differ from the twin by 16 times the twin's OWN spread -- the largest difference between float64 evaluations
of the twin that differ only in the solver (LU against Cholesky) and in the direction of the edge sums -- per quantity and case, at
least 1e-13: pose_graph_fixture.MARGINS, measured by tools/pose_graph_probe.py into profiles/pose_graph_probe.txt.  A graph built inside
a test gets the same rule, evaluated on the spot (pose_graph_fixture.spread_margins)."""
import numpy as np
import pytest

import icp_fixture as I
import pose_graph_fixture as F

T = F.twin
QUANTITIES = ('poses', 'confidence', 'residuals')


def _accepted(trials):
    return [[bool(t[2]) for t in p] for p in trials]


def _same_path(got, twin, what=''):
    """The trial sequence (accepted / rejected), the counts and stop reasons of both passes, the kept mask and the status."""
    assert got['status'] == twin['status'], what
    assert np.array_equal(got['info'], twin['info']), '%s: info %s, the twin %s' % (what, got['info'], twin['info'])
    assert _accepted(got['trials']) == _accepted([p['trials'] for p in twin['passes']]), what
    assert np.array_equal(got['kept'], twin['kept']), what


def _within(got, twin, margins, what=''):
    for q in QUANTITIES:
        if not twin[q].size:
            continue
        d = float(np.abs(got[q] - twin[q]).max())
        print('%s %s: |d| %.2e, margin %.2e' % (what, q, d, margins[q]))
        assert d <= margins[q], '%s: %s differ by %.3e (margin %.3e)' % (what, q, d, margins[q])


def _same_as_twin(graph, what='', **options):
    twin, margins = F.spread_margins(graph, **options)
    got = F.host_pgo(graph, **options)
    _same_path(got, twin, what)
    _within(got, twin, margins, what)
    return got, twin


def _small(N, seed, closures='all'):
    g = F.scene(N, seed, closures, 'odometry', 40.0, 1.0)[0]
    rng = np.random.default_rng(seed + 1000)
    return dict(g, poses=np.stack([I.rigid(rng, 1.0, 0.01) @ x for x in g['poses']]) if N else g['poses'])


def test_constants_are_the_headers():
    from se3et_amd import ops
    assert ops.PGO_STATUS == {'nonfinite': T.NONFINITE, 'singular': T.SINGULAR, 'empty': T.EMPTY, 'step_refused': T.STEP_REFUSED,
                              'bad_index': T.BAD_INDEX}
    assert {k: ops.PGO_STATUS[k] for k in ops.PGO_STATUS if k in ops.FGR_STATUS} == {k: ops.FGR_STATUS[k] for k in ops.PGO_STATUS}
    assert ops.PGO_STOP == {'none': 0, 'right_term': 1, 'relative_increment': 2, 'relative_residual': 3, 'residual': 4, 'max_iteration': 5,
                            'max_iteration_lm': 6, 'refused': 7}
    assert (ops.PGO_MAX_NODES, ops.PGO_MAX_EDGES) == (64, 2016) and ops.PGO_MAX_EDGES == 64 * 63 // 2
    assert ops.PGO_MAX_ITERATION >= 1000 and ops.PGO_MAX_ITERATION_LM >= 100


def test_the_arc_tangent_against_numpy():
    """Bound.  t = min / max is one rounding (0.5 ulp).  Above tan(pi / 8) the reduction u = (t - 1) / (t + 1) adds three (1.5 ulp of u,
    |u| <= 0.4143, d atan / du <= 1, the result >= 0.39: at most 1.6 ulp of the result).  The series' remainder is z^21 / 43 < 2e-18 of u;
    its Horner sum is rounded at the size of z / 3 <= 0.06, so u + (u z) q carries at most 0.6 ulp.  Each of the three constants is added
    as a high and a low part: two roundings, 1 ulp of a result that is then at least as large as before, so the earlier errors do not
    grow in ulp.  The worst chain is 0.5 + 1.6 + 0.6 + 1 with the later constants only shrinking the share of the earlier terms as the
    result doubles: below 3.7, and 4 ulp is asserted against numpy.arctan2 (itself within 1 ulp)."""
    rng = np.random.default_rng(1)
    ones = np.nextafter(1.0, [0.0, 2.0, 1.0])
    near = np.concatenate([ones, np.tan(np.pi / 8) * (1 + np.linspace(-1e-12, 1e-12, 41)), 1 + np.linspace(-1e-9, 1e-9, 41),
                           rng.uniform(0.0, 1.0, 4000), 10.0 ** rng.uniform(-20, 0, 500)])
    ys, xs = [], []
    for mag in 10.0 ** np.arange(-300.0, 301.0, 50.0):
        for sy in (1.0, -1.0):
            for sx in (1.0, -1.0):
                ys += [sy * mag * near, sy * mag * np.ones_like(near)]
                xs += [sx * mag * np.ones_like(near), sx * mag * near]
    y, x = np.concatenate(ys), np.concatenate(xs)
    got, ref = F.host_atan2(y, x), np.arctan2(y, x)
    ulp = np.abs(got - ref) / np.spacing(np.abs(ref))
    print('largest error %.2f ulp over %d points' % (ulp.max(), len(y)))
    assert ulp.max() <= 4.0
    # the axes and the signs of zero: the exact cases of the header comment
    axes_y = np.array([0.0, -0.0, 0.0, -0.0, 1e-300, -1e300, 3.0, -3.0])
    axes_x = np.array([2.0, 1e300, -2.0, -1e-300, 0.0, -0.0, -0.0, 0.0])
    got = F.host_atan2(axes_y, axes_x)
    assert np.array_equal(got, np.arctan2(axes_y, axes_x)) and np.array_equal(np.signbit(got), np.signbit(axes_y))
    zeros = F.host_atan2(np.array([0.0, -0.0, 0.0, -0.0]), np.array([0.0, 0.0, -0.0, -0.0]))
    assert np.array_equal(zeros, np.zeros(4))                               # (0, 0) gives a zero whatever the signs (numpy: +-pi for x = -0)
    tiny = F.host_atan2(np.array([1e-300, 5e-324]), np.array([1e300, 1.0]))
    assert np.array_equal(tiny, np.arctan2(np.array([1e-300, 5e-324]), np.array([1e300, 1.0])))


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('name', sorted(I.FAMILIES))
def test_information_matrix_equals_the_twin(name, dtype):
    c = I.case(name, 'point_to_point', dtype)                               # (asserts the fixture's margins at every evaluation)
    Tm, r = c['twin']['transform'], c['r']
    twin = T.information_matrix(c['src'], c['ref'], Tm, r)
    assert twin['threshold_margin'] >= I.THRESHOLD_MARGIN and twin['gap_margin'] >= I.GAP_MARGIN
    got = F.host_information(c['src'], c['ref'], Tm, r)
    assert got['status'] == 0 and np.array_equal(got['corr'], twin['corr'])
    assert got['count'] == got['information'][5, 5] == twin['count'] == c['twin']['evaluations'][-1]['n_corr']
    d = float(np.abs(got['information'] - twin['information']).max())
    print('%s %s: |dL| %.2e, margin %.2e' % (name, dtype, d, F.INFORMATION_MARGIN))
    assert d <= F.INFORMATION_MARGIN and np.array_equal(got['information'], got['information'].T)


def test_information_matrix_refusals():
    c = I.case('sheet700', 'point_to_point', 'float64')
    src, ref, Tm = c['src'].copy(), c['ref'].copy(), c['T0'].copy()
    for where in ('src', 'ref', 'T'):
        a = {'src': src.copy(), 'ref': ref.copy(), 'T': Tm.copy()}
        a[where][2, 1] = np.inf
        got = F.host_information(a['src'], a['ref'], a['T'], 0.1)
        assert got['status'] == T.NONFINITE and np.isnan(got['information']).all()
    for s, q in ((src[:0], ref), (src, ref[:0])):
        got = F.host_information(s, q, Tm, 0.1)
        assert got['status'] == T.EMPTY and not got['information'].any() and got['count'] == 0
    got = F.host_information(src + 40.0, ref, np.eye(4), 0.1)
    assert got['status'] == 0 and not got['information'].any() and (got['corr'] == -1).all()


@pytest.mark.parametrize('name', sorted(F.FAMILIES))
def test_host_entry_follows_the_twin(name):
    c = F.case(name)
    got, twin = F.host_pgo(c['graph'], **c['options']), c['twin']
    _same_path(got, twin, name)
    _within(got, twin, F.MARGINS[name], name)
    for (lam, rho, _acc, res), t in zip(got['trials'][0] + got['trials'][1], twin['passes'][0]['trials'] + twin['passes'][1]['trials']):
        assert abs(lam - t[0]) <= 1e-6 * t[0] and (np.isnan(res) and np.isnan(t[3]) or abs(res - t[3]) <= 1e-9 * max(1.0, abs(t[3])))


def test_the_fixture_holds_a_case_that_rejects_trials_and_one_at_every_size():
    assert F.rejected_trials(F.case('identity6')['twin']['passes']) > 0 and F.rejected_trials(F.case('identity12')['twin']['passes']) > 0
    assert sorted(len(F.case(n)['graph']['poses']) for n in F.FAMILIES) == [3, 6, 6, 12, 12, 42, 43, 64]
    assert len(F.case('complete64')['graph']['edges']) == 2016
    assert set(F.MARGINS) == set(F.FAMILIES) and all(m[q] >= F.FLOOR for m in F.MARGINS.values() for q in QUANTITIES)


@pytest.mark.parametrize('name', ['ring6', 'sparse12', 'sparse43', 'complete64'])
def test_the_line_process_prunes_the_false_edges_and_beats_the_odometry_chain(name):
    """On the twin alone: the optimised poses are nearer the truth than the odometry chain, and with every edge marked certain they are
    farther than with the line process."""
    c = F.case(name)
    twin = c['twin']
    assert np.array_equal(~twin['kept'], c['false']) and c['false'].any()
    err, chain = F.relative_error(twin['poses'], c['gt']), F.relative_error(c['graph']['poses'], c['gt'])
    if name == 'complete64':
        certain = None                                                      # (the twin at this size again: the smaller cases make the point)
    else:
        certain = T.global_optimization(dict(c['graph'], uncertain=np.zeros(len(c['false']), bool)))
    print('%s: error %.2e, the chain %.2e, all certain %s' % (name, err, chain, certain and F.relative_error(certain['poses'], c['gt'])))
    assert err < chain
    assert certain is None or F.relative_error(certain['poses'], c['gt']) > err


def test_refusals_in_their_order():
    g = _small(5, 60)
    nan_pose, nan_T, nan_info = dict(g, poses=g['poses'].copy()), dict(g, transforms=g['transforms'].copy()), dict(g, informations=g['informations'].copy())
    nan_pose['poses'][1, 0, 0], nan_T['transforms'][2, 1, 3], nan_info['informations'][0, 5, 5] = np.nan, np.inf, np.nan
    bad = dict(g, edges=g['edges'].copy())
    bad['edges'][1, 0] = -1
    for graph, opts in ((nan_pose, {}), (nan_T, {}), (nan_info, {}), (g, dict(min_right_term=np.nan)), (dict(nan_pose, edges=bad['edges']), {})):
        got = F.host_pgo(graph, **opts)
        assert got['status'] == T.NONFINITE and np.isnan(got['poses']).all() and not got['kept'].any()
        assert got['info'][0] == got['info'][3] == T.STOP_REFUSED
    for e in ((-1, 2), (5, 2), (2, 5), (3, 3)):
        bad['edges'][1] = e
        got = F.host_pgo(bad)
        assert got['status'] == T.BAD_INDEX and np.isnan(got['poses']).all()
    empty = {k: v[:0] for k, v in g.items()}
    got = F.host_pgo(empty)
    assert got['status'] == T.EMPTY
    got = F.host_pgo(dict(empty, **{k: bad[k] for k in ('edges', 'transforms', 'informations', 'uncertain')}))
    assert got['status'] == T.EMPTY                                         # no node: empty comes before the index
    from se3et_amd._lib import lib
    assert F.host_pgo(g)['status'] == 0
    with pytest.raises(RuntimeError, match='debug_pose_graph_host'):
        F.host_pgo(g, max_iteration=10 ** 6)
    with pytest.raises(RuntimeError, match='reference node'):
        F.host_pgo(g, reference_node=5)
    big = {'poses': np.tile(np.eye(4), (65, 1, 1)), 'edges': np.zeros((0, 2), np.int64), 'transforms': np.zeros((0, 4, 4)),
           'informations': np.zeros((0, 6, 6)), 'uncertain': np.zeros((0,), bool)}
    with pytest.raises(RuntimeError, match='65 nodes'):
        F.host_pgo(big)
    assert b'65 nodes' in lib().se3_last_error()


def test_no_edge_one_node_and_duplicate_edges():
    g = _small(4, 61)
    none = dict(g, **{k: g[k][:0] for k in ('edges', 'transforms', 'informations', 'uncertain')})
    got = F.host_pgo(none)
    assert got['status'] == 0 and np.array_equal(got['poses'], g['poses']) and list(got['info']) == [T.STOP_RIGHT_TERM, 0, 0, T.STOP_RIGHT_TERM, 0, 0]
    one = _small(1, 62)
    got = F.host_pgo(one, reference_node=0)
    assert got['status'] == 0 and np.array_equal(got['poses'], one['poses'])
    twice = dict(g, **{k: np.concatenate([g[k], g[k]]) for k in ('edges', 'transforms', 'informations', 'uncertain')})
    got, _twin = _same_as_twin(twice, 'every edge twice')
    single = F.host_pgo(g)
    assert got['status'] == 0 and not np.array_equal(got['residuals'], single['residuals'])          # each copy adds
    assert np.abs(got['poses'] - single['poses']).max() < 1e-2


@pytest.mark.parametrize('ref', [0, 3, 6])
def test_the_reference_node_returns_its_input_pose_exactly(ref):
    g = _small(7, 50)
    got, _twin = _same_as_twin(g, 'reference node %d' % ref, reference_node=ref)
    free = F.host_pgo(g)
    assert np.array_equal(got['poses'][ref], g['poses'][ref]) and not np.array_equal(free['poses'][ref], g['poses'][ref])
    rel = lambda X: np.stack([np.linalg.inv(X[ref]) @ x for x in X])
    assert np.abs(rel(got['poses']) - rel(free['poses'])).max() <= 1e-13
    assert np.array_equal(got['confidence'], free['confidence']) and np.array_equal(got['residuals'], free['residuals'])


def test_renumbering_the_nodes_gives_the_same_poses():
    c = F.case('sparse12')
    g = c['graph']
    perm = np.random.default_rng(3).permutation(12)                          # new index of every node
    inv = np.argsort(perm)
    moved = dict(g, poses=g['poses'][inv], edges=perm[g['edges']])
    a, b = F.host_pgo(g), F.host_pgo(moved)
    assert np.array_equal(a['info'], b['info']) and np.array_equal(a['kept'], b['kept'])
    d = float(np.abs(b['poses'][perm] - a['poses']).max())
    print('|d| %.2e, margin %.2e' % (d, F.MARGINS['sparse12']['poses']))
    assert d <= F.MARGINS['sparse12']['poses'] and np.abs(a['confidence'] - b['confidence']).max() <= F.MARGINS['sparse12']['confidence']


def test_runs_are_bit_identical():
    c = F.case('sparse42')
    a, b = F.host_pgo(c['graph']), F.host_pgo(c['graph'])
    assert all(np.array_equal(a[q], b[q]) for q in QUANTITIES)
    assert all(np.array_equal(np.array(x), np.array(y), equal_nan=True) for x, y in zip(a['trials'], b['trials']))


def test_batched_functions_refuse_bad_arguments():
    import torch
    from se3et_amd import pose_graph
    a = torch.zeros((4, 3))
    with pytest.raises(RuntimeError, match='GPU tensor'):
        pose_graph.information_matrix_pairs([a], [a], None, 0.1)
    with pytest.raises(ValueError, match='one source and one reference'):
        pose_graph.information_matrix_pairs([a], [], None, 0.1)
    with pytest.raises(ValueError, match='max_correspondence_distance'):
        pose_graph.information_matrix_pairs([a], [a], None, -1.0)
    g = _small(3, 63)
    with pytest.raises(ValueError, match='unknown option'):
        pose_graph.optimize_pose_graphs([g], device='cpu', tolerance=1.0)
    with pytest.raises(ValueError, match='max_iteration'):
        pose_graph.optimize_pose_graphs([g], device='cpu', max_iteration=-1)
    with pytest.raises(ValueError, match='one reference node per graph'):
        pose_graph.optimize_pose_graphs([g], [0, 1], device='cpu')
    with pytest.raises(ValueError, match='has no'):
        pose_graph.optimize_pose_graphs([{k: v for k, v in g.items() if k != 'uncertain'}], device='cpu')
    with pytest.raises(ValueError, match='needs the normals'):
        pose_graph.multiway_registration([a, a], estimation='point_to_plane', device='cpu')
