"""Multiway registration on the device (csrc/pose_graph.hip, se3et_amd/pose_graph.py) against the host entries, the same text on host
memory, BIT FOR BIT; and multiway_registration against the same recipe run through the twins.  Shapes are the smallest at which the
kernels can go wrong: source row counts around one wave and around the lanes of the sums (63 .. 65, 255 .. 257); graphs of 1, 2 and 3
nodes, of 42 and 43 nodes (252 / 258 unknowns, either side of the 256 lanes of the factorisation), the node limit with the complete edge
set (2016), edge counts 0, 1 and around the lanes (255 .. 257, by duplicate edges), a start that rejects trials, and 32 graphs of mixed
sizes in one call."""
import numpy as np
import pytest
import torch

import icp_fixture as I
import pose_graph_fixture as F
from icp_twin import icp as twin_icp

pytestmark = pytest.mark.gpu

DEV = 'cuda'
T = F.twin


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the information matrix -------------------------------------------------------------------------------------------------------------------
def _info_pair(n, dtype, seed=70, nref=300, far=False):
    rng = np.random.default_rng(seed + n)
    ref, _nrm = I.sheet(rng, nref)
    on_ref = ref[rng.integers(0, nref, n)] + 0.004 * rng.normal(size=(n, 3))
    gt = I.rigid(rng, 25.0, 0.5)
    inv = np.linalg.inv(gt)
    src = on_ref @ inv[:3, :3].T + inv[:3, 3] + (50.0 if far else 0.0)
    return src.astype(dtype), ref.astype(dtype), I.rigid(rng, 1.0, 0.01) @ gt, 0.02


def _info_device(pairs):
    from se3et_amd.pose_graph import information_matrix_pairs
    r = pairs[0][3]
    out = information_matrix_pairs([_gpu(p[0]) for p in pairs], [_gpu(p[1]) for p in pairs], np.stack([p[2] for p in pairs]), r)
    return [{k: out[k][p].cpu().numpy() for k in out} for p in range(len(pairs))]


def _info_same(got, pair, what=''):
    want = F.host_information(*pair)
    assert np.array_equal(got['information'], want['information'], equal_nan=True), '%s: |dL| %.3e' % (
        what, np.nanmax(np.abs(got['information'] - want['information'])))
    assert got['count'] == want['count'] == want['information'][5, 5] and got['status'] == want['status'], what
    return want


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('n', [63, 64, 65, 255, 256, 257])
def test_information_matrix_equals_the_host_entry(n, dtype):
    pair = _info_pair(n, dtype)
    want = _info_same(_info_device([pair])[0], pair, 'n %d %s' % (n, dtype))
    assert 0 < want['count'] < n and want['status'] == 0


def test_information_matrix_of_a_pair_alone_and_in_a_batch_of_32():
    pairs = [_info_pair(40 + 7 * p, 'float64', seed=90 + p, nref=150 + 11 * p) for p in range(32)]
    batch = _info_device(pairs)
    for p in (0, 15, 31):
        alone = _info_device([pairs[p]])[0]
        assert np.array_equal(alone['information'], batch[p]['information']) and alone['count'] == batch[p]['count']
    for p in range(32):
        _info_same(batch[p], pairs[p], 'pair %d' % p)


def test_information_matrix_without_a_correspondence_is_zero():
    pair = _info_pair(65, 'float64', far=True)
    got = _info_device([pair])[0]
    _info_same(got, pair)
    assert got['count'] == 0 and not got['information'].any() and got['status'] == 0


def test_information_count_is_the_fitness_of_icp_times_the_rows():
    """count = fitness n of icp_pairs(max_iteration = 0) on the same inputs, exactly: fitness is count / n, one division, so the test is
    on that quotient (fitness n itself rounds once more and need not give the integer back) and on the integer nearest to fitness n."""
    from se3et_amd.icp import icp_pairs
    pairs = [_info_pair(n, 'float32') for n in (65, 257)]
    got = _info_device(pairs)
    ev = icp_pairs([_gpu(p[0]) for p in pairs], [_gpu(p[1]) for p in pairs], np.stack([p[2] for p in pairs]), pairs[0][3], max_iteration=0)
    fitness = ev['fitness'].cpu().numpy()
    for p, pair in enumerate(pairs):
        n = len(pair[0])
        assert got[p]['count'] / n == fitness[p] and round(fitness[p] * n) == got[p]['count'] > 0


# ---- the pose graphs ---------------------------------------------------------------------------------------------------------------------------
def _device(graphs, reference_node=-1, **options):
    from se3et_amd.pose_graph import optimize_pose_graphs
    out = optimize_pose_graphs([{k: (_gpu(v.astype(np.uint8)) if k == 'uncertain' else _gpu(v)) for k, v in g.items()} for g in graphs],
                               reference_node, **options)
    status, info, res = out['status'].cpu().numpy(), out['info'].cpu().numpy(), out['residuals'].cpu().numpy()
    return [{'poses': out['poses'][g].cpu().numpy(), 'confidence': out['confidence'][g].cpu().numpy(), 'kept': out['kept'][g].cpu().numpy(),
             'status': int(status[g]), 'info': info[g], 'residuals': res[g]} for g in range(len(graphs))]


def _assert_same(got, want, what=''):
    assert got['status'] == want['status'] and np.array_equal(got['info'], want['info']), '%s: status %d / %d, info %s / %s' % (
        what, got['status'], want['status'], got['info'], want['info'])
    assert np.array_equal(got['kept'], want['kept']), what
    for k in ('poses', 'confidence', 'residuals'):
        assert np.array_equal(got[k], want[k], equal_nan=True), '%s: %s differ by %.3e' % (what, k, np.nanmax(np.abs(got[k] - want[k])))


def _small(N, seed, closures='all'):
    """A scene of poses up to 40 degrees / 1 m whose start is the odometry chain with a 1 degree / 1 cm error on every node: no graph,
    however small, starts at its minimum."""
    g = F.scene(N, seed, closures, 'odometry', 40.0, 1.0)[0]
    rng = np.random.default_rng(seed + 1000)
    return dict(g, poses=np.stack([I.rigid(rng, 1.0, 0.01) @ x for x in g['poses']]) if N else g['poses'])


@pytest.mark.parametrize('name', ['chain3', 'sparse42', 'sparse43', 'complete64', 'identity6'])
def test_fixture_graphs_equal_the_host_entry(name):
    c = F.case(name)
    got = _device([c['graph']])[0]
    want = F.host_pgo(c['graph'])
    _assert_same(got, want, name)
    assert want['status'] == 0 and np.array_equal(want['info'], c['twin']['info'])
    if name == 'identity6':
        assert F.rejected_trials(want['trials']) > 0
    if name == 'complete64':
        assert len(c['graph']['edges']) == 2016


@pytest.mark.parametrize('N', [1, 2, 3])
def test_the_smallest_graphs(N):
    g = _small(N, 30 + N)
    assert len(g['edges']) == N * (N - 1) // 2
    _assert_same(_device([g])[0], F.host_pgo(g), 'N %d' % N)


@pytest.mark.parametrize('E', [0, 1, 255, 256, 257])
def test_edge_counts_around_the_lanes_by_duplicate_edges(E):
    g = _small(6, 40)
    pick = np.arange(E) % len(g['edges'])
    g = dict(g, **{k: g[k][pick] for k in ('edges', 'transforms', 'informations', 'uncertain')})
    want = F.host_pgo(g)
    _assert_same(_device([g])[0], want, 'E %d' % E)
    if E == 0:
        assert np.array_equal(want['poses'], g['poses']) and want['info'][0] == T.STOP_RIGHT_TERM


def test_a_graph_alone_and_in_a_batch_of_32_mixed_sizes():
    graphs = [_small(1 + (5 * g) % 13, 100 + g, 'all' if g % 3 else 2) for g in range(32)]
    batch = _device(graphs)
    for g in (0, 16, 31):
        _assert_same(_device([graphs[g]])[0], batch[g], 'graph %d alone' % g)
    for g in range(32):
        _assert_same(batch[g], F.host_pgo(graphs[g]), 'graph %d' % g)


@pytest.mark.parametrize('which', ['first', 'last'])
def test_the_reference_node_keeps_its_input_pose(which):
    g = _small(7, 50)
    ref = 0 if which == 'first' else 6
    got = _device([g], reference_node=ref)[0]
    _assert_same(got, F.host_pgo(g, reference_node=ref), 'reference node %d' % ref)
    assert np.array_equal(got['poses'][ref], g['poses'][ref])


def test_each_refusal_and_a_good_call_after_it():
    g = _small(5, 60)
    bad_pose, bad_index, loop = dict(g, poses=g['poses'].copy()), dict(g, edges=g['edges'].copy()), dict(g, edges=g['edges'].copy())
    bad_pose['poses'][2, 1, 3] = np.nan
    bad_index['edges'][3, 1] = 5
    loop['edges'][2] = (4, 4)
    empty = {k: v[:0] for k, v in g.items()}
    for graph, status in ((bad_pose, T.NONFINITE), (bad_index, T.BAD_INDEX), (loop, T.BAD_INDEX), (empty, T.EMPTY)):
        got, want = _device([graph, g]), F.host_pgo(graph)
        assert got[0]['status'] == want['status'] == status
        assert np.isnan(got[0]['poses']).all() and np.array_equal(got[0]['kept'], want['kept'])
        _assert_same(got[1], F.host_pgo(g), 'the good graph beside status %d' % status)
    got = _device([g], min_residual=float('nan'))[0]
    assert got['status'] == T.NONFINITE and np.isnan(got['poses']).all()
    _assert_same(_device([g])[0], F.host_pgo(g), 'the good call after the refusals')


# ---- multiway registration ---------------------------------------------------------------------------------------------------------------------
def _fragments(seed=5, K=4, n=700):
    """K overlapping fragments of one sampling of the sheet over [0, 1.6] x [0, 1]: fragment i holds the points with x in
    [0.2 i, 0.2 i + 1] (about 440 of them), with 1 mm of noise of its own, in its own frame (a few degrees and centimetres from the
    scene frame)."""
    rng = np.random.default_rng(seed)
    x, y = 1.6 * rng.random(n), rng.random(n)
    scene = np.stack([x, y, I._height(x, y)], 1)
    clouds, poses = [], []
    for i in range(K):
        pts = scene[(x >= 0.2 * i) & (x <= 0.2 * i + 1.0)]
        pts = pts + 0.001 * rng.normal(size=pts.shape)
        X = I.rigid(rng, 3.0, 0.02)
        inv = np.linalg.inv(X)
        clouds.append(pts @ inv[:3, :3].T + inv[:3, 3])
        poses.append(X)
    return clouds, np.stack(poses)


def _twin_recipe(clouds, coarse, fine, solver, descending):
    K = len(clouds)
    pairs = [(i, j) for i in range(K) for j in range(i + 1, K)]
    Ts, infos = [], []
    for s, t in pairs:
        a = twin_icp(clouds[s], clouds[t], np.eye(4), coarse)
        b = twin_icp(clouds[s], clouds[t], a['transform'], fine)
        for ev in a['evaluations'] + b['evaluations']:
            assert ev['threshold_margin'] >= I.THRESHOLD_MARGIN and ev['gap_margin'] >= I.GAP_MARGIN, 'another seed'
        m = T.information_matrix(clouds[s], clouds[t], b['transform'], fine)
        assert m['threshold_margin'] >= I.THRESHOLD_MARGIN and m['gap_margin'] >= I.GAP_MARGIN, 'another seed'
        Ts.append(b['transform']), infos.append(m['information'])
    poses = [np.eye(4)]
    for i in range(K - 1):
        poses.append(poses[i] @ np.linalg.inv(Ts[pairs.index((i, i + 1))]))
    graph = dict(poses=np.stack(poses), edges=np.array(pairs), transforms=np.stack(Ts), informations=np.stack(infos),
                 uncertain=np.array([t - s != 1 for s, t in pairs]))
    out = T.global_optimization(graph, solver, descending, max_correspondence_distance=fine, reference_node=0)
    F.check_margins('the fragments', out)
    return out


def test_multiway_registration_equals_the_recipe_through_the_twins():
    """The relative poses X_0^-1 X_i against icp_twin + pose_graph_twin.  Margin: 16 times the difference between two evaluations of the
    twin recipe that differ in the solver and the direction of the edge sums, with the floor of 1e-13 (the fixture's rule)."""
    from se3et_amd.pose_graph import multiway_registration
    clouds, gt = _fragments()
    coarse, fine = 0.1, 0.02
    out = multiway_registration([_gpu(c) for c in clouds], max_correspondence_distance_coarse=coarse, max_correspondence_distance_fine=fine)
    one, two = _twin_recipe(clouds, coarse, fine, 'cholesky', False), _twin_recipe(clouds, coarse, fine, 'lu', True)
    rel = lambda X: np.stack([np.linalg.inv(X[0]) @ x for x in X])
    bound = max(16 * np.abs(rel(one['poses']) - rel(two['poses'])).max(), F.FLOOR)
    got = out['poses'].cpu().numpy()
    diff = np.abs(rel(got) - rel(one['poses'])).max()
    print('|d rel| %.3e, margin %.3e, error against the truth %.3e' % (diff, bound, F.relative_error(got, gt)))
    assert int(out['status'][0]) == 0 and np.array_equal(out['kept'].cpu().numpy(), one['kept'])
    assert np.array_equal(got[0], np.eye(4)) and diff <= bound
    assert F.relative_error(got, gt) < 0.02
