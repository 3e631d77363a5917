"""The twin of the superpoint-level selections (superpoint_twin.py) on the seeded lattice cases of superpoint_edge_fixture.py: every case
holds the property it exists for, the lattice makes the reference's float32 distance expression (and the cross and dot products of the
angle) exact, and the twin agrees with oracle.se3et_oracle -- point_to_node_partition and the topk line of embedding_indices -- on every
case the oracle can take (limit <= N, N >= 4), everywhere except inside groups of exactly tied distances, which the oracle's torch.topk /
min leave to an unstable selection.  tests/test_gpu_superpoint_edges.py holds the HIP kernels to the twin, which closes the chain HIP
kernel == twin == oracle up to the reference's own tie freedom."""
import numpy as np
import pytest
import torch

import superpoint_edge_fixture as F
import superpoint_twin as T


def _t(a):
    return torch.from_numpy(np.array(a))                                    # (a copy: the fixture's arrays are read-only)


@pytest.mark.parametrize('name', list(F.partition_cases()))
def test_partition_case_holds_its_property(name):
    F.check_partition_case(name, F.partition_cases()[name])


@pytest.mark.parametrize('name', list(F.knn3_cases()))
def test_knn3_case_holds_its_property(name):
    F.check_knn3_case(name, F.knn3_cases()[name])


@pytest.mark.parametrize('name', list(F.embedding_cases()))
def test_embedding_case_holds_its_property(name):
    case = F.embedding_cases()[name]
    F.check_embedding_case(name, case, T.knn3(case['points']))


def _all_clouds():
    for name, case in F.partition_cases().items():
        yield 'partition/' + name, case['nodes'], case['points']
    for kind, cases in (('knn3', F.knn3_cases()), ('embedding', F.embedding_cases())):
        for name, case in cases.items():
            yield '%s/%s' % (kind, name), case['points'], case['points']


def test_the_lattice_makes_the_float32_distance_expression_exact():
    """x2 - 2 xy + y2 in float32 -- as torch evaluates it (the oracle) and one float32 operation at a time in the kernel's order -- times 64
    IS the integer squared distance, on every case."""
    from oracle import se3et_oracle as O
    for name, x, y in _all_clouds():
        want = T.sq_units(x, y)
        assert want.max() < 2 ** 16
        got = O.pairwise_distance(_t(x), _t(y))
        assert got.dtype == torch.float32 and np.array_equal(got.numpy().astype(np.float64) * 64, want), name
        assert np.array_equal(T.ref_sq_dist_f32(x, y).astype(np.float64) * 64, want), name


def test_the_lattice_makes_cross_and_dot_products_exact():
    """ref x anc and ref . anc of the angle index in float32 equal the integer products (in 1 / 64 units) on every embedding case."""
    for name, case in F.embedding_cases().items():
        p, k, knn = case['points'], T.lattice_units(case['points']), T.knn3(case['points'])
        ref, anc = np.broadcast_arrays((p[knn] - p[:, None, :])[:, None], (p[None, :, :] - p[:, None, :])[:, :, None])
        iref, ianc = np.broadcast_arrays((k[knn] - k[:, None, :])[:, None], (k[None, :, :] - k[:, None, :])[:, :, None])
        cross = np.stack([ref[..., 1] * anc[..., 2] - ref[..., 2] * anc[..., 1], ref[..., 2] * anc[..., 0] - ref[..., 0] * anc[..., 2],
                          ref[..., 0] * anc[..., 1] - ref[..., 1] * anc[..., 0]], -1)
        dot = (ref[..., 0] * anc[..., 0] + ref[..., 1] * anc[..., 1]) + ref[..., 2] * anc[..., 2]
        assert cross.dtype == dot.dtype == np.float32
        assert np.array_equal(cross.astype(np.float64) * 64, np.cross(iref, ianc)), name
        assert np.array_equal(dot.astype(np.float64) * 64, (iref * ianc).sum(-1)), name


def _oracle_partition_clouds():
    """(id, points, nodes, limit) of every single cloud and every cloud of a stack case that the oracle's topk can take."""
    out = []
    for name, case in F.partition_cases().items():
        clouds = [(name, case['points'], case['nodes'])] if 'point_lengths' not in case else \
            [('%s[%d]' % (name, c),) + F.cloud_of(case, c) for c in range(len(case['point_lengths']))]
        for cid, p, nd in clouds:
            out += [('%s-limit%d' % (cid, k), p, nd, k) for k in case['limits'] if k <= len(p) and len(p) >= 4]
    return out


@pytest.mark.parametrize('cid,points,nodes,limit', _oracle_partition_clouds(), ids=[c[0] for c in _oracle_partition_clouds()])
def test_twin_partition_equals_the_oracle_outside_exact_ties(cid, points, nodes, limit):
    from oracle import se3et_oracle as O
    want = [t.numpy() for t in O.point_to_node_partition(_t(points), _t(nodes), limit)]
    got = T.point_to_node_partition(points, nodes, limit)
    d = T.sq_units(nodes, points)
    ways = (d == d.min(0, keepdims=True)).sum(0)
    differ = got[0] != want[0]
    assert (ways[differ] > 1).all(), 'point_to_node differs away from an exact node tie'
    assert (d[got[0], np.arange(len(points))] == d[want[0], np.arange(len(points))]).all()
    # nodes whose own points the two sides agree on (an exact node tie resolved differently moves a point between two nodes)
    settled = np.ones(len(nodes), bool)
    settled[got[0][differ]] = settled[want[0][differ]] = False
    if not differ.any():
        assert np.array_equal(got[1], want[1]), 'node_masks'
    n = len(points)
    dpad = np.concatenate([d, np.full((len(nodes), 1), -1)], 1)            # (padding: distance -1)
    for m in np.nonzero(settled)[0]:
        assert np.array_equal(got[3][m], want[3][m]), 'node %d: node_knn_masks' % m
        dg, dw = dpad[m][got[2][m]], dpad[m][want[2][m]]
        assert np.array_equal(dg, dw), 'node %d: the selected distances differ' % m
        own = d[m][got[0] == m]
        untied = np.array([(own == v).sum() == 1 for v in dg]) | (got[2][m] == n)
        assert np.array_equal(got[2][m][untied], want[2][m][untied]), 'node %d: differs outside a group of tied distances' % m
        assert (got[0][got[2][m][got[3][m]]] == m).all() and len(set(want[2][m][want[3][m]].tolist())) == int(want[3][m].sum())


@pytest.mark.parametrize('name', [k for k, v in list(F.knn3_cases().items()) + list(F.embedding_cases().items())
                                  if 'lengths' not in v and len(v['points']) >= 4])
def test_twin_knn3_equals_the_oracles_topk_outside_exact_ties(name):
    """The topk line of oracle.se3et_oracle.embedding_indices: dist.topk(k + 1, largest=False)[1][:, 1:]."""
    from oracle import se3et_oracle as O
    case = F.knn3_cases().get(name) or F.embedding_cases()[name]
    p = case['points']
    dist = torch.sqrt(O.pairwise_distance(_t(p), _t(p)))
    want = dist.topk(4, dim=1, largest=False)[1][:, 1:].numpy()
    got = T.knn3(p)
    d = T.sq_units(p, p)
    rows = np.arange(len(p))[:, None]
    assert np.array_equal(d[rows, got], d[rows, want]), 'the kept distances differ'
    s = np.sort(d, 1)[:, :5]
    untied = ~(s[:, 1:] == s[:, :-1]).any(1)
    assert np.array_equal(got[untied], want[untied]), 'differs in a row without tied distances'


@pytest.mark.parametrize('name', [k for k, v in F.embedding_cases().items() if len(v['points']) >= 4])
def test_twin_embedding_indices_equal_the_oracle_for_the_same_knn(name):
    """float64 on both sides; the oracle's knn is its own topk line on the same float64 distances, handed to the twin."""
    from oracle import se3et_oracle as O
    p = _t(F.embedding_cases()[name]['points']).double()
    knn = torch.sqrt(O.pairwise_distance(p, p)).topk(4, dim=1, largest=False)[1][:, 1:]
    want_d, want_a = O.embedding_indices(p, 0.2, 15.0, 3)
    got_d, got_a = T.embedding_indices(p.numpy(), knn.numpy(), 0.2, 15.0)
    np.testing.assert_allclose(got_d, want_d.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(got_a, want_a.numpy(), rtol=0, atol=1e-12)
    assert got_a.min() == 0.0 and got_a.max() <= 12.0 + 1e-12


def test_twin_contract_on_a_hand_made_cloud():
    """knn3 drops rank 0 and not 'self'; fewer than 4 points give the own index; the nearest node and the own points go by index among equals;
    a limit above the cloud pads."""
    pts = np.array([[1, 1, 1], [1, 1, 1], [2, 1, 1], [1, 1, 1]], np.float32)            # points 0, 1, 3 coincide
    assert T.knn3(pts).tolist() == [[1, 3, 2], [1, 3, 2], [0, 1, 3], [1, 3, 2]]
    assert T.knn3(pts[:1]).tolist() == [[0, 0, 0]]
    assert T.knn3(pts[1:3]).tolist() == [[1, 0, 0], [0, 1, 1]]
    assert T.knn3_stack(pts, [1, 3]).tolist() == [[0, 0, 0], [2, 1, 0], [0, 2, 1], [2, 1, 2]]
    nodes = np.array([[3, 1, 1], [1, 1, 1], [1, 1, 1], [0, 1, 1]], np.float32)
    p2n, masks, knn, km = T.point_to_node_partition(pts, nodes, 5)
    assert p2n.tolist() == [1, 1, 0, 1] and masks.tolist() == [True, True, False, False]
    assert knn.tolist() == [[2, 4, 4, 4, 4], [0, 1, 3, 4, 4], [4] * 5, [4] * 5] and np.array_equal(km, knn < 4)
    p2n, masks, knn, km = T.point_to_node_partition_stack(pts, nodes, [1, 3], [1, 3], 2)
    assert p2n.tolist() == [0, 1, 1, 1] and masks.tolist() == [True, True, False, False]
    assert knn.tolist() == [[0, 4], [1, 3], [4, 4], [4, 4]]
