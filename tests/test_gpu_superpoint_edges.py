"""GPU: the selections on the superpoint level at their exact ties and capacity edges -- csrc/partition.hip (se3_knn3,
se3_point_to_node_partition and their stack forms), the index half of the geometric embedding (csrc/geo_records.hip,
csrc/geo_embedding.hip) and the superpoint scores (csrc/matching.hip) -- on the seeded lattice cases of superpoint_edge_fixture.py
against the twin (superpoint_twin.py), which tests/test_superpoint_edges_cpu.py pins to the oracle on the same cases.

On the lattice every distance is exact in float32, so ties are real ties and the contract of csrc/partition.hip -- ascending (distance,
index) -- leaves nothing open: every selection is compared with torch.equal.  The only tolerances in this file are the ones the
existing tests of the same ops use: 1e-4 (embedding, scores) and 1e-5 (equivariant embedding), helpers.assert_close."""
import numpy as np
import pytest
import torch

import superpoint_edge_fixture as F
import superpoint_twin as T
from helpers import assert_close, rel_err

pytestmark = pytest.mark.gpu

SIGMA_D, SIGMA_A = 0.2, 15.0
_cache = {}


def _t(a):
    return torch.from_numpy(np.array(a))                                    # (a copy: the fixture's arrays are read-only)


def _twin(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _assert_partition(got, want, context):
    assert len(got) == len(want) == 4
    for g, w, what in zip(got, want, ('point_to_node', 'node_masks', 'node_knn_indices', 'node_knn_masks')):
        w = _t(w)
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w), '%s: %s' % (context, what)


# ---- point_to_node_partition ------------------------------------------------------------------------------------------------------------
_SINGLE = [(name, k) for name, case in F.single_cloud_cases().items() for k in case['limits']]
_STACK = [(name, k) for name, case in F.stack_cases().items() for k in case['limits']]


@pytest.mark.parametrize('name,limit', _SINGLE, ids=['%s-limit%d' % c for c in _SINGLE])
def test_partition_equals_the_twin(name, limit):
    """All four outputs, exactly; the stack entry point with this one cloud gives the same."""
    from se3et_amd import ops
    case = F.partition_cases()[name]
    want = _twin(('partition', name, limit), lambda: T.point_to_node_partition(case['points'], case['nodes'], limit))
    p, nd = _t(case['points']).cuda(), _t(case['nodes']).cuda()
    _assert_partition(ops.point_to_node_partition(p, nd, limit), want, '%s limit %d' % (name, limit))
    _assert_partition(ops.point_to_node_partition_stack(p, nd, [len(p)], [len(nd)], limit), want, '%s limit %d, one-cloud stack' % (name, limit))


@pytest.mark.parametrize('name,limit', _STACK, ids=['%s-limit%d' % c for c in _STACK])
def test_partition_stack_equals_the_twin_and_per_cloud_calls(name, limit):
    from se3et_amd import ops
    case = F.partition_cases()[name]
    pl, nl = case['point_lengths'], case['node_lengths']
    want = _twin(('partition', name, limit), lambda: T.point_to_node_partition_stack(case['points'], case['nodes'], pl, nl, limit))
    P, M = _t(case['points']).cuda(), _t(case['nodes']).cuda()
    got = ops.point_to_node_partition_stack(P, M, pl, nl, limit)
    _assert_partition(got, want, '%s limit %d' % (name, limit))
    p0 = m0 = 0
    for c, (n, m) in enumerate(zip(pl, nl)):
        a, b, k, km = ops.point_to_node_partition(P[p0:p0 + n].contiguous(), M[m0:m0 + m].contiguous(), limit)
        assert torch.equal(got[0][p0:p0 + n], a + m0), 'cloud %d' % c
        assert torch.equal(got[1][m0:m0 + m], b), 'cloud %d' % c
        assert torch.equal(got[2][m0:m0 + m], torch.where(k == n, torch.full_like(k, P.shape[0]), k + p0)), 'cloud %d' % c
        assert torch.equal(got[3][m0:m0 + m], km), 'cloud %d' % c
        p0 += n
        m0 += m


# ---- knn3 -------------------------------------------------------------------------------------------------------------------------------
def _knn3(points):
    from se3et_amd import ops
    from se3et_amd._lib import check, lib
    knn = torch.empty((points.shape[0], 3), dtype=torch.int64, device='cuda')
    check(lib().se3_knn3(points.data_ptr(), points.shape[0], knn.data_ptr(), ops._stream()), 'se3_knn3')
    return knn


@pytest.mark.parametrize('name', list(F.knn3_cases()))
def test_knn3_equals_the_twin(name):
    """Rank 0 of the (distance, index) order is dropped whichever point it is; clouds of 1, 2 and 3 points fill up with the own index."""
    from se3et_amd import ops
    case = F.knn3_cases()[name]
    p = _t(case['points']).cuda()
    lengths = case.get('lengths', [len(p)])
    want = _t(_twin(('knn3', name), lambda: T.knn3_stack(case['points'], lengths)))
    assert torch.equal(ops.knn3_stack(p, lengths).cpu(), want), 'se3_knn3_stack'
    o = 0
    for n in lengths:
        assert torch.equal(_knn3(p[o:o + n].contiguous()).cpu(), want[o:o + n]), 'se3_knn3, cloud at %d' % o
        o += n


# ---- rejections -------------------------------------------------------------------------------------------------------------------------
def test_bad_limits_and_clouds_are_rejected_and_the_next_call_works():
    from se3et_amd import ops
    case = F.partition_cases()['stack_cuts']
    pl, nl = case['point_lengths'], case['node_lengths']
    P, M = _t(case['points']).cuda(), _t(case['nodes']).cuda()
    one_p, one_n = P[:pl[0] + pl[1] + pl[2]][-pl[2]:].contiguous(), M[:nl[0] + nl[1] + nl[2]][-nl[2]:].contiguous()          # cloud 2: 3 points, 2 nodes
    want_stack = T.point_to_node_partition_stack(case['points'], case['nodes'], pl, nl, 3)
    want_one = T.point_to_node_partition(one_p.cpu().numpy(), one_n.cpu().numpy(), 3)
    want_knn = _t(T.knn3_stack(case['points'], pl))
    spread = lambda total, parts: [1] * (parts - 1) + [total - (parts - 1)]
    empty = lambda lengths, at: [0 if i == at else v + (lengths[at] if i == at + 1 else 0) for i, v in enumerate(lengths)]
    bad = [lambda: ops.point_to_node_partition(one_p, one_n, 0),
           lambda: ops.point_to_node_partition(one_p, one_n, F.MAX_LIMIT + 1),
           lambda: ops.point_to_node_partition(one_p[:0], one_n, 3),
           lambda: ops.point_to_node_partition(one_p, one_n[:0], 3),
           lambda: ops.point_to_node_partition_stack(P, M, pl, nl, 0),
           lambda: ops.point_to_node_partition_stack(P, M, pl, nl, F.MAX_LIMIT + 1),
           lambda: ops.point_to_node_partition_stack(P, M, spread(len(P), F.MAX_BATCH + 1), spread(len(M), F.MAX_BATCH + 1), 3),
           lambda: ops.point_to_node_partition_stack(P, M, empty(pl, 3), nl, 3),
           lambda: ops.point_to_node_partition_stack(P, M, pl, empty(nl, 3), 3),
           lambda: ops.knn3_stack(P, spread(len(P), F.MAX_BATCH + 1)),
           lambda: ops.knn3_stack(P, empty(pl, 3))]
    assert sum(empty(pl, 3)) == len(P) and empty(pl, 3)[3] == 0 and len(spread(len(M), F.MAX_BATCH + 1)) == F.MAX_BATCH + 1
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
        _assert_partition(ops.point_to_node_partition_stack(P, M, pl, nl, 3), want_stack, 'stack call after rejection %d' % i)
        _assert_partition(ops.point_to_node_partition(one_p, one_n, 3), want_one, 'call after rejection %d' % i)
        assert torch.equal(ops.knn3_stack(P, pl).cpu(), want_knn), 'knn3_stack after rejection %d' % i
    # exactly 32 clouds are taken
    assert torch.equal(ops.knn3_stack(P, spread(len(P), F.MAX_BATCH)).cpu(), _t(T.knn3_stack(case['points'], spread(len(P), F.MAX_BATCH))))


# ---- geometric embedding ----------------------------------------------------------------------------------------------------------------
def _weights(C):
    def make():
        from se3et_amd import tables
        g = torch.Generator().manual_seed(80 + C)
        st = {'e.embedding.div_term': torch.exp(torch.arange(0, C, 2).float() * (-np.log(10000.0) / C))}
        for n in ('d', 'a'):
            st['e.proj_%s.weight' % n] = torch.randn(C, C, generator=g) / C ** 0.5
            st['e.proj_%s.bias' % n] = torch.randn(C, generator=g) * 0.1
        st['e.anchors_wignerD.0'], st['e.anchors_wignerD.1'] = [torch.from_numpy(t) for t in tables.wigner_tables()]
        return st
    return _twin(('weights', C), make)


def _embedding_twin(name, C):
    def make():
        st, pts = _weights(C), F.embedding_cases()[name]['points']
        knn = T.knn3(pts)
        return knn, T.embedding(pts, knn, SIGMA_D, SIGMA_A, st['e.embedding.div_term'], st['e.proj_d.weight'], st['e.proj_d.bias'],
                                st['e.proj_a.weight'], st['e.proj_a.bias'])
    return _twin(('embedding', name, C), make)


def _embed(name, C, eq, knn, dtype=torch.float32):
    from se3et_amd import functional as SF
    st = _weights(C)
    c = lambda k: st[k].cuda()
    return SF.geometric_embedding(_t(F.embedding_cases()[name]['points']).cuda(), c('e.embedding.div_term'), c('e.proj_d.weight'), c('e.proj_d.bias'),
                                  c('e.proj_a.weight'), c('e.proj_a.bias'), SIGMA_D, SIGMA_A, 3, wigner_d1=c('e.anchors_wignerD.1') if eq else None,
                                  dtype=dtype, knn=None if knn is None else _t(knn).cuda())


@pytest.mark.parametrize('eq', [False, True])
@pytest.mark.parametrize('C', [32, 48])                   # 32: channel slices (csrc/geo_records.hip writes the indices); 48: the single-kernel form
@pytest.mark.parametrize('name', list(F.embedding_cases()))
def test_geometric_embedding_at_degenerate_geometry_equals_the_twin(name, C, eq):
    """Coincident superpoints, vanishing reference vectors, angles of exactly 0, 90 and 180 degrees: the embedding from the twin's knn
    against the float64 twin, the n == m diagonal included (on the lattice the self distance is exactly 0); with knn=None (se3_knn3's own
    tie order) the result is the same bit for bit."""
    from oracle import se3et_oracle as O
    knn, want = _embedding_twin(name, C)
    out = _embed(name, C, eq, knn)
    emb = out[0] if eq else out
    assert bool(torch.isfinite(emb).all())
    assert_close(emb.cpu(), want, 1e-4, '%s C %d: geometric embedding' % (name, C))
    own = _embed(name, C, eq, None)
    assert torch.equal(own[0] if eq else own, emb), 'knn=None differs from the twin knn: tie order of se3_knn3'
    if eq:
        pts = _t(F.embedding_cases()[name]['points'])
        assert_close(out[1].cpu(), O.equiv_embedding(_weights(C), 'e.', pts), 1e-5, '%s: equivariant embedding' % name)
        assert torch.equal(own[1], out[1])
        same = (pts[:, None, :] == pts[None, :, :]).all(-1)
        assert bool((out[1].cpu()[:, same][:, :, 1:] == 0).all()), 'coincident points must give the zero vector in channels 1..3'


@pytest.mark.parametrize('C', [32, 48])
def test_geometric_embedding_bf16_at_coincident_points(C):
    """The bf16 entry on `coincident`: bit for bit the f32 result rounded to nearest even -- the f32 result is held to the twin at 1e-4
    above -- and therefore within 1e-4 + 2^-8 of the float64 twin (bf16 keeps 8 significant bits: |rne(x) - x| <= 2^-8 |x|, half a unit in the
    last place)."""
    knn, want = _embedding_twin('coincident', C)
    e32, e16 = _embed('coincident', C, False, knn), _embed('coincident', C, False, knn, torch.bfloat16)
    assert e16.dtype == torch.bfloat16
    assert_close(e32.cpu(), want, 1e-4, 'f32')
    assert torch.equal(e16, e32.to(torch.bfloat16))
    assert rel_err(e16.float().cpu(), want) <= 1e-4 + 2.0 ** -8
    assert torch.equal(_embed('coincident', C, False, None, torch.bfloat16), e16)


# ---- superpoint scores ------------------------------------------------------------------------------------------------------------------
def _unit_features(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(7, C, generator=g)
    return torch.nn.functional.normalize(torch.randn(rows, C, generator=g) + base[torch.randint(0, 7, (rows,), generator=g)], dim=1)


@pytest.mark.parametrize('N,M', [(1, 1), (1, 65), (65, 1), (64, 257), (9, 40)])
def test_superpoint_scores_smallest_shapes_equal_the_float64_restatement(N, M):
    """One row, one column, M > 256 (a thread strides to a second column) and N = 9 (a second workgroup of eight rows holding one row),
    each at C = 32, at the smallest C, at C > 1024 (one row per workgroup) and without the dual normalisation (raw scores: the single
    form launches no normalise kernel).  The single form takes ref and src features from two allocations; the stack form, with every
    node present, takes them from one array and gives the same bit for bit."""
    from se3et_amd import ops
    for C, dual in ((32, True), (4, True), (1028, True), (32, False)):
        f = _unit_features(N + M, C, 90 + N + M)
        want = T.superpoint_scores(f[:N].numpy(), f[N:].numpy(), dual=dual)
        ref, src = f[:N].clone().cuda(), f[N:].clone().cuda()
        assert ref.untyped_storage().data_ptr() != src.untyped_storage().data_ptr()
        got = ops.superpoint_scores(ref, src, dual).cpu()
        assert_close(got, want, 1e-4, 'superpoint scores (%d, %d), C %d, dual %s' % (N, M, C, dual))
        S = ops.superpoint_scores_stack(f.cuda(), torch.ones(N + M, dtype=torch.bool).cuda(), [0], [N], [N], [M], [0], [N], dual).cpu()
        assert S.shape == (1, N * M)
        assert_close(S.view(N, M), want, 1e-4, 'stack form (%d, %d), C %d, dual %s' % (N, M, C, dual))
        assert torch.equal(S.view(N, M), got), 'single and stack form differ (%d, %d), C %d, dual %s' % (N, M, C, dual)


def test_superpoint_scores_stack_with_masked_rows_and_blocks():
    """A pair in which all but one ref node is absent and a pair with one fully absent block of 8 ref rows (the kernel's rows per
    workgroup), some src nodes absent in both: present entries against the float64 restatement, absent ones exactly -1, no NaN anywhere
    in the padded rows."""
    from se3et_amd import ops
    C = 32
    Ns, Ms = [9, 20], [70, 5]
    f = _unit_features(sum(Ns) + sum(Ms), C, 97)
    ref_rows, src_rows = [0, 9 + 70], [9, 9 + 70 + 20]
    masks = torch.ones(sum(Ns) + sum(Ms), dtype=torch.bool)
    ref_off, src_off = ref_rows, src_rows                     # the node masks are laid out like the feature rows
    masks[0:9] = False
    masks[4] = True                                            # pair 0: only ref node 4
    masks[9 + 3], masks[9 + 69] = False, False
    masks[79 + 8:79 + 16] = False                             # pair 1: ref rows 8 .. 15
    masks[99 + 4] = False
    S = ops.superpoint_scores_stack(f.cuda(), masks.cuda(), ref_rows, src_rows, Ns, Ms, ref_off, src_off, True).cpu()
    assert S.shape == (2, 630) and not bool(torch.isnan(S).any())
    for p, (n, m) in enumerate(zip(Ns, Ms)):
        rm, sm = masks[ref_off[p]:ref_off[p] + n].numpy(), masks[src_off[p]:src_off[p] + m].numpy()
        want = T.superpoint_scores(f[ref_rows[p]:ref_rows[p] + n].numpy(), f[src_rows[p]:src_rows[p] + m].numpy(), rm, sm)
        got = S[p, :n * m].view(n, m).numpy()
        present = rm[:, None] & sm[None, :]
        assert present.any() and (got[~present] == -1).all() and bool((S[p, n * m:] == -1).all()), 'pair %d: absent entries' % p
        assert_close(got[present], want[present], 1e-4, 'pair %d' % p)
