"""CPU: pins the float64 twin of the KPConvInterSO3 forward (tests/kpconv_twin.py), its judge and the cases that
tests/test_gpu_kpconv_edges.py runs the kernels on, so that a failure on the GPU can be trusted: the twin against the oracle, the float32
restatement, the reference fixture and a brute-force loop; the judge against three planted kernel faults that the whole-tensor figure of
the older tests lets through; and every crafted case against the valid counts it claims."""
import numpy as np
import pytest
import torch

import kpconv_twin as T
from helpers import rel_err

OLD_GLOBAL = 2e-6             # the whole-tensor bound of tests/test_gpu_ops.py::test_fused_kpconv_edge_shapes


def _text(figures):
    return '   '.join('%s %.2e (restatement %.2e, allowed %.2e)' % f for f in figures)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P,Ns,NN,Cin,Cout,seed', [(37, 64, 12, 8, 32, 1), (50, 80, 38, 24, 16, 2)])
def test_twin_matches_the_oracle_and_the_restatement(P, Ns, NN, Cin, Cout, seed):
    from oracle import se3et_oracle as O
    case = T.geometric(P, Ns, NN, Cin, Cout, 0.08, seed)
    want = T.twin(case)
    assert want.dtype == T.F64 and want.shape == (P, 6, Cout)
    st = {'c.kernel_points': case['kernel_points'], 'c.weights': case['weights'], 'c.kidx_rot': case['kidx'][:, None, :].expand(-1, 6, -1),
          'c.ridx_rot': case['ridx'][None].expand(15, -1, -1)}
    oracle = O.kpconv_inter_so3(st, 'c.', case['q_pts'], case['s_pts'], case['idx'], case['x'], case['sigma'])
    assert rel_err(oracle, want) <= 2e-6
    assert rel_err(T.restatement(case), want) <= 2e-6
    # the twin on float64 inputs is the restatement on float64 inputs: one formula
    both = T.AG.kpconv_inter_so3(*[t.double() if torch.is_tensor(t) and t.is_floating_point() else t for t in T.args(case)])
    assert rel_err(both, want) <= 1e-12


def test_twin_matches_the_reference_fixture(golden_dir):
    g = np.load(golden_dir + '/micro_se3ete.npz')
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('sd/')}
    for name, blk, sigma in (('kpconv_2_2', 'encoder2_2', 0.1), ('kpconv_2_1', 'encoder2_1', 0.05)):
        q, s, idx, x = [torch.from_numpy(g['op/%s/in%d' % (name, i)]) for i in range(4)]
        pre = 'backbone.%s.interso3.conv.' % blk
        got = T.forward(x, q, s, idx.long(), sd[pre + 'kernel_points'], sd[pre + 'weights'], sd[pre + 'kidx_rot'][:, 0, :],
                        sd[pre + 'ridx_rot'][0], sigma)
        assert rel_err(got, torch.from_numpy(g['op/%s/out0' % name])) <= 2e-6, name


def test_twin_matches_a_brute_force_loop():
    """Five points: a repeated row, an index below 0 and one above Ns (both the shadow), an empty list."""
    Ns, NN, Cin, Cout = 7, 4, 2, 3
    case = T.craft([3, 4, 0, 2, 1], NN, Ns, Cin, Cout, seed=5, lists=[[2, 5, 2], [0, 1, 3, 6], [], [4, 4], [6]])
    idx = case['idx'].clone()
    shadow = (idx[0] == Ns).nonzero()[0]
    idx[0, shadow] = -3                                   # below the range
    free = (idx[3] == Ns).nonzero()
    idx[3, free[0]] = Ns + 5                              # above it
    case['idx'] = idx
    assert T.valid_counts(case).tolist() == [3, 4, 0, 2, 1]
    x, q, s, kp, W = [case[n].double() for n in ('x', 'q_pts', 's_pts', 'kernel_points', 'weights')]
    kidx, ridx = case['kidx'], case['ridx']
    F = torch.zeros(5, 15, 6, Cin, dtype=T.F64)
    for p in range(5):
        for n in range(NN):
            j = int(idx[p, n])
            if j < 0 or j >= Ns:
                continue
            for k in range(15):
                w = max(0.0, 1.0 - float((s[j] - q[p] - kp[k]).norm()) / case['sigma'])
                F[p, k] += w * x[j]
    want = torch.zeros(5, 6, Cout, dtype=T.F64)
    for p in range(5):
        for r in range(6):
            for k in range(15):
                for a in range(6):
                    want[p, r] += F[p, k, a] @ W[int(kidx[k, r]), int(ridx[a, r])]
    got = T.twin(case)
    assert rel_err(got, want) <= 1e-12
    assert float(got[2].abs().max()) == 0.0               # the empty list
    assert float(got[3].abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# the judge
# ---------------------------------------------------------------------------------------------------------------------------------------
def _private_lists(counts, Ns):
    """Point 0's rows are its own (shrink_point needs that); the others share the rest."""
    g = torch.Generator().manual_seed(3)
    lists = [list(range(counts[0]))]
    for c in counts[1:]:
        lists.append((counts[0] + torch.randperm(Ns - counts[0], generator=g)[:c]).tolist())
    return lists


def _planted(case, faulty):
    """-> the figures of `faulty` (the output of a modelled kernel mistake, float64) on `case`; the mistake must pass the old whole-tensor
    bound and be rejected per row."""
    want, rest = T.twin(case), T.restatement(case)
    assert not T.rejected(T.check(rest, want, rest))      # the honest float32 answer passes
    figures = T.check(faulty, want, rest)
    print(_text(figures))
    (_, g_err, _, _), (_, r_err, _, r_allowed) = figures
    assert g_err <= OLD_GLOBAL, 'the planted fault must pass the old bound: %s' % _text(figures)
    assert r_err > r_allowed and T.rejected(figures), 'the judge must catch it: %s' % _text(figures)


def test_judge_catches_a_scaled_row_of_a_one_neighbour_point():
    """The rows of a 1-neighbour point times 1.01 in a tensor that also holds 64-neighbour points."""
    counts = [1] + [64] * 7
    case = T.craft(counts, 64, 96, 8, 32, seed=21, lists=_private_lists(counts, 96))
    case = T.shrink_point(case, 0, 1e-4)
    faulty = T.twin(case)
    faulty[0] *= 1.01
    _planted(case, faulty)


def test_judge_catches_the_dropped_tail_pair():
    """Valid neighbours 32 and 33 of a 34-neighbour point dropped: the tail slot pair of the EXT rounds."""
    counts = [34] + [64] * 7
    case = T.craft(counts, 64, 128, 8, 32, seed=22, lists=_private_lists(counts, 128))
    case = T.shrink_point(case, 0, 5e-6)
    Ns = 128
    idx = case['idx'].clone()
    slots = ((idx[0] >= 0) & (idx[0] < Ns)).nonzero().flatten()
    assert slots.numel() == 34
    idx[0, slots[32:]] = Ns                               # compacted entries 32 and 33
    faulty = T.twin(dict(case, idx=idx))
    _planted(case, faulty)


def test_judge_catches_a_dropped_repeat():
    """A row named twice, counted once."""
    counts = [9] + [64] * 7
    lists = _private_lists(counts, 96)
    lists[0][8] = lists[0][2]
    case = T.craft(counts, 64, 96, 8, 32, seed=23, lists=lists)
    case = T.shrink_point(case, 0, 1e-5)
    idx = case['idx'].clone()
    twice = (idx[0] == lists[0][2]).nonzero().flatten()
    assert twice.numel() == 2
    idx[0, twice[1]] = 96
    faulty = T.twin(dict(case, idx=idx))
    _planted(case, faulty)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_every_gpu_case_is_present():
    assert len(T.CASES) == 40 + 7 + 6 + 5 + 1 + 6 + 1 + 8


@pytest.mark.parametrize('name', list(T.CASES))
def test_crafted_case_holds_what_it_claims(name):
    """The valid counts are the claimed ones, and the float32 restatement alone stays within 1e-4 / 16 of the twin in both figures: the
    min(1e-4, ...) cap is never what decides a case."""
    case = T.case(name)
    assert T.valid_counts(case).tolist() == case['counts']
    Ns, NN = case['s_pts'].shape[0], case['idx'].shape[1]
    assert NN <= 64 and Ns <= 1200
    figures = T.check(case['restatement'], case['twin'], case['restatement'])
    print(name, _text(figures))
    for _, _, r, a in figures:
        assert r <= T.CEILING / T.FACTOR and a < T.CEILING, _text(figures)
    if name.startswith('magnitude') or name == 'row 0 large':
        return
    idx = case['idx']
    for p, c in enumerate(case['counts']):                # with a shadow entry in the list, slot 0 holds one: the compaction has to move entries
        if c < NN:
            assert int(idx[p, 0]) == Ns
    if 'on' in case['placed']:
        p, row, k = case['placed']['on']
        assert row in idx[p].tolist()
        assert float((case['s_pts'][row] - case['q_pts'][p] - case['kernel_points'][k]).norm()) <= 1e-8
    if 'far' in case['placed']:
        p, row = case['placed']['far']
        assert row in idx[p].tolist()
        d = (case['s_pts'][row] - case['q_pts'][p] - case['kernel_points']).norm(dim=-1)
        assert float(d.min()) > case['sigma']


def test_ladder_counts_and_weights():
    """The ladder puts points exactly on every count of {0, 1, 7, 8, 9, 31, 32, 33, 39, 40, 41, 63, 64} that the list length allows, and
    most weights of the crafted geometry are non-zero."""
    case = T.case('ladder NN 64 (16, 64)')
    assert set(case['counts']) == set(T.LADDER)
    assert set(T.case('ladder NN 33 (16, 64)')['counts']) == {0, 1, 7, 8, 9, 31, 32, 33}
    Ns = case['s_pts'].shape[0]
    idx = case['idx']
    nb = torch.cat((case['s_pts'], torch.full((1, 3), 1e6)))[idx] - case['q_pts'][:, None]
    w = (1 - (nb[:, :, None] - case['kernel_points']).norm(dim=-1) / case['sigma']).clamp(min=0)
    live = (w.sum(-1) > 0)[idx < Ns]
    assert float(live.double().mean()) > 0.5
    # the row-scale spread the per-row figure is there for: a 1-neighbour point far below a 64-neighbour one
    top = case['twin'].abs().amax((1, 2))
    counts = torch.tensor(case['counts'])
    assert float(top[counts == 1].max()) < 0.5 * float(top[counts == 64].max())


def test_union_plan_cases_have_the_unions_they_claim():
    """Distinct rows of the 16-point group: 128 (the cap), 129, 16 x 64 disjoint, 64 shared."""
    distinct = lambda name: len(set(T.case(name)['idx'].flatten().tolist()) - {T.case(name)['s_pts'].shape[0]})
    assert distinct('union cap') == 128 and distinct('union cap+1') == 129
    assert distinct('union disjoint64') == 1024 and distinct('union same64') == 64
    assert T.case('union clouds')['lens'] == [1, 16, 17, 31]
    rep = T.case('repeats')
    l0, l1 = rep['idx'][0].tolist(), rep['idx'][1].tolist()
    assert l0.count(3) == 2 and l1.count(40) == 3 and rep['counts'][1] == 40
