"""CPU: the twins and crafted cases of tests/vgtk_twin.py, which tests/test_gpu_vgtk_edges.py holds the EPN toolkit kernels to.

  * every twin equals oracle/vgtk_oracle.py and the stored tests/golden/vgtk_ops.npz on their own cases; the literal reduction tree of
    furthest point sampling equals the oracle's selection key on every case (the first check of that equivalence: the key `k mod bs
    ascending` that kernel and oracle shared until now does not survive it, the bit-reversed one does);
  * every input condition that a case states holds;
  * every allowance is usable (the float32 restatement lies inside it) and not vacuous (deliberately wrong restatements lie outside it or
    change an integer);
  * a host emulation of the schedule of the gather backward before its passes were made uniform (a wave left after its own last pass
    and staged no further index chunk) gets the cases wrong that the case list was built around, and the others right."""
import numpy as np
import pytest
import torch

import vgtk_twin as T

F32 = np.float32


def _oracle():
    from oracle import vgtk_oracle as VO
    return VO


def _exact_f32(v):
    return np.array_equal(np.asarray(v, np.float64), np.asarray(v, np.float64).astype(F32).astype(np.float64))


# ---- twins against the oracle and the fixture -----------------------------------------------------------------------------------------
def test_twins_equal_the_reference_fixture(golden_dir):
    g = np.load(golden_dir + '/vgtk_ops.npz')
    assert np.array_equal(T.gather_fwd(g['points'], g['gather_idx']), g['gathered'])
    idx = g['inter_idx']
    b, p, nn_ = idx.shape
    na, ks = g['inter_w'].shape[2], g['inter_w'].shape[3]
    full = np.ascontiguousarray(np.broadcast_to(idx[:, :, None, None, :], (b, p, na, ks, nn_)))
    ref = T._zp_reference(T.inter_fwd_t, full, g['inter_w'], g['feats'], g['cotangent'])
    assert T.rel_to_largest(ref['out'], g['inter_out']) < 1e-6 and T.rel_to_largest(ref['grad'], g['feats_grad']) < 1e-6
    ref = T._zp_reference(T.intra_fwd_t, g['intra_idx'], g['intra_w'], g['intra_feats'], g['intra_cotangent'])
    assert T.rel_to_largest(ref['out'], g['intra_out']) < 1e-6 and T.rel_to_largest(ref['grad'], g['intra_feats_grad']) < 1e-6
    # the float32 restatements on the fixture
    o, gr = T.inter_f32(full, g['inter_w'], g['feats'], g['cotangent'])
    assert T.rel_to_largest(o, g['inter_out']) < 1e-6 and T.rel_to_largest(gr, g['feats_grad']) < 1e-6
    o, gr = T.intra_f32(g['intra_idx'], g['intra_w'], g['intra_feats'], g['intra_cotangent'])
    assert T.rel_to_largest(o, g['intra_out']) < 1e-6 and T.rel_to_largest(gr, g['intra_feats_grad']) < 1e-6


def test_ball_query_twin_equals_the_oracle():
    VO = _oracle()
    for c in T.ball_cases():
        assert np.array_equal(c['want'], VO.ball_query(c['query'], c['support'], c['radius'], c['nsample'])), c['name']


@pytest.mark.parametrize('n', T.FPS_N)
def test_literal_fps_tree_equals_the_oracle_key(n):
    VO = _oracle()
    for m in T.fps_samples(n):
        c = T.fps_case(n, m)
        assert np.array_equal(c['want'], VO.furthest_point_sampling(c['pc'], m)), c['name']


def test_zpconv_and_anchor_twins_equal_the_oracle():
    VO = _oracle()
    for name in T.INTRA_SHAPES:
        c = T.intra_case(name)
        assert T.rel_to_largest(VO.intra_zpconv(c['nbr'], c['w'], c['feats']), c['out']) < 1e-5, name
    for name in T.ANCHOR_SHAPES:
        c = T.anchor_case(name)
        assert T.rel_to_largest(VO.anchor_query(c['xyz'], c['anchors'], c['kp']), c['want']) < 1e-5, name
    for name in T.INITIAL_SHAPES:
        c = T.initial_case(name)
        w, n = VO.initial_anchor_query(c['centers'], c['xyz'], c['kp'], c['radius'], c['sigma'])
        assert np.array_equal(n.astype(np.int64), c['want_n']), name
        assert T.rel_to_largest(w, c['want_w']) < 1e-5, name


# ---- the stated input conditions --------------------------------------------------------------------------------------------------------
def test_gather_cases_hold_their_claims():
    shapes = T.gather_shapes()
    assert {s[0] for s in shapes if s[1:] == (65, 4097)} == set(T.GATHER_C)
    for c in (3, 34):
        assert {s[2] for s in shapes if s[:2] == (c, 65)} >= set(T.GATHER_M)
    assert {s[1] for s in shapes if s[0] == 3 and s[2] == 4097} >= set(T.GATHER_N)
    classes = set()
    for s in shapes:
        trips = T.gather_wave_trips(s[0])
        for pattern in T.GATHER_PATTERNS:
            c = T.gather_case(*s, pattern)
            assert c['uniform_trips'] == (len(set(trips)) == 1), c['name']
            assert c['idx'].shape == (2, s[2]) and (s[2] == 0 or (0 <= c['idx'].min() and c['idx'].max() < s[1]))
            assert s[2] < 2 or s[1] < 2 or not np.array_equal(c['idx'][0], c['idx'][1])
            if pattern == 'one':
                assert all(len(set(r.tolist())) <= 1 for r in c['idx'])
            if pattern == 'sparse' and s[1] > 64 and s[2]:
                assert 0 in c['empty_workgroups'][0] and 1 in c['empty_workgroups'][1], c['name']
                for bi, e in enumerate(c['empty_workgroups']):
                    for w in e:
                        assert not c['bwd32'][bi, :, 64 * w:64 * w + 64].any() and not c['allowed'][bi, :, 64 * w:64 * w + 64].any()
            assert np.all(np.abs(c['bwd32'] - c['bwd64']) <= c['allowed']), c['name']          # the allowance is usable
        classes.add((len(set(trips)) == 1, min(-(-s[2] // 2048), 2)))
    assert classes >= {(False, 1), (False, 2), (True, 2)}
    assert T.gather_case(3, 130, 4097, 'sparse')['empty_workgroups'] == [[0, 2], [1, 2]]


def test_ball_cases_hold_their_claims():
    seen = {}
    for c in T.ball_cases():
        q, s, ns = c['query'].astype(np.float64), c['support'].astype(np.float64), c['nsample']
        for a in (q, s):
            assert np.array_equal(a * 4, np.round(a * 4)) and np.abs(a).max() <= 64, c['name']
        r2 = c['radius'] ** 2
        for bi in range(2):
            assert not np.array_equal(q[0], q[1]) or c['m'] == 0
            for j in range(c['m']):
                d2 = ((q[bi, :, j, None] - s[bi]) ** 2).sum(0)
                d32 = c['query'][bi, :, j, None] - c['support'][bi]
                d32 = (d32[0] * d32[0] + d32[1] * d32[1]) + d32[2] * d32[2]
                assert d32.dtype == F32 and np.array_equal(d32.astype(np.float64), d2), c['name']     # exact in float32
                assert np.all((d2 == r2) | (np.abs(d2 - r2) >= 1 / 16)), c['name']
                assert np.nonzero(d2 < r2)[0].tolist() == c['hits'][bi][j] and c['total'][bi, j] == len(c['hits'][bi][j])
                assert np.nonzero(d2 == r2)[0].tolist() == sorted(c['edges'][bi][j])
                seen.setdefault(ns, set()).add(len(c['hits'][bi][j]))
    assert seen[8] >= {0, 1, 6, 7, 8, 9} and seen[64] >= {0, 1, 62, 63} and seen[65] >= {0, 1, 63, 64, 65} and seen[2] >= {0, 1, 2, 3}
    assert seen[1] >= {0, 1, 2}
    by = {c['name']: c for c in T.ball_cases()}
    assert {(c['n'], c['nsample']) for c in T.ball_cases()} >= {(n, k) for n in (1, 63, 64, 65, 128, 129) for k in (1, 2, 8, 64, 65)}
    assert {c['m'] for c in T.ball_cases()} >= {1, 3, 4, 5}
    h = by['ball cut-off at 63']['hits']
    assert h[0][0][7] == 63 and max(h[0][0]) > 63 and h[1][0][7] == 63 and h[1][0][8] == 64
    h = by['ball cut-off at 64']['hits']
    assert h[0][0][7] == 64 and h[0][0][8:] == [65, 70, 127] and h[1][0][7] == 64 and by['ball cut-off at 64']['edges'][0][0] == [63]
    h = by['ball cut-off mid-round']['hits']
    assert h[0][0][7] == 20 and h[0][0][8:] == [21, 40, 64] and len(h[1][0]) == 9
    assert sorted(map(len, by['ball hit classes nsample=8']['hits'][0])) == [0, 1, 6, 7, 8, 9]


def test_fps_cases_hold_their_claims():
    for n in T.FPS_N:
        pc = T.fps_cloud(n).astype(np.float64)
        assert np.array_equal(pc, np.round(pc)) and pc.shape == (3, 3, n)
        mag = (pc * pc).sum(1)
        assert np.all((mag == 0) | (mag >= 1 / 16))
        assert mag[0, 0] == 0 and ((mag[0] == 0).sum() >= 2 or n < 4) and mag[1, 0] > 0 and not mag[2].any()
        assert n < 3 or ((mag[0] > 0).any() and not np.array_equal(pc[0], pc[1]))
        assert sorted({1, 2, n - 1, n + 5} - {0}) == T.fps_samples(n) or n == 2
        for m in T.fps_samples(n):
            want = T.fps_case(n, m)['want']
            assert want.shape == (3, m) and not want[:, 0].any() and not want[2].any()
            assert not (mag[0][want[0, 1:]] == 0).any() or not (mag[0] > 0).any()        # a point at the origin is never selected
    lattice = T.fps_cloud(1331)[0].astype(np.int64)
    moved = int((lattice == 0).all(0).sum()) - 1                                   # lattice points that were put at the origin too
    assert len({tuple(v) for v in lattice.T}) == 1331 - moved and moved >= 1 and lattice.min() == -5 and lattice.max() == 5
    assert T.fps_block_size(2049) == 1024 and T.fps_block_size(63) == 32 and T.fps_block_size(3) == 2 and T.fps_block_size(1) == 1


def test_zpconv_cases_hold_their_claims():
    assert {T.inter_case(n)['outputs'] for n in T.INTER_SHAPES} >= {255, 256, 257}
    assert {T.inter_case(n)['targets'] for n in T.INTER_SHAPES} >= {63, 64, 65}
    one = T.inter_case('inter 257 outputs, 63 targets, ann=ks=na=c=1')
    assert one['idx'].shape[2:] == (1, 1, 1) and one['feats'].shape[1] == 1
    assert T.inter_case('inter nq=1')['feats'].shape[2] == 1
    for name in T.INTER_SHAPES:
        c = T.inter_case(name)
        assert (c['w'] == 0).any() and (c['w'] > 0).any() and (c['w'] < 0).any() and not np.array_equal(c['idx'][0], c['idx'][1]) or name == 'inter nq=1'
        if c['feats'].shape[2] > 1:
            row = np.abs(c['feats']).max(axis=(0, 1, 3))
            assert row[-1] / row[0] > 1e4
        if c['pattern'] == 'one':
            for bi in range(2):
                q = int(c['idx'][bi].flat[0])
                assert (c['idx'][bi] == q).all()
                others = np.delete(c['grad'][bi], q, axis=1)
                assert not others.any() and not np.delete(c['grad_allowed'][bi], q, axis=1).any()
                assert c['grad_terms'][bi][:, q].min() == c['idx'][bi].size / c['idx'].shape[2]
    shapes = [(T.intra_case(n)['nbr'].shape[0], T.intra_case(n)['feats'].shape[3]) for n in T.INTRA_SHAPES]
    assert (7, 5) in shapes and (5, 7) in shapes
    assert {T.intra_case(n)['outputs'] for n in T.INTRA_SHAPES} >= {255, 256, 257}
    assert {T.intra_case(n)['gradients'] for n in T.INTRA_SHAPES} >= {255, 256, 257}
    assert any(T.intra_case(n)['nbr'].shape[1] == 1 for n in T.INTRA_SHAPES)
    for name in T.INTRA_SHAPES:
        c = T.intra_case(name)
        if c['feats'].shape[3] > 1:
            assert c['unreferenced'] == [c['feats'].shape[3] - 1], name
            assert not c['grad'][..., c['unreferenced'][0]].any() and not c['grad_allowed'][..., c['unreferenced'][0]].any()
        if c['nbr'].shape[1] > 1:
            assert 0 in c['by_all'], name


def test_anchor_cases_hold_their_claims():
    assert {int(np.prod(T.anchor_case(n)['xyz'].shape[2:])) for n in T.ANCHOR_SHAPES} >= {255, 256, 257}
    for name in T.ANCHOR_SHAPES:
        c = T.anchor_case(name)
        x, a = c['xyz'].astype(np.float64), c['anchors'].astype(np.float64)
        norm = np.sqrt((x * x).sum(1))
        ratio = np.abs(np.einsum('bdpn,ad->bpan', x, a)) / np.maximum(norm, 1e-300)[:, :, None, :]
        assert ratio.max() <= 0.99 and c['zero'].any() and not norm[c['zero']].any(), name
        assert np.isfinite(T.anchor_query_f32(c['xyz'], c['anchors'], c['kp'])[0]).all()
    p = T.anchor_parallel_case()
    x = p['xyz'].astype(np.float64)
    for pi, s in enumerate(T.PARALLEL_NORMS):
        for ni in range(6):
            assert np.array_equal(x[0, :, pi, ni], p['anchors'][ni].astype(np.float64) * float(F32(s)))
            assert np.array_equal(x[1, :, pi, ni], -x[0, :, pi, ni])
    rows = np.nonzero(p['nan_allowed'].any(axis=(0, 2, 3, 4)))[0].tolist()
    assert rows == list(T.PARALLEL_NAN_ROWS)                       # a NaN is accepted in the |x| = 100 rows alone
    assert np.array_equal(p['nan_allowed'][:, :, :, 0, :], np.abs(p['ratio32']) >= F32(1 - 2.0 ** -22))
    got, _ = T.anchor_query_f32(p['xyz'], p['anchors'], p['kp'])
    assert np.all(((got >= p['lo']) & (got <= p['hi'])) | (p['nan_allowed'] & np.isnan(got)))
    assert np.all((p['want'] >= p['lo']) & (p['want'] <= p['hi']))
    # not vacuous: the spread is narrow against the values where acos is well conditioned, and a wrong angle leaves it
    wide = (p['hi'] - p['lo']) / np.maximum(p['hi'], 1e-300)
    assert wide[:, 0][..., 1:5].max() < 1e-4
    wrong = T.anchor_query_from_ratio(*[(r * 0.999, n) for r, n in [T.anchor_ratio(p['xyz'], p['anchors'])]][0], p['kp'])
    assert ((wrong < p['lo']) | (wrong > p['hi'])).any(axis=(2, 3, 4)).all()


def test_initial_anchor_cases_hold_their_claims():
    assert {int(np.prod(T.initial_case(n)['want_w'].shape[1:])) for n in T.INITIAL_SHAPES} == {255, 256, 257}
    for name in T.INITIAL_SHAPES:
        c = T.initial_case(name)
        ct, x = c['centers'].astype(np.float64), c['xyz'].astype(np.float64)
        assert not np.array_equal(ct[0], ct[1])
        on = 0
        for bi in range(2):
            d2 = ((ct[bi].T[:, None, :] - x[None]) ** 2).sum(-1)
            d = np.sqrt(d2)
            near = d < c['radius'] + 1
            assert _exact_f32(d2) and _exact_f32(d[near]) and np.array_equal(d[near] ** 2, d2[near]), name      # exact distances
            assert np.all((d == c['radius']) | (np.abs(d - c['radius']) >= 1 / 16)), name
            on += int((d == c['radius']).sum())
            assert (d < c['radius']).any() and (near & (d > c['radius'])).any()
        assert on >= 2, name
        k, pn, a = c['zero_weight_at']
        e = c['kp'][k, a].astype(np.float64)[:, None] + ct[0][:, pn, None] - x.T
        d2k = (e * e).sum(0)
        counted = ((ct[0][:, pn, None] - x.T) ** 2).sum(0) <= c['radius'] ** 2
        assert (counted & (d2k == c['sigma'])).sum() == 1 and c['want_n'][0, k, pn, a] == counted.sum()
        assert c['want_w'].max() > 0 and (c['want_w'] == 0).any() and c['want_n'].max() >= 3
    assert not T.initial_anchor_query(T.initial_case('initial 255 outputs')['centers'], np.zeros((0, 3), F32),
                                      T.initial_case('initial 255 outputs')['kp'], 1.25, 1.5625)[0].any()


# ---- the allowances: usable and not vacuous -------------------------------------------------------------------------------------------------
def _outside(got, want, allowed):
    return bool(np.any(np.abs(np.asarray(got, np.float64) - want) > allowed))


def test_gather_allowance_rejects_a_stale_quarter_of_the_stage():
    """The defect's shape as a mutant: in every chunk after the first, the slots of one wave (a quarter) keep the previous chunk's indices."""
    for s in [(3, 65, 4097), (34, 65, 6145), (67, 65, 4097), (3, 130, 4097)]:
        c = T.gather_case(*s, 'uniform')
        j = np.arange(s[2])
        stale = (j >= 2048) & (((j % 2048) % 256) >> 6 == 3)
        idx = c['idx'].copy()
        idx[:, stale] = c['idx'][:, j[stale] - 2048]
        wrong = T.gather_bwd_f32_in_order(c['cot'], idx, s[1])
        assert _outside(wrong, c['bwd64'], c['allowed']) and not np.array_equal(wrong, c['bwd32']), c['name']
    c = T.gather_case(34, 65, 4097, 'uniform')
    off = T.gather_bwd_f32_in_order(c['cot'], ((c['idx'] + 1) % 65).astype(np.int32), 65)              # one target further
    assert _outside(off, c['bwd64'], c['allowed'])
    rev = T.gather_bwd_f32_in_order(c['cot'][:, :, ::-1], c['idx'][:, ::-1], 65)                         # descending j: inside, other bits
    assert not _outside(rev, c['bwd64'], c['allowed']) and not np.array_equal(rev, c['bwd32'])


def test_ball_query_mutants_change_an_index():
    def mutant(c, le=False, copy_last=False):
        q, s, ns = c['query'].astype(np.float64), c['support'].astype(np.float64), c['nsample']
        out = np.zeros((2, c['m'], ns), np.int32)
        for bi in range(2):
            for j in range(c['m']):
                d2 = ((q[bi, :, j, None] - s[bi]) ** 2).sum(0)
                f = np.nonzero(d2 <= c['radius'] ** 2 if le else d2 < c['radius'] ** 2)[0][:ns]
                if len(f) and (len(f) < ns - 1 or (copy_last and len(f) == ns - 1)):
                    out[bi, j] = f[np.arange(ns) % len(f)]
                else:
                    out[bi, j, :len(f)] = f
        return out
    changed_le = changed_last = 0
    for c in T.ball_cases():
        assert np.array_equal(mutant(c), c['want'])
        changed_le += not np.array_equal(mutant(c, le=True), c['want'])
        changed_last += not np.array_equal(mutant(c, copy_last=True), c['want'])
    assert changed_le >= 10 and changed_last >= 5
    for name in ('ball cut-off at 63', 'ball cut-off at 64', 'ball cut-off mid-round'):
        c = [k for k in T.ball_cases() if k['name'] == name][0]
        assert not np.array_equal(mutant(c, le=True), c['want'])


def test_fps_mutants_change_an_index():
    higher = by_k = 0
    for n in T.FPS_N:
        m = T.fps_samples(n)[-2]
        c = T.fps_case(n, m)
        higher += not np.array_equal(T.furthest_point_sampling(c['pc'], m, ties_to_higher=True), c['want'])
        if n > T.fps_block_size(n) and n >= 63:
            assert not np.array_equal(T.furthest_point_sampling(c['pc'], m, key_by_k=True), c['want']), c['name']
            by_k += 1
    assert higher >= len(T.FPS_N) - 2 and by_k >= 6
    # the key that kernel and oracle shared before this check existed -- lower thread first -- is not the tree's: threads 1 and 2 tied
    pc = np.zeros((1, 3, 4), F32)
    pc[0, :, 0], pc[0, :, 1], pc[0, :, 2], pc[0, :, 3] = (1, 0, 0), (1, 2, 0), (1, -2, 0), (1, 1, 0)
    assert T.furthest_point_sampling(pc, 2).tolist() == [[0, 2]]


def test_zpconv_allowances_are_usable_and_not_vacuous():
    for name in T.INTER_SHAPES:
        c = T.inter_case(name)
        o, g = T.inter_f32(c['idx'], c['w'], c['feats'], c['cot'])
        assert not _outside(o, c['out'], c['out_allowed']) and not _outside(g, c['grad'], c['grad_allowed']), name
        if c['idx'].shape[-1] > 1:
            o, g = T.inter_f32(c['idx'], c['w'], c['feats'], c['cot'], drop_last=True)
            assert _outside(o, c['out'], c['out_allowed']) and _outside(g, c['grad'], c['grad_allowed']), name
        if c['feats'].shape[2] > 1:
            o, g = T.inter_f32(c['idx'], c['w'], c['feats'], c['cot'], shift=1)
            assert _outside(o, c['out'], c['out_allowed']) and _outside(g, c['grad'], c['grad_allowed']), name
    for name in T.INTRA_SHAPES:
        c = T.intra_case(name)
        o, g = T.intra_f32(c['nbr'], c['w'], c['feats'], c['cot'])
        assert not _outside(o, c['out'], c['out_allowed']) and not _outside(g, c['grad'], c['grad_allowed']), name
        if c['nbr'].shape[1] > 1:
            o, g = T.intra_f32(c['nbr'], c['w'], c['feats'], c['cot'], drop_last=True)
            assert _outside(o, c['out'], c['out_allowed']) and _outside(g, c['grad'], c['grad_allowed']), name
        if c['feats'].shape[3] > 1:
            o, g = T.intra_f32(c['nbr'], c['w'], c['feats'], c['cot'], shift=1)
            assert _outside(o, c['out'], c['out_allowed']) and _outside(g, c['grad'], c['grad_allowed']), name


def test_anchor_allowances_are_usable_and_not_vacuous():
    for name in T.ANCHOR_SHAPES:
        c = T.anchor_case(name)
        assert c['restatement'] <= c['allowed'] < 1e-4, name                     # the cap decides no case
        ratio, norm = T.anchor_ratio(c['xyz'], c['anchors'])
        assert T.rel_to_largest(T.anchor_query_from_ratio(ratio * (1 + 1e-4), norm, c['kp']), c['want']) > c['allowed'], name
    for name in T.INITIAL_SHAPES:
        c = T.initial_case(name)
        assert c['restatement'] <= c['allowed'] < 1e-4, name
        w, n = T.initial_anchor_query(c['centers'], c['xyz'], c['kp'], c['radius'], c['sigma'], strict=True)          # `<` for `<=`
        assert not np.array_equal(n, c['want_n']) and T.rel_to_largest(w, c['want_w']) > c['allowed'], name
        w32, n32 = T.initial_anchor_query_f32(c['centers'], c['xyz'], c['kp'], c['radius'], c['sigma'])
        assert np.array_equal(n32.astype(np.int64), c['want_n']), name


# ---- the schedule of the gather backward before its passes were uniform -----------------------------------------------------------------
def _parent_error(c, n, m, seed=0):
    g = np.random.default_rng(seed)
    idx = g.integers(0, n, (2, m)).astype(np.int32)
    cot = g.standard_normal((2, c, m)).astype(F32)
    got, unwritten = T.gather_bwd_parent_schedule(cot, idx, n)
    return float(np.abs(got - T.gather_bwd_f64(cot, idx, n)[0]).max()), unwritten


def test_the_earlier_gather_schedule_fails_the_cases_built_for_it():
    """A wave that made fewer passes left the kernel and staged no further chunk: its quarter of the stage kept the last chunk of the
    previous pass.  Figures of the issue that motivated the uniform passes (n = 64, normal cotangents): (c, m) = (3, 5000) 98.6,
    (34, 5000) 22.6, (35, 4097) 12.3 wrong; (37, 5000), (34, 2048), (33, 2049) exactly right -- the last two by luck."""
    for (c, m), quoted in {(3, 5000): 98.6, (34, 5000): 22.6, (35, 4097): 12.3}.items():
        err, _ = _parent_error(c, 64, m)
        print('parent schedule c=%d m=%d: max abs error %.1f (quoted %.1f)' % (c, m, err, quoted))
        assert quoted / 4 < err < quoted * 4
    for c, m in ((37, 5000), (34, 2048), (33, 2049)):
        assert _parent_error(c, 64, m) == (0.0, False)
    wrong, right = [], []
    for s in T.gather_shapes():
        case = T.gather_case(*s, 'uniform')
        got, unwritten = T.gather_bwd_parent_schedule(case['cot'], case['idx'], s[1])
        bad = bool(np.any(np.abs(got - case['bwd64']) > case['allowed']))
        (wrong if bad else right).append(s)
        if case['uniform_trips']:
            assert not bad and not unwritten, case['name']
        elif s[2] >= 4097 and s[1] > 1:                  # (one target: a stale index is the same index)
            assert bad, case['name']
        if s[0] < 4 and s[2] > 192:
            assert unwritten, case['name']               # a wave that never runs never stages: those slots are read as they were found
    assert {(c, 65, 4097) for c in (1, 2, 3, 33, 34, 35, 65, 67)} <= set(wrong)
    assert {(c, 65, 4097) for c in (4, 5, 31, 32, 36, 64)} <= set(right) and (34, 65, 2048) in right and (34, 65, 2047) in right
    print('wrong under the earlier schedule:', wrong)


def test_the_uniform_schedule_as_emulated_is_right():
    """The same emulation with every wave making ceil(c / 32) passes: all slots staged in every chunk."""
    for s in [(3, 65, 4097), (34, 65, 6145), (35, 65, 4097)]:
        case = T.gather_case(*s, 'uniform')
        padded = np.concatenate([case['cot'], np.zeros((2, -s[0] % 32, s[2]), F32)], 1)        # c a multiple of 32: equal trips
        got, unwritten = T.gather_bwd_parent_schedule(padded, case['idx'], s[1])
        assert not unwritten and np.array_equal(got[:, :s[0]], T.gather_bwd_parent_schedule(padded, case['idx'], s[1])[0][:, :s[0]])
        assert np.all(np.abs(got[:, :s[0]] - case['bwd64']) <= case['allowed'])
