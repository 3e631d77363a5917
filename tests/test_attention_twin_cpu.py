"""CPU: pins the float64 twin of the forward attention kernels (tests/attention_twin.py) and the inputs that
tests/test_gpu_attention_edges.py runs the kernels on, so that a failure on the GPU can be trusted: the twin against the unfolded formula,
the oracle and the reference fixture; the stress kinds against the properties they are there for; and the error rule against modelled
kernel mistakes -- including one that the whole-tensor 1e-4 rule of helpers.assert_close lets through."""
import math

import numpy as np
import pytest
import torch

import attention_twin as T
from helpers import rel_err

F64 = T.F64


def _figures_text(figures):
    return '   '.join('%s %.2e (restatement %.2e, allowed %.2e)' % f for f in figures)


def _assert_accepted(got, want, restatement, name):
    figures = T.check(got, want, restatement)
    print(name, _figures_text(figures))
    assert not T.rejected(figures), '%s: %s' % (name, _figures_text(figures))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('A,N,M,C,H,eq', [(6, 33, 31, 64, 4, True), (1, 5, 65, 32, 4, False), (2, 7, 9, 64, 8, True)])
def test_rpe_logits_equal_the_unfolded_form(A, N, M, C, H, eq):
    """(W_p^T q).e = q.(W_p e + b_p) - q.b_p head by head: the folded form drops the bias term, which is constant along the keys."""
    case = T.attention_case(A, C, H, eq, seed=N + M, pair=(N, M))
    q, k, vt, emb, w_p, eq_emb, w_eq = T.pair_inputs(case)
    g = torch.Generator().manual_seed(1)
    b_p, b_eq = torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    d = C // H
    qh = q.reshape(A, N, H, d)
    p = (emb @ w_p.t() + b_p).reshape(N, M, H, d)
    want = torch.einsum('anhd,nmhd->ahnm', qh, p) - torch.einsum('anhd,hd->ahn', qh, b_p.reshape(H, d))[..., None]
    if eq:
        e = (eq_emb @ w_eq.t() + b_eq).reshape(A, N, M, H, d)
        want = want + torch.einsum('anhd,anmhd->ahnm', qh, e) - torch.einsum('anhd,hd->ahn', qh, b_eq.reshape(H, d))[..., None]
    got = T.rpe_logits(q, emb, w_p, eq_emb, w_eq, H)
    assert got.dtype == F64 and got.shape == (A * H, N, M)
    assert rel_err(got, want.reshape(A * H, N, M)) <= 1e-12


def test_scores_times_values_are_the_hidden_states():
    """rpe_scores (written out here) and autograd.rpe_attention (called with float64) are one softmax."""
    case = T.pair_case(64, 33, 31)
    hidden, scores = T.pair_attention(case)
    q, k, vt, *_ = T.pair_inputs(case)
    v = vt[..., :31].transpose(1, 2).reshape(6, 31, 4, 16)
    assert rel_err(torch.einsum('ahnm,amhd->anhd', scores, v).reshape(6, 33, 64), hidden) <= 1e-12
    assert float((scores.sum(-1) - 1).abs().max()) <= 1e-12


def test_key_stride_is_the_front_ends():
    from se3et_amd import ops
    assert all(T.key_stride(m) == ops.key_stride(m) for m in (1, 31, 32, 33, 97, 160))


def test_twin_matches_the_oracle():
    """(A, N, C, H, eq) = (6, 59, 32, 4, True): the oracle's float32 hidden states and scores (unfolded, with the biases) sit at the
    float32 restatement's distance from the twin."""
    from oracle import se3et_oracle as O
    case = T.attention_case(6, 32, 4, True, seed=59, lengths=(59,))
    g = torch.Generator().manual_seed(2)
    st = {'l.proj_%s.%s' % (n, w): case['%s_%s' % (w[0], n)] for n in ('q', 'k', 'v') for w in ('weight', 'bias')}
    st.update({'l.proj_p.weight': case['w_p'], 'l.proj_p.bias': torch.randn(32, generator=g) * 0.1, 'l.proj_eq.weight': case['w_eq'],
               'l.proj_eq.bias': torch.randn(32, generator=g) * 0.1})
    x = case['xs'][0]
    got, got_scores = O.rpe_attention(st, 'l.', x, x, case['embs'][0], case['eq_embs'][0], 4)
    want, rest = T.self_attention(case)[0], T.self_attention(case, T.f32)[0]
    _assert_accepted(got, want, rest, 'oracle hidden')
    pick = lambda t: (t[0], t[1], t[3], t[4], t[5], t[6])
    _assert_accepted(got_scores, T.rpe_scores(*pick(T.projected(case, 0)), 4), T.rpe_scores(*pick(T.projected(case, 0, T.f32)), 4), 'oracle scores')


def test_twin_matches_the_reference_fixture(golden_dir):
    """op/attn_0 (equivariant term) and op/attn_4 (invariant) of tests/golden/micro_se3ete.npz: hidden states and scores."""
    g = np.load(golden_dir + '/micro_se3ete.npz')
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('sd/')}
    emb, eq_emb = torch.from_numpy(g['op/embedding/out0'])[0], torch.from_numpy(g['op/embedding/out1'])[0]
    for layer, eq in ((0, True), (4, False)):
        pre = 'transformer.transformer.layers.%d.attention.attention.' % layer
        x = torch.from_numpy(g['op/attn_%d/in0' % layer])[0]
        x = x if x.dim() == 3 else x[None]
        weights = {'%s_%s' % (w[0], n): sd[pre + 'proj_%s.%s' % (n, w)] for n in ('q', 'k', 'v') for w in ('weight', 'bias')}
        weights.update(w_p=sd[pre + 'proj_p.weight'], w_eq=sd[pre + 'proj_eq.weight'] if eq else None)
        case = T.stack_case_from([x], [emb], [eq_emb if eq else None], weights, 4)
        want, rest = T.self_attention(case)[0], T.self_attention(case, T.f32)[0]
        out0, out1 = torch.from_numpy(g['op/attn_%d/out0' % layer])[0], torch.from_numpy(g['op/attn_%d/out1' % layer])[0]
        _assert_accepted(out0.reshape(want.shape), want, rest, 'fixture layer %d hidden' % layer)
        pick = lambda t: (t[0], t[1], t[3], t[4], t[5], t[6])
        _assert_accepted(out1.reshape(x.shape[0], 4, 59, 59), T.rpe_scores(*pick(T.projected(case, 0)), 4),
                         T.rpe_scores(*pick(T.projected(case, 0, T.f32)), 4), 'fixture layer %d scores' % layer)


def test_the_two_figures():
    """global against the tensor's largest entry; per row against the row's own, a small row against 1e-3 of the tensor's."""
    want = torch.tensor([[[512.0, 1.0], [1.0, 0.5], [0.25, 0.0]]], dtype=F64)
    got = want.clone()
    got[0, 1, 1] += 0.125
    assert T.error_figures(got, want) == (0.125 / 512, 0.125 / 1.0)
    got = want.clone()
    got[0, 2, 1] += 0.125                         # the row's own maximum 0.25 is below 1e-3 x 512
    assert T.error_figures(got, want) == (0.125 / 512, 0.125 / (1e-3 * 512))
    assert T.allowed(0.0) == 16 * 1.2e-7 and T.allowed(1e-6) == 1.6e-5 and T.allowed(1e-5) == 1e-4


# ---------------------------------------------------------------------------------------------------------------------------------------
# the stress kinds
# ---------------------------------------------------------------------------------------------------------------------------------------
def _stress_cases():
    for kind in T.STACK_STRESS_KINDS:
        yield 'stack %s' % kind, T.stack_stress_case(kind)
    for kind, (N, M) in T.PAIR_STRESS:
        yield 'pair %s' % kind, T.pair_case(256, N, M, kind)


@pytest.mark.parametrize('name,case', list(_stress_cases()), ids=[n for n, _ in _stress_cases()])
def test_stress_cases_show_what_they_are_for(name, case):
    """On the twin's own softmax, at every shape the GPU file runs a stress kind at.  peaked: more than half of the rows have a top
    probability above 0.5.  late: in at least half of the rows of every cloud with >= 3 key tiles the largest logit of a 32-key tile
    rises from each tile to the next, and in at least 70 % of the rows the largest logit lies in the last quarter of the keys; early:
    the mirror image.  offset: the median |row mean| of the scaled logits is at least twice their (median) standard deviation along the
    keys.  All: 16 x the float32 restatement's error stays below 1e-4 in both figures, so the ceiling of the rule never binds."""
    kind = case['kind']
    for c, s in enumerate(T.case_logits(case)):
        stats = T.stress_statistics(s, kind)
        print(name, 'cloud', c, stats)
        if kind == 'peaked':
            assert stats['peaked_rows'] > 0.5
        elif kind == 'offset':
            assert stats['mean_over_std'] >= 2.0
        else:
            assert stats['outer_quarter'] >= 0.7
            assert T.key_stride(s.shape[-1]) // 32 >= 3 and stats['monotone_rows'] >= 0.5
    if 'q' in case:
        pairs = [(T.pair_attention(case, T.f32)[0], T.pair_attention(case)[0])]
    else:
        pairs = list(zip(T.self_attention(case, T.f32), T.self_attention(case)))
    for rest, want in pairs:
        for what, r in zip(('global', 'per row'), T.error_figures(rest, want)):
            print(name, what, 'restatement %.3e' % r)
            assert 16 * r < 1e-4, '%s %s: the restatement is at %.3e' % (name, what, r)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the power of the check
# ---------------------------------------------------------------------------------------------------------------------------------------
def _float32_attention(case, mistake=None, tile=1):
    """The float32 restatement of a pair case written out tile by tile, with one modelled kernel mistake."""
    q, k, vt, emb, w_p, eq_emb, w_eq = T.pair_inputs(case, T.f32)
    A, N, C = q.shape
    M, H = k.shape[1], case['H']
    d = C // H
    if mistake == 'f16 embedding':
        emb = emb.to(torch.float16).to(torch.float32)
    qk = torch.einsum('anhd,amhd->ahnm', q.reshape(A, N, H, d), k.reshape(A, M, H, d))
    rpe = T.rpe_logits(q, emb, w_p, eq_emb, w_eq, H).reshape(A, H, N, M)
    if mistake == 'padding logit':
        rpe[..., M - 1] = 0.0
    s = (qk + rpe) / math.sqrt(d)
    if mistake == 'last key masked':
        s[..., M - 1] = float('-inf')
    top = s.amax(-1, keepdim=True)
    w = torch.exp(s - top)
    l = w.sum(-1, keepdim=True)
    cols = slice(32 * tile, min(32 * tile + 32, M))
    if mistake == 'stale maximum':                # the tile's P.V product formed with the running maximum and not rescaled afterwards
        w = w.clone()
        w[..., cols] = torch.exp(s[..., cols] - s[..., :cols.stop].amax(-1, keepdim=True))
    if mistake == 'tile missing in l':
        l = l - w[..., cols].sum(-1, keepdim=True)
    v = vt[..., :M].transpose(1, 2).reshape(A, M, H, d)
    out = torch.einsum('ahnm,amhd->anhd', w / l, v)
    if mistake == 'neighbouring row':
        out[A - 1, N // 2, H - 1] = out[A - 1, N // 2 + 1, H - 1]
    return out.reshape(A, N, C)


MISTAKES = (('f16 embedding', 'plain', 1), ('f16 embedding', 'late', 1), ('last key masked', 'plain', 1), ('padding logit', 'plain', 1), ('stale maximum', 'plain', 1),
            ('tile missing in l', 'late', 2), ('neighbouring row', 'plain', 1))


def test_the_rule_rejects_modelled_kernel_mistakes_and_the_old_rule_does_not():
    """A `got` built from the float32 restatement with one mistake, at (A, N, M, C) = (6, 40, 97, 256), a shape of case (c): the embedding
    rounded to f16 before the product (a lost lo piece), on the `plain` and on the `late` inputs; key M - 1 masked out; key M - 1's
    relative-position logit replaced by a padding column's 0; one 32-key tile weighted with the maximum of the tiles up to it and not
    rescaled; on the `late` inputs one tile's part of l left out; one output row of one (anchor, head) replaced by its neighbour's.  The
    rule rejects every one of them, and accepts the same code without a mistake.

    helpers.assert_close's whole-tensor 1e-4 accepts the f16 embedding on the `late` inputs (2.4e-5 of the largest entry, against the
    1.6e-5 that the rule allows there); on the `plain` inputs the same mistake is at 2.4e-4, within a factor 3 of passing it.  That is
    the gap this file closes."""
    old_rule_accepts = []
    for mistake, kind, tile in MISTAKES:
        case = T.pair_case(256, 40, 97, kind)
        want, rest = T.pair_attention(case)[0], T.pair_attention(case, T.f32)[0]
        clean = T.check(_float32_attention(case), want, rest)
        assert not T.rejected(clean), 'the tile-by-tile restatement itself: ' + _figures_text(clean)
        got = _float32_attention(case, mistake, tile)
        figures = T.check(got, want, rest)
        old = rel_err(got, want)
        print('%-18s %-6s %s   whole-tensor %.2e' % (mistake, kind, _figures_text(figures), old))
        assert T.rejected(figures), '%s passes: %s' % (mistake, _figures_text(figures))
        if old <= 1e-4:
            old_rule_accepts.append((mistake, kind))
    assert ('f16 embedding', 'late') in old_rule_accepts, old_rule_accepts
