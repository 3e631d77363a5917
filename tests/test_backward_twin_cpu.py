"""The float64 twin of the backward kernels (tests/backward_twin.py) on its own, no GPU: every gradient against central finite differences,
the max-pool tie table, the float32 restatements of se3et_amd/autograd.py against the twin on benign inputs, and the input-side conditions
of the stress cases that tests/test_gpu_backward_edges.py runs the kernels on."""
import pytest
import torch

import backward_twin as T
from helpers import assert_close
from se3et_amd import autograd as AG


def _directional(fn, inputs, seed, eps=1e-5):
    """<grad, d> by autograd against (f(x + eps d) - f(x - eps d)) / (2 eps), f = <fn(x), c>, one random direction d over all float inputs and
    a random cotangent c, float64: -> relative error."""
    g = torch.Generator().manual_seed(seed)
    inputs = [T.f64(t) if torch.is_tensor(t) else t for t in inputs]
    out = fn(*inputs)
    out = out[0] if isinstance(out, tuple) else out
    c = torch.randn(out.shape, generator=g, dtype=T.F64)
    grads = T.vjp(fn, inputs, c)[1]
    dirs = [torch.randn(t.shape, generator=g, dtype=T.F64) if gr is not None else None for t, gr in zip(inputs, grads)]
    an = sum(float((gr * d).sum()) for gr, d in zip(grads, dirs) if gr is not None)

    def f(sign):
        moved = [t + sign * eps * d if d is not None else t for t, d in zip(inputs, dirs)]
        o = fn(*moved)
        return float(((o[0] if isinstance(o, tuple) else o) * c).sum())
    fd = (f(1.0) - f(-1.0)) / (2 * eps)
    return abs(fd - an) / abs(an)


def test_twin_gradients_match_central_differences():
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g)
    # Sinkhorn 2 x 5 x 4 with masks; the cotangent of _directional reads masked entries too: they are constants there (-inf value), which
    # central differences see as well
    rm, cm = torch.tensor([[1, 1, 0, 1, 1], [0, 1, 1, 1, 0]]).bool(), torch.tensor([[1, 0, 1, 1], [1, 1, 1, 0]]).bool()
    sink = lambda s, a: T.log_optimal_transport(s, a, rm, cm, 20, 1e12)
    out = sink(T.f64(rn(2, 5, 4)), torch.tensor(0.7, dtype=T.F64))
    assert out.dtype == T.F64                                                    # (no float32 left in the restatement)
    masked = torch.zeros(2, 6, 5, dtype=torch.bool)
    masked[:, :5] |= ~rm[:, :, None]
    masked[:, :, :4] |= ~cm[:, None, :]
    valid_only = lambda s, a: torch.where(masked, torch.zeros((), dtype=T.F64), sink(s, a))
    assert _directional(valid_only, [rn(2, 5, 4), torch.tensor(0.7)], 2) <= 1e-6
    # GroupNorm 12 x 8, two segments, bias of the producing layer, residual, LeakyReLU
    gn = lambda x, w, b, r, xb: T.group_norm_rows(x, w, b, r, xb, 2, 1e-5, 0.1, [0, 6, 12])
    assert _directional(gn, [rn(12, 8), rn(8), rn(8), rn(12, 8), rn(8)], 3) <= 1e-6
    # add + LayerNorm 2 x 3 x 8 with the residual broadcast over the leading axis
    ln = lambda h, r, w, b, hb: T.add_layer_norm(h, r, w, b, hb, 1e-5)
    assert _directional(ln, [rn(2, 3, 8), rn(3, 8), rn(8), rn(8), rn(8)], 4) <= 1e-6
    # KPConv P = 6, NN = 4, Cin = 2, Cout = 3
    case = T.kpconv_case(6, 9, 4, 2, 3, seed=5)
    kp = lambda x, w: T.kpconv_inter_so3(x, T.f64(case['q_pts']), T.f64(case['s_pts']), case['idx'], T.f64(case['kernel_points']), w,
                                         case['kidx'], case['ridx'], case['sigma'])
    assert _directional(kp, [case['x'], case['weights']], 6) <= 1e-6
    # padded gather (linear)
    idx = torch.tensor([[0, 5, 2], [4, 4, 5]])
    assert _directional(lambda x: T.gather_rows_padded(x, idx), [rn(5, 3)], 7) <= 1e-6


def test_max_pool_ties_go_to_the_first_entry_in_table_order():
    x, idx, cot, want = T.max_pool_tie_cases()
    out, (dx, _) = T.vjp(T.neighbor_max_pool, [x, idx], cot)
    assert torch.equal(out, torch.tensor([[1.5, 0.0], [1.5, 0.0], [1.5, 0.0], [-1.0, 0.0]], dtype=T.F64))
    assert torch.equal(dx, want)
    # the restatement of se3et_amd/autograd.py states the same rule, in float32 too
    for conv in (T.f64, T.f32):
        out_r, (dx_r, _) = T.vjp(AG.neighbor_max_pool, [x, idx], cot, conv)
        assert torch.equal(out_r.double(), out) and torch.equal(dx_r.double(), want)
    # the three named cases one by one
    one = lambda table: T.vjp(T.neighbor_max_pool, [x, torch.tensor([table])], torch.ones(1, 2))[1][0]
    assert one([2, 0, 1])[:, 0].tolist() == [0.0, 0.0, 1.0, 0.0]                 # three tied real neighbours
    assert one([0, 4])[:, 1].tolist() == [1.0, 0.0, 0.0, 0.0]                    # real 0.0 in front of a padded entry
    assert one([4, 0])[:, 1].tolist() == [0.0, 0.0, 0.0, 0.0]                    # padded entry in front of the real 0.0
    assert one([-1, 3])[:, 0].tolist() == [0.0, 0.0, 0.0, 1.0]                   # -1 marker in front of a negative real value
    assert float(T.vjp(T.neighbor_max_pool, [x, torch.tensor([[-1, -1]])], torch.ones(1, 2))[1][0].abs().max()) == 0.0
    assert torch.equal(T.max_pool_winners(x, idx), torch.tensor([[2.0, 2.0], [0.0, 0.0], [1.0, 0.0], [1.0, 1.0]], dtype=T.F64))


def test_float32_restatements_match_the_twin_on_benign_inputs():
    """The change of se3et_amd/autograd.py (Sinkhorn follows the dtype of its scores, the max-pool ends in max(dim)) moved nothing for
    float32 callers: the figures of tests/test_gpu_training.py hold against the twin."""
    case = T.sinkhorn_case(3, 20, 24, seed=11)
    want, got = T.sinkhorn_twin(case, 100), T.sinkhorn_twin(case, 100, convert=T.f32)
    assert got[0].dtype == torch.float32
    v, m = case['valid'], case['valid'][:, :20, :24]
    assert_close(got[0][v], want[0][v], 1e-4, 'sinkhorn forward')
    assert float(got[1][~m].abs().max()) == 0.0 and float(want[1][~m].abs().max()) == 0.0
    assert_close(got[1][m], want[1][m], 1e-4, 'sinkhorn d/dscores')
    assert abs(float(got[2]) - float(want[2])) <= 1e-4 * max(1.0, abs(float(want[2])))
    gn = T.group_norm_case(120, 32, seed=12)
    want, got = T.group_norm_twin(gn, 4, 1e-5, 0.1, [0, 48, 120]), T.group_norm_twin(gn, 4, 1e-5, 0.1, [0, 48, 120], convert=T.f32)
    assert not bool(T.kink_mask(want[1]).any())
    assert_close(got[0], want[0], 2e-5, 'group norm forward')
    for name, a, b in zip(('x', 'weight', 'bias', 'residual', 'x_bias'), got[2], want[2]):
        assert_close(a, b, 2e-5, 'group norm d/d' + name)
    g = torch.Generator().manual_seed(13)
    rn = lambda *s: torch.randn(*s, generator=g)
    ln_in, c = [rn(6, 11, 32), rn(11, 32), rn(32), rn(32), rn(32)], rn(6, 11, 32)
    ln = lambda h, r, w, b, hb: T.add_layer_norm(h, r, w, b, hb, 1e-5)
    for a, b in zip(T.vjp(ln, ln_in, c, T.f32)[1], T.vjp(ln, ln_in, c)[1]):
        assert_close(a, b, 2e-5, 'layer norm')
    kp = T.kpconv_case(40, 60, 12, 8, 16, seed=14)
    want, got = T.kpconv_twin(kp), T.kpconv_twin(kp, T.f32)
    for name, a, b in zip(('forward', 'dL/dx', 'dL/dW'), got, want):
        assert_close(a, b, 2e-5, 'kpconv ' + name)
    x, c2 = rn(60, 6, 8), rn(40, 6, 8)
    assert bool((kp['idx'] == 60).any())
    for a, b in zip(T.vjp(AG.neighbor_max_pool, [x, kp['idx']], c2, T.f32)[1][:1], T.vjp(T.neighbor_max_pool, [x, kp['idx']], c2)[1][:1]):
        assert_close(a, b, 1e-6, 'max pool dL/dx')
    for a, b in zip(T.vjp(AG.gather_rows_padded, [x, kp['idx'][:, 0]], c2, T.f32)[1][:1], T.vjp(T.gather_rows_padded, [x, kp['idx'][:, 0]], c2)[1][:1]):
        assert_close(a, b, 1e-6, 'padded gather dL/dx')


@pytest.mark.parametrize('offset', [10.0, 100.0, 1000.0])
def test_group_norm_offset_inputs_keep_away_from_the_kink(offset):
    """x = randn + offset at (1800, 32, 4): float32 arithmetic places a pre-activation to about 1e-3 there (the restatement at offset 1000),
    far more than the kink window, so these inputs keep every pre-activation 0.02 away from 0: nothing sits in the window (the cap is
    0.1 %), and the float32 restatement takes the twin's slope everywhere -- its error against the twin, which sets the kernels' tolerance,
    is then a rounding error and not a flipped slope."""
    case = T.group_norm_offset_case(offset)
    _, pre, _ = T.group_norm_twin(case, 4, 1e-5, 0.1, None)
    assert float(pre.abs().min()) >= 0.02 - 1e-6
    assert float(T.kink_mask(pre).double().mean()) <= T.KINK_CAP
    pre32 = AG.group_norm_rows(T.f32(case['x']), T.f32(case['weight']), T.f32(case['bias']), T.f32(case['residual']), T.f32(case['x_bias']), 4, 1e-5,
                               None, None)
    assert float((pre32.double() - pre).abs().max()) < 0.01 and not bool(((pre32 > 0) != (pre > 0)).any())
    assert abs(float(case['x'].mean()) - offset) < 0.1 and abs(float(case['x'].std()) - 1.0) < 0.1


def test_group_norm_edge_shapes_keep_away_from_the_kink():
    for rows, C, groups in T.GN_EDGE_SHAPES + ((240, 32, 4),):
        case = T.group_norm_case(rows, C, seed=rows)
        _, pre, _ = T.group_norm_twin(case, groups, 1e-5, 0.1, T.SIXTEEN_SEGMENTS if rows == 240 else None)
        assert float(T.kink_mask(pre).double().mean()) <= T.KINK_CAP, (rows, C)
    assert len(T.SIXTEEN_SEGMENTS) == 17 and T.SIXTEEN_SEGMENTS[-1] == 240
    sizes = [b - a for a, b in zip(T.SIXTEEN_SEGMENTS[:-1], T.SIXTEEN_SEGMENTS[1:])]
    assert 6 in sizes and 120 in sizes and min(sizes) == 6


@pytest.mark.parametrize('size,scale', [(64, 10.0), (64, 30.0), (128, 10.0), (128, 30.0)])
def test_sinkhorn_wide_scores_have_finite_twin_gradients(size, scale):
    case = T.sinkhorn_case(3, size, size, seed=size, scale=scale)
    out, ds, da = T.sinkhorn_twin(case, 100)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(ds).all()) and bool(torch.isfinite(da))
    assert float(case['scores'].abs().max()) > 3 * scale
    m = case['valid'][:, :size, :size]
    assert float(ds[~m].abs().max()) == 0.0 and float(ds[m].abs().max()) > 0.0
    # the masks are what the GPU test expects: every pair has a valid row and column, the last pair exactly one of each, not the first
    rm, cm = case['row_masks'], case['col_masks']
    assert int(rm.sum(1).min()) >= 1 and int(cm.sum(1).min()) >= 1
    assert int(rm[-1].sum()) == 1 and int(cm[-1].sum()) == 1 and not bool(rm[-1, 0]) and not bool(cm[-1, 0])


def test_neighbour_tables_of_the_stress_cases_hold_the_intended_padding():
    blind = T.kpconv_blind_case()
    Ns = blind['x'].shape[0]
    assert bool((blind['idx'][::3] == Ns).all())
    seen = torch.zeros(Ns + 1, dtype=torch.bool)
    seen[blind['idx'].reshape(-1)] = True
    assert 0 < int((~seen[:Ns]).sum()) < Ns                                      # support rows that nobody gathers, and rows that somebody does
    full = T.kpconv_case(40, 60, 64, 8, 32, seed=202)
    assert full['idx'].shape == (40, 64) and bool((full['idx'][:, 60:] == 60).all()) and int((full['idx'] < 60).sum(1).min()) >= 1
    for case in (blind, full, T.kpconv_mixed_case()[0]):                         # a support point at most once per query: contributions = references
        real = torch.where(case['idx'] < case['x'].shape[0], case['idx'], -1 - torch.arange(case['idx'].shape[1])[None, :])
        assert all(len(set(r)) == len(r) for r in real.tolist())
    case, loud, reached = T.kpconv_mixed_case()
    assert 0 < int(reached.sum()) < 140 and float(case['cot'][loud].abs().max()) > 1e6 and float(case['cot'].abs().median()) < 10
    res, count = T.kpconv_fixed_resolution(case)
    assert int(count.max()) <= 90 and 0 < res < 1e-4                             # (1e6 * 4 * 0.1 * 32 * 2^-40: about 1e-5)
    x, idx, _, _ = T.max_pool_tie_cases()
    assert float(x[0, 0]) == float(x[1, 0]) == float(x[2, 0]) and float(x[0, 1]) == 0.0 and bool((idx == 4).any()) and bool((idx == -1).any())
