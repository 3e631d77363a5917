"""CPU: pins the float64 twin of the dense + GroupNorm family (tests/dense_twin.py), its judge and the cases that
tests/test_gpu_dense_edges.py runs the kernels on, so that a failure on the GPU can be trusted: the twin's GroupNorm against
torch.nn.functional.group_norm, its pending algebra against the plain composition, its layout maps against BlockedFeatures.plain();
every case against what it claims (segment lengths at the row tile, tiny rows below 2^-4, a zero-variance segment, a float32 restatement
small enough that the 1e-4 cap never decides, r < 1e-3 where the statistics cancel); the judge against six planted kernel faults, the
first of which the whole-tensor figure of the older tests lets through."""
import pytest
import torch
import torch.nn.functional as F

import backward_twin as B
import dense_twin as T

OLD_TENSOR_BOUND = 2e-5       # tests/test_gpu_ops.py: max |got - want| <= 2e-5 max(1, max |want|)
OUTPUTS = (('raw', T.F_PRODUCT), ('normed', T.F_TABLE), ('residual', T.F_TABLE), ('nothing', T.F_TABLE), ('shortcut', T.F_TABLE),
           ('linear', T.F_PRODUCT), ('linear relu', T.F_PRODUCT))


def _text(figures):
    return '   '.join('%s %.2e (restatement %.2e, allowed %.2e)' % f for f in figures)


def _gn_reference(y, gw, gb, groups, eps, segments):
    """torch.nn.functional.group_norm in float64 on per-segment slices: a segment's rows are the spatial axis of ONE sample."""
    out = torch.empty_like(y)
    for a, b in T.bounds(y.shape[0], segments):
        out[a:b] = F.group_norm(y[a:b].t()[None], groups, gw, gb, eps)[0].t()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,C,groups,segments', [(50, 32, 4, None), (77, 40, 8, [0, 1, 30, 77]), (33, 64, 64, [0, 20, 33]), (9, 16, 1, None)])
def test_twin_group_norm_is_torch_group_norm_per_segment(rows, C, groups, segments):
    g = torch.Generator().manual_seed(rows)
    y, xb, gw, gb = [torch.randn(*s, generator=g, dtype=T.F64) for s in ((rows, C), (C,), (C,), (C,))]
    y = y + 3.0
    want = _gn_reference(y + xb, gw, gb, groups, T.EPS, segments)
    table = T.group_norm_table(y, xb, gw, gb, groups, T.EPS, segments)
    assert table.shape == (len(T.bounds(rows, segments)), 2, C)
    got = T.apply(y, [table], [1.0], None, None, 1.0, segments)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # the composition group_norm_rows is the twin of tests/backward_twin.py with a residual and a LeakyReLU
    res = torch.randn(rows, C, generator=g, dtype=T.F64)
    mine = T.group_norm_rows(y, gw, gb, res, xb, groups, T.EPS, 0.1, segments)
    theirs = B.group_norm_rows(y, gw, gb, res, xb, groups, T.EPS, 0.1, segments)[0]
    assert float((mine - theirs).abs().max()) <= 1e-12 * float(theirs.abs().max())
    assert torch.equal(T.group_norm_rows(y, gw, gb, None, None, groups, T.EPS, None, segments),
                       T.apply(y, [T.group_norm_table(y, None, gw, gb, groups, T.EPS, segments)], [1.0], None, None, 1.0, segments))


def test_twin_pending_algebra_is_normalise_leaky_relu_linear():
    """Two layers in the pending form (the product without its bias, the norm as a table that the consumer applies) against the plain
    composition linear + bias -> GroupNorm -> LeakyReLU -> linear + bias -> GroupNorm [+ shortcut norm] -> LeakyReLU."""
    c = T.evaluate(T.dense_case(90, 32, 64, 8, (), 5, segments=[0, 31, 90]), T.f64)
    case = {k: T.f64(v) for k, v in T.dense_case(90, 32, 64, 8, (), 5, segments=[0, 31, 90]).items() if torch.is_tensor(v)}
    seg = [0, 31, 90]
    h = F.leaky_relu(_gn_reference(F.linear(case['x'], case['w'], case['b']), case['gw'], case['gb'], 8, T.EPS, seg), 0.1)
    assert float((c['normed'] - h).abs().max()) <= 1e-12 * float(h.abs().max())
    g = torch.Generator().manual_seed(6)
    w3, b3, gw3, gb3 = [torch.randn(*s, generator=g, dtype=T.F64) for s in ((32, 64), (32,), (32,), (32,))]
    raw3, table3 = T.dense_norm(c['raw'], [c['table']], [0.1], w3, b3, gw3, gb3, 4, T.EPS, seg)
    plain3 = _gn_reference(F.linear(h, w3, b3), gw3, gb3, 4, T.EPS, seg)
    assert float((T.apply(raw3, [table3], [1.0], None, None, 1.0, seg) - plain3).abs().max()) <= 1e-11 * float(plain3.abs().max())
    # the three tails of dense_residual
    main = _gn_reference(F.linear(case['x'], case['w'], case['b']), case['gw'], case['gb'], 8, T.EPS, seg)
    short = _gn_reference(F.linear(case['x2'], case['w2'], case['b2']), case['gw2'], case['gb2'], 8, T.EPS, seg)
    for name, want in (('nothing', main), ('residual', main + case['residual']), ('shortcut', main + short)):
        want = F.leaky_relu(want, 0.1)
        assert float((c[name] - want).abs().max()) <= 1e-11 * float(want.abs().max()), name
    assert torch.equal(c['linear'], c['raw'] + case['b'])


@pytest.mark.parametrize('kind,C', [(1, 16), (1, 48), (2, 8), (2, 40)])
def test_layout_maps_are_blocked_features_plain(kind, C):
    from se3et_amd import ops
    data = torch.randn(7 * 6 * C, generator=torch.Generator().manual_seed(C))
    idx = T.layout_index(kind, 7, C)
    assert sorted(idx.flatten().tolist()) == list(range(7 * 6 * C))                 # a permutation
    assert torch.equal(data[idx], ops.BlockedFeatures(data, (7, 6, C), kind).plain())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_row_counts_and_segment_lengths_sit_at_the_row_tile():
    assert [T.tile_rows(N) for N in T.TILE_WIDTHS] == [128, 128, 128, 64, 64]
    for N in T.TILE_WIDTHS:
        TR = T.tile_rows(N)
        assert T.tile_row_counts(N) == (1, TR - 1, TR, TR + 1, 2 * TR + 1)
    for N in (64, 256, 1024):
        TR = T.tile_rows(N)
        lengths = T.sixteen_lengths(N)
        assert len(lengths) == T.MAX_SEGMENTS and {1, TR - 1, TR, TR + 1} <= set(lengths)
        assert max(lengths) * 2 == sum(lengths) and lengths != sorted(lengths) and sum(lengths) <= 1000
        case = T.case('segments N %d' % N)
        assert case['segments'] == T.offsets(lengths) and case['x'].shape[0] == sum(lengths)
        # neighbouring stage tables an order of magnitude apart
        for aff in case['affines']:
            size = aff[:, 0].abs().mean(1)
            ratio = size[1:] / size[:-1]
            assert bool(((ratio > 8) | (ratio < 1 / 8)).all())
    wide = T.case('segments N 4096')
    assert tuple(wide['x'].shape) == (65, 32) and wide['w'].shape[0] == 4096 == 16 * 256
    assert [N // G for N, G in T.GROUP_SHAPES] == [1, 32, 32, 32, 32]


def _assert_cap_never_decides(name):
    case = T.case(name)
    seg, G = case['segments'], case['groups']
    for out, factor in OUTPUTS:
        figs = T.check(case['restatement'][out], case['twin'][out], case['restatement'][out], factor, seg, G)
        for fig, _, r, a in figs:
            assert factor * max(r, T.F32_EPS) < T.CEILING and a < T.CEILING, '%s %s %s: restatement %.3e' % (name, out, fig, r)
    for t in ('table', 'table2'):
        raw = case['twin']['raw' if t == 'table' else 'raw2']
        for fig, _, r, a in T.check_table(case['restatement'][t], case['twin'][t], case['restatement'][t], raw, seg, G):
            assert T.F_TABLE * max(r, T.F32_EPS) < T.CEILING, '%s %s %s: restatement %.3e' % (name, t, fig, r)


@pytest.mark.parametrize('N', T.TILE_WIDTHS)
def test_cap_never_decides_a_tile_case(N):
    for name in T.ORDINARY:
        if name.startswith('tile N %d ' % N):
            _assert_cap_never_decides(name)


@pytest.mark.parametrize('name', [n for n in T.ORDINARY if not n.startswith('tile')])
def test_cap_never_decides_an_ordinary_case(name):
    _assert_cap_never_decides(name)


@pytest.mark.parametrize('name', T.CANCELLING)
def test_cancellation_cases_cancel_and_keep_their_restatement_small(name):
    case = T.case(name)
    assert case['cancel']
    seg, G = case['segments'], case['groups']
    if name.startswith('offset'):
        offset = float(name.split()[1])
        for raw in ('raw', 'raw2'):
            for a, b in T.bounds(300, seg):
                blk = case['twin'][raw][a:b].reshape(b - a, G, -1)
                ratio = blk.mean((0, 2)).abs() / blk.std((0, 2))
                assert float(ratio.min()) >= 0.3 * offset, (raw, float(ratio.min()))
    for out, factor in OUTPUTS:
        for fig, _, r, _ in T.check(case['restatement'][out], case['twin'][out], case['restatement'][out], factor, seg, G, cancel=True):
            assert r < T.CANCEL_R, (out, fig, r)
    for t, raw in (('table', 'raw'), ('table2', 'raw2')):
        for fig, _, r, _ in T.check_table(case['restatement'][t], case['twin'][t], case['restatement'][t], case['twin'][raw], seg, G, True):
            assert r < T.CANCEL_R, (t, fig, r)


@pytest.mark.parametrize('name', list(T.ROWS_FORWARD))
def test_group_norm_rows_forward_cases_keep_their_restatement_small(name):
    c = T.rows_forward(name)
    want = B.group_norm_rows(*[T.f64(c['case'][k]) for k in T.GN_NAMES], c['groups'], T.EPS, c['slope'], c['segments'])[0]
    assert float((c['twin'] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    for fig, _, r, a in T.check(c['restatement'], c['twin'], c['restatement'], T.F_TABLE, c['segments'], c['groups'], c['cancel']):
        if c['cancel']:
            assert r < T.CANCEL_R, (fig, r)
        else:
            assert T.F_TABLE * max(r, T.F32_EPS) < T.CEILING, (fig, r)


@pytest.mark.parametrize('kind', T.ZERO_KINDS)
def test_zero_segment_has_zero_variance(kind):
    case = T.case('zero segment ' + kind)
    tw = case['twin']
    assert float(tw['raw'][:70].abs().max()) == 0.0 and float(tw['raw'][70:].abs().min()) > 0.0
    yb = tw['raw'][:70] + (T.f64(case['b']) if case['b'] is not None else 0.0)
    var = yb.reshape(70, case['groups'], -1).var((0, 2), unbiased=False)
    if kind == 'bias':
        assert float(var.min()) > 0.0                       # the variance of the bias over the group's channels
        return
    assert float(var.max()) == 0.0
    # scale = gw / sqrt(eps), the means are the bias: the segment's normalised value is gb
    gb = T.f64(case['gb'])
    want = T.lrelu(gb, case['final_slope'])
    assert float((tw['nothing'][:70] - want).abs().max()) <= 1e-12
    assert float((tw['residual'][:70] - T.lrelu(gb + T.f64(case['residual'][:70]), case['final_slope'])).abs().max()) <= 1e-12


@pytest.mark.parametrize('kind', T.SCALE_KINDS)
@pytest.mark.parametrize('shape', T.SCALE_SHAPES)
def test_scaled_rows_are_where_the_case_says(kind, shape):
    case = T.case('%s (%d, %d, %d, %d)' % ((kind,) + shape))
    rows = shape[0]
    TR = T.tile_rows(shape[2])
    picked = case['picked']
    assert rows - 1 in picked and rows % TR != 0 and len({r // TR for r in picked}) >= 2
    # float32, as the kernel forms T(x); the split decides on the first 32 values of a row
    t = T.pending(case['x'], case['affines'], case['slopes'], None)
    first = t[:, :32].abs().amax(1)
    others = torch.ones(rows, dtype=torch.bool)
    others[picked] = False
    assert bool((first[others] >= T.TINY).all()) and bool((first[others] < 128).all())
    if kind == 'tiny start':
        assert bool((first[picked] < T.TINY).all()) and bool((t[picked][:, 32:].abs().amax(1) >= T.TINY).all())
    else:
        lo, hi = (2.0 ** -14, 2.0 ** -10) if kind == 'main 2^-13' else (2.0 ** 11, 2.0 ** 15)
        assert bool(((first[picked] > lo) & (first[picked] < hi)).all())
    # each input on its own is inside the headroom of its own scale: nothing beyond 2^8 times the largest of the row's first 32 values
    for v in (t, case['x2']):
        assert bool((v.abs().amax(1) < 2.0 ** 8 * v[:, :32].abs().amax(1)).all())
    x2 = case['x2'][:, :32].abs().amax(1)
    assert bool(((x2 >= T.TINY) & (x2 < 128)).all())
    assert bool((case['gw2'] < 0).any()) and bool((case['gw2'] > 0).any()) and float(case['gw2'].abs().min()) < 2e-3 and float(case['gw2'].abs().min()) > 1e-30


# ---------------------------------------------------------------------------------------------------------------------------------------
# the judge
# ---------------------------------------------------------------------------------------------------------------------------------------
def _judged(case, out, got, factor=T.F_TABLE):
    figs = T.check(got, case['twin'][out], case['restatement'][out], factor, case['segments'], case['groups'], case['cancel'])
    return figs


def test_judge_passes_the_restatement_and_the_twin():
    case = T.case('segments N 64')
    for out, factor in OUTPUTS:
        assert not T.rejected(_judged(case, out, case['restatement'][out], factor)), out
        assert not T.rejected(_judged(case, out, case['twin'][out], factor)), out


def test_fault_one_row_of_a_short_segment_off_by_a_thousandth():
    """... and the whole-tensor figure of the older tests lets it through when the tensor's other segment is 100 times larger."""
    case = T.case('segments N 64')
    seg = case['segments']
    s = T.sixteen_lengths(64).index(5)
    row = seg[s] + 2
    for out, factor in (('raw', T.F_PRODUCT), ('shortcut', T.F_TABLE)):
        got = case['twin'][out].clone()
        got[row] += 1e-3 * got[row].abs().max()
        figs = _judged(case, out, got, factor)
        assert T.rejected(figs), _text(figs)
        assert dict((f[0], f[1] > f[3]) for f in figs)['per row']
    # the gap: two segments, the second 100 times larger
    two = T.dense_case(200, 64, 64, 2, (), 9, segments=[0, 40, 200])
    two['x'][40:] *= 100.0
    want, rest = T.evaluate(two, T.f64)['raw'], T.evaluate(two, T.f32)['raw']
    got = want.clone()
    got[7] += 1e-3 * got[7].abs().max()
    assert float((got - want).abs().max()) <= OLD_TENSOR_BOUND * max(1.0, float(want.abs().max()))          # the older assertion passes
    figs = T.check(got, want, rest, T.F_PRODUCT, two['segments'], 2)
    assert T.rejected(figs), _text(figs)
    fig = {f[0]: f for f in figs}
    assert fig['per row'][1] > fig['per row'][3] and fig['per block'][1] > fig['per block'][3]


def test_fault_two_neighbouring_segments_swap_their_stage_tables():
    case = T.case('segments N 64')
    c = {k: T.f64(case[k]) for k in T.FLOAT_KEYS}
    swapped = []
    for aff in case['affines']:
        a = T.f64(aff).clone()
        a[[4, 5]] = a[[5, 4]]
        swapped.append(a)
    raw, table = T.dense_norm(c['x'], swapped, case['slopes'], c['w'], c['b'], c['gw'], c['gb'], case['groups'], T.EPS, case['segments'])
    figs = _judged(case, 'raw', raw, T.F_PRODUCT)
    assert T.rejected(figs), _text(figs)
    figs = T.check_table(table, case['twin']['table'], case['restatement']['table'], case['twin']['raw'], case['segments'], case['groups'])
    assert T.rejected(figs), _text(figs)
    # the layer's own table taken from the neighbour
    t = case['twin']['table'].clone()
    t[[4, 5]] = t[[5, 4]]
    figs = T.check_table(t, case['twin']['table'], case['restatement']['table'], case['twin']['raw'], case['segments'], case['groups'])
    assert T.rejected(figs), _text(figs)


def test_fault_layer_bias_left_out_of_the_means():
    case = T.case('groups N 256 / 8')
    tw = case['twin']
    wrong = T.group_norm_table(tw['raw'], None, T.f64(case['gw']), T.f64(case['gb']), case['groups'], T.EPS, case['segments'])
    right = T.group_norm_table(tw['raw'] + T.f64(case['b']), None, T.f64(case['gw']), T.f64(case['gb']), case['groups'], T.EPS, case['segments'])
    shift = right[:, 1] + T.f64(case['b']) * right[:, 0]              # GroupNorm(y + b) as a map of y
    assert float((shift - tw['table'][:, 1]).abs().max()) <= 1e-12 and float((right[:, 0] - tw['table'][:, 0]).abs().max()) <= 1e-12
    figs = T.check_table(wrong, tw['table'], case['restatement']['table'], tw['raw'], case['segments'], case['groups'])
    assert T.rejected(figs), _text(figs)


def test_fault_statistics_count_the_padding_rows_of_a_partial_tile():
    """129 rows at TR = 128: the second tile holds one row and 127 padding rows, which the kernel reads as zeros and stages as T(0)."""
    case = T.case('tile N 64 rows 129 K 64 stages 2')
    c = {k: T.f64(case[k]) for k in T.FLOAT_KEYS}
    aff = [T.f64(a) for a in case['affines']]
    padded = torch.cat((c['x'], torch.zeros(127, 64, dtype=T.F64)))
    table = T.dense_stats(padded, aff, case['slopes'], c['w'], c['b'], c['gw'], c['gb'], case['groups'], T.EPS, None)
    assert float(T.pending(padded, aff, case['slopes'], None)[129:].abs().max()) > 0.0          # T(0) is not 0: the padding rows would count
    figs = T.check_table(table, case['twin']['table'], case['restatement']['table'], case['twin']['raw'], None, case['groups'])
    assert T.rejected(figs), _text(figs)


def test_fault_one_group_takes_its_neighbours_rstd():
    case = T.case('groups N 256 / 8')
    tw = case['twin']
    N, G = 256, 8
    cpg = N // G
    gw = T.f64(case['gw'])
    t = tw['table'].clone()
    rstd = (t[1, 0] / gw).reshape(G, cpg)
    assert float((rstd - rstd[:, :1]).abs().max()) <= 1e-12 * float(rstd.abs().max())
    # group 3 of segment 1 with the rstd of group 4: scale and the mean's share of the shift follow
    mean_term = (t[1, 1] - T.f64(case['gb'])) / t[1, 0]
    scale = t[1, 0].clone().reshape(G, cpg)
    scale[3] = rstd[4, 0] * gw.reshape(G, cpg)[3]
    t[1, 0] = scale.reshape(N)
    t[1, 1] = T.f64(case['gb']) + mean_term * t[1, 0]
    figs = T.check_table(t, tw['table'], case['restatement']['table'], tw['raw'], case['segments'], G)
    assert T.rejected(figs), _text(figs)
    assert abs(float(rstd[4, 0] / rstd[3, 0]) - 1) < 0.2           # (a fault of a few per cent, not of a factor)
    got = T.apply(tw['raw'], [t], [1.0], None, None, case['final_slope'], case['segments'])
    figs = _judged(case, 'normed', got)
    assert T.rejected(figs), _text(figs)
    assert figs[0][1] < 0.1


def test_fault_one_shortcut_row_is_clamped_at_the_main_rows_scale():
    """A row whose T(x) is about 2^-13 is scaled by 2^(6 + 13 .. 14) for the f16 split; its unit-size x2 row at that scale leaves the
    f16 range and is clamped to +-65000 x 2^-e."""
    case = T.case('main 2^-13 (300, 64, 128, 64)')
    c = {k: T.f64(case[k]) for k in T.FLOAT_KEYS}
    aff = [T.f64(a) for a in case['affines']]
    row = case['picked'][3]
    t = T.pending(c['x'], aff, case['slopes'], None)
    e = 6 - int(torch.floor(torch.log2(t[row, :32].abs().max())))          # the first 32 values go to [2^6, 2^7)
    assert 18 <= e <= 21
    x2 = c['x2'].clone()
    x2[row] = torch.clamp(x2[row] * 2.0 ** e, -65000.0, 65000.0) * 2.0 ** -e
    assert float((x2[row] - c['x2'][row]).abs().max()) > 0.5
    tw = case['twin']
    got = T.dense_residual(c['x'], aff, case['slopes'], c['w'], tw['table'], None, (x2, c['w2'], tw['table2']), case['final_slope'], None)
    figs = _judged(case, 'shortcut', got)
    assert T.rejected(figs), _text(figs)
    assert (got - tw['shortcut']).abs().amax(1).nonzero().flatten().tolist() == [row]
