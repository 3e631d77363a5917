"""GPU: the dense + GroupNorm family (csrc/dense_norm.hip: ops.dense_norm, dense_stats, dense_residual in its three forms, linear_stream;
the statistics and apply half of csrc/rowops.hip: ops.group_norm_stats, group_norm_apply, group_norm_rows) against the float64 twin
(tests/dense_twin.py) at the edges of the kernels: row counts and segment lengths of 1, TR - 1, TR, TR + 1 and 2 TR + 1 rows at both row
tile heights, one-step walks (K = 32), 16 segments at once with stage tables that differ by an order of magnitude between neighbours, 16
column blocks, 1 and 32 channels per group, statistics that cancel (|mean| >> sigma, an all-zero segment), rows that take a power-of-two
scale of their own in the final modes -- with a shortcut input of another magnitude -- and the two feature layouts of the apply pass.
tests/test_gpu_ops.py compares the same kernels on larger random shapes with one figure per tensor.

Every output is judged in three figures (dense_twin.error_figures): `global`, `per row` and `per block` (per (segment, group), against
the block's own largest |want|).  Allowed: min(1e-4, F max(r, 1.2e-7)), r the same figure of the float32 restatement against the twin;
F = 8 for a product, 16 behind a table that the kernel derived from its own statistics; the cancellation cases: F r without the cap.  A
table is judged by what it does to the twin's raw product.  tests/test_dense_twin_cpu.py holds every case to its claim and shows that the
cap never decides an ordinary case.  With SE3_DENSE_EDGES_PROBE=<file> every case appends a line to that file: per figure `kernel / restatement /
allowed` of the output that came closest to its allowance, and its name (profiles/dense_edges_probe.txt was recorded so; the printed
output of a test has the figures of every output)."""
import os

import pytest
import torch

import dense_twin as T

pytestmark = pytest.mark.gpu

FORMS = ('residual', 'nothing', 'shortcut')


def _dev(t):
    return None if t is None else t.cuda()


_WORST = {}          # case -> {figure: (kernel / allowed, output, kernel, restatement, allowed)} of the test that is running


def _ratio(k, a):
    return k / a if a > 0 else (0.0 if k == 0 else float('inf'))


@pytest.fixture(autouse=True)
def _probe():
    """One line per case behind every test, passed or failed: per figure, the output of the case that came closest to its allowance."""
    _WORST.clear()
    yield
    path = os.environ.get('SE3_DENSE_EDGES_PROBE')
    if path and _WORST:
        with open(path, 'a') as f:
            for case, figs in _WORST.items():
                f.write('%-36s %s\n' % (case, '   '.join('%s %.2e / %.2e / %.2e (%s)' % ((fig,) + v[2:] + (v[1],)) for fig, v in figs.items())))


def _judge(name, figures):
    """`case [output]`: printed, noted for the case's line of the probe, then asserted."""
    print('%s: %s' % (name, '   '.join('%s %.2e / %.2e / %.2e' % f for f in figures)))
    case, _, what = name.partition(' [')
    mine = _WORST.setdefault(case, {})
    for fig, k, r, a in figures:
        if fig not in mine or _ratio(k, a) > mine[fig][0]:
            mine[fig] = (_ratio(k, a), what.rstrip(']') or 'out', k, r, a)
    for fig, k, r, a in figures:
        assert k <= a, '%s %s: error %.3e > %.3e (restatement %.3e)' % (name, fig, k, a, r)


def _check(case, what, got, key, factor):
    assert bool(torch.isfinite(got).all()), '%s [%s] is not finite' % (case['name'], what)
    _judge('%s [%s]' % (case['name'], what),
           T.check(got.cpu(), case['twin'][key], case['restatement'][key], factor, case['segments'], case['groups'], case['cancel']))


def _check_table(case, what, got, key='table', raw='raw'):
    assert bool(torch.isfinite(got).all()), '%s [%s] is not finite' % (case['name'], what)
    _judge('%s [%s]' % (case['name'], what),
           T.check_table(got.cpu(), case['twin'][key], case['restatement'][key], case['twin'][raw], case['segments'], case['groups'], case['cancel']))


def _operands(case):
    from se3et_amd import ops
    d = {k: _dev(case[k]) for k in T.FLOAT_KEYS}
    pend = ops.Pending(d['x'], [a.cuda() for a in case['affines']], list(case['slopes']), case['segments'])
    return d, pend


def _family(name):
    """Every operator of the family on one case, each output judged; the statistics twice (bit-identical); no saturated row.
    -> {output: tensor on the device}."""
    from se3et_amd import ops
    case = T.case(name)
    seg, G, eps, fs = case['segments'], case['groups'], case['eps'], case['final_slope']
    d, pend = _operands(case)
    assert ops.dense_norm_ok(pend, d['w'], G) and ops.dense_norm_ok(d['x2'], d['w2'], G) and ops.norm_weight_nonzero(d['gw2'])
    ops.dense_saturated_rows()
    out = {}
    stored = ops.dense_norm(pend, d['w'], d['b'], d['gw'], d['gb'], G, eps, seg)
    out['raw'], out['table'] = stored.raw, stored.affines[0]
    _check(case, 'dense_norm raw', out['raw'], 'raw', T.F_PRODUCT)
    _check_table(case, 'dense_norm table', out['table'])
    out['normed'] = ops.group_norm_apply(ops.Pending(stored.raw, stored.affines, [1.0], seg), None, fs)
    _check(case, 'dense_norm + apply', out['normed'], 'normed', T.F_TABLE)
    stats = ops.dense_stats(pend, d['w'], d['b'], d['gw'], d['gb'], G, eps, seg)
    _check_table(case, 'dense_stats', stats)
    assert torch.equal(ops.dense_stats(pend, d['w'], d['b'], d['gw'], d['gb'], G, eps, seg), stats), name + ': the statistics repeat bit-identically'
    assert torch.equal(ops.dense_norm(pend, d['w'], d['b'], d['gw'], d['gb'], G, eps, seg).affines[0], out['table']), name
    stats2 = ops.dense_stats(d['x2'], d['w2'], d['b2'], d['gw2'], d['gb2'], G, eps, seg)
    _check_table(case, 'dense_stats shortcut', stats2, 'table2', 'raw2')
    out['stats'], out['stats2'] = stats, stats2
    for form in FORMS:
        out[form] = ops.dense_residual(pend, d['w'], stats, residual=d['residual'] if form == 'residual' else None,
                                       shortcut=(d['x2'], d['w2'], stats2) if form == 'shortcut' else None, final_slope=fs, segments=seg)
        _check(case, 'dense_residual ' + form, out[form], form, T.F_TABLE)
    out['linear'] = ops.linear_stream(d['x'], d['w'], d['b'])
    _check(case, 'linear_stream', out['linear'], 'linear', T.F_PRODUCT)
    out['linear relu'] = ops.linear_stream(d['x'], d['w'], d['b'], relu=True)
    _check(case, 'linear_stream relu', out['linear relu'], 'linear relu', T.F_PRODUCT)
    assert ops.dense_saturated_rows() == 0, name + ': every input is inside the headroom of its own scale'
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# rows against the row tile
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,position', [(N, i) for N in T.TILE_WIDTHS for i in range(5)])
def test_rows_against_the_row_tile(N, position):
    """1, TR - 1, TR, TR + 1 and 2 TR + 1 rows at TR = 128 (N = 32, 64, 128) and TR = 64 (N = 256, 512): a chunk shorter than a tile, a full
    one, a tile of one row behind full ones.  K = 32 (with rows <= TR the workgroup's whole walk is ONE K-step, three request steps
    behind it), 64, 1024; 0 / 1 / 2 pending stages with the slopes 0.0, 0.1 and 1.0."""
    rows = T.tile_row_counts(N)[position]
    for K in T.TILE_K:
        for form in range(3):
            _family('tile N %d rows %d K %d stages %d' % (N, rows, K, form))


# ---------------------------------------------------------------------------------------------------------------------------------------
# segments
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [64, 256, 1024])
def test_sixteen_segments_with_their_own_tables(N):
    """kGNMaxSegments = 16 segments of 1, TR - 1, TR, TR + 1 rows, one of half of all rows and short ones, out of order, two pending stages
    whose tables differ by an order of magnitude from one segment to the next.  N = 1024: 4 column blocks x 16 arrival counters live."""
    _family('segments N %d' % N)


def test_sixteen_column_blocks():
    """N = 4096 (the limit of 16 column blocks), K = 32, 65 rows: two tiles of one K-step each per column block, 128 groups."""
    _family('segments N 4096')


def test_refused_calls_leave_the_next_call_right():
    """17 segments, a segment table that does not cover the rows, N = 4352 (17 column blocks: dense_norm_ok is false): each is refused,
    and the good call behind it returns the bits of the good call in front (the arrival counters are back at zero)."""
    from se3et_amd import ops
    case = dict(T.case('segments N 64'), name='refusals, segments N 64')
    seg, G = case['segments'], case['groups']
    d, pend = _operands(case)
    stats = lambda p, s: ops.dense_stats(p, d['w'], d['b'], d['gw'], d['gb'], G, T.EPS, s)
    good = stats(pend, seg)
    _check_table(case, 'before the refusals', good)

    def with_segments(s):
        n = len(s) - 1
        aff = [torch.cat([a] * 2)[:n].contiguous().cuda() for a in case['affines']]
        return ops.Pending(d['x'], aff, list(case['slopes']), s)

    seventeen = [0, 2] + seg[1:]
    assert len(seventeen) == 18 and seg[1] == 5
    short = seg[:-1] + [seg[-1] - 1]
    for bad, match in ((seventeen, '17 segments'), (short, 'cover all')):
        with pytest.raises(RuntimeError, match=match):
            stats(with_segments(bad), bad)
        assert torch.equal(stats(pend, seg), good), match
        with pytest.raises(RuntimeError, match=match):
            ops.dense_norm(with_segments(bad), d['w'], d['b'], d['gw'], d['gb'], G, T.EPS, bad)
        assert torch.equal(stats(pend, seg), good), match
    g = torch.Generator().manual_seed(4352)
    w = (torch.randn(4352, 64, generator=g) / 8).cuda()
    gw, gb = torch.ones(4352).cuda(), torch.zeros(4352).cuda()
    assert not ops.dense_norm_ok(pend, w, 136)
    with pytest.raises(RuntimeError, match='output features'):
        ops.dense_stats(pend, w, None, gw, gb, 136, T.EPS, seg)
    assert torch.equal(stats(pend, seg), good)
    _check(case, 'after the refusals', ops.dense_residual(pend, d['w'], good, final_slope=case['final_slope'], segments=seg), 'nothing', T.F_TABLE)


# ---------------------------------------------------------------------------------------------------------------------------------------
# groups
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,groups', T.GROUP_SHAPES)
def test_channels_per_group_at_both_ends(N, groups):
    """1 and 32 channels per group at N = 32; 32 per group at N = 256, 1024 and 4096 (8, 32, 128 groups); 200 rows in two segments."""
    _family('groups N %d / %d' % (N, groups))


# ---------------------------------------------------------------------------------------------------------------------------------------
# statistics that cancel
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', T.OFFSETS)
def test_products_with_a_mean_far_above_their_sigma(offset):
    """x = randn + offset against weights of positive row sums: |mean| = 0.5 .. 1 x offset sigma per group.  F r without the cap."""
    _family('offset %g' % offset)


@pytest.mark.parametrize('kind', T.ZERO_KINDS)
def test_an_all_zero_segment_beside_a_live_one(kind):
    """Rows [0, 70) are exactly 0.  Without a layer bias, and with one that is constant inside every group, the segment has zero variance:
    its output is gb (+ residual), to the floor of the figure -- the raw product is exactly 0 and the shift exactly gb.  (With any other
    layer bias the segment's variance is the bias's own over the group's channels: judged against the twin like the live segment, whose
    figures are per block on its own scale.)"""
    case = T.case('zero segment ' + kind)
    out = _family('zero segment ' + kind)
    assert float(out['raw'][:70].abs().max()) == 0.0
    if kind == 'bias':
        return
    gb, res, fs = T.f64(case['gb']), T.f64(case['residual'][:70]), case['final_slope']
    assert torch.equal(out['stats'][0, 1].cpu(), case['gb'])
    floor = [T.allowed(0.0, T.F_TABLE)] * 3
    for form, want in (('nothing', T.lrelu(gb, fs).expand(70, -1)), ('residual', T.lrelu(gb + res, fs)), ('normed', T.lrelu(gb, fs).expand(70, -1))):
        k = T.error_figures(out[form][:70].cpu(), want, None, case['groups'])
        _judge('zero segment %s [%s = gb]' % (kind, form), [(n, e, 0.0, a) for n, e, a in zip(T.FIGURES, k, floor)])


# ---------------------------------------------------------------------------------------------------------------------------------------
# row scales in the final modes
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', T.SCALE_SHAPES)
@pytest.mark.parametrize('kind', T.SCALE_KINDS)
def test_scaled_rows_in_the_final_modes(kind, shape):
    """Rows at assorted tile positions, the last row of the partial last tile among them, that take a power-of-two scale of their own:
    `tiny start` (first 32 values of T(x) below 2^-4), T(x) about 2^-13 throughout, T(x) about 2^12 throughout -- through dense_residual
    with a residual tensor, with nothing and with a shortcut layer whose input rows are of unit size.  Each input is inside the headroom
    of its own scale, so no row may be counted as saturated, and every row is judged on its own (`per row`).  Shortcut norm weights of
    both signs, every fourth of size 1e-3."""
    case = T.case('%s (%d, %d, %d, %d)' % ((kind,) + shape))
    out = _family(case['name'])
    # the chosen rows on their own: each against its own largest entry
    for form in FORMS:
        got, want = out[form].cpu().double()[case['picked']], case['twin'][form][case['picked']]
        rest = case['restatement'][form][case['picked']]
        _judge('%s [dense_residual %s, the scaled rows]' % (case['name'], form), T.check(got, want, rest, T.F_TABLE))


@pytest.mark.parametrize('K,K2', T.UNIT_K_PAIRS)
def test_shortcut_layers_of_unequal_depth(K, K2):
    """(K, K2) = (32, 1024), (1024, 32), (64, 64) at unit magnitudes: one K-step of one source beside 32 of the other."""
    _family('unit K %d K2 %d' % (K, K2))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the rowops half
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rows_table(case, pending, convert):
    x = convert(case['x']).reshape(-1, case['x'].shape[-1])
    if pending:
        x = T.pending(x, [convert(case['affines'][0])], case['slopes'][:1], case['segments'])
    return x, T.group_norm_table(x, convert(case['xb']), convert(case['gw']), convert(case['gb']), case['groups'], case['eps'], case['segments'])


def _judge_stats(name, case, got, pending):
    raw64, want = _rows_table(case, pending, T.f64)
    _, rest = _rows_table(case, pending, T.f32)
    assert bool(torch.isfinite(got).all()), name
    _judge(name, T.check_table(got.cpu(), want, rest, raw64, case['segments'], case['groups']))


@pytest.mark.parametrize('C,groups,fast', T.STATS_CHANNELS)
def test_group_norm_stats_on_both_paths(C, groups, fast):
    """The float4 pass with the in-kernel finalize (C = 16, 1024) and the generic pass (C = 40, 48, 96), two segments, a layer bias: on a
    tensor and -- fast path only -- on a one-stage Pending.  A Pending on the generic path is refused, and the next call is right."""
    from se3et_amd import ops
    case = T.rows_case(45, C, groups, T.case_seed(9, C), [0, 6 * 17, 6 * 45])
    x, gw, gb, xb, aff = [_dev(case[k]) for k in ('x', 'gw', 'gb', 'xb')] + [case['affines'][0].cuda()]
    seg = case['segments']
    plain = ops.group_norm_stats(ops.Pending(x, [], [], seg), gw, gb, groups, T.EPS, x_bias=xb)
    _judge_stats('group_norm_stats C %d' % C, case, plain, False)
    assert torch.equal(ops.group_norm_stats(ops.Pending(x, [], [], seg), gw, gb, groups, T.EPS, x_bias=xb), plain)
    staged = ops.Pending(x, [aff], case['slopes'][:1], seg)
    if fast:
        _judge_stats('group_norm_stats C %d [one stage]' % C, case, ops.group_norm_stats(staged, gw, gb, groups, T.EPS, x_bias=xb), True)
    else:
        with pytest.raises(RuntimeError, match='pending input form'):
            ops.group_norm_stats(staged, gw, gb, groups, T.EPS, x_bias=xb)
        assert torch.equal(ops.group_norm_stats(ops.Pending(x, [], [], seg), gw, gb, groups, T.EPS, x_bias=xb), plain)


def test_group_norm_stats_on_a_misaligned_view():
    """C = 32 is a power of two, but a view that starts 4 bytes off a 16-byte boundary cannot be read as float4: the generic pass."""
    from se3et_amd import ops
    case = T.rows_case(45, 32, 4, T.case_seed(9, 32), [0, 6 * 17, 6 * 45])
    buf = torch.zeros(45 * 6 * 32 + 4).cuda()
    x = buf[1:1 + 45 * 6 * 32].view(45, 6, 32)
    x.copy_(case['x'])
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    gw, gb, xb = [_dev(case[k]) for k in ('gw', 'gb', 'xb')]
    got = ops.group_norm_stats(ops.Pending(x, [], [], case['segments']), gw, gb, 4, T.EPS, x_bias=xb)
    _judge_stats('group_norm_stats C 32 [misaligned]', case, got, False)
    aligned = ops.group_norm_stats(ops.Pending(case['x'].cuda(), [], [], case['segments']), gw, gb, 4, T.EPS, x_bias=xb)
    _judge_stats('group_norm_stats C 32 [aligned]', case, aligned, False)


@pytest.mark.parametrize('nstage', [1, 2])
@pytest.mark.parametrize('C,kind', T.APPLY_SHAPES)
def test_group_norm_apply_in_every_form_and_layout(C, kind, nstage):
    """One and two stages; no residual, a tensor, a Pending with its own table; a final slope; C = 4 and C = 1024; 16 segments and two.
    The blocked (kind 1, C % 16 == 0) and chunked (kind 2, C % 8 == 0) layouts, with and without segments of whole points: read
    through the twin's index maps they are the unblocked call bit for bit, and the magnitude word is the largest |value| of the
    kernel's own output, bit for bit."""
    from se3et_amd import ops
    case = T.apply_case(C, kind, nstage)
    seg, fs = case['segments'], case['final_slope']
    points = case['x'].shape[0]
    x, res, raff = case['x'].cuda(), case['residual'].cuda(), case['residual_affine'].cuda()
    aff = [a.cuda() for a in case['affines']]
    pend = ops.Pending(x, aff, case['slopes'], seg)
    residuals = {'none': (None, None, None), 'tensor': (res, case['residual'], None),
                 'pending': (ops.Pending(res, [raff], [1.0], seg), case['residual'], case['residual_affine'])}
    for name, (r_dev, r_host, r_aff) in residuals.items():
        run = lambda convert: T.apply(convert(case['x']), [convert(a) for a in case['affines']], case['slopes'], convert(r_host), convert(r_aff), fs, seg)
        got = ops.group_norm_apply(pend, r_dev, fs)
        assert bool(torch.isfinite(got).all())
        label = 'group_norm_apply C %d %s stages %d [residual %s]' % (C, kind, nstage, name)
        _judge(label, T.check(got.cpu(), run(T.f64), run(T.f32), T.F_PRODUCT, seg, 1))
        for layout, multiple in ((1, 16), (2, 8)):
            if C % multiple:
                continue
            blocked = ops.group_norm_apply(pend, r_dev, fs, blocked=True if layout == 1 else 2)
            assert blocked.kind == layout and blocked.shape == (points, 6, C)
            flat = blocked.data.flatten().cpu()
            assert torch.equal(flat[T.layout_index(layout, points, C)], got.cpu()), label + ': layout %d' % layout
            assert torch.equal(blocked.amax.cpu(), got.abs().max().reshape(1).cpu()), label + ': magnitude word of layout %d' % layout


# ---------------------------------------------------------------------------------------------------------------------------------------
# ops.group_norm_rows forward
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(T.ROWS_FORWARD))
def test_group_norm_rows_forward(name):
    """se3_group_norm_segments_fwd, the training and fallback path, on the cases that tests/test_gpu_backward_edges.py compares only the
    gradients of: C = 40 with 8 groups, 1024 with 2, one channel per group, 6 rows, 16 segments, x = randn + 10 / 100 / 1000, an
    all-zero segment.  No exemption at the LeakyReLU kink: the forward is continuous there."""
    from se3et_amd import ops
    c = T.rows_forward(name)
    case = c['case']
    got = ops.group_norm_rows(_dev(case['x']), _dev(case['weight']), _dev(case['bias']), c['groups'], T.EPS, c['slope'], _dev(case['residual']),
                              _dev(case['x_bias']), c['segments'])
    assert bool(torch.isfinite(got).all())
    _judge(name, T.check(got.cpu(), c['twin'], c['restatement'], T.F_TABLE, c['segments'], c['groups'], c['cancel']))
