"""GPU: the hand-written backward kernels of the training step (csrc/sinkhorn.hip sinkhorn_bwd_kernel; csrc/rowops.hip gn_bwd_*,
add_ln_bwd_kernel, neighbor_max_bwd_kernel, scatter_add_rows_fixed_kernel; csrc/kpconv_so3.hip kpconv_scatter_kernel; ops.mm_tn_splitk)
against the float64 twin (tests/backward_twin.py) at the shapes where the code takes another path and on inputs that make float32 sums
cancel.  tests/test_gpu_training.py compares the same kernels with the float32 restatement on generic random shapes.

Tolerances.  Benign inputs (unit-scale randn): the project's own figures, of the largest entry of the twin's result -- 2e-5 GroupNorm,
LayerNorm, KPConv, mm_tn_splitk; 1e-4 Sinkhorn (alpha: 1e-4 max(1, |d alpha|)); max-pool and row scatter exact where one contribution meets
an element, 1e-6 elsewhere.  Stress inputs (offset means, wide scores, mixed magnitudes): max(project figure, 4 x the error of the float32
restatement of se3et_amd/autograd.py, run on the CPU on the same inputs, against the twin) -- the factor 4 for another association of the
sums (chunk partials, wave butterflies) and the hardware exp / log; a wrong or missing term shows at 1e-3 or above.  With
SE3_BACKWARD_EDGES_PROBE=<file> every stress case appends its figures to that file (profiles/backward_edges_probe.txt was recorded so)."""
import os

import pytest
import torch

import backward_twin as T
from se3et_amd import autograd as AG

pytestmark = pytest.mark.gpu

EPS = 1e-5


def _dev(t):
    return None if t is None else t.cuda()


def _host(t):
    return None if t is None else t.detach().cpu().double()


def _err(got, want, keep=None):
    """max |got - want| over the kept elements / max |want| over all."""
    d = (got.double() - want.double()).abs()
    if keep is not None:
        d = d[keep]
    return float(d.max()) / max(float(want.abs().max()), 1e-300) if d.numel() else 0.0


def _stress(figure, restatement_err):
    return max(figure, 4.0 * restatement_err)


def _record(case, figures):
    """figures: [(name, kernel error, restatement error, allowed)] -> one line in the probe file."""
    for name, k, r, a in figures:
        print('%s %s: kernel %.3e restatement %.3e allowed %.3e' % (case, name, k, r, a))
    path = os.environ.get('SE3_BACKWARD_EDGES_PROBE')
    if path:
        with open(path, 'a') as f:
            f.write('%-34s %s\n' % (case, '   '.join('%s kernel %.2e restatement %.2e allowed %.2e' % fig for fig in figures)))


class _Switch:
    """ops.<name> = value inside the block."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        from se3et_amd import ops
        self.saved = getattr(ops, self.name)
        setattr(ops, self.name, self.value)

    def __exit__(self, *exc):
        from se3et_amd import ops
        setattr(ops, self.name, self.saved)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Sinkhorn
# ---------------------------------------------------------------------------------------------------------------------------------------
def _sinkhorn_kernels(case, iters):
    from se3et_amd import ops
    sc, rm, cm, al = _dev(case['scores']), _dev(case['row_masks']), _dev(case['col_masks']), _dev(case['alpha'])
    out = ops.log_optimal_transport(sc, rm, cm, al, iters, 1e12)
    ds, da = ops.log_optimal_transport_bwd(_dev(case['cot']), sc, rm, cm, al, iters, 1e12)
    return _host(out), _host(ds), _host(da)


def _check_sinkhorn(case, iters, name, stress=False):
    B, R, C = case['scores'].shape
    want = T.sinkhorn_twin(case, iters)
    got = _sinkhorn_kernels(case, iters)
    v, m = case['valid'], case['valid'][:, :R, :C]
    alpha_err = lambda g: abs(float(g[2]) - float(want[2])) / max(1.0, abs(float(want[2])))
    errs = lambda g: (_err(g[0][v], want[0][v]), _err(g[1][m], want[1][m]), alpha_err(g))
    k = errs(got)
    r = errs(T.sinkhorn_twin(case, iters, convert=T.f32)) if stress else (0.0, 0.0, 0.0)
    allowed = [_stress(1e-4, e) for e in r]
    if stress:
        _record(name, list(zip(('forward', 'd/dscores', 'd/dalpha'), k, r, allowed)))
    assert bool(torch.isfinite(got[1]).all()) and bool(torch.isfinite(got[2]))
    assert torch.equal(got[0] > -1e11, v), name
    if bool((~m).any()):
        assert float(got[1][~m].abs().max()) == 0.0, name + ': the gradient of a masked score must be exactly 0'
    for what, e, a in zip(('forward', 'd/dscores', 'd/dalpha'), k, allowed):
        assert e <= a, '%s %s: error %.3e > %.3e' % (name, what, e, a)


@pytest.mark.parametrize('R,C,iters', [(128, 128, 100), (71, 71, 100), (72, 71, 100), (71, 72, 30), (143, 143, 100), (1, 1, 100), (1, 143, 50),
                                       (64, 1, 50)])
def test_sinkhorn_at_the_patch_size_the_kernel_switch_and_the_limits(R, C, iters):
    """Both instantiations (<8, 9> up to 71 x 71, <4, 36> above) at the switch, at the 143 limit, at the KITTI patch size with its 100
    iterations of history in LDS, and at a single row / column; B = 3: random masks, and a last pair with exactly one valid row and column,
    not the first.  Forward and backward; the gradient of every masked score is exactly 0."""
    case = T.sinkhorn_case(3, R, C, seed=1000 * R + C)
    rm, cm = case['row_masks'], case['col_masks']
    assert int(rm[-1].sum()) == 1 and int(cm[-1].sum()) == 1 and int(rm.sum(1).min()) >= 1 and int(cm.sum(1).min()) >= 1
    assert (R == 1 or not bool(rm[-1, 0])) and (C == 1 or not bool(cm[-1, 0]))
    _check_sinkhorn(case, iters, 'sinkhorn %dx%dx%d' % (R, C, iters))


@pytest.mark.parametrize('size,scale', [(64, 10.0), (64, 30.0), (128, 10.0), (128, 30.0)])
def test_sinkhorn_with_wide_scores(size, scale):
    """Scores of 10 and 30 standard deviations through the forward (base 2, carried shifts) and the backward (__expf, exact maximum)."""
    case = T.sinkhorn_case(3, size, size, seed=size, scale=scale)
    _check_sinkhorn(case, 100, 'sinkhorn %dx%d scores x%g' % (size, size, scale), stress=True)


def test_sinkhorn_backward_refuses_a_history_that_does_not_fit():
    """100 iterations of 143 + 143 + 2 duals are 115 200 bytes of history and fit; 150 iterations of 128 + 128 + 2 are 154 800 against the
    153 600 that fit: an ordinary returned error, nothing launched, and the next call works."""
    from se3et_amd import ops
    assert 150 * (128 + 128 + 2) * 4 == 154800 > 150 * 1024 >= 100 * (143 + 143 + 2) * 4 == 115200
    case = T.sinkhorn_case(2, 128, 128, seed=5)
    args = [_dev(case[k]) for k in ('cot', 'scores', 'row_masks', 'col_masks', 'alpha')]
    with pytest.raises(RuntimeError, match='do not fit in LDS'):
        ops.log_optimal_transport_bwd(*args, 150, 1e12)
    torch.cuda.synchronize()
    ds, da = ops.log_optimal_transport_bwd(*args, 100, 1e12)
    want = T.sinkhorn_twin(case, 100)
    assert _err(_host(ds), want[1]) <= 1e-4
    big = T.sinkhorn_case(2, 143, 143, seed=6)
    ds, da = ops.log_optimal_transport_bwd(*[_dev(big[k]) for k in ('cot', 'scores', 'row_masks', 'col_masks', 'alpha')], 100, 1e12)
    assert bool(torch.isfinite(ds).all()) and bool(torch.isfinite(da))


# ---------------------------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------------------------------
GN_NAMES = ('x', 'weight', 'bias', 'residual', 'x_bias')


def _gn_kernel(case, groups, slope, segments):
    from se3et_amd import ops
    got = ops.group_norm_rows_bwd(_dev(case['cot']), _dev(case['x']), _dev(case['weight']), _dev(case['bias']), groups, EPS, slope,
                                  _dev(case['residual']), _dev(case['x_bias']), segments)
    return [_host(g) for g in got]


def _gn_restatement(case, groups, slope, segments):
    fn = lambda x, w, b, r, xb: AG.group_norm_rows(x, w, b, r, xb, groups, EPS, slope, segments)
    return T.vjp(fn, [case[k] for k in ('x', 'weight', 'bias', 'residual', 'x_bias')], case['cot'], T.f32)[1]


def _kink_allowance(case, pre, groups, slope, segments):
    """An element in the kink window may take either slope: its dz moves by up to (1 - slope) |dy|.  -> (window mask, what that can add to
    the dx of the other elements of its (segment, group) through the two group means (rows, C), per-channel additions for dweight, dbias,
    dx_bias)."""
    rows, C = case['x'].shape
    zero = torch.zeros(C, dtype=T.F64)
    kink = T.kink_mask(pre) if slope is not None else torch.zeros(rows, C, dtype=torch.bool)
    dx_extra = torch.zeros(rows, C, dtype=T.F64)
    if not bool(kink.any()):
        return kink, dx_extra, zero, zero, zero
    x = T.f64(case['x']) + (T.f64(case['x_bias']) if case['x_bias'] is not None else 0.0)
    w = T.f64(case['weight']).abs()
    jump = (1.0 - slope) * T.f64(case['cot']).abs() * kink
    dw_extra, db_extra, dxb_extra = zero.clone(), zero.clone(), zero.clone()
    bounds = list(segments) if segments is not None else [0, rows]
    cpg = C // groups
    for a, b in zip(bounds[:-1], bounds[1:]):
        g = x[a:b].reshape(b - a, groups, cpg)
        mean = g.mean((0, 2), keepdim=True)
        rstd = 1.0 / torch.sqrt(((g - mean) ** 2).mean((0, 2), keepdim=True) + EPS)
        xhat = ((g - mean) * rstd).reshape(b - a, C).abs()
        J = jump[a:b]
        K = (J * w).reshape(b - a, groups, cpg).sum((0, 2))                                       # largest change of sum_g (w dz)
        through_means = rstd.reshape(groups) * K / ((b - a) * cpg) * (1.0 + xhat.reshape(b - a, groups, cpg).amax((0, 2)) ** 2)
        dx_extra[a:b] = through_means.repeat_interleave(cpg)
        dw_extra += (J * xhat).sum(0)
        db_extra += J.sum(0)
        dxb_extra += (rstd.reshape(groups).repeat_interleave(cpg) * w * J).sum(0) + (b - a) * through_means.repeat_interleave(cpg)
    return kink, dx_extra, dw_extra, db_extra, dxb_extra


def _check_group_norm(case, groups, slope, segments, name, stress=False, rows=None):
    """All five gradients against the twin; rows: compare dx / dresidual on that row range only, relative to its own largest entry."""
    _, pre, want = T.group_norm_twin(case, groups, EPS, slope, segments)
    got = _gn_kernel(case, groups, slope, segments)
    kink, dx_extra, dw_extra, db_extra, dxb_extra = _kink_allowance(case, pre, groups, slope, segments)
    assert float(kink.double().mean()) <= T.KINK_CAP, name
    rest = _gn_restatement(case, groups, slope, segments) if stress else [None] * 5
    extras = (dx_extra, dw_extra, db_extra, 0.0, dxb_extra)
    figures = []
    for what, g, w_, r, extra in zip(GN_NAMES, got, want, rest, extras):
        if w_ is None:
            assert g is None
            continue
        assert bool(torch.isfinite(g).all()), '%s d/d%s is not finite' % (name, what)
        if what in ('x', 'residual'):
            sl = slice(*rows) if rows is not None else slice(None)
            g, w_, keep = g[sl], w_[sl], ~kink[sl]
            r = r[sl] if r is not None else None
            extra = extra[sl] if what == 'x' else extra
        else:
            keep = None
        scale = float(w_.abs().max())
        if what == 'x_bias' and groups == case['x'].shape[1]:
            # one channel per group: d x_bias[c] = sum_r dx[r, c] is the sum over a whole group, which is 0 identically -- the twin's
            # entries are its own rounding; the kernel's are held to the figure on the scale of the terms that cancel
            scale = float(want[0].abs().sum(0).max())
        r_err = _err(r, w_, keep) if r is not None else 0.0
        tol = _stress(2e-5, r_err)
        d = (g - w_).abs()
        if keep is not None:
            d = torch.where(keep, d, torch.zeros_like(d))
        figures.append((what, float(d.max()) / max(scale, 1e-300), r_err, tol))
        over = d > tol * scale + extra
        assert not bool(over.any()), '%s d/d%s: error %.3e of the largest entry > %.3e' % (name, what, float(d.max()) / scale, tol)
    if stress:
        _record(name, figures)


@pytest.mark.parametrize('rows,C,groups', T.GN_EDGE_SHAPES)
def test_group_norm_backward_branches(rows, C, groups):
    """512 channels per group (the strided loop of gn_bwd_finalize_kernel), one channel per group (256 chunk lanes), 5 channels per group
    (C no multiple of 64, no divisor of 256: the serial chunk loop), a single point (6 rows, shorter than one chunk): every combination of
    residual / bias of the producing layer / LeakyReLU that the existing test runs."""
    for slope, with_res, with_xb in T.GN_VARIANTS:
        case = T.group_norm_case(rows, C, seed=rows, with_res=with_res, with_xb=with_xb)
        _check_group_norm(case, groups, slope, None, 'group norm (%d, %d, %d) slope %s res %d xb %d' % (rows, C, groups, slope, with_res, with_xb))


def test_group_norm_backward_with_sixteen_segments():
    """kGNMaxSegments = 16 segments over 6 * 40 rows, one of a single point (6 rows), one holding half of all rows; 17 are refused."""
    from se3et_amd import ops
    for slope, with_res, with_xb in T.GN_VARIANTS:
        case = T.group_norm_case(240, 32, seed=240, with_res=with_res, with_xb=with_xb)
        _check_group_norm(case, 4, slope, T.SIXTEEN_SEGMENTS, 'group norm 16 segments slope %s res %d xb %d' % (slope, with_res, with_xb))
    case = T.group_norm_case(17 * 6, 32, seed=17)
    with pytest.raises(RuntimeError, match='17 segments'):
        ops.group_norm_rows_bwd(_dev(case['cot']), _dev(case['x']), _dev(case['weight']), _dev(case['bias']), 4, EPS, 0.1, _dev(case['residual']),
                                _dev(case['x_bias']), list(range(0, 18 * 6, 6)))


@pytest.mark.parametrize('offset', [10.0, 100.0, 1000.0])
def test_group_norm_backward_with_offset_inputs(offset):
    """x = randn + offset: the raw moment sums of the backward (t2 + shift * s1, e * x + f) cancel when |mean| >> sigma."""
    _check_group_norm(T.group_norm_offset_case(offset), 4, 0.1, None, 'group norm x = randn + %g' % offset, stress=True)


def test_group_norm_backward_with_an_all_zero_segment():
    """Rows [0, 60) are exactly 0 (mean 0, rstd = 1 / sqrt(eps)), rows [60, 132) live: dx of the zero segment is rstd (w dz - mean_g(w dz)),
    and the live segment, compared on its own scale (316 times smaller), is untouched by its neighbour."""
    case = T.group_norm_case(132, 32, seed=132, with_xb=False, zero_rows=(0, 60))
    segments = [0, 60, 132]
    _, pre, want = T.group_norm_twin(case, 4, EPS, 0.1, segments)
    dz = T.f64(case['cot'])[:60] * torch.where(pre[:60] > 0, torch.tensor(1.0, dtype=T.F64), torch.tensor(0.1, dtype=T.F64))
    wdz = (dz * T.f64(case['weight'])).reshape(60, 4, 8)
    closed = ((wdz - wdz.mean((0, 2), keepdim=True)) / EPS ** 0.5).reshape(60, 32)
    assert _err(want[0][:60], closed) <= 1e-12
    _check_group_norm(case, 4, 0.1, segments, 'group norm zero segment', rows=(0, 60))
    _check_group_norm(case, 4, 0.1, segments, 'group norm beside a zero segment', rows=(60, 132))
    assert float(want[0][:60].abs().max()) > 100 * float(want[0][60:].abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------------
# add + LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------------
LN_NAMES = ('hidden', 'residual', 'weight', 'bias', 'hidden_bias')


def _ln_case(shape, res_shape, C, with_hb, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return [rn(*shape, C), rn(*res_shape, C), rn(C), rn(C), rn(C) if with_hb else None], rn(*shape, C)


def _check_layer_norm(inputs, cot, name, live_rows=None):
    from se3et_amd import ops
    fn = lambda h, r, w, b, hb: T.add_layer_norm(h, r, w, b, hb, EPS)
    out, want = T.vjp(fn, inputs, cot)
    h, r, w, b, hb = [_dev(t) for t in inputs]
    fwd = _host(ops.add_layer_norm(h, r, w, b, EPS, hb))
    assert _err(fwd, out) <= 2e-5, '%s forward: %.3e' % (name, _err(fwd, out))
    runs = []
    for deterministic in (True, False):
        with _Switch('TRAINING_DETERMINISTIC', deterministic):
            got = [_host(g) for g in ops.add_layer_norm_bwd(_dev(cot), h, r, w, EPS, hb)]
        runs.append(got)
        for what, g, w_ in zip(LN_NAMES, got, want):
            if w_ is None:
                assert g is None
                continue
            assert g.shape == w_.shape and bool(torch.isfinite(g).all())
            e = _err(g, w_)
            assert e <= 2e-5, '%s (deterministic %s) d/d%s: error %.3e' % (name, deterministic, what, e)
            if live_rows is not None and what == 'hidden':
                e = _err(g.reshape(-1, g.shape[-1])[live_rows], w_.reshape(-1, g.shape[-1])[live_rows])
                assert e <= 2e-5, '%s (deterministic %s) d/dhidden, live rows: error %.3e' % (name, deterministic, e)
    for what, a, b_, w_ in zip(LN_NAMES, runs[0], runs[1], want):
        if w_ is not None:
            assert float((a - b_).abs().max()) <= 2e-6 * float(w_.abs().max()), '%s: the two variants differ in d/d%s' % (name, what)


@pytest.mark.parametrize('shape,res_shape,C,with_hb', [
    ((6, 5), (5,), 4, True), ((37,), (37,), 4, False), ((6, 5), (5,), 1024, False), ((37,), (37,), 1024, True), ((6, 5), (5,), 2048, True),
    ((37,), (37,), 2048, False), ((6, 41), (41,), 260, True), ((1,), (1,), 32, True)])
def test_layer_norm_backward_at_the_channel_limits(shape, res_shape, C, with_hb):
    """C = 4 (one lane of one vector), 1024 and 2048 (VPL 4 and 8, the limit), 260 (the tail of VPL 2), fewer rows than the 32 one workgroup
    walks and 37 (two workgroups, the second with 5 rows), a single row; the residual broadcast over the anchor axis; both forms of the
    parameter sums (per-workgroup partials, float atomics)."""
    inputs, cot = _ln_case(shape, res_shape, C, with_hb, seed=C + len(shape))
    _check_layer_norm(inputs, cot, 'layer norm %s C %d' % (shape, C))


def test_layer_norm_backward_with_an_all_zero_row():
    """hidden + residual exactly 0 in one row (mean 0, variance 0, rstd = 1 / sqrt(eps)) among live rows."""
    inputs, cot = _ln_case((6, 5), (5,), 64, False, seed=64)
    inputs[0][2, 3] = 0.0
    inputs[1][3] = 0.0
    live = torch.ones(30, dtype=torch.bool)
    live[2 * 5 + 3] = False
    _check_layer_norm(inputs, cot, 'layer norm zero row', live_rows=live)


@pytest.mark.parametrize('C', [2052, 6])
def test_layer_norm_backward_refuses_unsupported_channel_counts(C):
    from se3et_amd import ops
    inputs, cot = _ln_case((3,), (3,), C, False, seed=C)
    h, r, w, b, _ = [_dev(t) for t in inputs]
    for deterministic in (True, False):
        with _Switch('TRAINING_DETERMINISTIC', deterministic):
            with pytest.raises(RuntimeError, match='channels %d' % C):
                ops.add_layer_norm_bwd(_dev(cot), h, r, w, EPS, None)


# ---------------------------------------------------------------------------------------------------------------------------------------
# neighbour max-pool and the row scatter
# ---------------------------------------------------------------------------------------------------------------------------------------
def _assert_scatter(got, want, count, name):
    """Exact where at most one contribution meets an element, 1e-6 of the largest entry elsewhere."""
    single = count <= 1
    assert torch.equal(got[single], want[single]), name + ': elements with one contribution must be exact'
    if bool((~single).any()):
        e = float((got - want).abs().max())
        assert e <= 1e-6 * float(want.abs().max()), '%s: error %.3e of the largest entry' % (name, e / float(want.abs().max()))


def _check_max_pool(x, idx, cot, name, want_dx=None):
    from se3et_amd import ops
    out, (dx, _) = T.vjp(T.neighbor_max_pool, [x, idx], cot)
    if want_dx is not None:
        assert torch.equal(dx, want_dx)
    count = T.max_pool_winners(x, idx)
    fwd = _host(ops.neighbor_max_pool(_dev(x), _dev(idx)))
    assert torch.equal(fwd, out), name + ' forward'
    for deterministic in (True, False):
        with _Switch('TRAINING_DETERMINISTIC', deterministic):
            got = _host(ops.neighbor_max_pool_bwd(_dev(x), _dev(idx), _dev(cot)))
        _assert_scatter(got, dx, count, '%s (deterministic %s)' % (name, deterministic))
    return dx, count


def _pool_table(m, nn, n, g):
    """Random table over rows 0 .. n - 1, padding (n) and trailing -1 markers; row 1 is padding only, row 2 markers only."""
    idx = torch.randint(0, n + 1, (m, nn), generator=g)
    if nn > 1:
        width = torch.randint(1, nn + 1, (m,), generator=g)
        idx[torch.arange(nn)[None, :] >= width[:, None]] = -1
    idx[1], idx[2] = n, -1
    return idx


@pytest.mark.parametrize('nn', [1, 64])
@pytest.mark.parametrize('tail', [(6,), (7,), (6, 16)])
def test_max_pool_backward_at_the_table_limits(nn, tail):
    """nn = 1 and nn = 64 (the limit); widths 6 and 7 (the forward's scalar path) and 96 (its float4 path); a row of padding only, a row of -1
    markers only; forward and backward, both forms of the sums."""
    g = torch.Generator().manual_seed(100 * nn + len(tail) + tail[0])
    n, m = 50, 40
    x = torch.randn(n, *tail, generator=g)
    idx = _pool_table(m, nn, n, g)
    dx, _ = _check_max_pool(x, idx, torch.randn(m, *tail, generator=g), 'max pool nn %d width %s' % (nn, tail))
    assert float(dx.abs().max()) > 0.0


def test_max_pool_backward_ties():
    """Three tied real neighbours: the first in table order takes all; a real 0.0 in front of a padded entry takes it; behind one, nothing
    flows; a -1 marker never wins."""
    x, idx, cot, want = T.max_pool_tie_cases()
    _check_max_pool(x, idx, cot, 'max pool ties', want_dx=want)


def test_max_pool_backward_many_rows_into_one_and_the_neighbour_limit():
    """300 rows pool the same support row: 300 contributions meet in each of its positive elements (its negative ones lose to the padded 0);
    nn = 65 is refused."""
    from se3et_amd import ops
    g = torch.Generator().manual_seed(300)
    n, m = 20, 300
    x = torch.randn(n, 6, 4, generator=g)
    idx = torch.full((m, 3), n, dtype=torch.int64)
    idx[:, 1] = 7
    cot = torch.randn(m, 6, 4, generator=g)
    dx, count = _check_max_pool(x, idx, cot, 'max pool 300 rows into one')
    assert torch.equal(count[7] == 300, x[7] > 0) and int(count.sum()) == 300 * int((x[7] > 0).sum())
    wide = torch.zeros(4, 65, dtype=torch.int64).cuda()
    for deterministic in (True, False):
        with _Switch('TRAINING_DETERMINISTIC', deterministic):
            with pytest.raises(RuntimeError, match='nn <= 64'):
                ops.neighbor_max_pool_bwd(_dev(x), wide, _dev(cot[:4]))
    with pytest.raises(RuntimeError, match='nn <= 64'):
        ops.neighbor_max_pool(_dev(x), wide)


@pytest.mark.parametrize('tail', [(6,), (7,), (6, 16)])
def test_scatter_add_rows_against_the_twin(tail):
    """The transpose of the padded gather: a one-column and a many-column table with padding and -1 markers, and 300 rows into one."""
    from se3et_amd import ops
    g = torch.Generator().manual_seed(7 + tail[0] + len(tail))
    n = 50
    tables = [_pool_table(40, 1, n, g)[:, 0], _pool_table(40, 64, n, g), torch.full((300,), 7, dtype=torch.int64)]
    for idx in tables:
        cot = torch.randn(*idx.shape, *tail, generator=g)
        want = T.vjp(T.gather_rows_padded, [torch.zeros(n, *tail), idx], cot)[1][0]
        count = torch.bincount(idx[(idx >= 0) & (idx < n)].reshape(-1), minlength=n).reshape((n,) + (1,) * len(tail)).expand_as(want)
        for deterministic in (True, False):
            with _Switch('TRAINING_DETERMINISTIC', deterministic):
                got = _host(ops.scatter_add_rows(_dev(cot), _dev(idx), n))
            _assert_scatter(got, want, count, 'scatter_add_rows %s width %s' % (tuple(idx.shape), tail))


# ---------------------------------------------------------------------------------------------------------------------------------------
# KPConv
# ---------------------------------------------------------------------------------------------------------------------------------------
def _kpconv_kernel(case, deterministic):
    from se3et_amd import ops
    with _Switch('KPCONV_BACKWARD_DETERMINISTIC', deterministic):
        dx, dw = ops.kpconv_inter_so3_bwd(*[_dev(case[k]) for k in ('cot', 'x', 'q_pts', 's_pts', 'idx', 'kernel_points', 'weights', 'kidx', 'ridx')],
                                          case['sigma'])
    return _host(dx), _host(dw)


@pytest.mark.parametrize('P,Ns,NN,Cin,Cout', [(1, 30, 20, 16, 32), (40, 60, 64, 8, 32), (40, 60, 1, 8, 16), (50, 80, 24, 1, 16), (64, 64, 30, 32, 40)])
def test_kpconv_backward_at_the_shape_limits(P, Ns, NN, Cin, Cout):
    """One query; NN = 64 (kMaxNN) with more columns than support points; NN = 1; Cin = 1 (the first layer: 6 columns on 64 threads);
    Cout = 40 (no multiple of 32: dG through the library product).  dx and dW, fixed-point and float-atomic scatter."""
    case = T.kpconv_case(P, Ns, NN, Cin, Cout, seed=P + NN + Cin)
    assert int((case['idx'] < Ns).sum()) > 0
    _, dx, dw = T.kpconv_twin(case)
    for deterministic in (True, False):
        got = _kpconv_kernel(case, deterministic)
        for what, g, w_ in (('dL/dx', got[0], dx), ('dL/dW', got[1], dw)):
            e = _err(g, w_)
            assert e <= 2e-5, 'kpconv (%d, %d, %d, %d, %d) deterministic %s %s: error %.3e' % (P, Ns, NN, Cin, Cout, deterministic, what, e)


def test_kpconv_backward_with_queries_that_see_only_padding():
    case = T.kpconv_blind_case()
    Ns = case['x'].shape[0]
    assert bool((case['idx'][::3] == Ns).all())
    seen = torch.zeros(Ns + 1, dtype=torch.bool)
    seen[case['idx'].reshape(-1)] = True
    _, dx, dw = T.kpconv_twin(case)
    assert float(dx[~seen[:Ns]].abs().max()) == 0.0
    for deterministic in (True, False):
        got = _kpconv_kernel(case, deterministic)
        assert float(got[0][~seen[:Ns]].abs().max()) == 0.0, 'support rows that nobody gathers must stay exactly 0'
        assert _err(got[0], dx) <= 2e-5 and _err(got[1], dw) <= 2e-5, deterministic


def test_kpconv_backward_with_mixed_magnitudes():
    """The cotangent is of unit scale, except that one query's rows are scaled by 1e6.  The float-atomic scatter is held to the stress
    tolerance.  The fixed-point scatter takes its scale from max |dout| max |W| Cout of the whole call, so a support row that only quiet
    queries reach is resolved on the loud query's scale: csrc/kpconv_so3.hip documents bound 2^-(54 - 7 - ceil(log2(P + 1))) per
    contribution (derived from csrc/common.h: scale exponent 61 - (exponent of the bound + 7 + ceil(log2(P + 1)))), and that, times the
    contributions meeting in the element, is what the quiet rows may lose on top of the float32 figure of their own scale (2e-5 of the
    largest quiet entry: nothing loud enters them, in either form of the sums)."""
    case, loud, reached = T.kpconv_mixed_case()
    _, dx, dw = T.kpconv_twin(case)
    _, rdx, rdw = T.kpconv_twin(case, T.f32)
    r_dx, r_dw = _err(rdx, dx), _err(rdw, dw)
    tol_dx, tol_dw = _stress(2e-5, r_dx), _stress(2e-5, r_dw)
    resolution, count = T.kpconv_fixed_resolution(case)
    quiet = ~reached
    quiet_scale = float(dx[quiet].abs().max())
    assert float(dx[reached].abs().max()) > 1e4 * quiet_scale > 0.0
    figures = []
    for deterministic in (True, False):
        got_dx, got_dw = _kpconv_kernel(case, deterministic)
        d = (got_dx - dx).abs()
        form = 'fixed' if deterministic else 'float'
        figures += [('dx %s' % form, float(d.max()) / float(dx.abs().max()), r_dx, tol_dx),
                    ('dx %s, quiet rows' % form, float(d[quiet].max()) / quiet_scale, _err(rdx[quiet], dx[quiet]), 2e-5)]
        if deterministic:
            figures.append(('dW', _err(got_dw, dw), r_dw, tol_dw))
        fixed = count.double().reshape(-1, 1, 1) * resolution if deterministic else torch.zeros(count.shape[0], 1, 1, dtype=T.F64)
        assert not bool((d[reached] > tol_dx * float(dx.abs().max()) + fixed[reached]).any()), (form, figures)
        assert not bool((d[quiet] > 2e-5 * quiet_scale + fixed[quiet]).any()), (form, figures)
        assert _err(got_dw, dw) <= tol_dw, (form, figures)
    figures.append(('fixed-point resolution x most contributions / quiet scale', float(count.max()) * resolution / quiet_scale, 0.0, 0.0))
    _record('kpconv one query x 1e6', figures)


# ---------------------------------------------------------------------------------------------------------------------------------------
# ops.mm_tn_splitk
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [32768 + 36, 32768, 32767])
def test_mm_tn_splitk_with_split_and_tail(K):
    """64 splits of 512 rows and a tail of 36; 64 splits, no tail; one row fewer: the library path (K // 64 < 512).  M = N = 32."""
    from se3et_amd import ops
    g = torch.Generator().manual_seed(K)
    a, b = torch.randn(K, 32, generator=g), torch.randn(K, 32, generator=g)
    assert (K // 64 >= 512) == (K >= 32768) and (K - 64 * (K // 64) > 0) == (K != 32768)
    want = a.double().t() @ b.double()
    e = _err(_host(ops.mm_tn_splitk(_dev(a), _dev(b))), want)
    assert e <= 2e-5, 'mm_tn_splitk K = %d: error %.3e' % (K, e)
