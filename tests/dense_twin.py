"""The float64 twin of the dense + GroupNorm family (csrc/dense_norm.hip: dense_norm, dense_stats, dense_residual, linear_stream; the
statistics and apply half of csrc/rowops.hip: group_norm_stats, group_norm_apply, group_norm_rows; csrc/group_norm.h): plain PyTorch on the
CPU without a fused op, one function per operation, written out rather than calling se3et_amd.ops.  tests/test_dense_twin_cpu.py pins
the twin, the judge and the cases; tests/test_gpu_dense_edges.py holds the kernels to it.

    pending     v -> lrelu(v scale[seg] + shift[seg], slope), up to two stages, per (segment, channel)
    linear      y = x W^T (the layer's bias is never added to y: it shifts the GroupNorm's means and nothing else)
    table       scale = rstd gw, shift = gb + (x_bias - mean(y + x_bias)) scale; biased variance per (segment, group)
    apply       lrelu(T_b(T_a(raw)) + R, final slope), R a tensor, a raw tensor with its own table, or nothing

Every function follows the dtype of its inputs: called on a case converted with f64 it is the twin, with f32 the float32 restatement --
the yardstick `r` of the allowed error, never a figure of the kernel.

The judge has three figures: `global` and `per row` as tests/kpconv_twin.py, and `per block`: for every (segment, group) the largest
error of the block divided by the block's own largest |want|.  A table is judged by what it does: the kernel's table and the twin's are
applied to the twin's raw product in float64 and the difference is measured per (segment, group) -- the raw `shift` entries cancel by
design under a large mean.  Allowed: min(1e-4, F max(r, 1.2e-7)); F = 8 for a product (4: split products keep 2^-22 per term against
float32's 2^-24, x 2 for another association of the sums), 16 for anything behind a table that the kernel derived from its own
statistics (x 2 for the Welford merge order).  The cancellation cases drop the cap: F r, provided r < 1e-3.

The second half builds the cases that both test files share, from seeds; CASES names them so that the CPU test can hold each to its
claim."""
import functools

import torch

from attention_twin import CEILING, F32_EPS, SMALL_ROW
from backward_twin import F64, f32, f64                                   # noqa: F401

F_PRODUCT, F_TABLE = 8.0, 16.0
CANCEL_R = 1e-3               # a cancellation case must keep its restatement below this
EPS = 1e-5
TINY = 2.0 ** -4              # a row whose first 32 values are all below this takes a power-of-two scale of its own
MAX_SEGMENTS = 16


def tile_rows(N):
    """Rows per row tile of the dense kernel (dense_chunks in csrc/dense_norm.hip)."""
    return 64 if N >= 256 else 128


# ---------------------------------------------------------------------------------------------------------------------------------------
# the operations
# ---------------------------------------------------------------------------------------------------------------------------------------
def bounds(rows, segments):
    b = [int(v) for v in segments] if segments is not None else [0, rows]
    assert b[0] == 0 and b[-1] == rows and all(x < y for x, y in zip(b[:-1], b[1:])), (b, rows)
    return list(zip(b[:-1], b[1:]))


def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def per_segment(v, table, segments):
    """v (rows, C) * table[seg, 0] + table[seg, 1]."""
    out = torch.empty_like(v)
    for s, (a, b) in enumerate(bounds(v.shape[0], segments)):
        out[a:b] = v[a:b] * table[s, 0] + table[s, 1]
    return out


def pending(raw, affines, slopes, segments):
    """The stages v -> lrelu(v scale[seg] + shift[seg], slope) in order; raw (..., C), affines [(nseg, 2, C)], slopes [float]."""
    v = raw.reshape(-1, raw.shape[-1])
    for aff, slope in zip(affines, slopes):
        v = lrelu(per_segment(v, aff, segments), slope)
    return v.reshape(raw.shape)


def linear(x, w):
    return x @ w.t()


def group_norm_table(y, x_bias, gw, gb, groups, eps, segments):
    """(nseg, 2, N): the GroupNorm of y + x_bias over (rows of the segment x channels of the group) as the affine map of y."""
    rows, N = y.shape
    cpg = N // groups
    xb = x_bias if x_bias is not None else torch.zeros(N, dtype=y.dtype)
    out = []
    for a, b in bounds(rows, segments):
        g = (y[a:b] + xb).reshape(b - a, groups, cpg)
        mean = g.mean((0, 2))
        var = ((g - mean[None, :, None]) ** 2).mean((0, 2))
        rstd = 1.0 / torch.sqrt(var + eps)
        scale = rstd.repeat_interleave(cpg) * gw
        out.append(torch.stack((scale, gb + (xb - mean.repeat_interleave(cpg)) * scale)))
    return torch.stack(out)


def apply(raw, affines, slopes, residual, residual_affine, final_slope, segments):
    """lrelu(T_b(T_a(raw)) + R, final_slope); R = residual [scale_r[seg] + shift_r[seg]] or nothing."""
    shape = raw.shape
    v = pending(raw, affines, slopes, segments).reshape(-1, shape[-1])
    if residual is not None:
        r = residual.reshape(-1, shape[-1])
        v = v + (per_segment(r, residual_affine, segments) if residual_affine is not None else r)
    return lrelu(v, final_slope).reshape(shape)


def dense_norm(x, affines, slopes, w, b, gw, gb, groups, eps, segments):
    """-> (raw = T(x) W^T, table of GroupNorm(raw + b))."""
    raw = linear(pending(x, affines, slopes, segments), w)
    return raw, group_norm_table(raw, b, gw, gb, groups, eps, segments)


def dense_stats(x, affines, slopes, w, b, gw, gb, groups, eps, segments):
    return dense_norm(x, affines, slopes, w, b, gw, gb, groups, eps, segments)[1]


def dense_residual(x, affines, slopes, w, table, residual, shortcut, final_slope, segments):
    """lrelu(T(x) W^T scale + shift + R); R = residual, or shortcut = (x2, w2, table2): x2 W2^T scale_2 + shift_2, or nothing."""
    raw = linear(pending(x, affines, slopes, segments), w)
    if shortcut is not None:
        assert residual is None
        x2, w2, table2 = shortcut
        return apply(raw, [table], [1.0], linear(x2, w2), table2, final_slope, segments)
    return apply(raw, [table], [1.0], residual, None, final_slope, segments)


def group_norm_rows(x, weight, bias, residual, x_bias, groups, eps, slope, segments):
    """GroupNorm of x + x_bias, affine, [+ residual], [LeakyReLU] as table + apply."""
    x2 = x.reshape(-1, x.shape[-1])
    table = group_norm_table(x2, x_bias, weight, bias, groups, eps, segments)
    return apply(x, [table], [1.0], residual, None, 1.0 if slope is None else slope, segments)


def layout_index(kind, points, C):
    """The feature layouts of ops.BlockedFeatures as index maps: idx (points, 6, C) with plain[p, a, c] = data.flatten()[idx[p, a, c]].
    kind 1: [point][C / 16][anchor pair][16 channels][2 anchors]; kind 2: [point][C / 8][6 anchors][8 channels]."""
    p = torch.arange(points)[:, None, None]
    a = torch.arange(6)[None, :, None]
    c = torch.arange(C)[None, None, :]
    if kind == 1:
        return p * 6 * C + (c // 16) * 96 + (a // 2) * 32 + (c % 16) * 2 + a % 2
    assert kind == 2
    return p * 6 * C + (c // 8) * 48 + a * 8 + c % 8


# ---------------------------------------------------------------------------------------------------------------------------------------
# the error figures and the allowed error
# ---------------------------------------------------------------------------------------------------------------------------------------
FIGURES = ('global', 'per row', 'per block')


def error_figures(got, want, segments=None, groups=1):
    """(global, per row, per (segment, group)) of got against want (..., rows, N) read as rows x N.  global: max |got - want| /
    max |want|.  per row: the same per row, a row below SMALL_ROW of the tensor's maximum measured against that share.  per block: the
    same per (segment, group) block against the block's OWN largest |want| (a block that is all zero: any error is infinite)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    N = want.shape[-1]
    got, want = got.reshape(-1, N), want.reshape(-1, N)
    d = (got - want).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
    top = max(float(want.abs().max()), 1e-300)
    rows = torch.clamp(want.abs().amax(-1), min=SMALL_ROW * top)
    block = 0.0
    cpg = N // groups
    for a, b in bounds(want.shape[0], segments):
        e = d[a:b].reshape(b - a, groups, cpg).amax((0, 2))
        m = want[a:b].abs().reshape(b - a, groups, cpg).amax((0, 2))
        ratio = torch.where(e == 0, torch.zeros_like(e), e / m.clamp(min=1e-300))
        block = max(block, float(ratio.max()))
    return float(d.max()) / top, float((d.amax(-1) / rows).max()), block


def allowed(r, factor, cancel=False):
    """min(1e-4, factor max(r, 1.2e-7)); a cancellation case: factor r without the cap (its r is asserted below CANCEL_R)."""
    return factor * r if cancel else min(CEILING, factor * max(r, F32_EPS))


def check(got, want, restatement, factor, segments=None, groups=1, cancel=False):
    """-> [(figure name, kernel error, restatement error, allowed)] for the three figures."""
    k, r = error_figures(got, want, segments, groups), error_figures(restatement, want, segments, groups)
    return [(name, ke, re, allowed(re, factor, cancel)) for name, ke, re in zip(FIGURES, k, r)]


def table_effect(table, raw64, segments):
    """What a table does: applied to the twin's raw product in float64."""
    return per_segment(raw64, table.detach().cpu().double(), segments)


def check_table(got, want, restatement, raw64, segments, groups, cancel=False):
    """The three tables applied to the twin's raw product; the figures of the difference (the per block figure is the one that
    counts: a table is per (segment, channel))."""
    eff = lambda t: table_effect(t, raw64, segments)
    return check(eff(got), eff(want), eff(restatement), F_TABLE, segments, groups, cancel)


def rejected(figures):
    return any(not (k <= a) for _, k, _, a in figures)


# ---------------------------------------------------------------------------------------------------------------------------------------
# shared cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def case_seed(*v):
    s = 23
    for t in v:
        s = (s * 1000003 + int(t)) % (2 ** 31 - 1)
    return s


STAGE_FORMS = ((), (0.0,), (0.1, 1.0))          # the slopes of 0 / 1 / 2 pending stages: the limits the entry accepts and one inside


def dense_case(rows, K, N, groups, slopes, seed, segments=None, bias=True, K2=64, contrast=False):
    """One layer: x (rows, K), pending stages with `slopes`, weight (N, K), layer bias, GroupNorm weight / bias, a residual (rows, N)
    and a shortcut layer (x2 (rows, K2), w2, b2, gw2, gb2: norm weights of both signs, every fourth of size 1e-3).  contrast: the stage
    tables of neighbouring segments differ by an order of magnitude (x 0.3 / x 3), so that a table of the wrong segment shows."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    nseg = 1 if segments is None else len(segments) - 1
    x = rn(rows, K) * (1 + torch.rand(1, K, generator=g)) + 0.5 * rn(1, K)
    affines = []
    for _ in slopes:
        aff = rn(nseg, 2, K) * 0.3 + torch.tensor([1.0, 0.0])[None, :, None]
        if contrast:
            aff = aff * torch.tensor([0.3 if s % 2 else 3.0 for s in range(nseg)])[:, None, None]
        affines.append(aff.contiguous())
    gw2 = (torch.rand(N, generator=g) + 0.5) * torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
    gw2[1::4] *= 1e-3
    return dict(x=x, affines=affines, slopes=list(slopes), w=rn(N, K) / K ** 0.5, b=rn(N) if bias else None,
                gw=torch.rand(N, generator=g) + 0.5, gb=rn(N), groups=groups, eps=EPS, segments=segments, residual=rn(rows, N),
                x2=rn(rows, K2), w2=rn(N, K2) / K2 ** 0.5, b2=rn(N), gw2=gw2, gb2=rn(N), final_slope=0.1, cancel=False)


FLOAT_KEYS = ('x', 'w', 'b', 'gw', 'gb', 'residual', 'x2', 'w2', 'b2', 'gw2', 'gb2')


def evaluate(case, convert=f64):
    """Every output of the family on one case, in the dtype of `convert`: raw, table, table2 (the shortcut layer's), the three forms of
    dense_residual (each with the tables of the same dtype), linear_stream's out = x W^T + b and its ReLU."""
    c = {k: convert(case[k]) for k in FLOAT_KEYS}
    aff = [convert(a) for a in case['affines']]
    sl, seg, G, eps, fs = case['slopes'], case['segments'], case['groups'], case['eps'], case['final_slope']
    raw, table = dense_norm(c['x'], aff, sl, c['w'], c['b'], c['gw'], c['gb'], G, eps, seg)
    raw2, table2 = dense_norm(c['x2'], [], [], c['w2'], c['b2'], c['gw2'], c['gb2'], G, eps, seg)
    out = dict(raw=raw, table=table, raw2=raw2, table2=table2)
    out['normed'] = apply(raw, [table], [1.0], None, None, fs, seg)
    out['residual'] = dense_residual(c['x'], aff, sl, c['w'], table, c['residual'], None, fs, seg)
    out['nothing'] = dense_residual(c['x'], aff, sl, c['w'], table, None, None, fs, seg)
    out['shortcut'] = dense_residual(c['x'], aff, sl, c['w'], table, None, (c['x2'], c['w2'], table2), fs, seg)
    plain = linear(c['x'], c['w'])
    out['linear'] = plain + c['b'] if c['b'] is not None else plain
    out['linear relu'] = lrelu(out['linear'], 0.0)
    return out


def transformed(case):
    """T(x) in float64: what the kernel's f16 split sees."""
    return pending(f64(case['x']), [f64(a) for a in case['affines']], case['slopes'], case['segments'])


# ---- rows against the row tile --------------------------------------------------------------------------------------------------------
TILE_WIDTHS = (32, 64, 128, 256, 512)
TILE_K = (32, 64, 1024)


def tile_row_counts(N):
    TR = tile_rows(N)
    return (1, TR - 1, TR, TR + 1, 2 * TR + 1)


def _tile(N, rows, K, form):
    return dense_case(rows, K, N, max(1, N // 32), STAGE_FORMS[form], case_seed(1, N, rows, K, form))


# ---- segments -------------------------------------------------------------------------------------------------------------------------
def sixteen_lengths(N):
    """16 segment lengths out of order: 1, TR - 1, TR, TR + 1, one segment of half of all rows, the rest short."""
    TR = tile_rows(N)
    rest = [5, TR + 1, 1, 17, TR, 3, None, TR - 1, 9, 2, 33, 1, 7, 12, 20, 6]
    half = sum(v for v in rest if v is not None)
    return [half if v is None else v for v in rest]


def offsets(lengths):
    out = [0]
    for n in lengths:
        out.append(out[-1] + n)
    return out


def _segments(N, K=64, form=2):
    seg = offsets(sixteen_lengths(N))
    return dense_case(seg[-1], K, N, max(1, N // 32), STAGE_FORMS[form], case_seed(2, N, K), segments=seg, contrast=True)


def _wide():
    """N = 4096 (16 column blocks), K = 32, 65 rows: one K-step per tile, two tiles."""
    return dense_case(65, 32, 4096, 128, STAGE_FORMS[1], case_seed(2, 4096))


# ---- groups ---------------------------------------------------------------------------------------------------------------------------
GROUP_SHAPES = ((32, 32), (32, 1), (256, 8), (1024, 32), (4096, 128))          # (N, groups): 1 and 32 channels per group at both ends


def _groups(N, groups):
    return dense_case(200, 64, N, groups, STAGE_FORMS[2], case_seed(3, N, groups), segments=[0, 67, 200])


# ---- statistics that cancel -----------------------------------------------------------------------------------------------------------
OFFSETS = (10.0, 100.0, 1000.0)


def _offset(offset):
    """x = randn + offset against weights whose row sums are positive and equal inside a group (0.5 .. 1 from group to group): the
    product has mean = offset x row sum and sigma = |w row| ~ 1 per group, |mean| >> sigma."""
    case = dense_case(300, 32, 64, 8, (), case_seed(4, int(offset)), segments=[0, 129, 300])
    g = torch.Generator().manual_seed(case_seed(4, 1, int(offset)))
    case['x'] = torch.randn(300, 32, generator=g) + offset
    case['x2'] = torch.randn(300, 64, generator=g) + offset
    for name in ('w', 'w2'):
        w = case[name]
        sums = (0.5 + 0.5 * torch.rand(8, generator=g)).repeat_interleave(8)
        case[name] = (w + (sums - w.sum(1))[:, None] / w.shape[1]).contiguous()
    case['cancel'] = True
    return case


ZERO_KINDS = ('none', 'group bias', 'bias')


def _zero_segment(kind):
    """Rows [0, 70) all zero beside a live segment [70, 200), 8 channels per group.  `none`: no layer bias; `group bias`: a layer bias that
    is constant inside every group -- in both the zero segment has zero variance and its normalised value is gb; `bias`: any layer bias:
    the zero segment's variance is that of the bias over the group's channels, and its value (b - mean) rstd gw + gb."""
    case = dense_case(200, 64, 64, 8, (), case_seed(5, len(kind)), segments=[0, 70, 200], bias=kind != 'none')
    if kind == 'group bias':
        case['b'] = case['b'][::8].repeat_interleave(8).contiguous()
    case['x'][:70] = 0.0
    case['x2'][:70] = 0.0
    case['cancel'] = True                 # zero variance: rstd = 1 / sqrt(eps) multiplies every rounding of a float32 mean by 316
    return case


# ---- row scales in the final modes ----------------------------------------------------------------------------------------------------
def scaled_row_positions(rows):
    return [19, 20, 36, 51, 83, 100, rows // 2 + 3, rows - 7, rows - 1]


SCALE_SHAPES = ((300, 64, 128, 64), (150, 128, 256, 32))          # (rows, K, N, K2): both tile heights; rows - 1 is the last row of a partial tile
SCALE_KINDS = ('tiny start', 'main 2^-13', 'main 2^12')


def _scaled(kind, rows, K, N, K2):
    """One pending stage of slope 1 (an affine map, inverted here) in front of the layer.  `tiny start`: the first 32 values of T(x) of the
    chosen rows are +-(0.03 .. 0.06), below 2^-4, the rest of the row randn: inside the 2^8 of headroom above the first 32 values.  `main 2^-13` / `main 2^12`: T(x) of the chosen rows is
    randn x 2^-13 (x 2^12) THROUGHOUT while their x2 rows stay of unit size: each input is inside the headroom of its own scale."""
    case = dense_case(rows, K, N, max(1, N // 32), (1.0,), case_seed(6, len(kind), rows, N), K2=K2)
    g = torch.Generator().manual_seed(case_seed(6, 1, rows))
    sc, sh = case['affines'][0][0, 0].double(), case['affines'][0][0, 1].double()
    sc = torch.where(sc.abs() < 0.25, torch.full_like(sc, 0.25), sc)
    case['affines'][0][0, 0] = sc.float()
    sc = case['affines'][0][0, 0].double()
    picked = scaled_row_positions(rows)
    x = case['x'].double()
    for r in picked:
        if kind == 'tiny start':
            want = torch.randn(K, generator=g).double()
            sign = torch.where(torch.rand(32, generator=g) < 0.5, -1.0, 1.0).double()
            want[:32] = sign * (0.03 + 0.03 * torch.rand(32, generator=g).double())
            x[r] = (want - sh) / sc
        else:
            want = torch.randn(K, generator=g).double() * (2.0 ** -13 if kind == 'main 2^-13' else 2.0 ** 12)
            x[r] = (want - sh) / sc
    case['x'] = x.float()
    case['picked'] = picked
    return case


UNIT_K_PAIRS = ((32, 1024), (1024, 32), (64, 64))


def _unit_pair(K, K2):
    return dense_case(193, K, 128, 4, STAGE_FORMS[2], case_seed(7, K, K2), K2=K2)


# ---- the rowops half ------------------------------------------------------------------------------------------------------------------
STATS_CHANNELS = ((16, 4, True), (1024, 32, True), (40, 8, False), (48, 6, False), (96, 32, False))          # (C, groups, fast path)


def rows_case(points, C, groups, seed, segments=None, nstage=1):
    """x (points, 6, C) with a stage table per pending stage, GroupNorm parameters, a layer bias, a residual and a residual table."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    nseg = 1 if segments is None else len(segments) - 1
    tab = lambda: (rn(nseg, 2, C) * 0.3 + torch.tensor([1.0, 0.0])[None, :, None]).contiguous()
    return dict(x=rn(points, 6, C) * (1 + torch.rand(1, 1, C, generator=g)) + 0.5 * rn(1, 1, C), affines=[tab() for _ in range(nstage)],
                slopes=[0.1, 0.2][:nstage], gw=torch.rand(C, generator=g) + 0.5, gb=rn(C), xb=rn(C) * 0.5, groups=groups, eps=EPS,
                segments=segments, residual=rn(points, 6, C), residual_affine=tab(), final_slope=0.1)


APPLY_SHAPES = ((4, None), (1024, None), (32, 'sixteen'), (16, 'two'))          # (C, segments)


def point_segments(kind, points):
    """Row offsets of segments that are whole numbers of points."""
    if kind is None:
        return None
    if kind == 'two':
        return [0, 6 * (points // 3), 6 * points]
    from backward_twin import SIXTEEN_SEGMENTS
    assert points == SIXTEEN_SEGMENTS[-1] // 6
    return list(SIXTEEN_SEGMENTS)


def apply_case(C, kind, nstage):
    points = 40 if kind == 'sixteen' else 50
    return rows_case(points, C, 1, case_seed(8, C, nstage), point_segments(kind, points), nstage)


CASES = {}
CASES.update({'tile N %d rows %d K %d stages %d' % (N, rows, K, form): functools.partial(_tile, N, rows, K, form)
              for N in TILE_WIDTHS for rows in tile_row_counts(N) for K in TILE_K for form in range(3)})
CASES.update({'segments N %d' % N: functools.partial(_segments, N) for N in (64, 256, 1024)})
CASES['segments N 4096'] = _wide
CASES.update({'groups N %d / %d' % s: functools.partial(_groups, *s) for s in GROUP_SHAPES})
CASES.update({'offset %g' % o: functools.partial(_offset, o) for o in OFFSETS})
CASES.update({'zero segment %s' % k: functools.partial(_zero_segment, k) for k in ZERO_KINDS})
CASES.update({'%s (%d, %d, %d, %d)' % ((k,) + s): functools.partial(_scaled, k, *s) for k in SCALE_KINDS for s in SCALE_SHAPES})
CASES.update({'unit K %d K2 %d' % p: functools.partial(_unit_pair, *p) for p in UNIT_K_PAIRS})
CANCELLING = [n for n in CASES if n.startswith('offset') or n.startswith('zero segment')]
ORDINARY = [n for n in CASES if n not in CANCELLING]


@functools.lru_cache(maxsize=64)
def case(name):
    """The named case with its twin and its float32 restatement, computed once and shared (nobody changes them)."""
    c = CASES[name]()
    c['name'] = name
    c['twin'] = evaluate(c, f64)
    c['restatement'] = evaluate(c, f32)
    return c


# ---- ops.group_norm_rows forward on the cases of tests/backward_twin.py ----------------------------------------------------------------
def _rows_forward(builder, groups, slope, segments, cancel):
    return lambda: (builder(), groups, slope, segments, cancel)


def _rows_forward_cases():
    import backward_twin as B
    out = {}
    for rows, C, groups in B.GN_EDGE_SHAPES:
        for slope, with_res, with_xb in B.GN_VARIANTS:
            build = functools.partial(B.group_norm_case, rows, C, seed=rows, with_res=with_res, with_xb=with_xb)
            out['rows (%d, %d, %d) slope %s res %d xb %d' % (rows, C, groups, slope, with_res, with_xb)] = _rows_forward(build, groups, slope, None, False)
    for slope, with_res, with_xb in B.GN_VARIANTS:
        build = functools.partial(B.group_norm_case, 240, 32, seed=240, with_res=with_res, with_xb=with_xb)
        out['rows 16 segments slope %s res %d xb %d' % (slope, with_res, with_xb)] = _rows_forward(build, 4, slope, list(B.SIXTEEN_SEGMENTS), False)
    for offset in OFFSETS:
        out['rows x = randn + %g' % offset] = _rows_forward(functools.partial(B.group_norm_offset_case, offset), 4, 0.1, None, True)
    out['rows zero segment'] = _rows_forward(functools.partial(B.group_norm_case, 132, 32, seed=132, with_xb=False, zero_rows=(0, 60)), 4, 0.1,
                                             [0, 60, 132], True)
    return out


ROWS_FORWARD = _rows_forward_cases()
GN_NAMES = ('x', 'weight', 'bias', 'residual', 'x_bias')


@functools.lru_cache(maxsize=None)
def rows_forward(name):
    """-> dict(case, groups, slope, segments, cancel, twin, restatement): the twin is this module's group_norm_rows (pinned to the one of
    tests/backward_twin.py by the CPU test)."""
    case, groups, slope, segments, cancel = ROWS_FORWARD[name]()
    run = lambda convert: group_norm_rows(*[convert(case[k]) for k in GN_NAMES], groups, EPS, slope, segments)
    return dict(case=case, groups=groups, slope=slope, segments=segments, cancel=cancel, twin=run(f64), restatement=run(f32))
