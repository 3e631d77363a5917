"""GPU: every form of the KPConvInterSO3 forward (ops.kpconv_inter_so3: the fused kernel of csrc/kpconv_mfma.hip, its two-launch `sums`
form, the gather + GEMM path of csrc/kpconv_so3.hip, the union kernel of csrc/kpconv_union.hip) against the float64 twin
(tests/kpconv_twin.py) where the schedule branches: points put exactly on 0, 1, 7 .. 64 valid neighbours with the valid entries at the
back of their lists, tables of 32 / 40 / 80 slots, odd chunk counts and K-split consumers, empty tiles and tiles of one point, the channel
split at z = 2 / 4 / 8, union plans at the cap, a row named several times by one list, plain inputs of any magnitude, the first layer.
tests/test_gpu_ops.py compares the same kernels on random geometry with one figure per tensor.

Every output is judged in two figures (kpconv_twin.error_figures): `global`, max |got - want| / max |want|, and `per row`, the same per
output row (point, anchor), a row below 1e-3 of the tensor's maximum measured against that share.  Allowed, for both:
min(1e-4, 16 x max(r, 1.2e-7)), r the same figure of the float32 restatement (se3et_amd.autograd.kpconv_inter_so3 on the CPU) against the
twin; 16 = 4 (split products keep 2^-22 per term against float32's 2^-24) x 2 (two split stages) x 2 (another association of the sums).
The rows of a point without a valid neighbour must be exactly 0.  tests/test_kpconv_twin_cpu.py holds every case to its claimed counts
and shows that the cap never decides.  With SE3_KPCONV_EDGES_PROBE=<file> every case appends its figures to that file
(profiles/kpconv_edges_probe.txt was recorded so)."""
import contextlib
import os

import numpy as np
import pytest
import torch

import kpconv_twin as T

pytestmark = pytest.mark.gpu

FORMS = ('fused', 'sums', 'gemm', 'union')
_SWITCH = {'fused': (True, False), 'sums': ('sums', False), 'gemm': (False, False), 'union': (True, True)}      # (KPCONV_MATRIX_CORE, union)


@contextlib.contextmanager
def _switches(form, split=True):
    from se3et_amd import ops
    saved = (ops.KPCONV_MATRIX_CORE, ops.KPCONV_UNION, ops.KPCONV_UNION_ALL, ops.KPCONV_SPLIT)
    try:
        ops.KPCONV_MATRIX_CORE, union = _SWITCH[form]
        ops.KPCONV_UNION = ops.KPCONV_UNION_ALL = union
        ops.KPCONV_SPLIT = split
        yield
    finally:
        ops.KPCONV_MATRIX_CORE, ops.KPCONV_UNION, ops.KPCONV_UNION_ALL, ops.KPCONV_SPLIT = saved


def _accepts(form, case):
    Cin, Cout = case['weights'].shape[2:]
    return form == 'gemm' or (Cin % 8 == 0 and Cout % 32 == 0)


def _device(case):
    return T.args(case, lambda t: t.cuda())


def _run(case, form, dev, x=None, split=True, grad=False):
    """One call of the operator in the given form -> the output on the CPU.  x: another first argument (a blocked layout)."""
    from se3et_amd import functional as SF
    from se3et_amd import ops
    with _switches(form, split), torch.set_grad_enabled(grad):
        if form == 'union':
            order = ops.register_point_order(dev[1], case['lens'], T.RADIUS / 2.5)
            assert order is not None and ops.point_order(dev[1]) is not None
        return SF.kpconv_inter_so3(dev[0] if x is None else x, *dev[1:]).cpu()


def _blocked(case, kind):
    from se3et_amd import ops
    x = case['x']
    Ns, _, Cin = x.shape
    if kind == 1:
        data = x.view(Ns, 3, 2, Cin // 16, 16).permute(0, 3, 1, 4, 2).contiguous()
    else:
        data = x.view(Ns, 6, Cin // 8, 8).permute(0, 2, 1, 3).contiguous()
    xb = ops.BlockedFeatures(data.cuda(), (Ns, 6, Cin), kind)
    assert torch.equal(xb.plain().cpu(), x)
    return xb


def _record(name, figures):
    for fig in figures:
        print('%s %s: kernel %.3e restatement %.3e allowed %.3e' % ((name,) + fig))
    path = os.environ.get('SE3_KPCONV_EDGES_PROBE')
    if path:
        with open(path, 'a') as f:
            f.write('%-44s %s\n' % (name, '   '.join('%s kernel %.2e restatement %.2e allowed %.2e' % fig for fig in figures)))


def _judge(case, what, got):
    """Both figures of one output against the case's twin, recorded, then asserted; the rows of empty points exactly 0."""
    name = '%s [%s]' % (case['name'], what)
    assert got.shape == case['twin'].shape
    assert bool(torch.isfinite(got).all()), name + ' is not finite'
    figures = T.check(got, case['twin'], case['restatement'])
    _record(name, figures)
    empty = torch.tensor(case['counts']) == 0
    if bool(empty.any()):
        assert float(got[empty].abs().max()) == 0.0, name + ': the rows of a point without a valid neighbour must be exactly 0'
    for fig, k, r, a in figures:
        assert k <= a, '%s %s: error %.3e > %.3e (restatement %.3e)' % (name, fig, k, a, r)


def _same(got, want, what):
    """Bit equality, with the points that differ in the message."""
    if not torch.equal(got, want):
        d = (got - want).abs().amax((1, 2))
        raise AssertionError('%s: max difference %.3e at points %s' % (what, float(d.max()), d.nonzero().flatten().tolist()[:20]))


def _all_forms(name, forms=FORMS, blocked=True):
    """Every form that accepts the case's shape, judged; the bit equalities of the older tests: repeats of the fused and union calls, the
    blocked layouts (kind 1 into the fused kernel, kinds 2 and 1 into the union kernel) against the plain tensor.  -> {form: output}."""
    case = T.case(name)
    dev = _device(case)
    Cin = case['x'].shape[2]
    outs = {}
    for form in forms:
        if not _accepts(form, case):
            continue
        outs[form] = _run(case, form, dev)
        _judge(case, form, outs[form])
    if 'fused' in outs:
        _same(_run(case, 'fused', dev), outs['fused'], name + ': the fused kernel repeats bit-identically')
        if blocked and Cin % 16 == 0:
            _same(_run(case, 'fused', dev, x=_blocked(case, 1)), outs['fused'], name + ': blocked kind 1 = plain')
    if 'union' in outs:
        _same(_run(case, 'union', dev), outs['union'], name + ': the union kernel repeats bit-identically')
        if blocked:
            _same(_run(case, 'union', dev, x=_blocked(case, 2)), outs['union'], name + ': blocked kind 2 = plain')
        if blocked and Cin % 16 == 0:
            _same(_run(case, 'union', dev, x=_blocked(case, 1)), outs['union'], name + ': a kind-1 input is converted')
    return outs


# ---------------------------------------------------------------------------------------------------------------------------------------
# the count ladder
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Cin,Cout', T.LADDER_CHANNELS)
@pytest.mark.parametrize('NN', T.LADDER_NN)
def test_count_ladder(NN, Cin, Cout):
    """P = 48 points on every count of {0, 1, 7, 8, 9, 31, 32, 33, 39, 40, 41, 63, 64} that NN allows, Ns = 96: nv > 0, nv > 32 (the tail
    slot pair of the EXT rounds), S rd < nv with S = 32 and 40 (the further rounds), NNp = 32 / 40 / 80; channel pairs with 1, 3, 2, 4
    and 8 chunks and column tiles (odd chunk counts, K-split consumers)."""
    outs = _all_forms('ladder NN %d (%d, %d)' % (NN, Cin, Cout))
    assert set(outs) == set(FORMS)


# ---------------------------------------------------------------------------------------------------------------------------------------
# tiles
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [str(p) for p in T.TILE_POINTS] + ['empty-middle', 'last-one-64'])
def test_tiles(kind):
    """P = 1, 15, 16, 17, 33 at NN = 38; a middle tile of 16 points without a valid neighbour; a last tile of one point with 64."""
    case = T.case('tiles ' + kind)
    if kind == 'empty-middle':
        assert case['counts'][16:32] == [0] * 16 and min(case['counts'][:16] + case['counts'][32:]) == 0 < max(case['counts'])
    if kind == 'last-one-64':
        assert len(case['counts']) == 33 and case['counts'][32] == 64
    assert set(_all_forms('tiles ' + kind)) == set(FORMS)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the channel split
# ---------------------------------------------------------------------------------------------------------------------------------------
def _split_factor(nbytes, tiles, Cout):
    z, rest = divmod(nbytes - 65536, tiles * 16 * 6 * Cout * 4)
    assert nbytes > 65536 and rest == 0
    return z


def test_channel_split_shapes_reach_every_factor():
    """z = (bytes - 65536) / (tiles . 16 . 6 . Cout . 4) of both kernels' workspaces: 2, 4 and 8 each occur, on one tile and on three."""
    from se3et_amd import ops
    for P in (9, 40):
        tiles = (P + 15) // 16
        shapes = [s for s in T.SPLIT_SHAPES if s[0] == P]
        fused = [_split_factor(ops.lib().se3_kpconv_fused_split_workspace_bytes(P, ci, co), tiles, co) for _, ci, co in shapes]
        union = [_split_factor(ops.lib().se3_kpconv_union_split_workspace_bytes(tiles, ci, co), tiles, co) for _, ci, co in shapes]
        assert fused == [2, 4, 8] and union == [2, 4, 8], (P, fused, union)


@pytest.mark.parametrize('P,Cin,Cout', T.SPLIT_SHAPES)
def test_channel_split(P, Cin, Cout):
    """Few tiles: the input channels are split over z workgroups whose partial sums the last one adds in a fixed order.  The split result
    against the twin (both kernels), bit-identical when repeated, within 5e-6 of the unsplit form."""
    from se3et_amd import ops
    name = 'split P %d (%d, %d)' % (P, Cin, Cout)
    case = T.case(name)
    tiles = (P + 15) // 16
    assert ops.lib().se3_kpconv_fused_split_workspace_bytes(P, Cin, Cout) and ops.lib().se3_kpconv_union_split_workspace_bytes(tiles, Cin, Cout)
    outs = _all_forms(name)                                # (the repeats inside are the split form's)
    dev = _device(case)
    top = float(case['twin'].abs().max())
    for form in ('fused', 'union'):
        whole = _run(case, form, dev, split=False)
        _judge(case, form + ' unsplit', whole)
        assert float((whole - outs[form]).abs().max()) <= 5e-6 * top, form
        assert torch.equal(_run(case, form, dev), outs[form]), form + ': the arrival counters are back at zero'


# ---------------------------------------------------------------------------------------------------------------------------------------
# the union plan
# ---------------------------------------------------------------------------------------------------------------------------------------
def _plan_passes(dev, G):
    """nsub of every group, read from the plan of the last union call on this stream (csrc/kpconv_union.hip: PlanViews)."""
    from se3et_amd import ops
    plan = ops._union_plans.entry(ops._stream().value)[1].cpu().numpy()
    a16 = lambda v: (v + 15) & ~15
    return plan[a16(G * 64):a16(G * 64) + 4 * G].view(np.int32).tolist()


@pytest.mark.parametrize('kind', list(T.UNION_PLANS))
def test_union_plan(kind):
    """Clouds of 1, 16, 17 and 31 points in one stack (every cloud starts a group: 6 groups, 31 padding positions); a group of 16 disjoint
    lists of 8 rows, whose union is exactly kUCap = 128 (one pass); the same with one more row (it splits in two); 16 disjoint lists of
    64 (the halving goes down to PAIRS of points, whose 2 x 64 rows are exactly the cap: 8 passes -- with at most 64 neighbours two lists
    always fit, so a pass of a single point and kMaxSub = 16 passes cannot be reached); every point the same 64 rows (one pass)."""
    from se3et_amd import ops
    name = 'union ' + kind
    case = T.case(name)
    outs = _all_forms(name)
    assert set(outs) == set(FORMS)
    dev = _device(case)
    got = _run(case, 'union', dev)                         # a fresh device copy of the points: order and plan are built for it
    assert torch.equal(got, outs['union'])
    order = ops.point_order(dev[1])[0].cpu()
    G = order.numel() // 16
    passes = _plan_passes(dev, G)
    if kind == 'clouds':
        assert G == 6 and int((order < 0).sum()) == 6 * 16 - 65
        start = row = 0
        for n in case['lens']:                             # every cloud's points fill whole groups of their own
            g = (n + 15) // 16
            mine = order[16 * start:16 * (start + g)]
            assert sorted(mine[mine >= 0].tolist()) == list(range(row, row + n))
            start, row = start + g, row + n
        assert passes == [1] * 6                           # 96 support rows: every union is below the cap
    else:
        assert G == 1 and passes == [T.UNION_PLANS[kind]], passes


# ---------------------------------------------------------------------------------------------------------------------------------------
# repeated rows
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_repeated_neighbour_rows_count_as_often_as_they_appear():
    """One list names a row twice among 9 entries, another a row three times among 40: the reference (and the twin) count the row as often
    as it appears, and so must every form.  The neighbour table folds a repeat into its first occurrence (weights times the
    multiplicity), so the union kernel, whose plan gives equal rows of one list ONE union index, no longer loses a contribution."""
    outs = _all_forms('repeats')
    assert set(outs) == set(FORMS)


# ---------------------------------------------------------------------------------------------------------------------------------------
# plain inputs of any magnitude
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', T.MAGNITUDES)
def test_plain_input_magnitudes(scale):
    """The shape of test_fused_kpconv_input_scale_over_magnitudes with a PLAIN float32 tensor times 1e-6 .. 1e8, both fused kernels: a plain
    input carries no magnitude word of its own, so ops.kpconv_inter_so3 forms one (the largest magnitude among the rows the lists name)
    and the kernels scale by a power of two before their f16 split as they do for the blocked input.  (A hand-made BlockedFeatures
    without a magnitude word is split as it is: no blocked comparison here.)"""
    outs = _all_forms('magnitude %g' % scale, forms=('fused', 'union'), blocked=False)
    assert set(outs) == {'fused', 'union'}


def test_a_large_support_row_that_no_list_names():
    """Support row 0 at 1e6 and no list names it: the padding slots of the neighbour table must not bring it in (0 x Inf), and the result
    equals, bit for bit, the same call with row 0 set to zero."""
    case = T.case('row 0 large')
    assert not bool((case['idx'] == 0).any()) and float(case['x'][0].abs().min()) == 1e6
    outs = _all_forms('row 0 large', forms=('fused', 'union', 'gemm'))
    zeroed = dict(case, x=case['x'].clone())
    zeroed['x'][0] = 0.0
    dev = _device(zeroed)
    for form in ('fused', 'union', 'gemm'):
        assert torch.equal(_run(zeroed, form, dev), outs[form]), form


# ---------------------------------------------------------------------------------------------------------------------------------------
# the first layer
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P,Cout', T.FIRST_LAYER)
def test_first_layer(P, Cout):
    """Cin = 1, NN = 19, counts 0 .. 9: the gather of csrc/kpconv_so3.hip and, without autograd, the streaming GEMM over K = 36 read as 64
    (the rows of the slot sums are read past their end against zero weight columns, the last row past the buffer's); with autograd
    enabled the library GEMM."""
    name = 'first layer P %d Cout %d' % (P, Cout)
    case = T.case(name)
    assert 0 in case['counts'] or P == 1
    dev = _device(case)
    stream = _run(case, 'gemm', dev)
    _judge(case, 'gemm streaming', stream)
    assert torch.equal(_run(case, 'gemm', dev), stream)
    _judge(case, 'gemm library', _run(case, 'gemm', dev, grad=True))
    # the matrix-core switch leaves this shape on the same path
    assert torch.equal(_run(case, 'fused', dev), stream)
