"""GPU: the EPN toolkit kernels (se3et_amd/vgtk.py -> csrc/vgtk_ops.hip) against the float64 / integer twins of tests/vgtk_twin.py at
crafted edges: channel counts around the gather backward's pass and wave structure and index counts around its 2048-entry stage; ball
queries with exact squared distances at every hit count and cut-off position; furthest point sampling on integer lattices (every tie is
exact) against the reference's literal reduction tree; the zpconv groupings at 255 / 256 / 257 outputs, with singleton dimensions, one
bucket that holds everything beside empty ones, zero weights and features spanning six decades by row; the anchor queries on exact
distances (a point exactly on the radius counts, a weight of exactly zero is not added) and where acos is ill-conditioned; and the
argument checks of every wrapper and C entry, each followed by an ordinary call.  Everything runs with b = 2 (3 for the sampling) and
batch elements that differ.  tests/test_gpu_vgtk.py compares the same kernels with the reference's fixture and on random shapes.

Integers and the gather must match bit for bit.  Allowed elsewhere (tests/vgtk_twin.py; nothing is measured on a kernel): per element
(L + 2) 2^-24 Sigma |w f| for the zpconv sums of L terms (L 2^-24 Sigma |terms| for the gather against float64); for the anchor queries
min(1e-4, 8 max(r, 1.2e-7)) of the largest |want|, r the float32 restatement's error.  tests/test_vgtk_twin_cpu.py holds every case to
its claims and shows that no allowance is vacuous.  With SE3_VGTK_EDGES_PROBE=<file> every case appends a line `kernel / restatement /
allowed` to that file (profiles/vgtk_edges_probe.txt was recorded so)."""
import os

import numpy as np
import pytest
import torch

import vgtk_twin as T

pytestmark = pytest.mark.gpu

_LINES = []


@pytest.fixture(autouse=True)
def _probe():
    _LINES.clear()
    yield
    path = os.environ.get('SE3_VGTK_EDGES_PROBE')
    if path and _LINES:
        with open(path, 'a') as f:
            f.write(''.join(_LINES))


def _record(name, what, kernel, restatement, allowed):
    _LINES.append('%-60s %-18s %.3e / %.3e / %.3e\n' % (name, what, kernel, restatement, allowed))


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def _inside(name, what, got, want, allowed, restated):
    """Per-element allowance; the line records the element where the kernel came closest to (or went furthest past) its allowance."""
    got = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    over = err - allowed
    share = np.where(allowed > 0, err / np.where(allowed > 0, allowed, 1.0), np.where(err > 0, np.inf, 0.0))
    at = np.unravel_index(int(np.argmax(share)), share.shape) if share.size else None
    if at is not None:
        _record(name, what, err[at], np.abs(np.asarray(restated, np.float64) - want)[at], allowed[at])
        print('%s %s: kernel %.3e restatement %.3e allowed %.3e at %s' % (name, what, err[at], np.abs(restated.astype(np.float64) - want)[at], allowed[at], at))
    assert np.isfinite(got).all() and not (over > 0).any(), '%s %s: %d elements past their allowance, worst %.3e against %.3e' % (
        name, what, int((over > 0).sum()), err[at], allowed[at])


# ---- gather ---------------------------------------------------------------------------------------------------------------------------------
def _gather_run(case):
    from se3et_amd import vgtk
    pts = _cuda(case['points']).requires_grad_(True)
    out = vgtk.Gathering.apply(pts, _cuda(case['idx']))
    (out * _cuda(case['cot'])).sum().backward()
    return out.detach(), pts.grad


@pytest.mark.parametrize('c,n,m', T.gather_shapes())
def test_gather_is_bit_equal_to_indexing_and_to_the_in_order_sum(c, n, m):
    for pattern in T.GATHER_PATTERNS:
        case = T.gather_case(c, n, m, pattern)
        out, grad = _gather_run(case)
        assert out.shape == (2, c, m) and torch.equal(out.cpu(), torch.from_numpy(np.array(case['fwd']))), case['name']
        g = grad.cpu().numpy()
        err64, r64 = np.abs(g.astype(np.float64) - case['bwd64']), np.abs(case['bwd32'].astype(np.float64) - case['bwd64'])
        print('%s: backward against float64 %.3e, in-order float32 %.3e, bits differing %d' % (case['name'], err64.max(), r64.max(),
                                                                                             int((g != case['bwd32']).sum())))
        _inside(case['name'], 'backward', grad, case['bwd64'], case['allowed'], case['bwd32'])
        assert np.array_equal(g, case['bwd32']), '%s: the gradient is not the float32 sum in ascending j' % case['name']
        for bi, empty in enumerate(case['empty_workgroups']):
            for w in empty:
                assert not g[bi, :, 64 * w:64 * w + 64].any(), case['name']
        out2, grad2 = _gather_run(case)
        assert torch.equal(out2, out) and torch.equal(grad2, grad), '%s: not bit-identical on repetition' % case['name']


def test_gather_backward_without_indices_is_zero_through_the_c_entry():
    from se3et_amd._lib import lib
    b, c, n = 2, 3, 65
    grad = torch.full((b, c, n), float('nan'), device='cuda')
    spare = torch.zeros(4, device='cuda')
    for go, ix in ((spare.data_ptr(), spare.data_ptr()), (None, None)):
        grad.fill_(float('nan'))
        assert lib().se3_vgtk_gather_points_bwd(go, ix, b, c, n, 0, grad.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(grad.cpu(), torch.zeros(b, c, n))


# ---- ball query -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(T.ball_cases())), ids=lambda i: T.ball_cases()[i]['name'])
def test_ball_query_equals_the_twin_in_every_entry(i):
    from se3et_amd import vgtk
    case = T.ball_cases()[i]
    got = vgtk.ball_query_index(_cuda(case['query']), _cuda(case['support']), case['radius'], case['nsample']).cpu().numpy()
    wrong = int((got != case['want']).sum())
    _record(case['name'], 'entries differing', wrong, 0, 0)
    assert got.dtype == np.int32 and got.shape == case['want'].shape
    assert wrong == 0, '%s: %d entries differ, first rows %s' % (case['name'], wrong, np.argwhere((got != case['want']).any(-1))[:4].tolist())


# ---- furthest point sampling ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', T.FPS_N)
def test_furthest_point_sampling_equals_the_literal_tree(n):
    from se3et_amd import vgtk
    pc = _cuda(T.fps_cloud(n))
    for m in T.fps_samples(n):
        case = T.fps_case(n, m)
        if m == n:
            continue                                         # (the wrapper's shortcut: below)
        got = vgtk.furthest_sample_index(pc, m).cpu().numpy()
        wrong = int((got != case['want']).sum())
        _record(case['name'], 'entries differing', wrong, 0, 0)
        assert got.dtype == np.int32 and got.shape == (3, m)
        assert wrong == 0, '%s: %d entries differ, first at %s' % (case['name'], wrong, np.argwhere(got != case['want'])[:4].tolist())
        assert not got[:, 0].any() and not got[2].any()      # point 0 first, also at the origin; a cloud at the origin selects 0 alone


def test_furthest_sample_index_shortcut_returns_arange():
    from se3et_amd import vgtk
    got = vgtk.furthest_sample_index(_cuda(T.fps_cloud(63)), 63)
    assert got.dtype == torch.int32 and got.is_contiguous() and torch.equal(got.cpu(), torch.arange(63, dtype=torch.int32).expand(3, 63))


# ---- zpconv groupings ---------------------------------------------------------------------------------------------------------------------
def _zp_run(fn, idx, w, case):
    feats = _cuda(case['feats']).requires_grad_(True)
    out = fn(idx, w, feats)
    (out * _cuda(case['cot'])).sum().backward()
    return out.detach(), feats.grad


@pytest.mark.parametrize('name', list(T.INTER_SHAPES))
def test_inter_zpconv_lies_inside_the_in_order_bound(name):
    from se3et_amd import vgtk
    case = T.inter_case(name)
    idx, w = _cuda(case['idx']), _cuda(case['w'])
    out, grad = _zp_run(vgtk.inter_zpconv_grouping, idx, w, case)
    o32, g32 = T.inter_f32(case['idx'], case['w'], case['feats'], case['cot'])
    _inside(name, 'forward', out, case['out'], case['out_allowed'], o32)
    _inside(name, 'backward', grad, case['grad'], case['grad_allowed'], g32)
    out2, grad2 = _zp_run(vgtk.inter_zpconv_grouping, idx, w, case)
    assert torch.equal(out2, out) and torch.equal(grad2, grad), '%s: not bit-identical on repetition' % name


@pytest.mark.parametrize('name', list(T.INTRA_SHAPES))
def test_intra_zpconv_lies_inside_the_in_order_bound(name):
    from se3et_amd import vgtk
    case = T.intra_case(name)
    nbr, w = _cuda(case['nbr']), _cuda(case['w'])
    out, grad = _zp_run(vgtk.intra_zpconv_grouping, nbr, w, case)
    o32, g32 = T.intra_f32(case['nbr'], case['w'], case['feats'], case['cot'])
    _inside(name, 'forward', out, case['out'], case['out_allowed'], o32)
    _inside(name, 'backward', grad, case['grad'], case['grad_allowed'], g32)
    out2, grad2 = _zp_run(vgtk.intra_zpconv_grouping, nbr, w, case)
    assert torch.equal(out2, out) and torch.equal(grad2, grad), '%s: not bit-identical on repetition' % name


# ---- anchor queries -----------------------------------------------------------------------------------------------------------------------
def _shared_rule(name, what, got, want, restatement, allowed):
    err = T.rel_to_largest(got, want)
    _record(name, what, err, restatement, allowed)
    print('%s %s: kernel %.3e restatement %.3e allowed %.3e' % (name, what, err, restatement, allowed))
    assert np.isfinite(got).all() and err <= allowed, '%s %s: %.3e against %.3e' % (name, what, err, allowed)


@pytest.mark.parametrize('name', list(T.ANCHOR_SHAPES))
def test_anchor_query_follows_the_shared_rule(name):
    from se3et_amd import vgtk
    case = T.anchor_case(name)
    got, = vgtk.anchor_query(None, None, _cuda(case['xyz']), _cuda(case['anchors']), _cuda(case['kp']), 0)
    assert got.shape == case['want'].shape
    _shared_rule(name, 'weights', got.cpu().numpy(), case['want'], case['restatement'], case['allowed'])


def test_anchor_query_where_acos_is_ill_conditioned():
    """x exactly parallel / antiparallel to an anchor at |x| = 1e-3, 1, 100: every entry inside the twin's spread over ratio (1 -+ 2^-22);
    a NaN only where the float32 |ratio| reaches 1 - 2^-22 (the |x| = 100 rows), as the reference."""
    from se3et_amd import vgtk
    case = T.anchor_parallel_case()
    got, = vgtk.anchor_query(None, None, _cuda(case['xyz']), _cuda(case['anchors']), _cuda(case['kp']), 0)
    got = got.cpu().numpy().astype(np.float64)
    nan = np.isnan(got)
    inside = (got >= case['lo']) & (got <= case['hi'])
    past = np.where(nan, 0.0, np.maximum(case['lo'] - got, got - case['hi']))
    at = np.unravel_index(int(np.argmax(past)), past.shape)
    _record(case['name'], 'past the spread', max(past[at], 0.0), 0, case['hi'][at] - case['lo'][at])
    _record(case['name'], 'NaN entries', int(nan.sum()), 0, int(case['nan_allowed'].sum()))
    assert not (nan & ~case['nan_allowed']).any(), 'NaN in rows %s' % np.argwhere(nan & ~case['nan_allowed'])[:4].tolist()
    assert (inside | nan).all(), 'outside the spread at %s: %.6e not in [%.6e, %.6e]' % (at, got[at], case['lo'][at], case['hi'][at])


@pytest.mark.parametrize('name', list(T.INITIAL_SHAPES))
def test_initial_anchor_query_counts_exactly_and_follows_the_shared_rule(name):
    from se3et_amd import vgtk
    case = T.initial_case(name)
    args = (_cuda(case['xyz']), _cuda(case['centers']), _cuda(case['kp']), case['radius'], case['sigma'])
    w, n = vgtk.initial_anchor_query(*args)
    wrong = int((n.cpu().numpy().astype(np.int64) != case['want_n']).sum())
    _record(name, 'counts differing', wrong, 0, 0)
    assert wrong == 0, '%s: %d counts differ' % (name, wrong)
    _shared_rule(name, 'weights', w.cpu().numpy(), case['want_w'], case['restatement'], case['allowed'])
    w2, n2 = vgtk.initial_anchor_query(*args)
    assert torch.equal(w2, w) and torch.equal(n2, n)
    w0, n0 = vgtk.initial_anchor_query(args[0][:0], *args[1:])                  # m = 0 points
    assert w0.shape == w.shape and not w0.any() and not n0.any()


# ---- rejections ---------------------------------------------------------------------------------------------------------------------------
class _Ctx:
    def __init__(self, saved, **kw):
        self.saved_tensors = saved
        self.__dict__.update(kw)


def _ordinary():
    """One small ordinary call of every operation -> name -> tensors, to compare before and after a rejection."""
    from se3et_amd import vgtk
    g, ball, fps = T.gather_case(3, 65, 1, 'uniform'), T.ball_cases()[7], T.fps_case(63, 2)
    inter, intra, anchor, initial = T.inter_case('inter nq=1'), T.intra_case('intra ann=1'), T.anchor_case('anchor np=1'), T.initial_case('initial 255 outputs')
    out = {}
    out['gather'] = _gather_run(g)
    out['ball'] = (vgtk.ball_query_index(_cuda(ball['query']), _cuda(ball['support']), ball['radius'], ball['nsample']),)
    out['fps'] = (vgtk.furthest_sample_index(_cuda(fps['pc']), 2),)
    out['inter'] = _zp_run(vgtk.inter_zpconv_grouping, _cuda(inter['idx']), _cuda(inter['w']), inter)
    out['intra'] = _zp_run(vgtk.intra_zpconv_grouping, _cuda(intra['nbr']), _cuda(intra['w']), intra)
    out['anchor'] = tuple(vgtk.anchor_query(None, None, _cuda(anchor['xyz']), _cuda(anchor['anchors']), _cuda(anchor['kp']), 0))
    out['initial'] = tuple(vgtk.initial_anchor_query(_cuda(initial['xyz']), _cuda(initial['centers']), _cuda(initial['kp']), 1.25, 1.5625))
    return out


def _assert_ordinary(first, context):
    again = _ordinary()
    for key, tensors in first.items():
        for a, b in zip(tensors, again[key]):
            assert torch.equal(a, b), '%s: %s changed' % (context, key)


def test_shape_disagreements_are_rejected_before_any_launch_and_the_next_call_works():
    from se3et_amd import vgtk
    first = _ordinary()
    assert torch.equal(first['ball'][0].cpu(), torch.from_numpy(np.array(T.ball_cases()[7]['want'])))
    assert np.array_equal(first['gather'][1].cpu().numpy(), T.gather_case(3, 65, 1, 'uniform')['bwd32'])
    f = lambda *s: torch.zeros(*s, device='cuda')
    i = lambda *s: torch.zeros(*s, dtype=torch.int32, device='cuda')
    bad = {
        'gather: idx batch': lambda: vgtk.gather_points(f(2, 3, 5), i(3, 4)),
        'gather backward: grad_out m': lambda: vgtk.Gathering.backward(_Ctx((i(2, 4),), n=5), f(2, 3, 5)),
        'gather backward: grad_out batch': lambda: vgtk.Gathering.backward(_Ctx((i(2, 4),), n=5), f(1, 3, 4)),
        'inter: weights shape': lambda: vgtk.inter_zpconv_grouping(i(2, 4, 3, 2, 5), f(2, 4, 3, 2, 4), f(2, 3, 6, 3)),
        'inter: feats anchors': lambda: vgtk.inter_zpconv_grouping(i(2, 4, 3, 2, 5), f(2, 4, 3, 2, 5), f(2, 3, 6, 4)),
        'inter: feats batch': lambda: vgtk.inter_zpconv_grouping(i(2, 4, 3, 2, 5), f(2, 4, 3, 2, 5), f(1, 3, 6, 3)),
        'inter backward: grad_out': lambda: vgtk.InterZPConvGrouping.backward(_Ctx((i(2, 4, 3, 2, 5), f(2, 4, 3, 2, 5)), nq=6), f(2, 3, 2, 5, 3)),
        'intra: weights anchors': lambda: vgtk.intra_zpconv_grouping(i(7, 3), f(6, 2, 3), f(2, 3, 4, 5)),
        'intra: weights neighbours': lambda: vgtk.intra_zpconv_grouping(i(7, 3), f(7, 2, 4), f(2, 3, 4, 5)),
        'intra backward: grad_out anchors': lambda: vgtk.IntraZPConvGrouping.backward(_Ctx((i(7, 3), f(7, 2, 3)), na_in=5), f(2, 3, 2, 4, 6)),
        'intra backward: grad_out kernel size': lambda: vgtk.IntraZPConvGrouping.backward(_Ctx((i(7, 3), f(7, 2, 3)), na_in=5), f(2, 3, 1, 4, 7)),
    }
    for name, call in bad.items():
        with pytest.raises(RuntimeError, match='disagree|does not fit|is not'):            # the wrappers' own messages: raised before a launch
            call()
        _assert_ordinary(first, 'after ' + name)


def _entries():
    """name -> (arguments of a valid call, positions of the pointers, {position of a size: a value below its minimum}, the wrapper-level
    key of _ordinary)."""
    f = lambda *s: torch.zeros(*s, device='cuda')
    i = lambda *s: torch.zeros(*s, dtype=torch.int32, device='cuda')
    keep, p = [], lambda t: (keep.append(t), t.data_ptr())[1]
    b = 2
    ws = 4096
    e = {
        'vgtk_gather_points_fwd': ([p(f(b, 3, 5)), p(i(b, 4)), b, 3, 5, 4, p(f(b, 3, 4)), None], (0, 1, 6), {2: 0, 3: 0, 4: 0, 5: -1}),
        'vgtk_gather_points_bwd': ([p(f(b, 3, 4)), p(i(b, 4)), b, 3, 5, 4, p(f(b, 3, 5)), None], (0, 1, 6), {2: 0, 3: 0, 4: 0, 5: -1}),
        'vgtk_anchor_query': ([p(f(b, 3, 4, 5)), p(f(6, 3)), p(f(2, 2)), b, 4, 5, 6, 2, p(f(b, 4, 6, 2, 5)), None], (0, 1, 2, 8),
                              {3: 0, 4: 0, 5: 0, 6: 0, 7: 0}),
        'vgtk_initial_anchor_query': ([p(f(b, 3, 4)), p(f(7, 3)), p(f(2, 3, 3)), b, 4, 7, 3, 2, 1.0, 1.0, p(f(b, 2, 4, 3)), p(f(b, 2, 4, 3)), None],
                                      (0, 1, 2, 10, 11), {3: 0, 4: 0, 5: -1, 6: 0, 7: 0}),
        'vgtk_ball_query': ([p(f(b, 3, 4)), p(f(b, 3, 9)), b, 9, 4, 1.0, 3, p(i(b, 4, 3)), None], (0, 1, 7), {2: 0, 3: 0, 4: 0, 6: 0}),
        'vgtk_furthest_point_sampling': ([p(f(b, 3, 9)), b, 9, 4, p(f(b, 9)), p(i(b, 4)), None], (0, 4, 5), {1: 0, 2: 0, 3: -1}),
        'vgtk_inter_zpconv_fwd': ([p(i(b, 4, 3, 2, 5)), p(f(b, 4, 3, 2, 5)), p(f(b, 3, 6, 3)), b, 4, 6, 3, 2, 5, 3, p(f(b, 3, 2, 4, 3)), None],
                                  (0, 1, 2, 10), {k: 0 for k in range(3, 10)}),
        'vgtk_inter_zpconv_bwd': ([p(i(b, 4, 3, 2, 5)), p(f(b, 4, 3, 2, 5)), p(f(b, 3, 2, 4, 3)), b, 4, 6, 3, 2, 5, 3, p(f(b, 3, 6, 3)),
                                   p(torch.zeros(ws, dtype=torch.uint8, device='cuda')), ws, None], (0, 1, 2, 10, 11), {k: 0 for k in range(3, 10)}),
        'vgtk_intra_zpconv_fwd': ([p(i(7, 3)), p(f(7, 2, 3)), p(f(b, 3, 4, 5)), b, 4, 5, 7, 2, 3, 3, p(f(b, 3, 2, 4, 7)), None], (0, 1, 2, 10),
                                  {k: 0 for k in range(3, 10)}),
        'vgtk_intra_zpconv_bwd': ([p(i(7, 3)), p(f(7, 2, 3)), p(f(b, 3, 2, 4, 7)), b, 4, 5, 7, 2, 3, 3, p(f(b, 3, 4, 5)), None], (0, 1, 2, 10),
                                  {k: 0 for k in range(3, 10)}),
    }
    return e, keep


def test_c_entries_reject_bad_arguments_with_their_message_and_the_next_call_works():
    from se3et_amd._lib import CONSTANTS, lib
    L = lib()
    first = _ordinary()
    entries, keep = _entries()
    need = L.se3_vgtk_inter_zpconv_bwd_workspace_bytes(2, 4, 6, 3, 2, 5)
    assert 0 < need <= 4096
    rejected = 0
    for name, (args, pointers, sizes) in entries.items():
        fn = getattr(L, 'se3_' + name)
        assert fn(*args) == 0, name                                                   # the valid call
        variants = [(k, None, 'null pointer') for k in pointers] + [(k, v, 'bad sizes') for k, v in sizes.items()]
        if name == 'vgtk_inter_zpconv_bwd':
            variants.append((12, need - 1, 'workspace too small'))
        for k, v, message in variants:
            call = list(args)
            call[k] = v
            status = fn(*call)
            assert status == CONSTANTS['SE3_ERR_INVALID_ARG'], '%s argument %d = %r: status %d' % (name, k, v, status)
            assert L.se3_last_error().decode() == '%s: %s' % (name, message), '%s argument %d: %r' % (name, k, L.se3_last_error())
            rejected += 1
            _assert_ordinary(first, 'after %s argument %d = %r' % (name, k, v))
    assert rejected >= 10 * 7 and len(keep) >= 30
