"""GPU: no op reads or returns memory that it did not write, and every op leaves the arrival counters of its workspace zero (DESIGN.md
section 4, "What a call may assume about memory": the audit table; every case below names its row).  The parity tests start from fresh or
zero memory and compare one call with a twin, so a kernel that reads a workspace word before writing it, leaves an element of its
`torch.empty` output unwritten or returns with a counter at 1 passes them all and goes wrong only in a long-running process, where the
caching allocator and the grow-only workspaces hand back yesterday's bytes.  tests/hygiene.py hands every case that memory:

  (a) cold: after caches.clear_caches(), one call gives O0;
  (b) poisoned: every workspace (behind its counter prefix) and every torch.empty* result filled with 0xFF, then with 0x00 -- the weight
      caches dropped first, so that the pieces derived from long-lived weights are built in poisoned memory too;
  (c) stale: a larger problem of the same op, a smaller one, or another op on the same workspace, then the case;
  (d) after every call the counter prefixes are zero;
  (e) a documented refusal, then the counters, then the case.

Every result must equal O0 bit for bit on the contractual region of each output (NaN equals NaN).  The region is the whole output unless
the op's docstring calls a part unspecified; the case then cites the line, and the share compared is printed.  Every case builds its inputs
on the host and moves them to the device inside the call: the caches keyed by tensor identity (neighbour tables, union plans, point orders)
miss, and their buffers are built anew in the memory of that run.  Ops without a Workspace go through (a), (b) and (e) only.
tests/test_hygiene_cpu.py shows that the judge sees planted faults and holds this table to one case per Workspace."""
import contextlib

import numpy as np
import pytest
import torch

import hygiene

pytestmark = pytest.mark.gpu


class Case:
    """name; row: the row of the audit table; workspaces: names as hygiene.workspaces() gives them; run(size) -> tuple of tensors;
    sizes: (the case, other problems of the same op for the stale runs ..); stale: further (label, callable) on the same workspace;
    regions: O0 -> per-output region or None; refusals: callables that must raise."""

    def __init__(self, name, row, workspaces, run, sizes, stale=(), regions=None, refusals=()):
        self.name, self.row, self.workspaces, self.run, self.sizes = name, row, tuple(workspaces), run, tuple(sizes)
        self.stale, self.regions, self.refusals = tuple(stale), regions, tuple(refusals)


CASES = []


def case(*args, **kw):
    CASES.append(Case(*args, **kw))


def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * int(s) for i, s in enumerate(seed)) + 12345)


def _gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _flat(*parts):
    """One tuple of tensors out of tensors, None, and lists / dicts of them (dict values in key order)."""
    out = []
    for p in parts:
        if isinstance(p, dict):
            out += list(_flat(*[p[k] for k in sorted(p)]))
        elif isinstance(p, (list, tuple)):
            out += list(_flat(*p))
        else:
            out.append(p)
    return tuple(out)


# =========================================================================================================================================
# counter workspaces: more than one workgroup arrives at a counter
# =========================================================================================================================================
def _dense_inputs(rows, K, N, nstage, seg):
    g = _gen(rows, K, N, nstage, len(seg or ()))
    nseg = 1 if seg is None else len(seg) - 1
    x = torch.randn(rows, K, generator=g) * 2
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b, gw, gb = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    stages = [torch.randn(nseg, 2, K, generator=g) * 0.5 + torch.tensor([1.0, 0.0])[None, :, None] for _ in range(nstage)]
    return x, w, b, gw, gb, stages


def _dense(kind, rows, K, N, groups, nstage, seg):
    """dense_norm / dense_stats (csrc/dense_norm.hip).  dense_chunks: row tile TR = 64 for N >= 256 else 128, column block BN = 256 for
    N >= 256 else N, one chunk per row tile while tiles <= 768 / column blocks."""
    from se3et_amd import ops
    x, w, b, gw, gb, stages = (t.cuda() if torch.is_tensor(t) else [s.cuda() for s in t] for t in _dense_inputs(rows, K, N, nstage, seg))
    pend = ops.Pending(x, stages, [0.1, 0.2][:nstage], seg)
    if kind == 'dense_stats':
        return (ops.dense_stats(pend, w, b, gw, gb, groups, 1e-5, seg),)
    out = ops.dense_norm(pend, w, b, gw, gb, groups, 1e-5, seg)
    return out.raw, out.affines[0]


def _dense_refusals():
    return [lambda: _dense('dense_norm', 17 * 8, 32, 64, 4, 0, list(range(0, 17 * 8 + 1, 8))),           # 17 segments (kGNMaxSegments = 16)
            lambda: _dense('dense_stats', 17 * 8, 32, 64, 4, 0, list(range(0, 17 * 8 + 1, 8))),
            lambda: _dense('dense_norm', 300, 32, 96, 4, 0, None)]                                      # 96 output features: no tile shape


_SEG16 = list(range(0, 16 * 150 + 1, 150))
for _kind in ('dense_norm', 'dense_stats'):
    # N = 512: two column blocks (blockIdx.y = 0, 1 -> two counters per segment), rows 300 / TR 64 = five row chunks per counter
    case('%s two column blocks' % _kind, '_ws_dense', ['ops._ws_dense'], lambda s, k=_kind: _dense(k, s, 32, 512, 32, 2, None), (300, 700, 100),
         refusals=_dense_refusals() if _kind == 'dense_norm' else ())
    # rows 300 cut at 40: a segment shorter than a row tile (one chunk, its counter expects 1) beside one of five chunks
    case('%s segment shorter than a tile' % _kind, '_ws_dense', ['ops._ws_dense'],
         lambda s, k=_kind: _dense(k, s[-1], 32, 512, 32, 1, list(s)), ((0, 40, 300), (0, 300, 700), (0, 10, 50)))
    # 16 segments of 150 rows, N = 64: TR 128 -> two chunks per segment, all 16 counter rows in use
    case('%s 16 segments' % _kind, '_ws_dense', ['ops._ws_dense'],
         lambda s, k=_kind: _dense(k, s[-1], 32, 64, 4, 0, list(s)), (tuple(_SEG16), (0, 700, 1500), (0, 20, 60)))


def _gn_stats(rows, C, groups, pending, seg, bias=True):
    """group_norm_stats (csrc/rowops.hip).  C = 64 is the fast path (gn_partial4_kernel<.., FIN>: counters + in-kernel finalize), rows = 300
    are three chunks by gn_chunks; C = 48 takes gn_partial_kernel + gn_finalize_kernel (no counter).  A Pending input may carry ONE stage
    here (ops.group_norm_stats refuses more); dense_norm / dense_stats above carry two."""
    from se3et_amd import ops
    g = _gen(rows, C, groups, int(pending), len(seg or ()))
    nseg = 1 if seg is None else len(seg) - 1
    x, w, b, xb = torch.randn(rows, C, generator=g) * 3 + 1, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g), torch.randn(C, generator=g)
    aff = torch.randn(nseg, 2, C, generator=g) * 0.5 + torch.tensor([1.0, 0.0])[None, :, None]
    pend = ops.Pending(x.cuda(), [aff.cuda()] if pending else [], [0.1] if pending else [], seg)
    return (ops.group_norm_stats(pend, w.cuda(), b.cuda(), groups, 1e-5, x_bias=xb.cuda() if bias else None),)


case('group_norm_stats fast path', '_ws_dense', ['ops._ws_dense'], lambda s: _gn_stats(s, 64, 4, False, None), (300, 1300, 20),
     stale=[('dense_norm on the same workspace', lambda: _dense('dense_norm', 300, 32, 512, 32, 2, None))])
case('group_norm_stats fast path, one pending stage', '_ws_dense', ['ops._ws_dense'], lambda s: _gn_stats(s, 64, 4, True, None), (300, 1300, 20))
case('group_norm_stats fast path, two and 16 segments', '_ws_dense', ['ops._ws_dense'],
     lambda s: _gn_stats(s[-1], 64, 4, True, list(s)), ((0, 40, 300), tuple(_SEG16), (0, 5, 9)))
case('group_norm_stats generic path', '_ws_dense', ['ops._ws_dense'], lambda s: _gn_stats(s[-1], 48, 4, False, list(s)), ((0, 40, 300), (0, 900), (0, 7)))


@contextlib.contextmanager
def _kpconv_form(union):
    from se3et_amd import ops
    saved = (ops.KPCONV_MATRIX_CORE, ops.KPCONV_UNION, ops.KPCONV_UNION_ALL, ops.KPCONV_SPLIT)
    try:
        ops.KPCONV_MATRIX_CORE, ops.KPCONV_UNION, ops.KPCONV_UNION_ALL, ops.KPCONV_SPLIT = True, union, union, True
        yield
    finally:
        ops.KPCONV_MATRIX_CORE, ops.KPCONV_UNION, ops.KPCONV_UNION_ALL, ops.KPCONV_SPLIT = saved


def _kpconv(name, union):
    """kpconv_inter_so3 in its split form on a crafted case of tests/kpconv_twin.py.  'split P 9 (64, 64)' and 'split P 9 (256, 64)' are the
    smallest cases of tests/test_gpu_kpconv_edges.py::test_channel_split_shapes_reach_every_factor with z = 2 and z = 8 (one tile of 16
    points: fused_splits of csrc/kpconv_mfma.hip, union_splits of csrc/kpconv_union.hip); z workgroups arrive at each counter."""
    import kpconv_twin as T
    from se3et_amd import functional as SF
    from se3et_amd import ops
    c = T.CASES[name]()
    dev = T.args(c, lambda t: t.cuda())
    with _kpconv_form(union), torch.no_grad():
        if union:
            assert ops.register_point_order(dev[1], c['lens'], T.RADIUS / 2.5) is not None
        Cin, Cout = c['weights'].shape[2:]
        P = c['idx'].shape[0]
        if name.startswith('split'):
            assert (ops.lib().se3_kpconv_union_split_workspace_bytes((P + 15) // 16, Cin, Cout) if union else
                    ops.lib().se3_kpconv_fused_split_workspace_bytes(P, Cin, Cout)) > ops.COUNTER_BYTES['_ws_kpconv_split']
        return (SF.kpconv_inter_so3(*dev),)


for _z, _ch in ((2, '(64, 64)'), (8, '(256, 64)')):
    case('kpconv fused split z = %d' % _z, '_ws_kpconv_split', ['ops._ws_kpconv_split'], lambda s: _kpconv(s, False),
         ('split P 9 ' + _ch, 'split P 40 ' + _ch, 'split P 9 (128, 32)'))
    case('kpconv union split z = %d' % _z, '_ws_kpconv_union_split', ['ops._ws_kpconv_union_split'], lambda s: _kpconv(s, True),
         ('split P 9 ' + _ch, 'split P 40 ' + _ch, 'split P 9 (128, 32)'))
# a union plan whose one group splits into two passes (129 distinct rows against kUCap = 128), after plans of one and eight passes
case('kpconv union, a plan that splits', '_ws_kpconv_union_split', ['ops._ws_kpconv_union_split'], lambda s: _kpconv(s, True),
     ('union cap+1', 'union disjoint64', 'union cap'))


# =========================================================================================================================================
# other model workspaces
# =========================================================================================================================================
def _gn_rows(bwd, C, seg):
    """group_norm_rows / group_norm_rows_bwd (csrc/rowops.hip): C = 64 the float4 partial pass, C = 48 the generic one; one segment and
    three, the first shorter than anything a chunk holds.  The backward returns dx_bias only for an x_bias: both are given."""
    from se3et_amd import ops
    rows = seg[-1]
    g = _gen(int(bwd), C, rows, len(seg))
    x, res, cot = (torch.randn(rows, C, generator=g).cuda() for _ in range(3))
    w, b, xb = (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
    segments = list(seg) if len(seg) > 2 else None
    if bwd:
        return _flat(ops.group_norm_rows_bwd(cot, x, w, b, 4, 1e-5, 0.1, res, xb, segments))
    return (ops.group_norm_rows(x, w, b, 4, 1e-5, 0.1, res, xb, segments),)


for _C in (64, 48):
    for _seg, _what in (((0, 300), 'one segment'), ((0, 40, 170, 300), 'three segments')):
        _others = ((0, 2100), (0, 9)) if len(_seg) == 2 else ((0, 700, 1400, 2100), (0, 3, 6, 9))
        case('group_norm_rows C %d %s' % (_C, _what), '_ws_gn', ['ops._ws_gn'], lambda s, C=_C: _gn_rows(False, C, s), (_seg,) + _others)
        case('group_norm_rows_bwd C %d %s' % (_C, _what), '_ws_gn_bwd', ['ops._ws_gn_bwd'], lambda s, C=_C: _gn_rows(True, C, s), (_seg,) + _others)


def _self_attention(lengths):
    """Stack-mode RPE self attention (SF.rpe_self_attention_packed -> ops.rpe_self_attention_stack -> ops._attention_pieces): C = 256, H = 4
    is the f16 kernel that reads the K / V^T pieces of _ws_attn.  Two clouds of 160 and 7 rows: the key tile is 32 rows (csrc/attention.hip),
    7 and 160 + 7 are no multiples of it; the padding rows of the packed output are part of the contract (they stay exactly 0)."""
    import attention_twin as T
    from se3et_amd import functional as SF
    c = T.attention_case(6, 256, 4, True, seed=sum(lengths) + 42, lengths=lengths)
    w_stack, b_stack, offs = SF.compose_self_attention_weights(c['w_q'], c['b_q'], c['w_k'], c['b_k'], c['w_p'], c['w_eq'], c['H'])
    packed, starts = SF.pack_rows([x.cuda() for x in c['xs']])
    with torch.no_grad():
        return (SF.rpe_self_attention_packed(packed, starts, list(c['lengths']), [e.cuda() for e in c['embs']], [e.cuda() for e in c['eq_embs']],
                                             w_stack.cuda(), b_stack.cuda(), offs, c['w_v'].cuda(), c['b_v'].cuda(), c['H']),)


case('rpe self attention, two unequal clouds', '_ws_attn', ['ops._ws_attn'], _self_attention, ((160, 7), (129, 1, 128), (31,)))


def _cross_eq(mode, lengths):
    """cross_attention_eq_stack (csrc/attention.hip: cross_eq_apply_stack_x6_kernel reads the operand pieces of _ws_x6), A = 6, C = 256, H = 4
    as tests/test_gpu_ops.py::test_cross_attention_eq_stack_bf16x6_matches_the_single_pair_kernels, its smallest lengths.  `out` is the
    caller's: zeros here, so the rows outside the pairs ("left untouched", the docstring) are part of what is compared."""
    from se3et_amd import ops, tables
    g = _gen(len(lengths), lengths[0][0], len(mode))
    A, C, H = 6, 256, 4
    pad = lambda n: (n + 31) // 32 * 32
    q_starts, k_starts, rq, rk = [], [], 0, 0
    for n, m in lengths:
        q_starts.append(rq), k_starts.append(rk)
        rq, rk = rq + pad(n), rk + pad(m)
    q, k, v = torch.zeros(A, rq, C), torch.zeros(A, rk, C), torch.zeros(A, rk, C)
    for (n, m), s0, t0 in zip(lengths, q_starts, k_starts):
        q[:, s0:s0 + n], k[:, t0:t0 + m], v[:, t0:t0 + m] = (torch.randn(A, r, C, generator=g) for r in (n, m, m))
    trace = torch.from_numpy(tables.trace_indices()[0]).cuda()
    out = torch.zeros(A, rq, C, device='cuda')
    mix, w = ops.cross_attention_eq_stack(q.cuda(), k.cuda(), v.transpose(1, 2).contiguous().cuda(), q_starts, [n for n, _ in lengths], k_starts,
                                          [m for _, m in lengths], H, mode, trace, out)
    return out, mix, w


for _mode in ('a_soft', 'r_soft'):
    case('cross_attention_eq_stack ' + _mode, '_ws_x6', ['ops._ws_x6'], lambda s, m=_mode: _cross_eq(m, s),
         (((70, 61), (45, 90)), ((33, 40), (64, 64), (17, 100)), ((17, 20),)))


def _geo_embedding(C, eq, N):
    """geometric_embedding (csrc/geo_embedding.hip: the records of _ws_emb): C = 32 is one 32-channel slice of the angle table, C = 48 one
    and a half; 40 points are more than one workgroup's rows; with and without the equivariant output."""
    from se3et_amd import functional as SF
    from se3et_amd import tables
    g = _gen(C, int(eq), N)
    pts = (torch.rand(N, 3, generator=g) * torch.tensor([1.5, 1.2, 1.0])).cuda()
    div = torch.exp(torch.arange(0, C, 2).float() * (-np.log(10000.0) / C)).cuda()
    w = [(torch.randn(C, C, generator=g) / C ** 0.5).cuda() for _ in range(2)]
    b = [(torch.randn(C, generator=g) * 0.1).cuda() for _ in range(2)]
    w1 = torch.from_numpy(tables.wigner_tables()[1]).cuda() if eq else None
    with torch.no_grad():
        return _flat(SF.geometric_embedding(pts, div, w[0], b[0], w[1], b[1], 0.2, 15.0, 3, wigner_d1=w1))


for _C in (32, 48):
    for _eq in (False, True):
        case('geometric_embedding C %d%s' % (_C, ' equivariant' if _eq else ''), '_ws_emb', ['ops._ws_emb'],
             lambda s, C=_C, eq=_eq: _geo_embedding(C, eq, s), (40, 70, 9))

_micro = {}


def _transformer(lengths):
    """cdriver.transformer_forward through batched.transformer_pairs on the micro_i model (32 channels, the preset of
    tests/test_gpu_model.py::test_transformer_issued_from_c_equals_the_python_schedule): the ~130 launches of one library call carve
    cdriver._ws.  One pair after two, and two after one: the second layout moves every region of the first."""
    from se3et_amd import cdriver
    from se3et_amd.batched import transformer_pairs
    from se3et_amd.model import create_model, load_synthetic_weights, make_cfg
    if 'model' not in _micro:
        _micro['model'] = load_synthetic_weights(create_model(make_cfg('micro_i'))).cuda().eval()
    gt = _micro['model'].transformer
    assert cdriver.ENABLED and cdriver.supported(gt)
    g = _gen(*lengths)
    P = sum(lengths)
    pts, feats = torch.rand(P, 3, generator=g), torch.randn(P, 6, gt.in_proj.in_features, generator=g)
    with torch.no_grad():
        ref, src = transformer_pairs(gt, pts.cuda(), list(lengths), feats.cuda())
    return _flat(ref, src)


case('transformer_forward, one pair', 'cdriver._ws', ['cdriver._ws'], _transformer, ((37, 45), (37, 45, 50, 33)))
case('transformer_forward, two pairs', 'cdriver._ws', ['cdriver._ws'], _transformer, ((37, 45, 50, 33), (37, 45)))


def _forward(num_pairs):
    """The whole micro_i forward (batched.forward_pairs on synthetic.make_pair('micro')): the pyramid builder, every layer of the backbone in
    its pending forms, the transformer and the matching heads on one stream -- the process that bench.py --inflight N keeps alive.  Every
    workspace of the model is carved here in the order of a real forward; the outputs a caller reads are compared."""
    from se3et_amd.batched import forward_pairs
    from se3et_amd.data import precompute_data_stack_mode
    from se3et_amd.model import create_model, load_synthetic_weights, make_cfg
    from se3et_amd.synthetic import make_pair
    cfg = make_cfg('micro_i')
    if 'model' not in _micro:
        _micro['model'] = load_synthetic_weights(create_model(cfg)).cuda().eval()
    b = cfg.backbone
    clouds = [c for p in range(num_pairs) for c in make_pair('micro', index=p)[:2]]
    pts = torch.from_numpy(np.concatenate(clouds, 0)).cuda()
    with torch.no_grad():
        dd = precompute_data_stack_mode(pts, torch.tensor([len(c) for c in clouds]), b.num_stages, b.init_voxel_size, b.init_radius, cfg.neighbor_limits)
        dd['features'] = torch.ones((pts.shape[0], 1), device='cuda')
        out = forward_pairs(_micro['model'], dd)
    keys = ('ref_feats_c', 'src_feats_c', 'ref_node_corr_indices', 'src_node_corr_indices', 'matching_scores', 'estimated_transform')
    return _flat([[o[k] for k in keys] for o in out])


case('whole forward, one pair', 'the model workspaces in one forward',
     ['ops._ws_gn', 'ops._ws_dense', 'ops._ws_kpconv_split', 'ops._ws_kpconv_union_split', 'ops._ws_attn', 'ops._ws_emb', 'cdriver._ws'], _forward, (1, 2))


# =========================================================================================================================================
# tool workspaces: the smallest cases of each tool's own fixture module
# =========================================================================================================================================
def _sheet(seed, nsrc, nref=300, dtype='float64'):
    """(src, ref, ref normals, T0, r, src normals, src colours, ref colours) of tests/icp_fixture.py's sheet pair (the ICP tests' shapes:
    source rows around a wave and the 256 lanes of the step kernels against 300 reference rows)."""
    import colored_icp_fixture as X
    import icp_fixture as F
    import icp_robust_fixture as R
    ref, nrm, src, gt, T0 = F._pair(seed, nref, nsrc, 0.0)
    on = src @ gt[:3, :3].T + gt[:3, 3]
    cast = lambda a: np.ascontiguousarray(a.astype(dtype))
    return (cast(src), cast(ref), cast(nrm), T0, 0.15, cast(R.source_normals(src, gt)), cast(X.texture(on[:, 0], on[:, 1])), cast(X.texture(ref[:, 0], ref[:, 1])))


def _pair_grid(sizes):
    """pair_grid_build + pair_nearest_neighbor_stack (csrc/pair_geometry.hip): the grid IS the workspace; two pairs of unequal supports."""
    from se3et_amd import ops
    pairs = [_sheet(3 + i, n, nref) for i, (n, nref) in enumerate(sizes)]
    ref, src = torch.cat([_gpu(p[1]) for p in pairs]), torch.cat([_gpu(p[0]) for p in pairs])
    grid = ops.pair_grid_build(ref, [len(p[1]) for p in pairs], torch.eye(4, dtype=torch.float64).repeat(len(pairs), 1, 1), 0.0)
    return ops.pair_nearest_neighbor_stack(grid, src, [len(p[0]) for p in pairs])


case('pair_grid_build', '_ws_pair_grid', ['ops._ws_pair_grid'], _pair_grid, (((65, 300), (257, 150)), ((300, 900),), ((5, 9),)))


def _voxel_refused():
    import scan_prep_fixture as F
    from se3et_amd.scan_prep import voxel_downsample_clouds
    p = F.cloud('micro').astype(np.float64)
    p[int(np.argmax(p[:, 1])), 1] = p[:, 1].min() + 0.01 * 2.0 ** 21
    voxel_downsample_clouds([_gpu(p)], 0.01)


def _voxel(size):
    """voxel_downsample_stack on tests/scan_prep_fixture.py's 'micro' cloud with normals."""
    import scan_prep_fixture as F
    from se3et_amd import ops
    name, n = size
    p = np.asarray(F.cloud(name), np.float64)[:n]
    nr = np.random.default_rng(1).standard_normal(p.shape)
    return ops.voxel_downsample_stack(_gpu(p), [len(p)], F.VOXEL_SIZES[name], _gpu(nr))


def _voxel_regions(o0):
    # ops.voxel_downsample_stack: "the clouds' voxel means back to back in out_points[:sum(counts)]" -- the rows behind them are unspecified
    total = int(o0[2][:-1].sum())
    return [(slice(0, total),), (slice(0, total),), None]


case('voxel_downsample_stack', '_ws_voxel', ['ops._ws_voxel'], _voxel, (('micro', 10 ** 9), ('c1_2k', 10 ** 9), ('micro', 50)), regions=_voxel_regions,
     refusals=[_voxel_refused])

_ICP_KEYS = ('transforms', 'fitness', 'inlier_rmse', 'iterations', 'converged', 'status')


def _icp(entry, sizes):
    """icp_stack / icp_weighted_stack / icp_colored_stack through se3et_amd.icp (they share _ws_icp: nearest-neighbour rows and the `done`
    flags of a call).  max_iteration = 8: pairs of one call stop at different evaluations."""
    from se3et_amd import icp
    pairs = [_sheet(1 + i, n) for i, n in enumerate(sizes)]
    srcs, refs, T0, nrm = [_gpu(p[0]) for p in pairs], [_gpu(p[1]) for p in pairs], np.stack([p[3] for p in pairs]), [_gpu(p[2]) for p in pairs]
    if entry == 'icp_stack':
        out = icp.icp_pairs(srcs, refs, T0, 0.15, 'point_to_plane', nrm, max_iteration=8, return_correspondences=True)
    elif entry == 'icp_weighted_stack':
        out = icp.generalized_icp_pairs(srcs, refs, T0, 0.15, [_gpu(p[5]) for p in pairs], nrm, loss='huber', loss_k=0.05, max_iteration=8,
                                        return_correspondences=True)
    else:
        out = icp.colored_icp_pairs(srcs, refs, T0, 0.15, [_gpu(p[6]) for p in pairs], [_gpu(p[7]) for p in pairs], nrm, 0.968, 0.15, max_iteration=8,
                                    return_correspondences=True)
    return _flat([out[k] for k in _ICP_KEYS], out['correspondences'])


_ICP = ('icp_stack', 'icp_weighted_stack', 'icp_colored_stack')
for _entry in _ICP:
    # every order of two: each entry runs after each of the others (on more rows, so that every word it will read has been theirs)
    case(_entry, '_ws_icp', ['ops._ws_icp', 'ops._ws_pair_grid'], lambda s, e=_entry: _icp(e, s), ((65, 257), (700,), (5,)),
         stale=[('%s on the same workspace' % o, lambda o=o: _icp(o, (300, 64, 190))) for o in _ICP if o != _entry])


def _fgr(K):
    """fgr_stack through se3et_amd.fgr.fgr_pairs on tests/fgr_fixture.py's pair (K = 257: one row more than the 256 lanes).  The wrapper cuts
    tuples / trials to the rows the docstring of ops.fgr_stack calls written (num_correspondences / num_tuples)."""
    import fgr_fixture as F
    from se3et_amd import fgr
    src, ref, corr, _ = F.pair(seed=50 + K, n=max(K, 60), degrees=75.0, mismatch=0.3, noise=0.002)
    out = fgr.fgr_pairs([_gpu(src.astype(np.float32))], [_gpu(ref.astype(np.float32))], [_gpu(corr[:K])], evaluate=False, return_tuples=True,
                        maximum_tuple_count=100)
    return _flat([out[k] for k in ('transforms', 'status', 'num_correspondences', 'num_tuples', 'mu')], out['tuples'], out['trials'])


case('fgr_stack', '_ws_fgr', ['ops._ws_fgr'], _fgr, (257, 700, 10))


def _information(sizes):
    """pair_information_stack through se3et_amd.pose_graph.information_matrix_pairs (tests/test_gpu_pose_graph.py::_info_pair)."""
    import icp_fixture as I
    from se3et_amd.pose_graph import information_matrix_pairs
    pairs = []
    for n in sizes:
        rng = np.random.default_rng(70 + n)
        ref, _ = I.sheet(rng, 300)
        on_ref = ref[rng.integers(0, 300, n)] + 0.004 * rng.normal(size=(n, 3))
        gt = I.rigid(rng, 25.0, 0.5)
        inv = np.linalg.inv(gt)
        pairs.append((on_ref @ inv[:3, :3].T + inv[:3, 3], ref, I.rigid(rng, 1.0, 0.01) @ gt))
    out = information_matrix_pairs([_gpu(p[0]) for p in pairs], [_gpu(p[1]) for p in pairs], np.stack([p[2] for p in pairs]), 0.02)
    return _flat(out)


case('pair_information_stack', '_ws_pair_information', ['ops._ws_pair_information', 'ops._ws_pair_grid'], _information, ((65, 257), (700,), (3,)))


def _pose_graph(N):
    """pose_graph_optimize_stack through se3et_amd.pose_graph.optimize_pose_graphs on tests/pose_graph_fixture.py's scene (as
    tests/test_gpu_pose_graph.py::_small: the odometry chain with an error on every node, all loop closures)."""
    import icp_fixture as I
    import pose_graph_fixture as F
    from se3et_amd.pose_graph import optimize_pose_graphs
    graphs = []
    for i, n in enumerate(N):
        g = F.scene(n, 30 + n + i, 'all', 'odometry', 40.0, 1.0)[0]
        rng = np.random.default_rng(1030 + n + i)
        g = dict(g, poses=np.stack([I.rigid(rng, 1.0, 0.01) @ x for x in g['poses']]))
        graphs.append({k: (_gpu(v.astype(np.uint8)) if k == 'uncertain' else _gpu(v)) for k, v in g.items()})
    out = optimize_pose_graphs(graphs, -1)
    return _flat(out)


case('pose_graph_optimize_stack', '_ws_pose_graph', ['ops._ws_pose_graph'], _pose_graph, ((6, 3), (13,), (2,)))


def _nms(name):
    """keypoint_nms_stack through se3et_amd.keypoints.nms_keypoints_clouds on an edge cloud of tests/keypoint_fixture.py: 257 points are
    one more than a tile of the kernel."""
    import keypoint_fixture as F
    from se3et_amd.keypoints import nms_keypoints_clouds
    _, p, s, r = {c[0]: c for c in F.edge_cases()}[name]
    return _flat(nms_keypoints_clouds([_gpu(p)], [_gpu(s)], r, None))


case('keypoint_nms_stack', '_ws_keypoint_nms', ['ops._ws_keypoint_nms', 'ops._ws_pair_grid'], _nms, ('tile_257_float64', 'chain_descending', 'tile_2_float64'))


def _plane(name):
    """plane_segment_stack through se3et_amd.segmentation.segment_plane_clouds on a case of tests/segmentation_fixture.py: 'tile_p1' has one
    hypothesis more than a tile of them."""
    import segmentation_fixture as F
    from se3et_amd.segmentation import segment_plane_clouds
    p, thr, rn, H, seed, _ = F.planes()[name]
    return _flat(segment_plane_clouds([_gpu(p)], thr, rn, H, seed=seed, return_stats=True))


case('plane_segment_stack', '_ws_plane', ['ops._ws_plane'], _plane, ('tile_p1', 'seg2_p1', 'n3'))


def _dbscan(name):
    """dbscan_stack through se3et_amd.segmentation.cluster_dbscan_clouds on a cloud of tests/segmentation_fixture.py."""
    import segmentation_fixture as F
    from se3et_amd.segmentation import cluster_dbscan_clouds
    p, eps, min_points = F.clouds()[name]
    return _flat(cluster_dbscan_clouds([_gpu(p)], eps, min_points))


case('dbscan_stack', '_ws_dbscan', ['ops._ws_dbscan', 'ops._ws_pair_grid'], _dbscan, ('blobs', 'chain_shuffled', 'duplicates'))


def _rgbd(name):
    """rgbd_odometry_stack through se3et_amd.odometry.rgbd_odometry_pairs on a case of tests/rgbd_odometry_fixture.py (32 x 24 images)."""
    import rgbd_odometry_fixture as F
    from se3et_amd.odometry import rgbd_odometry_pairs
    c = F.cases()[name]
    out = rgbd_odometry_pairs(depths=_gpu(c['depths']), colors=_gpu(c['colors']), intrinsics=c['K'], pairs=c['pairs'], init_transforms=c['T0'],
                              method=c['method'], iterations=c['iterations'], max_depth_diff=c['max_depth_diff'], **F.convert_options(c))
    return _flat([out[k] for k in ('transforms', 'success', 'status', 'information', 'correspondences')])


case('rgbd_odometry_stack', '_ws_rgbd', ['ops._ws_rgbd'], _rgbd, ('32x24_hybrid_u16_u8rgb_l3', '32x24_orbit_shared_l2', '31x17_color_u16_f32rgb_l1'))


# =========================================================================================================================================
# ops without a Workspace: outputs and temporaries are torch.empty -- parts (a), (b) and (e)
# =========================================================================================================================================
def _sinkhorn(shape, bwd):
    from se3et_amd import ops
    R, C = shape
    g = _gen(R, C, int(bwd))
    sc = torch.randn(3, R, C, generator=g).cuda()
    rm, cm = (torch.rand(3, R, generator=g) < 0.8).cuda(), (torch.rand(3, C, generator=g) < 0.8).cuda()
    al = torch.tensor(0.7).cuda()
    if bwd:
        return _flat(ops.log_optimal_transport_bwd(torch.randn(3, R + 1, C + 1, generator=g).cuda(), sc, rm, cm, al, 10, 1e12))
    return (ops.log_optimal_transport(sc, rm, cm, al, 10, 1e12),)


for _shape in ((17, 40), (72, 71)):
    case('log_optimal_transport %d x %d' % _shape, 'ops without a Workspace', [], lambda s: _sinkhorn(s, False), (_shape,),
         refusals=[lambda: _sinkhorn((144, 10), False)])                          # (patches of 144 rows: "exceed 143")
    case('log_optimal_transport_bwd %d x %d' % _shape, 'ops without a Workspace', [], lambda s: _sinkhorn(s, True), (_shape,),
         refusals=[lambda: _sinkhorn((144, 10), True)])


def _patch_scores(_):
    from se3et_amd import ops
    g = _gen(7)
    feats = torch.randn(500, 64, generator=g).cuda()
    ri, si = torch.randint(0, 501, (5, 64), generator=g).cuda(), torch.randint(0, 501, (5, 64), generator=g).cuda()       # (500: the padding row)
    return (ops.patch_scores(feats, ri, si, 0.125),)


case('patch_scores', 'ops without a Workspace', [], _patch_scores, (0,))


def _superpoint_scores(stack):
    from se3et_amd import ops
    g = _gen(11, int(stack))
    f = torch.nn.functional.normalize(torch.randn(37 + 45, 32, generator=g), dim=1).cuda()
    if not stack:
        return (ops.superpoint_scores(f[:37].contiguous(), f[37:].contiguous(), True),)
    masks = (torch.rand(82, generator=g) < 0.9).cuda()
    return (ops.superpoint_scores_stack(f, masks, [0, 45], [20, 60], [20, 15], [25, 22], [0, 45], [20, 60], True),)


case('superpoint_scores', 'ops without a Workspace', [], _superpoint_scores, (False,))


def _mutual_topk_refused():
    from se3et_amd import ops
    ops.mutual_topk_mask(torch.zeros(1, 129, 128, device='cuda'), torch.ones(1, 129, dtype=torch.bool, device='cuda'),
                         torch.ones(1, 128, dtype=torch.bool, device='cuda'), 3, 0.05)          # 16512 entries: "rows * cols <= 16384"


case('superpoint_scores_stack', 'ops without a Workspace', [], _superpoint_scores, (True,), refusals=[_mutual_topk_refused])


def _partition(_):
    from se3et_amd import ops
    g = _gen(13)
    return _flat(ops.point_to_node_partition(torch.rand(300, 3, generator=g).cuda(), torch.rand(20, 3, generator=g).cuda(), 16))


def _knn3(_):
    from se3et_amd import ops
    return (ops.knn3_stack(torch.rand(70, 3, generator=_gen(17)).cuda(), [37, 33]),)


case('point_to_node_partition', 'ops without a Workspace', [], _partition, (0,))
case('knn3', 'ops without a Workspace', [], _knn3, (0,))


def _max_pool(bwd):
    from se3et_amd import ops
    g = _gen(19, int(bwd))
    n, m, nn_ = 300, 257, 9
    x = torch.randn(n, 6, 8, generator=g)
    idx = torch.randint(0, n, (m, nn_), generator=g)
    kind = torch.rand(m, nn_, generator=g)
    idx[kind < 0.25] = n                                    # padded entries
    idx[:, 0] = torch.randint(0, n, (m,), generator=g)
    idx[0] = n                                              # a row of padding alone
    if bwd:
        # the scatter as order-independent fixed-point sums, the default (ops.TRAINING_DETERMINISTIC); SE3_KPCONV_BWD=float selects float
        # atomics (csrc/rowops.hip: unsafeAtomicAdd in neighbor_max_pool_bwd_kernel), whose sums depend on the arrival order: not judged here
        saved, ops.TRAINING_DETERMINISTIC = ops.TRAINING_DETERMINISTIC, True
        try:
            return (ops.neighbor_max_pool_bwd(x.cuda(), idx.cuda(), torch.randn(m, 6, 8, generator=g).cuda()),)
        finally:
            ops.TRAINING_DETERMINISTIC = saved
    return (ops.neighbor_max_pool(x.cuda(), idx.cuda()),)


case('neighbor_max_pool', 'ops without a Workspace', [], _max_pool, (False,))
case('neighbor_max_pool_bwd', 'ops without a Workspace', [], _max_pool, (True,))


def _linear(kind):
    """The streaming dense kernels (csrc/dense_norm.hip plain mode, csrc/linear_f16.hip): 300 rows are no multiple of a row tile."""
    from se3et_amd import ops
    g = _gen(len(kind))
    rows, K, N = 300, 64, 128
    x, w, b = torch.randn(rows, K, generator=g).cuda(), (torch.randn(N, K, generator=g) / 8).cuda(), torch.randn(N, generator=g).cuda()
    if kind == 'linear_stream':
        return (ops.linear_stream(x, w, b, relu=True),)
    if kind == 'linear_stream_transposed':
        return (ops.linear_stream_transposed(x.view(3, 100, K), w, b, ld=128),)
    if kind == 'linear_f16':
        return (ops.linear_f16(x, w, b),)
    if kind == 'add_layer_norm':
        return (ops.add_layer_norm(torch.randn(rows, N, generator=g).cuda(), torch.randn(rows, N, generator=g).cuda(), b.abs() + 0.5, b, 1e-5,
                                   hidden_bias=torch.randn(N, generator=g).cuda()),)
    gw, gb = (torch.rand(N, generator=g) + 0.5).cuda(), torch.randn(N, generator=g).cuda()
    aff = ops.dense_stats(x, w, b, gw, gb, 4, 1e-5)
    return (ops.dense_residual(x, w, aff, residual=torch.randn(rows, N, generator=g).cuda(), final_slope=0.1),)


for _kind in ('linear_stream', 'linear_f16', 'add_layer_norm'):
    case(_kind, 'ops without a Workspace', [], _linear, (_kind,))
# ops.linear_stream_transposed: "columns R .. ld are left as allocated: callers pass ld = R padded rows" -- columns 100 .. 128 are unspecified
case('linear_stream_transposed', 'ops without a Workspace', [], _linear, ('linear_stream_transposed',), regions=lambda o0: [(slice(None), slice(None), slice(0, 100))])
case('dense_residual', '_ws_dense', ['ops._ws_dense'], _linear, ('dense_residual',))


def _vgtk(kind):
    """se3et_amd.vgtk: the inter zpconv backward sorts its entries into the buckets of a torch.empty workspace (counts and cursors cleared by
    the entry itself, csrc/vgtk_ops.hip); the gather backward writes every element of its torch.empty gradient."""
    from se3et_amd import vgtk
    g = _gen(len(kind))
    if kind == 'gather':
        pts = torch.randn(2, 5, 70, generator=g).cuda().requires_grad_()
        idx = torch.randint(0, 70, (2, 40), generator=g).int().cuda()
        vgtk.Gathering.apply(pts, idx).backward(torch.randn(2, 5, 40, generator=g).cuda())
        return (pts.grad,)
    b, np_, nq, na, ks, ann, c = 2, 9, 13, 6, 4, 5, 7
    idx = torch.randint(0, nq, (b, np_, na, ks, ann), generator=g).int().cuda()
    w = torch.rand(b, np_, na, ks, ann, generator=g).cuda()
    f = torch.randn(b, c, nq, na, generator=g).cuda().requires_grad_()
    vgtk.inter_zpconv_grouping(idx, w, f).backward(torch.randn(b, c, ks, np_, na, generator=g).cuda())
    return (f.grad,)


case('vgtk inter zpconv backward', 'ops without a Workspace', [], _vgtk, ('inter',))
case('vgtk gather backward', 'ops without a Workspace', [], _vgtk, ('gather',))


def _cluster_refused():
    import mesh_ops_fixture as F
    from se3et_amd import mesh
    v, t = F.cases()['fan_100'][:2]
    mesh.simplify_vertex_clustering_meshes([_gpu(v)], [_gpu(t)], float(np.ptp(v, 0).max()) / 2.0 ** 22)          # an axis of 2^22 cells


def _incidence(name):
    import mesh_ops_fixture as F
    from se3et_amd import ops
    v, t = F.cases()[name][:2]
    inc = ops.mesh_incidence_stack(ops.StackedMeshes(_gpu(v), _gpu(t), [len(v)], [len(t)]))
    return inc.tri_offsets, inc.tri_rows, inc.nbr_offsets, inc.nbr_rows


case('mesh incidence', 'ops without a Workspace', [], _incidence, ('fan_100',), refusals=[_cluster_refused])


def _tsdf(name):
    """TSDFVolumes.integrate + extract_point_clouds on one resolution-13 case of tests/tsdf_fixture.py."""
    import tsdf_fixture as F
    from se3et_amd.tsdf import TSDFVolumes
    c = F.cases()[name]
    vol = TSDFVolumes(1, c['R'], c['vl'], c['trunc'], origins=np.array([c['origin']]), color=c['colors'] is not None, device='cuda')
    E = np.zeros((len(c['table']), 4, 4))
    E[:, :3, :], E[:, 3, 3] = c['table'][:, :12].reshape(-1, 3, 4), 1.0
    vol.integrate(_gpu(c['depths']), c['table'][:, 12:].astype(np.float64), E, [len(c['table'])], _gpu(c['colors']), c['depth_scale'], c['depth_trunc'])
    return _flat(vol.tsdf, vol.weight, vol.color, vol.extract_point_clouds())


case('tsdf integrate and extract', 'ops without a Workspace', [], _tsdf, ('r13_u16_f3',))


def _stsdf(name, bad=None):
    import tsdf_sparse_fixture as F
    from se3et_amd.tsdf_sparse import SparseTSDFVolumes
    c = F.cases()[name]
    vol = SparseTSDFVolumes(len(c['counts']), c['vl'], c['trunc'], color=c['colors'] is not None, stride=c['stride'], device='cuda')
    for x in (c,) if bad is None else (c, bad):
        vol.integrate(_gpu(x['depths']), x['K'], x['E'], x['counts'], _gpu(x['colors']), x['depth_scale'], x['depth_trunc'])
    return _flat(vol.keys, vol.block_coords, vol.state(), vol.extract_point_clouds())


def _stsdf_refused():
    import tsdf_sparse_fixture as F
    _stsdf('face_quarter', F.range_case(131071.8))                   # "frame 1 touches a block coordinate outside" the key range


# 'face_quarter': one pixel whose truncation band ends exactly on block faces (8 blocks); the refused frame is the same pixel 2^18 blocks away
case('sparse tsdf integrate and extract', 'ops without a Workspace', [], _stsdf, ('face_quarter',), refusals=[_stsdf_refused])
case('sparse tsdf, three frames', 'ops without a Workspace', [], _stsdf, ('u16_f3_s1',))


def _raycast(name):
    """TSDFVolumes.ray_cast of one dense view of tests/raycast_fixture.py, every map."""
    import raycast_fixture as R
    from se3et_amd.tsdf import TSDFVolumes
    c = R.cases()[name]
    vol = TSDFVolumes(1, c['state']['tsdf'].shape[0], c['vl'], c['trunc'], origins=np.array([c['origin']]).reshape(-1, 3), color=c['color'], device='cuda')
    vol.tsdf.copy_(_gpu(c['state']['tsdf'])[None]), vol.weight.copy_(_gpu(c['state']['weight'])[None])
    if c['color']:
        vol.color.copy_(_gpu(c['state']['color'])[None])
    maps = vol.ray_cast(c['K'], _gpu(c['E']), c['H'], c['W'], [len(c['E'])], maps=tuple(k for k in R.MAP_NAMES if k != 'color' or c['color']),
                        depth_min=c['depth_min'], depth_max=c['depth_max'], weight_threshold=c['threshold'])
    return _flat(maps)


case('raycast, one dense view', 'ops without a Workspace', [], _raycast, ('r9_exact_zero_17x19',))


# =========================================================================================================================================
@pytest.mark.parametrize('name', [c.name for c in CASES])
def test_op_reads_and_returns_only_what_it_wrote(name):
    from se3et_amd import caches
    c = {c.name: c for c in CASES}[name]
    print('%s (audit row: %s)' % (c.name, c.row))
    stale = [('a %s problem of the same op (%r)' % (what, size), lambda size=size: c.run(size)) for what, size in zip(('larger', 'smaller'), c.sizes[1:])]
    report = []
    try:
        o0 = hygiene.judge(lambda: c.run(c.sizes[0]), stale=stale + list(c.stale), regions=c.regions, refusals=c.refusals,
                           before_poisoned=caches.clear_weight_caches, report=report, log=print)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if 'illegal memory access' in str(e) or 'HIP error' in str(e):          # a fault of the device: nothing more is started on it
            pytest.exit('%s: %s' % (name, e), returncode=3)
        raise
    assert len(report) == sum(o is not None for o in o0) >= 1
    if c.regions is None:
        assert all(compared == total for _, compared, total in report)          # no output compares fewer elements than its contract covers
    for o in o0:
        if o is not None and o.is_floating_point() and o.numel():
            assert not bool((hygiene.bits(o) == -1).all()), 'an output of the cold run is all ones: nothing was computed'


def test_the_judge_sees_unwritten_memory_on_the_device():
    """The control on real kernels: judged WITHOUT its region, linear_stream_transposed fails -- its columns R .. ld are as allocated, and
    the two poison bytes cannot both equal what the cold run found there; a stale word of a counter prefix is named with its offset."""
    from se3et_amd import caches, ops
    with pytest.raises(hygiene.Dirty, match=r'filled with 0x(FF|00): output 0: element \(0, 0, 1\d\d\)'):
        hygiene.judge(lambda: _linear('linear_stream_transposed'), before_poisoned=caches.clear_weight_caches)
    caches.clear_caches()
    _dense('dense_stats', 300, 32, 512, 32, 0, None)
    (buf,) = ops._ws_dense.buffers.values()
    buf[36:40].copy_(torch.tensor([1, 0, 0, 0], dtype=torch.uint8))          # counters[0][9]: as if a call had returned at its first arrival
    with pytest.raises(AssertionError, match=r'ops\._ws_dense: arrival counter at byte offset 36 holds 1'):
        hygiene.counters_are_zero()
    caches.clear_caches()


def test_the_counter_prefixes_are_the_headers():
    """The prefix lengths that hygiene.poison spares are the header's, and the workspace sizes that the library asks for begin with them."""
    from se3et_amd import ops
    from se3et_amd._lib import CONSTANTS
    by_name = {name: prefix for name, _, prefix in hygiene.workspaces()}
    assert by_name['ops._ws_dense'] == CONSTANTS['SE3_GN_COUNTER_BYTES'] == 1024
    assert by_name['ops._ws_kpconv_split'] == by_name['ops._ws_kpconv_union_split'] == CONSTANTS['SE3_KPCONV_SPLIT_COUNTER_BYTES'] == 65536
    assert sum(1 for p in by_name.values() if p) == 3
    L = ops.lib()
    assert L.se3_dense_norm_workspace_bytes(1) - 1024 == (1024 + 16) * 3 * 4                 # (chunks + segments) partials of one group
    assert L.se3_group_norm_stats_workspace_bytes(64) - 1024 == L.se3_group_norm_workspace_bytes(0, 64, 1)
    assert L.se3_kpconv_fused_split_workspace_bytes(9, 64, 64) - 65536 == 2 * 16 * 6 * 64 * 4      # z = 2 partial tiles
    assert L.se3_kpconv_union_split_workspace_bytes(1, 64, 64) - 65536 == 2 * 16 * 6 * 64 * 4
