"""GPU: the forward attention kernels (csrc/attention.hip: rpe_bias_kernel, attention_kernel<D>, attention_x6_kernel and their stack-mode
entry points) against the float64 twin (tests/attention_twin.py) at their tile edges: 1 to 5 key tiles around the three-deep tile ring
of the f16 kernel and its step count padded to a multiple of 3, one query, clouds with fewer 128-query blocks than the grid, waves
without a key tile in the merge, every dispatch cell of the logits kernel, the batch's plain cross attention, and softmax rows that
rescale at every step.  tests/test_gpu_ops.py compares the same kernels with the oracle on generic shapes at a whole-tensor 1e-4.

Every case is judged in two figures (attention_twin.error_figures): `global`, max |got - want| / max |want|, and `per row`, the same
per (anchor, query) row of the hidden states or (anchor . head, query) row of the logits / scores, a row below 1e-3 of the tensor's
maximum measured against that share.  Allowed, for both: min(1e-4, 16 x max(r, 1.2e-7)), r the same figure of the float32 restatement
(se3et_amd/autograd.py on the CPU, on the same inputs) against the twin; 16 = 4 (the split products keep 2^-22 per term against float32's
2^-24) x 2 (__expf and the reciprocal against libm) x 2 (another association of the sums: MFMA accumulation order, wave merge).  With
SE3_ATTENTION_EDGES_PROBE=<file> every case appends its figures to that file (profiles/attention_edges_probe.txt was recorded so)."""
import ctypes
import os

import pytest
import torch

import attention_twin as T

pytestmark = pytest.mark.gpu


def _dev(t):
    return None if t is None else t.cuda()


def _record(case, figures):
    """figures: [(name, kernel error, restatement error, allowed)] -> one line in the probe file."""
    for name, k, r, a in figures:
        print('%s %s: kernel %.3e restatement %.3e allowed %.3e' % (case, name, k, r, a))
    path = os.environ.get('SE3_ATTENTION_EDGES_PROBE')
    if path:
        with open(path, 'a') as f:
            f.write('%-58s %s\n' % (case, '   '.join('%s kernel %.2e restatement %.2e allowed %.2e' % fig for fig in figures)))


def _judge(case, parts, factor=T.FACTOR):
    """parts: [(what, got, twin, restatement)]: both figures of every part, recorded, then asserted."""
    figures = []
    for what, got, want, rest in parts:
        assert bool(torch.isfinite(got).all()), '%s %s is not finite' % (case, what)
        figures += [(('%s %s' % (what, name)).strip(), k, r, a) for name, k, r, a in T.check(got, want, rest, factor)]
    _record(case, figures)
    for name, k, r, a in figures:
        assert k <= a, '%s %s: error %.3e > %.3e (restatement %.3e)' % (case, name, k, a, r)


class _Saturation:
    """ops.attention_saturated reads 0 after the block (nothing here is non-finite)."""

    def __enter__(self):
        from se3et_amd import ops
        ops.attention_saturated()

    def __exit__(self, kind, *exc):
        from se3et_amd import ops
        if kind is None:
            assert ops.attention_saturated() == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# (a), (b): the stack-mode self attention of the layers, C = 256: rpe_bias_kernel + attention_x6_kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
def _self_attention_packed(case, bf16):
    """SF.rpe_self_attention_packed on the clouds of a stack case -> (hidden (A, R, C) on the CPU, the row start of every cloud)."""
    from se3et_amd import functional as SF
    H = case['H']
    w_stack, b_stack, offs = SF.compose_self_attention_weights(case['w_q'], case['b_q'], case['w_k'], case['b_k'], case['w_p'], case['w_eq'], H)
    packed, starts = SF.pack_rows([x.cuda() for x in case['xs']])
    embs = [e.to(torch.bfloat16).cuda() if bf16 else e.cuda() for e in case['embs']]
    got = SF.rpe_self_attention_packed(packed, starts, list(case['lengths']), embs, [_dev(e) for e in case['eq_embs']], w_stack.cuda(),
                                       b_stack.cuda(), offs, case['w_v'].cuda(), case['b_v'].cuda(), H)
    return got.cpu(), starts


def _check_stack(case, bf16, name):
    with _Saturation():
        got, starts = _self_attention_packed(case, bf16)
    twin_case = T.rounded_embedding(case) if bf16 else case
    want, rest = T.self_attention(twin_case), T.self_attention(twin_case, T.f32)
    pad = torch.ones(got.shape[1], dtype=torch.bool)
    for s0, n in zip(starts, case['lengths']):
        pad[s0:s0 + n] = False
    if bool(pad.any()):
        assert float(got[:, pad].abs().max()) == 0.0, name + ': the padding rows of out must stay exactly 0'
    _judge(name, [('cloud %d' % c, got[:, s0:s0 + n], w, r) for c, (s0, n, w, r) in enumerate(zip(starts, case['lengths'], want, rest))])


@pytest.mark.parametrize('bf16', [False, True], ids=['f32emb', 'bf16emb'])
@pytest.mark.parametrize('A,eq', [(1, False), (6, True)])
@pytest.mark.parametrize('lengths', T.STACK_EDGE_LENGTHS)
def test_self_attention_stack_at_the_tile_edges(lengths, A, eq, bf16):
    """SF.rpe_self_attention_packed, C = 256, H = 4 (head dimension 64, starts multiples of 32: the f16 kernel).  Clouds of 1; 31, 32, 33;
    64, 65, 96, 97; 129, 1, 128; 160, 7 rows: 1 to 5 key tiles around the ring depth 3 and the step count padded to a multiple of 3; one
    query; clouds with fewer 128-query blocks than the grid (blockIdx.x * 128 >= N returns early beside a cloud of 129 or 160); a last
    workgroup with one live row (129) whose three other waves still copy tiles; the padding rows of out stay exactly 0.  Both embeddings:
    for bf16 the twin and the restatement take the rounded embedding."""
    case = T.attention_case(A, 256, 4, eq, seed=sum(lengths) + 7 * A, lengths=lengths)
    _check_stack(case, bf16, 'stack %s A %d %s' % (lengths, A, 'bf16' if bf16 else 'f32'))


@pytest.mark.parametrize('kind', T.STACK_STRESS_KINDS)
def test_self_attention_stack_with_stressed_softmax_rows(kind):
    """The same entry point, A = 6, lengths (97, 160), f32 embedding: `peaked` rows, `offset` (a large row-constant logit that cancels in
    exact arithmetic), `late` (the running maximum rises at every key tile, so every step rescales O and l) and `early`;
    tests/test_attention_twin_cpu.py asserts on the twin that the inputs do that."""
    _check_stack(T.stack_stress_case(kind), False, 'stack (97, 160) A 6 %s' % kind)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (c): the single pair: se3_rpe_bias_fwd + attention_kernel<D>
# ---------------------------------------------------------------------------------------------------------------------------------------
def _check_pair(case, name):
    from se3et_amd import functional as SF
    q, k, vt, emb, w_p, eq_emb, w_eq = [_dev(case[n]) for n in ('q', 'k', 'vt', 'emb', 'w_p', 'eq_emb', 'w_eq')]
    with _Saturation():
        got, scores = SF.rpe_attention(q, k, vt, emb, w_p, eq_emb, w_eq, case['H'], return_scores=True)
        got, scores = got.cpu(), scores.cpu()
    want, want_scores = T.pair_attention(case)
    rest, rest_scores = T.pair_attention(case, T.f32)
    _judge(name, [('hidden', got, want, rest), ('scores', scores, want_scores, rest_scores)])


@pytest.mark.parametrize('N,M', T.PAIR_SHAPES)
@pytest.mark.parametrize('C', T.PAIR_CHANNELS)
def test_single_pair_attention_at_every_head_dimension(C, N, M):
    """SF.rpe_attention, A = 6 with the equivariant term, H = 4: head dimensions 8, 16, 32, 64 behind dispatch_head_dim with 1 to 5 key
    tiles over the 4 waves of attention_kernel<D> (M <= 96: waves without a tile enter the LDS merge with m = -inf, l = 0), N != M, one
    query and one key.  Hidden states and the returned scores."""
    _check_pair(T.pair_case(C, N, M), 'pair C %d (%d, %d)' % (C, N, M))


@pytest.mark.parametrize('kind,shape', T.PAIR_STRESS)
def test_single_pair_attention_with_stressed_softmax_rows(kind, shape):
    """attention_kernel<64> with logits at (40, 97): `late` (every wave's tile raises the maximum, the merge rescales all partial sums)
    and `peaked`."""
    _check_pair(T.pair_case(256, *shape, kind), 'pair C 256 %s %s' % (shape, kind))


# ---------------------------------------------------------------------------------------------------------------------------------------
# (d): the relative-position logits alone
# ---------------------------------------------------------------------------------------------------------------------------------------
def _folded(case, convert):
    """The folded queries [qp | qe] as ONE tensor (the kernel takes them as column blocks of one projection), formed on the CPU in the
    precision of `convert`."""
    logits, qp, qe = T.logits_twin(case, convert)
    return logits, torch.cat((qp, qe), -1).float().contiguous()


@pytest.mark.parametrize('A,H,C,N,M', T.LOGITS_CASES)
def test_rpe_logits_in_every_dispatch_cell(A, H, C, N, M):
    """ops.rpe_bias against rpe_logits (unscaled, float32 embedding): AH = 4 and 16 (one row tile, 16 the last shape on it), 20 (the second
    row tile partly empty), 24 and 32 (the limit: every row of both row tiles live), H = 2 (H % 4 != 0: the f32-MFMA variant), H = 8; every
    channel count; (N, M) = (5, 65) and (33, 31): 3 units per row and 4 per workgroup, so segments start and end inside a row.  The
    columns M .. ceil32(M) - 1 are exactly 0, which the attention kernels rely on.  The folded queries are formed on the CPU in float32
    and handed to the kernel as they are: the restatement folds in float32 too."""
    from se3et_amd import ops
    case = T.logits_case(A, H, C, N, M)
    want = T.logits_twin(case)[0]
    rest, both = _folded(case, T.f32)
    both = both.cuda()
    got = ops.rpe_bias(both[..., :H * C], both[..., H * C:], case['emb'].cuda(), case['eq_emb'].cuda(), H).cpu()
    assert got.shape == (A * H, N, T.key_stride(M))
    if T.key_stride(M) > M:
        assert float(got[..., M:].abs().max()) == 0.0, 'the columns from M to ceil32(M) must be exactly 0'
    _judge('logits A %d H %d C %d (%d, %d)' % (A, H, C, N, M), [('', got[..., :M], want, rest)])


@pytest.mark.parametrize('lengths', T.LOGITS_SHAPES)
@pytest.mark.parametrize('A,H,C', [(a, h, 64) for a, h in T.LOGITS_HEADS] + [(6, 4, c) for c in (32, 128, 256)])
def test_rpe_logits_with_the_bf16_embedding(A, H, C, lengths):
    """The bf16 embedding goes through ops.rpe_bias_stack, whose clouds are square (self attention): it refuses the (N, M) = (5, 65) /
    (33, 31) embedding itself with an ordinary error, and the next call serves a stack of two square clouds of those lengths -- the
    same key-tile counts, row counts and dispatch cells; the twin and the restatement take the rounded embedding.

    The factor here is 1024, not 16.  With the embedding in bf16 the kernel splits the folded queries into bf16 hi + lo fragments, and
    csrc/attention.hip documents what that keeps: "the query side stays exact to 2^-16" per term, where the f16 split of the float32
    path keeps 2^-22 -- the first part of the factor is 2^-16 / 2^-24 = 256 instead of 4, the other two stay: 256 x 2 x 2.  The
    restatement, whose products with an 8-bit embedding are nearly exact, sits at 1e-7 .. 5e-7 here, so the allowed error is the 1e-4
    ceiling in most cases; the kernel was measured at 17 to 26 times the restatement (2e-6 .. 8e-6), which 16 does not cover and a
    2^-16 rounding per term accounts for (2^-17 / sqrt(3) = 4.4e-6 of the largest logit for errors of random sign).  The hidden states
    behind these logits keep the factor 16 (test_self_attention_stack_at_the_tile_edges, both embeddings)."""
    from se3et_amd import ops
    cases = [T.rounded_embedding(T.logits_case(A, H, C, n, n)) for n in lengths]
    starts, total = [], 0
    for n in lengths:
        starts.append(total)
        total += T.key_stride(n)
    both = torch.zeros(A, total, H * C + 4 * H)
    wants, rests = [], []
    for case, s0, n in zip(cases, starts, lengths):
        rest, folded = _folded(case, T.f32)
        both[:, s0:s0 + n] = folded
        wants.append(T.logits_twin(case)[0])
        rests.append(rest)
    both = both.cuda()
    qp, qe = both[..., :H * C], both[..., H * C:]
    embs, eqs = [c['emb'].to(torch.bfloat16).cuda() for c in cases], [c['eq_emb'].cuda() for c in cases]
    crooked = T.logits_case(A, H, C, *lengths)
    with pytest.raises(RuntimeError, match='rpe_bias_stack'):
        ops.rpe_bias_stack(qp, qe, [crooked['emb'].to(torch.bfloat16).cuda()], [crooked['eq_emb'].cuda()], [0], [lengths[0]], H)
    torch.cuda.synchronize()
    bias, offs = ops.rpe_bias_stack(qp, qe, embs, eqs, starts, list(lengths), H)
    bias = bias.cpu()
    parts = []
    for c, (n, off) in enumerate(zip(lengths, offs)):
        block = bias[off:off + A * H * n * T.key_stride(n)].reshape(A * H, n, T.key_stride(n))
        if T.key_stride(n) > n:
            assert float(block[..., n:].abs().max()) == 0.0, 'the columns from M to ceil32(M) must be exactly 0'
        parts.append(('cloud %d' % c, block[..., :n], wants[c], rests[c]))
    _judge('logits bf16 A %d H %d C %d %s' % (A, H, C, lengths), parts, T.FACTOR_BF16_LOGITS)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (e): the plain cross attention of a batch
# ---------------------------------------------------------------------------------------------------------------------------------------
CROSS_PAIRS = ((33, 31), (1, 65), (40, 97))


@pytest.mark.parametrize('anchors', [0, 6], ids=['shared values', 'values per anchor'])
@pytest.mark.parametrize('C', [128, 256])
def test_plain_cross_attention_of_a_batch(C, anchors):
    """ops.attention_stack(..., None, None, ...) as batched._cross_plain calls it: three pairs with N != M packed by pack_rows, so
    q_starts (0, 64, 96) != k_starts (0, 32, 128); values shared (C, Rk) or per anchor (6, C, Rk) under the same scores.  Without
    logits the f16 kernel declines: attention_kernel<32> and <64>.  The rows of out outside the pairs are not written."""
    from se3et_amd import functional as SF
    from se3et_amd import ops
    H = 4
    pairs = T.cross_case(CROSS_PAIRS, C, anchors, seed=C + anchors)
    q, q_starts = SF.pack_rows([p['q'].cuda() for p in pairs])
    k, k_starts = SF.pack_rows([p['k'].cuda() for p in pairs])
    v, _ = SF.pack_rows([p['v'].cuda() for p in pairs])
    assert q_starts != k_starts
    vt = v.transpose(-1, -2).contiguous()
    A = max(anchors, 1)
    out = torch.full((A, q.shape[0], C), 7.0, device='cuda')
    with _Saturation():
        ops.attention_stack(q, k, vt, None, None, q_starts, [p['q'].shape[0] for p in pairs], k_starts, [p['k'].shape[0] for p in pairs], H,
                            out if anchors else out[0])
        got = out.cpu()
    outside = torch.ones(q.shape[0], dtype=torch.bool)
    parts = []
    for c, (p, s0) in enumerate(zip(pairs, q_starts)):
        n = p['q'].shape[0]
        outside[s0:s0 + n] = False
        parts.append(('pair %d' % c, got[:, s0:s0 + n], T.cross_twin(p, H), T.cross_twin(p, H, T.f32)))
    assert bool((got[:, outside] == 7.0).all()), 'rows of out outside the pairs must stay untouched'
    _judge('cross C %d %s' % (C, 'values per anchor' if anchors else 'shared values'), parts)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (f): the two stack ops with key starts that keep / leave the f16 kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
def _launch_tags(fn):
    """The tags of the attention launches fn() makes (csrc/attention.hip launch_kernel: 1 logits, 2 softmax.V, 3 the operand split that
    goes in front of the f16 kernel only)."""
    from se3et_amd import _lib
    cap = 64
    us, tags, aux = (ctypes.c_float * cap)(), (ctypes.c_int * cap)(), (ctypes.c_double * cap)()
    _lib.lib().se3_debug_kernel_timing(0)
    _lib.lib().se3_debug_kernel_timing_collect_ex(us, tags, aux, cap)
    _lib.lib().se3_debug_kernel_timing(1)
    try:
        out = fn()
    finally:
        _lib.lib().se3_debug_kernel_timing(0)
        n = _lib.lib().se3_debug_kernel_timing_collect_ex(us, tags, aux, cap)
    return out, [tags[i] for i in range(n)]


@pytest.mark.parametrize('second_start,f16_kernel', [(48, True), (36, False)])
def test_stack_ops_with_unpadded_key_starts(second_start, f16_kernel):
    """ops.rpe_bias_stack + ops.attention_stack, C = 256, A = 6, clouds of 33 and 65 rows at starts (0, 48) and (0, 36); queries, keys and
    value columns sit at the same starts, so the second cloud begins inside the first one's last 32-key tile (its columns there must
    weigh nothing).  48 is a multiple of 16 and keeps the f16 kernel; 36 is a multiple of 4 only: launch_attention_x6 declines and
    attention_kernel<64> serves the stack -- read off the launch tags (the operand split runs in front of the f16 kernel only)."""
    from se3et_amd import ops
    H, C, A, R = 4, 256, 6, 160
    lengths, starts = [33, 65], [0, second_start]
    case = T.attention_case(A, C, H, True, seed=second_start, lengths=lengths)
    assert all(s0 + T.key_stride(n) <= R for s0, n in zip(starts, lengths)) and starts[1] < T.key_stride(lengths[0])
    q, k, both = torch.zeros(A, R, C), torch.zeros(A, R, C), torch.zeros(A, R, H * C + 4 * H)
    vt = torch.zeros(A, C, R)
    wants, rests = [], []
    for c, (s0, n) in enumerate(zip(starts, lengths)):
        q32, k32, vt32, emb, w_p, eq_emb, w_eq = T.projected(case, c, T.f32)
        pair = dict(case, q=q32, k=k32, vt=vt32, emb=emb, w_p=w_p, eq_emb=eq_emb, w_eq=w_eq)        # the projected rows ARE this case's inputs
        q[:, s0:s0 + n], k[:, s0:s0 + n], vt[:, :, s0:s0 + n] = q32, k32, vt32[..., :n]
        both[:, s0:s0 + n] = _folded(pair, T.f32)[1]
        wants.append(T.pair_attention(pair)[0])
        rests.append(T.pair_attention(pair, T.f32)[0])
    q, k, vt, both = q.cuda(), k.cuda(), vt.cuda(), both.cuda()
    embs, eqs = [e.cuda() for e in case['embs']], [e.cuda() for e in case['eq_embs']]
    out = torch.zeros(A, R, C, device='cuda')

    def run():
        bias, offs = ops.rpe_bias_stack(both[..., :H * C], both[..., H * C:], embs, eqs, starts, lengths, H)
        ops.attention_stack(q, k, vt, bias, offs, starts, lengths, starts, lengths, H, out)
        torch.cuda.synchronize()

    with _Saturation():
        _, tags = _launch_tags(run)
    assert tags == ([1, 3, 2] if f16_kernel else [1, 2]), tags
    got = out.cpu()
    _judge('stack ops starts (0, %d)' % second_start,
           [('cloud %d' % c, got[:, s0:s0 + n], wants[c], rests[c]) for c, (s0, n) in enumerate(zip(starts, lengths))])
