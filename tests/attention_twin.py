"""The float64 twin of the forward attention kernels (csrc/attention.hip: rpe_bias_kernel, attention_kernel<D>, attention_x6_kernel and
their stack-mode entry points): plain PyTorch on the CPU, float64 throughout.  tests/test_attention_twin_cpu.py pins the twin and the
cases; tests/test_gpu_attention_edges.py holds the kernels to it.

The hidden states are the dtype-generic restatements of se3et_amd/autograd.py (rpe_attention, cross_attention) called with float64
tensors; the relative-position logits and the softmax in front of the values are written out here, because ops.rpe_bias returns the
logits alone and SF.rpe_attention can return the scores.  Called with float32 tensors (convert=f32) the same functions are the float32
restatement: the yardstick of the allowed error.

The second half builds the inputs that both test files share, the two error figures and the rule for the allowed error."""
import math

import torch
import torch.nn.functional as F

from backward_twin import F64, f32, f64
from se3et_amd import autograd as AG

F32_EPS = 1.2e-7              # a floor for a restatement that happens to round exactly
CEILING = 1e-4                # the project's figure (BASELINE.json): the allowed error never exceeds it
FACTOR = 16.0                 # 4 (split products keep 2^-22 per term against float32's 2^-24) x 2 (__expf, reciprocal) x 2 (association)
FACTOR_BF16_LOGITS = 1024.0   # the logits kernel with a bf16 embedding splits the folded queries into bf16 hi + lo: 2^-16 per term, not 2^-22
SMALL_ROW = 1e-3              # a row whose own maximum is below this share of the tensor's is measured against that share instead

PEAK_SCALE = 2.75             # `peaked`: the queries times this
OFFSET_CONST = 4.75           # `offset`: the embedding's part that is constant along the keys, times randn
OFFSET_RANDOM = 0.25          # ... and its random part
RAMP_QUERY = 0.05             # `late` / `early`: the queries' random part times this,
RAMP_SHIFT = 1.0              # ... every query moved by this along the unit diagonal u
RAMP_HEIGHT = 192.0           # ... and key m by RAMP_HEIGHT (2 m / (M - 1) - 1) u (`early`: the negative)
KINDS = ('plain', 'peaked', 'offset', 'late', 'early')


def key_stride(M):
    """ops.key_stride, restated so that this module loads without the native library."""
    return (M + 31) // 32 * 32


# ---------------------------------------------------------------------------------------------------------------------------------------
# the operations
# ---------------------------------------------------------------------------------------------------------------------------------------
def rpe_logits(q, emb, w_p, eq_emb, w_eq, H):
    """The relative-position term alone, (W_p^T q).e [+ (W_eq^T q).e_eq], unscaled: q (A, N, C), emb (N, M, C), w_p (C, C), eq_emb
    (A, N, M, 4), w_eq (C, 4) -> (A * H, N, M) in the dtype of the inputs."""
    A, N, C = q.shape
    d = C // H
    qh = q.reshape(A, N, H, d)
    qp = torch.einsum('anhd,hdc->anhc', qh, w_p.reshape(H, d, C))
    out = torch.einsum('anhc,nmc->ahnm', qp, emb)
    if eq_emb is not None:
        qe = torch.einsum('anhd,hde->anhe', qh, w_eq.reshape(H, d, 4))
        out = out + torch.einsum('anhe,anme->ahnm', qe, eq_emb)
    return out.reshape(A * H, N, emb.shape[1])


def scaled_logits(q, k, emb, w_p, eq_emb, w_eq, H):
    """(q.k + rpe_logits) / sqrt(d) -> (A, H, N, M): what the softmax sees."""
    A, N, C = q.shape
    M, d = k.shape[1], C // H
    s = torch.einsum('anhd,amhd->ahnm', q.reshape(A, N, H, d), k.reshape(A, M, H, d))
    return (s + rpe_logits(q, emb, w_p, eq_emb, w_eq, H).reshape(A, H, N, M)) / math.sqrt(d)


def rpe_scores(q, k, emb, w_p, eq_emb, w_eq, H):
    return torch.softmax(scaled_logits(q, k, emb, w_p, eq_emb, w_eq, H), -1)


def rpe_attention(q, k, vt, emb, w_p, eq_emb, w_eq, H):
    """rpe_transformer.py:85-131 (the restatement follows the dtype of its inputs)."""
    return AG.rpe_attention(q, k, vt, emb, w_p, eq_emb, w_eq, H)


def cross_attention(q, k, vt, H):
    """vanilla_transformer.py:39-85 with shared (C, >= M) or per-anchor (A, C, >= M) transposed values."""
    return AG.cross_attention(q, k, vt, H)


def transposed_values(v):
    """([A,] M, C) -> ([A,] C, key_stride(M)), zero beyond M."""
    M = v.shape[-2]
    return F.pad(v.transpose(-1, -2), (0, key_stride(M) - M)).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the error figures and the allowed error
# ---------------------------------------------------------------------------------------------------------------------------------------
def error_figures(got, want):
    """(global, per row) of got against want (..., rows, columns).  global: max |got - want| / max |want|.  per row: for every row of the
    last axis (an (anchor, query) row of the hidden states, an (anchor . head, query) row of the logits or scores) max |got - want| over
    the row / max |want| over the row, a row below SMALL_ROW of the tensor's maximum measured against that share; the largest of them."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    d = (got - want).abs()
    top = max(float(want.abs().max()), 1e-300)
    rows = torch.clamp(want.abs().amax(-1), min=SMALL_ROW * top)
    return float(d.max()) / top, float((d.amax(-1) / rows).max())


def allowed(restatement_figure, factor=FACTOR):
    """min(1e-4, factor x max(r, 1.2e-7)), r the same figure of the float32 restatement against the twin -- never of the kernel."""
    return min(CEILING, factor * max(restatement_figure, F32_EPS))


def check(got, want, restatement, factor=FACTOR):
    """-> [(figure name, kernel error, restatement error, allowed)] for the two figures."""
    k, r = error_figures(got, want), error_figures(restatement, want)
    return [(name, ke, re, allowed(re, factor)) for name, ke, re in zip(('global', 'per row'), k, r)]


def rejected(figures):
    return any(k > a for _, k, _, a in figures)


# ---------------------------------------------------------------------------------------------------------------------------------------
# shared inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _ramp(M, kind):
    r = torch.linspace(-1.0, 1.0, M) if M > 1 else torch.zeros(1)
    return RAMP_HEIGHT * (r if kind == 'late' else -r)


def _embedding(rn, N, M, C, kind):
    if kind == 'offset':
        return OFFSET_RANDOM * rn(N, M, C) + OFFSET_CONST * rn(N, 1, C)
    return rn(N, M, C)


def attention_case(A, C, H, eq, seed, kind='plain', pair=None, lengths=None):
    """The inputs of one RPE attention case, float32 on the CPU.

    pair = (N, M): one pair in projected form, as SF.rpe_attention takes it.  -> dict(q (A, N, C), k (A, M, C), vt (A, C, key_stride(M)),
    emb (N, M, C), w_p (C, C), eq_emb (A, N, M, 4) or None, w_eq (C, 4) or None).

    lengths = (N_0, N_1, ...): the clouds of one stack-mode self-attention call, as SF.rpe_self_attention_packed takes them: it projects
    q, k and the folded queries itself, so the case holds the rows in front of the projections, xs[c] (A, N_c, C), and the weights w_q,
    b_q, w_k, b_k, w_v, b_v; embs[c], eq_embs[c], w_p, w_eq as above.  self_attention() below projects them in the dtype asked for, so
    the float32 restatement carries the projection's rounding as the kernels' GEMM does.

    kind: `plain` unit randn; `peaked` queries x PEAK_SCALE; `offset` emb = OFFSET_RANDOM randn + OFFSET_CONST randn constant along the
    keys; `late` / `early` every query = RAMP_QUERY randn moved by RAMP_SHIFT along the unit diagonal u of the channels and key m moved by
    the ramp +- RAMP_HEIGHT (2 m / (M - 1) - 1) u, so the logit rises (falls) with the key index.  For a stack the ramp goes into the rows
    along a unit direction w of the inputs that W_q and W_v send to 0 and W_k to u, and the queries' shift into b_q.

    The constants.  The stress conditions of tests/test_attention_twin_cpu.py pull two ways: the float32 restatement must stay below
    1e-4 / 16 = 6.25e-6 per row (its error grows with the size of the logits), and with 97 keys the fourth key tile holds ONE key, which has
    to beat the largest of the 32 before it in half of the rows: the ramp's step from key to key must be about the spread of the logits
    around it.  Hence a small random part of the queries (the spread that is left is the keys' and embeddings' own, times the shift) and
    a tall ramp on the keys; measured on the twin: 0.66 of the rows rise through all four tiles at 97 keys, all of them at 160; the
    restatement is at 2.0e-6 .. 4.0e-6 per row.  `peaked` x 2.75: 0.59 .. 0.65 of the rows above 0.5 at 4.3e-6 .. 5.1e-6 (x 4: 6.6e-6);
    `offset` 4.75: |row mean| / std 2.2 .. 2.3 at 4.7e-6 .. 5.5e-6 (4.0: 1.9, too flat)."""
    assert kind in KINDS and (pair is None) != (lengths is None)
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    u = torch.full((C,), C ** -0.5)
    case = dict(A=A, C=C, H=H, kind=kind)
    case['w_p'] = rn(C, C) / C ** 0.5
    case['w_eq'] = rn(C, 4) * 0.5 if eq else None
    if pair is not None:
        N, M = pair
        q, k, v = rn(A, N, C), rn(A, M, C), rn(A, M, C)
        if kind == 'peaked':
            q = q * PEAK_SCALE
        if kind in ('late', 'early'):
            q = RAMP_QUERY * q + RAMP_SHIFT * u
            k = k + _ramp(M, kind)[:, None] * u
        case.update(q=q, k=k, vt=transposed_values(v), emb=_embedding(rn, N, M, C, kind), eq_emb=rn(A, N, M, 4) if eq else None)
        return case
    for n in ('q', 'k', 'v'):
        case['w_' + n] = rn(C, C) / C ** 0.5
        case['b_' + n] = rn(C) * 0.1
    if kind == 'peaked':
        case['w_q'], case['b_q'] = case['w_q'] * PEAK_SCALE, case['b_q'] * PEAK_SCALE
    w = rn(C)
    w = w / w.norm()
    if kind in ('late', 'early'):
        away = torch.eye(C) - torch.outer(w, w)
        case['w_q'], case['w_v'] = RAMP_QUERY * case['w_q'] @ away, case['w_v'] @ away
        case['w_k'] = case['w_k'] @ away + torch.outer(u, w)
        case['b_q'] = RAMP_QUERY * case['b_q'] + RAMP_SHIFT * u
    case['lengths'] = tuple(lengths)
    case['xs'], case['embs'], case['eq_embs'] = [], [], []
    for n in lengths:
        x = rn(A, n, C)
        if kind in ('late', 'early'):
            x = x + _ramp(n, kind)[:, None] * w
        case['xs'].append(x)
        case['embs'].append(_embedding(rn, n, n, C, kind))
        case['eq_embs'].append(rn(A, n, n, 4) if eq else None)
    return case


def rounded_embedding(case):
    """The same case with the geometric embedding rounded to bfloat16 (held in float32): what the bf16 entry points are compared on."""
    out = dict(case)
    rnd = lambda e: e.to(torch.bfloat16).to(torch.float32)
    if 'emb' in case:
        out['emb'] = rnd(case['emb'])
    else:
        out['embs'] = [rnd(e) for e in case['embs']]
    return out


def projected(case, c, convert=f64):
    """Cloud c of a stack case in projected form, in the dtype of `convert`: (q, k, vt, emb, w_p, eq_emb, w_eq)."""
    x = convert(case['xs'][c])
    lin = lambda n: F.linear(x, convert(case['w_' + n]), convert(case['b_' + n]))
    return (lin('q'), lin('k'), transposed_values(lin('v')), convert(case['embs'][c]), convert(case['w_p']), convert(case['eq_embs'][c]),
            convert(case['w_eq']))


def pair_inputs(case, convert=f64):
    return tuple(convert(case[n]) for n in ('q', 'k', 'vt', 'emb', 'w_p', 'eq_emb', 'w_eq'))


def self_attention(case, convert=f64):
    """The hidden states (A, N_c, C) of every cloud of a stack case (convert=f32: the float32 restatement on the CPU)."""
    return [rpe_attention(*projected(case, c, convert), case['H']) for c in range(len(case['lengths']))]


def pair_attention(case, convert=f64):
    """-> (hidden (A, N, C), scores (A, H, N, M)) of a pair case."""
    q, k, vt, emb, w_p, eq_emb, w_eq = pair_inputs(case, convert)
    return rpe_attention(q, k, vt, emb, w_p, eq_emb, w_eq, case['H']), rpe_scores(q, k, emb, w_p, eq_emb, w_eq, case['H'])


def case_logits(case, convert=f64):
    """The scaled logits (A, H, N, M) of a pair case, or of every cloud of a stack case."""
    H = case['H']
    pick = lambda t: (t[0], t[1], t[3], t[4], t[5], t[6])
    if 'q' in case:
        return [scaled_logits(*pick(pair_inputs(case, convert)), H)]
    return [scaled_logits(*pick(projected(case, c, convert)), H) for c in range(len(case['lengths']))]


def stack_case_from(xs, embs, eq_embs, weights, H):
    """A stack case from given rows xs[c] (A, N_c, C), embeddings and weights (w_q, b_q, w_k, b_k, w_v, b_v, w_p, w_eq): for inputs that
    come from a fixture."""
    case = dict(weights, A=xs[0].shape[0], C=xs[0].shape[-1], H=H, kind='plain', lengths=tuple(x.shape[1] for x in xs), xs=list(xs),
                embs=list(embs), eq_embs=list(eq_embs))
    return case


# the shapes that tests/test_gpu_attention_edges.py runs, and tests/test_attention_twin_cpu.py asserts the stress conditions at
STACK_EDGE_LENGTHS = ((1,), (31, 32, 33), (64, 65, 96, 97), (129, 1, 128), (160, 7))
STACK_STRESS_LENGTHS = (97, 160)
STACK_STRESS_KINDS = ('peaked', 'offset', 'late', 'early')
PAIR_SHAPES = ((1, 1), (33, 31), (32, 32), (5, 65), (40, 97), (3, 129))
PAIR_STRESS = (('late', (40, 97)), ('peaked', (40, 97)))               # at C = 256
PAIR_CHANNELS = (32, 64, 128, 256)


def stack_stress_case(kind):
    return attention_case(6, 256, 4, True, seed=97, kind=kind, lengths=STACK_STRESS_LENGTHS)


def pair_case(C, N, M, kind='plain'):
    return attention_case(6, C, 4, True, seed=1000 * N + M + C, kind=kind, pair=(N, M))


LOGITS_HEADS = ((1, 4), (4, 4), (5, 4), (6, 4), (8, 4), (2, 8), (6, 2))            # (A, H): AH = 4 / 16 / 20 / 24 / 32 / 16 / 12
LOGITS_SHAPES = ((5, 65), (33, 31))
LOGITS_CASES = [(A, H, 64, N, M) for A, H in LOGITS_HEADS for N, M in LOGITS_SHAPES] + \
               [(6, 4, C, N, M) for C in (32, 128, 256) for N, M in LOGITS_SHAPES]


def logits_case(A, H, C, N, M):
    return attention_case(A, C, H, True, seed=10000 * A + 1000 * H + C + N + M, pair=(N, M))


def logits_twin(case, convert=f64):
    """-> (the relative-position logits (A * H, N, M), the folded queries qp (A, N, H * C) and qe (A, N, 4 * H) they are formed from)."""
    q, _, _, emb, w_p, eq_emb, w_eq = pair_inputs(case, convert)
    A, N, C = q.shape
    H = case['H']
    qh = q.reshape(A, N, H, C // H)
    qp = torch.einsum('anhd,hdc->anhc', qh, w_p.reshape(H, C // H, C)).reshape(A, N, H * C)
    qe = torch.einsum('anhd,hde->anhe', qh, w_eq.reshape(H, C // H, 4)).reshape(A, N, 4 * H)
    return rpe_logits(q, emb, w_p, eq_emb, w_eq, H), qp, qe


def cross_case(pairs, C, anchors, seed):
    """The plain cross attention of a batch: for every pair (N, M) queries (N, C), keys (M, C) and values (M, C) (anchors = 0: shared) or
    (anchors, M, C)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return [dict(q=rn(N, C), k=rn(M, C), v=rn(anchors, M, C) if anchors else rn(M, C)) for N, M in pairs]


def cross_twin(pair, H, convert=f64):
    out = cross_attention(convert(pair['q']), convert(pair['k']), transposed_values(convert(pair['v'])), H)
    return out if out.dim() == 3 else out[None]


# ---------------------------------------------------------------------------------------------------------------------------------------
# what the stress kinds must show (asserted on the twin's own softmax by tests/test_attention_twin_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
def stress_statistics(s, kind):
    """s: the twin's scaled logits (A, H, N, M) of one cloud -> dict of the figures that the kind's conditions are about."""
    M = s.shape[-1]
    rows = s.reshape(-1, M)
    if kind == 'peaked':
        return dict(peaked_rows=float((torch.softmax(rows, -1).amax(-1) > 0.5).double().mean()))
    if kind == 'offset':
        return dict(mean_over_std=float(rows.mean(-1).abs().median() / rows.std(-1).median()),
                    median_mean=float(rows.mean(-1).abs().median()), std=float(rows.std(-1).max()))
    quarter = (M + 3) // 4
    top = rows.argmax(-1)
    out = dict(outer_quarter=float(((top >= M - quarter) if kind == 'late' else (top < quarter)).double().mean()))
    tiles = key_stride(M) // 32
    if tiles >= 3:                       # the kernels' own tiles: 32 keys from key 0, the last one short
        tops = torch.stack([rows[:, 32 * t:min(32 * t + 32, M)].amax(-1) for t in range(tiles)], -1)
        step = (tops[:, 1:] > tops[:, :-1]) if kind == 'late' else (tops[:, 1:] < tops[:, :-1])
        out['monotone_rows'] = float(step.all(-1).double().mean())
    return out
