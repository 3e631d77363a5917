"""The float64 twin of the KPConvInterSO3 forward (csrc/kpconv_mfma.hip, csrc/kpconv_union.hip, csrc/kpconv_so3.hip, dispatched by
ops.kpconv_inter_so3): plain PyTorch on the CPU, float64 from the float32 inputs.  tests/test_kpconv_twin_cpu.py pins the twin, the judge
and the cases; tests/test_gpu_kpconv_edges.py holds every form of the operator to it.

    out[p, r, d] = sum_{k, a, c} F[p, k, a, c] W[kidx[k, r], ridx[a, r], c, d],    F[p, k, a, c] = sum_n w[p, n, k] x[idx[p, n], a, c],
    w[p, n, k] = max(0, 1 - |s[idx[p, n]] - q[p] - kp[k]| / sigma)

An index outside [0, Ns) names the shadow row (features 0); a row that a list names several times counts as often as it appears.

The judge is the one of tests/attention_twin.py: two figures, `global` (max |got - want| / max |want|) and `per row` (the same per output
row (p, r), a row below 1e-3 of the tensor's maximum measured against that share), both allowed min(1e-4, 16 x max(r, 1.2e-7)) with r the
same figure of the float32 restatement (se3et_amd.autograd.kpconv_inter_so3 on the CPU, on the same inputs) against the twin -- never of
the kernel.  16 = 4 (the split products keep 2^-22 per term against float32's 2^-24) x 2 (two split stages: x -> orbit sums, orbit sums
-> output) x 2 (another association of the sums).

craft() builds a case from explicit per-point valid counts (the kernels' schedule branches on them); CASES names every case that the GPU
test runs, so that the CPU test can hold each of them to what it claims."""
import functools

import torch

from attention_twin import CEILING, F32_EPS, FACTOR, SMALL_ROW, allowed, check, error_figures, rejected      # noqa: F401  (one judge for all twins)
from backward_twin import F64
from se3et_amd import autograd as AG
from se3et_amd import tables

RADIUS, SIGMA = 0.0625, 0.05
BOX = 2 * SIGMA               # the crafted points lie in a box of this edge: most weights are non-zero
ON_KERNEL_POINT = 3           # the kernel point that one support point is put exactly on
LADDER = (0, 1, 7, 8, 9, 31, 32, 33, 39, 40, 41, 63, 64)      # valid counts around nv > 0, the 32-slot round, the 40-slot EXT round, the tail pair
ARG_NAMES = ('x', 'q_pts', 's_pts', 'idx', 'kernel_points', 'weights', 'kidx', 'ridx', 'sigma')


# ---------------------------------------------------------------------------------------------------------------------------------------
# the operation
# ---------------------------------------------------------------------------------------------------------------------------------------
def forward(x, q_pts, s_pts, idx, kernel_points, weights, kidx, ridx, sigma):
    """The formula above in float64 -> (P, 6, Cout).  One anchor r at a time, so that the expanded weights stay (K, A, Cin, Cout)."""
    x, q, s, kp, W = [t.detach().cpu().to(F64) for t in (x, q_pts, s_pts, kernel_points, weights)]
    idx, kidx, ridx = idx.detach().cpu().long(), kidx.detach().cpu().long(), ridx.detach().cpu().long()
    Ns = s.shape[0]
    safe = torch.where((idx < 0) | (idx >= Ns), torch.full_like(idx, Ns), idx)
    xs = torch.cat((x, torch.zeros_like(x[:1])))                                   # the shadow row
    sp = torch.cat((s, torch.full((1, 3), 1e6, dtype=F64)))
    nb = sp[safe] - q[:, None]                                                     # (P, NN, 3)
    w = (1 - (nb[:, :, None] - kp[None, None]).norm(dim=-1) / float(sigma)).clamp(min=0)      # (P, NN, K)
    Fk = torch.einsum('pnk,pnac->pkac', w, xs[safe])
    out = [torch.einsum('pkac,kacd->pd', Fk, W[kidx[:, r]][:, ridx[:, r]]) for r in range(ridx.shape[1])]
    return torch.stack(out, 1)


def state(Cin, Cout, seed=0):
    """A layer's constants as the model holds them: the 15 kernel points, weights (6, 6, Cin, Cout), kidx (15, 6), ridx (6, 6)."""
    g = torch.Generator().manual_seed(seed)
    return {'kernel_points': torch.from_numpy(tables.kernel_points(RADIUS)),
            'weights': torch.randn(6, 6, Cin, Cout, generator=g) / (36 * Cin) ** 0.5,
            'kidx': torch.from_numpy(tables.kernel_slot_table()).contiguous(),
            'ridx': torch.from_numpy(tables.anchor_slot_table()).contiguous(),
            'sigma': SIGMA}


def args(case, convert=None):
    """The case's inputs in the order of the operator's arguments; convert: applied to every tensor (e.g. lambda t: t.cuda())."""
    vals = [case[n] for n in ARG_NAMES]
    return tuple(convert(v) if (convert is not None and torch.is_tensor(v)) else v for v in vals)


def twin(case):
    return forward(*args(case))


def restatement(case):
    """se3et_amd.autograd.kpconv_inter_so3 in float32 on the CPU: the yardstick of the allowed error."""
    with torch.no_grad():
        return AG.kpconv_inter_so3(*args(case))


def valid_counts(case):
    idx = case['idx']
    return ((idx >= 0) & (idx < case['s_pts'].shape[0])).sum(1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# crafted cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def ladder_counts(P, NN, start=0):
    vals = [v for v in LADDER if v <= NN]
    return [vals[(start + p) % len(vals)] for p in range(P)]


def craft(counts, NN, Ns, Cin, Cout, seed, lists=None, lens=None):
    """A case whose point p has exactly counts[p] valid list entries: counts[p] distinct rows of [0, Ns) (or lists[p], which may repeat a
    row), the list filled up to NN with the shadow index Ns and permuted, so that the valid entries do not sit in front (with a shadow
    entry in the list, slot 0 holds one).  Support points uniform in a box of 2 sigma, query points in its middle half.  Two support
    points are put by hand: one exactly on q + kp_k of a point that lists it (distance 0, weight 1), one farther than sigma from every
    kernel point of a point that lists it (a valid neighbour whose weights are all 0).  lens: the clouds of the stack (tile membership of
    the union kernel).  Everything from one seeded generator."""
    g = torch.Generator().manual_seed(seed)
    P = len(counts)
    st = state(Cin, Cout, seed)
    s_pts = torch.rand(Ns, 3, generator=g) * BOX
    q_pts = BOX / 4 + torch.rand(P, 3, generator=g) * BOX / 2
    idx = torch.full((P, NN), Ns, dtype=torch.int64)
    rows_of = []
    for p in range(P):
        if lists is not None and lists[p] is not None:
            rows = torch.as_tensor(lists[p], dtype=torch.int64)
        else:
            rows = torch.randperm(Ns, generator=g)[:counts[p]]
        assert rows.numel() == counts[p] <= NN and (rows.numel() == 0 or (0 <= int(rows.min()) and int(rows.max()) < Ns))
        rows_of.append(rows)
        entry = torch.full((NN,), Ns, dtype=torch.int64)
        entry[:rows.numel()] = rows
        entry = entry[torch.randperm(NN, generator=g)]
        if rows.numel() < NN and int(entry[0]) != Ns:
            hole = int((entry == Ns).nonzero()[-1])
            entry[0], entry[hole] = entry[hole].clone(), entry[0].clone()
        idx[p] = entry
    placed = {}
    listing = [p for p in range(P) if counts[p] > 0]
    if listing:
        p_on = listing[0]
        row_on = int(rows_of[p_on][0])
        s_pts[row_on] = q_pts[p_on] + st['kernel_points'][ON_KERNEL_POINT]
        placed['on'] = (p_on, row_on, ON_KERNEL_POINT)
        for p_far in listing[1:]:
            other = [int(r) for r in rows_of[p_far] if int(r) != row_on]
            if other:
                s_pts[other[0]] = q_pts[p_far] + 4 * SIGMA
                placed['far'] = (p_far, other[0])
                break
    x = torch.randn(Ns, 6, Cin, generator=g)
    case = dict(st, x=x, q_pts=q_pts.contiguous(), s_pts=s_pts.contiguous(), idx=idx, counts=list(counts), placed=placed,
                lens=list(lens) if lens is not None else [P])
    assert sum(case['lens']) == P
    return case


def geometric(P, Ns, NN, Cin, Cout, box, seed):
    """The geometry of the older tests: uniform points in a box, the NN nearest support points of every query inside the radius."""
    g = torch.Generator().manual_seed(seed)
    st = state(Cin, Cout, 0)
    s_pts = torch.rand(Ns, 3, generator=g) * box
    q_pts = s_pts.clone() if P == Ns else s_pts[torch.randperm(Ns, generator=g)[:P]].contiguous()
    d = ((q_pts[:, None] - s_pts[None]) ** 2).sum(-1)
    idx = d.topk(NN, dim=1, largest=False)[1]
    idx[d.gather(1, idx) > RADIUS ** 2] = Ns
    x = torch.randn(Ns, 6, Cin, generator=g)
    case = dict(st, x=x, q_pts=q_pts, s_pts=s_pts, idx=idx, placed={}, lens=[P])
    case['counts'] = valid_counts(case).tolist()
    return case


def shrink_point(case, p, share):
    """Scales the features of the rows that ONLY point p lists so that p's largest output is `share` of the tensor's (the output is
    linear in them): a row far below the tensor's maximum, as a point with few or faint neighbours has."""
    Ns = case['s_pts'].shape[0]
    mine = set(int(r) for r in case['idx'][p] if 0 <= int(r) < Ns)
    others = set(int(r) for q in range(case['idx'].shape[0]) if q != p for r in case['idx'][q] if 0 <= int(r) < Ns)
    assert mine and not (mine & others), 'point %d shares rows' % p
    out = twin(case).abs()
    ratio = float(out[p].max()) / float(torch.cat((out[:p], out[p + 1:])).max())
    case = dict(case, x=case['x'].clone())
    case['x'][sorted(mine)] *= share / ratio
    return case


# ---- the cases of tests/test_gpu_kpconv_edges.py --------------------------------------------------------------------------------------
LADDER_NN = (1, 8, 31, 32, 33, 40, 41, 64)                                          # NNp = 32, 40 and 80
LADDER_CHANNELS = ((8, 32), (24, 96), (16, 64), (32, 128), (64, 256))               # chunks 1, 3, 2, 4, 8; NCT 1, 3, 2, 4, 8
TILE_POINTS = (1, 15, 16, 17, 33)
SPLIT_SHAPES = tuple((P, Cin, Cout) for P in (9, 40) for Cin, Cout in ((64, 64), (128, 32), (256, 64)))        # z = 2, 4, 8 on 1 and 3 tiles
MAGNITUDES = (1e-6, 1e-3, 1.0, 3e2, 1e4, 1e8)
FIRST_LAYER = tuple((P, Cout) for Cout in (16, 64) for P in (1, 5, 64, 65))
UNION_PLANS = {'clouds': None, 'cap': 1, 'cap+1': 2, 'disjoint64': 8, 'same64': 1}     # name -> the passes of its (only) group


def _seed(*v):
    s = 17
    for t in v:
        s = (s * 1000003 + int(t)) % (2 ** 31 - 1)
    return s


def _ladder(NN, Cin, Cout):
    return craft(ladder_counts(48, NN, start=NN), NN, 96, Cin, Cout, _seed(1, NN, Cin))


def _tiles(kind):
    if kind == 'empty-middle':            # three tiles, the middle one without a single valid neighbour
        counts = ladder_counts(16, 38, 1) + [0] * 16 + ladder_counts(16, 38, 5)
        # (the draw of _seed(2, 0) holds a row in which the float32 restatement itself is at 6.6e-6 -- weights 1 - d / sigma next to 0 -- so
        # that the allowed error would be the 1e-4 cap: ill-conditioned for float32, hence another draw)
        return craft(counts, 38, 96, 16, 64, _seed(2, 0, 3))
    if kind == 'last-one-64':             # the last tile holds one point, and that point has 64
        return craft(ladder_counts(32, 64, 2) + [64], 64, 96, 16, 64, _seed(2, 1))
    return craft(ladder_counts(int(kind), 38, 3), 38, 96, 16, 64, _seed(2, 2, int(kind)))


def _split(P, Cin, Cout):
    return craft(ladder_counts(P, 38, P), 38, 96, Cin, Cout, _seed(3, P, Cin))


def _union_plan(kind):
    if kind == 'clouds':                  # every cloud starts a group: 1 + 1 + 2 + 2 groups, padding positions in all but one
        return craft(ladder_counts(65, 38, 4), 38, 96, 16, 64, _seed(4, 0), lens=(1, 16, 17, 31))
    if kind in ('cap', 'cap+1'):          # 16 points with pairwise disjoint lists of 8 rows: the union is exactly kUCap = 128 (one more row: it splits)
        lists = [list(range(8 * p, 8 * p + 8)) for p in range(16)]
        if kind == 'cap+1':
            lists[5].append(128)
        return craft([len(v) for v in lists], 12, 160, 16, 64, _seed(4, 1), lists=lists)
    if kind == 'disjoint64':              # 16 disjoint lists of 64: halved down to pairs of points, whose 2 x 64 rows fit the cap exactly
        lists = [list(range(64 * p, 64 * p + 64)) for p in range(16)]
        return craft([64] * 16, 64, 1100, 16, 64, _seed(4, 2), lists=lists)
    lists = [list(range(10, 74)) for _ in range(16)]                                # every point the same 64 rows
    return craft([64] * 16, 64, 96, 16, 64, _seed(4, 3), lists=lists)


def _repeats():
    """Point 0 names a row twice among 9 entries, point 1 a row three times among 40; the other points climb the ladder."""
    counts = ladder_counts(20, 40, 6)
    lists = [None] * 20
    lists[0] = [3, 11, 3, 20, 21, 22, 23, 24, 25]
    lists[1] = [40, 40, 40] + list(range(41, 78))
    counts[0], counts[1] = len(lists[0]), len(lists[1])
    return craft(counts, 40, 96, 16, 64, _seed(5), lists=lists)


def _magnitude(scale):
    """The shape of test_fused_kpconv_input_scale_over_magnitudes with a plain float32 tensor."""
    case = geometric(400, 400, 34, 32, 64, 0.12, 11)
    case['x'] = case['x'] * scale
    return case


def _row0():
    """Only support row 0 is large, and no list names it."""
    case = geometric(400, 400, 34, 32, 64, 0.12, 11)
    case['idx'][case['idx'] == 0] = 400
    case['counts'] = valid_counts(case).tolist()
    case['x'][0] = 1e6
    return case


def _first_layer(P, Cout):
    return craft(ladder_counts(P, 19, P), 19, 96, 1, Cout, _seed(6, P, Cout))


CASES = {}
CASES.update({'ladder NN %d (%d, %d)' % (NN, ci, co): functools.partial(_ladder, NN, ci, co) for NN in LADDER_NN for ci, co in LADDER_CHANNELS})
CASES.update({'tiles %s' % k: functools.partial(_tiles, k) for k in [str(p) for p in TILE_POINTS] + ['empty-middle', 'last-one-64']})
CASES.update({'split P %d (%d, %d)' % s: functools.partial(_split, *s) for s in SPLIT_SHAPES})
CASES.update({'union %s' % k: functools.partial(_union_plan, k) for k in UNION_PLANS})
CASES['repeats'] = _repeats
CASES.update({'magnitude %g' % s: functools.partial(_magnitude, s) for s in MAGNITUDES})
CASES['row 0 large'] = _row0
CASES.update({'first layer P %d Cout %d' % s: functools.partial(_first_layer, *s) for s in FIRST_LAYER})


@functools.lru_cache(maxsize=None)
def case(name):
    """The named case with its twin and restatement, computed once and shared (nobody changes them)."""
    c = CASES[name]()
    c['name'] = name
    c['twin'] = twin(c)
    c['restatement'] = restatement(c)
    return c
