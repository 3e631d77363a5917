"""The float64 twin of the training step's hand-written backward kernels (csrc/sinkhorn.hip sinkhorn_bwd_kernel, csrc/rowops.hip gn_bwd_*,
add_ln_bwd_kernel, neighbor_max_bwd_kernel, scatter_add_rows_fixed_kernel, csrc/kpconv_so3.hip kpconv_scatter_kernel): plain PyTorch on the
CPU, float64 throughout, one function per operation and gradients by autograd through it.  tests/test_backward_twin_cpu.py pins the twin
itself (finite differences, the max-pool tie table); tests/test_gpu_backward_edges.py holds the kernels to it.

Where a restatement of se3et_amd/autograd.py is dtype-generic the twin calls it with float64 tensors (Sinkhorn, add + LayerNorm, the padded
gather, KPConv); GroupNorm is written out here because the tests need the value in front of the LeakyReLU, and the max-pool because the
twin states the tie rule itself: torch.max(dim) takes ONE index, the first in table order.

The second half builds the inputs that both test files share (the GPU test runs the kernels on them, the CPU test asserts what can be
asserted about them without a GPU)."""
import torch
import torch.nn.functional as F

from se3et_amd import autograd as AG

F64 = torch.float64
KINK_WINDOW = 1e-5            # an element whose pre-activation is within this share of the largest one may take either LeakyReLU slope
KINK_CAP = 1e-3               # at most this share of the elements of a case may sit in the window


def f64(t):
    """float tensors -> float64 on the CPU, everything else (index tables, masks, None) -> the CPU unchanged."""
    if t is None:
        return None
    t = t.detach().cpu()
    return t.to(F64) if t.is_floating_point() else t


def f32(t):
    if t is None:
        return None
    t = t.detach().cpu()
    return t.to(torch.float32) if t.is_floating_point() else t


def vjp(fn, inputs, cotangent, convert=f64):
    """out = fn(*inputs) on converted copies; -> (out, [d <out, cotangent> / d input] for every floating-point input, None for the others)."""
    leaves = []
    for t in inputs:
        c = convert(t) if torch.is_tensor(t) else t
        if torch.is_tensor(c) and c.is_floating_point():
            c = c.clone().requires_grad_(True)
        leaves.append(c)
    out = fn(*leaves)
    first = out[0] if isinstance(out, tuple) else out
    wanted = [t for t in leaves if torch.is_tensor(t) and t.requires_grad]
    got = iter(torch.autograd.grad(first, wanted, convert(cotangent), allow_unused=True))
    grads = []
    for t in leaves:
        if torch.is_tensor(t) and t.requires_grad:
            g = next(got)
            grads.append(torch.zeros_like(t) if g is None else g)
        else:
            grads.append(None)
    return (tuple(o.detach() for o in out) if isinstance(out, tuple) else out.detach()), grads


# ---------------------------------------------------------------------------------------------------------------------------------------
# the operations
# ---------------------------------------------------------------------------------------------------------------------------------------
def log_optimal_transport(scores, alpha, row_masks, col_masks, num_iterations, inf):
    """learnable_sinkhorn.py:13-66 (the restatement follows the dtype of `scores`)."""
    return AG.log_optimal_transport(scores, alpha, row_masks, col_masks, num_iterations, inf)


def group_norm_rows(x, weight, bias, residual, x_bias, groups, eps, leaky_slope, segments):
    """blocks_epn.py:684-701 on rows: GroupNorm of x [+ x_bias] with statistics over (rows of the segment x channels of the group), affine,
    [+ residual], [LeakyReLU].  -> (y, pre): pre is the value in front of the LeakyReLU."""
    C = x.shape[-1]
    y = x.reshape(-1, C)
    if x_bias is not None:
        y = y + x_bias
    bounds = list(segments) if segments is not None else [0, y.shape[0]]
    outs = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        g = y[a:b].reshape(b - a, groups, C // groups)
        mean = g.mean((0, 2), keepdim=True)
        var = ((g - mean) ** 2).mean((0, 2), keepdim=True)
        outs.append(((g - mean) / torch.sqrt(var + eps)).reshape(b - a, C))
    pre = (torch.cat(outs, 0) * weight + bias).reshape(x.shape)
    if residual is not None:
        pre = pre + residual
    return (F.leaky_relu(pre, leaky_slope) if leaky_slope is not None else pre), pre


def add_layer_norm(hidden, residual, weight, bias, hidden_bias, eps):
    """LayerNorm(hidden [+ hidden_bias] + residual); the residual may lack leading (anchor) dims of hidden."""
    return AG.add_layer_norm(hidden, residual, weight, bias, hidden_bias, eps)


def neighbor_max_pool(x, idx):
    """blocks.py:93-110: the maximum over the gathered rows.  idx == len(x) addresses the zero row, idx < 0 (the width marker of stacked
    pairs) takes no part; torch.max(dim) gives the gradient to the first maximal entry in table order."""
    n = x.shape[0]
    xs = torch.cat((x, torch.zeros_like(x[:1])), 0)
    rows = xs[torch.where((idx < 0) | (idx > n), torch.full_like(idx, n), idx)]
    marker = (idx < 0).reshape(idx.shape + (1,) * (rows.dim() - 2))
    return rows.masked_fill(marker, float('-inf')).max(1)[0]


def gather_rows_padded(x, idx):
    return AG.gather_rows_padded(x, idx)


def kpconv_inter_so3(x, q_pts, s_pts, idx, kernel_points, weights, kidx, ridx, sigma):
    """blocks_epn.py:454-546."""
    return AG.kpconv_inter_so3(x, q_pts, s_pts, idx, kernel_points, weights, kidx, ridx, sigma)


def max_pool_winners(x, idx):
    """How many pooled rows hand the gradient of element (row, ...) of x to it: the number of contributions that meet there."""
    ones = torch.ones((idx.shape[0],) + tuple(x.shape[1:]), dtype=F64)
    return vjp(neighbor_max_pool, [x, idx], ones)[1][0]


# ---------------------------------------------------------------------------------------------------------------------------------------
# shared inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def sinkhorn_case(B, R, C, seed, scale=1.0):
    """scores (B, R, C) * scale, alpha, random masks with at least one valid row and column per pair; the LAST pair has exactly one valid row
    and one valid column, not the first where there is a choice; cotangent (B, R + 1, C + 1), zero on masked entries (the dustbin row and
    column are read); valid (B, R + 1, C + 1)."""
    g = torch.Generator().manual_seed(seed)
    scores = torch.randn(B, R, C, generator=g) * scale
    rm, cm = torch.rand(B, R, generator=g) > 0.2, torch.rand(B, C, generator=g) > 0.2
    rm[:, R // 2] = True
    cm[:, C // 3] = True
    rm[0], cm[0] = True, True
    rm[B - 1], cm[B - 1] = False, False
    rm[B - 1, min(R - 1, 1 + R // 2)] = True
    cm[B - 1, min(C - 1, 1 + C // 3)] = True
    valid = torch.ones(B, R + 1, C + 1, dtype=torch.bool)
    valid[:, :R] &= rm[:, :, None]
    valid[:, :, :C] &= cm[:, None, :]
    cot = torch.randn(B, R + 1, C + 1, generator=g) * valid
    return dict(scores=scores, alpha=torch.tensor(0.7), row_masks=rm, col_masks=cm, cot=cot, valid=valid)


def sinkhorn_twin(case, iters, inf=1e12, convert=f64):
    """-> (out, d scores, d alpha) of the twin (convert=f32: of the float32 restatement on the CPU)."""
    fn = lambda s, a: AG.log_optimal_transport(s, a, case['row_masks'], case['col_masks'], iters, inf)
    out, (ds, da) = vjp(fn, [case['scores'], case['alpha']], case['cot'], convert)
    return out, ds, da


GN_EDGE_SHAPES = ((60, 1024, 2), (66, 64, 64), (54, 40, 8), (6, 32, 4))        # (rows, C, groups); the case's seed is its row count
GN_VARIANTS = ((0.1, True, True), (None, False, False), (0.1, True, False), (0.1, False, True))       # (slope, residual, x_bias)


def group_norm_case(rows, C, seed, offset=0.0, with_res=True, with_xb=True, zero_rows=None, clear_kink=None):
    """x = randn + offset (rows, C), weight, bias, residual, x_bias, cotangent.  The affine weight keeps away from 0 and the bias is of unit
    size, so that the pre-activations spread over a unit range and few of them sit at the LeakyReLU kink.  clear_kink = (groups, eps, margin):
    the residual of every element whose pre-activation (the twin's) would be closer to 0 than `margin` is moved so that it sits `margin` or
    more away -- for inputs on which float32 arithmetic cannot place the pre-activation to within the kink window (a mean far from 0)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rn(rows, C) + offset
    if zero_rows is not None:
        x[zero_rows[0]:zero_rows[1]] = 0.0
    w = rn(C)
    w = torch.where(w >= 0, w + 0.25, w - 0.25)
    case = dict(x=x, weight=w, bias=rn(C), residual=rn(rows, C) if with_res else None, x_bias=rn(C) * 0.5 if with_xb else None,
                cot=rn(rows, C))
    if clear_kink is not None:
        groups, eps, margin = clear_kink
        with torch.no_grad():
            pre = group_norm_rows(*[f64(case[k]) for k in ('x', 'weight', 'bias', 'residual', 'x_bias')], groups, eps, None, None)[1]
        near = pre.abs() < margin
        push = torch.where(pre >= 0, 2 * margin, -2 * margin).float()
        case['residual'] = torch.where(near, case['residual'] + push, case['residual'])
    return case


def group_norm_offset_case(offset):
    """(1800, 32, 4 groups), x = randn + offset, every pre-activation 0.02 or more away from the kink."""
    return group_norm_case(1800, 32, seed=1800, offset=offset, clear_kink=(4, 1e-5, 0.02))


def group_norm_twin(case, groups, eps, slope, segments, convert=f64):
    """-> (y, pre, [dx, dweight, dbias, dresidual, dx_bias])."""
    fn = lambda x, w, b, r, xb: group_norm_rows(x, w, b, r, xb, groups, eps, slope, segments)
    (y, pre), grads = vjp(fn, [case['x'], case['weight'], case['bias'], case['residual'], case['x_bias']], case['cot'], convert)
    return y, pre, grads


def kink_mask(pre):
    return pre.abs() <= KINK_WINDOW * float(pre.abs().max())


SIXTEEN_SEGMENTS = [6 * p for p in (0, 20, 21, 23, 24, 26, 27, 29, 30, 32, 33, 35, 36, 37, 38, 39, 40)]      # points per segment: 20, 1, 2, 1, 2, ...


def kpconv_case(P, Ns, NN, Cin, Cout, seed, box=0.12, radius=0.0625, blind_every=None):
    """Random support points in a box, the first P of them as queries, the NN nearest support points of each (fewer than NN support points:
    the rest of the row is padding), those beyond the radius padded; blind_every = 3: every third query sees padding only."""
    from se3et_amd import tables
    g = torch.Generator().manual_seed(seed)
    s_pts = torch.rand(Ns, 3, generator=g) * box
    q_pts = s_pts[:P].contiguous()
    d = ((q_pts[:, None] - s_pts[None]) ** 2).sum(-1)
    near = d.topk(min(NN, Ns), dim=1, largest=False)[1]
    near[d.gather(1, near) > radius ** 2] = Ns
    idx = torch.full((P, NN), Ns, dtype=torch.int64)
    idx[:, :near.shape[1]] = near
    if blind_every:
        idx[::blind_every] = Ns
    return dict(x=torch.randn(Ns, 6, Cin, generator=g), q_pts=q_pts, s_pts=s_pts, idx=idx,
                kernel_points=torch.from_numpy(tables.kernel_points(radius)), weights=torch.randn(6, 6, Cin, Cout, generator=g) / (36 * Cin) ** 0.5,
                kidx=torch.from_numpy(tables.kernel_slot_table()), ridx=torch.from_numpy(tables.anchor_slot_table()), sigma=0.05,
                cot=torch.randn(P, 6, Cout, generator=g))


def kpconv_twin(case, convert=f64):
    """-> (out, dx, dW)."""
    fn = lambda x, w: AG.kpconv_inter_so3(x, convert(case['q_pts']), convert(case['s_pts']), case['idx'], convert(case['kernel_points']), w,
                                          case['kidx'], case['ridx'], case['sigma'])
    out, (dx, dw) = vjp(fn, [case['x'], case['weights']], case['cot'], convert)
    return out, dx, dw


def kpconv_blind_case():
    """Every third query sees padding only; some support rows are gathered by nobody."""
    return kpconv_case(45, 150, 20, 8, 16, seed=303, box=0.2, blind_every=3)


def kpconv_mixed_case():
    """Unit-scale cotangent, except that the rows of ONE query are scaled by 1e6: -> (case, the query, mask of the support rows it reaches)."""
    case = kpconv_case(90, 140, 24, 16, 32, seed=404)
    refs = (case['idx'] < 140).sum(1)
    loud = int(refs.argmax())
    case['cot'][loud] *= 1e6
    reached = torch.zeros(140, dtype=torch.bool)
    reached[case['idx'][loud][case['idx'][loud] < 140]] = True
    return case, loud, reached


def kpconv_fixed_resolution(case):
    """The bound that csrc/kpconv_so3.hip documents for its 64-bit fixed-point sums: a contribution is resolved to
    bound * 2^-(54 - 7 - ceil(log2(P + 1))), with bound = max |dout| * max |W| * Cout formed in float32 exactly as ops.kpconv_inter_so3_bwd
    forms it.  -> (resolution, number of contributions per support row)."""
    P, Ns = case['idx'].shape[0], case['x'].shape[0]
    Cout = case['weights'].shape[-1]
    d2, W2 = case['cot'].float().reshape(P * 6, Cout), case['weights'].float().reshape(-1, Cout)
    bound = (torch.linalg.vector_norm(d2, float('inf')) * torch.linalg.vector_norm(W2, float('inf'))).mul_(float(Cout))
    lg = 1
    while (1 << lg) < P + 1:
        lg += 1
    count = torch.bincount(case['idx'].reshape(-1), minlength=Ns + 1)[:Ns]
    return float(bound.double()) * 2.0 ** -(54 - 7 - lg), count


def max_pool_tie_cases():
    """The tie table: x (4, 2) with rows 0, 1, 2 exactly equal in column 0, and four pooled rows.  n = 4 is the padded (zero) entry, -1 the
    width marker.  -> (x, idx, cotangent, expected dx)."""
    x = torch.tensor([[1.5, 0.0], [1.5, -2.0], [1.5, -3.0], [-1.0, 0.0]])
    idx = torch.tensor([[2, 0, 1, -1],          # three tied real neighbours in column 0: the first in table order (row 2) takes all
                        [0, 4, 3, 3],           # column 1: a real 0.0 (row 0) in front of a padded entry: the real row takes it
                        [4, 0, 3, 3],           # column 1: a padded entry in front of the real 0.0: nothing flows
                        [-1, 3, -1, -1]])       # the marker never wins, although row 3 holds -1.0 < 0
    cot = torch.tensor([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0], [8.0, 80.0]])
    want = torch.zeros(4, 2, dtype=F64)
    want[2, 0] += 1.0        # row 0, column 0: tie of x[2], x[0], x[1] -> x[2]
    want[0, 1] += 10.0       # row 0, column 1: 0.0 (x[0]) beats -3, -2
    want[0, 0] += 2.0        # row 1, column 0: 1.5 (x[0]) beats the zero row and -1
    want[0, 1] += 20.0       # row 1, column 1: x[0] = 0.0 in front of the padded 0
    want[0, 0] += 4.0        # row 2, column 0: 1.5 beats the padded 0 in front of it
    #                          row 2, column 1: the padded 0 comes first: nothing
    want[3, 0] += 8.0        # row 3: only x[3] is real
    want[3, 1] += 80.0
    return x, idx, cot, want
