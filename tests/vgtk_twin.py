"""TEST INFRASTRUCTURE: float64 / integer twins of the EPN toolkit kernels (se3et_amd/csrc/vgtk_ops.hip), their float32 restatements,
the allowances, and the crafted edge cases that tests/test_gpu_vgtk_edges.py (GPU) and tests/test_vgtk_twin_cpu.py (no GPU) share.

A second, independent statement of every operation: written from the definitions in the kernel file's comments and the reference's
semantics, it does not import oracle/vgtk_oracle.py (tests/test_vgtk_twin_cpu.py compares the two).  numpy / torch on the host only.

  gather            indexing; backward as a float64 index_add AND as the float32 in-order sum (ascending j, additions only: the order
                    is the kernel's contract, so this statement is bit-reproducible)
  ball query        float64: the first nsample ascending indices with d^2 < r^2, cyclic repetition, the zero last slot
  fps               the reference's LITERAL reduction: bs threads with a first strict maximum each, then pairwise updates at strides
                    bs/2 .. 1 that take the upper slot only when it is strictly larger -- deliberately not a selection key
  inter / intra     float64 einsum and autograd of the definitions, with Sigma |w f| and the number of terms of every element
  anchor queries    float64 on the float32 inputs; counts as integers

Allowances (nothing in them is measured on a kernel):
  in-order float32 sum of L terms           L 2^-24 Sigma |terms|            (gather backward; additions only)
  ... of L rounded or fused products        (L + 2) 2^-24 Sigma |w f|        (both zpconv ops, forward and backward)
  anchor queries                            min(1e-4, 8 max(r, 1.2e-7)) of the largest |want|, r the float32 restatement's error
                                            (the rule of tests/test_gpu_dense_edges.py)"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24                      # unit round-off of float32
F32 = np.float32


def cached(fn):
    return functools.lru_cache(maxsize=None)(fn)


def frozen(a):
    """References are computed once and shared: nobody changes them."""
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# =======================================================================================================================================
# gather_points
# =======================================================================================================================================
def gather_fwd(points, idx):
    """points (b, c, n), idx (b, m) -> (b, c, m)."""
    return np.stack([points[bi][:, idx[bi].astype(np.int64)] for bi in range(points.shape[0])])


def gather_bwd_f64(grad_out, idx, n):
    """-> (float64 index_add (b, c, n), number of terms per target (b, n), Sigma |terms| (b, c, n))."""
    b, c, m = grad_out.shape
    want, mag, cnt = np.zeros((b, c, n)), np.zeros((b, c, n)), np.zeros((b, n), np.int64)
    for bi in range(b):
        j = idx[bi].astype(np.int64)
        np.add.at(cnt[bi], j, 1)
        for ci in range(c):
            np.add.at(want[bi, ci], j, grad_out[bi, ci].astype(np.float64))
            np.add.at(mag[bi, ci], j, np.abs(grad_out[bi, ci].astype(np.float64)))
    return want, cnt, mag


def gather_bwd_f32_in_order(grad_out, idx, n):
    """float32 sums in ascending j starting from 0: round r adds the r-th occurrence of every target (the targets of a round are distinct)."""
    b, c, m = grad_out.shape
    out = np.zeros((b, c, n), F32)
    for bi in range(b):
        j = idx[bi].astype(np.int64)
        order = np.argsort(j, kind='stable')
        js = j[order]
        start = np.r_[0, np.nonzero(js[1:] != js[:-1])[0] + 1] if len(js) else np.zeros(0, np.int64)
        rank = np.arange(len(js)) - np.repeat(start, np.diff(np.r_[start, len(js)]))
        by_rank = np.argsort(rank, kind='stable')
        bounds = np.searchsorted(rank[by_rank], np.arange(rank.max() + 2)) if len(js) else [0]
        for r in range(len(bounds) - 1):
            e = order[by_rank[bounds[r]:bounds[r + 1]]]
            out[bi][:, j[e]] = out[bi][:, j[e]] + grad_out[bi][:, e]
    return out


def gather_wave_trips(c):
    """Passes that each of the four waves of the PARENT's gather backward makes: `for (c0 = cg; c0 < c; c0 += 32)` counted literally."""
    trips = []
    for cg in range(4):
        t, c0 = 0, cg
        while c0 < c:
            t, c0 = t + 1, c0 + 32
        trips.append(t)
    return trips


def gather_bwd_parent_schedule(grad_out, idx, n, chunk=2048):
    """Host emulation of the parent's gather backward: a wave leaves after its own last pass; departed threads stage nothing, so their
    slots of the 2048-entry stage keep what the last write left there (LDS assumed to start at zero; a departed wave is assumed to simply
    stop taking part in the barriers).  -> (gradient float64, True if a scanned slot was never staged at all)."""
    b, c, m = grad_out.shape
    out = np.zeros((b, c, n))
    trips = gather_wave_trips(c)
    owner = (np.arange(chunk) % 256) >> 6                      # the wave whose threads stage slot t
    unwritten_read = False
    for bi in range(b):
        j = idx[bi].astype(np.int64)
        sidx, written = np.zeros(chunk, np.int64), np.zeros(chunk, bool)
        for p in range(max(trips)):
            staging = np.array([trips[w] > p for w in range(4)])[owner]
            chans = [ch for ch in range(32 * p, min(32 * p + 32, c))]
            for j0 in range(0, m, chunk):
                cnt = min(chunk, m - j0)
                t = np.nonzero(staging[:cnt])[0]
                sidx[t], written[t] = j[j0 + t], True
                unwritten_read |= not written[:cnt].all()
                hit = sidx[:cnt] < n
                for ch in chans:
                    np.add.at(out[bi, ch], sidx[:cnt][hit], grad_out[bi, ch, j0:j0 + cnt][hit].astype(np.float64))
    return out, unwritten_read


GATHER_C = (1, 2, 3, 4, 5, 31, 32, 33, 34, 35, 36, 64, 65, 67)
GATHER_M = (0, 1, 2047, 2048, 2049, 4097, 6145)
GATHER_N = (1, 63, 64, 65, 130)
GATHER_PATTERNS = ('uniform', 'one', 'sparse')


def gather_shapes():
    """(c, n, m) of the grid, each once."""
    s = [(c, 65, 4097) for c in GATHER_C] + [(c, 65, m) for c in (3, 34) for m in GATHER_M] + [(3, n, 4097) for n in GATHER_N]
    return list(dict.fromkeys(s))


@cached
def gather_case(c, n, m, pattern):
    """b = 2, the two batch elements differ.  `sparse` draws its targets from one 64-target workgroup alone where there are several (the
    second in batch element 0, the first in 1: the other workgroups must come out exactly 0), else from every second / third target."""
    g = np.random.default_rng(1000003 * c + 1009 * n + 7 * m + GATHER_PATTERNS.index(pattern))
    b = 2
    if pattern == 'uniform':
        idx = g.integers(0, n, (b, m))
    elif pattern == 'one':
        idx = np.stack([np.full(m, n - 1), np.zeros(m, np.int64)])
    else:
        pools = [np.arange(64, min(128, n)), np.arange(1, 64, 3)] if n > 64 else [np.arange(0, n, 2), np.arange(0, n, 3)]
        idx = np.stack([pool[g.integers(0, len(pool), m)] for pool in pools])
    points = g.standard_normal((b, c, n)).astype(F32)
    cot = g.standard_normal((b, c, m)).astype(F32)
    idx = idx.astype(np.int32)
    want64, cnt, mag = gather_bwd_f64(cot, idx, n)
    return dict(name='gather c=%d n=%d m=%d %s' % (c, n, m, pattern), c=c, n=n, m=m, pattern=pattern, points=frozen(points), idx=frozen(idx),
                cot=frozen(cot), fwd=frozen(gather_fwd(points, idx)), bwd32=frozen(gather_bwd_f32_in_order(cot, idx, n)), bwd64=frozen(want64),
                cnt=frozen(cnt), allowed=frozen(cnt[:, None, :] * U * mag),
                uniform_trips=(c % 32 == 0 or c % 32 >= 4), chunks=-(-m // 2048),
                empty_workgroups=[[w for w in range(-(-n // 64)) if not ((idx[bi] // 64) == w).any()] for bi in range(b)])


# =======================================================================================================================================
# ball query
# =======================================================================================================================================
def ball_query(new_xyz, xyz, radius, nsample):
    """new_xyz (b, 3, m), xyz (b, 3, n) -> (idx (b, m, nsample) int32, hits (b, m): support points with d^2 < r^2, uncut)."""
    q, s = np.asarray(new_xyz, np.float64), np.asarray(xyz, np.float64)
    b, _, m = q.shape
    r2 = float(radius) * float(radius)
    idx, total = np.zeros((b, m, nsample), np.int32), np.zeros((b, m), np.int64)
    for bi in range(b):
        for j in range(m):
            d2 = ((q[bi, :, j, None] - s[bi]) ** 2).sum(0)
            found = np.nonzero(d2 < r2)[0]
            total[bi, j] = len(found)
            found = found[:nsample]
            cnt = len(found)
            if cnt == 0:
                continue                                        # zeros
            if cnt < nsample - 1:
                idx[bi, j] = found[np.arange(nsample) % cnt]    # cyclic repetition
            else:
                idx[bi, j, :cnt] = found                        # cnt == nsample - 1: the last slot stays zero
    return idx, total


BALL_RADIUS = 2.0
_BALL_EDGE = np.array([[2, 0, 0], [0, 2, 0], [0, 0, 2], [-2, 0, 0], [0, -2, 0], [0, 0, -2]], np.float64)       # d^2 == r^2 exactly


def _ball_build(name, n, nsample, hits, edges, seed):
    """hits / edges: per batch element, per query, the support indices inside the ball / exactly on it (disjoint between the queries of a
    batch element).  Every coordinate is a multiple of 1/4 below 64; hits lie within sqrt(3) of their query, the rest at 48 or more."""
    g = np.random.default_rng(seed)
    b, m = len(hits), len(hits[0])
    q, s = np.zeros((b, 3, m)), np.zeros((b, 3, n))
    for bi in range(b):
        q[bi, 0], q[bi, 1:] = -32 + 16 * np.arange(m), 1.25 * bi
        s[bi] = np.stack([-60 + 0.25 * (np.arange(n) % 400), np.full(n, 48.0), np.full(n, 48.0 + 4 * bi)])
        used = set()
        for j in range(m):
            for k in hits[bi][j]:
                s[bi, :, k] = q[bi, :, j] + 0.25 * g.integers(-4, 5, 3)
            for e, k in enumerate(edges[bi][j]):
                s[bi, :, k] = q[bi, :, j] + _BALL_EDGE[(e + j) % 6]
            both = list(hits[bi][j]) + list(edges[bi][j])
            assert not used & set(both) and len(set(both)) == len(both)
            used |= set(both)
    q, s = q.astype(F32), s.astype(F32)
    want, total = ball_query(q, s, BALL_RADIUS, nsample)
    return dict(name=name, n=n, m=m, nsample=nsample, radius=BALL_RADIUS, query=frozen(q), support=frozen(s), want=frozen(want),
                hits=[[sorted(h) for h in hb] for hb in hits], edges=edges, total=frozen(total))


def _ball_grid_case(n, nsample, m):
    g = np.random.default_rng(7919 * n + 31 * nsample + m)
    classes = [0, 1, nsample - 2, nsample - 1, nsample, nsample + 1]
    hits, edges = [], []
    for bi in range(2):
        free = list(g.permutation(n))
        hb, eb = [], []
        for j in range(m):
            want = max(classes[(j + 2 * bi + n + nsample) % 6], 0)
            take = min(want, max(len(free) - (m - 1 - j), 0))
            hb.append(sorted(int(k) for k in free[:take]))
            free = free[take:]
            ne = min(1, max(len(free) - (m - 1 - j), 0))
            eb.append([int(k) for k in free[:ne]])
            free = free[ne:]
        hits.append(hb)
        edges.append(eb)
    return _ball_build('ball n=%d nsample=%d m=%d' % (n, nsample, m), n, nsample, hits, edges, n * 1000 + nsample)


@cached
def ball_cases():
    cases = []
    ms = (1, 3, 4, 5)
    for a, n in enumerate((1, 63, 64, 65, 128, 129)):
        for c, ns in enumerate((1, 2, 8, 64, 65)):
            cases.append(_ball_grid_case(n, ns, ms[(a + c) % 4]))
    # every hit class at nsample = 8 in one call of 6 queries a batch element, both with room to spare
    ns = 8
    lay = lambda order: [sorted(range(o, 129, 6))[:k] for o, k in zip(range(6), order)]
    cases.append(_ball_build('ball hit classes nsample=8', 129, ns, [lay([0, 1, 6, 7, 8, 9]), lay([9, 8, 7, 6, 1, 0])], [[[]] * 6, [[]] * 6], 1))
    # the cut-off: the nsample-th hit at support index 63 (last lane of round 0) / 64 (first lane of round 1) / mid-round, with further
    # hits behind it in the same round of 64; an on-the-ball point before the cut-off, which a `<=` would take
    first7 = [3, 10, 20, 30, 40, 50, 60]
    cases.append(_ball_build('ball cut-off at 63', 129, ns, [[first7 + [63, 64, 65, 100]], [first7[:6] + [62, 63, 64]]], [[[5]], [[61]]], 2))
    cases.append(_ball_build('ball cut-off at 64', 129, ns, [[first7 + [64, 65, 70, 127]], [first7 + [64, 128]]], [[[63]], [[1]]], 3))
    cases.append(_ball_build('ball cut-off mid-round', 65, ns, [[[0, 1, 2, 3, 4, 5, 6, 20, 21, 40, 64]], [[8, 9, 10, 11, 12, 13, 14, 15, 16]]],
                             [[[7]], [[0]]], 4))
    return cases


# =======================================================================================================================================
# furthest point sampling: the reference's literal reduction tree
# =======================================================================================================================================
def fps_block_size(n):
    return max(min(1 << int(math.log(float(n)) / math.log(2.0)), 1024), 1)


def furthest_point_sampling(dataset, m, ties_to_higher=False, key_by_k=False):
    """dataset (b, 3, n) -> (b, m) int32.  Thread t of bs scans k = t, t + bs, ... and keeps its first strict maximum from (-1, 0); slot
    t + s is folded into slot t at strides s = bs / 2 .. 1, its index taken only when its value is strictly larger.
    ties_to_higher / key_by_k: deliberately wrong variants (the fold takes the upper slot on ties; the lowest k of the maximum wins)."""
    x = np.asarray(dataset, np.float64)
    b, _, n = x.shape
    bs = fps_block_size(n)
    rows = -(-n // bs)
    out = np.zeros((b, m), np.int32)
    kk = np.arange(rows * bs).reshape(rows, bs)                  # kk[r, t] = t + r bs
    for bi in range(b):
        p = x[bi]
        selectable = (p * p).sum(0) > float(F32(1e-3))
        temp = np.full(n, float(F32(1e10)))
        old = 0
        for j in range(1, m):
            d = ((p - p[:, old:old + 1]) ** 2).sum(0)
            temp = np.where(selectable, np.minimum(d, temp), temp)
            v = np.full(rows * bs, -np.inf)
            v[:n] = np.where(selectable, temp, -np.inf)
            v = v.reshape(rows, bs)
            if key_by_k:
                flat = v.reshape(-1)
                old = int(np.argmax(flat)) if flat.max() >= 0 else 0
                out[bi, j] = old
                continue
            first = v.argmax(0)                                   # the first of the maxima of every thread
            dist = v[first, np.arange(bs)]
            besti = np.where(dist >= 0, kk[first, np.arange(bs)], 0)
            dist = np.where(dist >= 0, dist, -1.0)
            s = bs // 2
            while s >= 1:
                v1, v2 = dist[:s], dist[s:2 * s]
                take = (v2 >= v1) if ties_to_higher else (v2 > v1)
                besti[:s] = np.where(take, besti[s:2 * s], besti[:s])
                dist[:s] = np.maximum(v1, v2)
                s //= 2
            old = int(besti[0])
            out[bi, j] = old
    return out


FPS_N = (2, 3, 63, 64, 65, 127, 128, 1023, 1024, 1025, 1331, 2049)


def fps_samples(n):
    return sorted({max(v, 1) for v in (1, 2, n - 1, n + 5)})


@cached
def fps_cloud(n):
    """Three clouds of different content on the integer lattice: A with point 0 and a few others at the origin (n = 1331: the 11^3 lattice
    with its centre moved to index 0), B a denser lattice with point 0 elsewhere, C with every point at the origin."""
    g = np.random.default_rng(40 + n)
    if n == 1331:
        ax = np.arange(-5, 6)
        a = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), 0).reshape(3, -1)
        centre = int(np.nonzero((a == 0).all(0))[0][0])
        a[:, [0, centre]] = a[:, [centre, 0]]
    else:
        a = g.integers(-4, 5, (3, n))
    a[:, 0] = 0
    if not a[:, 1].any():
        a[:, 1] = (1, 2, -1)
    if n > 3:
        a[:, g.integers(2, n, max(n // 16, 1))] = 0
    bcl = g.integers(-2, 3, (3, n))
    bcl[:, 0] = (1, -2, 2)
    return frozen(np.stack([a, bcl, np.zeros((3, n), np.int64)]).astype(F32))


@cached
def fps_case(n, m):
    pc = fps_cloud(n)
    return dict(name='fps n=%d m=%d' % (n, m), n=n, m=m, pc=pc, want=frozen(furthest_point_sampling(pc, m)))


# =======================================================================================================================================
# inter / intra zpconv
# =======================================================================================================================================
def _t64(a):
    return torch.from_numpy(np.array(a, np.float64))


def inter_fwd_t(idx, w, feats):
    """torch: out[b, c, k, p, a] = sum_n w[b, p, a, k, n] feats[b, c, idx[b, p, a, k, n], a]."""
    b, p, na, ks, ann = idx.shape
    bi, ai = torch.arange(b).view(b, 1, 1, 1, 1), torch.arange(na).view(1, 1, na, 1, 1)
    g = feats.permute(0, 2, 3, 1)[bi, idx.long(), ai]                        # (b, p, a, k, n, c)
    return torch.einsum('bpaknc,bpakn->bckpa', g, w)


def intra_fwd_t(nbr, w, feats):
    """torch: out[b, c, k, p, a] = sum_n w[a, k, n] feats[b, c, p, nbr[a, n]]."""
    return torch.einsum('bcpan,akn->bckpa', feats[:, :, :, nbr.long()], w)


def _zp_reference(fwd, idx, w, feats, cot):
    """-> forward, backward (float64) and their allowances (L + 2) 2^-24 Sigma |w f| per element, L = the number of terms."""
    it = torch.from_numpy(np.array(idx))
    f = _t64(feats).requires_grad_(True)
    out = fwd(it, _t64(w), f)
    (out * _t64(cot)).sum().backward()
    fa = _t64(np.abs(feats)).requires_grad_(True)
    mag_out = fwd(it, _t64(np.abs(w)), fa)
    (mag_out * _t64(np.abs(cot))).sum().backward()
    ones = torch.ones_like(f).requires_grad_(True)
    fwd(it, torch.ones_like(_t64(w)), ones).sum().backward()
    ann = idx.shape[-1]
    return dict(out=frozen(out.detach().numpy()), grad=frozen(f.grad.numpy()),
                out_allowed=frozen((ann + 2) * U * mag_out.detach().numpy()),
                grad_allowed=frozen((ones.grad.numpy() + 2) * U * fa.grad.numpy()), grad_terms=frozen(ones.grad.numpy()))


def inter_f32(idx, w, feats, cot, drop_last=False, shift=0):
    """float32 restatement in the kernels' order: forward n ascending, backward entries (p, k, n) ascending per target.
    drop_last / shift: deliberately wrong variants (the last neighbour left out; every index one target further)."""
    b, p, na, ks, ann = idx.shape
    c, nq = feats.shape[1], feats.shape[2]
    ix = (idx.astype(np.int64) + shift) % nq
    bi, ai = np.arange(b).reshape(b, 1, 1, 1), np.arange(na).reshape(1, 1, na, 1)
    fq = np.ascontiguousarray(feats.transpose(0, 2, 3, 1))                   # (b, q, a, c)
    out = np.zeros((b, p, na, ks, c), F32)
    for n in range(ann - int(drop_last)):
        out = out + w[..., n, None] * fq[bi, ix[..., n], ai]
    out = np.ascontiguousarray(out.transpose(0, 4, 3, 1, 2))                 # (b, c, k, p, a)
    grad = np.zeros((b, nq, na, c), F32)
    cp = np.ascontiguousarray(cot.transpose(0, 3, 4, 2, 1))                  # (b, p, a, k, c)
    b1, a1 = np.arange(b).reshape(b, 1), np.arange(na).reshape(1, na)
    for pi in range(p):
        for k in range(ks):
            for n in range(ann - int(drop_last)):
                q = ix[:, pi, :, k, n]                                        # (b, a): distinct targets
                grad[b1, q, a1] = grad[b1, q, a1] + w[:, pi, :, k, n, None] * cp[:, pi, :, k]
    return out, np.ascontiguousarray(grad.transpose(0, 3, 1, 2))


def intra_f32(nbr, w, feats, cot, drop_last=False, shift=0):
    """float32 restatement: forward n ascending, backward (a, k, n) ascending per input anchor."""
    na_out, ann = nbr.shape
    b, c, p, na_in = feats.shape
    ks = w.shape[1]
    nb = (nbr.astype(np.int64) + shift) % na_in
    out = np.zeros((b, c, ks, p, na_out), F32)
    for n in range(ann - int(drop_last)):
        out = out + w[:, :, n].T[None, None, :, None, :] * feats[:, :, None, :, nb[:, n]]
    grad = np.zeros((b, c, p, na_in), F32)
    for a in range(na_out):
        for k in range(ks):
            for n in range(ann - int(drop_last)):
                grad[..., nb[a, n]] = grad[..., nb[a, n]] + w[a, k, n] * cot[:, :, k, :, a]
    return out, grad


def _signed_weights(g, shape):
    w = g.standard_normal(shape).astype(F32)
    w[g.random(shape) < 0.2] = 0.0                                            # exact zeros, both signs elsewhere
    return w


def _row_scaled(g, shape, axis):
    """randn times 1e-3 .. 1e3 along `axis`: a misplaced row index cannot hide."""
    n = shape[axis]
    scale = 10.0 ** np.linspace(-3, 3, n) if n > 1 else np.ones(1)
    return (g.standard_normal(shape) * scale.reshape([-1 if i == axis else 1 for i in range(len(shape))])).astype(F32)


# name -> (np, nq, na, ks, ann, c, pattern); b = 2
INTER_SHAPES = {
    'inter 255 outputs, 65 targets': (17, 13, 5, 3, 3, 3, 'random'),
    'inter 256 outputs, 64 targets': (16, 16, 4, 4, 5, 2, 'random'),
    'inter 257 outputs, 63 targets, ann=ks=na=c=1': (257, 63, 1, 1, 1, 1, 'random'),
    'inter nq=1': (9, 1, 3, 2, 4, 3, 'random'),
    'inter one support point holds all, 63 targets': (11, 21, 3, 2, 3, 2, 'one'),
    'inter one target holds all, na=1, 64 targets': (40, 64, 1, 2, 3, 2, 'one'),
}


@cached
def inter_case(name):
    p, nq, na, ks, ann, c, pattern = INTER_SHAPES[name]
    g = np.random.default_rng(sorted(INTER_SHAPES).index(name) + 500)
    b = 2
    if pattern == 'one':
        idx = np.empty((b, p, na, ks, ann), np.int64)
        idx[0], idx[1] = nq - 1, nq // 3
    else:
        idx = g.integers(0, nq, (b, p, na, ks, ann))
    idx = idx.astype(np.int32)
    w, feats = _signed_weights(g, (b, p, na, ks, ann)), _row_scaled(g, (b, c, nq, na), 2)
    cot = _row_scaled(g, (b, c, ks, p, na), 3)
    d = dict(name=name, idx=frozen(idx), w=frozen(w), feats=frozen(feats), cot=frozen(cot), pattern=pattern,
             outputs=p * na * ks, targets=nq * na)
    d.update(_zp_reference(inter_fwd_t, idx, w, feats, cot))
    return d


# name -> (np, na_in, na_out, ks, ann, c); b = 2.  Input anchor 0 is referenced by every output anchor, the last one by none (na_in > 1).
INTRA_SHAPES = {
    'intra 5 -> 7 anchors, 255 gradients': (17, 5, 7, 2, 3, 3),
    'intra 7 -> 5 anchors, 255 outputs': (17, 7, 5, 1, 3, 3),
    'intra 256 outputs, 256 gradients': (16, 8, 4, 2, 3, 2),
    'intra 257 outputs, 257 gradients, ann=1': (257, 1, 1, 1, 1, 1),
    'intra ann=1': (6, 5, 7, 3, 1, 2),
}


@cached
def intra_case(name):
    p, na_in, na_out, ks, ann, c = INTRA_SHAPES[name]
    g = np.random.default_rng(sorted(INTRA_SHAPES).index(name) + 700)
    b = 2
    nbr = g.integers(0, max(na_in - 1, 1), (na_out, ann))                    # never the last input anchor
    if ann > 1:
        nbr[:, 0] = 0                                                         # every output anchor reads input anchor 0
    nbr = nbr.astype(np.int32)
    w, feats = _signed_weights(g, (na_out, ks, ann)), _row_scaled(g, (b, c, p, na_in), 3)
    if na_in == 1:
        feats = _row_scaled(g, (b, c, p, na_in), 2)
    cot = _row_scaled(g, (b, c, ks, p, na_out), 3)
    d = dict(name=name, nbr=frozen(nbr), w=frozen(w), feats=frozen(feats), cot=frozen(cot), outputs=c * ks * p * na_out,
             gradients=c * p * na_in, unreferenced=[q for q in range(na_in) if not (nbr == q).any()],
             by_all=[q for q in range(na_in) if (nbr == q).any(1).all()])
    d.update(_zp_reference(intra_fwd_t, nbr, w, feats, cot))
    return d


# =======================================================================================================================================
# anchor queries
# =======================================================================================================================================
EPS32 = float(F32(1e-6))


def shared_allowance(r):
    """The rule of tests/test_gpu_dense_edges.py, relative to the largest |want|: r is the float32 restatement's error."""
    return min(1e-4, 8 * max(r, 1.2e-7))


def rel_to_largest(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-300)) if want.size else 0.0


def anchor_query_from_ratio(ratio, norm, kernel_points):
    """ratio (b, p, na, nn) = x . a / r, norm (b, p, nn) = r -> (b, p, na, ks, nn)."""
    theta = np.arccos(np.clip(ratio, -1.0, 1.0))
    kw, kh = kernel_points[:, 0].astype(np.float64), kernel_points[:, 1].astype(np.float64)
    dr = kw[None, None, None, :, None] - norm[:, :, None, None, :]
    da = (kh[None, None, None, :, None] - theta[:, :, :, None, :]) * norm[:, :, None, None, :]
    return dr * dr + da * da


def anchor_ratio(grouped_xyz, anchors):
    g, a = np.asarray(grouped_xyz, np.float64), np.asarray(anchors, np.float64)
    norm = np.sqrt((g * g).sum(1)) + EPS32                                    # (b, p, nn)
    return np.einsum('bdpn,ad->bpan', g, a) / norm[:, :, None, :], norm


def anchor_query(grouped_xyz, anchors, kernel_points):
    """float64 on the float32 inputs: w = (kw - r)^2 + ((kh - theta) r)^2, r = |x| + 1e-6, theta = acos(x . a / r)."""
    ratio, norm = anchor_ratio(grouped_xyz, anchors)
    return anchor_query_from_ratio(ratio, norm, kernel_points)


def anchor_query_f32(grouped_xyz, anchors, kernel_points):
    """float32 restatement -> (weights, ratio); NaN where the float32 ratio leaves [-1, 1], as the reference."""
    g, a, kp = grouped_xyz.astype(F32), anchors.astype(F32), kernel_points.astype(F32)
    x, y, z = g[:, 0], g[:, 1], g[:, 2]
    norm = np.sqrt(x * x + y * y + z * z) + F32(1e-6)
    ratio = (x[:, :, None] * a[:, 0, None] + y[:, :, None] * a[:, 1, None] + z[:, :, None] * a[:, 2, None]) / norm[:, :, None]
    with np.errstate(invalid='ignore'):
        theta = np.arccos(ratio)
    dr = kp[:, 0][None, None, None, :, None] - norm[:, :, None, None, :]
    da = (kp[:, 1][None, None, None, :, None] - theta[:, :, :, None, :]) * norm[:, :, None, None, :]
    return (dr * dr + da * da).astype(F32), ratio


def anchor_query_spread(grouped_xyz, anchors, kernel_points):
    """Where acos is ill-conditioned: the range of the twin over ratio (1 -+ 2^-22) clipped to [-1, 1] (2^-22 covers the roundings of a
    float32 dot product, norm and quotient), widened by the float32 roundings of the remaining arithmetic, 16 2^-24 of the scale of its
    terms.  -> (lo, hi)."""
    ratio, norm = anchor_ratio(grouped_xyz, anchors)
    e = 2.0 ** -22
    t1, t2 = np.arccos(np.clip(ratio * (1 - e), -1, 1)), np.arccos(np.clip(ratio * (1 + e), -1, 1))
    tlo, thi = np.minimum(t1, t2)[:, :, :, None, :], np.maximum(t1, t2)[:, :, :, None, :]
    kw, kh = kernel_points[:, 0].astype(np.float64), kernel_points[:, 1].astype(np.float64)
    khb, nb = kh[None, None, None, :, None], norm[:, :, None, None, :]
    dr2 = (kw[None, None, None, :, None] - nb) ** 2
    ends = np.stack([((khb - tlo) * nb) ** 2, ((khb - thi) * nb) ** 2])
    inside = (khb >= tlo) & (khb <= thi)                                       # the angular term vanishes inside the interval
    slack = 16 * U * (nb * nb * (1 + (np.abs(khb) + np.pi) ** 2) + kw[None, None, None, :, None] ** 2)
    return dr2 + np.where(inside, 0.0, ends.min(0)) - slack, dr2 + ends.max(0) + slack


# name -> (np, nn, na, ks); b = 2
ANCHOR_SHAPES = {'anchor 255 entries': (17, 15, 12, 5), 'anchor 256 entries, na=1': (16, 16, 1, 3), 'anchor 257 entries, nn=1, ks=1': (257, 1, 7, 1),
                 'anchor np=1': (1, 9, 12, 2)}


@cached
def anchor_case(name):
    """Ordinary: |x . a| / |x| <= 0.99 for every anchor; some x = 0."""
    p, nn, na, ks = ANCHOR_SHAPES[name]
    g = np.random.default_rng(sorted(ANCHOR_SHAPES).index(name) + 900)
    anchors = g.standard_normal((na, 3))
    anchors = (anchors / np.linalg.norm(anchors, axis=1, keepdims=True)).astype(F32)
    x = np.zeros((2, 3, p, nn), F32)
    for bi in range(2):
        for pi in range(p):
            for ni in range(nn):
                while True:
                    v = (g.standard_normal(3) * 10.0 ** g.uniform(-2, 1)).astype(F32)
                    if np.abs(anchors.astype(np.float64) @ v.astype(np.float64)).max() / np.linalg.norm(v.astype(np.float64)) <= 0.985:
                        break
                x[bi, :, pi, ni] = v
    zero = g.random((2, p, nn)) < 0.1
    zero[1, -1, -1] = True
    x[np.broadcast_to(zero[:, None], x.shape)] = 0.0
    kp = np.stack([g.uniform(0.1, 0.6, ks), g.uniform(0.0, 1.2, ks)], 1).astype(F32)
    want = anchor_query(x, anchors, kp)
    r = rel_to_largest(anchor_query_f32(x, anchors, kp)[0], want)
    return dict(name=name, xyz=frozen(x), anchors=frozen(anchors), kp=frozen(kp), want=frozen(want), zero=frozen(zero), restatement=r,
                allowed=shared_allowance(r))


PARALLEL_NORMS = (1e-3, 1.0, 100.0)
PARALLEL_NAN_ROWS = (2,)              # rows (index into PARALLEL_NORMS) whose float32 |ratio| reaches 1 - 2^-22: a NaN is accepted there only


@cached
def anchor_parallel_case():
    """x exactly parallel (b = 0) and antiparallel (b = 1) to anchor n of the six axis anchors, |x| = PARALLEL_NORMS[p]."""
    anchors = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], F32)
    x = np.zeros((2, 3, len(PARALLEL_NORMS), 6), F32)
    for pi, s in enumerate(PARALLEL_NORMS):
        x[0, :, pi], x[1, :, pi] = (anchors * F32(s)).T, (-anchors * F32(s)).T
    kp = np.array([[0.2, 0.0], [0.5, 0.7], [1.0, 3.1415927], [100.0, 1.5]], F32)
    lo, hi = anchor_query_spread(x, anchors, kp)
    _, ratio32 = anchor_query_f32(x, anchors, kp)
    return dict(name='anchor parallel / antiparallel', xyz=frozen(x), anchors=frozen(anchors), kp=frozen(kp), lo=frozen(lo), hi=frozen(hi),
                want=frozen(anchor_query(x, anchors, kp)), ratio32=frozen(ratio32),
                nan_allowed=frozen(np.broadcast_to((np.abs(ratio32) >= F32(1 - 2.0 ** -22))[:, :, :, None, :], lo.shape)))


def initial_anchor_query(centers, xyz, kernel_points, radius, sigma, strict=False):
    """centers (b, 3, nc), xyz (m, 3), kernel_points (ks, na, 3) -> (weights float64, counts int64) (b, ks, nc, na): every point within
    `radius` of a centre (<=) counts, and adds 1 - |kp + centre - point|^2 / sigma where that is positive.  strict: the wrong `<`."""
    c, x, kp = np.asarray(centers, np.float64), np.asarray(xyz, np.float64), np.asarray(kernel_points, np.float64)
    b, _, nc = c.shape
    ks, na, _ = kp.shape
    w, n = np.zeros((b, ks, nc, na)), np.zeros((b, ks, nc, na), np.int64)
    if x.shape[0] == 0:
        return w, n
    r2 = float(radius) ** 2
    for bi in range(b):
        ct = c[bi].T                                                          # (nc, 3)
        d2 = ((ct[:, None, :] - x[None]) ** 2).sum(-1)                        # (nc, m)
        near = (d2 < r2) if strict else (d2 <= r2)
        e = kp[:, None, :, None, :] + ct[None, :, None, None, :] - x[None, None, None, :, :]          # (ks, nc, na, m, 3)
        wt = 1.0 - (e * e).sum(-1) / float(sigma)
        gate = near[None, :, None, :]
        w[bi] = np.where(gate & (wt > 0), wt, 0.0).sum(-1)
        n[bi] = np.broadcast_to(gate, wt.shape).sum(-1)
    return w, n


def initial_anchor_query_f32(centers, xyz, kernel_points, radius, sigma):
    """float32 restatement in the kernel's order: points ascending, distance as a rounded square root, squared again."""
    c, x, kp = centers.astype(F32), xyz.astype(F32), kernel_points.astype(F32)
    b, _, nc = c.shape
    ks, na, _ = kp.shape
    w, n = np.zeros((b, ks, nc, na), F32), np.zeros((b, ks, nc, na), F32)
    for bi in range(b):
        ct = c[bi].T
        k = kp[:, None, :, :] + ct[None, :, None, :]                           # (ks, nc, na, 3)
        for pm in range(x.shape[0]):
            d = ct - x[pm]
            near = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) <= F32(radius)
            e = k - x[pm]
            dk = np.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2])
            wt = F32(1) - dk * dk / F32(sigma)
            gate = near[None, :, None]
            w[bi] = w[bi] + np.where(gate & (wt > 0), wt, F32(0))
            n[bi] = n[bi] + np.where(gate, F32(1), F32(0))
    return w, n


INITIAL_RADIUS, INITIAL_SIGMA = 1.25, 1.5625
# offsets of a point from its centre with an exact length: inside (<= 1), exactly on the radius (3-4-5 / 4), outside (>= 1.5)
_INSIDE = np.array([[0.25, 0, 0], [0, -0.5, 0], [0.25, 0.5, 0.5], [-0.5, 0.25, -0.5], [0, 0, 1.0], [-0.75, 0, 0], [0, 0, 0]])
_ON = np.array([[0.75, 1.0, 0], [0, -0.75, 1.0], [-1.0, 0, 0.75], [1.25, 0, 0], [0, 0, -1.25]])
_OUTSIDE = np.array([[0.5, 1.0, 1.0], [1.5, 0, 0], [0.5, 0.75, -1.5], [0, 2.25, 0]])
# name -> (ks, nc, na); b = 2
INITIAL_SHAPES = {'initial 255 outputs': (3, 17, 5), 'initial 256 outputs': (4, 16, 4), 'initial 257 outputs, ks=na=1': (1, 257, 1)}


@cached
def initial_case(name):
    """Centres on a lattice of spacing 8; batch element 1 holds them in reversed order and moves every third one away from all points."""
    ks, nc, na = INITIAL_SHAPES[name]
    g = np.random.default_rng(sorted(INITIAL_SHAPES).index(name) + 1100)
    i = np.arange(nc)
    c0 = 8.0 * np.stack([i % 8, (i // 8) % 8, i // 64]) - 24.0
    c1 = c0[:, ::-1].copy()
    c1[:, ::3] += 4.0
    centers = np.stack([c0, c1]).astype(F32)
    pts = []
    for ci in range(0, nc, max(nc // 12, 1)):
        for off in (_INSIDE[g.integers(0, len(_INSIDE), 2)], _ON[g.integers(0, len(_ON), 1)], _OUTSIDE[g.integers(0, len(_OUTSIDE), 1)]):
            pts += [c0[:, ci] + o for o in off]
    pts.append(c0[:, 0] + _ON[0])
    xyz = np.array(pts)[g.permutation(len(pts))].astype(F32)
    kp = (0.25 * g.integers(-3, 4, (ks, na, 3))).astype(F32)
    # a kernel point at exactly d^2 == sigma from a counted point (the one at _ON[0] from centre 0): weight 0, not added, the count is
    kp[0, 0] = _ON[0] - np.array([0, 1.25, 0])
    want_w, want_n = initial_anchor_query(centers, xyz, kp, INITIAL_RADIUS, INITIAL_SIGMA)
    r = rel_to_largest(initial_anchor_query_f32(centers, xyz, kp, INITIAL_RADIUS, INITIAL_SIGMA)[0], want_w)
    return dict(name=name, centers=frozen(centers), xyz=frozen(xyz), kp=frozen(kp), radius=INITIAL_RADIUS, sigma=INITIAL_SIGMA,
                want_w=frozen(want_w), want_n=frozen(want_n), restatement=r, allowed=shared_allowance(r), zero_weight_at=(0, 0, 0))
