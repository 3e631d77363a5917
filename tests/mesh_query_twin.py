"""The float64 twin of the mesh queries, written from the contract in the header comment of se3et_amd/csrc/mesh_query.hip, not from the C:
which triangles are live, the BRUTE-FORCE ray cast and closest point over all triangles with the two tie rules, and a plain-Python walk
over a tree with switches for the mistakes a kernel could make.  numpy's element-wise arithmetic does not fuse, so operations written in
the contract's order give the contract's bits.

cast / closest are vectorised over (rays, triangles); walk_* are scalar and slow, for the small named cases only."""
import numpy as np

LIVE, BAD, NONFINITE, FLAT = 0, 1, 2, 3
INF = np.inf


def kinds(vertices, tri):
    """contract 1: the kind of every triangle"""
    n, out = len(vertices), np.zeros(len(tri), np.int64)
    with np.errstate(all='ignore'):
        for t, (a, b, c) in enumerate(tri.tolist()):
            if min(a, b, c) < 0 or max(a, b, c) >= n:
                out[t] = BAD
                continue
            p = vertices[[a, b, c]]
            if not np.isfinite(p).all():
                out[t] = NONFINITE
                continue
            e, f = p[1] - p[0], p[2] - p[0]
            x = np.array([e[1] * f[2] - e[2] * f[1], e[2] * f[0] - e[0] * f[2], e[0] * f[1] - e[1] * f[0]])
            out[t] = FLAT if (x == 0).all() else LIVE
    return out


def _corners(vertices, tri, live):
    idx = np.where(live[:, None], tri, 0)
    safe = vertices if len(vertices) else np.zeros((1, 3))
    return safe[idx[:, 0]], safe[idx[:, 1]], safe[idx[:, 2]]


def normals_of(vertices, tri, ids):
    """cross(b - a, c - a) over its length ((0, 0, 1) where the length is zero or not finite); zero rows for ids < 0"""
    out = np.zeros((len(ids), 3))
    with np.errstate(all='ignore'):
        for r, t in enumerate(ids.tolist()):
            if t < 0:
                continue
            a, b, c = vertices[tri[t]]
            e, f = b - a, c - a
            x = np.array([e[1] * f[2] - e[2] * f[1], e[2] * f[0] - e[0] * f[2], e[0] * f[1] - e[1] * f[0]])
            xx, yy, zz = x * x
            length = np.sqrt((xx + yy) + zz)
            out[r] = x / length if length > 0 and np.isfinite(length) else (0.0, 0.0, 1.0)
    return out


def ray_frame(rays):
    """contract 6: (valid, kx, ky, kz, Sx, Sy, Sz) per ray"""
    rays = np.asarray(rays, np.float64).reshape(-1, 6)
    d = rays[:, 3:]
    valid = np.isfinite(rays).all(1) & (d != 0).any(1)
    mag = np.abs(np.where(valid[:, None], d, 1.0))
    kz = np.zeros(len(rays), np.int64)
    kz[mag[:, 1] > mag[:, 0]] = 1
    kz[mag[:, 2] > np.maximum(mag[:, 0], mag[:, 1])] = 2
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    rows = np.arange(len(rays))
    dd = np.where(valid[:, None], d, 1.0)
    swap = dd[rows, kz] < 0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    with np.errstate(all='ignore'):
        return valid, kx, ky, kz, dd[rows, kx] / dd[rows, kz], dd[rows, ky] / dd[rows, kz], 1.0 / dd[rows, kz]


def _sheared(p, o, frame):
    """p (M, 3) against rays (R,): x, y, z (R, M)"""
    _, kx, ky, kz, sx, sy, sz = frame
    A = [p[:, k][None, :] - o[:, k][:, None] for k in range(3)]           # A[k]: (R, M)
    pick = lambda k: np.where(k[:, None] == 0, A[0], np.where(k[:, None] == 1, A[1], A[2]))
    x, y, z = pick(kx), pick(ky), pick(kz)
    return x - sx[:, None] * z, y - sy[:, None] * z, sz[:, None] * z


def cast(vertices, tri, rays, t_min=0.0, t_max=INF, test='watertight'):
    """(t_hit (R,), primitive_ids (R,), primitive_uvs (R, 2), primitive_normals (R, 3)): every ray against every live triangle, the winner
    the smallest computed t and among equal t the lowest triangle number.  test='naive': a Moeller-Trumbore test with u, v >= 0 and
    u + v <= 1, the modelled mistake that is NOT watertight."""
    rays = np.asarray(rays, np.float64).reshape(-1, 6)
    R, M = len(rays), len(tri)
    t_hit, ids, uvs = np.full(R, INF), np.full(R, -1, np.int64), np.zeros((R, 2))
    live = kinds(vertices, tri) == LIVE
    frame = ray_frame(rays)
    if R == 0 or not live.any():
        return t_hit, ids, uvs, np.zeros((R, 3))
    a, b, c = _corners(vertices, tri, live)
    with np.errstate(all='ignore'):
        if test == 'naive':
            o, d = rays[:, None, :3], rays[:, None, 3:]
            e1, e2 = (b - a)[None], (c - a)[None]
            h = np.cross(d, e2)
            det = (e1 * h).sum(-1)
            s = o - a[None]
            u = (s * h).sum(-1) / det
            q = np.cross(s, e1)
            v = (d * q).sum(-1) / det
            t = (e2 * q).sum(-1) / det
            hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
            uu, vv = u, v
        else:
            o = rays[:, :3]
            ax, ay, az = _sheared(a, o, frame)
            bx, by, bz = _sheared(b, o, frame)
            cx, cy, cz = _sheared(c, o, frame)
            U, V, W = cx * by - cy * bx, ax * cy - ay * cx, bx * ay - by * ax
            mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
            det = (U + V) + W
            t = ((U * az + V * bz) + W * cz) / det
            hit = ~mixed & (det != 0)
            uu, vv = V / det, W / det
        hit &= live[None, :] & frame[0][:, None] & (t >= t_min) & (t <= t_max)
    tt = np.where(hit, t, INF)
    best = tt.min(1)
    first = np.argmax(tt == best[:, None], 1)                              # the lowest triangle number among the equal t
    found = hit.any(1)
    rows = np.arange(R)
    t_hit[found], ids[found] = tt[rows, first][found], first[found]       # (the winner's own t: -0.0 and 0.0 are equal and differ in bits)
    uvs[found, 0], uvs[found, 1] = uu[rows, first][found], vv[rows, first][found]
    return t_hit, ids, uvs, normals_of(vertices, tri, ids)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def closest_on_triangles(p, a, b, c):
    """contract 7 for one point against triangles (M,): (points (M, 3), v (M,), w (M,)), every case computed and the first that applies
    selected, in the order of the region walk"""
    with np.errstate(all='ignore'):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        s_ab, s_ac, s_bc = d1 / (d1 - d3), d2 / (d2 - d6), e43 / (e43 + e56)
        inv = 1.0 / ((va + vb) + vc)
        sv, sw = vb * inv, vc * inv
        one, zero = np.ones_like(d1), np.zeros_like(d1)
        cases = [
            (((d1 <= 0) & (d2 <= 0)), a, zero, zero),
            (((d3 >= 0) & (d4 <= d3)), b, one, zero),
            (((vc <= 0) & (d1 >= 0) & (d3 <= 0)), a + s_ab[:, None] * ab, s_ab, zero),
            (((d6 >= 0) & (d5 <= d6)), c, zero, one),
            (((vb <= 0) & (d2 >= 0) & (d6 <= 0)), a + s_ac[:, None] * ac, zero, s_ac),
            (((va <= 0) & (e43 >= 0) & (e56 >= 0)), b + s_bc[:, None] * (c - b), 1.0 - s_bc, s_bc),
        ]
        point, v, w = (a + ab * sv[:, None]) + ac * sw[:, None], sv, sw
        for cond, pt, cv, cw in reversed(cases):
            point, v, w = np.where(cond[:, None], pt, point), np.where(cond, cv, v), np.where(cond, cw, w)
    return point, v, w


def _dist2(q, x):
    d = q - x
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def closest(vertices, tri, queries):
    """(points (Q, 3), distances (Q,), primitive_ids (Q,), primitive_uvs (Q, 2), primitive_normals (Q, 3)): brute force over the live
    triangles; the smallest computed squared distance, then the lowest triangle number.  NaN, NaN, -1, NaN, NaN for a query that is not
    finite; inf and -1 (NaN elsewhere) for a mesh without a live triangle."""
    queries = np.asarray(queries, np.float64).reshape(-1, 3)
    Q = len(queries)
    points, dist, ids, uvs = np.full((Q, 3), np.nan), np.full(Q, np.nan), np.full(Q, -1, np.int64), np.full((Q, 2), np.nan)
    live = kinds(vertices, tri) == LIVE
    valid = np.isfinite(queries).all(1)
    dist[valid] = INF
    if live.any():
        a, b, c = (x[live] for x in _corners(vertices, tri, live))
        numbers = np.nonzero(live)[0]
        for i in np.nonzero(valid)[0]:
            pt, v, w = closest_on_triangles(queries[i], a, b, c)
            d2 = _dist2(queries[i], pt)
            k = int(np.argmax(d2 == d2.min()))
            points[i], dist[i], ids[i], uvs[i] = pt[k], np.sqrt(d2[k]), numbers[k], (v[k], w[k])
    normals = normals_of(vertices, tri, ids)
    normals[ids < 0] = np.nan
    return points, dist, ids, uvs, normals


# ---- a walk over a tree, with the mistakes a kernel could make ------------------------------------------------------------------------------------
# nodes: a structured array with lo (3,), hi (3,), left, right, parent (tests/mesh_query_fixture.NODE); root: -1 for none.
MISTAKES = ('strict_tie', 'skip_on_equal', 'no_margin', 'short_trail')
DEPTH_SLACK, POINT_SLACK, SQUARE_SLACK = 2.0 ** -49, 2.0 ** -48, 2.0 ** -50


class _RayQuery:
    def __init__(self, vertices, tri, ray, t_min, t_max, mistake):
        self.v, self.tri, self.ray, self.t_min, self.t_max, self.mistake = vertices, tri, np.asarray(ray, np.float64), t_min, t_max, mistake
        self.frame = ray_frame(self.ray[None])
        self.valid = bool(self.frame[0][0])
        self.t, self.id = INF, -1

    def leaf(self, t):
        got, ids, _, _ = cast(self.v, self.tri[t:t + 1], self.ray[None], self.t_min, self.t_max)
        if ids[0] < 0:
            return
        s = got[0]
        if s < self.t or (s == self.t and t < self.id and self.mistake != 'strict_tie'):
            self.t, self.id = s, t

    def box(self, node):
        _, kx, ky, kz, sx, sy, sz = (x[0] for x in self.frame)
        o, lo, hi = self.ray[:3], node['lo'], node['hi']
        with np.errstate(all='ignore'):
            zl, zh = lo[kz] - o[kz], hi[kz] - o[kz]
            xa, xb, ya, yb = sx * zl, sx * zh, sy * zl, sy * zh
            xlo, xhi = (lo[kx] - o[kx]) - max(xa, xb), (hi[kx] - o[kx]) - min(xa, xb)
            ylo, yhi = (lo[ky] - o[ky]) - max(ya, yb), (hi[ky] - o[ky]) - min(ya, yb)
            if xlo > 0 or xhi < 0 or ylo > 0 or yhi < 0:
                return False
            za, zb = sz * zl, sz * zh
            near, far = min(za, zb), max(za, zb)
            slack = 0.0 if self.mistake == 'no_margin' else max(abs(near), abs(far)) * DEPTH_SLACK
            bound = min(self.t, self.t_max)
            if self.mistake == 'skip_on_equal':
                return not (near - slack >= bound or far + slack < self.t_min)
            return not (near - slack > bound or far + slack < self.t_min)


class _PointQuery:
    def __init__(self, vertices, tri, q, mistake):
        self.v, self.tri, self.q, self.mistake = vertices, tri, np.asarray(q, np.float64), mistake
        self.valid = bool(np.isfinite(self.q).all())
        self.d2, self.id = INF, -1

    def leaf(self, t):
        a, b, c = (self.v[self.tri[t, k]][None] for k in range(3))
        pt, _, _ = closest_on_triangles(self.q, a, b, c)
        s = _dist2(self.q, pt)[0]
        if s < self.d2 or (s == self.d2 and t < self.id and self.mistake != 'strict_tie'):
            self.d2, self.id = s, t

    def box(self, node):
        s = 0.0
        for k in range(3):
            lo, hi = node['lo'][k], node['hi'][k]
            e = max(lo - self.q[k], self.q[k] - hi)
            if self.mistake != 'no_margin':
                e = e - max(abs(lo), abs(hi)) * POINT_SLACK
            e = e if e > 0 else 0.0
            s = s + e * e
        if self.mistake != 'no_margin':
            s = s - s * SQUARE_SLACK
        return not (s >= self.d2) if self.mistake == 'skip_on_equal' else not (s > self.d2)


def _walk(nodes, root, Q, trail_bits):
    """contract 8: depth first, a leaf where it is met, one trail bit a level for a waiting child.  This walk always enters the left child
    first and lets the right one wait; the kernels enter the nearer one first, which cannot change an answer under the tie rules."""
    if root < 0 or not Q.valid:
        return
    top = nodes[root]
    if not Q.box(top):
        return
    if top['left'] < 0:
        Q.leaf(-1 - int(top['left']))
        return
    trail, level, cur = set(), 0, root
    while True:
        x, y = nodes[nodes[cur]['left']], nodes[nodes[cur]['right']]
        go_x, go_y = Q.box(x), Q.box(y)
        if go_x and x['left'] < 0:
            Q.leaf(-1 - int(x['left']))
            go_x, go_y = False, go_y and Q.box(y)
        if go_y and y['left'] < 0:
            Q.leaf(-1 - int(y['left']))
            go_y = False
        if go_x or go_y:
            if go_x and go_y and level < trail_bits:                      # (a trail that is too short forgets the waiting child)
                trail.add(level)
            cur, level = int(nodes[cur]['left'] if go_x else nodes[cur]['right']), level + 1
            continue
        while True:
            if level == 0:
                return
            cur, level = int(nodes[cur]['parent']), level - 1
            if level not in trail:
                continue
            trail.discard(level)
            nxt = int(nodes[cur]['right'])
            if nodes[nxt]['left'] < 0 or not Q.box(nodes[nxt]):
                continue
            cur, level = nxt, level + 1
            break


def walk_cast(nodes, root, vertices, tri, rays, t_min=0.0, t_max=INF, mistake=None):
    """(t_hit, primitive_ids) of the walk over the tree; mistake: None or one of MISTAKES"""
    rays = np.asarray(rays, np.float64).reshape(-1, 6)
    t_hit, ids = np.full(len(rays), INF), np.full(len(rays), -1, np.int64)
    for r, ray in enumerate(rays):
        Q = _RayQuery(vertices, tri, ray, t_min, t_max, mistake)
        _walk(nodes, root, Q, 64 if mistake == 'short_trail' else 128)
        t_hit[r], ids[r] = Q.t, Q.id
    return t_hit, ids


def walk_closest(nodes, root, vertices, tri, queries, mistake=None):
    """(squared distances, primitive_ids) of the walk over the tree"""
    queries = np.asarray(queries, np.float64).reshape(-1, 3)
    d2, ids = np.full(len(queries), INF), np.full(len(queries), -1, np.int64)
    for i, q in enumerate(queries):
        Q = _PointQuery(vertices, tri, q, mistake)
        _walk(nodes, root, Q, 64 if mistake == 'short_trail' else 128)
        d2[i], ids[i] = Q.d2, Q.id
    return d2, ids
