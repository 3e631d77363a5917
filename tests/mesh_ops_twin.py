"""A float64 twin of the mesh post-processing contract (the header comment of se3et_amd/csrc/mesh_ops.hip), written from the contract with
dictionaries and sets; it shares no text with the C core.  One mesh at a time: vertices (n, 3) float64, triangles (m, 3) int64.

Integers (tables, labels, counts, maps, triangle lists) are the contract's; floats follow its operation order, so the library's host
entries must give the same bits.  Row sums are taken column by column over rows padded with +0.0: a running sum that starts at +0.0 is
never -0.0, so adding +0.0 changes no bit and the padded sum equals the sequential one."""
import numpy as np

BAD_TRIANGLE = 1
LANES = 64


def valid(tri, n):
    """per triangle: all three numbers inside [0, n)"""
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    return np.all((t >= 0) & (t < n), axis=1)


def incidence(tri, n):
    """(tri_rows, nbr_rows, status): per vertex the ascending list of its triangles and of its distinct other vertices"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    ok = valid(tri, n)
    of_vertex = {v: set() for v in range(n)}
    near = {v: set() for v in range(n)}
    for t, (row, good) in enumerate(zip(tri.tolist(), ok)):
        if not good:
            continue
        for v in set(row):
            of_vertex[v].add(t)
            near[v] |= set(row) - {v}
    return [sorted(of_vertex[v]) for v in range(n)], [sorted(near[v]) for v in range(n)], 0 if ok.all() else BAD_TRIANGLE


def csr(rows):
    """lists -> (offsets (n + 1) int64, entries int32)"""
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return off, np.array([x for r in rows for x in r], np.int32)


# ---- areas and normals ----------------------------------------------------------------------------------------------------------------------------
def cross(vertices, tri, n):
    """cross(v1 - v0, v2 - v0) per triangle, zero for a triangle out of range"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    ok = valid(tri, n)
    safe = np.where(ok[:, None], tri, 0)
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    if len(v) == 0:
        return np.zeros((len(tri), 3))
    a, b = v[safe[:, 1]] - v[safe[:, 0]], v[safe[:, 2]] - v[safe[:, 0]]
    out = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    out[~ok] = 0.0
    return out


def norm(x):
    return np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])


def normalize(x):
    r = norm(x)
    good = (r > 0) & np.isfinite(r)
    out = np.zeros_like(x)
    out[:, 2] = 1.0
    with np.errstate(all='ignore'):
        out[good] = x[good] / r[good, None]
    return out


def triangle_areas(vertices, tri, n):
    return 0.5 * norm(cross(vertices, tri, n))


def triangle_normals(vertices, tri, n, normalized=True):
    c = cross(vertices, tri, n)
    return normalize(c) if normalized else c


def _row_sums(values, rows):
    """per row the sum of values[row] in row order, from +0.0"""
    width = max([len(r) for r in rows] + [0])
    s = np.zeros((len(rows), values.shape[1]))
    for k in range(width):
        idx = np.array([r[k] if k < len(r) else -1 for r in rows], np.int64)
        s = s + np.where(idx[:, None] >= 0, values[np.maximum(idx, 0)], 0.0)
    return s


def vertex_normals(vertices, tri, n):
    tri_rows, _, _ = incidence(tri, n)
    c = cross(vertices, tri, n)
    if len(c) == 0:
        c = np.zeros((1, 3))
    return normalize(_row_sums(c, tri_rows))


# ---- components -------------------------------------------------------------------------------------------------------------------------------------
def tree_sum(a):
    """lane l of 64 adds a[l], a[l + 64], .. in order from 0.0; then lane[l] += lane[l ^ o] for o = 32 .. 1; lane 0"""
    lane = np.zeros(LANES)
    for i, x in enumerate(a):
        lane[i % LANES] = lane[i % LANES] + x
    o = LANES // 2
    while o:
        lane = lane + lane[np.arange(LANES) ^ o]
        o //= 2
    return float(lane[0])


def components(vertices, tri, n):
    """(labels (m,), n_triangles (k,), area (k,), status): breadth-first search from triangle 0 upward over shared undirected edges"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    ok = valid(tri, n)
    on_edge = {}
    for t, (row, good) in enumerate(zip(tri.tolist(), ok)):
        if not good:
            continue
        for a, b in ((row[0], row[1]), (row[1], row[2]), (row[2], row[0])):
            if a != b:
                on_edge.setdefault(frozenset((a, b)), set()).add(t)
    labels = np.full(len(tri), -1, np.int64)
    k = 0
    for start in range(len(tri)):
        if labels[start] >= 0:
            continue
        labels[start] = k
        queue = [start]
        while queue:
            t = queue.pop()
            if not ok[t]:
                continue
            row = tri[t].tolist()
            for a, b in ((row[0], row[1]), (row[1], row[2]), (row[2], row[0])):
                for u in on_edge.get(frozenset((a, b)), ()) if a != b else ():
                    if labels[u] < 0:
                        labels[u] = k
                        queue.append(u)
        k += 1
    areas = triangle_areas(vertices, tri, n)
    count = np.array([int(np.sum(labels == c)) for c in range(k)], np.int64)
    area = np.array([tree_sum(areas[labels == c]) for c in range(k)], np.float64)
    return labels, count, area, 0 if ok.all() else BAD_TRIANGLE


# ---- selection ----------------------------------------------------------------------------------------------------------------------------------------
def select(vertices, tri, keep, attributes=()):
    """(vertices, triangles, attributes, vertex_map, status)"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    n = len(vertices)
    ok = valid(tri, n)
    kept = [t for t in range(len(tri)) if ok[t] and keep[t]]
    used = sorted({v for t in kept for v in tri[t].tolist()})
    new = {v: i for i, v in enumerate(used)}
    vmap = np.array([new.get(v, -1) for v in range(n)], np.int64)
    out_tri = np.array([[new[v] for v in tri[t].tolist()] for t in kept], np.int64).reshape(-1, 3)
    pick = np.array(used, np.int64)
    return (np.asarray(vertices)[pick].reshape(-1, 3), out_tri, [None if a is None else np.asarray(a)[pick].reshape(-1, 3) for a in attributes], vmap,
            0 if ok.all() else BAD_TRIANGLE)


# ---- smoothing ----------------------------------------------------------------------------------------------------------------------------------------
def smooth_step(values, nbr_rows, simple, lam):
    values = np.asarray(values, np.float64)
    if len(values) == 0:
        return values.copy()
    s = _row_sums(values, nbr_rows)
    count = np.array([len(r) for r in nbr_rows], np.float64)[:, None]
    with np.errstate(all='ignore'):
        new = (values + s) / (count + 1.0) if simple else values + lam * (s / count - values)
    return np.where(count > 0, new, values)


def smooth(values, nbr_rows, method, iterations, lam=0.5, mu=-0.53):
    x = np.array(values, np.float64, copy=True)
    for _ in range(iterations):
        if method == 'simple':
            x = smooth_step(x, nbr_rows, True, 0.0)
        elif method == 'laplacian':
            x = smooth_step(x, nbr_rows, False, lam)
        elif method == 'taubin':
            x = smooth_step(smooth_step(x, nbr_rows, False, lam), nbr_rows, False, mu)
        else:
            raise ValueError(method)
    return x


# ---- vertex clustering --------------------------------------------------------------------------------------------------------------------------------
NONFINITE, TOO_MANY_CELLS = 2, 4
AXIS_CAP = 2.0 ** 21


def cluster_vertices(vertices, tri, voxel_size, attributes=()):
    """(vertices, triangles, attributes, vertex_map, status): cells of floor((v - (min - voxel_size / 2)) / voxel_size) in ascending (x, y, z)
    order, means summed in ascending vertex order; triangles remapped, collapsed ones dropped, rotated lowest first, first of equals kept"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    n = len(v)
    empty = (np.zeros((0, 3)), np.zeros((0, 3), np.int64), [None if a is None else np.zeros((0, 3)) for a in attributes], np.full(n, -1, np.int64))
    if not all(np.isfinite(x).all() for x in (v,) + tuple(a for a in attributes if a is not None)):
        return empty + (NONFINITE,)
    members = {}
    if n:
        org = v.min(0) - voxel_size / 2
        if ((v.max(0) - org) / voxel_size >= AXIS_CAP).any():
            return empty + (TOO_MANY_CELLS,)
        for i, cell in enumerate(map(tuple, np.floor((v - org) / voxel_size).astype(np.int64).tolist())):
            members.setdefault(cell, []).append(i)
    new = {i: k for k, cell in enumerate(sorted(members)) for i in members[cell]}

    def mean(x):
        if x is None:
            return None
        out = np.zeros((len(members), 3))
        for k, cell in enumerate(sorted(members)):
            s = np.zeros(3)
            for i in members[cell]:
                s = s + np.asarray(x, np.float64)[i]
            out[k] = s / float(len(members[cell]))
        return out
    ok = valid(tri, n)
    seen, out_tri = set(), []
    for t, row in enumerate(tri.tolist()):
        if not ok[t]:
            continue
        r = [new[a] for a in row]
        if len(set(r)) < 3:
            continue
        k = r.index(min(r))
        r = (r[k], r[(k + 1) % 3], r[(k + 2) % 3])
        if r not in seen:
            seen.add(r)
            out_tri.append(r)
    vmap = np.array([new[i] for i in range(n)], np.int64).reshape(-1)
    return mean(v), np.array(out_tri, np.int64).reshape(-1, 3), [mean(a) for a in attributes], vmap, 0 if ok.all() else BAD_TRIANGLE
