"""A numpy restatement of the triangle mesh contract (se3et_amd/tsdf.py, se3et_amd/tsdf_sparse.py, csrc/tsdf_mesh.hip): the triangle table
built from its rule, marching cubes as the plain loop over cubes with the vertices collected from the triangles that use them, and the
vertex values as the float64 formulas of tsdf_twin / tsdf_sparse_twin.  Nothing here is shared with the library, and the table is not read
from csrc/mesh_table.h nor built by tools/gen_mesh_table.py: the faces are walked as runs of negative corners here."""
import functools
import itertools

import numpy as np

import tsdf_sparse_twin as sparse

F32 = np.float32
CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)])
EDGES = [(0, 1), (1, 2), (3, 2), (0, 3), (4, 5), (5, 6), (7, 6), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7)]
AXIS = [int(np.flatnonzero(CORNERS[b] - CORNERS[a])[0]) for a, b in EDGES]
WIDTH = 16
_EDGE_OF = {frozenset(pair): e for e, pair in enumerate(EDGES)}
_MID = [(CORNERS[a] + CORNERS[b]) / 2.0 for a, b in EDGES]


def _face_cycles():
    """(outward normal, the face's corners in cyclic order) of the six faces"""
    corner_at = {tuple(c): i for i, c in enumerate(CORNERS)}
    out = []
    for axis, side in itertools.product(range(3), (0, 1)):
        b, c = [a for a in range(3) if a != axis]
        cycle = []
        for u, v in ((0, 0), (1, 0), (1, 1), (0, 1)):
            p = [0, 0, 0]
            p[axis], p[b], p[c] = side, u, v
            cycle.append(corner_at[tuple(p)])
        n = np.zeros(3)
        n[axis] = 2 * side - 1
        out.append((n, cycle))
    return out


FACES = _face_cycles()


def same_face(e, f):
    """do the cube edges e and f lie in one face of the cube?"""
    return any(set(EDGES[e]) <= set(cycle) and set(EDGES[f]) <= set(cycle) for _, cycle in FACES)


def segments(case):
    """The rule's directed segments (edge a, edge b) of a cube index: on each face, every maximal run of negative corners is cut off by one
    segment between the two edges that leave the run."""
    neg = [bool(case >> c & 1) for c in range(8)]
    out = []
    for n, cycle in FACES:
        signs = [neg[c] for c in cycle]
        if all(signs) or not any(signs):
            continue
        for i in range(4):
            if not (signs[i] and not signs[i - 1]):
                continue                                                # (a run starts at i)
            j = i
            while signs[(j + 1) % 4]:
                j += 1
            a = _EDGE_OF[frozenset((cycle[i - 1], cycle[i]))]
            b = _EDGE_OF[frozenset((cycle[j % 4], cycle[(j + 1) % 4]))]
            pc = CORNERS[cycle[i]].astype(np.float64)
            forward = float(np.dot(np.cross(_MID[b] - _MID[a], pc - _MID[a]), n)) > 0
            out.append((a, b) if forward else (b, a))
    return out


def loops(case):
    follow = dict(segments(case))
    assert sorted(follow) == sorted(follow.values()), 'every crossing edge has one outgoing and one incoming segment'
    out, seen = [], set()
    for start in sorted(follow):
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = follow[e]
        if loop:
            out.append(loop)
    return out


def triangles_of(case):
    out = []
    for loop in loops(case):
        for r in range(len(loop)):
            L = loop[r:] + loop[:r]
            if not any(same_face(L[0], L[k]) for k in range(2, len(L) - 1)):
                break
        else:
            raise AssertionError('case %d: no rotation of %r keeps the fan out of the faces' % (case, loop))
        out += [(L[0], L[k + 1], L[k]) for k in range(1, len(L) - 1)]
    return out


@functools.lru_cache(maxsize=None)
def table():
    """(256, 16) int8, rows -1 terminated"""
    rows = np.full((256, WIDTH), -1, np.int8)
    for case in range(256):
        flat = [e for tri in triangles_of(case) for e in tri]
        rows[case, :len(flat)] = flat
    rows.setflags(write=False)
    return rows


# ---- marching cubes ---------------------------------------------------------------------------------------------------------------------------
def marching(cubes, bits, rank):
    """cubes: the min corners of the cubes in output order; bits(p) -> (observed, negative) of voxel p; rank(p): the sort key of an owning
    voxel.  Returns (the vertices [(owner, axis)] in their order, triangles (m, 3) int64): the vertices are those that a triangle uses."""
    T = table()
    corners = [tuple(int(v) for v in c) for c in CORNERS]
    used, flat = set(), []
    for p in cubes:
        at = [(p[0] + c[0], p[1] + c[1], p[2] + c[2]) for c in corners]
        b = [bits(q) for q in at]
        if not all(o for o, _ in b):
            continue
        row = T[sum(1 << c for c in range(8) if b[c][1])]
        for e in row[row >= 0]:
            key = (at[EDGES[e][0]], AXIS[e])
            used.add(key)
            flat.append(key)
    order = sorted(used, key=lambda k: (rank(k[0]), k[1]))
    number = {k: i for i, k in enumerate(order)}
    return order, np.array([number[k] for k in flat], np.int64).reshape(-1, 3)


def sign_grid_mesh(negative):
    """the triangles of a grid of signs (n, n, n) bool, every voxel observed, every cube taken"""
    n = negative.shape[0]
    cubes = itertools.product(range(n - 1), repeat=3)
    return marching(cubes, lambda p: (True, bool(negative[p])), lambda p: p)


def _rows(rows):
    return np.array(rows, dtype=np.float64).reshape(-1, 3)


def _vertex(p0, axis, vl, f0, f1, c0, c1, trilinear, origin):
    """extraction items 3 and 4 for one edge: p0 the owner's indices, f0, f1 the tsdf at its ends, c0, c1 their colours or None"""
    r0, r1 = abs(float(f0)), abs(float(f1))
    p = [vl / 2.0 + vl * float(i) for i in p0]
    p1 = p[axis] + vl
    p[axis] = ((p[axis] * r1) + (p1 * r0)) / (r0 + r1)
    color = None if c0 is None else [((float(c0[k]) * r1) + (float(c1[k]) * r0)) / (r0 + r1) for k in range(3)]
    h = 0.99 * vl
    n = []
    for a in range(3):
        hi, lo = list(p), list(p)
        hi[a], lo[a] = p[a] + h, p[a] - h
        n.append(trilinear(hi) - trilinear(lo))
    length = float(np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
    return [p[a] + float(origin[a]) for a in range(3)], [v / length for v in n] if length > 0 else n, color


def mesh_dense(state, vl, origin):
    """(vertices, triangles, normals, colors or None) of a tsdf_twin state"""
    import tsdf_twin as uniform
    t, w, col = state['tsdf'], state['weight'], state['color']
    R, vl = t.shape[0], float(vl)
    order, tri = marching(itertools.product(range(1, R - 2), repeat=3), lambda p: (w[p] != 0, t[p] < 0), lambda p: p)
    out = ([], [], [])
    with np.errstate(all='ignore'):
        for p0, axis in order:
            p1 = tuple(p0[a] + (a == axis) for a in range(3))
            rows = _vertex(p0, axis, vl, t[p0], t[p1], None if col is None else col[(slice(None),) + p0], None if col is None else col[(slice(None),) + p1],
                           lambda q: uniform._trilinear(t, vl, q), origin)
            for dst, r in zip(out, rows):
                dst.append(r)
    return _rows(out[0]), tri, _rows(out[1]), _rows(out[2]) if col is not None else None


def mesh_sparse(blocks, vl, num_volumes, color):
    """per volume (vertices, triangles, normals, colors or None) of a {(volume, bx, by, bz): state}"""
    vl = float(vl)
    B, L = sparse.BLOCK, sparse.BLOCK * vl
    result = []
    for v in range(num_volumes):
        def voxel(p):
            s = blocks.get((v, p[0] // B, p[1] // B, p[2] // B))
            return s, (p[0] % B, p[1] % B, p[2] % B)

        def bits(p):
            s, i = voxel(p)
            return (False, False) if s is None else (s['weight'][i] != 0, s['tsdf'][i] < 0)
        coords = sorted((c for c in blocks if c[0] == v), key=sparse.key_of)
        cubes = ((B * c[1] + x, B * c[2] + y, B * c[3] + z) for c in coords for x, y, z in itertools.product(range(B), repeat=3))
        order, tri = marching(cubes, bits, lambda p: (p[0] // B, p[1] // B, p[2] // B, p[0] % B, p[1] % B, p[2] % B))
        out = ([], [], [])
        with np.errstate(all='ignore'):
            for p0, axis in order:
                p1 = tuple(p0[a] + (a == axis) for a in range(3))
                (s0, i0), (s1, i1) = voxel(p0), voxel(p1)
                coord = (v, p0[0] // B, p0[1] // B, p0[2] // B)
                rows = _vertex(i0, axis, vl, s0['tsdf'][i0], s1['tsdf'][i1], s0['color'][(slice(None),) + i0] if color else None,
                               s1['color'][(slice(None),) + i1] if color else None, lambda q: sparse._trilinear(blocks, coord, vl, q),
                               [L * float(b) for b in coord[1:]])
                for dst, r in zip(out, rows):
                    dst.append(r)
        result.append((_rows(out[0]), tri, _rows(out[1]), _rows(out[2]) if color else None))
    return result
