"""Named, seeded LATTICE clouds that put the selections on the superpoint level at their exact ties and capacity edges (numpy only):
csrc/partition.hip (knn3, point_to_node_partition and their stack forms) and the index half of the geometric embedding
(csrc/geo_records.hip, csrc/geo_embedding.hip).  tests/test_superpoint_edges_cpu.py holds the twin (superpoint_twin.py) to the oracle on
them, tests/test_gpu_superpoint_edges.py the HIP kernels to the twin.

Every coordinate is k / 8 with integer 0 <= k < 128, so squared distances, cross and dot products are exact in float32 and the twin
is integer arithmetic (superpoint_twin.py).  The generators work in the integer k and divide at the end.

  partition_cases()  name -> dict(points (N, 3) f32, nodes (M, 3) f32, limits (...), expect[, point_lengths, node_lengths])
  knn3_cases()       name -> dict(points (N, 3) f32, expect[, lengths])
  embedding_cases()  name -> dict(points (N, 3) f32, expect)

`expect` names the property a case exists for; check_partition_case / check_knn3_case / check_embedding_case assert it with plain integer
predicates, so that a later edit of a generator cannot quietly hollow a case out.  At most ~1500 points and 130 nodes per case (the
`between` case needs 130 nodes: two passes and a remainder of the 64 lanes that stride over them); the arrays are read-only."""
import functools

import numpy as np

from superpoint_twin import LATTICE, lattice_units

MAX_BATCH = 32                      # SE3_MAX_BATCH of include/se3et_hip.h
MAX_LIMIT = 128                     # csrc/partition.hip: two registers of 64 ranks
STACK_CUT_POINTS = [1, 2, 3, 5, 63, 65, 130, 4]
STACK_CUT_NODES = [1, 1, 2, 3, 7, 64, 9, 6]          # (the last cloud has more nodes than points)
OWN_COUNTS = [1, 63, 64, 65, 127, 128, 129, 200, 2, 66, 126]          # own points of nodes 0 .. 10 of `counts`; node 11 duplicates node 7


def _pts(k):
    k = np.asarray(k, np.int64).reshape(-1, 3)
    assert (k >= 0).all() and (k < 128).all()
    a = np.ascontiguousarray(k.astype(np.float32) / np.float32(LATTICE))
    a.setflags(write=False)
    return a


def _case(points, nodes, limits, point_lengths=None, node_lengths=None, **expect):
    c = dict(points=_pts(points), nodes=_pts(nodes), limits=tuple(int(v) for v in limits), expect=expect)
    if point_lengths is not None:
        c['point_lengths'], c['node_lengths'] = [int(v) for v in point_lengths], [int(v) for v in node_lengths]
    return c


# ---- integer predicates -----------------------------------------------------------------------------------------------------------------
def units(a, b):
    """(len(a), len(b)) int64 squared distances in 1 / 64 units."""
    d = lattice_units(a)[:, None, :] - lattice_units(b)[None, :, :]
    return (d * d).sum(-1)


def split(a, lengths):
    return np.split(np.asarray(a), np.cumsum(lengths)[:-1])


def owners(points, nodes):
    """(nearest node per point with the lowest index among equals, number of nodes at the minimal distance per point)."""
    d = units(nodes, points)
    return d.argmin(0), (d == d.min(0, keepdims=True)).sum(0)


def own_distances(points, nodes, node):
    """Distances of a node's own points in STORAGE order."""
    d = units(nodes, points)
    return d[node][owners(points, nodes)[0] == node]


def check_partition_case(name, case):
    e, pts, nodes = case['expect'], case['points'], case['nodes']
    assert len(pts) <= 1500 and len(nodes) <= 130 and all(1 <= k for k in case['limits']), name
    lattice_units(pts), lattice_units(nodes)
    if 'point_lengths' in case:
        pl, nl = case['point_lengths'], case['node_lengths']
        assert sum(pl) == len(pts) and sum(nl) == len(nodes) and len(pl) == len(nl) <= MAX_BATCH and min(pl) >= 1 and min(nl) >= 1, name
        if 'lengths' in e:
            assert (pl, nl) == e['lengths'], name
        if e.get('cut_inside_workgroup'):
            inner = np.cumsum(pl)[:-1]
            assert (inner % 4 != 0).any() and (inner % 64 != 0).all() and (np.cumsum(nl)[:-1] % 4 != 0).any(), name
        if e.get('more_nodes_than_points'):
            assert any(m > n for n, m in zip(pl, nl)), name
        return
    own, ways = owners(pts, nodes)
    counts = np.bincount(own, minlength=len(nodes))
    if 'own_counts' in e:
        assert counts.tolist() == e['own_counts'], '%s: own-point counts %s' % (name, counts.tolist())
    if 'duplicate_nodes' in e:
        lo, hi = e['duplicate_nodes']
        assert lo < hi and (nodes[lo] == nodes[hi]).all() and counts[hi] == 0 and counts[lo] > 0, name
    if 'descending' in e or 'ascending' in e:
        d = own_distances(pts, nodes, 0)
        assert len(d) == e.get('descending', e.get('ascending')), name
        assert ((d[1:] < d[:-1]) if 'descending' in e else (d[1:] > d[:-1])).all(), '%s: own distances must be strictly monotonic in storage' % name
    if 'shell_size' in e:
        d = own_distances(pts, nodes, 0)
        assert np.unique(d, return_counts=True)[1].min() >= e['shell_size'], name
        assert not (d[1:] >= d[:-1]).all(), '%s: storage order must not be distance order' % name
        s = np.sort(d)
        for k in case['limits']:
            assert k < len(s) and s[k - 1] == s[k], '%s: limit %d must cut inside a shell' % (name, k)
    if 'tie_ways' in e:
        for w in e['tie_ways']:
            assert int((ways == w).sum()) >= 1, '%s: no point equidistant from exactly %d nodes' % (name, w)
        if e.get('ties_across_lanes'):          # a tie between nodes m and m + 64 or m + 128: ONE lane meets both, in two passes of its loop
            d = units(nodes, pts)
            tied = d == d.min(0, keepdims=True)
            same_lane = [i for i in range(len(pts)) if len(set(np.nonzero(tied[:, i])[0] % 64)) < int(tied[:, i].sum())]
            assert len(same_lane) >= 1, '%s: no point whose nearest nodes tie inside one lane' % name
    if 'tail_of' in e:
        n = len(pts)
        start = 64 * ((n - 1) // 64)
        assert n == e['tail_of'] and (np.nonzero(own == 0)[0] >= start).all() and counts[0] == n - start, name
    if 'limit_above_points' in e:
        assert max(case['limits']) > len(pts) == e['limit_above_points'], name
    if 'num_points' in e:
        assert len(pts) == e['num_points'], name


def check_knn3_case(name, case):
    e, pts = case['expect'], case['points']
    lattice_units(pts)
    if 'lengths' in case:
        assert sum(case['lengths']) == len(pts) and case['lengths'] == e['lengths'], name
        return
    assert len(pts) == e['points'], name
    d = units(pts, pts)
    if e.get('tied_rows'):
        # rows in which the cut between the 4 kept ranks and the rest, or the order among them, is decided by index
        s = np.sort(d, 1)[:, :5]
        assert int((s[:, 1:] == s[:, :-1]).any(1).sum()) >= e['tied_rows'], name
    if e.get('rank0_is_a_lower_duplicate'):
        rows = [i for i in range(len(pts)) if (d[i, :i] == 0).any()]
        assert len(rows) >= e['rank0_is_a_lower_duplicate'], name


def angle_census(points, knn):
    """Exact integer census of the (n, m, k) angle triples of an embedding case: dict(zero_ref, deg0, deg180, deg90, coincident_pairs)."""
    p, knn = lattice_units(points), np.asarray(knn, np.int64)
    anc = p[None, :, :] - p[:, None, :]
    ref = p[knn] - p[:, None, :]
    r, a = np.broadcast_arrays(ref[:, None, :, :], anc[:, :, None, :])
    cross0 = (np.cross(r, a) == 0).all(-1)
    dot = (r * a).sum(-1)
    nz = (r != 0).any(-1) & (a != 0).any(-1)
    off = ~np.eye(len(p), dtype=bool)
    return dict(zero_ref=int((ref == 0).all(-1).sum()), deg0=int((nz & cross0 & (dot > 0)).sum()), deg180=int((nz & cross0 & (dot < 0)).sum()),
                deg90=int((nz & ~cross0 & (dot == 0)).sum()), coincident_pairs=int(((anc == 0).all(-1) & off).sum()) // 2)


def check_embedding_case(name, case, knn):
    """`knn` is the twin's knn3 of the case (superpoint_twin.knn3)."""
    e = case['expect']
    assert len(case['points']) == e['points'] <= 65, name
    census = angle_census(case['points'], knn)
    for key, least in e.items():
        if key != 'points':
            assert census[key] >= least, '%s: %s = %d, expected at least %d' % (name, key, census[key], least)


# ---- partition cases --------------------------------------------------------------------------------------------------------------------
def _box(lo, hi):
    r = np.arange(lo, hi + 1)
    return np.stack(np.meshgrid(r, r, r, indexing='ij'), -1).reshape(-1, 3)


def _around(g, centre, count, reach=9):
    """`count` distinct lattice points within `reach` of `centre` along every axis."""
    offsets = _box(-reach, reach)
    return np.asarray(centre) + offsets[g.choice(len(offsets), count, replace=False)]


@functools.lru_cache(maxsize=None)
def partition_cases():
    g = np.random.default_rng(20263)
    cases = {}
    # node centres 40 lattice steps apart, own points within 9 steps of their centre: 15.6 from it at most, 31 from any other at least
    centres = (20 + 40 * _box(0, 2))[g.permutation(27)[:len(OWN_COUNTS)]]
    nodes = np.concatenate([centres, centres[7:8]])
    pts = np.concatenate([_around(g, c, n) for c, n in zip(centres, OWN_COUNTS)])
    cases['counts'] = _case(pts[g.permutation(len(pts))], nodes, (1, 63, 64, 65, 127, 128), own_counts=OWN_COUNTS + [0], duplicate_nodes=(7, 11))

    # one point per distinct squared distance, 200 of them, far first; a second node takes three points of its own
    offsets = _box(-12, 12)
    d2 = (offsets ** 2).sum(1)
    _, first = np.unique(d2, return_index=True)
    ring = offsets[first[1:201]][::-1]                                      # strictly descending distance
    assert len(ring) == 200
    far = np.array([[100, 100, 100], [101, 100, 100], [100, 103, 100]])
    two = np.array([[30, 30, 30], [100, 101, 100]])
    cases['descending'] = _case(np.concatenate([30 + ring, far]), two, (64, 128), descending=200)
    cases['ascending'] = _case(np.concatenate([30 + ring[::-1], far]), two, (64, 128), ascending=200)

    # (+-a, +-b, +-c) with a, b, c in 1..3: 216 points on shells of 8, 24 or 48; sorted shell ends at 8, 32, 56, 80, 88, 136, ...
    shell = _box(-3, 3)
    shell = shell[(shell != 0).all(1)]
    cases['shells'] = _case(np.concatenate([40 + shell, far])[g.permutation(len(shell) + 3)], np.array([[40, 40, 40], [100, 101, 100]]), (16, 64, 128),
                            shell_size=8)

    # nodes on half of the sites of a coarse grid (8 steps), points on the half-step sites in between: equidistant from 2, 3, 4 ... nodes
    for m, side in ((1, 1), (2, 2), (64, 5), (65, 5), (130, 6)):
        sites = 8 * _box(0, side - 1) + 40
        nd = sites[g.permutation(len(sites))[:m]] if m > 2 else np.array([[40, 40, 40], [48, 40, 40]])[:m]
        p = 40 - 4 + 4 * g.integers(0, 2 * side + 1, (300, 3))
        ways = tuple(w for w in (2, 3) if w <= m)
        cases['between_m%d' % m] = _case(p, nd, (64,), tie_ways=ways, ties_across_lanes=m > 64, num_points=300)

    # node 0 owns exactly the points of the last 64-chunk, node 1 all others
    for n in (1, 63, 64, 65, 129):
        start = 64 * ((n - 1) // 64)
        p = np.concatenate([_around(g, [90, 90, 90], start) if start else np.zeros((0, 3), np.int64), _around(g, [30, 30, 30], n - start)])
        cases['tail_n%d' % n] = _case(p, np.array([[30, 30, 30], [90, 90, 90]]), (64, 128), tail_of=n)

    cases['wide_small_n5'] = _case(g.integers(30, 40, (5, 3)), g.integers(30, 40, (2, 3)), (128, 64, 6), limit_above_points=5)
    cases['wide_small_n64'] = _case(g.integers(30, 40, (64, 3)), g.integers(30, 40, (3, 3)), (64, 128), num_points=64)

    # all clouds in the SAME small box: a point or node that looks across its cloud boundary finds nearer candidates there
    cases['stack_cuts'] = _case(g.integers(20, 36, (sum(STACK_CUT_POINTS), 3)), g.integers(20, 36, (sum(STACK_CUT_NODES), 3)), (3, 64, 128),
                                STACK_CUT_POINTS, STACK_CUT_NODES, lengths=(STACK_CUT_POINTS, STACK_CUT_NODES), cut_inside_workgroup=True,
                                more_nodes_than_points=True)
    pl, nl = g.integers(3, 10, MAX_BATCH).tolist(), g.integers(1, 5, MAX_BATCH).tolist()
    pl[0], pl[-1] = 3, 9
    cases['stack32'] = _case(g.integers(20, 30, (sum(pl), 3)), g.integers(20, 30, (sum(nl), 3)), (4, 65), pl, nl, lengths=(pl, nl))
    return cases


def single_cloud_cases():
    return {k: v for k, v in partition_cases().items() if 'point_lengths' not in v}


def stack_cases():
    return {k: v for k, v in partition_cases().items() if 'point_lengths' in v}


def cloud_of(case, c):
    """Cloud c of a stack case as a single-cloud (points, nodes)."""
    return split(case['points'], case['point_lengths'])[c], split(case['nodes'], case['node_lengths'])[c]


# ---- knn3 cases -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def knn3_cases():
    g = np.random.default_rng(20264)
    cases = {}
    for n in (1, 2, 3, 4, 5, 64, 65, 257):
        # a 6 x 6 x 6 box: ties in nearly every row from 64 points on, duplicates forced at 257
        cases['n%d' % n] = dict(points=_pts(g.integers(50, 56, (n, 3))), expect=dict(points=n, tied_rows=n // 2 if n >= 64 else 0))
    cases['lattice70'] = dict(points=_pts(g.integers(10, 14, (70, 3))), expect=dict(points=70, tied_rows=60, rank0_is_a_lower_duplicate=6))
    cases['stack_cuts'] = dict(points=_pts(g.integers(20, 28, (sum(STACK_CUT_POINTS), 3))), lengths=list(STACK_CUT_POINTS),
                               expect=dict(lengths=list(STACK_CUT_POINTS)))
    return cases


# ---- embedding cases --------------------------------------------------------------------------------------------------------------------
def _distinct(g, n, lo, hi):
    sites = _box(lo, hi - 1)
    return sites[g.choice(len(sites), n, replace=False)]


@functools.lru_cache(maxsize=None)
def embedding_cases():
    g = np.random.default_rng(20265)
    cases = {}
    p = _distinct(g, 40, 8, 20)
    p[5], p[17], p[21], p[33] = p[2], p[30], p[20], p[20]                   # two pairs and a triple
    cases['coincident'] = dict(points=_pts(p), expect=dict(points=40, coincident_pairs=5, zero_ref=7))
    p = _distinct(g, 33, 8, 16)
    p[9], p[19], p[29] = p[3], p[3], p[3]                                   # four identical points: all three reference vectors vanish
    p[32] = p[0]
    cases['zero_ref'] = dict(points=_pts(p), expect=dict(points=33, coincident_pairs=7, zero_ref=14))
    cases['zero_ref_n1'] = dict(points=_pts([[9, 9, 9]]), expect=dict(points=1, zero_ref=3))
    cases['zero_ref_n3'] = dict(points=_pts([[9, 9, 9], [9, 10, 9], [12, 9, 9]]), expect=dict(points=3, zero_ref=3))
    # four runs of lattice points on lines (the nearest neighbours of a run's inner points are its own points), 65 points in all
    runs = [np.array(b) + np.arange(n)[:, None] * np.array(s) for b, s, n in (([8, 8, 8], [1, 0, 0], 20), ([8, 40, 8], [1, 2, 0], 17),
                                                                               ([40, 8, 40], [1, 1, 1], 15), ([60, 60, 8], [0, 2, 1], 13))]
    cases['collinear'] = dict(points=_pts(np.concatenate(runs)[g.permutation(65)]), expect=dict(points=65, deg0=300, deg180=300))
    cases['right_angles'] = dict(points=_pts((8 + 2 * _box(0, 2))[g.permutation(27)]), expect=dict(points=27, deg90=500, deg180=10))
    return cases
