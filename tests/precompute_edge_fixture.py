"""Named, seeded clouds that put grid subsampling and the radius search at their geometric edges (numpy only): the cases of
tests/golden/precompute_edges.npz.  tests/golden/generate_precompute_edges_golden.py runs the reference's own binary over them,
tests/test_precompute_edges_cpu.py the C oracle, tests/test_gpu_precompute_edges.py the HIP kernels.

  grid_cases()    name -> dict(points (N, 3) f32, normals (N, 3) f32, lengths [per cloud], voxel, expect)
  radius_cases()  name -> dict(q (Nq, 3) f32, s (Ns, 3) f32, q_lengths, s_lengths, radius, limit, expect[, awkward_rows])

`expect` names the property a case exists for; check_grid_case / check_radius_case assert it with the plain numpy predicates below, so
that a later edit of a generator cannot quietly hollow a case out.  Every case holds at most ~6000 points; the arrays are read-only."""
import functools

import numpy as np

MAX_BATCH = 32                      # SE3_MAX_BATCH of include/se3et_hip.h
GRID_CAP = 64                       # kGridCap of csrc/radius_neighbors.hip: the uniform grid has at most 64 cells per axis
CHAIN_STAGES = 3                    # the grid cases run as a chain: voxel, 2 voxel, 4 voxel
EXACT_VOXEL_COUNTS = (13, 29, 59, 127, 257, 541, 1109, 2357)      # the bucket counts the order emulation steps through (V and V + 1 each)

f32 = np.float32


def _f(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


def _grid(clouds, voxel, seed, **expect):
    pts = np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds]) if clouds else np.zeros((0, 3), np.float32)
    nrm = np.random.default_rng(1000 + seed).normal(size=pts.shape)
    return dict(points=_f(pts), normals=_f(nrm), lengths=[int(np.asarray(c).reshape(-1, 3).shape[0]) for c in clouds], voxel=float(voxel),
                expect=expect)


# ---- predicates -------------------------------------------------------------------------------------------------------------------------
def voxel_indices(cloud, voxel):
    """Signed per-axis voxel indices (n, 3) int64 of ONE cloud, in the float32 arithmetic of the contract (csrc/grid_subsample.hip):
    origin = floor(min * float(1 / voxel)) * voxel, index = floor((p - origin) / voxel)."""
    cloud = np.asarray(cloud, np.float32)
    v = f32(voxel)
    inv = f32(1.0 / float(v))
    org = np.floor(cloud.min(0) * inv) * v
    return np.floor((cloud - org) / v).astype(np.int64)


def negative_index_points(cloud, voxel):
    """Number of points of one cloud that hold a negative (wrapping) voxel index."""
    return int((voxel_indices(cloud, voxel) < 0).any(1).sum()) if len(cloud) else 0


def voxel_keys(cloud, voxel):
    """The map keys ix + nx iy + nx ny iz of one cloud, modulo 2^64 as the contract evaluates them."""
    cloud = np.asarray(cloud, np.float32)
    v = f32(voxel)
    idx = voxel_indices(cloud, voxel)
    org = np.floor(cloud.min(0) * f32(1.0 / float(v))) * v
    nx, ny = [int(np.floor((cloud[:, d].max() - org[d]) / v) + f32(1)) for d in (0, 1)]
    return [(int(i) + nx * int(j) + nx * ny * int(k)) % 2 ** 64 for i, j, k in idx]


def voxel_count(cloud, voxel):
    return len(set(voxel_keys(cloud, voxel))) if len(cloud) else 0


def largest_voxel(cloud, voxel):
    return int(np.unique(np.array(voxel_keys(cloud, voxel), dtype=np.uint64), return_counts=True)[1].max()) if len(cloud) else 0


def split(a, lengths):
    return np.split(np.asarray(a), np.cumsum(lengths)[:-1]) if len(lengths) else []


def extent_over_radius(support, radius):
    """Largest axis extent of one support cloud in units of the radius: beyond GRID_CAP - 1 the uniform grid is capped."""
    support = np.asarray(support, np.float32)
    return float((support.max(0) - support.min(0)).max() / f32(radius)) if len(support) else 0.0


def sq_dists(q, s):
    """(nq, ns) float32 ((dx*dx + dy*dy) + dz*dz), d = query - support: the metric of the contract."""
    d = np.asarray(q, np.float32)[:, None, :] - np.asarray(s, np.float32)[None, :, :]
    with np.errstate(over='ignore', invalid='ignore'):
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def radius_counts(case):
    """(per-row in-radius counts (Nq,), number of (query, support) pairs at d2 == r2 exactly), clouds matched pairwise."""
    r2 = f32(case['radius']) * f32(case['radius'])
    counts, at = [], 0
    for q, s in zip(split(case['q'], case['q_lengths']), split(case['s'], case['s_lengths'])):
        if len(q) == 0 or len(s) == 0:
            counts.append(np.zeros(len(q), np.int64))
            continue
        d2 = sq_dists(q, s)
        counts.append((d2 < r2).sum(1))
        at += int((d2 == r2).sum())
    return (np.concatenate(counts) if counts else np.zeros(0, np.int64)), at


def check_grid_case(name, case):
    """Asserts the property the case exists for."""
    clouds, e, v = split(case['points'], case['lengths']), case['expect'], case['voxel']
    assert sum(case['lengths']) == len(case['points']) <= 6200 and 1 <= len(clouds) <= MAX_BATCH, name
    assert np.isfinite(case['points']).all(), name
    negative = [negative_index_points(c, v) for c in clouds]
    assert negative == e.get('negative', [0] * len(clouds)), '%s: points with a negative voxel index %s' % (name, negative)
    if 'negative_axis' in e:
        for c in clouds:
            assert (voxel_indices(c, v) < 0).any(0).tolist() == [d == e['negative_axis'] for d in range(3)], name
    if 'voxels' in e:
        assert [voxel_count(c, v) for c in clouds] == e['voxels'], '%s: voxel counts %s' % (name, [voxel_count(c, v) for c in clouds])
    if 'one_bucket' in e:
        for c in clouds:
            keys = set(voxel_keys(c, v))
            assert len(keys) == e['one_bucket'] and all(len({k % b for k in keys}) == 1 for b in (13, 29)), name
    if 'largest_voxel' in e:
        assert max(largest_voxel(c, v) for c in clouds) >= e['largest_voxel'], name
        dense = max(clouds, key=lambda c: largest_voxel(c, v))
        assert len(np.unique(dense, axis=0)) == len(dense), '%s: the points of the dense voxel must be distinct' % name
    if 'lengths' in e:
        assert case['lengths'] == e['lengths'], name
    if 'min_coord_below' in e:
        assert float(case['points'].max()) < e['min_coord_below'], name
    if 'min_coord_above' in e:
        assert float(case['points'].min()) > e['min_coord_above'], name


def check_radius_case(name, case):
    e = case['expect']
    assert sum(case['q_lengths']) == len(case['q']) and sum(case['s_lengths']) == len(case['s']), name
    assert len(case['q_lengths']) == len(case['s_lengths']) <= MAX_BATCH and len(case['q']) + len(case['s']) <= 6200, name
    assert np.isfinite(case['s']).all(), name
    ratios = [extent_over_radius(s, case['radius']) for s in split(case['s'], case['s_lengths'])]
    if e.get('capped'):
        assert max(ratios) > GRID_CAP - 1 and max(case['s_lengths']) >= 1500, '%s: extent / radius %s' % (name, ratios)
    else:
        assert max(ratios) < GRID_CAP - 1, '%s: extent / radius %s' % (name, ratios)
    counts, at_radius = radius_counts(case)
    if 'at_radius' in e:
        assert at_radius >= e['at_radius'], '%s: %d pairs at d2 == r2' % (name, at_radius)
    if 'max_count_at_least' in e:
        assert counts.max() >= e['max_count_at_least'], '%s: largest in-radius count %d' % (name, counts.max())
    if 'max_count_below' in e:
        assert 0 < counts.max() < e['max_count_below'], '%s: largest in-radius count %d' % (name, counts.max())
    if 'min_rows_with_hits' in e:
        assert int((counts > 0).sum()) >= e['min_rows_with_hits'], '%s: %d rows with a neighbour' % (name, int((counts > 0).sum()))
    if 'near_radius_pairs' in e:
        r, near = f32(case['radius']), 0
        for q, s in zip(split(case['q'], case['q_lengths']), split(case['s'], case['s_lengths'])):
            near += int(((sq_dists(q, s) < r * r) & (np.abs(q[:, None, :] - s[None, :, :]).max(-1) > f32(0.995) * r)).sum())
        assert near >= e['near_radius_pairs'], '%s: %d in-radius pairs further than 0.995 r apart along an axis' % (name, near)
    if 'flat_axes' in e:
        for s in split(case['s'], case['s_lengths']):
            assert int(((s.max(0) - s.min(0)) == 0).sum()) >= e['flat_axes'], name
    if 'lengths' in e:
        assert (case['q_lengths'], case['s_lengths']) == e['lengths'], name
    if 'awkward_rows' in case:
        assert counts[case['awkward_rows']].max() == 0 and not np.isfinite(case['q'][case['awkward_rows']]).all(), name
        assert counts.max() > 0


# ---- grid-subsampling cases -------------------------------------------------------------------------------------------------------------
def _wrapped(axis, minimum, n, span, seed):
    """Two points whose `axis` coordinate is exactly `minimum`, the other n - 2 above it (by 0.2 ... span), in shuffled order."""
    g = np.random.default_rng(seed)
    c = g.uniform(0.0, span, (n, 3)).astype(np.float32)
    c[:, axis] = f32(minimum) + g.uniform(0.2, span, n).astype(np.float32)
    at = g.choice(n, 2, replace=False)
    c[at, axis] = f32(minimum)
    assert c[:, axis].min() == f32(minimum)
    return c


def _one_per_voxel(count, voxel, seed):
    """`count` points in `count` distinct voxels of a 24^3 block (around the origin), one each, in random order."""
    g = np.random.default_rng(seed)
    cells = g.choice(24 ** 3, count, replace=False)
    ijk = np.stack([cells % 24, cells // 24 % 24, cells // 576], 1) - 12
    return ((ijk + 0.5 + g.uniform(-0.3, 0.3, (count, 3))) * voxel).astype(np.float32)


STACK_SIZES = [0, 1, 13, 14, 700, 0, 29, 30, 2, 59, 60, 127, 128, 5, 1, 0, 257, 258, 3, 541, 542, 1, 7, 100, 0, 33, 64, 65, 1000, 12, 250, 0]


@functools.lru_cache(maxsize=None)
def grid_cases():
    g = np.random.default_rng(20261)
    u = lambda lo, hi, n: g.uniform(lo, hi, (n, 3))
    cases = {}
    cases['centred'] = _grid([u(-1, 1, 3000), u(-1, 1, 2500)], 0.1, 1)
    for axis, ax in enumerate('xyz'):
        # origin = floor(min * float(1 / v)) * v lands one ulp ABOVE the cloud's own minimum: its two points take index -1
        cases['wrap_%s_v0.3' % ax] = _grid([_wrapped(axis, f32(3.3), 900, 6.0, 10 + axis), _wrapped(axis, f32(5.1), 700, 6.0, 20 + axis)], 0.3,
                                           2 + axis, negative=[2, 2], negative_axis=axis)
        lo = [np.nextafter(f32(k) * f32(0.025), f32(-np.inf)) for k in (-319, -314)]
        cases['wrap_%s_v0.025' % ax] = _grid([_wrapped(axis, lo[0], 900, 1.0, 30 + axis), _wrapped(axis, lo[1], 700, 1.0, 40 + axis)], 0.025,
                                             5 + axis, negative=[2, 2], negative_axis=axis)
    # coordinates on multiples of half the voxel (every second one a voxel boundary), all negative or zero
    cases['negative_lattice'] = _grid([g.integers(-40, 1, (3000, 3)) * f32(0.025), g.integers(-24, 1, (2000, 3)) * f32(0.025)], 0.05, 8,
                                      min_coord_below=1e-9)
    kitti = lambda n: u(-1, 1, n) * np.array([80.0, 80.0, 3.0])
    cases['kitti_extent'] = _grid([kitti(3500), kitti(2500)], 0.3, 9)
    cases['offset_p1000'] = _grid([u(0, 2, 3000) + 1000.0, u(0, 1, 2000) + 1000.0], 0.1, 10, min_coord_above=999.0)
    cases['offset_m777'] = _grid([u(0, 2, 3000) - 777.0, u(0, 1, 2000) - 777.0], 0.1, 11, min_coord_below=-774.0)
    t = g.uniform(-3, 3, (1500, 1))
    cases['line'] = _grid([t * np.array([[1.0, 0.5, -0.25]]), t[:400] * np.array([[0.0, 0.0, 1.0]])], 0.1, 12)
    plane = u(-2, 2, 2500)
    plane[:, 2] = 0.375
    cases['plane'] = _grid([plane, plane[:300, [2, 0, 1]]], 0.1, 13)
    cases['identical'] = _grid([np.tile([[0.3, -1.7, 2.9]], (500, 1)), np.tile([[-5.0, 0.0, 0.0]], (2, 1))], 0.1, 14, voxels=[1, 1])
    cases['single_point'] = _grid([[[1.5, -2.5, 0.25]], [[0.0, 0.0, 0.0]], [[-3.3, 3.3, 5.1]]], 0.1, 15, voxels=[1, 1, 1])
    base = u(-1, 1, 1200)
    cases['tripled'] = _grid([np.concatenate([base, base, base])[g.permutation(3600)], np.repeat(base[:300], 3, 0)], 0.1, 16)
    cases['exact_voxels_1'] = _grid([_one_per_voxel(1, 0.25, 50)], 0.25, 17, voxels=[1])
    for i, v in enumerate(EXACT_VOXEL_COUNTS):
        cases['exact_voxels_%d_%d' % (v, v + 1)] = _grid([_one_per_voxel(v, 0.25, 60 + i), _one_per_voxel(v + 1, 0.25, 80 + i)], 0.25, 18 + i,
                                                         voxels=[v, v + 1])
    # 12 voxels in one row whose x indices are multiples of 13 * 29: one bucket chain at the 13-bucket and at the 29-bucket step
    chain = lambda reps: np.stack([(np.repeat(g.permutation(12), reps) * 377 + g.uniform(0.1, 0.9, 12 * reps)) * 0.25,
                                   np.full(12 * reps, 0.125), np.full(12 * reps, -0.125)], 1)
    cases['bucket_chain'] = _grid([chain(1), chain(3)], 0.25, 30, voxels=[12, 12], one_bucket=12)
    # 2000 distinct points of one voxel at coordinates near 100, interleaved with a sparse cloud: the float32 sum of the voxel's
    # members depends on their order
    # (jitter of +-130 float32 steps of 2^-17 = +-1e-3: exact, so distinct integers stay distinct points)
    dense = (f32(100.05) + np.unique(g.integers(-130, 131, (2600, 3)), axis=0)[:2000].astype(np.float32) * f32(2.0 ** -17)).astype(np.float32)
    both = np.concatenate([dense, u(97, 103, 600)])[g.permutation(len(dense) + 600)]
    cases['dense_voxel'] = _grid([both, u(97, 103, 500)], 0.3, 31, largest_voxel=2000)
    # point counts around the 1024 threads of the one-workgroup scans, nearly every point in a voxel of its own
    cases['sizes_1023_1024_1025'] = _grid([u(-1, 1, 1023), u(-1, 1, 1024), u(-1, 1, 1025)], 0.02, 32, lengths=[1023, 1024, 1025])
    cases['sizes_2047_2049'] = _grid([u(-1, 1, 2047), u(-1, 1, 2049)], 0.02, 33, lengths=[2047, 2049])
    cases['stack32'] = _grid([u(-1, 1, n) for n in STACK_SIZES], 0.1, 34, lengths=STACK_SIZES)
    assert len(STACK_SIZES) == MAX_BATCH and STACK_SIZES[0] == STACK_SIZES[15] == STACK_SIZES[-1] == 0
    return cases


# ---- radius-search cases ----------------------------------------------------------------------------------------------------------------
def _radius(q, s, q_lengths, s_lengths, radius, limit, awkward_rows=None, **expect):
    c = dict(q=_f(np.asarray(q).reshape(-1, 3)), s=_f(np.asarray(s).reshape(-1, 3)), q_lengths=[int(v) for v in q_lengths],
             s_lengths=[int(v) for v in s_lengths], radius=float(radius), limit=int(limit), expect=expect)
    if awkward_rows is not None:
        c['awkward_rows'] = [int(r) for r in awkward_rows]
    return c


# the rows put behind the `awkward` case's second cloud; all but the first two must come back as padding only
AWKWARD_FAR = [[1e6, 0.5, 0.5], [0.5, 1e30, 0.5], [0.5, 0.5, -1e30], [np.inf, 0.5, 0.5], [0.5, -np.inf, 0.5], [0.5, 0.5, np.nan],
               [np.nan, np.nan, np.nan], [np.inf, -np.inf, np.nan]]


def without_awkward_rows(case):
    """The same case without the rows listed in awkward_rows (they all sit in the last cloud)."""
    keep = np.setdiff1d(np.arange(len(case['q'])), case['awkward_rows'])
    ql = list(case['q_lengths'])
    ql[-1] -= len(case['awkward_rows'])
    assert min(case['awkward_rows']) >= sum(case['q_lengths'][:-1])
    return dict(case, q=_f(case['q'][keep]), q_lengths=ql), keep


@functools.lru_cache(maxsize=None)
def radius_cases():
    g = np.random.default_rng(20262)
    u = lambda lo, hi, n: g.uniform(lo, hi, (n, 3))
    cases = {}
    # extent / radius = 200: cell = extent / 63 instead of the radius
    bar = u(0, 1, 3000) * np.array([100.0, 1.0, 1.0])
    cases['capped_bar'] = _radius(u(-0.02, 1.02, 800) * np.array([100.0, 1.0, 1.0]), bar, [800], [3000], 0.5, 40, capped=True,
                                  min_rows_with_hits=700)
    centres = u(-1, 1, 250) * np.array([80.0, 80.0, 3.0])
    slab = lambda n: centres[g.integers(0, 250, n)] + g.normal(0, 0.4, (n, 3))
    cases['capped_slab'] = _radius(np.concatenate([slab(500), slab(400)]), np.concatenate([slab(2500), slab(1600)]), [500, 400], [2500, 1600],
                                   0.75, 38, capped=True, min_rows_with_hits=700, max_count_at_least=10)
    plane = u(0, 2, 2000)
    plane[:, 2] = -0.5
    qp = u(-0.1, 2.1, 500)
    qp[:, 2] = g.choice([-0.5, -0.45, -0.65], 500)
    cases['flat_plane'] = _radius(qp, plane, [500], [2000], 0.1, 30, flat_axes=1, min_rows_with_hits=300)
    line = g.uniform(0, 4, (1600, 1)) * np.array([[1.0, 0.0, 0.0]]) + np.array([[0.0, 1.0, 2.0]])
    ql = g.uniform(-0.2, 4.2, (300, 1)) * np.array([[1.0, 0.0, 0.0]]) + np.array([[0.0, 1.0, 2.0]]) + g.choice([0.0, 0.03], (300, 1))
    cases['flat_line'] = _radius(ql, line, [300], [1600], 0.08, 64, flat_axes=2, min_rows_with_hits=250)
    same = np.tile([[0.25, -0.5, 1.0]], (300, 1))
    qs = same[:60] + g.choice([0.0, 0.05, 0.2], (60, 1)) * np.array([[1.0, 0.0, 0.0]])
    cases['identical_support'] = _radius(qs, same, [60], [300], 0.1, 64, flat_axes=3, max_count_at_least=300)
    cases['offset_p1000'] = _radius(u(0, 1, 500) + 1000.0, u(0, 1, 2000) + 1000.0, [300, 200], [1200, 800], 0.1, 38, min_rows_with_hits=400)
    cases['offset_m1000'] = _radius(u(0, 1, 500) - 1000.0, u(0, 1, 2000) - 1000.0, [300, 200], [1200, 800], 0.1, 38, min_rows_with_hits=400)
    # pairs whose separation along ONE axis is just under the radius (0.999 r): a grid cell that is not strictly larger than the radius puts
    # some of them two cells apart, where the 3 x 3 x 3 block no longer reaches
    sup = u(0, 2, 2100)
    cases['near_radius'] = _radius(sup + np.repeat(np.eye(3), 700, 0) * g.choice([-0.0999, 0.0999], (2100, 1)), sup, [1200, 900], [1200, 900], 0.1, 38,
                                   near_radius_pairs=2000)
    # lattice step 0.25, radius 0.5: the neighbours two steps away along an axis sit at d2 == r2 exactly and are NOT neighbours
    lattice = lambda n: np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing='ij'), -1).reshape(-1, 3) * f32(0.25) - f32(1.0)
    a, b = lattice(8)[g.permutation(512)], lattice(12)[g.permutation(1728)]
    cases['exact_radius'] = _radius(np.concatenate([a, b]), np.concatenate([a, b]), [512, 1728], [512, 1728], 0.5, 30, at_radius=6000,
                                    max_count_below=28)
    # the exhaustive kernel: 1024 support points per LDS tile, 16 queries per workgroup
    for name, sl, ql_, limits in (('tile_a', [1023, 1024, 1025], [1, 15, 16], (1, 64)), ('tile_b', [2048, 2049, 300], [17, 63, 65], (2, 63))):
        s, q = u(0, 1, sum(sl)), u(-0.05, 1.05, sum(ql_))
        for limit in limits:
            cases['%s_limit%d' % (name, limit)] = _radius(q, s, ql_, sl, 0.25, limit, max_count_at_least=65, lengths=(ql_, sl))
    cluster, qc = u(0, 0.35, 1600), u(0.12, 0.23, 200)
    for limit in (64, 5):
        cases['dense_cluster_limit%d' % limit] = _radius(qc, cluster, [120, 80], [1000, 600], 0.125, limit, max_count_at_least=150)
    cases['small_support'] = _radius(u(0, 0.3, 30), u(0, 0.3, 8), [20, 10], [5, 3], 0.3, 16, max_count_below=6)
    # 32 stacked clouds, some of them empty on the query side, on the support side, or on both
    sizes = [0, 3, 40, 17, 0, 65, 16, 1, 90, 33, 0, 15, 64, 7, 120, 0, 63, 2, 31, 100, 5, 0, 48, 16, 9, 200, 1, 0, 77, 12, 150, 0]
    zero = lambda v, at: [0 if i in at else n for i, n in enumerate(v)]
    some = (2, 8, 13, 19, 24, 29)                   # (non-empty clouds; no two neighbouring clouds end up without queries)
    for name, q_len, s_len in (('stack32_empty_queries', zero(sizes, some[::2]), [2 * n for n in sizes]),
                               ('stack32_empty_supports', sizes, zero([2 * n for n in sizes], some[1::2])),
                               ('stack32_empty_both', sizes, [2 * n for n in sizes])):
        cases[name] = _radius(u(0, 1, sum(q_len)), u(0, 1, sum(s_len)), q_len, s_len, 0.2, 24, lengths=(q_len, s_len),
                              min_rows_with_hits=300)
    assert len(sizes) == MAX_BATCH
    # awkward queries behind an ordinary cloud: one cell outside the support box, exactly on a corner of it, far away, infinite, NaN
    s = u(0, 1, 3200)
    s[0], s[1700] = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    near = [[1.0 + 0.12, 0.5, 0.5], [-0.12, -0.12, 0.5], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]
    q = np.concatenate([u(-0.1, 1.1, 400), u(-0.1, 1.1, 300), near, AWKWARD_FAR])
    cases['awkward'] = _radius(q, s, [400, 300 + len(near) + len(AWKWARD_FAR)], [1700, 1500], 0.1, 38,
                               awkward_rows=range(len(q) - len(AWKWARD_FAR), len(q)), min_rows_with_hits=500)
    return cases
