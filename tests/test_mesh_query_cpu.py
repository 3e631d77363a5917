"""CPU: the se3_debug_mesh_*_host entries of csrc/mesh_query.hip against the float64 twin written from the contract
(tests/mesh_query_twin.py): the brute-force cast and closest point equal exactly (ids) and bit for bit (t, uvs, normals, points,
distances) on every named case; the host tree's invariants; the kernels' walk over that tree equal to the brute force; watertightness as
a condition; the twin's closest point against an independent bound; the hit point; and the modelled kernel mistakes, each of which
changes a named case."""
import numpy as np
import pytest

import mesh_query_fixture as F
import mesh_query_twin as twin

CASES = F.cases()
NAMES = list(CASES)
EPS = 2.0 ** -52


def _tree(name):
    nodes, counts, keys, order = F.host_tree(name)
    return nodes, counts, keys, order, int(counts[3])


# ---- host against twin ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_brute_force_cast_equals_the_twin(name):
    v, t = CASES[name]
    rays = F.rays(name)
    got, want = F.host_brute(name)[0], twin.cast(v, t, rays)
    assert F.same(got[1], want[1])
    for g, w, what in zip(got, want, ('t_hit', 'primitive_ids', 'primitive_uvs', 'primitive_normals')):
        assert F.same(g, w), what
    assert F.same(got[4], (got[0] < np.inf).astype(np.uint8))                                 # any-hit is t_hit < inf
    assert (got[1] >= 0).sum() > 0 or name == 'no_triangles'


@pytest.mark.parametrize('name', NAMES)
def test_brute_force_closest_point_equals_the_twin(name):
    v, t = CASES[name]
    got, want = F.host_brute(name)[1], twin.closest(v, t, F.queries(name))
    for g, w, what in zip(got, want, ('points', 'distances', 'primitive_ids', 'primitive_uvs', 'primitive_normals')):
        assert F.same(g, w), what
    if name == 'no_triangles':
        assert got[1][0] == np.inf and got[2][0] == -1                                        # a mesh without a live triangle
    assert np.isnan(got[1][2]) and got[2][2] == -1 and np.isnan(got[0][2]).all()              # the query that is not finite


@pytest.mark.parametrize('name', ['one', 'cube', 'icosphere', 'coincident_200'])
def test_t_max_exactly_at_a_hit(name):
    v, t = CASES[name]
    rays = F.rays(name)
    t_hit, ids = F.host_brute(name)[0][:2]
    for r in np.nonzero(ids >= 0)[0][:24]:
        at = F.host_cast(v, t, rays[r:r + 1], t_max=t_hit[r])
        want = twin.cast(v, t, rays[r:r + 1], t_max=t_hit[r])
        assert at[1][0] == ids[r] == want[1][0] and F.same(at[0], want[0])
        below = F.host_cast(v, t, rays[r:r + 1], t_max=np.nextafter(t_hit[r], -np.inf))
        assert below[1][0] != ids[r] or below[0][0] < t_hit[r]


def test_inert_triangles_and_status_words():
    status = {name: F.host_tree(name)[1].tolist() for name in NAMES}
    assert status['bad_triangle'][:3] == [1, 2, 0] and status['nan_vertex'][:3] == [8, 2, 0] and status['zero_area'][:3] == [0, 2, 2]
    assert status['no_triangles'] == [0, 0, 0, -1] and status['one'] == [0, 1, 0, 1]          # one live triangle: the leaf m is the root
    for name in ('bad_triangle', 'nan_vertex', 'zero_area'):
        v, t = CASES[name]
        inert = np.nonzero(twin.kinds(v, t) != twin.LIVE)[0]
        assert not np.isin(F.host_brute(name)[0][1], inert).any() and not np.isin(F.host_brute(name)[1][2], inert).any()


# ---- the tree -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_tree_invariants(name):
    v, t = CASES[name]
    nodes, counts, keys, order, root = _tree(name)
    m, live = len(t), twin.kinds(v, t) == twin.LIVE
    assert counts[1] == live.sum() and (keys[live] >= 0).all() and (keys[~live] == -1).all()
    assert sorted(order.tolist()) == list(range(m)) and live[order[:live.sum()]].all()
    if root < 0:
        assert not live.any() and not nodes.view(np.int64).any()
        return
    seen, stack, inner = [], [root], 0
    assert nodes[root]['parent'] == -1
    while stack:
        i = stack.pop()
        node = nodes[i]
        if node['left'] < 0:
            tri = -1 - int(node['left'])
            assert node['right'] == node['left'] and i == m + list(order).index(tri)
            p = v[t[tri]]
            assert F.same(node['lo'], p.min(0)) and F.same(node['hi'], p.max(0))
            seen.append(tri)
            continue
        inner += 1
        a, b = nodes[int(node['left'])], nodes[int(node['right'])]
        assert a['parent'] == i and b['parent'] == i
        assert F.same(node['lo'], np.minimum(a['lo'], b['lo'])) and F.same(node['hi'], np.maximum(a['hi'], b['hi']))      # the exact union
        stack += [int(node['left']), int(node['right'])]
    assert sorted(seen) == np.nonzero(live)[0].tolist()                                       # every live triangle once, no inert one
    assert inner == live.sum() - 1
    used = np.zeros(len(nodes), bool)
    used[:inner], used[m:m + live.sum()] = True, True
    assert not nodes[~used].view(np.int64).any()                                              # every other node is cleared
    assert F.depth_of(nodes, root) <= 94


def test_the_chain_is_deeper_than_one_trail_word():
    nodes, counts, _, _, root = _tree('chain')
    assert F.depth_of(nodes, root) > 64


def test_topology_depends_on_the_sorted_order_only():
    v, t = CASES['icosphere']
    nodes, _, keys, order, _ = _tree('icosphere')
    moved = F.host_bvh(v * 4.0, t)                                    # (a power of two scales every step exactly: the keys are the same)
    assert F.same(moved[2], keys)
    for field in ('left', 'right', 'parent'):
        assert F.same(moved[0][field], nodes[field])
    assert not F.same(moved[0]['lo'], nodes['lo'])
    v, t = CASES['coincident_200']
    nodes, _, keys, order, _ = _tree('coincident_200')
    assert (keys == keys[0]).all() and order.tolist() == list(range(200))                     # equal keys: split by position alone
    other = F.host_bvh(v, t, order=order[::-1].copy())
    for field in ('left', 'right', 'parent'):
        assert F.same(other[0][field][:199], nodes[field][:199])


@pytest.mark.parametrize('name', NAMES)
def test_the_walk_over_the_tree_equals_the_brute_force(name):
    v, t = CASES[name]
    nodes, counts, _, _, _ = _tree(name)
    cast, closest = F.host_brute(name)
    for g, w in zip(F.host_cast(v, t, F.rays(name), tree=(nodes, counts)), cast):
        assert F.same(g, w)
    for g, w in zip(F.host_closest(v, t, F.queries(name), tree=(nodes, counts)), closest):
        assert F.same(g, w)
    t_hit, ids = cast[:2]
    for r in np.nonzero(ids >= 0)[0]:                                                         # t_max exactly at the hit
        at = F.host_cast(v, t, F.rays(name)[r:r + 1], t_max=t_hit[r], tree=(nodes, counts))
        assert at[1][0] == ids[r] and at[4][0] == 1


def test_coincident_copies_the_lowest_number_wins():
    cast, closest = F.host_brute('coincident_200')
    assert set(cast[1].tolist()) == {-1, 0} and set(closest[2].tolist()) == {-1, 0}


# ---- watertightness, as a condition -----------------------------------------------------------------------------------------------------------------
def _watertight_rays():
    v, t = CASES['icosphere']
    rng = np.random.default_rng(2013)
    edges = np.unique(np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1), axis=0)
    a, b = v[edges[:, 0]], v[edges[:, 1]]
    where = np.concatenate([np.array([0.5, 0.25, 1.0 / 3.0]), rng.uniform(0, 1, 20)])
    targets = np.concatenate([v] + [a + (b - a) * w for w in where])
    origin = F.ICOSPHERE_CENTER + np.array([0.11, -0.07, 0.05])
    return np.concatenate([np.broadcast_to(origin, targets.shape), targets - origin], 1)


def test_no_ray_slips_between_two_triangles():
    """From a point inside the closed icosphere, at every vertex and at 23 points of every edge: 11 202 rays, NONE may miss.  The naive
    Moeller-Trumbore test of the twin file misses several hundred of the same rays: the condition has power."""
    v, t = CASES['icosphere']
    rays = _watertight_rays()
    assert len(rays) == 11202
    missed = int((twin.cast(v, t, rays)[1] < 0).sum())
    naive = int((twin.cast(v, t, rays, test='naive')[1] < 0).sum())
    host = F.host_cast(v, t, rays)
    print('missed: watertight %d, naive %d, host %d' % (missed, naive, int((host[1] < 0).sum())))
    assert missed == 0 and (host[1] >= 0).all() and host[4].all()
    assert naive > 0
    tree = F.host_tree('icosphere')
    assert F.same(F.host_cast(v, t, rays, tree=(tree[0], tree[1]))[1], host[1])


# ---- the twin against independent bounds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['one', 'edge_pair', 'fan_100', 'icosphere'])
def test_twin_closest_point_between_two_grid_bounds(name):
    """The minimum over a 64 x 64 barycentric grid of every triangle bounds the distance from above; that minimum less one grid step of the
    longest edge bounds it from below."""
    v, t = CASES[name]
    q = F.queries(name)
    q = q[np.isfinite(q).all(1)]
    dist = twin.closest(v, t, q)[1]
    i, j = np.meshgrid(np.arange(65), np.arange(65), indexing='ij')
    keep = i + j <= 64
    wb, wc = i[keep] / 64.0, j[keep] / 64.0
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    grid = a[:, None] + wb[None, :, None] * (b - a)[:, None] + wc[None, :, None] * (c - a)[:, None]
    step = max(np.linalg.norm(b - a, axis=1).max(), np.linalg.norm(c - a, axis=1).max(), np.linalg.norm(c - b, axis=1).max()) / 64.0
    for k in range(len(q)):
        upper = np.sqrt(((grid - q[k]) ** 2).sum(-1).min())
        slack = 64 * EPS * (np.abs(q[k]).max() + np.abs(v).max())
        assert upper - step - slack <= dist[k] <= upper + slack, (name, k, dist[k], upper, step)


@pytest.mark.parametrize('name', ['one', 'fan_100', 'cube', 'icosphere', 'mc_sphere'])
def test_hit_point_agrees_with_the_point_of_the_uvs(name):
    """o + t d against a + u (b - a) + v (c - a).  The allowance is derived, not guessed: with S the largest sheared coordinate and Z the
    largest depth of the hit triangle, each of U, V, W carries 3 roundings of products of size S^2, so a weight is off by at most
    6 eps S^2 / |det| and t by at most three times that times Z; both points add a handful of roundings of their own coordinates."""
    v, t = CASES[name]
    rays = F.rays(name)
    t_hit, ids, uvs, _ = twin.cast(v, t, rays)
    frame = twin.ray_frame(rays)
    worst = 0.0
    for r in np.nonzero(ids >= 0)[0]:
        o, d = rays[r, :3], rays[r, 3:]
        a, b, c = v[t[ids[r]]]
        sheared = [twin._sheared(p[None], o[None], tuple(x[r:r + 1] for x in frame)) for p in (a, b, c)]
        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = [[float(x[0, 0]) for x in s] for s in sheared]
        S, Z = max(abs(x) for x in (ax, ay, bx, by, cx, cy)), max(abs(az), abs(bz), abs(cz))
        det = ((cx * by - cy * bx) + (ax * cy - ay * cx)) + (bx * ay - by * ax)
        weight = 6 * EPS * S * S / abs(det)
        edges = np.abs(b - a).max() + np.abs(c - a).max()
        allowance = 4 * (weight * edges + 3 * weight * Z * np.abs(d).max()) + 16 * EPS * (np.abs(o).max() + abs(t_hit[r]) * np.abs(d).max() + np.abs(v).max())
        from_t = o + t_hit[r] * d
        from_uv = a + uvs[r, 0] * (b - a) + uvs[r, 1] * (c - a)
        err = np.abs(from_t - from_uv).max()
        worst = max(worst, err / allowance)
        assert err <= allowance, (name, r, err, allowance)
    print('%s: the worst error is %.3g of its allowance' % (name, worst))


# ---- modelled kernel mistakes -----------------------------------------------------------------------------------------------------------------------
def _walk_differences(name, mistake, rays=None, queries=None, t_max_at_hit=False):
    """how many rays and query points of a case the Python walk answers differently from the brute-force host entries"""
    v, t = CASES[name]
    nodes, counts, _, _, root = _tree(name)
    cast, closest = F.host_brute(name)
    rays = np.arange(len(F.rays(name))) if rays is None else rays
    queries = np.arange(len(F.queries(name))) if queries is None else queries
    wrong = 0
    if t_max_at_hit:
        for r in rays:
            if cast[1][r] >= 0:
                wrong += int(twin.walk_cast(nodes, root, v, t, F.rays(name)[r:r + 1], t_max=cast[0][r], mistake=mistake)[1][0] != cast[1][r])
        return wrong
    t_hit, ids = twin.walk_cast(nodes, root, v, t, F.rays(name)[rays], mistake=mistake)
    wrong += int((ids != cast[1][rays]).sum() + (t_hit.view(np.int64) != cast[0][rays].view(np.int64)).sum())
    _, ids = twin.walk_closest(nodes, root, v, t, F.queries(name)[queries], mistake=mistake)
    return wrong + int((ids != closest[2][queries]).sum())


MISTAKE_CASES = {                                          # where each mistake shows (found by running them all; the test checks it)
    'strict_tie': [('edge_pair', {}), ('cube', {})],
    'skip_on_equal': [('cube', {}), ('edge_pair', {})],
    'no_margin': [('cube', dict(t_max_at_hit=True))],
    'short_trail': [('chain', dict(rays=np.arange(0)))],
}


@pytest.mark.parametrize('mistake', twin.MISTAKES)
def test_each_modelled_mistake_changes_a_named_case(mistake):
    """a strict < in the tie rule; a node skipped on >=; boxes without the margin; a trail one word short for the chain (the walk keeps no
    stack: its memory of waiting children is the trail, so that is what can be too short).  The walk without a mistake changes nothing."""
    for name, how in MISTAKE_CASES[mistake]:
        assert _walk_differences(name, None, **how) == 0, name
        assert _walk_differences(name, mistake, **how) > 0, name


# ---- end to end, measured -----------------------------------------------------------------------------------------------------------------------------
def test_sphere_volume_against_its_mesh():
    """se3_debug_tsdf_raycast_host against se3_debug_mesh_render_host on mesh_fixture's sphere, from the same three views: the largest depth
    difference where both hit and the mesh's normal is within 60 degrees of the ray is 1.0252 voxel lengths over 932 pixels.  The figure is
    the measurement that tests/test_gpu_mesh_query.py doubles; here it is printed and pinned."""
    worst, count, _ = F.end_to_end_host()
    print('sphere: volume against mesh, %.4f voxel lengths over %d pixels' % (worst, count))
    assert count > 500 and abs(worst - F.END_TO_END_HOST_ERROR) < 1e-4
