"""CPU: the se3_debug_mesh_*_host entries (the text the kernels of csrc/mesh_ops.hip run, serially on host memory) against the float64 twin
written from the contract (tests/mesh_ops_twin.py): tables, labels, counts, maps and triangle lists equal, smoothed values, normals and
areas equal bit for bit.  The twin itself is pinned to scipy's connected components, networkx's neighbours and the sphere's area."""
import numpy as np
import pytest

import mesh_fixture
import mesh_ops_fixture as F
import mesh_ops_twin as twin

CASES = F.cases()
NAMES = list(CASES)
# the figures measured on the twin (each test prints its figure again and checks it against the constant)
SPHERE_AREA_ERROR = 0.009          # relative: |twin area - 4 pi r^2| / (4 pi r^2) of the small sphere's mesh
SPHERE_NORMAL_ANGLE = 0.14         # radians: the worst angle of a twin vertex normal from the outward radius


def _csr_equal(rows, offsets, entries):
    off, ent = twin.csr(rows)
    return F.same(off, offsets) and F.same(ent, entries)


# ---- incidence --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_incidence_tables_equal_the_twin(name):
    tri_rows, nbr_rows, status = F.twin_incidence(name)
    toff, trows, noff, nrows, got_status = F.host_case(name, 'incidence')
    assert got_status == status == 0
    assert _csr_equal(tri_rows, toff, trows) and _csr_equal(nbr_rows, noff, nrows)


def test_incidence_edges():
    inc = {name: F.twin_incidence(name) for name in ('isolated_vertex', 'one_neighbor', 'fan_100', 'degenerate', 'edge_pair_same')}
    assert inc['isolated_vertex'][0][4] == [] and inc['isolated_vertex'][1][4] == []
    assert inc['isolated_vertex'][1][1] == [0, 2, 3]                                         # the edge {1, 2} is in two triangles: 2 once
    assert inc['one_neighbor'][0] == [[0], [0]] and inc['one_neighbor'][1] == [[1], [0]]     # (a, a, b): incident to a once
    assert len(inc['fan_100'][0][0]) == 100 and inc['fan_100'][1][0] == list(range(1, 101))   # a valence above one wave
    assert inc['degenerate'][0][0] == [0, 1] and inc['degenerate'][1][3] == []               # (3, 3, 3): incident once, no neighbour
    assert inc['edge_pair_same'][1][0] == [1, 2, 3]


@pytest.mark.parametrize('name', ['fan_100', 'strip_4096', 'sphere', 'degenerate', 'isolated_vertex'])
def test_twin_neighbors_against_networkx(name):
    import networkx as nx
    v, t = CASES[name]
    g = nx.Graph()
    g.add_nodes_from(range(len(v)))
    for a, b, c in t.tolist():
        g.add_edges_from(e for e in ((a, b), (b, c), (c, a)) if e[0] != e[1])
    assert F.twin_incidence(name)[1] == [sorted(g.neighbors(i)) for i in range(len(v))]


# ---- components -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_components_equal_the_twin(name):
    labels, count, area, status = F.twin_components(name)
    got = F.host_case(name, 'components')
    assert got[3] == status == 0
    assert F.same(got[0], labels) and F.same(got[1], count)
    assert F.same(got[2], area), np.abs(got[2] - area).max()                                 # bit for bit: the same reduction tree


def test_component_edges():
    k = {name: len(F.twin_components(name)[1]) for name in NAMES}
    assert k['two_tets_one_vertex'] == 2                                                     # a shared vertex alone does not connect
    assert k['edge_pair_same'] == k['edge_pair_opposite'] == k['three_on_edge'] == k['duplicate_triangle'] == 1
    assert F.twin_components('degenerate')[0].tolist() == [0, 0, 1]                          # (0, 0, 1) still has the edge {0, 1}
    assert F.twin_components('interleaved')[0].tolist() == [0, 1, 0, 1, 0]                   # numbered by the lowest triangle
    assert k['strip_4096'] == 1 and F.twin_components('strip_4096')[1].tolist() == [4096]
    assert k['no_triangles'] == 0 and k['nothing'] == 0 and k['sphere'] == 1


@pytest.mark.parametrize('name', ['two_tets_one_vertex', 'three_on_edge', 'duplicate_triangle', 'degenerate', 'interleaved', 'strip_4096', 'sphere'])
def test_twin_components_against_scipy(name):
    """the edge-adjacency graph built here from sorted edge keys, scipy's components relabelled by their lowest triangle"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    _, t = CASES[name]
    m = len(t)
    edges = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    owner = np.tile(np.arange(m), 3)
    real = edges[:, 0] != edges[:, 1]
    key = np.sort(edges[real], 1) @ np.array([t.max() + 1, 1])
    owner = owner[real]
    order = np.argsort(key, kind='stable')
    key, owner = key[order], owner[order]
    link = key[1:] == key[:-1]                                                               # consecutive owners of one edge: a chain per edge
    graph = coo_matrix((np.ones(link.sum()), (owner[:-1][link], owner[1:][link])), shape=(m, m))
    _, lab = connected_components(graph, directed=False)
    first = {}
    for i, c in enumerate(lab.tolist()):
        first.setdefault(c, len(first))
    assert F.twin_components(name)[0].tolist() == [first[c] for c in lab.tolist()]


def test_twin_area_of_the_sphere():
    """The twin's area of the small sphere's mesh (radius 6.3 voxel lengths) against 4 pi r^2: measured relative error 0.0079 below (the mesh cuts
    the sphere's curvature with chords of about one voxel length: of the order (h / r)^2 / 4 = 0.006); the bound is SPHERE_AREA_ERROR."""
    v, t, vl, _ = F.sphere()
    area = F.twin_components('sphere')[2]
    want = 4 * np.pi * (F.SPHERE_RADIUS * vl) ** 2
    err = abs(float(area[0]) - want) / want
    print('sphere area: twin %.9f, 4 pi r^2 %.9f, relative error %.4f' % (area[0], want, err))
    assert len(area) == 1 and err < SPHERE_AREA_ERROR
    assert abs(float(area[0]) - float(np.sum(twin.triangle_areas(v, t, len(v))))) < 1e-12 * want        # the tree against numpy's pairwise sum


# ---- selection ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['interleaved', 'fan_100', 'isolated_vertex', 'degenerate', 'strip_4096', 'no_triangles', 'nothing'])
def test_selection_equals_the_twin(name):
    v, t = CASES[name]
    nrm, col = F.attributes(len(v), 3)
    for mask, keep in F.keep_masks(len(t), 5).items():
        want = twin.select(v, t, keep, (nrm, col))
        got = F.host_select(v, t, keep, nrm, col)
        assert got[5] == want[4] == 0, mask
        assert F.same(got[0], want[0]) and F.same(got[1], want[1]) and F.same(got[2], want[2][0]) and F.same(got[3], want[2][1]), mask
        assert F.same(got[4], want[3]), mask
        if mask == 'all' and name not in ('isolated_vertex', 'no_triangles'):
            assert F.same(got[0], v) and F.same(got[1], t)
        if mask == 'none':
            assert len(got[0]) == 0 and len(got[1]) == 0 and (got[4] == -1).all()
        if mask == 'one' and len(t):
            assert len(got[1]) == 1 and len(got[0]) == len(set(t[len(t) // 2].tolist()))


def test_selection_shared_vertex():
    """vertex 1 is in a kept and in a dropped triangle: it stays, vertex 3 of the dropped one goes"""
    v, t = CASES['isolated_vertex']
    got = F.host_select(v, t, np.array([1, 0], np.uint8))
    assert got[4].tolist() == [0, 1, 2, -1, -1] and got[1].tolist() == [[0, 1, 2]] and F.same(got[0], v[:3])


# ---- normals --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_normals_equal_the_twin(name):
    v, t = CASES[name]
    tn, vn = F.host_case(name, 'normals')
    assert F.same(tn, twin.triangle_normals(v, t, len(v), True)) and F.same(vn, twin.vertex_normals(v, t, len(v)))
    assert F.same(F.host_case(name, 'normals_raw')[0], twin.triangle_normals(v, t, len(v), False))


def test_normal_edges():
    v, t = CASES['isolated_vertex']
    assert twin.vertex_normals(v, t, len(v))[4].tolist() == [0.0, 0.0, 1.0]                   # an unreferenced vertex
    v, t = CASES['degenerate']
    assert twin.triangle_normals(v, t, len(v), True)[0].tolist() == [0.0, 0.0, 1.0] and not twin.triangle_normals(v, t, len(v), False)[0].any()
    assert F.same(twin.vertex_normals(v, t, len(v))[:3], twin.vertex_normals(v, t[1:2], len(v))[:3])      # a degenerate triangle adds nothing
    assert twin.vertex_normals(v, t, len(v))[3].tolist() == [0.0, 0.0, 1.0]


def test_twin_normals_of_the_sphere():
    """Every vertex normal of the small sphere's mesh against the outward radius through the vertex: the twin's worst angle is 0.1307 rad
    (7.5 degrees: area-weighted facet normals of a surface of radius 6.3 voxel lengths cut by voxel-sized facets); the bound is
    SPHERE_NORMAL_ANGLE."""
    v, t, vl, origin = F.sphere()
    radial = (v - origin) / vl - F.SPHERE_CENTER
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    n = twin.vertex_normals(v, t, len(v))
    angle = np.arccos(np.clip(np.sum(n * radial, 1), -1, 1))
    print('sphere normals: worst angle %.4f rad' % angle.max())
    # marching cubes orders its triangles so that normals point to the positive (outer) side
    assert angle.max() < SPHERE_NORMAL_ANGLE


# ---- smoothing --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', F.METHODS)
@pytest.mark.parametrize('name', ['isolated_vertex', 'one_neighbor', 'fan_100', 'edge_pair_same', 'grid_dyadic', 'strip_4096', 'sphere', 'no_triangles'])
def test_smoothing_equals_the_twin(name, method):
    v, t = CASES[name]
    rows = F.twin_incidence(name)[1]
    for values in (v,) + F.attributes(len(v), 7):
        assert F.same(F.host_smooth(values, t, method, 3, 0.5, -0.53), twin.smooth(values, rows, method, 3, 0.5, -0.53))
    assert F.same(F.host_smooth(v, t, method, 1, 0.3, -0.2), twin.smooth(v, rows, method, 1, 0.3, -0.2))


@pytest.mark.parametrize('method', F.METHODS)
def test_smoothing_edges(method):
    v, t = CASES['isolated_vertex']
    got = F.host_smooth(v, t, method, 4)
    assert F.same(got[4], v[4]) and not F.same(got[0], v[0])                                  # an empty row keeps its value
    assert F.same(F.host_smooth(v, t, method, 0), v)                                          # 0 iterations: the input bits
    v, t = CASES['one_neighbor']
    want = {'simple': (v[0] + v[1]) / 2.0, 'laplacian': v[0] + 0.5 * (v[1] / 1.0 - v[0])}
    want['taubin'] = want['laplacian']
    one = F.host_smooth(v, t, 'laplacian' if method == 'taubin' else method, 1)
    assert F.same(one[0], want[method])


@pytest.mark.parametrize('method', F.METHODS)
def test_interior_of_a_planar_grid_stays(method):
    """spacing 0.25 in the plane z = 0.5: the six neighbours of an interior vertex are symmetric about it and every sum, mean and quotient
    is exact, so one step leaves the interior exactly where it was (the rim moves).  An iteration of taubin is two steps: its second step
    sees the moved rim, so there the vertices two or more rows from the rim stay"""
    v, t = CASES['grid_dyadic']
    got = F.host_smooth(v, t, method, 1)
    ij = np.rint(v[:, :2] / 0.25).astype(int)
    rim = 2 if method == 'taubin' else 1
    interior = np.all((ij >= rim) & (ij <= 8 - rim), axis=1)
    assert interior.sum() == (9 - 2 * rim) ** 2 and F.same(got[interior], v[interior]) and not F.same(got[~interior], v[~interior])
    assert F.same(got[:, 2], v[:, 2])


# ---- bad input --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(F.BAD))
def test_a_triangle_out_of_range_sets_the_status_word(name):
    """the bad triangle is skipped by every entry; the other triangles give what the mesh without it gives"""
    v, t = F.BAD[name]
    n = len(v)
    rows = twin.incidence(t, n)
    rest = twin.incidence(t[[0, 2]], n)                                                       # (its triangle 1 is triangle 2 here)
    assert rows[2] == twin.BAD_TRIANGLE and rows[1] == rest[1] and rows[0] == [[2 * x for x in r] for r in rest[0]]
    toff, trows, noff, nrows, status = F.host_incidence(t, n)
    assert status == twin.BAD_TRIANGLE and _csr_equal(rows[0], toff, trows) and _csr_equal(rows[1], noff, nrows)
    labels, count, area, cstatus = F.host_components(v, t)
    want = twin.components(v, t, n)
    assert cstatus == want[3] == twin.BAD_TRIANGLE and F.same(labels, want[0]) and F.same(count, want[1]) and F.same(area, want[2])
    assert labels.tolist() == [0, 1, 0] and area[1] == 0.0
    got = F.host_select(v, t, np.ones(3, np.uint8))
    assert got[5] == twin.BAD_TRIANGLE and got[1].tolist() == [[0, 1, 2], [2, 1, 3]]
    tn, vn = F.host_normals(v, t)
    assert F.same(tn, twin.triangle_normals(v, t, n)) and F.same(vn, twin.vertex_normals(v, t, n)) and tn[1].tolist() == [0.0, 0.0, 1.0]


def test_argument_checks():
    from se3et_amd import _lib
    L = _lib.lib()
    assert L.se3_debug_mesh_incidence_host(None, 1 << 31, 0, None, None, None, 0, None, None) != 0
    x = np.zeros((1, 3))
    off = np.zeros(2, np.int64)
    assert L.se3_debug_mesh_smooth_host(F._ptr(x), 1, F._ptr(off), None, 7, 1, 0.5, -0.53, F._ptr(x)) != 0 and b'method' in L.se3_last_error()
    assert L.se3_debug_mesh_smooth_host(F._ptr(x), 1, F._ptr(off), None, 0, -1, 0.5, -0.53, F._ptr(x)) != 0
    assert L.se3_mesh_smooth_workspace_bytes(10, 4) == 0 and L.se3_mesh_smooth_workspace_bytes(10, 2) >= 2 * 240
    assert L.se3_mesh_incidence_stack(None, None, None, 1, None, None, None, 0, None, None, None, 0, None) != 0


def test_front_end_refuses_host_tensors():
    import torch
    from se3et_amd import mesh
    v, t = torch.zeros((3, 3), dtype=torch.float64), torch.tensor([[0, 1, 2]])
    for call in (lambda: mesh.vertex_normals_meshes([v], [t]), lambda: mesh.cluster_connected_triangles_meshes([v], [t]),
                 lambda: mesh.filter_smooth_meshes([v], [t], 1), lambda: mesh.select_triangles_meshes([v], [t], [torch.ones(1, dtype=torch.bool)])):
        with pytest.raises(RuntimeError, match='no CPU implementation'):
            call()


# ---- the figure of the end-to-end test ------------------------------------------------------------------------------------------------------------------
def test_twin_taubin_on_the_fused_sphere():
    """The end-to-end case of tests/test_gpu_mesh_ops.py on the twin: the analytic sphere of mesh_fixture with a blob of 2^3 voxels in a
    corner, the blob's component removed, five Taubin iterations.  Measured: clusters of 44 and 1932 triangles, sphere error 0.0168 voxel lengths before, 0.0327 after,
    so the growth that the twin gives is 0.0159; tests/mesh_ops_fixture.py holds it as TAUBIN_SPHERE_GROWTH, which the device must not exceed."""
    v, t, vl, origin = F.fused_sphere()
    labels, count, _, _ = twin.components(v, t, len(v))
    assert count.tolist() == [44, 1932]                                                      # the blob's triangles come first
    big = int(np.argmax(count))
    sv, st, _, _, _ = twin.select(v, t, labels == big)
    before = mesh_fixture.sphere_error(sv, vl, origin)
    after = mesh_fixture.sphere_error(twin.smooth(sv, twin.incidence(st, len(sv))[1], 'taubin', 5), vl, origin)
    print('fused sphere: clusters %s, sphere error before %.4f, after five Taubin iterations %.4f, growth %.4f' % (count.tolist(), before, after, after - before))
    assert before <= 2 * mesh_fixture.SPHERE_TWIN_ERROR
    assert after - before <= F.TAUBIN_SPHERE_GROWTH and F.TAUBIN_SPHERE_GROWTH < 0.0161


# ---- vertex clustering ------------------------------------------------------------------------------------------------------------------------------------
CLUSTER = F.cluster_cases()


@pytest.mark.parametrize('name', list(CLUSTER))
def test_vertex_clustering_equals_the_twin(name):
    v, t, vs = CLUSTER[name]
    nrm, col = F.attributes(len(v), 17)
    want = twin.cluster_vertices(v, t, vs, (nrm, col))
    got = F.host_cluster(v, t, vs, nrm, col)
    assert got[5] == want[4] == 0
    assert F.same(got[1], want[1]) and F.same(got[4], want[3])                               # triangle lists and maps: equal
    assert F.same(got[0], want[0]) and F.same(got[2], want[2][0]) and F.same(got[3], want[2][1])      # means: bit for bit
    plain = F.host_cluster(v, t, vs)
    assert plain[2] is None and plain[3] is None and F.same(plain[0], got[0]) and F.same(plain[1], got[1])


def test_vertex_clustering_edges():
    got = {name: twin.cluster_vertices(*CLUSTER[name]) for name in CLUSTER}
    assert len(got['larger_than_mesh'][0]) == 1 and len(got['larger_than_mesh'][1]) == 0     # voxel_size larger than the mesh
    v, t, vs = CLUSTER['on_cell_face']
    assert (v[1, 0] - (v[:, 0].min() - vs / 2)) / vs == 1.0                                  # exactly on the face: vertex 1 is in cell 1 of x,
    assert got['on_cell_face'][3].tolist() == [0, 2, 1, 4, 3]                                # vertex 2, a hair below it, in cell 0
    v, t, vs = CLUSTER['negative']
    assert v.max() < 0 and len(got['negative'][0]) > 20 and len(got['negative'][1]) > 50
    assert got['collapse_to_edge'][3].tolist() == [0, 0, 1, 1, 2, 2, 3]                      # cells A, B, C, D in (x, y, z) order
    assert got['collapse_to_edge'][1].tolist() == [[0, 1, 2]]                                # (a, a, b) and (b, b, d) became edges
    # (a b c) stays; (b c a) is the same triangle; (a c b) is its mirror image and stays; (d a b) is rotated to (a b d): d -> a -> b kept;
    # (c a b) is (a b c) again
    assert got['equal_and_mirror'][1].tolist() == [[0, 1, 2], [0, 2, 1], [0, 1, 3]]
    assert len(got['grid'][0]) == 25 and np.array_equal(got['grid'][0][:, 2], np.full(25, 0.5))
    assert len(got['no_triangles'][0]) >= 1 and len(got['no_triangles'][1]) == 0 and len(got['nothing'][0]) == 0


def test_vertex_clustering_orders_cells_by_x_then_y_then_z():
    for name in ('sphere', 'negative', 'strip'):
        v, t, vs = CLUSTER[name]
        got = F.host_cluster(v, t, vs)
        cells = np.floor((got[0] - (v.min(0) - vs / 2)) / vs).astype(np.int64)               # a mean lies in its own cell
        assert list(map(tuple, cells.tolist())) == sorted(set(map(tuple, cells.tolist()))) and (got[1][:, 0] < got[1][:, 1]).all() and (got[1][:, 0] < got[1][:, 2]).all()
        assert len(np.unique(got[1], axis=0)) == len(got[1])


def test_vertex_clustering_refusals():
    v, t = CASES['fan_100']
    assert F.host_cluster(v, t, 1e-7)[5] == twin.cluster_vertices(v, t, 1e-7)[4] == twin.TOO_MANY_CELLS
    bad = v.copy()
    bad[3, 1] = np.nan
    assert F.host_cluster(bad, t, 0.5)[5] == twin.cluster_vertices(bad, t, 0.5)[4] == twin.NONFINITE
    nrm = np.zeros_like(v)
    nrm[7, 0] = np.inf
    assert F.host_cluster(v, t, 0.5, nrm)[5] == twin.NONFINITE
    from se3et_amd import _lib
    x, counts = np.zeros((1, 3)), np.zeros(4, np.int64)
    for vs in (0.0, -1.0, np.inf, np.nan):
        assert _lib.lib().se3_debug_mesh_cluster_vertices_host(F._ptr(x), None, None, None, 1, 0, vs, 0, 0, None, None, None, None, F._ptr(counts), F._ptr(counts)) != 0
    bv, bt = F.BAD['bad_n']
    got, want = F.host_cluster(bv, bt, 0.1), twin.cluster_vertices(bv, bt, 0.1)
    assert got[5] == want[4] == twin.BAD_TRIANGLE and F.same(got[1], want[1]) and F.same(got[0], want[0])
