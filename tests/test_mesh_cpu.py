"""Triangle meshes without a GPU: se3_debug_mesh_table, se3_debug_tsdf_mesh_host and se3_debug_stsdf_mesh_host (the text of
csrc/tsdf_mesh_core.h, csrc/mesh_table.h, csrc/tsdf_core.h and csrc/tsdf_sparse_core.h on host memory) against the numpy twin
(tests/mesh_twin.py), bit for bit on vertices, normals, colours and triangles; the triangle table against its rule and its pinned figures;
watertightness of the twin on random sign grids; the analytic sphere, torus and pair of spheres; agreement with the point extraction;
holes where a half-space is unobserved; the PLY writer and the edge census of se3et_amd/mesh.py.

The sphere bound is twice the twin's own worst distance from the analytic sphere (mesh_fixture.SPHERE_TWIN_ERROR, measured on the CPU on
the committed twin: 0.0168 voxel lengths, 968 vertices at a radius of 7.2 voxel lengths)."""
import numpy as np
import pytest

import mesh_fixture as M
import mesh_twin as twin
import tsdf_fixture as U

DENSE = M.dense_states()
SPARSE = M.sparse_states()


def _census(triangles):
    from se3et_amd.mesh import mesh_edge_census
    return mesh_edge_census(triangles)


def _closed(triangles):
    _, forward, backward = _census(triangles)
    return len(forward) > 0 and bool(np.all(forward == 1) and np.all(backward == 1))


def _all_referenced(mesh):
    return len(mesh[0]) == 0 or np.array_equal(np.unique(mesh[1]), np.arange(len(mesh[0])))


def test_limits_and_entries_are_the_headers():
    from se3et_amd import _lib, ops
    assert _lib.ENUMS['se3_mesh_limit'] == {'SE3_MESH_TABLE_WIDTH': twin.WIDTH, 'SE3_MESH_MAX_TRIANGLES': 5}
    assert ops.MESH_LIMITS == {'table_width': 16, 'max_triangles': 5}
    for name in ('se3_tsdf_mesh_stack', 'se3_stsdf_mesh_stack', 'se3_debug_tsdf_mesh_host', 'se3_debug_stsdf_mesh_host', 'se3_debug_mesh_table'):
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES, name


# ---- the table --------------------------------------------------------------------------------------------------------------------------------
def test_the_librarys_table_is_the_rules():
    rows, counts = M.host_table()
    assert rows.dtype == np.int8 and np.array_equal(rows, twin.table())
    assert np.array_equal(counts, (twin.table() >= 0).sum(1) // 3)


def test_the_tables_pinned_figures():
    T = twin.table()
    per_case = (T >= 0).sum(1) // 3
    assert np.bincount(per_case).tolist() == [2, 16, 50, 80, 76, 32] and int(per_case.sum()) == 820 and int(per_case.max()) == 5
    assert per_case[0] == per_case[255] == 0
    assert T[1].tolist() == [0, 3, 8] + [-1] * 13
    assert all(np.all(T[i, 3 * n:] == -1) and np.all(T[i, :3 * n] >= 0) and np.all(T[i] < 12) for i, n in enumerate(per_case))


@pytest.mark.parametrize('case', range(256))
def test_a_cases_triangles_close_over_the_rules_segments(case):
    """the directed triangle edges lying in a cube face are exactly the rule's segments reversed; every interior edge occurs once in each direction"""
    row = twin.table()[case]
    tris = row[row >= 0].reshape(-1, 3).tolist()
    directed = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
    assert len(set(directed)) == len(directed)
    in_face = [e for e in directed if twin.same_face(*e)]
    assert sorted(in_face) == sorted((b, a) for a, b in twin.segments(case))
    interior = [e for e in directed if not twin.same_face(*e)]
    assert all((b, a) in interior for a, b in interior)


def test_random_sign_grids_are_watertight():
    """300 seeds, 5^3 corners, the outer shell positive: every directed edge once and its reverse once"""
    for seed in range(300):
        rng = np.random.default_rng(seed)
        negative = np.zeros((5, 5, 5), bool)
        negative[1:4, 1:4, 1:4] = rng.random((3, 3, 3)) < rng.uniform(0.2, 0.8)
        if not negative.any():
            continue
        order, tri = twin.sign_grid_mesh(negative)
        assert _closed(tri) and np.array_equal(np.unique(tri), np.arange(len(order))), seed


# ---- bit for bit ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(DENSE))
def test_dense_host_entry_equals_the_twin(name):
    got, want = M.host_dense('dense', name), M.twin_mesh('dense', name)
    assert got[1].dtype == np.int64 and M.same_mesh(got, want) and _all_referenced(got)
    assert (len(got[0]) == 0) == (name == 'r9_flat')


@pytest.mark.parametrize('name', list(SPARSE))
def test_sparse_host_entry_equals_the_twin(name):
    blocks, vl, V, color = SPARSE[name]
    got, want = M.host_sparse(name), twin.mesh_sparse(blocks, vl, V, color)
    assert len(got) == len(want) == V and all(M.same_mesh(a, b) and _all_referenced(a) for a, b in zip(got, want))
    assert sum(len(m[1]) for m in got) > 1000


def test_all_256_cases_as_single_cubes():
    for case in range(256):
        s = M.one_cube(case)
        v, t, n, c = M.host_mesh(s, 0.1, np.zeros(3))
        row = twin.table()[case]
        row = row[row >= 0]
        used = sorted(set(row.tolist()), key=lambda e: (tuple(twin.CORNERS[twin.EDGES[e][0]]), twin.AXIS[e]))
        assert len(v) == len(used) and t.reshape(-1).tolist() == [used.index(e) for e in row], case


# ---- analytic states ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, characteristic', [('sphere', 2), ('torus', 0), ('two_spheres', 4)])
def test_analytic_surfaces_are_closed_manifolds(name, characteristic):
    mesh = M.host_dense('analytic', name)
    assert M.same_mesh(mesh, M.twin_mesh('analytic', name))
    assert _closed(mesh[1]) and _all_referenced(mesh) and M.euler(mesh) == characteristic


def test_the_sphere():
    state, vl, origin = M.analytic('sphere')
    v, t, n, _ = M.host_dense('analytic', 'sphere')
    twin_error = M.sphere_error(M.twin_mesh('analytic', 'sphere')[0], vl, origin)
    error = M.sphere_error(v, vl, origin)
    print('sphere: %d vertices, %d triangles, twin error %.4f, host error %.4f voxel lengths' % (len(v), len(t), twin_error, error))
    assert abs(twin_error - M.SPHERE_TWIN_ERROR) < 1e-4
    assert error <= 2 * M.SPHERE_TWIN_ERROR
    centre = origin + vl * np.array(M.SPHERE['center'])
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    normal = np.cross(b - a, c - a)
    outward = (a + b + c) / 3 - centre
    assert np.all((normal * outward).sum(1) > 0)                        # every triangle faces away from the centre, the positive side
    assert np.all((n * (v - centre)).sum(1) > 0)                        # and so does every vertex normal


def test_vertices_are_the_rows_of_the_point_extraction():
    state, vl, origin = M.agreement_state()
    v, t, n, c = M.host_dense('agreement', None)
    p, pn, pc = U.host_extract(state, vl, origin)
    assert len(v) > 100 and U.same(v, p) and U.same(n, pn) and U.same(c, pc) and _closed(t)


def test_an_unobserved_half_space_leaves_a_boundary():
    state, vl, origin = M.analytic('half_observed')
    mesh = M.host_dense('analytic', 'half_observed')
    assert M.same_mesh(mesh, M.twin_mesh('analytic', 'half_observed')) and _all_referenced(mesh)
    edges, forward, backward = _census(mesh[1])
    assert np.all(forward == 1) and np.all(backward <= 1) and 0 < int((backward == 0).sum()) < len(edges) // 4
    local = (mesh[0] - origin) / vl - 0.5                               # in voxel indices: nothing at or beyond the last observed layer, x = 11
    assert local[:, 0].max() <= 11.0 and local[:, 0].max() > 10.0
    full = M.host_dense('analytic', 'sphere')
    assert len(mesh[1]) < len(full[1])
    seen = {tuple(r) for r in np.round(full[0], 9).tolist()}
    assert all(tuple(r) in seen for r in np.round(mesh[0], 9).tolist())


def test_the_exact_zero_is_positive():
    v, t, n, _ = M.host_dense('dense', 'r9_exact_zero')
    state, vl, origin = DENSE['r9_exact_zero']
    # the surface sits on the centres of the voxels that hold 0.0f, as the far end of the edges from z = 2: p1 = (vl / 2 + vl 2) + vl
    assert len(v) == 49 and np.all(v[:, 2] == (vl / 2 + vl * 2) + vl) and len(t) == 72


# ---- se3et_amd/mesh.py ----------------------------------------------------------------------------------------------------------------------------
def _read_ply(path):
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    header = raw[:end].decode('ascii').split('\n')
    counts = {line.split()[1]: int(line.split()[2]) for line in header if line.startswith('element')}
    kinds = {'double': '<f8', 'uchar': 'u1'}
    fields = [(line.split()[2], kinds[line.split()[1]]) for line in header if line.startswith('property') and 'list' not in line]
    rows = np.frombuffer(raw, dtype=fields, count=counts['vertex'], offset=end)
    faces = np.frombuffer(raw, dtype=[('count', 'u1'), ('index', '<i4', (3,))], count=counts['face'], offset=end + rows.nbytes)
    assert end + rows.nbytes + faces.nbytes == len(raw)
    return header, rows, faces


@pytest.mark.parametrize('with_normals, with_colors', [(True, True), (False, False), (True, False)])
def test_ply_round_trip(tmp_path, with_normals, with_colors):
    import torch
    from se3et_amd.mesh import write_triangle_mesh_ply
    v, t, n, c = M.host_dense('dense', 'r11_color_holes')
    path = str(tmp_path / 'mesh.ply')
    write_triangle_mesh_ply(path, torch.from_numpy(v.copy()), torch.from_numpy(t.copy()), n if with_normals else None, c if with_colors else None)
    header, rows, faces = _read_ply(path)
    assert header[:2] == ['ply', 'format binary_little_endian 1.0'] and 'element vertex %d' % len(v) in header and 'element face %d' % len(t) in header
    assert 'property list uchar int vertex_indices' in header
    assert np.array_equal(np.stack([rows['x'], rows['y'], rows['z']], 1), v)
    assert ('nx' in rows.dtype.names) == with_normals and ('red' in rows.dtype.names) == with_colors
    if with_normals:
        assert np.array_equal(np.stack([rows['nx'], rows['ny'], rows['nz']], 1), n)
    if with_colors:
        assert np.array_equal(np.stack([rows['red'], rows['green'], rows['blue']], 1), np.rint(c * 255).astype(np.uint8))
    assert np.all(faces['count'] == 3) and np.array_equal(faces['index'], t)


def test_ply_refusals(tmp_path):
    from se3et_amd.mesh import write_triangle_mesh_ply
    v = np.zeros((3, 3))
    with pytest.raises(ValueError, match='outside'):
        write_triangle_mesh_ply(str(tmp_path / 'a.ply'), v, np.array([[0, 1, 3]]))
    with pytest.raises(ValueError, match='normals'):
        write_triangle_mesh_ply(str(tmp_path / 'a.ply'), v, np.array([[0, 1, 2]]), normals=np.zeros((2, 3)))
    write_triangle_mesh_ply(str(tmp_path / 'empty.ply'), np.zeros((0, 3)), np.zeros((0, 3), np.int64))
    assert _read_ply(str(tmp_path / 'empty.ply'))[1].shape == (0,)


def test_edge_census():
    from se3et_amd.mesh import mesh_edge_census
    edges, forward, backward = mesh_edge_census(np.array([[0, 1, 2], [2, 1, 3], [0, 1, 2]]))
    got = {tuple(e): (int(f), int(b)) for e, f, b in zip(edges.tolist(), forward, backward)}
    assert got == {(0, 1): (2, 0), (1, 2): (2, 1), (2, 0): (2, 0), (2, 1): (1, 2), (1, 3): (1, 0), (3, 2): (1, 0)}
    assert all(len(x) == 0 for x in mesh_edge_census(np.zeros((0, 3), np.int64)))
