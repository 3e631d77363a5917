"""Mesh post-processing on the device (se3et_amd/mesh.py, csrc/mesh_ops.hip) against the library's host entries -- the same text on host
memory, which tests/test_mesh_ops_cpu.py pins to the numpy twin -- bit for bit on every named case of tests/mesh_ops_fixture.py: the
incidence tables, components with their areas, selection, normals, the three smoothing filters with attributes, vertex clustering; alone against in a batch (the empty
mesh in the middle, more meshes than one call takes), two runs against each other, a triangle out of range (and its neighbours in the
batch), and the recipe end to end on a fused sphere with a blob."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_fixture as M
import mesh_ops_fixture as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CASES = F.cases()
NAMES = list(CASES)
SMOOTH_NAMES = ['isolated_vertex', 'one_neighbor', 'fan_100', 'edge_pair_same', 'grid_dyadic', 'strip_4096', 'sphere', 'no_triangles', 'nothing']


def _gpu(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _np(x):
    return None if x is None else x.cpu().numpy()


def _lists(names):
    return [_gpu(CASES[n][0]) for n in names], [_gpu(CASES[n][1]) for n in names]


def _stacked(names):
    from se3et_amd import ops
    v, t = [CASES[n][0] for n in names], [CASES[n][1] for n in names]
    return ops.StackedMeshes(_gpu(np.concatenate(v)), _gpu(np.concatenate(t)), [len(x) for x in v], [len(x) for x in t])


def _stack_offsets(parts):
    """the meshes' row offsets continued end to end"""
    out, base = [], 0
    for off in parts:
        out.append(off[:-1] + base)
        base += int(off[-1])
    return np.concatenate(out + [np.array([base])]).astype(np.int64)


def _same_incidence(inc, names):
    """the stacked tables of the device against the host tables of each mesh, end to end"""
    host = [F.host_case(n, 'incidence') for n in names]
    return (F.same(_np(inc.tri_offsets), _stack_offsets([h[0] for h in host])) and F.same(_np(inc.nbr_offsets), _stack_offsets([h[2] for h in host])) and
            F.same(_np(inc.tri_rows), np.concatenate([h[1] for h in host])) and F.same(_np(inc.nbr_rows), np.concatenate([h[3] for h in host])))


# ---- every case alone ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_incidence_equals_the_host_entry(name):
    from se3et_amd import ops
    assert _same_incidence(ops.mesh_incidence_stack(_stacked([name])), [name])


@pytest.mark.parametrize('name', NAMES)
def test_components_equal_the_host_entry(name):
    from se3et_amd import mesh
    clusters, count, area = mesh.cluster_connected_triangles_meshes(*_lists([name]))
    want = F.host_case(name, 'components')
    assert len(clusters) == len(count) == len(area) == 1
    assert F.same(_np(clusters[0]), want[0]) and F.same(_np(count[0]), want[1]) and F.same(_np(area[0]), want[2])


@pytest.mark.parametrize('name', NAMES)
def test_normals_equal_the_host_entry(name):
    from se3et_amd import mesh
    v, t = _lists([name])
    tn, vn = F.host_case(name, 'normals')
    assert F.same(_np(mesh.triangle_normals_meshes(v, t)[0]), tn) and F.same(_np(mesh.vertex_normals_meshes(v, t)[0]), vn)
    assert F.same(_np(mesh.triangle_normals_meshes(v, t, normalized=False)[0]), F.host_case(name, 'normals_raw')[0])


@pytest.mark.parametrize('method', F.METHODS)
def test_smoothing_equals_the_host_entry(method):
    """every smoothing case in one batch, positions with normals and colours, three iterations"""
    from se3et_amd import mesh
    v, t = _lists(SMOOTH_NAMES)
    attrs = [F.attributes(len(CASES[n][0]), 7) for n in SMOOTH_NAMES]
    got = mesh.filter_smooth_meshes(v, t, 3, method, normals_list=[_gpu(a[0]) for a in attrs], colors_list=[_gpu(a[1]) for a in attrs])
    zero = mesh.filter_smooth_meshes(v, t, 0, method)
    for i, name in enumerate(SMOOTH_NAMES):
        tri = CASES[name][1]
        for k, values in enumerate((CASES[name][0],) + attrs[i]):
            assert F.same(_np(got[k][i]), F.host_smooth(values, tri, method, 3)), (name, k)
        assert F.same(_np(zero[0][i]), CASES[name][0]) and zero[1] is None and zero[2] is None      # 0 iterations: the input bits


def test_smoothing_parameters_and_the_planar_grid():
    from se3et_amd import mesh
    v, t = _lists(['grid_dyadic'])
    for method in F.METHODS:
        got = _np(mesh.filter_smooth_meshes(v, t, 1, method, lambda_filter=0.3, mu=-0.2)[0][0])
        assert F.same(got, F.host_smooth(CASES['grid_dyadic'][0], CASES['grid_dyadic'][1], method, 1, 0.3, -0.2))
        ij = np.rint(CASES['grid_dyadic'][0][:, :2] / 0.25).astype(int)
        inner = np.all((ij >= 2) & (ij <= 6), axis=1)
        assert F.same(got[inner], CASES['grid_dyadic'][0][inner])                             # exact: see the CPU test
    with pytest.raises(ValueError):
        mesh.filter_smooth_meshes(v, t, 1, 'gaussian')
    with pytest.raises(ValueError):
        mesh.filter_smooth_meshes(v, t, -1)


@pytest.mark.parametrize('name', ['interleaved', 'fan_100', 'isolated_vertex', 'degenerate', 'strip_4096', 'no_triangles', 'nothing'])
def test_selection_equals_the_host_entry(name):
    from se3et_amd import mesh
    v, t = CASES[name]
    nrm, col = F.attributes(len(v), 3)
    masks = F.keep_masks(len(t), 5)
    B = len(masks)                                                          # the four masks as a batch of four copies of the mesh
    got = mesh.select_triangles_meshes([_gpu(v)] * B, [_gpu(t)] * B, [_gpu(k).bool() if i % 2 else _gpu(k) for i, k in enumerate(masks.values())],
                                       [_gpu(nrm)] * B, [_gpu(col)] * B)
    for i, keep in enumerate(masks.values()):
        want = F.host_select(v, t, keep, nrm, col)
        assert all(F.same(_np(got[k][i]), want[k]) for k in range(5)), (name, i)
    plain = mesh.select_triangles_meshes([_gpu(v)], [_gpu(t)], [_gpu(masks['half'])])
    assert plain[2] is None and plain[3] is None and F.same(_np(plain[0][0]), F.host_select(v, t, masks['half'])[0])


# ---- batches and runs -----------------------------------------------------------------------------------------------------------------------------------
def _everything(names):
    """every output of the front end for the meshes `names`, per mesh, as host arrays"""
    from se3et_amd import mesh
    v, t = _lists(names)
    attrs = [F.attributes(len(CASES[n][0]), 11) for n in names]
    nrm, col = [_gpu(a[0]) for a in attrs], [_gpu(a[1]) for a in attrs]
    keep = [_gpu(F.keep_masks(len(CASES[n][1]), 13)['half']) for n in names]
    out = list(mesh.cluster_connected_triangles_meshes(v, t)) + [mesh.triangle_normals_meshes(v, t), mesh.vertex_normals_meshes(v, t)]
    out += list(mesh.select_triangles_meshes(v, t, keep, nrm, col)) + list(mesh.filter_smooth_meshes(v, t, 2, 'taubin', normals_list=nrm, colors_list=col))
    out += list(mesh.filter_smooth_meshes(v, t, 2, 'simple')[:1]) + list(mesh.remove_small_components_meshes(v, t, keep_largest=1)[:2])
    return [[_np(x) for x in lst] for lst in out]


@pytest.mark.parametrize('names', [['interleaved', 'no_triangles', 'fan_100'], ['sphere', 'nothing', 'strip_4096'], NAMES],
                         ids=['empty_in_the_middle', 'nothing_in_the_middle', 'every_case'])
def test_a_mesh_is_the_same_alone_and_in_a_batch(names):
    from se3et_amd import ops
    assert _same_incidence(ops.mesh_incidence_stack(_stacked(names)), names)
    batch = _everything(names)
    for i, name in enumerate(names):
        alone = _everything([name])
        assert all(F.same(b[i], a[0]) for b, a in zip(batch, alone)), name


def test_two_runs_are_identical():
    names = ['strip_4096', 'sphere', 'fan_100', 'two_tets_one_vertex']
    first, second = _everything(names), _everything(names)
    assert all(F.same(a, b) for x, y in zip(first, second) for a, b in zip(x, y))


def test_more_meshes_than_one_call_takes():
    from se3et_amd import mesh, ops
    names = (['interleaved', 'degenerate', 'one_neighbor', 'isolated_vertex', 'no_triangles'] * 8)[:ops.PAIR_MAX_PAIRS + 5]
    v, t = _lists(names)
    clusters, count, area = mesh.cluster_connected_triangles_meshes(v, t)
    smooth = mesh.filter_smooth_meshes(v, t, 2, 'laplacian')[0]
    normals = mesh.vertex_normals_meshes(v, t)
    assert len(clusters) == len(smooth) == len(normals) == len(names)
    for i, name in enumerate(names):
        want = F.host_case(name, 'components')
        assert F.same(_np(clusters[i]), want[0]) and F.same(_np(count[i]), want[1]) and F.same(_np(area[i]), want[2]), i
        assert F.same(_np(smooth[i]), F.host_smooth(CASES[name][0], CASES[name][1], 'laplacian', 2)), i
        assert F.same(_np(normals[i]), F.host_case(name, 'normals')[1]), i


def test_remove_small_components():
    from se3et_amd import mesh
    v, t = _lists(['two_tets_one_vertex', 'interleaved', 'degenerate'])
    # keep_largest: 4 triangles against 4: the tie goes to the lower cluster; 3 against 2; 2 against 1
    got = mesh.remove_small_components_meshes(v, t, keep_largest=1)
    assert [_np(x).tolist() for x in got[1]] == [CASES['two_tets_one_vertex'][1][:4].tolist(), [[0, 1, 2], [2, 1, 3], [3, 1, 4]], [[0, 0, 1], [0, 1, 2]]]
    assert _np(got[4][1]).tolist() == [0, 1, 2, -1, -1, -1, 3, -1, 4] and got[2] is None
    got = mesh.remove_small_components_meshes(v, t, min_triangles=3)
    assert [len(x) for x in got[1]] == [8, 3, 0] and len(got[0][2]) == 0
    area = [_np(a) for a in mesh.cluster_connected_triangles_meshes(v, t)[2]]
    got = mesh.remove_small_components_meshes(v, t, min_area=float(area[1].max()))
    assert len(got[1][1]) == (3 if area[1][0] >= area[1][1] else 2)
    with pytest.raises(ValueError):
        mesh.remove_small_components_meshes(v, t)


# ---- bad input --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(F.BAD))
def test_a_triangle_out_of_range_raises(name):
    """A status check, not a fault: the kernels skip the triangle (mo_triangle is their only way to a vertex number), the status word of the
    mesh comes back with the counts, the front end raises ValueError, and the tables of the other meshes of the batch are what they are alone."""
    from se3et_amd import _lib, mesh, ops
    bv, bt = F.BAD[name]
    good = ['fan_100', 'interleaved']
    v = [_gpu(CASES[good[0]][0]), _gpu(bv), _gpu(CASES[good[1]][0])]
    t = [_gpu(CASES[good[0]][1]), _gpu(bt), _gpu(CASES[good[1]][1])]
    for call in (lambda: mesh.triangle_normals_meshes(v, t), lambda: mesh.vertex_normals_meshes(v, t), lambda: mesh.cluster_connected_triangles_meshes(v, t),
                 lambda: mesh.filter_smooth_meshes(v, t, 1), lambda: mesh.select_triangles_meshes(v, t, [torch.ones(len(x), dtype=torch.bool, device=DEV) for x in t]),
                 lambda: mesh.postprocess_triangle_meshes(v, t, smooth_iterations=1)):
        with pytest.raises(ValueError, match='mesh 1'):
            call()
    # the count pass of the incidence entry itself: status 0, 1, 0, and the good meshes' rows untouched by their neighbour
    S = ops.StackedMeshes(torch.cat(v), torch.cat(t), [len(x) for x in v], [len(x) for x in t])
    toff = torch.empty((S.N + 1,), dtype=torch.int64, device=DEV)
    noff = torch.empty((S.N + 1,), dtype=torch.int64, device=DEV)
    trows = torch.full((3 * S.M,), -1, dtype=torch.int32, device=DEV)
    counts = S.counts()
    nbytes = _lib.lib().se3_mesh_incidence_workspace_bytes(S.N)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().se3_mesh_incidence_stack(S.triangles.data_ptr(), S.voff, S.toff, S.B, toff.data_ptr(), trows.data_ptr(), noff.data_ptr(), 0, None,
                                                   counts.data_ptr(), ws.data_ptr(), nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               'se3_mesh_incidence_stack')
    rows = counts.cpu().tolist()
    assert [r[0] for r in rows] == [0, 1, 0]
    toff, trows = _np(toff), _np(trows)
    first, bad, last = F.host_case(good[0], 'incidence'), F.host_incidence(bt, len(bv)), F.host_case(good[1], 'incidence')
    assert [r[1] for r in rows] == [len(first[1]), len(bad[1]), len(last[1])] and [r[2] for r in rows] == [len(first[3]), len(bad[3]), len(last[3])]
    assert F.same(trows[:rows[0][1]], first[1]) and F.same(trows[rows[0][1]:rows[0][1] + rows[1][1]], bad[1])
    assert F.same(trows[rows[0][1] + rows[1][1]:rows[0][1] + rows[1][1] + rows[2][1]], last[1])
    n0 = len(CASES[good[0]][0])
    assert F.same(toff[:n0 + 1], first[0]) and F.same(toff[n0:n0 + len(bv) + 1] - toff[n0], bad[0])


def test_host_tensors_and_wrong_types_are_refused():
    from se3et_amd import mesh
    v, t = _lists(['interleaved'])
    with pytest.raises(RuntimeError):
        mesh.vertex_normals_meshes([v[0].cpu()], t)
    with pytest.raises(RuntimeError):
        mesh.vertex_normals_meshes([v[0].float()], t)
    with pytest.raises(RuntimeError):
        mesh.filter_smooth_meshes(v, [t[0].int()], 1)
    with pytest.raises(RuntimeError):
        mesh.select_triangles_meshes(v, t, [torch.ones(5, dtype=torch.bool)])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------------
def test_fused_sphere_with_a_blob_end_to_end():
    """The analytic sphere of mesh_fixture with a blob of 2^3 voxels in a corner, in a volume on the device: two clusters; keep_largest = 1
    leaves a closed oriented surface; after postprocess_triangle_meshes with five Taubin iterations the sphere error is not larger than
    before plus F.TAUBIN_SPHERE_GROWTH = 0.016 voxel lengths, the growth measured on the twin (0.0168 -> 0.0327,
    tests/test_mesh_ops_cpu.py::test_twin_taubin_on_the_fused_sphere); and the result has the bits of the host entries' pipeline."""
    from se3et_amd import mesh
    from se3et_amd.tsdf import TSDFVolumes
    state, vl, origin = F.fused_state()
    vol = TSDFVolumes(1, state['tsdf'].shape[0], vl, 3 * vl, origins=np.array(origin, np.float64).reshape(1, 3), color=False, device=DEV)
    vol.tsdf.copy_(_gpu(state['tsdf'][None])), vol.weight.copy_(_gpu(state['weight'][None]))
    v, t, n, colors = vol.extract_triangle_meshes()
    hv, ht, _, _ = F.fused_sphere()
    assert F.same(_np(v[0]), hv) and F.same(_np(t[0]), ht)
    clusters, count, area = mesh.cluster_connected_triangles_meshes(v, t)
    assert _np(count[0]).tolist() == [44, 1932] and float(area[0][1]) > 10 * float(area[0][0])
    kv, kt, kn, _, vmap = mesh.remove_small_components_meshes(v, t, n, keep_largest=1)
    assert len(kt[0]) == 1932 and int((vmap[0] >= 0).sum()) == len(kv[0]) == len(kn[0])
    _, forward, backward = mesh.mesh_edge_census(kt[0])
    assert (forward == 1).all() and (backward == 1).all()
    before = M.sphere_error(_np(kv[0]), vl, origin)
    pv, pt, pn, pc = mesh.postprocess_triangle_meshes(v, t, n, colors, min_component_triangles=100, smooth_iterations=5)      # colors: [None]
    after = M.sphere_error(_np(pv[0]), vl, origin)
    print('fused sphere on the device: sphere error before %.4f, after %.4f' % (before, after))
    assert pc is None and F.same(_np(pt[0]), _np(kt[0])) and after <= before + F.TAUBIN_SPHERE_GROWTH
    labels = F.host_components(hv, ht)[0]
    sv, st, _, _, _, _ = F.host_select(hv, ht, (labels == 1).astype(np.uint8))
    smooth = F.host_smooth(sv, st, 'taubin', 5)
    assert F.same(_np(pv[0]), smooth) and F.same(_np(pn[0]), F.host_normals(smooth, st)[1])
    assert np.allclose(np.linalg.norm(_np(pn[0]), axis=1), 1.0, atol=1e-15)


def test_a_bad_mesh_leaves_its_neighbours_alone(monkeypatch):
    """With the front end's ValueError switched off (the status words are still set), every entry runs over the batch good, bad, good: the
    outputs of the good meshes are what they are alone, and the bad mesh's are what the host entries give with the triangle skipped."""
    from se3et_amd import mesh, ops
    status = []

    def read(self, counts, what):
        rows = counts.cpu().tolist()
        status.append([r[0] for r in rows])
        return rows
    monkeypatch.setattr(ops.StackedMeshes, 'read', read)
    bv, bt = F.BAD['bad_n']
    names = ['fan_100', None, 'interleaved']
    hv = [bv if n is None else CASES[n][0] for n in names]
    ht = [bt if n is None else CASES[n][1] for n in names]
    v, t = [_gpu(x) for x in hv], [_gpu(x) for x in ht]
    keep = [F.keep_masks(len(x), 13)['half'] for x in ht]
    clusters, count, area = mesh.cluster_connected_triangles_meshes(v, t)
    tn, vn = mesh.triangle_normals_meshes(v, t), mesh.vertex_normals_meshes(v, t)
    smooth = mesh.filter_smooth_meshes(v, t, 2, 'taubin')[0]
    sel = mesh.select_triangles_meshes(v, t, [_gpu(k) for k in keep])
    simple = mesh.simplify_vertex_clustering_meshes(v, t, 0.3)
    assert status and all(s == [0, 1, 0] for s in status)
    for i in range(3):
        want = F.host_components(hv[i], ht[i])
        assert F.same(_np(clusters[i]), want[0]) and F.same(_np(count[i]), want[1]) and F.same(_np(area[i]), want[2]), i
        hn = F.host_normals(hv[i], ht[i])
        assert F.same(_np(tn[i]), hn[0]) and F.same(_np(vn[i]), hn[1]), i
        assert F.same(_np(smooth[i]), F.host_smooth(hv[i], ht[i], 'taubin', 2)), i
        hs = F.host_select(hv[i], ht[i], keep[i])
        assert F.same(_np(sel[0][i]), hs[0]) and F.same(_np(sel[1][i]), hs[1]) and F.same(_np(sel[4][i]), hs[4]), i
        hc = F.host_cluster(hv[i], ht[i], 0.3)
        assert F.same(_np(simple[0][i]), hc[0]) and F.same(_np(simple[1][i]), hc[1]) and F.same(_np(simple[4][i]), hc[4]), i


# ---- vertex clustering ------------------------------------------------------------------------------------------------------------------------------------
CLUSTER = F.cluster_cases()


def _simplify(names, attributes=True):
    from se3et_amd import mesh
    sizes = {CLUSTER[n][2] for n in names}
    assert len(sizes) == 1                                                  # one voxel size per call
    attrs = [F.attributes(len(CLUSTER[n][0]), 17) for n in names]
    got = mesh.simplify_vertex_clustering_meshes([_gpu(CLUSTER[n][0]) for n in names], [_gpu(CLUSTER[n][1]) for n in names], sizes.pop(),
                                                 [_gpu(a[0]) for a in attrs] if attributes else None, [_gpu(a[1]) for a in attrs] if attributes else None)
    return got, attrs


@pytest.mark.parametrize('name', list(CLUSTER))
def test_vertex_clustering_equals_the_host_entry(name):
    v, t, vs = CLUSTER[name]
    got, attrs = _simplify([name])
    want = F.host_cluster(v, t, vs, *attrs[0])
    assert want[5] == 0 and all(F.same(_np(got[k][0]), want[k]) for k in range(5))
    plain, _ = _simplify([name], attributes=False)
    assert plain[2] is None and plain[3] is None and F.same(_np(plain[0][0]), want[0]) and F.same(_np(plain[1][0]), want[1])


def test_vertex_clustering_alone_in_a_batch_and_twice():
    """the cases of voxel size 0.5 as one batch (a mesh without triangles and one without vertices inside it) against each alone, and again"""
    names = ['on_cell_face', 'no_triangles', 'equal_and_mirror', 'nothing', 'grid', 'collapse_to_edge']
    first, attrs = _simplify(names)
    second, _ = _simplify(names)
    for i, name in enumerate(names):
        want = F.host_cluster(*CLUSTER[name], *attrs[i])
        assert all(F.same(_np(first[k][i]), want[k]) and F.same(_np(second[k][i]), want[k]) for k in range(5)), name


def test_vertex_clustering_refusals():
    from se3et_amd import mesh
    v, t = _lists(['interleaved', 'fan_100'])
    with pytest.raises(ValueError, match='mesh 0, 1 needs 2\\^21 cells'):
        mesh.simplify_vertex_clustering_meshes(v, t, 1e-7)
    for vs in (0.0, -0.5, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='voxel_size'):
            mesh.simplify_vertex_clustering_meshes(v, t, vs)
    bad = v[1].clone()
    bad[5, 2] = float('nan')
    with pytest.raises(ValueError, match='mesh 1 has a vertex or an attribute that is not finite'):
        mesh.simplify_vertex_clustering_meshes([v[0], bad], t, 0.5)
    with pytest.raises(ValueError, match='mesh 0'):
        mesh.simplify_vertex_clustering_meshes([_gpu(F.BAD['bad_minus_one'][0])], [_gpu(F.BAD['bad_minus_one'][1])], 0.5)
    with pytest.raises(RuntimeError):
        mesh.simplify_vertex_clustering_meshes([v[0].cpu()], t[:1], 0.5)


def test_the_recipe_with_simplification():
    """postprocess_triangle_meshes on the fused sphere with a blob: components, five Taubin iterations, clustering at three voxel lengths, fresh
    normals: the bits of the host entries' pipeline, fewer triangles, unit normals"""
    from se3et_amd import mesh
    hv, ht, vl, origin = F.fused_sphere()
    pv, pt, pn, pc = mesh.postprocess_triangle_meshes([_gpu(hv)], [_gpu(ht)], [_gpu(np.zeros_like(hv))], None, min_component_triangles=100,
                                                      smooth_iterations=5, simplify_voxel_size=3 * vl)
    labels = F.host_components(hv, ht)[0]
    sv, st, _, _, _, _ = F.host_select(hv, ht, (labels == 1).astype(np.uint8))
    cv, ct, _, _, _, status = F.host_cluster(F.host_smooth(sv, st, 'taubin', 5), st, 3 * vl)
    assert status == 0 and pc is None and 100 < len(ct) < len(st) // 4
    assert F.same(_np(pv[0]), cv) and F.same(_np(pt[0]), ct) and F.same(_np(pn[0]), F.host_normals(cv, ct)[1])
    assert M.sphere_error(_np(pv[0]), vl, origin) < 1.0                     # still the sphere: within a voxel length
