"""Triangle meshes on the device (TSDFVolumes / SparseTSDFVolumes.extract_triangle_meshes, csrc/tsdf_mesh.hip) against the library's host
entries -- the same text on host memory, which tests/test_mesh_cpu.py pins to the numpy twin -- bit for bit on vertices, normals, colours
and triangles: all 256 cube cases as volumes of one cube, in chunks of SE3_PAIR_MAX_PAIRS; resolutions 5, 9, 11 and 260 (a row longer than
one chunk of 256 lanes), an exact 0.0f, a volume without a surface in the middle of a batch, no volumes at all, with and without colour,
alone and in a batch; crafted sparse blocks with the surface through faces, edges and the shared corner of 2 x 2 x 2 blocks, an absent
block, the sparse mesh against the dense one; integrate_scene_rgbd(mesh=True)."""
import numpy as np
import pytest
import torch

import mesh_fixture as M
import mesh_twin as twin
import tsdf_fixture as U
import tsdf_sparse_fixture as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DENSE = M.dense_states()
SPARSE = M.sparse_states()


def _gpu(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _dense_volumes(states, vl, origins):
    from se3et_amd.tsdf import TSDFVolumes
    color = states[0]['color'] is not None
    vol = TSDFVolumes(len(states), states[0]['tsdf'].shape[0], vl, 3 * vl, origins=np.array(origins, np.float64).reshape(-1, 3), color=color, device=DEV)
    vol.tsdf.copy_(_gpu(np.stack([s['tsdf'] for s in states])))
    vol.weight.copy_(_gpu(np.stack([s['weight'] for s in states])))
    if color:
        vol.color.copy_(_gpu(np.stack([s['color'] for s in states])))
    return vol


def _meshes(vol):
    v, t, n, c = vol.extract_triangle_meshes()
    assert all(x.dtype == torch.float64 and x.is_cuda and x.dim() == 2 and x.shape[1] == 3 for x in v + n)
    assert all(x.dtype == torch.int64 and x.is_cuda and x.dim() == 2 and x.shape[1] == 3 for x in t)
    return [(a.cpu().numpy(), b.cpu().numpy(), d.cpu().numpy(), None if e is None else e.cpu().numpy()) for a, b, d, e in zip(v, t, n, c)]


def _sparse_volumes(blocks, vl, V, color):
    from se3et_amd.tsdf_sparse import SparseTSDFVolumes
    vol = SparseTSDFVolumes(V, vl, 2 * vl, color=color, device=DEV)
    coords = list(blocks)
    slots = vol.allocate_blocks(np.array(coords)).cpu().tolist()
    for coord, slot in zip(coords, slots):
        vol.tsdf[slot].copy_(_gpu(blocks[coord]['tsdf'])), vol.weight[slot].copy_(_gpu(blocks[coord]['weight']))
        if color:
            vol.color[slot].copy_(_gpu(blocks[coord]['color']))
    return vol


@pytest.mark.parametrize('color', (False, True), ids=['plain', 'color'])
def test_all_256_cases(color):
    """256 volumes of R = 4, one cube each, through in chunks of SE3_PAIR_MAX_PAIRS: each volume's triangles are its table row"""
    states = [M.one_cube(case, color) for case in range(256)]
    got = _meshes(_dense_volumes(states, 0.1, np.zeros((256, 3))))
    assert len(got) == 256
    T = twin.table()
    for case in range(256):
        row = T[case][T[case] >= 0]
        used = sorted(set(row.tolist()), key=lambda e: (tuple(twin.CORNERS[twin.EDGES[e][0]]), twin.AXIS[e]))
        assert got[case][1].reshape(-1).tolist() == [used.index(e) for e in row], case
        if case in (0, 1, 105, 150, 254, 255):
            assert M.same_mesh(got[case], M.host_mesh(states[case], 0.1, np.zeros(3))), case


@pytest.mark.parametrize('name', list(DENSE))
def test_dense_device_equals_the_host_entry(name):
    state, vl, origin = DENSE[name]
    got = _meshes(_dense_volumes([state], vl, [origin]))
    assert len(got) == 1 and M.same_mesh(got[0], M.host_dense('dense', name))


def test_a_row_longer_than_one_chunk():
    state, vl, origin = M.sheet_state()
    got = _meshes(_dense_volumes([state], vl, [origin]))[0]
    want = M.host_dense('sheet', None)
    assert M.same_mesh(got, want)
    local = want[0][:, 2] / vl - 0.5
    assert local.min() < 254.5 and local.max() > 256.5 and len(want[1]) > 100000    # vertices on both sides of lane 255 / 256 of a row


def test_a_volume_is_the_same_alone_and_in_a_batch():
    """three states of R = 9 in one batch, the one without a surface in the middle; with colour through r11"""
    names = ['r9_holes', 'r9_flat', 'r9_exact_zero']
    states = [DENSE[n] for n in names]
    got = _meshes(_dense_volumes([s[0] for s in states], states[0][1], [s[2] for s in states]))
    assert len(got[1][0]) == 0 and len(got[1][1]) == 0
    for name, mesh, (state, vl, origin) in zip(names, got, states):
        alone = _meshes(_dense_volumes([state], states[0][1], [origin]))[0]
        assert M.same_mesh(mesh, alone)
        if vl == states[0][1]:
            assert M.same_mesh(mesh, M.host_dense('dense', name))
    state, vl, origin = DENSE['r11_color_holes']
    batch = _meshes(_dense_volumes([state] * 33, vl, [origin] * 33))     # one more than a chunk of SE3_PAIR_MAX_PAIRS
    assert all(M.same_mesh(m, M.host_dense('dense', 'r11_color_holes')) for m in batch)


def test_no_volumes_and_no_surface():
    from se3et_amd.tsdf import TSDFVolumes, fuse_depth_frames
    assert TSDFVolumes(0, 8, 0.1, 0.3, device=DEV).extract_triangle_meshes() == ([], [], [], [])
    v, t, n, c = TSDFVolumes(2, 8, 0.1, 0.3, color=True, device=DEV).extract_triangle_meshes()
    assert [tuple(x.shape) for x in v + t + n + c] == [(0, 3)] * 8 and t[0].dtype == torch.int64
    assert fuse_depth_frames([], [1.0, 1.0, 0.0, 0.0], [], 8, 0.1, 0.3, device=DEV, mesh=True) == ([], [], [], None)


def test_two_runs_are_bit_identical():
    state, vl, origin = DENSE['r11_color_holes']
    vol = _dense_volumes([state] * 3, vl, [origin] * 3)
    a, b = _meshes(vol), _meshes(vol)
    assert all(M.same_mesh(x, y) for x, y in zip(a, b))


def test_fuse_depth_frames_mesh_keyword():
    from se3et_amd.tsdf import fuse_depth_frames
    c = U.cases()['sphere16']
    E = np.array(c['table'][:, :12], np.float64).reshape(-1, 3, 4)
    E = np.concatenate([E, np.tile([[[0.0, 0.0, 0.0, 1.0]]], (len(E), 1, 1))], 1)
    args = ([_gpu(c['depths'])], c['table'][0, 12:].astype(np.float64), [E], c['R'], c['vl'], c['trunc'])
    points = fuse_depth_frames(*args, device=DEV)
    assert len(points) == 3                                             # the default return value is as it was
    v, t, n, col = fuse_depth_frames(*args, device=DEV, mesh=True)
    from se3et_amd.mesh import mesh_edge_census
    _, forward, backward = mesh_edge_census(t[0])
    assert col is None and len(t[0]) > 100 and int(t[0].max()) == len(v[0]) - 1 and int((forward + backward).max()) <= 2


# ---- sparse -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(SPARSE))
def test_sparse_device_equals_the_host_entry(name):
    blocks, vl, V, color = SPARSE[name]
    got = _meshes(_sparse_volumes(blocks, vl, V, color))
    want = M.host_sparse(name)
    assert len(got) == V and all(M.same_mesh(a, b) for a, b in zip(got, want))


def test_an_absent_block_leaves_a_hole_and_no_unreferenced_vertex():
    from se3et_amd.mesh import mesh_edge_census
    blocks, vl, V, color = SPARSE['absent_block']
    v, t, n, c = _meshes(_sparse_volumes(blocks, vl, V, color))[0]
    full = M.host_sparse('corner_sphere')[0]
    _, forward, backward = mesh_edge_census(t)
    assert 0 < len(t) < len(full[1]) and np.all(forward == 1) and int((backward == 0).sum()) > 0
    assert np.array_equal(np.unique(t), np.arange(len(v)))


def _sorted_mesh(mesh):
    """vertices in lexicographic order, triangles relabelled and sorted"""
    v, t, n, c = mesh
    order = np.lexsort((v[:, 2], v[:, 1], v[:, 0]))
    new = np.empty_like(order)
    new[order] = np.arange(len(order))
    tri = new[t]
    tri = tri[np.lexsort((tri[:, 2], tri[:, 1], tri[:, 0]))]
    return v[order], tri, n[order], None if c is None else c[order]


def test_the_sparse_mesh_equals_the_dense_mesh():
    """2 x 2 x 2 blocks allocated by hand at the origin against the dense R = 32 volume at the same corner: a small sphere clear of the outer
    shell.  After sorting the vertices and relabelling, the triangles and the colours are equal; points and normals are the same float64
    formulas evaluated in block-local coordinates (contract C, item 4) and in the volume's, so they differ by roundings of 2^-53 of values
    below 1 (1.1e-16 and 8.9e-16 on the host entries): the bound is that of the cloud agreement test of tests/test_tsdf_sparse_cpu.py,
    1e-9 voxel lengths and 1e-9."""
    state = M.small_sphere_state()
    vl = 1.0 / 32
    sparse = _sorted_mesh(_meshes(_sparse_volumes(M.split_blocks(state), vl, 1, True))[0])
    dense = _sorted_mesh(_meshes(_dense_volumes([state], vl, [np.zeros(3)]))[0])
    assert len(dense[1]) > 1000 and sparse[0].shape == dense[0].shape and np.array_equal(sparse[1], dense[1])
    print('sparse against dense: points %.3g, normals %.3g, colours %.3g' % tuple(np.abs(sparse[i] - dense[i]).max() for i in (0, 2, 3)))
    assert np.abs(sparse[0] - dense[0]).max() <= 1e-9 * vl and np.abs(sparse[2] - dense[2]).max() <= 1e-9 and U.same(sparse[3], dense[3])


def test_integrate_scene_rgbd_as_a_mesh():
    from se3et_amd.mesh import mesh_edge_census
    from se3et_amd.tsdf_sparse import integrate_scene_rgbd
    c = F.cases()['f32_u8color_f3_s1_31x17']
    import tsdf_sparse_twin
    poses = _gpu(tsdf_sparse_twin.camera_poses(c['E']))
    depths, colors = [_gpu(c['depths'][:2]), _gpu(c['depths'][2:])], [_gpu(c['colors'][:2]), _gpu(c['colors'][2:])]
    eye = torch.eye(4, dtype=torch.float64, device=DEV).repeat(2, 1, 1)
    args = (depths, colors, c['K'], [poses[:2], poses[2:]], eye, c['vl'], c['trunc'])
    pts, nrm, col, volume = integrate_scene_rgbd(*args, stride=c['stride'])                    # the default return value is as it was
    v, t, n, vc, volume = integrate_scene_rgbd(*args, stride=c['stride'], mesh=True)
    assert all(x.is_cuda for x in (v, t, n, vc)) and t.dtype == torch.int64 and len(t) > 100 and tuple(vc.shape) == tuple(v.shape)
    assert int(t.min()) == 0 and int(t.max()) == len(v) - 1
    edges, forward, backward = mesh_edge_census(t)
    assert int((forward + backward).max()) <= 2                         # no edge is used more than twice
    assert M.same_mesh((v.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy(), vc.cpu().numpy()),
                       M.host_mesh_sparse({k: s for k, s in _blocks(volume).items()}, c['vl'], 1, True)[0])


def _blocks(vol):
    coords = vol.block_coords.cpu().numpy()
    t, w, col = (None if x is None else x.cpu().numpy() for x in vol.state())
    return {tuple(int(b) for b in c): dict(tsdf=t[i], weight=w[i], color=None if col is None else col[i]) for i, c in enumerate(coords)}
