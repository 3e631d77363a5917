"""Block-sparse TSDF volumes without a GPU: se3_debug_stsdf_touch_host, se3_debug_stsdf_integrate_host and se3_debug_stsdf_extract_host (the
text of csrc/tsdf_sparse_core.h and csrc/tsdf_core.h on host memory) against the numpy twin (tests/tsdf_sparse_twin.py), bit for bit
(values and sign bits), on every case of tests/tsdf_sparse_fixture.py; the deliberate allocation cases; each block against the uniform
host entry at the block's origin with the block's frame subset; the extraction states written by hand; frames split over two calls; the
rendered sphere; agreement with the uniform volume on one state; the limits and the refusals of se3et_amd/tsdf_sparse.py.

The sphere bound is twice the twin's own worst radial error on that case (tsdf_sparse_fixture.SPHERE_TWIN_ERROR, measured on the CPU on the
committed twin: 0.6550 voxel lengths for the scene at the origin, 0.6607 for the one shifted by (-0.7, -1.2, -0.3); 32 x 24 images, stride
1, three poses each)."""
import numpy as np
import pytest

import tsdf_fixture as U
import tsdf_sparse_fixture as F
import tsdf_sparse_twin as twin

CASES = F.cases()
CRAFTED = F.crafted_blocks()


def _coords(keys):
    return {twin.coord_of(k) for k in keys}


def test_limits_are_the_headers():
    from se3et_amd import _lib, ops
    assert _lib.ENUMS['se3_stsdf_limit'] == {'SE3_STSDF_BLOCK': twin.BLOCK, 'SE3_STSDF_COORD_BITS': twin.COORD_BITS,
                                             'SE3_STSDF_MAX_TRUNC_VOXELS': twin.MAX_TRUNC_VOXELS, 'SE3_STSDF_MAX_STRIDE': twin.MAX_STRIDE,
                                             'SE3_STSDF_POSE_WORDS': twin.POSE_WORDS}
    assert (twin.BLOCK, twin.COORD_BITS, twin.MAX_TRUNC_VOXELS, twin.MAX_STRIDE) == (16, 19, 16, 64)
    assert ops.STSDF_LIMITS == {k[len('SE3_STSDF_'):].lower(): v for k, v in _lib.ENUMS['se3_stsdf_limit'].items()}
    for name in ('se3_stsdf_touch_groups', 'se3_stsdf_touch_stack', 'se3_stsdf_neighbors', 'se3_stsdf_integrate_stack', 'se3_stsdf_extract_stack',
                 'se3_debug_stsdf_touch_host', 'se3_debug_stsdf_integrate_host', 'se3_debug_stsdf_extract_host'):
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES, name
    # the key: 5 bits of volume above 3 x 19 bits, non-negative, ordered as (volume, bx, by, bz)
    coords = [(0, -2 ** 18, 5, 5), (0, -1, 2 ** 18 - 1, -2 ** 18), (0, -1, 2 ** 18 - 1, 7), (0, 0, -2 ** 18, 0), (31, -2 ** 18, 0, 0), (31, 2 ** 18 - 1, 2 ** 18 - 1, 2 ** 18 - 1)]
    keys = [twin.key_of(c) for c in coords]
    assert keys == sorted(keys) and keys[0] >= 0 and keys[-1] < 2 ** 63 and [twin.coord_of(k) for k in keys] == coords
    from se3et_amd.tsdf_sparse import block_keys, key_coords
    assert block_keys(np.array(coords)).tolist() == keys and key_coords(block_keys(np.array(coords))).tolist() == [list(c) for c in coords]
    # the sizes the issue asks for are among the cases
    assert {c['depths'].shape[1:] for c in CASES.values()} == {(24, 32), (17, 31)}
    assert {c['stride'] for c in CASES.values()} >= {1, 4, 5}
    assert {c['depths'].shape[0] for c in CASES.values()} >= {0, 1, 3, U.FRAME_TILE + 1}
    assert {c['depths'].dtype for c in CASES.values()} == {np.dtype(np.uint16), np.dtype(np.float32)}
    assert {None if c['colors'] is None else c['colors'].dtype for c in CASES.values()} == {None, np.dtype(np.uint8), np.dtype(np.float32)}


@pytest.mark.parametrize('name', list(CASES))
def test_touch_sets_against_the_twin(name):
    want = F.twin_records(name)
    keys, frames, bad = F.host_touch(CASES[name])
    print('%s: %d records, %d blocks' % (name, len(want), len({k for k, _ in want})))
    assert bad == -1 and list(zip(keys.tolist(), frames.tolist())) == want
    assert keys.dtype == np.int64 and frames.dtype == np.int32


def test_deliberate_allocation_cases():
    # a pixel exactly on block faces in both directions, with sdf_trunc at 16 voxels: 27 blocks
    keys, _, _ = F.host_touch(CASES['face'])
    assert _coords(keys) == {(0, x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (1, 2, 3)}
    keys, _, _ = F.host_touch(CASES['face_quarter'])
    assert _coords(keys) == {(0, x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (1, 2)}
    # negative block coordinates: floor, not truncation
    shifted = _coords(F.host_touch(CASES['shifted_u16_f3_s4'])[0])
    assert min(c[1] for c in shifted) <= -2 and min(c[2] for c in shifted) <= -3 and min(c[3] for c in shifted) < 0
    q = F.SHIFT[0] + U.SPHERE_CENTER[0] - U.SPHERE_RADIUS                  # the sphere's low side along x lies in block floor(q / 0.5)
    assert min(c[1] for c in shifted) <= int(np.floor(q / 0.5)) < int(q / 0.5)
    # stride: a coarser sampling touches a subset
    assert _coords(F.host_touch(CASES['u16_f3_s4'])[0]) <= _coords(F.host_touch(CASES['u16_f3_s1'])[0])
    assert _coords(k for k, _ in F.twin_records('u16_f3_s1')) == {(0, x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)}          # the eight blocks that meet at the sphere's centre
    # a truncation of a whole block reaches more blocks than one of three voxels
    assert len({k for k, _ in F.twin_records('trunc16_u8color_f2_s4')}) > len({k for k, _ in F.twin_records('u16_f3_s4')})
    # a block touched by frame 0 and not by frame 1, and the other way round
    lists = twin.frame_lists(F.twin_records('apart_u16_f2_s1'))
    assert [0] in lists.values() and [1] in lists.values()
    # 65 frames in one block: one more than a table tile
    assert max(len(v) for v in twin.frame_lists(F.twin_records('u8color_f65_s4')).values()) == U.FRAME_TILE + 1
    # mangled depths touch less, and only through valid pixels; the two volumes of a batch have keys apart
    assert 0 < len(F.twin_records('mangled_f32_s1')) < len(F.twin_records('u16_f3_s1'))
    assert np.isnan(CASES['mangled_f32_s1']['depths']).any() and (CASES['mangled_f32_s1']['depths'] == 3000).any()
    assert {twin.coord_of(k)[0] for k, _ in F.twin_records('two_volumes_s1')} == {0, 1}
    assert F.twin_records('f0') == [] and F.host_volumes('f0').keys.shape == (0,)


def test_out_of_range_blocks_are_reported_with_their_frame():
    keys, frames, bad = F.host_touch(F.range_case(131071.8))
    assert bad == 1 and len(keys) == 0
    with pytest.raises(ValueError, match='frame 1'):
        c = F.range_case(131071.8)
        twin.touch(c['depths'], c['poses'], c['counts'], c['vl'], c['trunc'], c['stride'])
    near = F.range_case(131071.7)
    keys, frames, bad = F.host_touch(near)
    assert bad == -1 and max(c[1] for c in _coords(keys)) == 2 ** 18 - 1
    assert list(zip(keys.tolist(), frames.tolist())) == twin.touch(near['depths'], near['poses'], near['counts'], near['vl'], near['trunc'], near['stride'])


@pytest.mark.parametrize('name', list(CASES))
def test_host_entries_against_the_twin(name):
    c = CASES[name]
    want, got = F.twin_blocks(name), F.host_volumes(name)
    print('%s: %d blocks, %d voxels touched' % (name, len(want), sum(int((s['weight'] > 0).sum()) for s in want.values())))
    assert F.same_blocks(got.blocks(), want)
    assert got.keys.tolist() == sorted(got.keys.tolist()) and sorted(got.slots.tolist()) == list(range(len(got.keys)))
    wp, gp = F.twin_clouds(name), F.host_clouds(name)
    print('   %s points' % [len(p[0]) for p in wp])
    assert F.same_clouds(gp, wp)
    assert all((p[2] is not None) == (c['colors'] is not None) for p in wp)


@pytest.mark.parametrize('name', ['u16_f3_s4', 'f32_u8color_f3_s1_31x17', 'apart_u16_f2_s1', 'u8color_f65_s4', 'shifted_u16_f3_s4', 'mangled_f32_s1'])
def test_a_block_is_a_uniform_volume_of_resolution_16(name):
    c = CASES[name]
    got = F.host_volumes(name).blocks()
    lists = twin.frame_lists(F.twin_records(name))
    assert len(got) == len(lists) > 0
    for key, frames in lists.items():
        coord = twin.coord_of(key)
        case = dict(c, R=16, origin=np.array([16 * c['vl'] * b for b in coord[1:]]))
        want = U.host_integrate(case, frames=frames)
        assert all((want[k] is None and got[coord][k] is None) or U.same(got[coord][k], want[k]) for k in ('tsdf', 'weight', 'color')), coord
    assert any(s['weight'].any() for s in got.values())


def test_the_cases_are_not_empty():
    assert len(F.twin_clouds('u16_f3_s1')[0][0]) > 300 and len(F.twin_clouds('f32_u8color_f3_s1_31x17')[0][0]) > 100
    assert len(F.twin_clouds('shifted_u16_f3_s4')[0][0]) > 50
    assert max(float(s['weight'].max()) for s in F.twin_blocks('u8color_f65_s4').values()) > 40
    both = F.twin_clouds('two_volumes_s1')
    assert len(both) == 2 and len(both[0][0]) > 100 and len(both[1][0]) > 100
    assert all(len(x) == 0 for x in F.twin_clouds('f0')[0][:2])
    col = F.twin_clouds('f32_u8color_f3_s1_31x17')[0][2]
    assert col.min() >= 0 and col.max() <= 1 and col.std() > 0.05
    # points on both sides of the block faces through the sphere's centre, and points whose edge crosses one
    pts = F.twin_clouds('u16_f3_s1')[0][0]
    assert (pts[:, 0] < 0.5).any() and (pts[:, 0] > 0.5).any() and (np.abs(pts - 0.5) < 0.5 / 32).any()


@pytest.mark.parametrize('name', list(CRAFTED))
def test_extraction_of_crafted_blocks(name):
    blocks, vl, color = CRAFTED[name]
    V = 1 + max(c[0] for c in blocks)
    want = twin.extract(blocks, vl, V, color)
    got = F.HostVolumes(color).put(blocks).extract(vl, V)
    print('%s: %s points' % (name, [len(p[0]) for p in want]))
    assert F.same_clouds(got, want)


def test_deliberate_extraction_cases():
    def cloud(name, v=0):
        blocks, vl, color = CRAFTED[name]
        return F.HostVolumes(color).put(blocks).extract(vl, 1 + max(c[0] for c in blocks))[v]
    vl = F.VL
    pts, nrm, _ = cloud('faces')
    assert len(pts) == 3                                                # one edge across a face along each axis, blocks in key order
    cells = pts / vl - 0.5
    assert np.allclose(cells[:, 0], [-16 + 3, -16 + 7, -16 + 15 + 2 / 3]) and np.allclose(cells[:, 1], [4, 15.4, 5]) and np.allclose(cells[:, 2], [32 + 15.2, 32 + 9, 32 + 5])
    pts, nrm, _ = cloud('absent_face')
    assert len(pts) == 1 and abs(pts[0, 0] / vl - 0.5 - 15) < 1e-12     # along z only: the block at x + 1 is absent
    assert nrm[0].tolist() == [0.0, 0.0, -1.0]                          # the stencil reads 0 at x = 16 as it does at the unobserved x = 14
    pa, na, _ = cloud('diagonal_absent')
    pp, npp, _ = cloud('diagonal_present')
    assert len(pa) == len(pp) == 1 and np.array_equal(pa, pp) and na[0, 1] == 0 and npp[0, 1] > 0          # 0.5 x 0.99 x 0.75 from the diagonal block
    full, lone = cloud('local_zero', 1), cloud('local_zero', 0)
    assert len(lone[0]) == 1 and len(full[0]) == 2                      # volume 1 has the edge across the face as well
    assert np.array_equal(lone[0][0], full[0][1]) and not np.array_equal(lone[1][0], full[1][1])          # block b - e read by the stencil
    assert full[2][0].tolist() == [(0.0 * 0.5 + 0.5 * 0.75) / 1.25, (1.0 * 0.5 + 0.5 * 0.75) / 1.25, (0.75 * 0.5 + 0.0 * 0.75) / 1.25]          # colours of both blocks
    assert len(cloud('uniform_at_098')[0]) == 2 and len(cloud('uniform_zeros')[0]) == 2
    pts, nrm, col = cloud('uniform_nan_stencil')
    assert len(pts) == 1 and np.isnan(nrm).any() and np.isfinite(pts).all()
    # no border exclusion: the uniform extraction drops the edge from x = 0 and the one towards x = 12 of 'borders' only through its own border
    assert len(cloud('uniform_borders')[0]) > len(U.host_extract(*U.crafted_states()['borders'])[0])


@pytest.mark.parametrize('name,cut', [('u16_f3_s4', 1), ('u8color_f65_s4', 64), ('f32_u8color_f3_s1_31x17', 2), ('u16_f32color_f1_s5', 0)])
def test_frames_split_over_two_calls(name, cut):
    c = CASES[name]
    n = len(c['depths'])
    v = F.HostVolumes(c['colors'] is not None).integrate(c, slice(0, cut), [cut])
    first = dict(zip(v.keys.tolist(), v.slots.tolist()))
    v.integrate(c, slice(cut, None), [n - cut])
    assert F.same_blocks(v.blocks(), F.host_volumes(name).blocks())
    assert F.same_clouds(v.extract(c['vl'], 1), F.host_clouds(name))
    now = dict(zip(v.keys.tolist(), v.slots.tolist()))                  # a block keeps its slot when later blocks arrive; the keys stay sorted
    assert all(now[k] == s for k, s in first.items()) and v.keys.tolist() == sorted(now)


@pytest.mark.parametrize('name', list(F.SPHERE_TWIN_ERROR))
def test_rendered_sphere(name):
    c = CASES[name]
    twin_error = U.sphere_error(F.twin_clouds(name)[0][0] - (c['center'] - U.SPHERE_CENTER), c['vl'])
    pts, nrm, _ = F.host_clouds(name)[0]
    got = U.sphere_error(pts - (c['center'] - U.SPHERE_CENTER), c['vl'])
    print('%s: %d points, worst radial error %.4f voxel lengths (twin, now: %.4f; recorded: %.4f)' % (name, len(pts), got, twin_error,
                                                                                                       F.SPHERE_TWIN_ERROR[name]))
    assert abs(twin_error - F.SPHERE_TWIN_ERROR[name]) < 5e-4          # the recorded figure is the committed twin's
    assert len(pts) > 100 and got <= 2.0 * F.SPHERE_TWIN_ERROR[name]
    outward = np.einsum('ij,ij->i', nrm, (pts - c['center']) / U.SPHERE_RADIUS)
    print('   normals against the radial direction: median %.3f' % float(np.median(outward)))
    assert np.median(outward) > 0.9


def test_agreement_with_the_uniform_volume():
    """One state as a uniform 32^3 volume and as 2 x 2 x 2 blocks: every uniform point has a sparse point within 1e-9 voxel lengths with
    an equal normal and colour to 1e-9 (only the rounding of vl idx differs: vl (16 + i) against vl 16 + vl i); the sparse points without a
    partner are exactly those that the uniform volume's border excludes."""
    state, blocks = F.agreement_state()
    vl = F.VL
    up, un, uc = U.host_extract(state, vl, np.zeros(3))
    sp, sn, sc = F.HostVolumes(True).put(blocks).extract(vl, 1)[0]
    assert len(up) > 500 and len(sp) > len(up)
    cell = lambda p: tuple(np.round(p / vl * 4).astype(np.int64))       # quarter-voxel cells: partners land in one cell or in adjacent ones
    index = {}
    for i, p in enumerate(sp):
        index.setdefault(cell(p), []).append(i)
    matched = set()
    for p, n, c in zip(up, un, uc):
        near = [i for d in np.ndindex(3, 3, 3) for i in index.get(tuple(np.array(cell(p)) + np.array(d) - 1), [])]
        hits = [i for i in near if np.abs(sp[i] - p).max() <= 1e-9 * vl]
        assert len(hits) == 1, p
        assert np.abs(sn[hits[0]] - n).max() <= 1e-9 and np.abs(sc[hits[0]] - c).max() <= 1e-9
        matched.add(hits[0])
    assert len(matched) == len(up)
    for i, p in enumerate(sp):
        g = p / vl - 0.5
        axis = int(np.argmax(np.abs(g - np.round(g))))                  # the edge's axis: the one coordinate off the voxel centres
        idx = np.round(g).astype(int)
        idx[axis] = int(np.floor(g[axis]))
        border = bool((idx < 1).any() or (idx >= 31).any() or idx[axis] + 1 >= 31)
        assert border == (i not in matched), (p, idx, axis)
    print('agreement: %d uniform points, %d sparse points, %d on the uniform border' % (len(up), len(sp), len(sp) - len(matched)))


def test_refusals_fire_before_any_launch():
    """Every refusal is a ValueError from the Python side's own checks, reached here without a GPU on CPU tensors, where a call that passed
    them ends at the 'no CPU implementation' RuntimeError instead; nothing has been allocated or written by then."""
    import torch
    from se3et_amd import ops
    from se3et_amd.tsdf_sparse import SparseTSDFVolumes, fuse_depth_frames_sparse, integrate_scene_rgbd
    lim = ops.STSDF_LIMITS
    for V in (-1, ops.PAIR_MAX_PAIRS + 1, 1.5):
        with pytest.raises(ValueError, match='num_volumes'):
            SparseTSDFVolumes(V, 0.01, 0.04, device='cpu')
    for trunc in (0.0, -1.0, float('nan'), float('inf'), 0.01 * lim['max_trunc_voxels'] * 1.01):
        with pytest.raises(ValueError, match='sdf_trunc'):
            SparseTSDFVolumes(1, 0.01, trunc, device='cpu')
    with pytest.raises(ValueError, match='voxel_length'):
        SparseTSDFVolumes(1, 0.0, 0.04, device='cpu')
    for stride in (0, lim['max_stride'] + 1, 2.5):
        with pytest.raises(ValueError, match='stride'):
            SparseTSDFVolumes(1, 0.01, 0.04, stride=stride, device='cpu')
    vol, colvol = SparseTSDFVolumes(1, 0.01, 0.04, device='cpu'), SparseTSDFVolumes(1, 0.01, 0.04, color=True, device='cpu')
    two = SparseTSDFVolumes(2, 0.01, 0.04, device='cpu')
    depths, K, E = torch.zeros((3, 24, 32), dtype=torch.float32), [30.0, 30.0, 16.0, 12.0], torch.eye(4, dtype=torch.float64).repeat(3, 1, 1)
    with pytest.raises(ValueError, match='each side'):
        vol.integrate(torch.zeros((1, 1, ops.TSDF_LIMITS['max_image'] + 1), dtype=torch.uint16), K, E[:1])
    bad = E.clone()
    bad[1, 0, 3] = float('nan')
    with pytest.raises(ValueError, match='not finite'):
        vol.integrate(depths, K, bad)
    bad[1, 0, 3] = 1e39                                                 # finite in float64, not in float32
    with pytest.raises(ValueError, match='not finite'):
        vol.integrate(depths, K, bad)
    with pytest.raises(ValueError, match='not finite'):
        vol.integrate(depths, [30.0, float('inf'), 16.0, 12.0], E)
    singular = E.clone()
    singular[2, :3, :3] = torch.tensor([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match='frame 2 cannot be inverted'):
        vol.integrate(depths, K, singular)
    with pytest.raises(ValueError, match='one \\(4, 4\\) transform per pair'):
        vol.integrate(depths, K, E[:2])
    for counts in ([2], [4], [3, 0], [-1]):
        with pytest.raises(ValueError, match='frame_counts'):
            vol.integrate(depths, K, E, frame_counts=counts)
    with pytest.raises(ValueError, match='frame_counts'):
        two.integrate(depths, K, E)                                     # no default for two volumes
    colors = torch.zeros((3, 24, 32, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match='colour'):
        vol.integrate(depths, K, E, colors=colors)
    with pytest.raises(ValueError, match='colour'):
        colvol.integrate(depths, K, E)
    with pytest.raises(ValueError, match='do not match'):
        colvol.integrate(depths, K, E, colors=colors[:, :, :31])
    with pytest.raises(ValueError, match='intrinsics'):
        vol.integrate(depths, [1.0, 2.0, 3.0], E)
    for key in ('depth_scale', 'depth_trunc'):
        with pytest.raises(ValueError, match=key):
            vol.integrate(depths, K, E, **{key: 0.0})
    with pytest.raises(ValueError, match='one entry per scene'):
        fuse_depth_frames_sparse([depths], K, [E, E], 0.01, 0.04, device='cpu')
    with pytest.raises(ValueError, match='one entry per fragment'):
        integrate_scene_rgbd([depths], None, K, [E, E], E[:1], 0.01, 0.04, device='cpu')
    with pytest.raises(ValueError, match='volume in'):
        vol.allocate_blocks([[1, 0, 0, 0]])
    with pytest.raises(ValueError, match='coordinates in'):
        vol.allocate_blocks([[0, 0, 2 ** 18, 0]])
    # what passes every check ends at the device check, not in a kernel: nothing has been allocated or written
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        vol.integrate(depths, K, E)
    for v in (vol, colvol, two):
        assert v.num_blocks == 0 and v.tsdf.shape[0] == 0 and tuple(v.block_coords.shape) == (0, 4)
    # the library refuses on its own as well, through the host entries
    c = CASES['u16_f3_s4']
    for key, value in (('trunc', 0.0), ('trunc', 17 * c['vl']), ('vl', float('nan')), ('stride', 0), ('stride', 65)):
        with pytest.raises(RuntimeError, match='code'):
            F.host_touch({**c, key: value})
