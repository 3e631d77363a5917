"""Block-sparse TSDF volumes on the device (se3et_amd/tsdf_sparse.py, csrc/tsdf_sparse.hip) against the library's host entries -- the same
text on host memory, which tests/test_tsdf_sparse_cpu.py pins to the numpy twin -- bit for bit, on every case of
tests/tsdf_sparse_fixture.py in both depth dtypes: the touch records, the blocks' states and the clouds; the extraction states written by
hand; a volume alone and as volume 0, 13 and 31 of a batch of 32; storage that grows between two calls; slots past voxel 2^31 of the
storage; from run to run; an object
without frames; a block against TSDFVolumes(1, 16, ...) on the device; the out-of-range refusal; integrate_scene_rgbd against
fuse_depth_frames_sparse, into voxel_downsample_clouds."""
import numpy as np
import pytest
import torch

import tsdf_fixture as U
import tsdf_sparse_fixture as F
import tsdf_sparse_twin as twin

pytestmark = pytest.mark.gpu

CASES = F.cases()
CRAFTED = F.crafted_blocks()
DEV = 'cuda'


def _gpu(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _volumes(c, num_volumes=None):
    from se3et_amd.tsdf_sparse import SparseTSDFVolumes
    return SparseTSDFVolumes(len(c['counts']) if num_volumes is None else num_volumes, c['vl'], c['trunc'], color=c['colors'] is not None,
                             stride=c['stride'], device=DEV)


def _integrate(vol, c, frames=slice(None), counts=None):
    colors = None if c['colors'] is None else _gpu(c['colors'][frames])
    return vol.integrate(_gpu(c['depths'][frames]), c['K'], c['E'][frames], c['counts'] if counts is None else counts, colors, c['depth_scale'],
                         c['depth_trunc'])


def _blocks(vol, volume=None):
    """{coord: state} of the device volumes (of one volume, as volume 0, if given)"""
    coords = vol.block_coords.cpu().numpy()
    t, w, col = (None if x is None else x.cpu().numpy() for x in vol.state())
    assert t.shape == (len(coords), 16, 16, 16) and t.dtype == np.float32 and (col is None or col.shape == (len(coords), 3, 16, 16, 16))
    out = {}
    for i, c in enumerate(coords):
        if volume is None or c[0] == volume:
            out[(0 if volume is not None else int(c[0]),) + tuple(int(b) for b in c[1:])] = dict(tsdf=t[i], weight=w[i], color=None if col is None else col[i])
    return out


def _clouds(vol):
    pts, nrm, col = vol.extract_point_clouds()
    assert all(x.dtype == torch.float64 and x.is_cuda and x.shape[1] == 3 for x in pts + nrm)
    return [(p.cpu().numpy(), n.cpu().numpy(), None if c is None else c.cpu().numpy()) for p, n, c in zip(pts, nrm, col)]


def _with_depth(case, dtype):
    """the case with its depth images as dtype: uint16 becomes float32 exactly; float32 is rounded, a NaN becoming 0"""
    d = case['depths']
    if d.dtype == dtype:
        return case
    with np.errstate(invalid='ignore'):
        d = d.astype(np.float32) if dtype == np.float32 else np.where(np.isnan(d), 0, np.round(d)).astype(np.uint16)
    return dict(case, depths=np.ascontiguousarray(d))


@pytest.mark.parametrize('dtype', (np.uint16, np.float32), ids=['uint16', 'float32'])
@pytest.mark.parametrize('name', list(CASES))
def test_device_equals_the_host_entries(name, dtype):
    from se3et_amd import ops
    c = _with_depth(CASES[name], dtype)
    own = c is CASES[name]                                              # the case's own dtype: the shared host results
    host = F.host_volumes(name) if own else F.HostVolumes(c['colors'] is not None).integrate(c)
    if len(c['depths']):
        keys, frames, bad = ops.stsdf_touch_stack(_gpu(c['depths']), _gpu(c['poses']), c['counts'], c['vl'], c['trunc'], c['stride'])
        hk, hf, hb = F.host_touch(c)
        assert bad == hb == -1 and keys.dtype == torch.int64 and frames.dtype == torch.int32
        assert np.array_equal(keys.cpu().numpy(), hk) and np.array_equal(frames.cpu().numpy(), hf)
    vol = _integrate(_volumes(c), c)
    assert vol.num_blocks == len(host.keys) and np.array_equal(vol.keys.cpu().numpy(), host.keys)
    assert np.array_equal(vol.block_coords.cpu().numpy(), np.array([twin.coord_of(k) for k in host.keys], np.int64).reshape(-1, 4))
    assert F.same_blocks(_blocks(vol), host.blocks())
    assert F.same_clouds(_clouds(vol), F.host_clouds(name) if own else host.extract(c['vl'], len(c['counts'])))


@pytest.mark.parametrize('name', list(CRAFTED))
def test_extraction_of_crafted_blocks_on_the_device(name):
    from se3et_amd.tsdf_sparse import SparseTSDFVolumes
    blocks, vl, color = CRAFTED[name]
    V = 1 + max(c[0] for c in blocks)
    vol = SparseTSDFVolumes(V, vl, 2 * vl, color=color, device=DEV)
    coords = list(blocks)
    slots = vol.allocate_blocks(np.array(coords)).cpu().tolist()
    for coord, slot in zip(coords, slots):
        vol.tsdf[slot].copy_(_gpu(blocks[coord]['tsdf'])), vol.weight[slot].copy_(_gpu(blocks[coord]['weight']))
        if color:
            vol.color[slot].copy_(_gpu(blocks[coord]['color']))
    assert F.same_blocks(_blocks(vol), blocks)
    assert F.same_clouds(_clouds(vol), F.HostVolumes(color).put(blocks).extract(vl, V))


def _batch(position, n=32):
    """n volumes: the sphere's three clean frames at `position`, the mangled ones (the same blocks, other numbers) everywhere else"""
    own, other = CASES['u16_f3_s1'], dict(CASES['mangled_u16_color_s1'], colors=None)
    pick = [own if v == position else other for v in range(n)]
    return dict(own, depths=np.concatenate([p['depths'] for p in pick]), E=np.concatenate([p['E'] for p in pick]), counts=[3] * n)


@pytest.mark.parametrize('position', (0, 13, 31))
def test_a_volume_is_the_same_alone_and_in_a_batch(position):
    alone = _integrate(_volumes(CASES['u16_f3_s1']), CASES['u16_f3_s1'])
    c = _batch(position)
    vol = _integrate(_volumes(c), c)
    coords = vol.block_coords.cpu().numpy()
    assert sorted(set(coords[:, 0].tolist())) == list(range(32))
    assert {tuple(r[1:]) for r in coords if r[0] == position} >= {tuple(r[1:]) for r in coords if r[0] == (position + 1) % 32} != set()
    assert F.same_blocks(_blocks(vol, position), _blocks(alone)) and F.same_blocks(_blocks(alone), F.host_volumes('u16_f3_s1').blocks())
    clouds = _clouds(vol)
    assert len(clouds) == 32 and F.same_clouds([clouds[position]], F.host_clouds('u16_f3_s1'))
    assert not U.same(clouds[position][0], clouds[(position + 1) % 32][0])


def test_storage_that_grows_keeps_earlier_blocks():
    name = 'trunc16_u8color_f2_s4'
    c = CASES[name]
    vol = _integrate(_volumes(c), c, slice(0, 1), [1])
    before, slots, size = _blocks(vol), dict(zip(vol.keys.cpu().tolist(), vol.slots.cpu().tolist())), vol.tsdf.shape[0]
    assert 0 < vol.num_blocks <= size
    far = np.array([[0, 1000 + i, -7, 3] for i in range(2 * size)])
    vol.allocate_blocks(far)                                            # more blocks than the storage held: it grows
    assert vol.tsdf.shape[0] >= 2 * size + len(before) and vol.num_blocks == len(before) + 2 * size
    after = _blocks(vol)
    assert F.same_blocks({k: after[k] for k in before}, before)
    now = dict(zip(vol.keys.cpu().tolist(), vol.slots.cpu().tolist()))
    assert all(now[k] == s for k, s in slots.items()) and vol.keys.cpu().tolist() == sorted(now)
    _integrate(vol, c, slice(1, 2), [1])                                # the second frame, in the grown storage: as one call
    after = _blocks(vol)
    want = F.host_volumes(name).blocks()
    assert F.same_blocks({k: after[k] for k in want}, want)
    assert not any(after[tuple(k)]['weight'].any() for k in far.tolist())
    assert F.same_clouds(_clouds(vol), F.host_clouds(name))


def test_slots_past_2_to_the_31_voxels():
    """2^19 empty blocks with smaller keys take the low slots, so the case's blocks sit past voxel 2^31 of the storage (17 GB of state):
    integration, the neighbour table and extraction address them with 64-bit indices."""
    name = 'u16_f3_s4'
    c = CASES[name]
    host = F.host_volumes(name)
    own = np.array([twin.coord_of(k) for k in host.keys])
    i = np.arange(2 ** 19)
    filler = np.stack([np.zeros_like(i), -2000 - i // 512, i % 512, np.full_like(i, -7)], 1)
    vol = _volumes(c)
    slots = vol.allocate_blocks(np.concatenate([filler, own]))[len(filler):]
    assert int(slots.min()) * 4096 >= 2 ** 31 and vol.tsdf.shape[0] == len(filler) + len(own)
    _integrate(vol, c)
    assert vol.num_blocks == len(filler) + len(own)                     # nothing new: the frames touch the blocks that are there
    at = slots.long()
    got = {tuple(int(b) for b in coord): dict(tsdf=vol.tsdf[s].cpu().numpy(), weight=vol.weight[s].cpu().numpy(), color=None) for coord, s in zip(own, at)}
    assert F.same_blocks(got, host.blocks())
    assert not bool(vol.weight[:len(filler)].any())
    assert F.same_clouds(_clouds(vol), F.host_clouds(name))


@pytest.mark.parametrize('name,cut', [('u8color_f65_s4', 64), ('f32_u8color_f3_s1_31x17', 1)])
def test_a_second_integrate_call_equals_one_call(name, cut):
    c = CASES[name]
    n = len(c['depths'])
    vol = _integrate(_volumes(c), c, slice(0, cut), [cut])
    _integrate(vol, c, slice(cut, None), [n - cut])
    assert F.same_blocks(_blocks(vol), F.host_volumes(name).blocks()) and F.same_clouds(_clouds(vol), F.host_clouds(name))


def test_two_runs_are_bit_identical():
    c = _batch(5, 7)
    runs = []
    for _ in range(2):
        vol = _integrate(_volumes(c), c)
        runs.append((_blocks(vol), _clouds(vol), vol.keys.cpu().tolist(), vol.slots.cpu().tolist()))
    assert F.same_blocks(runs[0][0], runs[1][0]) and F.same_clouds(runs[0][1], runs[1][1]) and runs[0][2:] == runs[1][2:]


def test_an_object_without_frames_gives_empty_clouds():
    from se3et_amd.tsdf_sparse import SparseTSDFVolumes, fuse_depth_frames_sparse
    for color in (False, True):
        vol = SparseTSDFVolumes(2, 0.01, 0.04, color=color, device=DEV)
        pts, nrm, col = vol.extract_point_clouds()
        assert vol.num_blocks == 0 and tuple(vol.block_coords.shape) == (0, 4) and len(pts) == len(nrm) == len(col) == 2
        for v in range(2):
            assert tuple(pts[v].shape) == tuple(nrm[v].shape) == (0, 3) and pts[v].dtype == torch.float64 and pts[v].is_cuda
            assert (col[v] is None) if not color else (tuple(col[v].shape) == (0, 3) and col[v].is_cuda)
    c = CASES['f0']
    vol = _integrate(_volumes(c), c)
    assert vol.num_blocks == 0 and _clouds(vol)[0][0].shape == (0, 3)
    blank = dict(CASES['u16_f3_s4'], depths=np.zeros_like(CASES['u16_f3_s4']['depths']))          # frames that see nothing
    assert _integrate(_volumes(blank), blank).num_blocks == 0
    assert fuse_depth_frames_sparse([], [1.0, 1.0, 0.0, 0.0], [], 0.01, 0.04, device=DEV) == ([], [], None)


@pytest.mark.parametrize('name', ['u16_f3_s4', 'f32_u8color_f3_s1_31x17', 'apart_u16_f2_s1'])
def test_a_block_equals_a_uniform_volume_on_the_device(name):
    from se3et_amd.tsdf import TSDFVolumes
    c = CASES[name]
    got = _blocks(_integrate(_volumes(c), c))
    lists = twin.frame_lists(F.twin_records(name))
    assert len(got) == len(lists) > 0
    for key, frames in lists.items():
        coord = twin.coord_of(key)
        one = TSDFVolumes(1, 16, c['vl'], c['trunc'], origins=np.array([[16 * c['vl'] * b for b in coord[1:]]]), color=c['colors'] is not None, device=DEV)
        one.integrate(_gpu(c['depths'][frames]), c['K'], c['E'][frames], None, None if c['colors'] is None else _gpu(c['colors'][frames]))
        want = dict(tsdf=one.tsdf[0].cpu().numpy(), weight=one.weight[0].cpu().numpy(), color=None if one.color is None else one.color[0].cpu().numpy())
        assert F.same_blocks({coord: got[coord]}, {coord: want}), coord


def test_an_out_of_range_block_is_refused_before_any_state_changes():
    c = CASES['face_quarter']
    vol = _integrate(_volumes(c), c)
    before, keys, size = _blocks(vol), vol.keys.clone(), vol.tsdf.shape[0]
    bad = F.range_case(131071.8)
    with pytest.raises(ValueError, match='frame 1 touches a block coordinate outside'):
        _integrate(vol, bad)
    assert torch.equal(vol.keys, keys) and vol.tsdf.shape[0] == size and F.same_blocks(_blocks(vol), before)
    near = F.range_case(131071.7)
    assert int(_integrate(vol, near).block_coords[:, 1].max()) == 2 ** 18 - 1


def test_integrate_scene_rgbd_equals_fusing_the_concatenated_frames():
    from se3et_amd.scan_prep import voxel_downsample_clouds
    from se3et_amd.tsdf_sparse import fuse_depth_frames_sparse, integrate_scene_rgbd, rigid_inverse
    c = CASES['f32_u8color_f3_s1_31x17']
    poses = _gpu(twin.camera_poses(c['E']))                             # camera to world, as make_fragments_rgbd returns them
    assert np.abs(rigid_inverse(poses).cpu().numpy() - c['E']).max() < 1e-12
    cut = 2
    depths, colors = [_gpu(c['depths'][:cut]), _gpu(c['depths'][cut:])], [_gpu(c['colors'][:cut]), _gpu(c['colors'][cut:])]
    eye = torch.eye(4, dtype=torch.float64, device=DEV).repeat(2, 1, 1)
    pts, nrm, col, volume = integrate_scene_rgbd(depths, colors, c['K'], [poses[:cut], poses[cut:]], eye, c['vl'], c['trunc'], stride=c['stride'])
    want = fuse_depth_frames_sparse([_gpu(c['depths'])], c['K'], [rigid_inverse(poses)], c['vl'], c['trunc'], [_gpu(c['colors'])], stride=c['stride'])
    assert volume.num_blocks > 0 and len(pts) > 100 and all(x.dtype == torch.float64 and x.is_cuda for x in (pts, nrm, col))
    assert all(U.same(a.cpu().numpy(), b[0].cpu().numpy()) for a, b in zip((pts, nrm, col), want))
    # a fragment pose moves the scene: the cloud follows it
    move = eye.clone()
    move[:, :3, 3] = torch.tensor([0.25, -0.5, 1.0], dtype=torch.float64)
    moved = integrate_scene_rgbd(depths, None, c['K'], [poses[:cut], poses[cut:]], move, c['vl'], c['trunc'], stride=c['stride'])
    assert moved[2] is None and abs(float((moved[0].mean(0) - pts.mean(0) - move[0, :3, 3]).abs().max())) < 2 * c['vl']
    down = voxel_downsample_clouds([pts], 2.5 * c['vl'], [nrm])
    assert len(down[0]) == 1 and 0 < len(down[0][0]) < len(pts)
