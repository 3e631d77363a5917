"""RGB-D odometry on the device (se3et_amd/odometry.py, csrc/rgbd_odometry.hip) against the library's host entry -- the same text on host
memory, which tests/test_rgbd_odometry_cpu.py pins to the numpy twin -- bit for bit in transforms, status, information and counts: every
case of tests/rgbd_odometry_fixture.py; a pair alone, at positions 0 and 31 of a batch of 32 and through the chunking at 33 pairs; pairs
that share frames against the same pairs on separate copies of the frames; from run to run; a failing pair beside healthy ones;
compute_rgbd_odometry; the recovered motion at 160 x 120; make_fragments_rgbd on the 6-frame orbit against the same public calls composed
by hand and against the ground truth.

The orbit's bound is twice the error of the twin's odometry chained the same way (rgbd_odometry_fixture.ORBIT_TWIN_ERROR: 0.3351 degrees
and 5.797 mm, the worst frame against frame 0, measured on the CPU by tests/test_rgbd_odometry_cpu.py)."""
import numpy as np
import pytest
import torch

import rgbd_odometry_fixture as F
import rgbd_odometry_twin as twin

pytestmark = pytest.mark.gpu

CASES = F.cases()
DEV = 'cuda'
KEYS = ('transforms', 'success', 'status', 'information', 'correspondences')
BASE = '32x24_hybrid_u16_u8rgb_l3'
ORBIT = '32x24_orbit_shared_l2'


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _options(case):
    return dict(method=case['method'], iterations=case['iterations'], max_depth_diff=case['max_depth_diff'], **F.convert_options(case))


def _device(case, **kw):
    from se3et_amd.odometry import rgbd_odometry_pairs
    args = dict(depths=_gpu(case['depths']), colors=_gpu(case['colors']), intrinsics=case['K'], pairs=case['pairs'], init_transforms=case['T0'])
    args.update(_options(case), **kw)
    out = rgbd_odometry_pairs(**args)
    assert all(out[k].is_cuda for k in KEYS) and out['transforms'].dtype == torch.float64 and out['success'].dtype == torch.bool
    assert out['status'].dtype == torch.int32 and out['correspondences'].dtype == torch.int64
    return {k: out[k].cpu().numpy() for k in KEYS}


def _same_pair(got, p, want, q):
    return all(F.same(got[k][p], want[k][q].astype(bool) if k == 'success' else want[k][q]) for k in KEYS)


@pytest.mark.parametrize('name', list(CASES))
def test_device_equals_the_host_entry(name):
    case = CASES[name]
    got, want = _device(case), F.host_results(name)
    print('%s: status %s, correspondences %s' % (name, got['status'].tolist(), got['correspondences'].tolist()))
    for p in range(len(case['pairs'])):
        assert _same_pair(got, p, want, p), p


def _mixed_batch(P):
    """P pairs over six frames: the base case's two, then the orbit's four; the base pair at positions 0, 31 and 32, the orbit's pairs
    between; every pair with the base case's schedule.  Returns the case and, per position, (host results, index) of the same pair alone."""
    base, orbit = CASES[BASE], dict(CASES[ORBIT], iterations=CASES[BASE]['iterations'])
    alone, orbit_alone = F.host_results(BASE), F.host_run(orbit)
    pairs, want = [], []
    for p in range(P):
        if p in (0, 31, 32):
            pairs.append((0, 1)), want.append((alone, 0))
        else:
            q = p % len(orbit['pairs'])
            pairs.append((2 + orbit['pairs'][q][0], 2 + orbit['pairs'][q][1])), want.append((orbit_alone, q))
    case = dict(base, depths=np.concatenate([base['depths'], orbit['depths']]), colors=np.concatenate([base['colors'], orbit['colors']]), pairs=pairs,
                T0=np.tile(np.eye(4), (P, 1, 1)))
    return case, want


@pytest.mark.parametrize('P', [1, 32, 33])
def test_alone_in_a_batch_and_through_the_chunking(P):
    case, want = _mixed_batch(P)
    got = _device(case)
    assert got['transforms'].shape == (P, 4, 4)
    for p, (w, q) in enumerate(want):
        assert _same_pair(got, p, w, q), p


def test_shared_frames_against_separate_copies_and_run_to_run():
    case = CASES[ORBIT]
    shared = _device(case)
    again = _device(case)
    assert all(F.same(shared[k], again[k]) for k in KEYS)
    frames = [f for pair in case['pairs'] for f in pair]
    copies = dict(case, depths=case['depths'][frames], colors=case['colors'][frames], pairs=[(2 * p, 2 * p + 1) for p in range(len(case['pairs']))])
    apart = _device(copies)
    assert all(F.same(shared[k], apart[k]) for k in KEYS)
    assert shared['success'].all()


def test_a_failing_pair_beside_healthy_ones():
    base = CASES[BASE]
    case = dict(base, depths=np.concatenate([base['depths'], np.zeros_like(base['depths'][:1])]),
                colors=np.concatenate([base['colors'], base['colors'][:1]]), pairs=[(0, 1), (2, 1), (0, 1), (0, 2)], T0=np.tile(np.eye(4), (4, 1, 1)))
    got, alone = _device(case), F.host_results(BASE)
    assert _same_pair(got, 0, alone, 0) and _same_pair(got, 2, alone, 0)
    for p in (1, 3):                                                        # an all-zero source, an all-zero target
        assert got['status'][p] == twin.STATUS['empty'] and not got['success'][p] and got['correspondences'][p] == 0
        assert np.array_equal(got['transforms'][p], np.eye(4)) and not got['information'][p].any()
    nan = np.tile(np.eye(4), (4, 1, 1))
    nan[1, 0, 3] = np.nan
    got = _device(dict(case, pairs=[(0, 1)] * 4, T0=nan))
    assert got['status'][1] == twin.STATUS['nonfinite'] and np.array_equal(got['transforms'][1], np.eye(4))
    assert all(_same_pair(got, p, alone, 0) for p in (0, 2, 3))


def test_no_pairs_and_no_information():
    case = CASES[BASE]
    got = _device(dict(case, pairs=np.zeros((0, 2), np.int64), T0=None))
    assert got['transforms'].shape == (0, 4, 4) and got['status'].shape == (0,)
    from se3et_amd.odometry import rgbd_odometry_pairs
    out = rgbd_odometry_pairs(_gpu(case['depths']), _gpu(case['colors']), case['K'], return_information=False, **_options(case))
    assert out['information'] is None and F.same(out['transforms'].cpu().numpy(), F.host_results(BASE)['transforms'])      # the default pairs


def test_compute_rgbd_odometry():
    from se3et_amd.odometry import compute_rgbd_odometry
    case, want = CASES[BASE], F.host_results(BASE)
    ok, T, info = compute_rgbd_odometry(case['colors'][0], case['depths'][0], case['colors'][1], case['depths'][1], case['K'], **_options(case))
    assert ok is True and F.same(T, want['transforms'][0]) and F.same(info, want['information'][0])
    K33 = np.array([[case['K'][0], 0, case['K'][2]], [0, case['K'][1], case['K'][3]], [0, 0, 1]])
    ok, T2, _info = compute_rgbd_odometry(case['colors'][0], case['depths'][0], case['colors'][1], case['depths'][1], K33, np.eye(4), **_options(case))
    assert ok and F.same(T2, T)


@pytest.mark.parametrize('method', ['hybrid', 'color'])
def test_recovered_motion(method):
    case = F.motion_case(method)
    got, want = _device(case), F.host_run(case)
    assert _same_pair(got, 0, want, 0)
    err, bound = F.motion_error(got['transforms'][0], F.truth_of(case, (0, 1))), F.MOTION_TWIN_ERROR[method]
    print('%s: off by %.4f deg %.4f mm (the twin: %r)' % ((method,) + err + (bound,)))
    assert got['success'][0] and err[0] <= 2 * bound[0] and err[1] <= 2 * bound[1]


def test_make_fragments_rgbd_on_the_orbit():
    from se3et_amd.odometry import _rigid_inverses, make_fragments_rgbd, rgbd_odometry_pairs
    from se3et_amd.pose_graph import optimize_pose_graphs
    from se3et_amd.tsdf import fuse_depth_frames
    case = F.orbit_case()
    d, c, K = _gpu(case['depths']), _gpu(case['colors']), case['K']
    volume = dict(resolution=64, voxel_length=3.2 / 64, sdf_trunc=0.15, origins=np.array([[-1.6, -1.6, 0.4]]))
    out = make_fragments_rgbd([d], [c], K, keyframe_stride=5, **volume)
    # the same public calls, composed by hand (the module's rigid inverse is the only glue): five odometry edges, the loop closure (0, 5)
    # from the chained poses, one graph, one volume
    first = rgbd_odometry_pairs(d, c, K)
    back = _rigid_inverses(first['transforms'])
    X = [torch.eye(4, dtype=torch.float64, device=DEV)]
    for k in range(5):
        X.append(X[-1] @ back[k])
    X = torch.stack(X)
    second = rgbd_odometry_pairs(d, c, K, [(0, 5)], torch.stack([_rigid_inverses(X[5:6])[0] @ X[0]]))
    assert bool(first['success'].all()) and bool(second['success'].all())
    graph = dict(poses=X, edges=torch.tensor([(i, i + 1) for i in range(5)] + [(0, 5)], device=DEV),
                 transforms=torch.cat([first['transforms'], second['transforms']]), informations=torch.cat([first['information'], second['information']]),
                 uncertain=torch.tensor([0] * 5 + [1], dtype=torch.uint8, device=DEV))
    solved = optimize_pose_graphs([graph], 0, DEV, max_correspondence_distance=0.03, preference_loop_closure=0.1)
    assert F.same(out['poses'][0].cpu().numpy(), solved['poses'][0].cpu().numpy()) and int(out['status'][0]) == int(solved['status'][0]) == 0
    assert out['edges'][0].cpu().tolist() == graph['edges'].cpu().tolist() and out['uncertain'][0].cpu().tolist() == [False] * 5 + [True]
    pts, nrm, col = fuse_depth_frames([d], K, [_rigid_inverses(solved['poses'][0])], colors_list=[c], **volume)
    assert F.same(out['points'][0].cpu().numpy(), pts[0].cpu().numpy()) and F.same(out['normals'][0].cpu().numpy(), nrm[0].cpu().numpy())
    assert F.same(out['colors'][0].cpu().numpy(), col[0].cpu().numpy()) and len(pts[0]) > 1000
    worst = [0.0, 0.0]
    for k, pose in enumerate(out['poses'][0].cpu().numpy()):
        e = F.motion_error(np.linalg.inv(pose), case['poses'][k])
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print('the poses are off by at most %.4f deg %.4f mm (the chained twin: %r); %d points' % (worst[0], worst[1], F.ORBIT_TWIN_ERROR, len(pts[0])))
    assert worst[0] <= 2 * F.ORBIT_TWIN_ERROR[0] and worst[1] <= 2 * F.ORBIT_TWIN_ERROR[1]
    # the surface lies on the scene: the points are on the sphere or on the plane
    p = pts[0].cpu().numpy()
    off = np.minimum(np.abs(np.linalg.norm(p - F.SPHERE_CENTER, axis=1) - F.SPHERE_RADIUS), np.abs(p @ F.PLANE_NORMAL - F.PLANE_OFFSET))
    assert np.median(off) < volume['voxel_length']
