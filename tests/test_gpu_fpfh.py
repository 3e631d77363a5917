"""FPFH on the device (se3et_amd/fpfh.py, csrc/fpfh.hip) against the library's host entry -- the same text on host memory, which
tests/test_fpfh_cpu.py pins to the numpy twin -- bit for bit, for SPFH and FPFH, float32 and float64 inputs, and the radius, k-nearest and
hybrid searches.  R = 4 is the rows-per-workgroup of both kernels (one wave per row): the clouds n3, n4, n5 of the fixture have R - 1, R
and R + 1 rows; `clusters` has rows with 0, 1, 63, 64, 65 and 300 neighbours (the lane stride of 64 and the tile of the neighbour loop)."""
import numpy as np
import pytest
import torch

import fpfh_fixture as F
import fpfh_twin as twin

pytestmark = pytest.mark.gpu

EDGES = F.edge_clouds()
DTYPES = (np.float64, np.float32)
DEV = 'cuda'


def _gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _device(points, normals, radius, max_nn):
    from se3et_amd.fpfh import compute_fpfh_clouds, spfh_clouds
    p, nr = [_gpu(points)], [_gpu(normals)]
    spfh, fpfh = spfh_clouds(p, nr, radius, max_nn), compute_fpfh_clouds(p, nr, radius, max_nn)
    for out in (spfh, fpfh):
        assert len(out) == 1 and out[0].dtype == torch.float64 and out[0].is_cuda and tuple(out[0].shape) == (len(points), twin.DIM)
    return spfh[0].cpu().numpy(), fpfh[0].cpu().numpy()


def _assert_equals_host(points, normals, radius, max_nn):
    want_s, want_f, status = F.host_fpfh(points, normals, radius, max_nn)
    assert status == 0
    got_s, got_f = _device(points, normals, radius, max_nn)
    assert np.array_equal(got_s, want_s)
    assert np.array_equal(got_f, want_f)


@pytest.mark.parametrize('dtype', DTYPES, ids=['float64', 'float32'])
@pytest.mark.parametrize('case', list(F.CASES))
def test_device_equals_the_host_entry(case, dtype):
    name, radius, max_nn = F.CASES[case]
    p, nr = (a.astype(dtype) for a in F.cloud(name))
    _assert_equals_host(p, nr, radius, max_nn)


@pytest.mark.parametrize('dtype', DTYPES, ids=['float64', 'float32'])
@pytest.mark.parametrize('name', list(EDGES))
def test_device_equals_the_host_entry_on_the_edges(name, dtype):
    """Every edge of the CPU file: the exact pairs, rows with 0 .. 300 neighbours, R - 1, R, R + 1 rows, n = 0, 1, 2, K = 1, 2, 64, n < K,
    duplicates."""
    p, nr, radius, max_nn = EDGES[name]
    _assert_equals_host(p.astype(dtype), nr.astype(dtype), radius, max_nn)


@pytest.mark.parametrize('name', list(F.PAIR_EDGES))
def test_pair_edges_have_their_pinned_bins(name):
    p, nr, (bt, b1, b2) = F.pair_edge(name)
    want = np.zeros(twin.DIM)
    want[[bt, twin.BINS + b1, 2 * twin.BINS + b2]] = 100.0
    spfh, fpfh = _device(p, nr, F.PAIR_RADIUS, None)
    assert np.array_equal(spfh[0], want)
    if name == 'duplicate':
        assert np.array_equal(fpfh, spfh)


def _batch():
    """33 small clouds (the chunk boundary at 32), float32 and float64 side by side, all searched at radius 0.25: the edge clouds of the
    radius search, with dense beside isolated, n = 0, 1, 2 and R - 1, R, R + 1 rows among them."""
    names = [n for n, v in EDGES.items() if v[3] is None and v[2] == 0.25]
    g = np.random.default_rng(3)
    clouds = [(EDGES[n][0], EDGES[n][1]) for n in names]
    while len(clouds) < 33:
        n = 20 + 7 * len(clouds)
        clouds.append((g.uniform(0, 0.6, (n, 3)), F._unit(g, n)))
    assert len(clouds) == 33 and 'dense' in names and names.index('isolated') == names.index('dense') + 1
    return [(p.astype(np.float32 if i % 2 else np.float64), nr.astype(np.float32 if i % 3 == 0 else np.float64)) for i, (p, nr) in enumerate(clouds)]


def test_batch_of_33_equals_the_single_calls():
    from se3et_amd.fpfh import compute_fpfh_clouds, spfh_clouds
    clouds = _batch()
    pts, nrs = [_gpu(p) for p, _ in clouds], [_gpu(nr) for _, nr in clouds]
    first, second = compute_fpfh_clouds(pts, nrs, 0.25), compute_fpfh_clouds(pts, nrs, 0.25)
    spfh = spfh_clouds(pts, nrs, 0.25)
    rounded = compute_fpfh_clouds(pts, nrs, 0.25, dtype=torch.float32)
    assert len(first) == 33
    for i, (p, nr) in enumerate(clouds):
        assert torch.equal(first[i], second[i]), i                                           # two runs are identical
        assert rounded[i].dtype == torch.float32 and torch.equal(rounded[i], first[i].to(torch.float32)), i     # rounded once
        assert torch.equal(first[i], compute_fpfh_clouds([pts[i]], [nrs[i]], 0.25)[0]), i     # alone
        want_s, want_f, status = F.host_fpfh(p, nr, 0.25)
        assert status == 0 and np.array_equal(spfh[i].cpu().numpy(), want_s) and np.array_equal(first[i].cpu().numpy(), want_f), i
    assert compute_fpfh_clouds([], [], 0.25) == []


@pytest.mark.parametrize('mode', ['radius', 'knn', 'hybrid'])
def test_fixture_clouds_in_one_call_and_under_a_small_pair_budget(mode, monkeypatch):
    """All fixture clouds in one call equal the single calls; a pair budget far below the list's size cuts the chunk into row slices (both
    passes then search again) and changes no bit."""
    from se3et_amd import fpfh
    radius, max_nn = {'radius': (0.25, None), 'knn': (None, 33), 'hybrid': (0.2, 48)}[mode]
    clouds = [F.cloud(n) for n in ('surface', 'micro', 'c1_2k')]
    pts, nrs = [_gpu(p) for p, _ in clouds], [_gpu(nr) for _, nr in clouds]
    whole = fpfh.compute_fpfh_clouds(pts, nrs, radius, max_nn)
    whole_s = fpfh.spfh_clouds(pts, nrs, radius, max_nn)
    monkeypatch.setattr(fpfh, 'PAIR_BUDGET', 20000)
    cut = fpfh.compute_fpfh_clouds(pts, nrs, radius, max_nn)
    cut_s = fpfh.spfh_clouds(pts, nrs, radius, max_nn)
    for i, (p, nr) in enumerate(clouds):
        want_s, want_f, _ = F.host_fpfh(p, nr, radius, max_nn)
        assert np.array_equal(whole[i].cpu().numpy(), want_f) and np.array_equal(whole_s[i].cpu().numpy(), want_s), i
        assert torch.equal(cut[i], whole[i]) and torch.equal(cut_s[i], whole_s[i]), i


def test_numpy_wrapper():
    from se3et_amd.fpfh import compute_fpfh_feature
    p, nr = F.cloud('micro')
    got = compute_fpfh_feature(p, nr, radius=0.12)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, F.host_fpfh(p, nr, 0.12)[1])


def test_refusals():
    from se3et_amd import ops
    from se3et_amd.fpfh import compute_fpfh_clouds, spfh_clouds
    p, nr = F.cloud('micro')
    good_p, good_n = _gpu(p), _gpu(nr)
    for which, bad in ((0, np.nan), (1, np.inf)):
        arrays = [p.copy(), nr.copy()]
        arrays[which][9, 2] = bad
        bad_p, bad_n = _gpu(arrays[0]), _gpu(arrays[1])
        for search in ((0.12, None), (None, 8)):
            with pytest.raises(ValueError, match='cloud 1: a point or normal is not finite'):
                compute_fpfh_clouds([good_p, bad_p, good_p], [good_n, bad_n, good_n], *search)
        # the call raises, so no rows come back; "the other clouds of the chunk are unaffected" here means that the status words, which
        # are all a refusal is made from, name cloud 1 alone (the rows of good clouds beside each other are pinned by the batch test)
        words = ops.fpfh_check_stack(torch.cat([good_p, bad_p, good_p]), torch.cat([good_n, bad_n, good_n]), [len(p)] * 3)
        assert words.cpu().tolist() == [0, 1, 0, 1]
    with pytest.raises(ValueError, match='cloud 33'):                                      # the index counts across chunks
        q = p.copy()
        q[0, 0] = np.nan
        spfh_clouds([good_p[:5]] * 33 + [_gpu(q)], [good_n[:5]] * 33 + [good_n], 0.12)
    with pytest.raises(ValueError, match='radius, max_nn or both'):
        compute_fpfh_clouds([good_p], [good_n])
    with pytest.raises(ValueError, match='SE3_KNN_MAX'):
        compute_fpfh_clouds([good_p], [good_n], max_nn=65)
    for radius in (0, -0.1, np.inf, np.nan):
        with pytest.raises(ValueError, match='radius'):
            compute_fpfh_clouds([good_p], [good_n], radius)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        compute_fpfh_clouds([torch.from_numpy(p)], [good_n], 0.12)
    with pytest.raises(ValueError, match='normals'):
        compute_fpfh_clouds([good_p], [good_n[:-1]], 0.12)


def test_global_registration_of_the_moved_surface():
    """global_registration_pairs on the surface cloud and its moved, permuted copy at voxel size 0.1 (517 and 532 voxels), seed 0, with ICP:
    the result meets the reference's acceptance (cfg.eval: RRE below 15 degrees, RTE below 0.3 m).  Measured without a GPU on the twins of
    the three stages: 249 mutual feature matches of the voxelised pair, 89.6 % of them within 1.5 voxel sizes of their true position
    (83.2 % of all nearest-feature matches)."""
    from se3et_amd.fpfh import global_registration_pairs
    p, _ = F.cloud('surface')
    mp, _, _, Rm, t = F.moved_surface()
    v = 0.1
    out = global_registration_pairs([_gpu(mp)], [_gpu(p)], v, icp_distance=1.5 * v, seed=0)
    assert tuple(out['transforms'].shape) == (1, 4, 4) and out['src_feats'][0].dtype == torch.float32
    assert out['src_feats'][0].shape == (out['src_points'][0].shape[0], twin.DIM)
    for key in ('ransac_transforms', 'transforms'):
        T = out[key][0].cpu().numpy().astype(np.float64)                                    # ref ~ T src: the inverse of the motion
        rot, shift = T[:3, :3], T[:3, 3]
        rre = np.degrees(np.arccos(np.clip((np.trace(rot @ Rm) - 1.0) / 2.0, -1.0, 1.0)))
        rte = np.linalg.norm(shift - (-Rm.T @ t))
        print('%s: RRE %.4f deg, RTE %.5f' % (key, rre, rte))
        if key == 'transforms':                                                             # the result with ICP: the reference's acceptance
            assert rre < 15.0 and rte < 0.3
