"""GPU: the scan preparation kernels (csrc/voxel_downsample.hip, csrc/knn_normals.hip) through se3et_amd/scan_prep.py.

The kernels run the same __host__ __device__ text as the library's host entries, so the device results are compared with those BIT FOR BIT
(and hence meet the twin's demands, which tests/test_scan_prep_cpu.py checks of the host entries); batches equal single calls, two runs are
bit-identical, and the wiring into data.py and pair_geometry.py changes nothing at its defaults."""
import os

import numpy as np
import pytest
import torch

import scan_prep_fixture as F
import scan_prep_twin as twin

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scan_prep.npz')


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).cuda()          # (a copy: the fixture arrays are read-only)


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def all_clouds():
    """name -> float64 or float32 points: the fixture clouds and the edge cases"""
    out = {name: F.cloud(name) for name in F.CLOUDS}
    out.update({name: p for name, (p, _) in F.edge_clouds().items()})
    return out


def test_voxel_downsample_equals_the_host_entry():
    from se3et_amd.scan_prep import voxel_downsample, voxel_downsample_clouds
    cases = [(name, F.cloud(name), v) for name in F.CLOUDS for v in F.VOXEL_SIZES.values()]
    cases += [(name, p, v) for name, (p, v, _) in F.voxel_edge_cases().items()]
    for dtype in (np.float32, np.float64):
        for v in sorted({c[2] for c in cases}):
            group = [(name, np.asarray(p, dtype)) for name, p, vv in cases if vv == v]
            normals = [np.random.default_rng(1).standard_normal(p.shape).astype(dtype) for _, p in group]
            pts, nrm = voxel_downsample_clouds([dev(p) for _, p in group], v, [dev(n) for n in normals])
            plain = voxel_downsample_clouds([dev(p) for _, p in group], v)
            for (name, p), n, gp, gn, gq in zip(group, normals, _np(pts), _np(nrm), _np(plain)):
                hp, hn, status = F.host_voxel(p, v, n)
                assert status == 0 and gp.dtype == np.float64 and gp.shape == hp.shape, name
                assert np.array_equal(gp, hp) and np.array_equal(gn, hn) and np.array_equal(gq, hp), name
    p, v, voxels = F.voxel_edge_cases()['own_voxels_2000']
    assert len(voxel_downsample(p, v)) == voxels                         # the reference's single-cloud signature: numpy in and out
    a, b = voxel_downsample(p.astype(np.float32), v, p.astype(np.float32))
    assert isinstance(a, np.ndarray) and np.array_equal(a, b)


def test_voxel_downsample_at_the_chunk_sizes_of_the_rank_scans():
    """Three clouds of 1023, 1024 and 1025 points in one call: the last sizes at which a thread of voxel_rank_kernel scans one point, and the
    first with two.  The first two clouds share voxels (both kinds of flag, member lists of several points); the third is a jittered lattice
    with one point per voxel, so its 1025 voxels take the scan of the member counts past one voxel per thread as well."""
    from se3et_amd.scan_prep import voxel_downsample_clouds
    rng = np.random.default_rng(5)
    v = 0.05
    lattice = np.stack(np.unravel_index(rng.permutation(11 * 11 * 9)[:1025], (11, 11, 9)), 1) * v + rng.uniform(-0.2 * v, 0.2 * v, (1025, 3))
    clouds = [rng.uniform(0, 8 * v, (1023, 3)), rng.uniform(0, 8 * v, (1024, 3)), lattice]
    for dtype in (np.float32, np.float64):
        group = [np.asarray(p, dtype) for p in clouds]
        normals = [rng.standard_normal(p.shape).astype(dtype) for p in group]
        pts, nrm = voxel_downsample_clouds([dev(p) for p in group], v, [dev(n) for n in normals])
        counts = []
        for p, n, gp, gn in zip(group, normals, _np(pts), _np(nrm)):
            hp, hn, status = F.host_voxel(p, v, n)
            assert status == 0 and gp.shape == hp.shape and np.array_equal(gp, hp) and np.array_equal(gn, hn)
            counts.append(len(hp))
        assert counts[0] < 1023 and counts[1] < 1024 and counts[2] == 1025


def test_voxel_downsample_refusals():
    from se3et_amd.scan_prep import voxel_downsample_clouds
    p = F.cloud('micro').astype(np.float64)
    bad = p.copy()
    bad[7, 2] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        voxel_downsample_clouds([dev(p), dev(bad)], 0.05)
    wide = p.copy()
    wide[int(np.argmax(p[:, 1])), 1] = p[:, 1].min() + 0.01 * 2.0 ** 21
    with pytest.raises(ValueError, match='2\\^21 voxels'):
        voxel_downsample_clouds([dev(wide)], 0.01)
    assert np.array_equal(voxel_downsample_clouds([dev(p)], 0.05)[0].cpu().numpy(), F.host_voxel(p, 0.05)[0])     # and the next call is clean
    assert voxel_downsample_clouds([], 0.05) == []


def test_knn_equals_the_host_entry():
    from se3et_amd.scan_prep import knn_clouds
    clouds = all_clouds()
    names = list(clouds)
    for k in (1, 3, 33, 64):
        idx, d2 = knn_clouds([dev(clouds[n], np.float64) for n in names], k)
        for name, gi, gd in zip(names, _np(idx), _np(d2)):
            hi, hd = F.host_knn(clouds[name], k)
            assert gi.shape == (len(clouds[name]), k) and np.array_equal(gi, hi) and np.array_equal(gd, hd), (name, k)
    # other queries than the support, some far outside its box; float32
    for name in ('micro', 'clusters', 'lattice', 'n2'):
        p = np.asarray(clouds[name], np.float32)
        q = np.concatenate([p[:40], p[:5] + 100.0, np.array([[-3.0, 7.0, 0.5]], np.float32)], 0)
        idx, d2 = knn_clouds([dev(p)], 33, [dev(q)])
        hi, hd = F.host_knn(p, 33, q, np.float32)
        assert np.array_equal(idx[0].cpu().numpy(), hi) and np.array_equal(d2[0].cpu().numpy(), hd), name
    ti, td = F.twin_knn('micro')
    idx, d2 = knn_clouds([dev(F.cloud('micro'))], 64)
    assert np.array_equal(idx[0].cpu().numpy(), ti) and np.array_equal(d2[0].cpu().numpy(), td)                  # and the twin itself


def test_normals_equal_the_host_entry():
    from se3et_amd.scan_prep import estimate_normals, estimate_normals_clouds
    clouds = all_clouds()
    names = list(clouds)
    for dtype in (np.float32, np.float64):
        got = _np(estimate_normals_clouds([dev(clouds[n], dtype) for n in names]))
        for name, g in zip(names, got):
            h, _ = F.host_normals(np.asarray(clouds[name], dtype))
            assert g.shape == h.shape and np.array_equal(g, h), name
    got = _np(estimate_normals_clouds([dev(clouds[n], np.float64) for n in names], knn=7))
    for name, g in zip(names, got):
        assert np.array_equal(g, F.host_normals(np.asarray(clouds[name], np.float64), 7)[0]), name
    for name in F.CLOUDS:                                                # hence the twin's demands
        _, _, tn, w = F.twin_normals(name)
        n = estimate_normals(F.cloud(name))
        F.assert_unit(n)
        F.assert_directions(n, tn, w, max_excluded=0.0)


def test_batches_equal_single_calls_and_runs_repeat():
    from se3et_amd.scan_prep import estimate_normals_clouds, knn_clouds, voxel_downsample_clouds
    g = np.random.default_rng(9)
    clouds = [dev(F.cloud('micro')), dev(np.zeros((0, 3), np.float32)), dev(F.cloud('c1_2k')[:777]), dev(g.uniform(-1, 1, (65, 3))),
              dev(F.cloud('c3_1500')[:300])]

    def run(cs):
        return (voxel_downsample_clouds(cs, 0.1), knn_clouds(cs, 33)[0], knn_clouds(cs, 33)[1], estimate_normals_clouds(cs))
    batch, again = run(clouds), run(clouds)
    for a, b in zip(batch, again):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    for i, c in enumerate(clouds):
        for a, b in zip(batch, run([c])):
            assert torch.equal(a[i], b[0]), i
    many = [clouds[i % 5] for i in range(33)]                            # more than one chunk of 32
    for a, b in zip(batch, run(many)):
        assert len(b) == 33 and all(torch.equal(b[i], a[i % 5]) for i in range(33))


def test_viewpoints_orient_the_normals():
    from se3et_amd.scan_prep import estimate_normals_clouds
    names = ('micro', 'c1_2k')
    clouds = [dev(F.cloud(n)) for n in names]
    views = np.array([[0.3, 0.25, 0.2], [5.0, -4.0, 3.0]])
    plain = _np(estimate_normals_clouds(clouds))
    got = _np(estimate_normals_clouds(clouds, viewpoints=views))
    for name, n, p0, v in zip(names, got, plain, views):
        p = F.cloud(name).astype(np.float64)
        assert (((n * (v - p)).sum(1)) >= 0).all() and np.array_equal(np.abs(n), np.abs(p0))
        assert np.array_equal(n, F.host_normals(p.astype(np.float32), viewpoint=v)[0])
    one = _np(estimate_normals_clouds(clouds, viewpoints=views[0]))
    assert np.array_equal(one[0], got[0])


def _pyramid_inputs(presets):
    from se3et_amd.model import make_cfg
    from se3et_amd.synthetic import make_pair
    cfg = make_cfg('micro_e')
    clouds = []
    for preset in presets:
        ref, src, _ = make_pair(preset)
        clouds += [ref, src]
    b = cfg.backbone
    return (dev(np.concatenate(clouds, 0)), torch.tensor([len(c) for c in clouds]), b.num_stages, b.init_voxel_size, b.init_radius,
            cfg.neighbor_limits)


@pytest.mark.parametrize('presets', [('micro',), ('micro', 'c1_2k')])
def test_precompute_carries_the_normals(presets):
    from se3et_amd.data import precompute_data_stack_mode
    from se3et_amd.modules.ops import grid_subsample
    from se3et_amd.scan_prep import estimate_normals_clouds
    points, lengths, stages, voxel, radius, limits = _pyramid_inputs(presets)
    plain = precompute_data_stack_mode(points, lengths, stages, voxel, radius, limits)
    off = precompute_data_stack_mode(points, lengths, stages, voxel, radius, limits, normals=False)
    on = precompute_data_stack_mode(points, lengths, stages, voxel, radius, limits, normals=True)
    assert sorted(plain) == sorted(off) == ['lengths', 'neighbors', 'points', 'subsampling', 'upsampling']
    assert sorted(on) == sorted(list(plain) + ['normals'])
    for key in plain:
        for a, b, c in zip(plain[key], off[key], on[key]):
            assert torch.equal(a, b) and torch.equal(a.cpu(), c.cpu()), key
    normals = on['normals']
    assert [tuple(n.shape) for n in normals] == [tuple(p.shape) for p in on['points']] and all(n.dtype == torch.float32 for n in normals)
    want = torch.cat(estimate_normals_clouds(list(torch.split(points, lengths.tolist()))), 0).float()
    assert torch.equal(normals[0], want)
    v = voxel
    for i in range(1, stages):
        v *= 2
        pts, lens, nrm = grid_subsample(on['points'][i - 1], on['lengths'][i - 1], normals[i - 1], v)
        assert int(lens.max()) <= 2000                                   # (no cap at these sizes: the stage is the subsampling itself)
        assert torch.equal(pts, on['points'][i]) and torch.equal(nrm, normals[i]), i


def test_collate_passes_the_normals_switch():
    from se3et_amd.data import registration_collate_fn_stack_mode
    from se3et_amd.model import make_cfg
    from se3et_amd.synthetic import make_pair
    cfg = make_cfg('micro_e')
    ref, src, T = make_pair('micro')
    d = dict(ref_points=ref, src_points=src, ref_feats=np.ones((len(ref), 1), np.float32), src_feats=np.ones((len(src), 1), np.float32),
             transform=T)
    b = cfg.backbone
    args = ([d], b.num_stages, b.init_voxel_size, b.init_radius, cfg.neighbor_limits)
    plain, on = registration_collate_fn_stack_mode(*args), registration_collate_fn_stack_mode(*args, normals=True)
    assert 'normals' not in plain and sorted(on) == sorted(list(plain) + ['normals'])
    assert all(torch.equal(a, c) for a, c in zip(plain['points'], on['points'])) and len(on['normals']) == b.num_stages


def test_calibrate_ground_truth_downsample():
    from se3et_amd import pair_geometry as PG
    from se3et_amd.scan_prep import voxel_downsample_clouds
    from se3et_amd.synthetic import make_pair
    refs, srcs, Ts = [], [], []
    for preset in ('micro', 'c1_2k'):
        ref, src, T = make_pair(preset)
        refs.append(dev(ref)), srcs.append(dev(src)), Ts.append(T.astype(np.float64))
    np.random.seed(0)
    ov0, cov0 = PG.calibrate_ground_truth_pairs(refs, srcs, Ts, voxel_size=0.02)
    np.random.seed(0)
    ov1, cov1 = PG.calibrate_ground_truth_pairs(refs, srcs, Ts, voxel_size=0.02, downsample=None)
    assert torch.equal(ov0, ov1) and torch.equal(cov0, cov1)
    ov2, cov2 = PG.calibrate_ground_truth_pairs(refs, srcs, Ts, voxel_size=0.02, downsample=0.01)
    ov3, cov3 = PG.calibrate_ground_truth_pairs(voxel_downsample_clouds(refs, 0.01), voxel_downsample_clouds(srcs, 0.01), Ts, voxel_size=0.02)
    assert torch.equal(ov2, ov3) and torch.equal(cov2, cov3)
    assert sum(len(c) for c in voxel_downsample_clouds(refs, 0.01)) < sum(len(c) for c in refs)          # (it did merge points)
    ov4, cov4 = PG.calibrate_ground_truth(refs[0].cpu().numpy(), srcs[0].cpu().numpy(), Ts[0], voxel_size=0.02, downsample=0.01)
    assert ov4 == ov2[0].item() and np.array_equal(cov4, cov2[0].cpu().numpy())


def test_modified_chamfer_distance():
    from se3et_amd import pair_geometry as PG
    g = np.load(GOLDEN)
    args = [g['mcd/' + k] for k in ('raw', 'ref', 'src', 'gt_transform', 'transform')]
    bound = F.chamfer_float32_bound(*args)
    t = [dev(a) for a in args]
    want = twin.modified_chamfer_distance(*args, reduction='none')
    none = PG.modified_chamfer_distance(*t, reduction='none')
    assert none.dtype == torch.float64 and none.is_cuda
    for reduction, reduce, b in (('none', lambda x: x, bound), ('mean', np.mean, bound.mean()), ('sum', np.sum, bound.sum())):
        got = PG.modified_chamfer_distance(*t, reduction=reduction).cpu().numpy()
        print(reduction, got, reduce(want), g['mcd/' + reduction])
        assert (np.abs(got - reduce(want)) <= 1e-12 * np.abs(reduce(want))).all()
        assert (np.abs(got - g['mcd/' + reduction]) <= b).all()
    pairs = PG.modified_chamfer_distance_pairs([t[0][0], t[0][1][:250]], [t[1][0], t[1][1]], [t[2][0], t[2][1][:100]], args[3], args[4])
    assert torch.equal(pairs[0], none[0]) and pairs.shape == (2,)


def test_the_coarsest_stage_caps_the_normals_with_its_points():
    """A hall whose coarsest stage holds more than 2000 points per cloud: the normals keep the rows the points keep."""
    from se3et_amd.data import stage_clouds
    from se3et_amd.modules.ops import grid_subsample
    from se3et_amd.synthetic import make_pair
    ref, src, _ = make_pair('cap_30k')
    points, lengths = dev(np.concatenate([ref, src], 0)), torch.tensor([len(ref), len(src)])
    normals = dev(np.random.default_rng(4).standard_normal((len(ref) + len(src), 3)).astype(np.float32))
    stages, voxel = 4, 0.025
    plain_p, plain_l = stage_clouds(points, lengths, stages, voxel)
    got_p, got_l, got_n = stage_clouds(points, lengths, stages, voxel, normals)
    assert all(torch.equal(a, b) for a, b in zip(plain_p, got_p)) and all(torch.equal(a, b) for a, b in zip(plain_l, got_l))
    p, l, n, v = points, lengths, normals, voxel
    for i in range(1, stages):
        v *= 2
        p, l, n = grid_subsample(p, l, n, v)
        if i < stages - 1:
            assert torch.equal(p, got_p[i]) and torch.equal(n, got_n[i]) and torch.equal(l, got_l[i])
    assert int(l.min()) > 2000                                           # both clouds are cut
    keep = torch.cat([torch.arange(2000), int(l[0]) + torch.arange(2000)]).cuda()
    assert got_l[-1].tolist() == [2000, 2000]
    assert torch.equal(got_p[-1], p[keep]) and torch.equal(got_n[-1], n[keep]) and got_n[-1].shape == got_p[-1].shape


def test_refusals_name_the_cloud():
    from se3et_amd.scan_prep import voxel_downsample_clouds
    p = F.cloud('micro').astype(np.float64)
    bad = p.copy()
    bad[7, 2] = np.inf
    wide = p.copy()
    wide[int(np.argmax(p[:, 1])), 1] = p[:, 1].min() + 0.05 * 2.0 ** 21
    with pytest.raises(ValueError, match='cloud 1: a point .* is not finite; cloud 3: an axis would need 2\\^21 voxels'):
        voxel_downsample_clouds([dev(p), dev(bad), dev(p), dev(wide)], 0.05)
    many = [dev(p)] * 34 + [dev(bad)]
    with pytest.raises(ValueError, match='cloud 34: a point'):
        voxel_downsample_clouds(many, 0.05)
