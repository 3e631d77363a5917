"""GPU: RANSAC registration from correspondences (se3et_amd.ransac, csrc/ransac.hip) against the host twin (tests/ransac_twin.py), on
synthetic recoveries, for determinism and batch independence, its edge cases, and as eval.py's registration step on forward_pairs outputs.

Device and twin are compared hypothesis by hypothesis through explicit indices.  Inlier counts may differ only by the hypothesis'
borderline correspondences (|d_f64 - thr| <= 1e-5 (1 + |s| + |r|)) and are not compared for degenerate samples (second singular value
below 1e-9 of the first: the rotation is not determined there).  Error sums agree to 1e-4 relative plus the float32 rounding floor of
the inliers' d^2 (ransac_twin.py)."""
import numpy as np
import pytest
import torch

import ransac_twin as RT

pytestmark = pytest.mark.gpu

SIZES = (50, 500, 2000, 5000)
RATIOS = (0.5, 0.3, 0.15, 0.08)


def _pairs(seed, sizes, ratios):
    rng = np.random.default_rng(seed)
    return [RT.synthetic_pair(rng, n, r) for n, r in zip(sizes, ratios)]


def _order_best(counts, errs):
    """The device's own total order: most inliers, smallest error sum, lowest h; -1 when no hypothesis has an inlier."""
    c, e = counts.astype(np.int64), errs.astype(np.float64)
    if c.max() <= 0:
        return -1
    return int(np.lexsort((np.arange(len(c)), e, -c))[0])


def _rre_rte(E, T):
    rre = np.degrees(np.arccos(np.clip((np.trace(E[:3, :3].T @ T[:3, :3]) - 1) / 2, -1, 1)))
    return rre, np.linalg.norm(E[:3, 3] - T[:3, 3])


@pytest.mark.parametrize('rn', [3, 4, 12])
def test_explicit_hypotheses_match_the_twin(rn):
    from se3et_amd.ransac import ransac_pairs
    H, thr = 4096, 0.05
    pairs = _pairs(10 + rn, SIZES, RATIOS)
    rng = np.random.default_rng(rn)
    idx = np.stack([rng.integers(0, n, (H, rn)) for n in SIZES]).astype(np.int32)
    idx[:, 5, 1] = idx[:, 5, 0]                              # a repeated index in every pair
    idx[:, 6, :] = idx[:, 6, :1]                             # one point rn times: rank 0
    out = ransac_pairs([p[0] for p in pairs], [p[1] for p in pairs], thr, rn, H, hypothesis_indices=torch.from_numpy(idx),
                       per_hypothesis=True)
    counts, errs = out['counts'].cpu().numpy(), out['err_sums'].cpu().numpy()
    best, fit, rmse = out['best_hypothesis'].cpu().numpy(), out['fitness'].cpu().numpy(), out['inlier_rmse'].cpu().numpy()
    Ts = out['transforms'].cpu().numpy()
    assert np.isfinite(Ts).all()
    for p, ((src, ref, _), n) in enumerate(zip(pairs, SIZES)):
        tw = RT.run(src, ref, thr, rn, idx[p])
        ok = ~tw['degenerate']
        assert ok.sum() > 0.9 * H
        diff = np.abs(counts[p].astype(np.int64) - tw['counts'])
        assert np.all(diff[ok] <= tw['n_border'][ok]), (p, np.flatnonzero(diff[ok] > tw['n_border'][ok])[:5])
        same = ok & (diff == 0) & (tw['n_border'] == 0)
        assert same.sum() > 0.9 * H
        err_tol = 1e-4 * tw['err_sums'] + tw['err_floor']
        bad = np.abs(errs[p] - tw['err_sums']) > err_tol
        assert not np.any(bad & same), (p, np.flatnonzero(bad & same)[:5])
        # the winner: exactly the maximum of the device's own order, and as good as the twin's best within the allowance
        h = _order_best(counts[p], errs[p])
        assert best[p] == h
        assert h >= 0
        assert fit[p] == np.float32(counts[p, h] / n)
        assert rmse[p] == np.float32(np.sqrt(np.float64(errs[p, h]) / counts[p, h]))
        hb = tw['best']
        assert tw['counts'][h] + tw['n_border'][h] >= tw['counts'][hb] - tw['n_border'][hb]
        if not tw['degenerate'][h]:             # the winner's transform is its own float64 fit, rounded
            assert np.abs(Ts[p, :3, :3] - tw['R'][h]).max() < 1e-5 and np.abs(Ts[p, :3, 3] - tw['t'][h]).max() < 1e-4
        assert np.array_equal(Ts[p, 3], [0, 0, 0, 1])
        # degenerate samples still give finite rotations (the repeated-point hypothesis scores as any other)
        assert counts[p, 6] >= 0


@pytest.mark.parametrize('rn', [3, 12])
def test_generated_samples_equal_explicit_sample_indices(rn):
    from se3et_amd.ransac import ransac_pairs, sample_indices
    H, seed = 3000, 1234567
    pairs = _pairs(20, (100, 1000, 3000), (0.3, 0.2, 0.1))
    src, ref = [p[0] for p in pairs], [p[1] for p in pairs]
    gen = ransac_pairs(src, ref, 0.05, rn, H, seed=seed, per_hypothesis=True)
    idx = np.stack([sample_indices(seed, len(s), H, rn) for s in src]).astype(np.int32)
    exp = ransac_pairs(src, ref, 0.05, rn, H, seed=999, hypothesis_indices=torch.from_numpy(idx), per_hypothesis=True)
    for k in gen:
        assert torch.equal(gen[k], exp[k]), k


@pytest.fixture(scope='module')
def recovery():
    from se3et_amd.model import make_cfg
    from se3et_amd.ransac import ransac_pairs
    r = make_cfg('se3ete').ransac
    pairs = _pairs(30, [5000] * 16, np.linspace(0.05, 0.5, 16))
    src, ref = [p[0] for p in pairs], [p[1] for p in pairs]
    out = ransac_pairs(src, ref, r.distance_threshold, r.num_points, r.num_iterations, seed=3)
    torch.cuda.synchronize()
    return r, pairs, src, ref, out


def test_recovery_of_synthetic_pairs(recovery):
    r, pairs, _, _, out = recovery
    Ts, fit = out['transforms'].cpu().numpy().astype(np.float64), out['fitness'].cpu().numpy()
    for p, (src, ref, T) in enumerate(pairs):
        rre, rte = _rre_rte(Ts[p], T)
        assert rre < 5.0 and rte < 0.1, (p, rre, rte)
        d = np.linalg.norm(src.astype(np.float64) @ T[:3, :3].T + T[:3, 3] - ref, axis=1)
        assert fit[p] >= 0.9 * np.mean(d < r.distance_threshold), (p, fit[p])


def test_deterministic_and_batch_independent(recovery):
    from se3et_amd.ransac import ransac_pairs
    r, _, src, ref, out = recovery
    again = ransac_pairs(src, ref, r.distance_threshold, r.num_points, r.num_iterations, seed=3)
    for k in out:
        assert torch.equal(out[k], again[k]), k
    alone = ransac_pairs(src[7:8], ref[7:8], r.distance_threshold, r.num_points, r.num_iterations, seed=3)
    for k in out:
        assert torch.equal(out[k][7:8], alone[k]), k


def test_edge_cases():
    from se3et_amd.ransac import ransac_pairs
    (s0, r0, _), (s1, r1, _) = _pairs(40, (300, 300), (0.5, 0.5))
    eye = torch.eye(4, device='cuda')
    # n < ransac_n and an empty pair inside a batch
    out = ransac_pairs([s0, s1[:2], s1[:0], s1], [r0, r1[:2], r1[:0], r1], 0.05, 3, 2000, per_hypothesis=True)
    for p in (1, 2):
        assert torch.equal(out['transforms'][p], eye) and out['fitness'][p] == 0 and out['inlier_rmse'][p] == 0
        assert out['best_hypothesis'][p] == -1 and int(out['counts'][p].abs().max()) == 0
    assert out['fitness'][0] > 0.4 and out['fitness'][3] > 0.4
    # distance_threshold <= 0 and ransac_n < 3: identity everywhere
    for thr, rn in ((0.0, 3), (-1.0, 3), (0.05, 2)):
        o = ransac_pairs([s0, s1], [r0, r1], thr, rn, 500, per_hypothesis=True)
        assert torch.equal(o['transforms'], eye.expand(2, 4, 4)) and not o['fitness'].any() and not o['inlier_rmse'].any()
        assert (o['best_hypothesis'] == -1).all() and not o['counts'].any() and not o['err_sums'].any()
    # NaN correspondences are never inliers; a sample touching one has none
    src, ref, _ = RT.synthetic_pair(np.random.default_rng(41), 400, 1.0, sigma=0.0)
    src[10:20, 1] = np.nan
    ref[30:35, 0] = np.inf
    idx = np.random.default_rng(42).integers(0, 400, (1, 256, 3)).astype(np.int32)
    idx[0, 0] = (10, 100, 200)
    idx[0, 1] = (30, 100, 200)
    o = ransac_pairs([src], [ref], 0.05, 3, 256, hypothesis_indices=torch.from_numpy(idx), per_hypothesis=True)
    c = o['counts'][0].cpu().numpy()
    assert c[0] == 0 and c[1] == 0 and c.max() == 385
    assert float(o['fitness'][0]) == np.float32(385 / 400)
    with pytest.raises(RuntimeError, match='ransac_n'):
        ransac_pairs([s0], [r0], 0.05, 17, 100)


@pytest.fixture(scope='module')
def c2_batch():
    from se3et_amd.batched import forward_pairs
    from se3et_amd.data import precompute_data_stack_mode
    from se3et_amd.model import create_model, load_synthetic_weights, make_cfg
    from se3et_amd.synthetic import make_pair
    cfg = make_cfg('se3ete')
    model = load_synthetic_weights(create_model(cfg)).cuda().eval()
    b = cfg.backbone
    clouds, Ts = [], []
    for i in range(16):
        ref, src, T = make_pair('c2_5k', i)
        clouds += [ref, src]
        Ts.append(T)
    pts = torch.from_numpy(np.concatenate(clouds, 0)).cuda()
    data = precompute_data_stack_mode(pts, torch.tensor([len(c) for c in clouds]), b.num_stages, b.init_voxel_size, b.init_radius,
                                      cfg.neighbor_limits)
    data['features'] = torch.ones((pts.shape[0], 1), device='cuda')
    with torch.no_grad():
        outs = forward_pairs(model, data)
    return cfg, outs, torch.from_numpy(np.stack(Ts)).cuda()


def test_register_pairs_end_to_end(c2_batch):
    from se3et_amd import ops
    from se3et_amd.evaluation import evaluate_pairs
    from se3et_amd.ransac import ransac_pairs, register_pairs, select_correspondences
    cfg, outs, gt = c2_batch
    lgr = register_pairs(cfg, outs, 'lgr')
    for p, out in enumerate(outs):
        assert torch.equal(lgr[p], out['estimated_transform'])
    for num_corr in (250, None):
        svd = register_pairs(cfg, outs, 'svd', num_corr)
        for p, out in enumerate(outs):
            r, s, w = select_correspondences(out, num_corr)
            one = ops.weighted_procrustes(s, r, w, torch.tensor([0, w.shape[0]], device='cuda'), eps=1e-5)
            assert torch.equal(svd[p], one[0]), (num_corr, p)
        rs = register_pairs(cfg, outs, 'ransac', num_corr, seed=5)
        cut = [select_correspondences(out, num_corr) for out in outs]
        want = ransac_pairs([c[1] for c in cut], [c[0] for c in cut], cfg.ransac.distance_threshold, cfg.ransac.num_points,
                            cfg.ransac.num_iterations, seed=5)['transforms']
        assert torch.equal(rs, want), num_corr
    assert any(o['corr_scores'].shape[0] > 250 for o in outs)
    for out, T in zip(outs, rs):
        out['estimated_transform'] = T
    res = evaluate_pairs(cfg, outs, gt)
    assert set(res) == {'PIR', 'IR', 'RRE', 'RTE', 'RMSE', 'RR'} and all(v.shape == (16,) for v in res.values())
    for out, T in zip(outs, lgr):
        out['estimated_transform'] = T
    with pytest.raises(ValueError):
        register_pairs(cfg, outs, 'icp')


def test_dropin_matches_the_batched_call(recovery):
    from se3et_amd.ransac import ransac_pairs, registration_with_ransac_from_correspondences
    _, _, src, ref, _ = recovery
    out = ransac_pairs(src[:3], ref[:3], 0.05, 3, 10000, seed=0)
    for p in range(3):
        T = registration_with_ransac_from_correspondences(src[p], ref[p])
        assert isinstance(T, np.ndarray) and T.dtype == np.float64 and T.shape == (4, 4)
        assert np.array_equal(T, out['transforms'][p].cpu().numpy().astype(np.float64))
    # a (K, 2) correspondence table over the clouds equals the pre-gathered call
    rng = np.random.default_rng(50)
    ps, pr = rng.permutation(5000), rng.permutation(5000)
    src_cloud, ref_cloud = np.empty_like(src[0]), np.empty_like(ref[0])
    src_cloud[ps], ref_cloud[pr] = src[0], ref[0]
    table = np.stack([ps, pr], 1)[:4000]
    a = registration_with_ransac_from_correspondences(src_cloud, ref_cloud, table, 0.05, 3, 20000, seed=9)
    b = registration_with_ransac_from_correspondences(src[0][:4000], ref[0][:4000], None, 0.05, 3, 20000, seed=9)
    assert np.array_equal(a, b)
