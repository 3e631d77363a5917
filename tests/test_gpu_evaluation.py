"""GPU: registration evaluation (se3et_amd.evaluation, csrc/evaluation.hip) against the reference's get_node_correspondences and Evaluator
(tests/golden/eval_metrics.npz, written by generate_eval_golden.py) and against the plain-torch ground truth of se3et_amd.training.

Borderline point pairs: the kernel transforms the src points with its own float32 FMAs, the reference (and training.node_correspondences)
through a GEMM whose summation order is the library's.  A patch pair may therefore come out differently only where one of its point pairs
lies within |d^2 - r^2| <= 1e-6 r^2 of the matching radius; the comparisons below find such pairs in float64 and allow exactly those."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LIMITS = [38, 36, 36, 38]
C2_PAIRS = 8


@pytest.fixture(scope='module')
def golden(golden_dir):
    import os
    return dict(np.load(os.path.join(golden_dir, 'eval_metrics.npz')))


def _cfg(kitti=False):
    from se3et_amd.model import make_cfg
    return make_cfg('se3eti_kitti' if kitti else 'se3ete')


_CLOUDS = {}


def _rebuild(kitti, index):
    """Pair `index` of make_pair('c3_20k' / 'c2_5k'): pyramid and node partition built on the device by this package.  Returns the
    partition inputs of one pair (knn local to its cloud), the stage-0 src points and the transform."""
    key = (kitti, index)
    if key not in _CLOUDS:
        from se3et_amd import ops
        from se3et_amd.data import precompute_data_stack_mode
        from se3et_amd.synthetic import make_pair
        cfg = _cfg(kitti)
        b = cfg.backbone
        ref, src, T = make_pair('c3_20k' if kitti else 'c2_5k', index)
        pts = torch.from_numpy(np.concatenate([ref, src], 0)).cuda()
        dd = precompute_data_stack_mode(pts, torch.tensor([len(ref), len(src)]), b.num_stages, b.init_voxel_size, b.init_radius,
                                        cfg.neighbor_limits)
        pf, pc, p0 = dd['points'][1], dd['points'][-1], dd['points'][0]
        lf, lc, l0 = dd['lengths'][1].tolist(), dd['lengths'][-1].tolist(), dd['lengths'][0].tolist()
        _, nm, knn, km = ops.point_to_node_partition_stack(pf, pc, lf, lc, cfg.model.num_points_in_patch)
        _CLOUDS[key] = dict(ref_points_f=pf[:lf[0]], src_points_f=pf[lf[0]:], ref_points_c=pc[:lc[0]], src_points_c=pc[lc[0]:],
                            src_points=p0[l0[0]:], ref_knn=knn[:lc[0]], src_knn=knn[lc[0]:] - lf[0], ref_knn_masks=km[:lc[0]],
                            src_knn_masks=km[lc[0]:], ref_node_masks=nm[:lc[0]], src_node_masks=nm[lc[0]:],
                            transform=torch.from_numpy(T).cuda())
    return _CLOUDS[key]


def _pair(g, prefix):
    """The clouds of a fixture pair ('c2/p<i>/', 'kitti/p0/', 'edge/' = C2 pair 0), rebuilt on the device and held to the checksums of
    the reference's collate and point_to_node_partition that the fixture stores (tests/eval_fixture.py)."""
    from eval_fixture import pair_checksums
    kitti, index = (True, 0) if prefix.startswith('kitti') else (False, int(prefix[4]) if prefix.startswith('c2/p') else 0)
    d = _rebuild(kitti, index)
    got = pair_checksums({k: v.cpu().numpy() for k, v in d.items() if k != 'transform'})
    for k, v in got.items():
        assert int(v) == int(g[prefix + 'checksum/' + k]), '%s: %s differs from the reference\'s' % (prefix, k)
    assert np.array_equal(d['transform'].cpu().numpy(), g[prefix + 'transform']) or prefix.startswith('edge/')
    return d


def _stack(pairs):
    """Stacked inputs of gt_node_overlaps_stack: clouds ref0, src0, ref1, ... with GLOBAL knn indices."""
    pf, pc, knn, km, nm, lc = [], [], [], [], [], []
    base = 0
    for d in pairs:
        for side in ('ref', 'src'):
            f = d[side + '_points_f']
            pf.append(f)
            pc.append(d[side + '_points_c'])
            knn.append(d[side + '_knn'].long() + base)
            km.append(d[side + '_knn_masks'].bool())
            nm.append(d[side + '_node_masks'].bool())
            lc.append(d[side + '_points_c'].shape[0])
            base += f.shape[0]
    knn = torch.cat(knn, 0)
    km = torch.cat(km, 0)
    knn = torch.where(km, knn, torch.full_like(knn, base))
    return (torch.cat(pf, 0).float(), torch.cat(pc, 0).float(), lc, knn, km, torch.cat(nm, 0),
            torch.stack([d['transform'].float() for d in pairs], 0))


def _kernel_gt(pairs, radius):
    from se3et_amd import ops
    pf, pc, lc, knn, km, nm, T = _stack(pairs)
    return ops.gt_node_overlaps_stack(pf, pc, lc, knn, km, nm, T, radius)


def _knn_points64(points, knn, masks):
    p = points.double()
    idx = torch.where(masks.bool(), knn.long(), torch.zeros_like(knn.long()))
    return p[idx]


def _borderline(d, r, ri, si):
    """True if patch pair (ri, si) has a masked point pair within 1e-6 r^2 of r^2 (float64)."""
    R, t = d['transform'].double()[:3, :3], d['transform'].double()[:3, 3]
    a = _knn_points64(d['ref_points_f'], d['ref_knn'][ri], d['ref_knn_masks'][ri])[d['ref_knn_masks'][ri].bool()]
    b = _knn_points64(d['src_points_f'], d['src_knn'][si], d['src_knn_masks'][si])[d['src_knn_masks'][si].bool()] @ R.T + t
    d2 = ((a[:, None] - b[None]) ** 2).sum(-1)
    return bool(((d2 - r * r).abs() <= 1e-6 * r * r).any())


def _assert_lists_match(d, r, gi, go, want_i, want_o, context):
    """Same pairs in the same row-major order and overlaps within 1e-6, except for borderline patch pairs."""
    gi, go = gi.cpu().long(), go.cpu()
    want_i, want_o = torch.as_tensor(want_i).long(), torch.as_tensor(want_o).float()
    key = lambda i: (i[:, 0] * 1000003 + i[:, 1]).tolist()                   # noqa: E731
    assert (np.diff(key(gi)) > 0).all(), '%s: kernel list not in row-major order' % context
    got, want = dict(zip(key(gi), go.tolist())), dict(zip(key(want_i), want_o.tolist()))
    odd = [k for k in set(got) | set(want) if k not in got or k not in want or abs(got[k] - want[k]) > 1e-6]
    for k in odd:
        assert _borderline(d, r, k // 1000003, k % 1000003), '%s: patch pair %s differs (%s vs %s) without a borderline point pair' % (
            context, divmod(k, 1000003), got.get(k), want.get(k))
    assert len(odd) <= max(2, len(want) // 500), '%s: %d patch pairs differ' % (context, len(odd))


def test_gt_overlaps_match_reference_fixture(golden):
    """C2 pairs 0..7 as one B = 8 stack and the KITTI C3 pair (K = 128) against the reference's get_node_correspondences."""
    pairs = [_pair(golden, 'c2/p%d/' % i) for i in range(C2_PAIRS)]
    gt = _kernel_gt(pairs, 0.05)
    for i, (gi, go) in enumerate(gt.lists()):
        p = 'c2/p%d/' % i
        _assert_lists_match(pairs[i], 0.05, gi, go, golden[p + 'gt_node_corr_indices'], golden[p + 'gt_node_corr_overlaps'], p)
    k = _pair(golden, 'kitti/p0/')
    (gi, go), = _kernel_gt([k], 0.6).lists()
    _assert_lists_match(k, 0.6, gi, go, golden['kitti/p0/gt_node_corr_indices'], golden['kitti/p0/gt_node_corr_overlaps'], 'kitti')


def test_gt_overlaps_match_training_fixture(golden_dir):
    """The ground truth stored with the C2 training step (train_c2_se3ete_5k.npz), from this package's own pyramid and partition."""
    import os
    from se3et_amd import ops
    from se3et_amd.data import precompute_data_stack_mode
    g = np.load(os.path.join(golden_dir, 'train_c2_se3ete_5k.npz'))
    cfg = _cfg()
    b = cfg.backbone
    pts = torch.from_numpy(np.concatenate([g['ref'], g['src']], 0)).cuda()
    dd = precompute_data_stack_mode(pts, torch.tensor([len(g['ref']), len(g['src'])]), b.num_stages, b.init_voxel_size, b.init_radius, LIMITS)
    pf, pc = dd['points'][1], dd['points'][-1]
    lf, lc = dd['lengths'][1].tolist(), dd['lengths'][-1].tolist()
    _, nm, knn, km = ops.point_to_node_partition_stack(pf, pc, lf, lc, 64)
    T = torch.from_numpy(g['transform']).cuda()[None]
    (gi, go), = ops.gt_node_overlaps_stack(pf, pc, lc, knn, km, nm, T, 0.05).lists()
    d = dict(ref_points_f=pf[:lf[0]], src_points_f=pf[lf[0]:], ref_knn=knn[:lc[0]], src_knn=knn[lc[0]:] - lf[0],
             ref_knn_masks=km[:lc[0]], src_knn_masks=km[lc[0]:], transform=T[0])
    _assert_lists_match(d, 0.05, gi, go, g['gt_node_corr_indices'], g['gt_node_corr_overlaps'], 'train_c2')


def _random_pair(seed, n=3000, m=150, K=64):
    g = torch.Generator().manual_seed(seed)
    ref = torch.rand((n, 3), generator=g) * torch.tensor([1.0, 0.8, 0.3])
    src = torch.rand((n, 3), generator=g) * torch.tensor([1.0, 0.8, 0.3])
    a = float(torch.rand((), generator=g)) * 0.3
    T = torch.eye(4)
    T[:3, :3] = torch.tensor([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=torch.float32)
    T[:3, 3] = torch.rand(3, generator=g) * 0.1
    return ref.cuda(), src.cuda(), ref[torch.randperm(n, generator=g)[:m]].cuda(), src[torch.randperm(n, generator=g)[:m]].cuda(), T.cuda()


def test_gt_overlaps_match_training_node_correspondences():
    """Kernel against se3et_amd.training.node_correspondences (plain torch) on 8 seeded random cloud pairs, same device inputs."""
    from se3et_amd import functional as SF
    from se3et_amd import ops
    from se3et_amd.training import node_correspondences
    r = 0.05
    pairs = []
    for s in range(8):
        ref_f, src_f, ref_c, src_c, T = _random_pair(s)
        d = dict(ref_points_f=ref_f, src_points_f=src_f, ref_points_c=ref_c, src_points_c=src_c, transform=T)
        for side, f, c in (('ref', ref_f, ref_c), ('src', src_f, src_c)):
            _, nm, knn, km = ops.point_to_node_partition_stack(f, c, [f.shape[0]], [c.shape[0]], 64)
            d[side + '_node_masks'], d[side + '_knn'], d[side + '_knn_masks'] = nm, knn, km
        pairs.append(d)
    gt = _kernel_gt(pairs, r)
    for s, (d, (gi, go)) in enumerate(zip(pairs, gt.lists())):
        rk = SF.gather_rows_padded(d['ref_points_f'], d['ref_knn'])
        sk = SF.gather_rows_padded(d['src_points_f'], d['src_knn'])
        wi, wo = node_correspondences(d['ref_points_c'], d['src_points_c'], rk, sk, d['transform'], r, d['ref_node_masks'],
                                      d['src_node_masks'], d['ref_knn_masks'], d['src_knn_masks'])
        assert wi.shape[0] > 50, 'pair %d: too few overlapping patches to test anything' % s
        _assert_lists_match(d, r, gi, go, wi.cpu(), wo.cpu(), 'random pair %d' % s)


def _outs(g, prefixes, kitti=False):
    """Output dicts of the fixture's pairs: reference ground truth and seeded predictions."""
    outs = []
    for p in prefixes:
        t = lambda k: torch.from_numpy(np.asarray(g[p + k])).cuda()           # noqa: E731
        d = _pair(g, p)
        out = {k: d[k] for k in ('ref_points_c', 'src_points_c', 'src_points')}
        out.update({k: t(k) for k in ('ref_node_corr_indices', 'src_node_corr_indices', 'ref_corr_points', 'src_corr_points',
                                      'estimated_transform')})
        out['gt_node_corr_indices'] = t('gt_node_corr_indices').long()
        out['gt_node_corr_overlaps'] = t('gt_node_corr_overlaps')
        for k in ('ref_node_corr_indices', 'src_node_corr_indices'):
            out[k] = out[k].long()
        outs.append(out)
    return outs


def _assert_metrics(got, g, prefix, context):
    for k in got:
        a, w = float(got[k]), float(g[prefix + 'metric/' + k])
        if np.isnan(w):
            assert np.isnan(a), '%s %s: %r, want NaN' % (context, k, a)
            continue
        assert not np.isnan(a), '%s %s: NaN, want %r' % (context, k, w)
        if k in ('PIR', 'IR', 'RR'):
            assert a == w, '%s %s: %r vs %r' % (context, k, a, w)          # ratios of counts: exact
        elif k == 'RRE':
            # acos of a float32 trace near 1 resolves no better than ~0.03 degrees (d acos / dx ~ 1 / sqrt(2 (1 - x)), x rounded to 6e-8)
            assert abs(a - w) <= 0.05, '%s RRE: %r vs %r' % (context, a, w)
        else:
            # (RMSE of an exact estimate: the reference's torch.inverse leaves ~1e-7 of residue, hence the absolute floor)
            assert abs(a - w) <= 1e-5 * abs(w) + 1e-6, '%s %s: %r vs %r' % (context, k, a, w)


def test_metrics_match_reference_fixture(golden):
    from se3et_amd.evaluation import evaluate_pairs
    cfg = _cfg()
    prefixes = ['c2/p%d/' % i for i in range(C2_PAIRS)]
    outs = _outs(golden, prefixes)
    T = torch.stack([torch.from_numpy(golden[p + 'transform']) for p in prefixes]).cuda()
    res = evaluate_pairs(cfg, outs, T)
    assert set(res) == {'PIR', 'IR', 'RRE', 'RTE', 'RMSE', 'RR'}
    for i, p in enumerate(prefixes):
        _assert_metrics({k: v[i] for k, v in res.items()}, golden, p, p)
    kc = _cfg(kitti=True)
    res = evaluate_pairs(kc, _outs(golden, ['kitti/p0/']), torch.from_numpy(golden['kitti/p0/transform']).cuda()[None])
    assert set(res) == {'PIR', 'IR', 'RRE', 'RTE', 'RR'}
    _assert_metrics({k: v[0] for k, v in res.items()}, golden, 'kitti/p0/', 'kitti')
    # edge cases through the single-pair Evaluator
    from se3et_amd.evaluation import Evaluator
    ev = Evaluator(cfg)
    for name in ('no_pred', 'no_corr', 'exact', 'flip', 'no_gt'):
        p = 'edge/%s/' % name
        d = _pair(golden, 'edge/')
        out = {k: d[k] for k in ('ref_points_c', 'src_points_c', 'src_points')}
        out['gt_node_corr_indices'] = torch.from_numpy(golden['edge/gt_node_corr_indices']).cuda().long()
        out['gt_node_corr_overlaps'] = torch.from_numpy(golden['edge/gt_node_corr_overlaps']).cuda()
        if name == 'no_gt':     # the far-away ground truth: recomputed by the kernel from the points (no correspondences)
            for k in ('gt_node_corr_indices', 'gt_node_corr_overlaps'):
                out.pop(k)
            for k in ('ref_points_f', 'src_points_f'):
                out[k] = d[k]
        for k in ('ref_node_corr_indices', 'src_node_corr_indices', 'ref_corr_points', 'src_corr_points', 'estimated_transform'):
            out[k] = torch.from_numpy(np.asarray(golden[p + k])).cuda()
            if 'indices' in k:
                out[k] = out[k].long()
        got = ev(out, {'transform': torch.from_numpy(golden[p + 'transform']).cuda()})
        assert all(v.dim() == 0 for v in got.values())
        _assert_metrics(got, golden, p, name)


def test_batch_independence_and_determinism(golden):
    """Pair p's ground-truth lists and metric row are bitwise the same alone (B = 1), inside the B = 8 stack, and in a second run."""
    from se3et_amd.evaluation import evaluate_pairs
    cfg = _cfg()
    prefixes = ['c2/p%d/' % i for i in range(C2_PAIRS)]
    pairs = [_pair(golden, p) for p in prefixes]
    T = torch.stack([d['transform'] for d in pairs]).float()

    def run(idx):
        gt = _kernel_gt([pairs[i] for i in idx], 0.05)
        outs = _outs(golden, [prefixes[i] for i in idx])
        for p, o in enumerate(outs):
            for k in ('gt_node_corr_indices', 'gt_node_corr_overlaps'):
                o.pop(k)
            o['gt_node_corr_overlap_map'] = gt.block(p)
        rows = evaluate_pairs(cfg, outs, T[idx])
        return gt.lists(), torch.stack([rows[k] for k in ('PIR', 'IR', 'RRE', 'RTE', 'RMSE', 'RR')], 1).cpu()

    all8, rows8 = run(list(range(C2_PAIRS)))
    again, rows8b = run(list(range(C2_PAIRS)))
    assert torch.equal(rows8, rows8b)
    for p in range(C2_PAIRS):
        assert torch.equal(all8[p][0], again[p][0]) and torch.equal(all8[p][1], again[p][1])
        one, row1 = run([p])
        assert torch.equal(one[0][0], all8[p][0]) and torch.equal(one[0][1].view(torch.int32), all8[p][1].view(torch.int32)), p
        assert torch.equal(row1[0].view(torch.int32), rows8[p].view(torch.int32)), p


def _demo_model_and_data(golden_dir):
    import os
    from se3et_amd.data import precompute_data_stack_mode
    from se3et_amd.model import create_model, load_synthetic_weights
    g = np.load(os.path.join(golden_dir, 'demo_se3ete.npz'))
    cfg = _cfg()
    model = load_synthetic_weights(create_model(cfg), int(g['synth_seed'])).cuda().eval()
    b = cfg.backbone
    pts = torch.from_numpy(np.concatenate([g['ref'], g['src']], 0)).cuda()
    dd = precompute_data_stack_mode(pts, torch.tensor([len(g['ref']), len(g['src'])]), b.num_stages, b.init_voxel_size, b.init_radius, LIMITS)
    dd['features'] = torch.ones((pts.shape[0], 1), device='cuda')
    dd['transform'] = torch.from_numpy(g['transform']).cuda()
    return cfg, model, dd


def test_demo_pair_end_to_end(golden, golden_dir):
    """data/demo through both paths: model(dd) + Evaluator (ground truth recomputed from the points) and forward_pairs(ground_truth=True)
    + evaluate_pairs; the two agree with each other and with the reference's Evaluator on its own forward."""
    from se3et_amd.batched import forward_pairs
    from se3et_amd.evaluation import Evaluator, evaluate_pairs
    cfg, model, dd = _demo_model_and_data(golden_dir)
    with torch.no_grad():
        out = model(dd)
    assert 'gt_node_corr_indices' not in out
    single = Evaluator(cfg)(out, dd)
    dd_b = dict(dd)
    dd_b['transform'] = dd['transform'][None]
    outs = forward_pairs(model, dd_b, ground_truth=True)
    assert outs[0]['gt_node_corr_indices'].shape[1] == 2 and outs[0]['gt_node_corr_overlaps'].shape[0] == outs[0]['gt_node_corr_indices'].shape[0]
    batched = {k: v[0] for k, v in evaluate_pairs(cfg, outs, dd_b['transform']).items()}
    for k in single:
        a, b = float(single[k]), float(batched[k])
        if k in ('PIR', 'IR', 'RR'):
            assert a == b, '%s: %r vs %r' % (k, a, b)
        else:
            assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), '%s: %r vs %r' % (k, a, b)
    n_pred, n_corr = int(golden['demo/num_node_corr']), int(golden['demo/num_corr'])
    for k in single:
        a, w = float(single[k]), float(golden['demo/metric/' + k])
        if k == 'RR':
            assert a == w
        elif k == 'PIR':        # the knn3 tie residue of test_gpu_demo_pair.py may move one node correspondence
            assert abs(a - w) <= 1.0 / n_pred + 1e-7, 'PIR %r vs %r' % (a, w)
        elif k == 'IR':
            assert abs(a - w) <= 1.0 / n_corr + 1e-7, 'IR %r vs %r' % (a, w)
        else:
            assert abs(a - w) <= 1e-3 * abs(w), '%s: %r vs %r' % (k, a, w)


def _stacked_data(cfg, pairs):
    """Pyramid of B pairs stacked ref0, src0, ref1, src1, ... (as bench.py builds it) with their (B, 4, 4) transforms."""
    from se3et_amd.data import precompute_data_stack_mode
    clouds = [c for ref, src, _ in pairs for c in (ref, src)]
    pts = torch.from_numpy(np.concatenate(clouds, 0)).cuda()
    b = cfg.backbone
    dd = precompute_data_stack_mode(pts, torch.tensor([len(c) for c in clouds]), b.num_stages, b.init_voxel_size, b.init_radius,
                                    cfg.neighbor_limits)
    dd['features'] = torch.ones((pts.shape[0], 1), device='cuda')
    dd['transform'] = torch.from_numpy(np.stack([T for _, _, T in pairs])).cuda()
    return dd


def test_forward_pairs_default_has_no_ground_truth():
    from se3et_amd.batched import forward_pairs
    from se3et_amd.model import create_model, load_synthetic_weights, make_cfg
    from se3et_amd.synthetic import make_pair
    cfg = make_cfg('micro_e')
    model = load_synthetic_weights(create_model(cfg)).cuda().eval()
    data = _stacked_data(cfg, [make_pair('micro', 0), make_pair('micro', 1)])
    outs = forward_pairs(model, data)
    assert len(outs) == 2
    for out in outs:
        assert not any(k.startswith('gt_') for k in out), sorted(out)
