"""GPU: eval.py's benchmark metrics (se3et_amd.benchmark, csrc/benchmark.hip) against the reference's values stored in
tests/golden/benchmark_metrics.npz, on all 1 623 + 1 781 3DMatch / 3DLoMatch pairs and the 555 KITTI pairs (inputs redrawn by
tests/benchmark_fixture.py and checked against the stored checksums first).

The fixture's correspondence sets keep every distance test at least benchmark_fixture.MARGIN r^2 away from r^2 in float64, so the float32
overlap test of the kernel and the reference's float64 test count the same points: the counts must be exactly equal."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from benchmark_fixture import inputs_checksum, pair_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, 'golden', 'benchmark_metrics.npz')
BENCHMARKS = ('3DMatch', '3DLoMatch', 'KITTI')
RADIUS = {'3DMatch': 0.1, '3DLoMatch': 0.1, 'KITTI': 1.0}


def _cfg(benchmark):
    from se3et_amd.model import make_cfg
    return make_cfg('se3eti_kitti' if benchmark == 'KITTI' else 'se3ete')


@pytest.fixture(scope='module')
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def inputs(gold):
    out = {}
    for b in BENCHMARKS:
        T, att, sums = gold[b + '/transform'], gold[b + '/attempt'], gold[b + '/checksum']
        pairs = []
        for i in range(len(T)):
            d = pair_inputs(b, i, int(att[i]), T[i], RADIUS[b])
            assert inputs_checksum(d) == sums[i], (b, i)
            pairs.append(d)
        out[b] = pairs
    return out


def _fine(pairs, T, r):
    from se3et_amd.benchmark import evaluate_correspondences_pairs
    return evaluate_correspondences_pairs([d['ref_corr_points'] for d in pairs], [d['src_corr_points'] for d in pairs], T, r)


def _sparse(pairs):
    from se3et_amd.benchmark import evaluate_sparse_correspondences_pairs
    return evaluate_sparse_correspondences_pairs([d['ref_node_corr_indices'] for d in pairs], [d['src_node_corr_indices'] for d in pairs],
                                                 [d['gt_node_corr_indices'] for d in pairs], [d['num_ref_nodes'] for d in pairs],
                                                 [d['num_src_nodes'] for d in pairs])


def _transform(gold, b, idx=None):
    from se3et_amd.benchmark import compute_transform_error_pairs
    idx = np.arange(len(gold[b + '/transform'])) if idx is None else np.asarray(idx)
    covs = None if b == 'KITTI' else [gold[b + '/covariance'][i] if gold[b + '/is_gt'][i] else None for i in idx]
    return compute_transform_error_pairs(gold[b + '/transform'][idx], covs, gold[b + '/estimated'][idx])


@pytest.fixture(scope='module')
def full(gold, inputs):
    """Every metric of every pair, each benchmark in one batched call per kernel, host copies."""
    out = {}
    for b in BENCHMARKS:
        f = _fine(inputs[b], gold[b + '/transform'], RADIUS[b])
        s = _sparse(inputs[b])
        t = _transform(gold, b)
        out[b] = {k: v.cpu().numpy() for k, v in list(f.items()) + list(s.items()) + list(t.items())}
    return out


@pytest.mark.parametrize('b', BENCHMARKS)
def test_fine_metrics_of_every_pair(gold, full, b):
    got, p = full[b], b + '/ref/'
    n = gold[p + 'num_corr']
    np.testing.assert_array_equal(got['num_corr'], n.astype(np.int64))
    # counts: exactly equal (the fixture keeps every test MARGIN r^2 away from the radius)
    np.testing.assert_array_equal(np.rint(got['overlap'] * n), np.rint(gold[p + 'overlap'] * n))
    np.testing.assert_array_equal(np.rint(got['inlier_ratio'] * n), np.rint(gold[p + 'inlier_ratio'] * n))
    np.testing.assert_array_equal(got['overlap'], gold[p + 'overlap'])
    np.testing.assert_array_equal(got['inlier_ratio'], gold[p + 'inlier_ratio'])
    np.testing.assert_allclose(got['residual'], gold[p + 'residual'], rtol=1e-6, atol=0)
    assert n.max() >= 20000 and n.min() < 100


@pytest.mark.parametrize('b', BENCHMARKS)
def test_sparse_metrics_are_exact(gold, full, b):
    for k in ('precision', 'recall', 'hit_ratio'):
        np.testing.assert_array_equal(full[b][k], gold[b + '/ref/' + k], err_msg=k)


@pytest.mark.parametrize('b', BENCHMARKS)
def test_transform_error(gold, full, b):
    got, p = full[b], b + '/ref/'
    np.testing.assert_allclose(got['rre'], gold[p + 'rre'], rtol=0, atol=1e-4)
    np.testing.assert_allclose(got['rte'], gold[p + 'rte'], rtol=0, atol=1e-4)
    if b == 'KITTI':
        assert np.isnan(got['err']).all()
        acc_got = (got['rre'] < 5.0) & (got['rte'] < 2.0)
        acc_want = (gold[p + 'rre'] < 5.0) & (gold[p + 'rte'] < 2.0)
    else:
        gt = gold[b + '/is_gt'].astype(bool)
        assert np.isnan(got['err'][~gt]).all() and np.isnan(gold[p + 'err'][~gt]).all()
        np.testing.assert_allclose(got['err'][gt], gold[p + 'err'][gt], rtol=1e-6, atol=0)
        acc_got, acc_want = gt & (got['err'] < 0.2 ** 2), gt & (gold[p + 'err'] < 0.2 ** 2)
    np.testing.assert_array_equal(acc_got, acc_want)
    assert 0 < acc_want.sum() < len(acc_want)


def _records(gold, inputs, b):
    p = b + '/'
    recs = []
    for i, d in enumerate(inputs[b]):
        rec = {k: torch.from_numpy(np.asarray(d[k])).cuda() for k in ('ref_corr_points', 'src_corr_points', 'corr_scores',
                                                                         'ref_node_corr_indices', 'src_node_corr_indices',
                                                                         'gt_node_corr_indices')}
        rec.update(num_ref_nodes=d['num_ref_nodes'], num_src_nodes=d['num_src_nodes'],
                   transform=torch.from_numpy(gold[p + 'transform'][i]).cuda(),
                   estimated_transform=torch.from_numpy(gold[p + 'estimated'][i]).cuda())
        if b != 'KITTI':
            rec.update(test_pair=[int(v) for v in gold[p + 'ids'][i]], num_fragments=int(gold[p + 'num_fragments'][i]),
                       covariance=gold[p + 'covariance'][i] if gold[p + 'is_gt'][i] else None)
        recs.append(rec)
    groups = [(str(s), int(n)) for s, n in zip(gold[p + 'scenes'], gold[p + 'group_lengths'])]
    return recs, groups


def _numbers(lines):
    return [[float(v) for v in re.findall(r': (-?[0-9.]+|nan)', line)] for line in lines if not line.startswith('  Timer')]


def _check_summary(res, gold, b):
    from se3et_amd.benchmark import SUMMARY_KEYS, format_summary
    p = b + '/summary/'
    groups = np.array([[res['groups'][str(s)][k] for k in SUMMARY_KEYS] for s in gold[b + '/scenes']])
    np.testing.assert_allclose(groups, gold[p + 'groups'], rtol=1e-6, atol=0, equal_nan=True)
    np.testing.assert_allclose([res['overall'][k] for k in SUMMARY_KEYS], gold[p + 'overall'], rtol=1e-6, atol=0, equal_nan=True)
    got, want = _numbers(format_summary(res, b)), _numbers(list(gold[p + 'critical_lines']))
    assert got == want


@pytest.mark.parametrize('b', BENCHMARKS)
def test_summaries_match_eval_one_epoch(gold, inputs, b):
    from se3et_amd.benchmark import BenchmarkEvaluator
    recs, groups = _records(gold, inputs, b)
    res = BenchmarkEvaluator(_cfg(b), b).evaluate(recs, groups, 'lgr')
    _check_summary(res, gold, b)
    assert res['pairs']['PIR'].shape == (len(recs),)


def _write_gt(root, gold, b):
    """gt.log / gt.info per scene from the stored (float32) arrays, in the documented 5- / 7-line record formats."""
    p, a = b + '/', 0
    for s, n in zip(gold[p + 'scenes'], gold[p + 'group_lengths']):
        os.makedirs(os.path.join(root, str(s)), exist_ok=True)
        with open(os.path.join(root, str(s), 'gt.log'), 'w') as fl, open(os.path.join(root, str(s), 'gt.info'), 'w') as fi:
            for i in range(a, a + n):
                head = '%d\t%d\t%d\n' % (gold[p + 'ids'][i][0], gold[p + 'ids'][i][1], gold[p + 'num_fragments'][i])
                fl.write(head + ''.join('\t'.join(repr(float(v)) for v in row) + '\n' for row in gold[p + 'transform'][i]))
                fi.write(head + ''.join('\t'.join(repr(float(v)) for v in row) + '\n' for row in gold[p + 'covariance'][i]))
        a += n


def _write_features(root, gold, inputs, b):
    p = b + '/'
    a = 0
    for s, n in zip(gold[p + 'scenes'], gold[p + 'group_lengths']):
        for i in range(a, a + n):
            d = inputs[b][i]
            name = '_'.join(str(int(v)) for v in gold[p + 'ids'][i]) + '.npz'
            path = os.path.join(root, name) if b == 'KITTI' else os.path.join(root, str(s), name)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.savez(path, ref_points_c=np.zeros((d['num_ref_nodes'], 3), np.float32), src_points_c=np.zeros((d['num_src_nodes'], 3), np.float32),
                     ref_node_corr_indices=d['ref_node_corr_indices'], src_node_corr_indices=d['src_node_corr_indices'],
                     ref_corr_points=d['ref_corr_points'], src_corr_points=d['src_corr_points'], corr_scores=d['corr_scores'],
                     gt_node_corr_indices=d['gt_node_corr_indices'], transform=gold[p + 'transform'][i],
                     estimated_transform=gold[p + 'estimated'][i], overlap=np.float32(0.5))
        a += n


@pytest.mark.parametrize('b', ('3DLoMatch', 'KITTI'))
def test_feature_tree_front_end_and_cli(gold, inputs, b, tmp_path, capsys):
    from se3et_amd import benchmark
    feats, gt_root, est_dir = str(tmp_path / 'features'), str(tmp_path / 'gt'), str(tmp_path / 'est')
    _write_features(feats, gold, inputs, b)
    if b != 'KITTI':
        _write_gt(gt_root, gold, b)
    res = benchmark.BenchmarkEvaluator(_cfg(b), b).evaluate_features(feats, gt_root if b != 'KITTI' else None, 'lgr',
                                                                     est_log_dir=est_dir)
    _check_summary(res, gold, b)
    if b != 'KITTI':
        scene = str(gold[b + '/scenes'][0])
        logs = benchmark.read_log_file(os.path.join(est_dir, scene, 'est.log'))
        n = int(gold[b + '/group_lengths'][0])
        np.testing.assert_array_equal(np.stack([r['transform'] for r in logs]), gold[b + '/estimated'][:n])
    args = ['--features', feats, '--benchmark', b, '--method', 'lgr', '--json'] + (['--gt-root', gt_root] if b != 'KITTI' else [])
    assert benchmark.main(args) == 0
    lines = capsys.readouterr().out.splitlines()
    assert _numbers(lines[:-1]) == _numbers(list(gold[b + '/summary/critical_lines']))
    assert '"overall"' in lines[-1]


def test_evaluate_registration_log(gold, tmp_path):
    from se3et_amd.benchmark import evaluate_registration_log
    _write_gt(str(tmp_path / 'gt'), gold, '3DMatch')
    scene = str(gold['est_log/scene'])
    est = tmp_path / 'est.log'
    est.write_text(str(gold['est_log/text']))
    res = evaluate_registration_log(str(tmp_path / 'gt' / scene), str(est))
    for k in ('num_pos_pairs', 'num_pred_pairs', 'num_gt_pairs'):
        assert res[k] == int(gold['est_log/' + k]), k
    # evaluate_registration_one_scene computes in float32 from the log's float32 values (measured: up to 5.5e-6 relative from the float64
    # twin on this scene); the acceptance counts above are exact, no error lies within 0.4 % of the threshold
    for k in ('precision', 'recall'):
        assert res[k] == gold['est_log/' + k], k
    for k in ('mean_rre', 'mean_rte', 'median_rre', 'median_rte'):
        np.testing.assert_allclose(res[k], gold['est_log/' + k], rtol=0, atol=1e-4, err_msg=k)
    np.testing.assert_allclose([e['error'] for e in res['errors']], gold['est_log/errors'], rtol=2e-5)


def test_rows_do_not_depend_on_the_batch(gold, inputs, full):
    """A pair's row is bit-identical alone, in a batch of 16, in the full benchmark batch, and from run to run."""
    b = '3DMatch'
    T = gold[b + '/transform']
    for i in (0, 199, 777):
        lo = min(max(i - 5, 0), len(T) - 16)
        sel = list(range(lo, lo + 16))
        for idx in ([i], sel):
            f = _fine([inputs[b][j] for j in idx], T[idx], RADIUS[b])
            s = _sparse([inputs[b][j] for j in idx])
            t = _transform(gold, b, idx)
            k = idx.index(i)
            for name, v in list(f.items()) + list(s.items()) + list(t.items()):
                a, w = v[k].cpu().numpy(), full[b][name][i]
                assert a.tobytes() == np.asarray(w).tobytes(), (i, len(idx), name)
    again = _fine(inputs[b], T, RADIUS[b])
    for name, v in again.items():
        assert v.cpu().numpy().tobytes() == full[b][name].tobytes(), name


def test_edge_cases():
    from se3et_amd import ops
    from se3et_amd.benchmark import (BenchmarkEvaluator, evaluate_correspondences_pairs, evaluate_sparse_correspondences_pairs,
                                     MAX_GROUP_PAIRS)
    eye = np.eye(4, dtype=np.float32)
    pts = np.random.default_rng(3).uniform(-1, 1, (50, 3)).astype(np.float32)
    # no correspondences: IR, OV and the residual are NaN (np.mean of an empty array in the reference)
    f = evaluate_correspondences_pairs([np.zeros((0, 3), np.float32), pts], [np.zeros((0, 3), np.float32), pts], np.stack([eye, eye]), 0.1)
    assert math.isnan(float(f['overlap'][0])) and math.isnan(float(f['inlier_ratio'][0])) and math.isnan(float(f['residual'][0]))
    assert int(f['num_corr'][0]) == 0
    assert float(f['overlap'][1]) == 1.0 and float(f['inlier_ratio'][1]) == 1.0 and float(f['residual'][1]) == 0.0
    # no predicted node pairs: precision 0 / (0 + 1e-12) = 0; duplicates count once
    s = evaluate_sparse_correspondences_pairs([[], [1, 1, 2]], [[], [0, 0, 0]], [[[1, 0], [3, 3]], [[1, 0], [1, 0], [3, 3]]], [5, 5], [4, 4])
    half = 1 / (2 + 1e-12)
    assert s['precision'].tolist() == [0.0, half] and s['recall'].tolist() == [0.0, half]
    assert s['hit_ratio'].tolist() == [0.0, 0.5 * (half + half)]
    # an empty group gives NaN; a group over the limit is refused
    rows = torch.zeros((3, 6), dtype=torch.float64, device='cuda')
    g, o = ops.benchmark_summary(rows, torch.ones(3, dtype=torch.int32, device='cuda'), [3, 0], False, 0.05, 0.2, 0, 0)
    g = g.cpu().numpy()
    assert np.isnan(g[1]).all() and g[0][0] == 0.0 and g[0][9] == 1.0
    assert np.isnan(o.cpu().numpy()[0])                      # the mean over scenes includes the empty one (np.mean of NaN)
    big = torch.zeros((MAX_GROUP_PAIRS + 1, 6), dtype=torch.float64, device='cuda')
    with pytest.raises(RuntimeError, match='4096'):
        ops.benchmark_summary(big, torch.zeros(MAX_GROUP_PAIRS + 1, dtype=torch.int32, device='cuda'), [MAX_GROUP_PAIRS + 1], False,
                              0.05, 0.2, 0, 0)
    with pytest.raises(ValueError):
        BenchmarkEvaluator(_cfg('KITTI'), 'KITTI').evaluate([{}] * (MAX_GROUP_PAIRS + 1), [('all', MAX_GROUP_PAIRS + 1)])
    with pytest.raises(RuntimeError, match='GPU'):
        ops.benchmark_summary(rows.cpu(), torch.ones(3, dtype=torch.int32), [3], False, 0.05, 0.2, 0, 0)


@pytest.fixture(scope='module')
def c2_outputs():
    from se3et_amd.batched import forward_pairs
    from se3et_amd.data import precompute_data_stack_mode
    from se3et_amd.model import create_model, load_synthetic_weights, make_cfg
    from se3et_amd.synthetic import make_pair
    cfg = make_cfg('se3ete')
    model = load_synthetic_weights(create_model(cfg)).cuda().eval()
    b = cfg.backbone
    clouds, Ts = [], []
    for i in range(8):
        ref, src, T = make_pair('c2_5k', i)
        clouds += [ref, src]
        Ts.append(T)
    pts = torch.from_numpy(np.concatenate(clouds, 0)).cuda()
    data = precompute_data_stack_mode(pts, torch.tensor([len(c) for c in clouds]), b.num_stages, b.init_voxel_size, b.init_radius,
                                      cfg.neighbor_limits)
    data['features'] = torch.ones((pts.shape[0], 1), device='cuda')
    data['transform'] = torch.from_numpy(np.stack(Ts)).cuda()
    with torch.no_grad():
        outs = forward_pairs(model, data, ground_truth=True)
    return cfg, outs, data['transform']


def test_end_to_end_on_forward_pairs(c2_outputs):
    from se3et_amd.benchmark import (BenchmarkEvaluator, compute_transform_error_pairs, evaluate_correspondences_pairs,
                                     evaluate_sparse_correspondences_pairs)
    from se3et_amd.evaluation import evaluate_pairs
    from se3et_amd.ransac import register_pairs, select_correspondences
    cfg, outs, gt = c2_outputs
    est = register_pairs(cfg, outs, 'ransac', 250)
    res = BenchmarkEvaluator(cfg, '3DMatch').evaluate_outputs(outs, gt, 'ransac', num_corr=250)
    assert torch.equal(res['pairs']['estimated_transform'], est)
    for p, out in enumerate(outs):
        r, s, _ = select_correspondences(out, 250)
        f = evaluate_correspondences_pairs([r], [s], gt[p:p + 1], cfg.eval.acceptance_radius)
        sp = evaluate_sparse_correspondences_pairs([out['ref_node_corr_indices']], [out['src_node_corr_indices']],
                                                   [out['gt_node_corr_indices']], [out['ref_points_c'].shape[0]],
                                                   [out['src_points_c'].shape[0]])
        t = compute_transform_error_pairs(gt[p:p + 1], None, est[p:p + 1])
        for mine, theirs in ((res['pairs']['IR'], f['inlier_ratio']), (res['pairs']['OV'], f['overlap']),
                             (res['pairs']['residual'], f['residual']), (res['pairs']['PIR'], sp['precision']),
                             (res['pairs']['hit_ratio'], sp['hit_ratio']), (res['pairs']['RRE'], t['rre']), (res['pairs']['RTE'], t['rte'])):
            assert mine[p].cpu().numpy().tobytes() == theirs[0].cpu().numpy().tobytes()
    # where the definitions coincide (acceptance_overlap 0, unique node pairs): the Evaluator's PIR and IR
    assert cfg.eval.acceptance_overlap == 0.0
    for out, T in zip(outs, est):
        out['estimated_transform'] = T
    ev = evaluate_pairs(cfg, outs, gt)
    cut = [dict(out, **dict(zip(('ref_corr_points', 'src_corr_points', 'corr_scores'), select_correspondences(out, 250)))) for out in outs]
    ev_cut = evaluate_pairs(cfg, cut, gt)
    np.testing.assert_allclose(res['pairs']['PIR'].cpu().numpy(), ev['PIR'].double().cpu().numpy(), rtol=0, atol=1e-7)
    np.testing.assert_allclose(res['pairs']['IR'].cpu().numpy(), ev_cut['IR'].double().cpu().numpy(), rtol=0, atol=1e-7)
    one = res['groups']['all']
    assert math.isnan(one['RR'])                             # no covariances: no 3DMatch benchmark pairs
    assert one['PIR'] == pytest.approx(float(res['pairs']['PIR'].mean()), rel=1e-12)
    kitti = BenchmarkEvaluator(cfg, 'KITTI').evaluate_outputs(outs, gt, estimated=est)
    e = cfg.eval
    acc = ((res['pairs']['RRE'] < e.rre_threshold) & (res['pairs']['RTE'] < e.rte_threshold)).double().mean().item()
    assert kitti['overall']['RR'] == pytest.approx(acc, rel=1e-12)
