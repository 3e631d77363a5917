"""Fixture generator of eval.py's benchmark metrics (runs ONLY where the reference tree exists; data only travels).

Imports the genuine reference through oracle/ref_shims.py (geotransformer.engine, which needs tensorboard, is replaced by a module that
only holds the capturing logger eval_one_epoch is called with).  nibabel is not installed here, so a minimal nibabel.quaternions stand-in is put
into sys.modules before datasets/registration/threedmatch/utils.py is imported: mat2quat by the published algorithm (Bar-Itzhack 2000, as
nibabel implements it: the eigenvector of the symmetric 4x4 K for its largest eigenvalue by numpy.linalg.eigh, sign so that w >= 0).

Writes tests/golden/benchmark_metrics.npz:
  <b>/...        for b in 3DMatch, 3DLoMatch (all 8 scenes, from the reference's read_log_file / read_info_file of gt.log / gt.info) and
                 KITTI (the 555 pairs of data/Kitti/metadata/test.pkl): per pair, in eval.py's order, the ids, ground truth (float32),
                 covariance and benchmark flag, the estimated transform (float32, perturbed from the ground truth), the redraw attempt and
                 input checksum of tests/benchmark_fixture.py, and the reference's evaluate_correspondences,
                 evaluate_sparse_correspondences, compute_transform_error and compute_registration_error outputs;
  <b>/summary/*  the genuine eval_one_epoch of the experiment's eval.py with --method lgr over a temporary feature tree in test.py's
                 format: its critical lines, and the full-precision per-scene and overall values of a float64 restatement of its
                 summary code (3DMatch eval.py:240-357, KITTI eval.py:84-185) from the reference's per-pair values;
  raw/*          a few gt.log / gt.info records verbatim with the reference's parse;
  est_log/*      the reference's write_log_file text of one scene's estimates and evaluate_registration_one_scene on it.
The feature tree holds the float32 inputs promoted to float64, so the reference computes every per-pair value in float64; the estimated
transforms are redrawn until no err / RRE / RTE lies within 1e-3 relative of its threshold, and the correspondence sets until no distance
test lies within benchmark_fixture.MARGIN r^2 of r^2.
Re-run with:  python tests/golden/generate_benchmark_golden.py"""
import importlib.util
import math
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_shims  # noqa: E402
from benchmark_fixture import MARGIN, inputs_checksum, pair_inputs  # noqa: E402

OUT = os.path.join(HERE, 'benchmark_metrics.npz')
DATA = os.path.join(ref_shims.REFERENCE_ROOT, 'data')


def _mat2quat(M):
    Qxx, Qyx, Qzx, Qxy, Qyy, Qzy, Qxz, Qyz, Qzz = np.asarray(M).flat
    K = np.array([[Qxx - Qyy - Qzz, 0, 0, 0],
                  [Qyx + Qxy, Qyy - Qxx - Qzz, 0, 0],
                  [Qzx + Qxz, Qzy + Qyz, Qzz - Qxx - Qyy, 0],
                  [Qyz - Qzy, Qzx - Qxz, Qxy - Qyx, Qxx + Qyy + Qzz]]) / 3.0
    vals, vecs = np.linalg.eigh(K)
    q = vecs[[3, 0, 1, 2], np.argmax(vals)]
    if q[0] < 0:
        q *= -1
    return q


def _install_nibabel():
    nib = types.ModuleType('nibabel')
    nq = types.ModuleType('nibabel.quaternions')
    nq.mat2quat = _mat2quat
    nib.quaternions = nq
    sys.modules['nibabel'], sys.modules['nibabel.quaternions'] = nib, nq


def _load_eval(experiment):
    make_cfg, _ = ref_shims.load_experiment(experiment)
    path = os.path.join(ref_shims.REFERENCE_ROOT, 'experiments', experiment, 'eval.py')
    # eval.py imports Logger from geotransformer.engine, whose trainers need tensorboard (not installed); the logger is passed in
    if 'geotransformer.engine' not in sys.modules:
        sys.modules['geotransformer.engine'] = types.SimpleNamespace(Logger=_Capture)
    spec = importlib.util.spec_from_file_location('ref_eval_' + experiment.replace('.', '_'), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return make_cfg(), mod


class _Capture:
    def __init__(self):
        self.lines = []

    def critical(self, msg):
        self.lines.append(msg)

    def info(self, msg):
        pass


def _rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def _near(x, thr):
    return abs(x - thr) <= 1e-3 * thr


def _estimate(rng, T, kitti, cov, ref_utils, reg_err):
    """A float32 estimate perturbed from T, redrawn until no tested error lies within 1e-3 relative of its threshold."""
    while True:
        ang = math.radians(rng.uniform(0, 10 if kitti else 20))
        D = np.eye(4)
        D[:3, :3] = _rotation(rng.normal(size=3), ang)
        D[:3, 3] = rng.normal(size=3) / math.sqrt(3) * rng.uniform(0, 4.0 if kitti else 0.4)
        E = (np.asarray(T, np.float64) @ D).astype(np.float32)
        rre, rte = reg_err(T.astype(np.float64), E.astype(np.float64))
        if kitti:
            if not (_near(rre, 5.0) or _near(rte, 2.0)):
                return E
            continue
        if cov is None or not _near(ref_utils.compute_transform_error(T.astype(np.float64), cov.astype(np.float64),
                                                                     E.astype(np.float64)), 0.04):
            return E


def _margin_ok(d, T, r):
    from scipy.spatial import cKDTree
    T = np.asarray(T, np.float64)
    ref = d['ref_corr_points'].astype(np.float64)
    moved = d['src_corr_points'].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    d2 = ((ref - moved) ** 2).sum(1)
    nn = cKDTree(moved).query(ref, k=1)[0] ** 2
    r2 = r * r
    return np.all(np.abs(d2 - r2) > MARGIN * r2) and np.all(np.abs(nn - r2) > MARGIN * r2)


def _pairs_3dmatch(benchmark, ref_utils):
    root = os.path.join(DATA, '3DMatch', 'metadata', 'benchmarks', benchmark)
    scenes = sorted(os.listdir(root))
    out = []
    for scene in scenes:
        logs = ref_utils.read_log_file(os.path.join(root, scene, 'gt.log'))
        infos = ref_utils.read_info_file(os.path.join(root, scene, 'gt.info'))
        assert [l_['test_pair'] for l_ in logs] == [i['test_pair'] for i in infos]
        recs = []
        for log, info in zip(logs, infos):
            a, b = log['test_pair']
            recs.append(dict(scene=scene, ids=(a, b), transform=log['transform'], covariance=info['covariance'],
                             is_gt=b > a + 1, num_fragments=log['num_fragments']))
        out += sorted(recs, key=lambda r: r['ids'])
    return scenes, out


def _pairs_kitti():
    with open(os.path.join(DATA, 'Kitti', 'metadata', 'test.pkl'), 'rb') as f:
        meta = pickle.load(f)
    recs = [dict(scene='KITTI', ids=(int(m['seq_id']), int(m['frame1']), int(m['frame0'])), transform=m['transform'].astype(np.float32),
                 covariance=None, is_gt=False, num_fragments=0) for m in meta]
    assert len({r['ids'] for r in recs}) == len(recs)
    return ['KITTI'], sorted(recs, key=lambda r: r['ids'])


def _restate(benchmark, recs, rows, cfg):
    """Float64 restatement of eval.py's summary (3DMatch eval.py:240-357, KITTI eval.py:84-185) from per-pair values."""
    e = cfg.eval
    if benchmark == 'KITTI':
        acc = [r < e.rre_threshold and t < e.rte_threshold for r, t in zip(rows['rre'], rows['rte'])]
        groups = [(['KITTI'], np.arange(len(recs)), acc)]
    else:
        scenes = sorted({r['scene'] for r in recs})
        groups = []
        for s in scenes:
            idx = np.array([i for i, r in enumerate(recs) if r['scene'] == s])
            acc = [bool(recs[i]['is_gt'] and rows['err'][i] < e.rmse_threshold ** 2) for i in idx]
            groups.append((s, idx, acc))
    table = []
    for _, idx, acc in groups:
        pr, ir, ov = rows['precision'][idx], rows['inlier_ratio'][idx], rows['overlap'][idx]
        acc = np.array(acc, bool)
        reg = np.ones(len(idx), bool) if benchmark == 'KITTI' else np.array([recs[i]['is_gt'] for i in idx], bool)
        rr_vals, rt_vals = rows['rre'][idx][acc], rows['rte'][idx][acc]
        fmr = (ir >= e.inlier_ratio_threshold).astype(np.float64)
        with np.errstate(all='ignore'):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                table.append([np.mean(pr), np.mean((pr > 0).astype(float)), np.mean((pr >= 0.1).astype(float)),
                              np.mean((pr >= 0.3).astype(float)), np.mean((pr >= 0.5).astype(float)), np.mean(fmr), np.mean(ir),
                              np.mean(ov), np.std(fmr), np.mean(acc[reg].astype(float)), np.mean(rr_vals), np.mean(rt_vals),
                              np.median(rr_vals), np.median(rt_vals)])
    table = np.array(table, np.float64)
    if benchmark == 'KITTI':
        return table, table[0].copy()
    overall = table.mean(0)
    overall[8] = np.std(table[:, 5])
    return table, overall


def generate(benchmark, cfg, ev_mod, ref_utils, reg_funcs, store, tmp):
    evaluate_correspondences, evaluate_sparse, compute_registration_error = reg_funcs
    kitti = benchmark == 'KITTI'
    scenes, recs = _pairs_kitti() if kitti else _pairs_3dmatch(benchmark, ref_utils)
    r = cfg.eval.acceptance_radius
    rng = np.random.default_rng([4242, len(benchmark), int(kitti)])
    keys = ('overlap', 'inlier_ratio', 'residual', 'num_corr', 'precision', 'recall', 'hit_ratio', 'err', 'rre', 'rte')
    rows = {k: np.zeros(len(recs)) for k in keys}
    attempts, sums, ests = np.zeros(len(recs), np.int64), np.zeros(len(recs), np.int64), np.zeros((len(recs), 4, 4), np.float32)
    feat_root = os.path.join(tmp, 'features', benchmark)
    for i, rec in enumerate(recs):
        T = np.asarray(rec['transform'], np.float32)
        att = 0
        while True:
            d = pair_inputs(benchmark, i, att, T, r)
            if _margin_ok(d, T, r):
                break
            att += 1
        E = _estimate(rng, T, kitti, rec['covariance'] if rec['is_gt'] else None, ref_utils, compute_registration_error)
        attempts[i], sums[i], ests[i] = att, inputs_checksum(d), E
        f64 = {k: d[k].astype(np.float64) for k in ('ref_corr_points', 'src_corr_points', 'corr_scores')}
        fine = evaluate_correspondences(f64['ref_corr_points'], f64['src_corr_points'], T.astype(np.float64), positive_radius=r)
        coarse = evaluate_sparse(np.zeros((d['num_ref_nodes'], 3)), np.zeros((d['num_src_nodes'], 3)), d['ref_node_corr_indices'],
                                 d['src_node_corr_indices'], d['gt_node_corr_indices'])
        rre, rte = compute_registration_error(T.astype(np.float64), E.astype(np.float64))
        err = ref_utils.compute_transform_error(T.astype(np.float64), rec['covariance'].astype(np.float64), E.astype(np.float64)) \
            if rec['is_gt'] else float('nan')
        for k, v in (('overlap', fine['overlap']), ('inlier_ratio', fine['inlier_ratio']), ('residual', fine['residual']),
                     ('num_corr', fine['num_corr']), ('precision', coarse['precision']), ('recall', coarse['recall']),
                     ('hit_ratio', coarse['hit_ratio']), ('err', err), ('rre', rre), ('rte', rte)):
            rows[k][i] = v
        name = '_'.join(str(x) for x in rec['ids']) + '.npz'
        path = os.path.join(feat_root, name) if kitti else os.path.join(feat_root, rec['scene'], name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez(path, ref_points_c=np.zeros((d['num_ref_nodes'], 3)), src_points_c=np.zeros((d['num_src_nodes'], 3)),
                 ref_node_corr_indices=d['ref_node_corr_indices'], src_node_corr_indices=d['src_node_corr_indices'],
                 ref_corr_points=f64['ref_corr_points'], src_corr_points=f64['src_corr_points'], corr_scores=f64['corr_scores'],
                 gt_node_corr_indices=d['gt_node_corr_indices'], transform=T.astype(np.float64),
                 estimated_transform=E.astype(np.float64), overlap=np.float64(0.5))
    # the genuine eval_one_epoch
    cfg.feature_dir = feat_root if kitti else os.path.join(tmp, 'features')
    cfg.registration_dir = os.path.join(tmp, 'registration')
    if not kitti:
        cfg.data.dataset_root = os.path.join(DATA, '3DMatch')
        for s in scenes:                                  # (the reference's ensure_dir makes one level only)
            os.makedirs(os.path.join(cfg.registration_dir, benchmark, s), exist_ok=True)
    args = types.SimpleNamespace(test_epoch=None, benchmark=benchmark, method='lgr', num_corr=None, verbose=False)
    log = _Capture()
    ev_mod.eval_one_epoch(args, cfg, log)
    table, overall = _restate(benchmark, recs, rows, cfg)
    p = benchmark + '/'
    store[p + 'scenes'] = np.array(scenes)
    store[p + 'group_lengths'] = np.array([sum(1 for x in recs if x['scene'] == s) for s in scenes], np.int64)
    store[p + 'ids'] = np.array([x['ids'] for x in recs], np.int64)
    store[p + 'transform'] = np.stack([np.asarray(x['transform'], np.float32) for x in recs])
    store[p + 'covariance'] = np.stack([np.zeros((6, 6), np.float32) if x['covariance'] is None else x['covariance'] for x in recs])
    store[p + 'is_gt'] = np.array([x['is_gt'] for x in recs], np.int32)
    store[p + 'num_fragments'] = np.array([x['num_fragments'] for x in recs], np.int64)
    store[p + 'estimated'] = ests
    store[p + 'attempt'] = attempts
    store[p + 'checksum'] = sums
    for k in keys:
        store[p + 'ref/' + k] = rows[k]
    store[p + 'summary/groups'] = table
    store[p + 'summary/overall'] = overall
    store[p + 'summary/critical_lines'] = np.array(log.lines)
    print(benchmark, len(recs), 'pairs, max attempt', attempts.max())
    for line in log.lines[:3]:
        print('  ', line)
    return recs, ests


def main():
    _install_nibabel()
    store = {}
    with tempfile.TemporaryDirectory() as tmp:
        for experiment, benchmarks in (('se3ete.3dmatch', ('3DMatch', '3DLoMatch')), ('se3eti.kitti', ('KITTI',))):
            cfg, ev_mod = _load_eval(experiment)
            from geotransformer.datasets.registration.threedmatch import utils as ref_utils
            from geotransformer.utils import registration as R
            funcs = (R.evaluate_correspondences, R.evaluate_sparse_correspondences, R.compute_registration_error)
            for b in benchmarks:
                recs, ests = generate(b, cfg, ev_mod, ref_utils, funcs, store, tmp)
                if b == '3DMatch':
                    scene = recs[0]['scene']
                    gt_dir = os.path.join(DATA, '3DMatch', 'metadata', 'benchmarks', b, scene)
                    est_log = os.path.join(tmp, 'est.log')
                    ref_utils.write_log_file(est_log, [dict(test_pair=list(x['ids']), num_fragments=x['num_fragments'],
                                                            transform=ests[i]) for i, x in enumerate(recs) if x['scene'] == scene])
                    store['est_log/scene'] = np.array(scene)
                    store['est_log/text'] = np.array(open(est_log).read())
                    res = ref_utils.evaluate_registration_one_scene(os.path.join(gt_dir, 'gt.log'), os.path.join(gt_dir, 'gt.info'),
                                                                    est_log)
                    for k in ('precision', 'recall', 'mean_rre', 'mean_rte', 'median_rre', 'median_rte', 'num_pos_pairs',
                              'num_pred_pairs', 'num_gt_pairs'):
                        store['est_log/' + k] = np.float64(res[k])
                    store['est_log/errors'] = np.array([e['error'] for e in res['errors']], np.float64)
                    lines = open(os.path.join(gt_dir, 'gt.log')).read().splitlines(True)[:15]
                    info = open(os.path.join(gt_dir, 'gt.info')).read().splitlines(True)[:21]
                    store['raw/gt_log'] = np.array(''.join(lines))
                    store['raw/gt_info'] = np.array(''.join(info))
                    raw_log, raw_info = os.path.join(tmp, 'raw.log'), os.path.join(tmp, 'raw.info')
                    open(raw_log, 'w').write(''.join(lines))
                    open(raw_info, 'w').write(''.join(info))
                    pl, pi = ref_utils.read_log_file(raw_log), ref_utils.read_info_file(raw_info)
                    store['raw/log_pairs'] = np.array([x['test_pair'] + [x['num_fragments']] for x in pl], np.int64)
                    store['raw/log_transforms'] = np.stack([x['transform'] for x in pl])
                    store['raw/info_covariances'] = np.stack([x['covariance'] for x in pi])
    np.savez_compressed(OUT, **store)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
