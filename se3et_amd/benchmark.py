"""eval.py's benchmark metrics on the device: the protocol of experiments/se3ete.3dmatch/eval.py:42-357 (3DMatch / 3DLoMatch, per scene
and overall) and experiments/se3eti.kitti/eval.py:32-185 (KITTI, over pairs), as batched HIP kernels (csrc/benchmark.hip).

  evaluate_correspondences_pairs(ref_list, src_list, transforms, r)        overlap, inlier_ratio, residual, num_corr (P,) per pair
  evaluate_sparse_correspondences_pairs(ref_idx, src_idx, gt, N, M)       precision, recall, hit_ratio (P,) per pair
  compute_transform_error_pairs(transforms, covariances, estimated)       err, rre, rte (P,) per pair
  read_log_file / read_info_file / write_log_file                          the gt.log / gt.info / est.log formats
  BenchmarkEvaluator(cfg, benchmark)                                       eval.py's per-pair table and scene / overall summaries
  evaluate_registration_log(gt_root, est_log)                              evaluate_registration_one_scene for an est.log of any method
  python -m se3et_amd.benchmark --features DIR --gt-root DIR --benchmark 3DMatch|3DLoMatch|KITTI --method lgr|svd|ransac

Contract (csrc/benchmark.hip carries the same text):
  - overlap: the fraction of ref_corr points whose nearest transformed src_corr point of the pair is closer than r.  The src points are
    transformed in float32 (fma(R[k][2], z, fma(R[k][1], y, R[k][0] x)) + t[k]) and d^2 < r^2 is tested in float32, where the reference
    takes a float32 GEMM and float64 cKDTree distances: only a point whose d^2 lies within float32 rounding of r^2 can count differently.
  - inlier_ratio and residual: float64 from the float32 inputs (|ref - (R src + t)| < r, and the mean of that distance).
  - Pairs without correspondences get inlier_ratio, overlap and residual NaN, as np.mean of an empty array does in the reference.
  - Sparse metrics use the reference's set semantics (duplicates count once) and its + 1e-12 denominators.
  - err = compute_transform_error in float64 with nibabel's mat2quat convention (w >= 0; q = the eigenvector of Bar-Itzhack's K for its
    largest eigenvalue); rre / rte = compute_registration_error in float64 (the arccos argument clipped to [-1, 1]).
  - 3DMatch registration counts only the benchmark pairs (listed in gt.log with id1 > id0 + 1) and accepts err < rmse_threshold^2
    (strict, as eval.py); evaluate_registration_log accepts err <= positive_threshold^2, as evaluate_registration_one_scene does.  KITTI
    accepts rre < rre_threshold and rte < rte_threshold.
  - Summaries: means, np.std and np.median (the mean of the two middle values) over a group, sums in pair order; empty sets give NaN.
    3DMatch's overall value is the mean over scenes of each scene value, KITTI's is over all pairs.
Counts are integers and every sum runs in a fixed order: a pair's row is bit-identical alone or in any batch, and from run to run."""
import argparse
import glob
import json
import math
import os
import sys

import numpy as np
import torch

from . import ops as _ops
from .stacking import as_rows, as_tensor, device_of, device_offsets, lengths, stack, transforms_of

SUMMARY_KEYS = ('PIR', 'PMR>0', 'PMR>=0.1', 'PMR>=0.3', 'PMR>=0.5', 'FMR', 'IR', 'OV', 'FMR_std', 'RR', 'mean_RRE', 'mean_RTE',
                'median_RRE', 'median_RTE')
BENCHMARKS = ('3DMatch', '3DLoMatch', 'KITTI')
MAX_GROUP_PAIRS = 4096


@torch.no_grad()
def evaluate_correspondences_pairs(ref_list, src_list, transforms, positive_radius, device=None):
    """evaluate_correspondences (geotransformer/utils/registration.py:133-250) for P pairs in one call: ref_list[p] / src_list[p] (n_p, 3)
    corresponding rows, transforms (P, 4, 4) ground truth src -> ref.  Returns {overlap, inlier_ratio, residual: (P,) float64,
    num_corr: (P,) int64} device tensors."""
    if len(ref_list) != len(src_list):
        raise ValueError('evaluate_correspondences_pairs: one ref and one src set per pair')
    dev = device_of(device, ref_list, src_list)
    refs, srcs = [as_rows(r, dev) for r in ref_list], [as_rows(s, dev) for s in src_list]
    for p, (r, s) in enumerate(zip(refs, srcs)):
        if r.shape != s.shape:
            raise ValueError('evaluate_correspondences_pairs: pair %d has %d ref and %d src rows' % (p, r.shape[0], s.shape[0]))
    counts = lengths(refs)
    empty = torch.zeros((0, 3), dtype=torch.float32, device=dev)
    T = transforms_of(transforms, len(refs), 'evaluate_correspondences_pairs', dev, torch.float32, error=RuntimeError)
    rows = _ops.benchmark_correspondences_stack(stack(refs, empty), stack(srcs, empty), device_offsets(counts, dev), max(counts, default=0), T,
                                                positive_radius)
    return dict(overlap=rows[:, 0], inlier_ratio=rows[:, 1], residual=rows[:, 2], num_corr=rows[:, 3].to(torch.int64))


@torch.no_grad()
def evaluate_sparse_correspondences_pairs(ref_node_idx_list, src_node_idx_list, gt_node_corr_list, num_ref_nodes, num_src_nodes, device=None):
    """evaluate_sparse_correspondences (registration.py:253-280) for P pairs: predicted node pairs (ref_node_idx_list[p][k],
    src_node_idx_list[p][k]), ground-truth node pairs gt_node_corr_list[p] (g_p, 2), node counts num_ref_nodes[p] / num_src_nodes[p]
    (host ints).  Returns {precision, recall, hit_ratio: (P,) float64} device tensors."""
    P = len(ref_node_idx_list)
    if not (len(src_node_idx_list) == len(gt_node_corr_list) == len(num_ref_nodes) == len(num_src_nodes) == P):
        raise ValueError('evaluate_sparse_correspondences_pairs: one entry per pair in every list')
    dev = device_of(device, ref_node_idx_list, gt_node_corr_list)
    ri = [as_rows(v, dev, None, torch.int64) for v in ref_node_idx_list]
    si = [as_rows(v, dev, None, torch.int64) for v in src_node_idx_list]
    gi = [as_rows(v, dev, 2, torch.int64) for v in gt_node_corr_list]
    for p in range(P):
        if ri[p].shape != si[p].shape:
            raise ValueError('evaluate_sparse_correspondences_pairs: pair %d has mismatched ref / src node indices' % p)
    z1, z2 = torch.zeros((0,), dtype=torch.int64, device=dev), torch.zeros((0, 2), dtype=torch.int64, device=dev)
    rows = _ops.benchmark_sparse_stack(stack(ri, z1), stack(si, z1), device_offsets(lengths(ri), dev), stack(gi, z2),
                                       device_offsets(lengths(gi), dev), list(zip(num_ref_nodes, num_src_nodes)))
    return dict(precision=rows[:, 0], recall=rows[:, 1], hit_ratio=rows[:, 2])


@torch.no_grad()
def compute_transform_error_pairs(transforms, covariances, estimated, device=None):
    """compute_transform_error (datasets/registration/threedmatch/utils.py:131-137) and compute_registration_error (registration.py:51-67)
    for P pairs in float64: transforms / estimated (P, 4, 4), covariances (P, 6, 6), a list with None for the pairs without one, or None.
    Returns {err (NaN without covariance), rre, rte: (P,) float64} device tensors."""
    dev = device_of(device, [estimated])
    P = len(estimated)
    gt, est = (transforms_of(t, P, 'compute_transform_error_pairs', dev, error=RuntimeError) for t in (transforms, estimated))
    cov = has = None
    if covariances is not None:
        if isinstance(covariances, (list, tuple)):
            has = torch.tensor([c is not None for c in covariances], dtype=torch.int32)
            cov = torch.stack([torch.zeros((6, 6), dtype=torch.float64) if c is None else as_tensor(c).to(torch.float64).cpu().reshape(6, 6)
                               for c in covariances], 0) if P else torch.zeros((0, 6, 6), dtype=torch.float64)
        else:
            cov = as_tensor(covariances).to(torch.float64).reshape(P, 6, 6)
            has = torch.ones((P,), dtype=torch.int32)
        cov, has = cov.to(dev).contiguous(), has.to(dev)
    rows = _ops.benchmark_transform_error_stack(gt, est, cov, has)
    return dict(err=rows[:, 0], rre=rows[:, 1], rte=rows[:, 2])


# ---- gt.log / gt.info / est.log ------------------------------------------------------------------------------------------------------------
def _read_records(file_name, rows):
    with open(file_name) as f:
        lines = [line.strip() for line in f.readlines()]
    out = []
    for i in range(len(lines) // (rows + 1)):
        head = lines[i * (rows + 1)].split()
        body = np.array([lines[i * (rows + 1) + j].split() for j in range(1, rows + 1)], dtype=np.float32)
        out.append((int(head[0]), int(head[1]), int(head[2]), body))
    return out


def read_log_file(file_name):
    """A gt.log / est.log: 5-line records 'id0 id1 num_fragments' + 4 rows of the (src id1 -> ref id0) transform.
    -> [dict(test_pair=[id0, id1], num_fragments, transform (4, 4) float32)]."""
    return [dict(test_pair=[a, b], num_fragments=n, transform=m) for a, b, n, m in _read_records(file_name, 4)]


def read_info_file(file_name):
    """A gt.info: 7-line records 'id0 id1 num_fragments' + 6 rows of the covariance.  -> [dict(test_pair, num_fragments, covariance
    (6, 6) float32)]."""
    return [dict(test_pair=[a, b], num_fragments=n, covariance=m) for a, b, n, m in _read_records(file_name, 6)]


def write_log_file(file_name, test_pairs):
    """Writes an est.log: per record 'id0\\tid1\\tnum_fragments' and the transform's 4 rows, each value as Python formats the float."""
    if os.path.dirname(file_name):
        os.makedirs(os.path.dirname(file_name), exist_ok=True)
    lines = []
    for rec in test_pairs:
        a, b = rec['test_pair']
        lines.append('{}\t{}\t{}\n'.format(a, b, rec['num_fragments']))
        for row in np.asarray(rec['transform']).tolist():
            lines.append('{}\t{}\t{}\t{}\n'.format(row[0], row[1], row[2], row[3]))
    with open(file_name, 'w') as f:
        f.writelines(lines)


def benchmark_pairs(gt_root):
    """The parsed gt.log / gt.info of one scene: {(id0, id1): (index, transform, covariance or None, num_fragments)} and the set of
    benchmark pairs (id1 > id0 + 1)."""
    logs = read_log_file(os.path.join(gt_root, 'gt.log'))
    infos = read_info_file(os.path.join(gt_root, 'gt.info'))
    info_by_pair = {tuple(r['test_pair']): r['covariance'] for r in infos}
    table = {}
    for i, r in enumerate(logs):
        a, b = r['test_pair']
        table[(a, b)] = (i, r['transform'], info_by_pair.get((a, b)), r['num_fragments'])
    gt_set = {k for k in table if k[1] > k[0] + 1}
    return table, gt_set


def evaluate_registration_log(gt_root, est_log, positive_threshold=0.2, device=None):
    """evaluate_registration_one_scene (threedmatch/utils.py:139-194) for an est.log of any method: benchmark pairs are accepted iff
    err <= positive_threshold^2.  Returns precision, recall, mean / median RRE and RTE, num_pos_pairs, num_pred_pairs, num_gt_pairs and
    errors [{id0, id1, error}]."""
    table, gt_set = benchmark_pairs(gt_root)
    results = [r for r in read_log_file(est_log) if tuple(r['test_pair']) in gt_set]
    errors, rre, rte = [], [], []
    if results:
        keys = [tuple(r['test_pair']) for r in results]
        m = compute_transform_error_pairs(np.stack([table[k][1] for k in keys]), [table[k][2] for k in keys],
                                          np.stack([r['transform'] for r in results]), device)
        err, rr, rt = (m[k].cpu().numpy() for k in ('err', 'rre', 'rte'))
        thr = positive_threshold ** 2
        for k, e, a, b in zip(keys, err, rr, rt):
            errors.append({'id0': k[0], 'id1': k[1], 'error': float(e)})
            if e <= thr:
                rre.append(float(a))
                rte.append(float(b))
    n_pred, n_pos, n_gt = len(results), len(rre), len(gt_set)
    with np.errstate(all='ignore'):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            stats = dict(mean_rre=np.mean(rre), mean_rte=np.mean(rte), median_rre=np.median(rre), median_rte=np.median(rte))
    return dict(precision=n_pos / n_pred if n_pred > 0 else 0, recall=n_pos / n_gt, **{k: float(v) for k, v in stats.items()},
                num_pos_pairs=n_pos, num_pred_pairs=n_pred, num_gt_pairs=n_gt, errors=errors)


# ---- the evaluator ---------------------------------------------------------------------------------------------------------------------------
class BenchmarkEvaluator:
    """eval.py for '3DMatch', '3DLoMatch' (per scene, then the mean over scenes) or 'KITTI' (over all pairs), with cfg = make_cfg(...)'s
    cfg.eval (acceptance_radius, inlier_ratio_threshold, rmse_threshold or rre_threshold / rte_threshold) and cfg.ransac.

      evaluate_outputs(outs, transforms, ...)      B output dicts of forward_pairs(..., ground_truth=True) as one group
      evaluate_features(features_root, gt_root)    a tree of test.py .npz files (3DMatch: <scene>/<id0>_<id1>.npz; KITTI: <seq>_<id0>_<id1>.npz)
      evaluate(records, groups, ...)               the common core

    Every call returns {'pairs': per-pair device tensors, 'groups': {name: {key: float}}, 'overall': {key: float}} with SUMMARY_KEYS;
    the summary is the only host read-back (and the est.log files, when asked for)."""

    def __init__(self, cfg, benchmark):
        if benchmark not in BENCHMARKS:
            raise ValueError('BenchmarkEvaluator: benchmark must be one of %s' % (BENCHMARKS,))
        self.cfg, self.benchmark, self.kitti = cfg, benchmark, benchmark == 'KITTI'
        e = cfg.eval
        self.acceptance_radius = e.acceptance_radius
        self.inlier_ratio_threshold = e.inlier_ratio_threshold
        if self.kitti:
            self.rmse_threshold, self.rre_threshold, self.rte_threshold = 0.0, e.rre_threshold, e.rte_threshold
        else:
            self.rmse_threshold, self.rre_threshold, self.rte_threshold = e.rmse_threshold, 0.0, 0.0

    @torch.no_grad()
    def evaluate(self, records, groups, method='lgr', num_corr=None, estimated=None, est_log_dir=None, seed=0):
        """records: per-pair dicts with ref_corr_points, src_corr_points, corr_scores, ref/src_node_corr_indices, gt_node_corr_indices,
        ref/src_points_c (or num_ref_nodes / num_src_nodes), transform, estimated_transform (for 'lgr'), and for 3DMatch covariance (None
        off the benchmark), test_pair and num_fragments; groups: [(name, number of consecutive records)].  estimated (P, 4, 4) replaces the
        registration step."""
        from . import ransac
        P = len(records)
        if sum(n for _, n in groups) != P:
            raise ValueError('BenchmarkEvaluator: the groups cover %d records, not %d' % (sum(n for _, n in groups), P))
        if max((n for _, n in groups), default=0) > MAX_GROUP_PAIRS:
            raise ValueError('BenchmarkEvaluator: a group holds more than %d pairs' % MAX_GROUP_PAIRS)
        if self.kitti and len(groups) != 1:
            raise ValueError('BenchmarkEvaluator: KITTI evaluates all pairs as one group')
        dev = records[0]['ref_corr_points'].device if P else torch.device('cuda')
        cut = [ransac.select_correspondences(r, num_corr) for r in records]
        fine = evaluate_correspondences_pairs([c[0] for c in cut], [c[1] for c in cut], [r['transform'] for r in records],
                                              self.acceptance_radius, dev)
        nodes = [(r['num_ref_nodes'], r['num_src_nodes']) if 'num_ref_nodes' in r else (int(r['ref_points_c'].shape[0]),
                                                                                          int(r['src_points_c'].shape[0])) for r in records]
        coarse = evaluate_sparse_correspondences_pairs([r['ref_node_corr_indices'] for r in records],
                                                       [r['src_node_corr_indices'] for r in records],
                                                       [r['gt_node_corr_indices'] for r in records], [n[0] for n in nodes],
                                                       [n[1] for n in nodes], dev)
        if estimated is None:
            estimated = ransac.register_pairs(self.cfg, records, method, num_corr, seed) if P else torch.zeros((0, 4, 4), device=dev)
        covs = None if self.kitti else [r.get('covariance') for r in records]
        reg = compute_transform_error_pairs([r['transform'] for r in records] if P else torch.zeros((0, 4, 4)), covs, estimated, dev)
        is_gt = torch.tensor([0 if self.kitti or r.get('covariance') is None else 1 for r in records], dtype=torch.int32).to(dev)
        rows = torch.stack([coarse['precision'], fine['inlier_ratio'], fine['overlap'], reg['err'], reg['rre'], reg['rte']], 1) if P else \
            torch.zeros((0, 6), dtype=torch.float64, device=dev)
        g_rows, overall = _ops.benchmark_summary(rows, is_gt, [n for _, n in groups], self.kitti, self.inlier_ratio_threshold,
                                                 self.rmse_threshold, self.rre_threshold, self.rte_threshold)
        pairs = dict(PIR=coarse['precision'], recall=coarse['recall'], hit_ratio=coarse['hit_ratio'], IR=fine['inlier_ratio'],
                     OV=fine['overlap'], residual=fine['residual'], num_corr=fine['num_corr'], err=reg['err'], RRE=reg['rre'],
                     RTE=reg['rte'], is_gt=is_gt, estimated_transform=estimated)
        if est_log_dir is not None and not self.kitti:
            est = estimated.detach().cpu().numpy()
            a = 0
            for name, n in groups:
                write_log_file(os.path.join(est_log_dir, name, 'est.log'),
                               [dict(test_pair=records[a + i]['test_pair'], num_fragments=records[a + i]['num_fragments'],
                                     transform=est[a + i]) for i in range(n)])
                a += n
        host = torch.cat([g_rows.reshape(-1), overall]).cpu().numpy()
        g_host, o_host = host[:-14].reshape(-1, 14), host[-14:]
        return dict(pairs=pairs, groups={name: dict(zip(SUMMARY_KEYS, map(float, g_host[i]))) for i, (name, _) in enumerate(groups)},
                    overall=dict(zip(SUMMARY_KEYS, map(float, o_host))))

    def evaluate_outputs(self, outs, transforms, method='lgr', num_corr=None, estimated=None, group='all', seed=0):
        """The B output dicts of batched.forward_pairs(..., ground_truth=True) as one group, transforms (B, 4, 4) their ground truth.
        (3DMatch: no covariances, so only RRE / RTE; RR follows the KITTI rule only for BenchmarkEvaluator(cfg, 'KITTI').)"""
        transforms = as_tensor(transforms).reshape(len(outs), 4, 4)
        records = [dict(out, transform=transforms[p]) for p, out in enumerate(outs)]
        return self.evaluate(records, [(group, len(records))], method, num_corr, estimated, seed=seed)

    def load_features(self, features_root, gt_root=None, device='cuda'):
        """(records, groups) of a test.py feature tree: 3DMatch <features_root>/<scene>/<id0>_<id1>.npz with <gt_root>/<scene>/gt.log and
        gt.info; KITTI <features_root>/<seq>_<id0>_<id1>.npz."""
        def key(path):
            return [int(i) for i in os.path.basename(path).split('.')[0].split('_')]

        def load(path):
            d = np.load(path)
            rec = {k: torch.from_numpy(np.ascontiguousarray(d[k])).to(device) for k in
                   ('ref_corr_points', 'src_corr_points', 'corr_scores', 'ref_node_corr_indices', 'src_node_corr_indices',
                    'gt_node_corr_indices', 'transform', 'estimated_transform')}
            rec['num_ref_nodes'], rec['num_src_nodes'] = int(d['ref_points_c'].shape[0]), int(d['src_points_c'].shape[0])
            return rec

        records, groups = [], []
        if self.kitti:
            files = sorted(glob.glob(os.path.join(features_root, '*.npz')), key=key)
            records = [load(f) for f in files]
            return records, [('KITTI', len(records))]
        if gt_root is None:
            raise ValueError('BenchmarkEvaluator: 3DMatch needs the gt_root of gt.log / gt.info')
        for scene_root in sorted(glob.glob(os.path.join(features_root, '*'))):
            scene = os.path.basename(scene_root)
            table, gt_set = benchmark_pairs(os.path.join(gt_root, scene))
            num_fragments = next(iter(table.values()))[3] if table else 0
            files = sorted(glob.glob(os.path.join(scene_root, '*.npz')), key=key)
            for f in files:
                rec = load(f)
                pair = tuple(key(f))
                rec['test_pair'], rec['num_fragments'] = list(pair), num_fragments
                rec['covariance'] = table[pair][2] if pair in gt_set else None
                records.append(rec)
            groups.append((scene, len(files)))
        return records, groups

    def evaluate_features(self, features_root, gt_root=None, method='lgr', num_corr=None, est_log_dir=None, seed=0, device='cuda'):
        records, groups = self.load_features(features_root, gt_root, device)
        return self.evaluate(records, groups, method, num_corr, est_log_dir=est_log_dir, seed=seed)


def format_summary(result, benchmark):
    """eval.py's critical lines (3 decimals) for a BenchmarkEvaluator result; groups are named as given."""
    o, scenes = result['overall'], result['groups']

    def f(*pairs):
        return ''.join(', {}: {:.3f}'.format(name, value) for name, value in pairs)
    coarse = [('PIR', 'PIR'), ('PMR>0', 'PMR>0'), ('PMR>=0.1', 'PMR>=0.1'), ('PMR>=0.3', 'PMR>=0.3'), ('PMR>=0.5', 'PMR>=0.5')]
    lines = ['  Coarse Matching' + f(*[(n, o[k]) for n, k in coarse])]
    if benchmark == 'KITTI':
        lines.append('  Fine Matching' + f(('FMR', o['FMR']), ('IR', o['IR']), ('OV', o['OV']), ('std', o['FMR_std'])))
        lines.append('  Registration' + f(('RR', o['RR']), ('RRE', o['mean_RRE']), ('RTE', o['mean_RTE'])))
        return lines
    lines += ['    ' + name + f(*[(n, s[k]) for n, k in coarse]) for name, s in scenes.items()]
    lines.append('  Fine Matching' + f(('FMR', o['FMR']), ('IR', o['IR']), ('OV', o['OV']), ('std', o['FMR_std'])))
    lines += ['    ' + name + f(('FMR', s['FMR']), ('IR', s['IR'])) for name, s in scenes.items()]
    reg = [('RR', 'RR'), ('mean_RRE', 'mean_RRE'), ('mean_RTE', 'mean_RTE'), ('median_RRE', 'median_RRE'), ('median_RTE', 'median_RTE')]
    lines.append('  Registration' + f(*[(n, o[k]) for n, k in reg]))
    lines += ['    ' + name + f(*[(n, s[k]) for n, k in reg]) for name, s in scenes.items()]
    return lines


def main(argv=None):
    parser = argparse.ArgumentParser(description="eval.py's benchmark metrics on the device")
    parser.add_argument('--features', required=True, help='test.py feature tree (3DMatch: <scene>/<id0>_<id1>.npz)')
    parser.add_argument('--gt-root', default=None, help='metadata/benchmarks/<benchmark> (3DMatch / 3DLoMatch: <scene>/gt.log, gt.info)')
    parser.add_argument('--benchmark', choices=BENCHMARKS, required=True)
    parser.add_argument('--method', choices=['lgr', 'svd', 'ransac'], required=True)
    parser.add_argument('--num_corr', type=int, default=None)
    parser.add_argument('--est-log-dir', default=None, help='write <dir>/<scene>/est.log')
    parser.add_argument('--json', action='store_true', help='also print the summaries as one JSON line')
    args = parser.parse_args(argv)
    from .model import make_cfg
    cfg = make_cfg('se3eti_kitti' if args.benchmark == 'KITTI' else 'se3ete')
    ev = BenchmarkEvaluator(cfg, args.benchmark)
    result = ev.evaluate_features(args.features, args.gt_root, args.method, args.num_corr, args.est_log_dir)
    for line in format_summary(result, args.benchmark):
        print(line)
    if args.json:
        print(json.dumps({'overall': result['overall'], 'groups': result['groups']},
                         default=lambda v: None if isinstance(v, float) and math.isnan(v) else v))
    return 0


if __name__ == '__main__':
    sys.exit(main())
