"""Cost of eval.py's benchmark metrics on the device (se3et_amd.benchmark, csrc/benchmark.hip) over the whole 3DMatch benchmark
(profiles/benchmark_probe.txt).

Workload: the 1 623 3DMatch pairs with the ground truth, covariances and estimates of tests/golden/benchmark_metrics.npz, each with a
seeded correspondence set of --num-corr points (default 5 000; 5 058 is the LGR count of the demo pair, tests/golden/demo_se3ete.npz):
ref points uniform in an 8 m box, half of the src points within 0.95 r of their ref point, the rest uniform; node predictions from
tests/benchmark_fixture.py.  Times:
  device   BenchmarkEvaluator.evaluate on all pairs as the 8 scenes (fine, sparse, transform, summary: 7 launches and 2 memsets), wall time
           of the call including its host work and the summary read-back, and device-event time of the overlap call alone;
  host     (--host, where the reference tree exists) the reference's per-pair evaluate_correspondences (cKDTree), evaluate_sparse_
           correspondences and compute_transform_error on --host-pairs pairs, scaled to 1 623.
Distance tests: sum over pairs of n^2 (the brute-force bound; waves stop early once all their lanes have a hit, so the kernel evaluates
fewer), at 8 FLOP per test (3 sub, 1 mul, 2 FMA) against the 157.3 TFLOP/s FP32 vector peak.  Kernel times: run under
`rocprofv3 --kernel-trace --stats`.  Run `python tools/benchmark_probe.py [--num-corr N] [--host] [--out FILE]`."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from benchmark_fixture import pair_inputs  # noqa: E402

PEAK_FP32_VECTOR = 157.3e12
FLOP_PER_TEST = 8
R = 0.1


def workload(gold, n):
    T = gold['3DMatch/transform']
    pairs = []
    for i in range(len(T)):
        d = pair_inputs('3DMatch', i, 0, T[i], R)
        rng = np.random.default_rng([7, i, n])
        ref = rng.uniform(-4, 4, (n, 3))
        world = ref + rng.normal(size=(n, 3)) * (0.95 * R / 3)
        out = rng.random(n) < 0.5
        world[out] = rng.uniform(-4, 4, (int(out.sum()), 3))
        Td = T[i].astype(np.float64)
        d['ref_corr_points'] = ref.astype(np.float32)
        d['src_corr_points'] = ((world - Td[:3, 3]) @ Td[:3, :3]).astype(np.float32)
        d['corr_scores'] = rng.random(n).astype(np.float32)
        pairs.append(d)
    return pairs


def device(gold, pairs, iters):
    import torch
    from se3et_amd.benchmark import BenchmarkEvaluator, evaluate_correspondences_pairs
    from se3et_amd.model import make_cfg
    recs = []
    for i, d in enumerate(pairs):
        rec = {k: torch.from_numpy(np.asarray(d[k])).cuda() for k in ('ref_corr_points', 'src_corr_points', 'corr_scores',
                                                                         'ref_node_corr_indices', 'src_node_corr_indices',
                                                                         'gt_node_corr_indices')}
        rec.update(num_ref_nodes=d['num_ref_nodes'], num_src_nodes=d['num_src_nodes'],
                   transform=torch.from_numpy(gold['3DMatch/transform'][i]).cuda(),
                   estimated_transform=torch.from_numpy(gold['3DMatch/estimated'][i]).cuda(),
                   covariance=gold['3DMatch/covariance'][i] if gold['3DMatch/is_gt'][i] else None)
        recs.append(rec)
    groups = [(str(s), int(n)) for s, n in zip(gold['3DMatch/scenes'], gold['3DMatch/group_lengths'])]
    ev = BenchmarkEvaluator(make_cfg('se3ete'), '3DMatch')
    for _ in range(2):
        res = ev.evaluate(recs, groups, 'lgr')
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        res = ev.evaluate(recs, groups, 'lgr')
    wall = (time.perf_counter() - t0) / iters * 1e3
    refs, srcs, Ts = [r['ref_corr_points'] for r in recs], [r['src_corr_points'] for r in recs], [r['transform'] for r in recs]
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    evaluate_correspondences_pairs(refs, srcs, Ts, R)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        evaluate_correspondences_pairs(refs, srcs, Ts, R)
    end.record()
    torch.cuda.synchronize()
    return wall, start.elapsed_time(end) / iters, res, torch.cuda.get_device_name(0)


def host(gold, pairs, count):
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import generate_benchmark_golden as G
    G._install_nibabel()
    G._load_eval('se3ete.3dmatch')
    from geotransformer.datasets.registration.threedmatch import utils as ref_utils
    from geotransformer.utils import registration as Rg
    t0 = time.perf_counter()
    for i in range(count):
        d = pairs[i]
        T, E = gold['3DMatch/transform'][i], gold['3DMatch/estimated'][i]
        Rg.evaluate_correspondences(d['ref_corr_points'], d['src_corr_points'], T, positive_radius=R)
        Rg.evaluate_sparse_correspondences(np.zeros((d['num_ref_nodes'], 3)), np.zeros((d['num_src_nodes'], 3)),
                                           d['ref_node_corr_indices'], d['src_node_corr_indices'], d['gt_node_corr_indices'])
        if gold['3DMatch/is_gt'][i]:
            ref_utils.compute_transform_error(T, gold['3DMatch/covariance'][i], E)
        Rg.compute_registration_error(T, E)
    return (time.perf_counter() - t0) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--num-corr', type=int, default=5000)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--host', action='store_true', help='time the reference path on the CPU instead (needs the reference tree)')
    ap.add_argument('--host-pairs', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'benchmark_metrics.npz')) as z:
        gold = {k: z[k] for k in z.files}
    pairs = workload(gold, args.num_corr)
    P, n = len(pairs), args.num_corr
    lines = []
    if args.host:
        per = host(gold, pairs, args.host_pairs)
        lines.append('benchmark_probe --host: %d 3DMatch pairs x %d correspondences, reference per-pair functions on the CPU (cKDTree '
                     'workers=-1, %d CPUs)' % (P, n, os.cpu_count()))
        lines.append('host    %.2f ms per pair (%d pairs timed) -> %.0f ms for the %d pairs' % (per * 1e3, args.host_pairs, per * 1e3 * P, P))
    else:
        wall, ov_ms, res, name = device(gold, pairs, args.iters)
        tests = float(P) * n * n
        lines.append('benchmark_probe: %d 3DMatch pairs x %d correspondences, 8 scenes, %s' % (P, n, name))
        lines.append('device  BenchmarkEvaluator.evaluate, all pairs    %.2f ms per call (host wall, %d calls, summary read back)'
                     % (wall, args.iters))
        lines.append('        evaluate_correspondences_pairs alone     %.3f ms per call (device events)' % ov_ms)
        lines.append('        %.3g distance tests (sum n^2) -> %.3g tests/s; %.3f of the 157.3 TF FP32 vector peak at %d FLOP per test'
                     % (tests, tests / (ov_ms * 1e-3), tests / (ov_ms * 1e-3) * FLOP_PER_TEST / PEAK_FP32_VECTOR, FLOP_PER_TEST))
        o = res['overall']
        lines.append('        overall: ' + ', '.join('%s %.3f' % (k, o[k]) for k in ('PIR', 'FMR', 'IR', 'OV', 'RR', 'median_RRE')))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
