"""The figures that the multiway-registration tests rest on, and the cost of the feature on the device (profiles/pose_graph_probe.txt).

Without a GPU: per case of tests/pose_graph_fixture.py the twin's own spread -- the largest difference, per quantity, between evaluations
of tests/pose_graph_twin.py that differ only in the solver (LU against Cholesky) and in the direction of the edge sums (ascending against
descending) -- and the margin that the tests allow between the library and the twin, 16 times that spread with a floor of 1e-13 (the
MARGINS line is copied into the fixture); beside it the deviation of se3_debug_pose_graph_host from the twin.  The same for the
information matrix (the twin's rows summed from either end), and the largest error of the arc tangent in ulp against numpy.arctan2.
With a GPU, recorded and not gated: the median (min .. max) host wall time, ended by a device synchronise, of
pose_graph.optimize_pose_graphs for 1 and 32 graphs of 16 and 64 nodes (complete edge sets) next to the twin on one graph, and of
pose_graph.information_matrix_pairs for 32 pairs of 5 000 + 5 000 points next to the twin with 16 threads; every shape warmed up first.
`python tools/pose_graph_probe.py [--iters N] [--out FILE] [--commit ID]`; without a device the timing rows say so."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

QUANTITIES = ('poses', 'confidence', 'residuals')


def commit(given=None):
    if given:
        return given
    try:
        return subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return 'unknown'


def graph_rows():
    import pose_graph_fixture as F
    rows = []
    for name in sorted(F.FAMILIES):
        c = F.case(name)
        base, got = c['twin'], F.host_pgo(c['graph'])
        spread = dict.fromkeys(QUANTITIES, 0.0)
        for solver, descending in (('lu', False), ('cholesky', True), ('lu', True)):
            other = F.twin.global_optimization(c['graph'], solver, descending)
            assert np.array_equal(other['info'], base['info']) and np.array_equal(other['kept'], base['kept']), name
            for q in QUANTITIES:
                spread[q] = max(spread[q], float(np.abs(other[q] - base[q]).max()))
        rows.append((name, len(c['graph']['poses']), len(c['graph']['edges']), base['info'], F.rejected_trials(base['passes']), spread,
                     {q: float(np.abs(got[q] - base[q]).max()) for q in QUANTITIES}))
    return rows


def information_rows():
    import icp_fixture as I
    import pose_graph_fixture as F
    rows = []
    for name in sorted(I.FAMILIES):
        c = I.case(name, 'point_to_point', 'float64')
        T = c['twin']['transform']
        a, b = F.twin.information_matrix(c['src'], c['ref'], T, c['r']), F.twin.information_matrix(c['src'], c['ref'], T, c['r'], descending=True)
        got = F.host_information(c['src'], c['ref'], T, c['r'])
        rows.append((name, a['count'], float(np.abs(a['information'] - b['information']).max()),
                     float(np.abs(got['information'] - a['information']).max())))
    return rows


def atan2_error(n=400000):
    import pose_graph_fixture as F
    rng = np.random.default_rng(0)
    th = rng.uniform(-np.pi, np.pi, n)
    mag = 10.0 ** rng.uniform(-150, 150, n)
    y, x = np.sin(th) * mag, np.cos(th) * mag
    got, ref = F.host_atan2(y, x), np.arctan2(y, x)
    return n, float((np.abs(got - ref) / np.spacing(np.abs(ref))).max())


def timed(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pose_graph_probe.txt'))
    ap.add_argument('--commit', default=None, help='the commit of the tree, where the tool runs outside its git checkout')
    args = ap.parse_args()
    import torch
    import pose_graph_fixture as F
    lines = ['the twin\'s own spread (solver LU / Cholesky, edge sums ascending / descending) per fixture case and quantity; the tests allow '
             'the library 16 times it, at least %.0e' % F.FLOOR]
    margins = {}
    for name, N, E, info, rejected, spread, dev in graph_rows():
        margins[name] = {q: max(16.0 * spread[q], F.FLOOR) for q in QUANTITIES}
        lines.append('  case %-11s N %2d E %4d  info %-22s rejected trials %d  spread %s  margin %s  host entry - twin %s'
                     % (name, N, E, ' '.join(str(int(v)) for v in info), rejected, ' '.join('%.2e' % spread[q] for q in QUANTITIES),
                        ' '.join('%.2e' % margins[name][q] for q in QUANTITIES), ' '.join('%.2e' % dev[q] for q in QUANTITIES)))
    lines.append('MARGINS = {%s}' % ', '.join('%r: {%s}' % (name, ', '.join('%r: %.2e' % (q, m[q]) for q in QUANTITIES))
                                              for name, m in sorted(margins.items())))
    info_margin = F.FLOOR
    for name, count, spread, dev in information_rows():
        info_margin = max(info_margin, 16.0 * spread)
        lines.append('  information matrix, ICP case %-12s %5d correspondences  spread (rows summed from either end) %.2e  host entry - twin %.2e'
                     % (name, count, spread, dev))
    lines.append('INFORMATION_MARGIN = %.2e' % info_margin)
    n, ulp = atan2_error()
    lines.append('arc tangent: largest error against numpy.arctan2 over %d points of all quadrants, magnitudes 1e-150 .. 1e150: %.2f ulp; the '
                 'test allows 4' % (n, ulp))
    if torch.cuda.is_available():
        from se3et_amd import pose_graph
        lines.insert(0, 'pose_graph_probe: %s, commit %s (+ the working tree of the change that adds the feature); median (min .. max) of %d '
                        'calls, ms, host wall ended by a device synchronise.  `python tools/pose_graph_probe.py --iters %d`.  Recorded, not '
                        'gated.' % (torch.cuda.get_device_name(0), commit(args.commit), args.iters, args.iters))
        gpu = lambda g: {k: torch.from_numpy(np.ascontiguousarray(v.astype(np.uint8) if k == 'uncertain' else v)).cuda() for k, v in g.items()}
        for N in (16, 64):
            graphs = [F.scene(N, 200 + g, 'all', 'odometry')[0] for g in range(32)]
            dev = [gpu(g) for g in graphs]
            t0 = time.perf_counter()
            tw = F.twin.global_optimization(graphs[0])
            twin_ms = (time.perf_counter() - t0) * 1e3
            for G in (1, 32):
                fn = lambda: pose_graph.optimize_pose_graphs(dev[:G])
                out = fn()
                info = out['info'].cpu().numpy()
                lines.append('  optimize_pose_graphs, %2d graphs of %2d nodes, %4d edges  %9.3f (%.3f .. %.3f)   trials %d .. %d per graph, '
                             'status %s; the twin on ONE such graph: %.0f ms'
                             % ((G, N, len(graphs[0]['edges'])) + timed(fn, args.iters) +
                                (int((info[:, 2] + info[:, 5]).min()), int((info[:, 2] + info[:, 5]).max()),
                                 sorted(set(out['status'].cpu().tolist())), twin_ms)))
            assert np.array_equal(tw['info'], pose_graph.optimize_pose_graphs(dev[:1])['info'][0].cpu().numpy())
        rng = np.random.default_rng(7)
        import icp_fixture as I
        pairs = []
        for p in range(32):
            ref, _n = I.sheet(rng, 5000)
            src = ref[rng.permutation(5000)] + 0.002 * rng.normal(size=(5000, 3))
            pairs.append((src, ref, I.rigid(rng, 0.5, 0.005)))
        srcs, refs = [torch.from_numpy(p[0]).cuda() for p in pairs], [torch.from_numpy(p[1]).cuda() for p in pairs]
        Ts = torch.from_numpy(np.stack([p[2] for p in pairs])).cuda()
        fn = lambda: pose_graph.information_matrix_pairs(srcs, refs, Ts, 0.02)
        out = fn()
        t0 = time.perf_counter()
        for p in pairs:
            F.twin.information_matrix(p[0], p[1], p[2], 0.02, workers=16)
        twin_ms = (time.perf_counter() - t0) * 1e3
        lines.append('  information_matrix_pairs, 32 pairs of 5000 + 5000 points, r = 0.02  %9.3f (%.3f .. %.3f)   correspondences %d .. %d; the '
                     'twin on the 32 pairs, 16 threads: %.0f ms' % (timed(fn, args.iters) + (int(out['count'].min()), int(out['count'].max()), twin_ms)))
    else:
        lines.insert(0, 'pose_graph_probe: run without a device, commit %s: the margins only' % commit(args.commit))
        lines.append('optimize_pose_graphs for 1 and 32 graphs of 16 / 64 nodes, information_matrix_pairs for 32 x (5000 + 5000) points: not measured')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
