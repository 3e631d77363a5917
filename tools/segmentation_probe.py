"""Cost of plane segmentation and DBSCAN on the device (se3et_amd.segmentation) next to the numpy twins (tests/segmentation_twin.py) and,
where it imports, scikit-learn on the same box (profiles/segmentation_probe.txt), and the twin's own spread that the CPU tests' tolerance
is made of.

Workloads, float32 on the device:
  plane    1 and 32 clouds of 100 000 rows (tests/segmentation_fixture.py's slab: a noisy tilted plane patch, 30 % uniform outliers),
           distance_threshold 0.03, ransac_n 3, at 100 and at 1 000 hypotheses;
  dbscan   1 and 32 clouds of 100 000 rows uniform in the unit cube at eps = 0.0363 (about 20 neighbours a row), min_points 10; and one
           chain of 100 000 core rows spaced 0.9 eps along a line in shuffled and in reversed index order (one component whose diameter is
           its length; the grid's axis cap puts ~1 560 rows into every cell of it, so the walks are long as well).
Per workload: host wall time per call, ended by a synchronisation, as the median (min .. max) over --windows windows of at least
--window-seconds each after a warm-up; for DBSCAN also the device-event time of ops.dbscan_stack alone on a grid built once.  The twins and
scikit-learn run once on one cloud (the DBSCAN twin is dense, n x n: on the first 5 000 rows).  Recorded, not gated.
Run `python tools/segmentation_probe.py [--out FILE]` on the GPU box."""
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


def spread(values):
    return statistics.median(values), min(values), max(values)


def windows(fn, count, seconds):
    out = []
    for _ in range(count):
        calls, own, t0 = 0, 0.0, time.perf_counter()
        while time.perf_counter() - t0 < seconds or calls < 3:
            own += fn() or 0.0
            calls += 1
        out.append(own / calls if own else (time.perf_counter() - t0) * 1e3 / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-seconds', type=float, default=0.5)
    ap.add_argument('--no-twin', action='store_true')
    ap.add_argument('--commit', default=None, help='what the numbers were taken at (default: git rev-parse of this tree)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'segmentation_probe.txt'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('segmentation_probe: no device (the probe measures the device; there is no fallback)')
    import segmentation_fixture as F
    import segmentation_twin as twin
    from se3et_amd import ops
    from se3et_amd.segmentation import cluster_dbscan_clouds, segment_plane_clouds
    from se3et_amd.stacking import identities, lengths, stack
    try:
        if args.commit:
            raise OSError
        commit = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
        commit = 'the working tree on top of ' + commit
    except (OSError, subprocess.CalledProcessError):
        commit = args.commit or 'a tree without git metadata'
    lines = ['segmentation_probe: %s, %s; median (min .. max) over %d windows of >= %.1f s, ms per call.  Recorded, not gated; the twin rows '
             'are the numpy restatements of tests/segmentation_twin.py on the same box (%d CPUs allowed), once.'
             % (torch.cuda.get_device_name(0), commit, args.windows, args.window_seconds, min(16, len(os.sched_getaffinity(0))))]
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def wall_of(fn):
        def call():
            fn()
            torch.cuda.synchronize()
        call()
        return spread(windows(call, args.windows, args.window_seconds))

    def timed(fn):
        def run():
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop)
        run()
        return spread(windows(run, args.windows, args.window_seconds))

    n, thr = 100000, 0.03
    host = [F.slab(n, 500 + c).astype(np.float32) for c in range(32)]
    pts = [torch.from_numpy(p).cuda() for p in host]
    for H in (100, 1000):
        for clouds in (1, 32):
            _, inl, st = segment_plane_clouds(pts[:clouds], thr, 3, H, return_stats=True)
            lines.append('segment_plane_clouds, %2d x %d rows, %4d hypotheses, host wall   %10.3f (%.3f .. %.3f)   inliers of cloud 0: %d, rmse %.5f'
                         % ((clouds, n, H) + wall_of(lambda: segment_plane_clouds(pts[:clouds], thr, 3, H)) + (len(inl[0]), float(st['inlier_rmse'][0]))))
        if not args.no_twin:
            t0 = time.perf_counter()
            want = twin.segment_plane(host[0], thr, 3, H, 0)
            t_twin = (time.perf_counter() - t0) * 1e3
            w1 = wall_of(lambda: segment_plane_clouds(pts[:1], thr, 3, H))[0]
            _, inl, st = segment_plane_clouds(pts[:1], thr, 3, H, return_stats=True)
            lines.append('  plane twin (numpy), one cloud, %4d hypotheses, host wall      %10.3f   %.0fx the device call on that cloud (%.3f); winning '
                         'hypothesis equal: %s, inlier sets equal: %s (margin to the threshold %.2e)'
                         % (H, t_twin, t_twin / w1, w1, int(st['best_hypothesis'][0]) == want['best_hypothesis'],
                            np.array_equal(inl[0].cpu().numpy(), np.flatnonzero(want['mask'])), want['margin']))
    eps, min_points = 0.0363, 10
    rng = np.random.default_rng(7)
    host = [rng.uniform(0, 1, (n, 3)).astype(np.float32) for _ in range(32)]
    pts = [torch.from_numpy(p).cuda() for p in host]
    for clouds in (1, 32):
        labels, num = cluster_dbscan_clouds(pts[:clouds], eps, min_points)
        p, pl = stack(pts[:clouds]), lengths(pts[:clouds])
        grid = ops.pair_grid_build(p, pl, identities(clouds), eps)
        ro = ops.pair_ball_count_stack(grid, p, pl, eps)
        alone = timed(lambda: ops.dbscan_stack(grid, p, pl, eps, min_points))              # (before the next call rebuilds the grid workspace)
        lines.append('cluster_dbscan_clouds, %2d x %d rows, eps %.4f (%.1f neighbours a row), min_points %d, host wall   %10.3f (%.3f .. %.3f)   '
                     'clusters of cloud 0: %d, noise rows %d' % ((clouds, n, eps, float(ro[-1]) / (clouds * n), min_points)
                                                                + wall_of(lambda: cluster_dbscan_clouds(pts[:clouds], eps, min_points))
                                                                + (int(num[0]), int((labels[0] == -1).sum()))))
        lines.append('  dbscan_stack alone (five launches, the grid built once), device events %10.3f (%.3f .. %.3f)'
                     % alone)
    if not args.no_twin:
        small = host[0][:5000].astype(np.float64)
        e5 = eps * (n / 5000.0) ** (1.0 / 3.0)
        t0 = time.perf_counter()
        want, _ = twin.cluster_dbscan(small, e5, min_points)
        t_twin = (time.perf_counter() - t0) * 1e3
        got = cluster_dbscan_clouds([torch.from_numpy(small).cuda()], e5, min_points)[0][0].cpu().numpy()
        lines.append('  dbscan twin (numpy, dense), the first 5 000 rows at eps %.4f, host wall   %10.3f   labels equal: %s'
                     % (e5, t_twin, np.array_equal(got, want)))
        try:
            from sklearn.cluster import DBSCAN
            t0 = time.perf_counter()
            sk = DBSCAN(eps=eps, min_samples=min_points, n_jobs=min(16, len(os.sched_getaffinity(0)))).fit(host[0].astype(np.float64)).labels_
            t_sk = (time.perf_counter() - t0) * 1e3
            w1 = wall_of(lambda: cluster_dbscan_clouds(pts[:1], eps, min_points))[0]
            got = cluster_dbscan_clouds(pts[:1], eps, min_points)[0][0].cpu().numpy()
            lines.append('  scikit-learn DBSCAN, one cloud of %d rows, host wall               %10.3f   %.0fx the device call on that cloud (%.3f); labels '
                         'equal: %s' % (n, t_sk, t_sk / w1, w1, np.array_equal(got, sk)))
        except ImportError:
            lines.append('  scikit-learn does not import here')
    x = 0.9 * eps * np.arange(n)
    for order, xs in (('shuffled', rng.permutation(x)), ('reversed', x[::-1].copy())):
        chain = [torch.from_numpy(np.stack([xs, np.zeros(n), np.zeros(n)], 1)).cuda()]
        labels, num = cluster_dbscan_clouds(chain, eps, 2)
        grid = ops.pair_grid_build(chain[0], [n], identities(1), eps)
        alone = timed(lambda: ops.dbscan_stack(grid, chain[0], [n], eps, 2))
        lines.append('cluster_dbscan_clouds, one chain of %d core rows, %s order, host wall   %10.3f (%.3f .. %.3f)   clusters %d; dbscan_stack '
                     'alone, device events %.3f' % ((n, order) + wall_of(lambda: cluster_dbscan_clouds(chain, eps, 2))
                                                    + (int(num[0]), alone[0])))
    worst = {}
    for name, case in F.planes().items():
        if not case[5]:
            for k, v in F.plane_tolerance(name)[1].items():
                worst[k] = max(worst.get(k, 0.0), v)
    lines.append("the twin's spread between two formulations (eigh and ascending sums against Jacobi and descending sums), the largest over the "
                 'plane cases of tests/segmentation_fixture.py without deliberate ties: plane coefficients %.3g, fitness %.3g, inlier_rmse %.3g; '
                 'the CPU tests allow 16 times the case\'s own spread and at least 1e-13' % (worst['plane'], worst['fitness'], worst['inlier_rmse']))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
