"""Cost of the ISS detector and of the outlier filters on the device (se3et_amd.iss, se3et_amd.scan_prep) next to the numpy twins
(tests/iss_twin.py, tests/outlier_twin.py) on the same box, and of global_registration_pairs with and without keypoints='iss'
(profiles/iss_probe.txt).

Workloads: points of the FPFH test surface (tests/fpfh_fixture.py: z = 0.3 sin(3x) cos(2y) + 0.1 x^2 over [-1, 1]^2), float32 on the device:
  16 x 5 000 points;   1 x 20 000 points.
The radii are Open3D's defaults for the first cloud, 6 and 4 model resolutions, given explicitly; the call with radius 0 (every cloud its
own radii from its own resolution, one more host copy) is timed beside it.
Per workload: host wall time per call of iss_keypoints_clouds, remove_statistical_outlier_clouds (20, 2.0) and remove_radius_outlier_clouds
(16, the salient radius), each ended by a synchronisation, and between device events the stages, each alone on inputs built once: the
search (grid build, count, fill at the salient radius), the saliency pass, the selection pass (grid build at the non-max radius and the
walk), the k-NN mean pass (grid build and knn_distance_stack, k = 20) and the statistics (the two fixed-shape sums and the mask).  All as
the median (min .. max) over --windows windows of at least --window-seconds each after a warm-up of every shape.  The twins are dense
(n x n): they run once, on the first cloud of the 16 x 5k workload alone.
The pipeline: global_registration_pairs on 4 pairs (5 000 points and their moved, permuted copies, voxel size 0.05, RANSAC, ICP) without
a detector -- the parent's path, unchanged -- and with keypoints='iss' at radii of 2.5 and 1.5 voxel sizes: host wall per call, the rows the
coarse method matches over, and the errors of the result.  These are recorded, not gated.
Run `python tools/iss_probe.py [--out FILE]` on the GPU box."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def spread(values):
    return statistics.median(values), min(values), max(values)


def windows(fn, count, seconds):
    """Per-call milliseconds of fn (which returns its own time in ms, or None for the host clock) in `count` windows."""
    out = []
    for _ in range(count):
        calls, own, t0 = 0, 0.0, time.perf_counter()
        while time.perf_counter() - t0 < seconds or calls < 3:
            v = fn()
            own += v or 0.0
            calls += 1
        out.append(own / calls if own else (time.perf_counter() - t0) * 1e3 / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-seconds', type=float, default=0.5)
    ap.add_argument('--no-twin', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'iss_probe.txt'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('iss_probe: no device (the probe measures the device; there is no fallback)')
    import fpfh_fixture as F
    import iss_twin
    import outlier_twin
    from se3et_amd import ops
    from se3et_amd.fpfh import global_registration_pairs
    from se3et_amd.iss import iss_keypoints_clouds, model_resolution_clouds
    from se3et_amd.scan_prep import remove_radius_outlier_clouds, remove_statistical_outlier_clouds
    from se3et_amd.stacking import identities, lengths, stack
    lines = ['iss_probe: %s, median (min .. max) over %d windows of >= %.1f s, ms per call.  Recorded, not gated; the twin rows are the numpy '
             'restatements of tests/iss_twin.py and tests/outlier_twin.py on the same box, once, on one cloud of 5 000 points.'
             % (torch.cuda.get_device_name(0), args.windows, args.window_seconds)]
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

    for label, clouds, n in (('16 x 5k', 16, 5000), ('1 x 20k', 1, 20000)):
        host = [F.surface(n, 100 + c)[0].astype(np.float32) for c in range(clouds)]
        pts = [torch.from_numpy(p).cuda() for p in host]
        res = float(model_resolution_clouds(pts)[0])
        rs, rn = 6.0 * res, 4.0 * res
        keys = iss_keypoints_clouds(pts, rs, rn)
        p, pl = stack(pts), lengths(pts)
        state = {}

        def search():
            grid = ops.pair_grid_build(p, pl, identities(clouds), rs)
            ro = ops.pair_ball_count_stack(grid, p, pl, rs)
            state['total'] = state.get('total') or int(ro[-1])               # (the read-back of the first call only)
            state['ro'], state['pairs'] = ro, ops.pair_ball_fill_stack(grid, p, pl, rs, ro, state['total'])
        t_search = timed(search)
        sal = torch.empty((p.shape[0],), dtype=torch.float64, device=p.device)
        t_sal = timed(lambda: ops.iss_saliency_stack(p, pl, state['ro'], state['pairs'], 0.975, 0.975, 5, sal))
        t_sel = timed(lambda: ops.iss_select_stack(ops.pair_grid_build(p, pl, identities(clouds), rn), p, pl, rn, sal, 5))

        def knn_mean():
            state['a'] = ops.knn_distance_stack(ops.pair_grid_build(p, pl, identities(clouds), 0.0), p, pl, 20, -1)
        t_knn = timed(knn_mean)
        t_stats = timed(lambda: ops.distance_stats_stack(state['a'], pl, 2.0))
        total = state['total']
        lines.append('%s points, model resolution %.5f, salient radius %.4f, non-max radius %.4f: %d list entries, %.1f members per row, '
                     '%d keypoints' % (label, res, rs, rn, total, total / (clouds * n), sum(len(k) for k in keys)))
        lines.append('  iss_keypoints_clouds (radii given), host wall   %10.3f (%.3f .. %.3f)' % wall_of(lambda: iss_keypoints_clouds(pts, rs, rn)))
        lines.append('  iss_keypoints_clouds (radius 0), host wall      %10.3f (%.3f .. %.3f)' % wall_of(lambda: iss_keypoints_clouds(pts)))
        lines.append('  model_resolution_clouds, host wall              %10.3f (%.3f .. %.3f)' % wall_of(lambda: model_resolution_clouds(pts)))
        lines.append('  remove_statistical_outlier_clouds, host wall    %10.3f (%.3f .. %.3f)'
                     % wall_of(lambda: remove_statistical_outlier_clouds(pts, 20, 2.0)))
        lines.append('  remove_radius_outlier_clouds, host wall         %10.3f (%.3f .. %.3f)' % wall_of(lambda: remove_radius_outlier_clouds(pts, 16, rs)))
        lines.append('  search (grid, count, fill), device events       %10.3f (%.3f .. %.3f)' % t_search)
        lines.append('  saliency pass, device events                    %10.3f (%.3f .. %.3f)   %.3f ns per list entry' % (t_sal + (t_sal[0] * 1e6 / total,)))
        lines.append('  selection pass (grid, walk), device events      %10.3f (%.3f .. %.3f)' % t_sel)
        lines.append('  k-NN mean pass (grid, k = 20), device events    %10.3f (%.3f .. %.3f)' % t_knn)
        lines.append('  statistics (two sums, mask), device events      %10.3f (%.3f .. %.3f)' % t_stats)
        if not args.no_twin and clouds > 1:
            one = host[0].astype(np.float64)
            t0 = time.perf_counter()
            want = iss_twin.compute(one, rs, rn)
            t_iss = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            stat = outlier_twin.statistical(one, 20, 2.0)
            t_out = (time.perf_counter() - t0) * 1e3
            got = iss_keypoints_clouds(pts[:1], rs, rn)[0].cpu().numpy()
            kept = remove_statistical_outlier_clouds(pts[:1], 20, 2.0)[0].cpu().numpy()
            w1 = wall_of(lambda: iss_keypoints_clouds(pts[:1], rs, rn))[0]
            w2 = wall_of(lambda: remove_statistical_outlier_clouds(pts[:1], 20, 2.0))[0]
            lines.append('  ISS twin (numpy), one cloud, host wall          %10.3f   %.0fx the device call on that cloud (%.3f); keypoints equal: %s, %d '
                         'rows flagged or tainted' % (t_iss, t_iss / w1, w1, np.array_equal(got, np.flatnonzero(want['keypoint'])),
                                                      int((want['flagged'] | want['tainted']).sum())))
            lines.append('  outlier twin (numpy), one cloud, host wall      %10.3f   %.0fx the device call on that cloud (%.3f); masks equal: %s, %d rows '
                         'flagged' % (t_out, t_out / w2, w2, np.array_equal(kept, np.flatnonzero(stat['keep'])), int(stat['flagged'].sum())))
    # the pipeline with and without the detector
    Rm, t = F.rotation(F.MOTION_ROTVEC), np.asarray(F.MOTION_SHIFT)
    refs = [F.surface(5000, 200 + c)[0] for c in range(4)]
    srcs = [(q @ Rm.T + t)[np.random.default_rng(c).permutation(len(q))] for c, q in enumerate(refs)]
    src, ref = [torch.from_numpy(a).cuda() for a in srcs], [torch.from_numpy(a).cuda() for a in refs]
    v = 0.05
    lines.append('global_registration_pairs, 4 pairs of 5 000 points, voxel size %.2f, RANSAC (50 000 iterations, mutual filter), ICP at 1.5 voxel '
                 'sizes:' % v)
    for name, extra in (('no detector (the parent\'s path)', {}),
                        ("keypoints='iss', radii 2.5 / 1.5 voxel sizes", {'keypoints': 'iss', 'iss_options': {'salient_radius': 2.5 * v,
                                                                                                             'non_max_radius': 1.5 * v}})):
        out = global_registration_pairs(src, ref, v, icp_distance=1.5 * v, seed=0, **extra)
        wall = wall_of(lambda: global_registration_pairs(src, ref, v, icp_distance=1.5 * v, seed=0, **extra))
        rows = [len(k) for k in out['src_keypoints']] if out.get('src_keypoints') is not None else [len(c) for c in out['src_points']]
        matched = [len(c) for c in out['ransac']['correspondences']]
        errs = []
        for T in out['transforms'].cpu().numpy():
            rre = np.degrees(np.arccos(np.clip((np.trace(T[:3, :3] @ Rm) - 1.0) / 2.0, -1.0, 1.0)))
            errs.append((rre, np.linalg.norm(T[:3, 3] - (-Rm.T @ t))))
        lines.append('  %-46s %10.3f (%.3f .. %.3f)   src rows offered %s of %s, matched %s; worst RRE %.3f deg, worst RTE %.4f'
                     % ((name + ', host wall',) + wall + (rows, [len(c) for c in out['src_points']], matched, max(e[0] for e in errs),
                                                          max(e[1] for e in errs))))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
