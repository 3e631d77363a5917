"""Cost of the pair ground truth on the device (se3et_amd.pair_geometry, csrc/pair_geometry.hip) next to the reference's own route on the same
box (profiles/pair_geometry_probe.txt).

Workloads: 16 make_pair('c2_5k', i) pairs (radii 0.05 / 0.0375, voxel 0.025), 2 make_pair('c3_20k', i) pairs (0.6 / 0.45, voxel 0.3) and the
demo pair of tests/golden/demo_se3ete.npz (0.05 / 0.0375, voxel 0.025), clouds resident on the device as float32.  Per workload and function,
median (min .. max) of --iters repetitions after a warm-up of every shape, all pairs of the workload in one call:
  nearest neighbour / overlap / correspondences / gt.info   the product call, host wall time (ended by a device synchronise; the calls that
               return lists or draw on the host end in their own read-back)
    grid       ops.pair_grid_build alone (nearest-neighbour grid, or the ball grid at the matching radius), device events
    search     the search kernels on the prebuilt grid (nearest neighbour; count + scan + fill), device events
  reference    the reference's route restated: per pair, src @ R^T + t, scipy cKDTree build plus query(k=1, workers=16) /
               query_ball_point plus the pair-list comprehension / the calibrate_ground_truth arithmetic, host wall, float64, --host-iters
               runs.  Without scipy the numpy twin is timed on ONE c1_2k pair instead and labelled as such.
Run `python tools/pair_geometry_probe.py [--iters N] [--out FILE]` on the GPU box."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

WORKLOADS = [('16 x c2_5k', 'c2_5k', 16, 0.05, 0.0375, 0.025), ('2 x c3_20k', 'c3_20k', 2, 0.6, 0.45, 0.3), ('demo pair', 'demo', 1, 0.05, 0.0375, 0.025)]


def spread(times):
    return statistics.median(times), min(times), max(times)


def timed(fn, iters, events):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        else:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    return spread(times)


def host_timed(fn, iters):
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return spread(times)


def reference_route(cKDTree, pairs, matching_radius, overlap_radius, voxel_size):
    """The four reference functions restated on float64 arrays (one tree per call, as the reference builds it)."""
    def moved(src, T):
        return src @ T[:3, :3].T + T[:3, 3]

    def nearest():
        return [cKDTree(moved(s, T)).query(r, k=1, workers=16) for r, s, T in pairs]

    def overlap():
        return [np.mean(cKDTree(moved(s, T)).query(r, k=1, workers=16)[0] < overlap_radius) for r, s, T in pairs]

    def correspondences():
        out = []
        for r, s, T in pairs:
            lists = cKDTree(moved(s, T)).query_ball_point(r, matching_radius)
            out.append(np.array([(i, j) for i, idx in enumerate(lists) for j in idx], dtype=np.int64))
        return out

    def info():
        out = []
        for r, s, T in pairs:
            m = moved(s, T)
            ov = np.mean(cKDTree(m).query(r, k=1, workers=16)[0] < 5 * voxel_size)
            d, i = cKDTree(m).query(r, k=1, workers=16)
            i = i[d < voxel_size]
            if len(i) > 5000:
                i = np.random.choice(i, 5000, replace=False)
            p = m[i]
            g = np.zeros([len(p), 3, 6])
            g[:, :3, :3] = np.eye(3)
            g[:, 0, 4], g[:, 0, 5], g[:, 1, 3], g[:, 1, 5], g[:, 2, 3], g[:, 2, 4] = p[:, 2], -p[:, 1], -p[:, 2], p[:, 0], p[:, 1], -p[:, 0]
            out.append((ov, np.matmul(g.transpose([0, 2, 1]), g).sum(0)))
        return out

    return nearest, overlap, correspondences, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=15)
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import pair_geometry_twin as twin
    from se3et_amd import ops, pair_geometry as PG
    if not torch.cuda.is_available():
        raise SystemExit('pair_geometry_probe needs a GPU: times are not measured anywhere else')
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    lines = ['pair_geometry_probe: %s (%s), median (min .. max) of %d runs, ms'
             % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, args.iters)]
    fmt = lambda t: '%9.3f (%.3f .. %.3f)' % t          # noqa: E731
    for title, preset, count, r_match, r_overlap, voxel in WORKLOADS:
        host = [twin.case_inputs(preset, i) for i in range(count)]
        refs, srcs = [torch.from_numpy(h[0]).cuda() for h in host], [torch.from_numpy(h[1]).cuda() for h in host]
        Ts = torch.from_numpy(np.stack([h[2] for h in host]).astype(np.float64))
        q, ql, s, sl = torch.cat(refs), [len(h[0]) for h in host], torch.cat(srcs), [len(h[1]) for h in host]
        corr = PG.get_correspondences_pairs(refs, srcs, Ts, r_match)
        total = sum(int(c.shape[0]) for c in corr)
        lines.append('%s: %d ref + %d src points, %d correspondences at %g' % (title, q.shape[0], s.shape[0], total, r_match))

        def nn_search(grid):
            return lambda: ops.pair_nearest_neighbor_stack(grid, q, ql)

        def ball_search(grid):
            def run():
                offsets = ops.pair_ball_count_stack(grid, q, ql, r_match)
                ops.pair_ball_fill_stack(grid, q, ql, r_match, offsets, total)
            return run

        device = {}
        for key, label, call, hint, search in (
                ('nn', 'nearest neighbour', lambda: PG.nearest_neighbor_pairs(refs, srcs, Ts, return_index=True), 0.0, nn_search),
                ('ov', 'overlap', lambda: PG.compute_overlap_pairs(refs, srcs, Ts, r_overlap), None, None),
                ('corr', 'correspondences', lambda: PG.get_correspondences_pairs(refs, srcs, Ts, r_match), r_match, ball_search),
                ('info', 'gt.info record', lambda: PG.calibrate_ground_truth_pairs(refs, srcs, Ts, voxel), None, None)):
            device[key] = timed(call, args.iters, False)
            lines.append('  %-18s%s   host wall' % (label, fmt(device[key])))
            if search is not None:
                lines.append('    %-16s%s   device events' % ('grid', fmt(timed(lambda: ops.pair_grid_build(s, sl, Ts, hint), args.iters, True))))
                lines.append('    %-16s%s   device events' % ('search', fmt(timed(search(ops.pair_grid_build(s, sl, Ts, hint)), args.iters, True))))
        if cKDTree is not None:
            pairs64 = [tuple(np.asarray(a, np.float64) for a in h) for h in host]
            for key, label, fn in zip(('nn', 'ov', 'corr', 'info'), ('nearest neighbour', 'overlap', 'correspondences', 'gt.info record'),
                                      reference_route(cKDTree, pairs64, r_match, r_overlap, voxel)):
                t = host_timed(fn, args.host_iters)
                lines.append('  reference %-18s%s   host wall, cKDTree, workers=16, %d runs: %.0fx the device call'
                             % (label, fmt(t), args.host_iters, t[0] / device[key][0]))
    if cKDTree is None:
        ref, src, T = twin.case_inputs('c1_2k')
        t = host_timed(lambda: twin.scan(ref, src, T.astype(np.float64), 0.05), args.host_iters)
        lines.append('scipy does not import on this box: no reference route.  The numpy twin (brute force) on ONE c1_2k pair, nearest neighbour and '
                     'correspondences in one pass: %s ms' % fmt(t).strip())
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
