"""Cost of the neighbour-limit calibration's histograms (se3et_amd.data.neighbor_histograms, csrc/radius_neighbors.hip: count-only
search) next to what a forward pays for its neighbour tables anyway (profiles/calibration_probe.txt).

Workloads: 16 stacked make_pair('c2_5k', i) pairs (3DMatch parameters: 4 stages, voxel 0.025, radius 0.0625, hist_n 180) and 2
make_pair('c3_4k', i) pairs (KITTI parameters: 5 stages, 0.3, 1.275, hist_n 607).  Per workload, median of --iters repetitions after a
warm-up of every shape:
  histograms   data.neighbor_histograms, host wall time of the call (it ends in its device-to-host copy)
    stages     data.stage_clouds alone (grid subsampling + the copy of the stage sizes), host wall
    counting   the count searches of all stages on prebuilt stage clouds, grids included, device events
  tables       data.precompute_data_stack_mode of the same clouds at limits [38, 36, 36, 38(, 38)], host wall: its stage building is the same
               call, the rest is the 3S-2 table searches
  table self   the S self searches of that pyramid alone (ops.radius_neighbors at the same limits, grids included), device events: the
               like-for-like of `counting`
  host         se3et_amd.ext.neighbor_histograms of the same clouds on the CPU with SE3_HOST_THREADS=16, host wall
Run `python tools/calibration_probe.py [--iters N] [--out FILE]` on the GPU box."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [('16 x c2_5k', 'c2_5k', 16, dict(num_stages=4, voxel_size=0.025, radius=0.0625), [38, 36, 36, 38]),
             ('2 x c3_4k', 'c3_4k', 2, dict(num_stages=5, voxel_size=0.3, radius=1.275), [38, 36, 36, 38, 38])]


def median_ms(fn, iters, events):
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
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=15)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('SE3_HOST_THREADS', '16')
    import torch
    from se3et_amd import data, ext, ops
    from se3et_amd.synthetic import make_pair
    if not torch.cuda.is_available():
        raise SystemExit('calibration_probe needs a GPU: times are not measured anywhere else')
    lines = ['calibration_probe: %s (%s), median (min .. max) of %d runs, ms'
             % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, args.iters)]
    fmt = lambda t: '%8.3f (%.3f .. %.3f)' % t
    for title, preset, pairs, p, limits in WORKLOADS:
        clouds = [c for i in range(pairs) for c in make_pair(preset, i)[:2]]
        host_pts = torch.from_numpy(np.concatenate(clouds))
        lengths = torch.tensor([len(c) for c in clouds], dtype=torch.int64)
        pts = host_pts.cuda()
        S, hist_n = p['num_stages'], data.calibration_hist_n(p['voxel_size'], p['radius'])
        points, lens = data.stage_clouds(pts, lengths, S, p['voxel_size'])
        radii = [p['radius'] * 2 ** i for i in range(S)]

        def counting():
            hist = torch.zeros((pairs * S, hist_n), dtype=torch.int32, device='cuda')
            for i in range(S):
                ops.radius_count_hist(points[i], points[i], lens[i], lens[i], radii[i], hist_n, data.pair_slots(pairs, S, i), hist=hist)

        def table_self():
            for i in range(S):
                ops.radius_neighbors(points[i], points[i], lens[i], lens[i], radii[i], limits[i])

        hist = data.neighbor_histograms(pts, lengths, S, p['voxel_size'], p['radius'])[0]
        lines.append('%s: %d stage-0 points, stage sizes %s, hist_n %d' % (title, pts.shape[0], [int(l.sum()) for l in lens], hist_n))
        lines.append('  histograms  %s   host wall' % fmt(median_ms(lambda: data.neighbor_histograms(pts, lengths, S, p['voxel_size'], p['radius']),
                                                                     args.iters, False)))
        lines.append('    stages    %s   host wall' % fmt(median_ms(lambda: data.stage_clouds(pts, lengths, S, p['voxel_size']), args.iters, False)))
        lines.append('    counting  %s   device events' % fmt(median_ms(counting, args.iters, True)))
        lines.append('  tables      %s   host wall' % fmt(median_ms(lambda: data.precompute_data_stack_mode(pts, lengths, S, p['voxel_size'], p['radius'],
                                                                                                                limits), args.iters, False)))
        lines.append('    table self %s  device events' % fmt(median_ms(table_self, args.iters, True)))
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            host_hist = ext.neighbor_histograms(host_pts, lengths, S, p['voxel_size'], p['radius'])[0]
            times.append((time.perf_counter() - t0) * 1e3)
        assert torch.equal(host_hist, hist)
        lines.append('  host        %s   host wall, SE3_HOST_THREADS=%s, 3 runs (same histograms as the device)'
                     % (fmt((statistics.median(times), min(times), max(times))), os.environ['SE3_HOST_THREADS']))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
