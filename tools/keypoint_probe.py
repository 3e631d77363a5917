"""Cost of the keypoint selection on the device (se3et_amd.keypoints.nms_keypoints_clouds) next to the numpy loop of the float64 twin
(tests/keypoint_twin.py) on the same box (profiles/keypoint_probe.txt).

Workloads, uniform random points in the unit cube with distinct scores, float32 on the device, the radius 0.62 n^(-1/3) (about the mean
spacing: a third to a half of the points are suppressed; the share is printed):
  16 x 5 000 points at K = 2 500 and at K = None;
  1 x 20 000 points at K = 5 000 and at K = None.
Per workload: host wall time per call of nms_keypoints_clouds (ranking, grid build, selection, the read-back of the counts), ended by the
call's own synchronisation, and the rank inverse + selection kernels alone between two device events on a grid and an order built once.
Both as the median (min .. max) over --windows windows of at least --window-seconds each after a warm-up of every shape.  The twin runs
once per workload.  These are recorded, not gated.  Run `python tools/keypoint_probe.py [--out FILE]` on the GPU box."""
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'keypoint_probe.txt'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('keypoint_probe: no device (the probe measures the device; there is no fallback)')
    import keypoint_twin as twin
    from se3et_amd import ops
    from se3et_amd.keypoints import _rank_chunk, nms_keypoints_clouds
    from se3et_amd.stacking import identities, lengths, stack
    lines = ['keypoint_probe: %s, median (min .. max) over %d windows of >= %.1f s, ms per call.  Recorded, not gated; the twin rows are the '
             'numpy loop of tests/keypoint_twin.py on the same box, once per workload.' % (torch.cuda.get_device_name(0), args.windows,
                                                                                             args.window_seconds)]
    for label, clouds, n, K in (('16 x 5k', 16, 5000, 2500), ('1 x 20k', 1, 20000, 5000)):
        radius = 0.62 * n ** (-1.0 / 3.0)
        g = np.random.default_rng(n)
        host = [(g.uniform(0, 1, (n, 3)).astype(np.float32), (g.permutation(n) / n + 0.01).astype(np.float32)) for _ in range(clouds)]
        pts, scs = [torch.from_numpy(p).cuda() for p, _ in host], [torch.from_numpy(s).cuda() for _, s in host]
        for k in (K, None):
            got = nms_keypoints_clouds(pts, scs, radius, k)             # (the warm-up of this shape)
            full = nms_keypoints_clouds(pts, scs, radius)
            torch.cuda.synchronize()
            wall = spread(windows(lambda: nms_keypoints_clouds(pts, scs, radius, k) and None, args.windows, args.window_seconds))
            p, pl = stack(pts), lengths(pts)
            order, _ = _rank_chunk(scs, pl, p.device)
            grid = ops.pair_grid_build(p, pl, identities(clouds), radius)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def kernels():
                start.record()
                ops.keypoint_nms_stack(grid, order, pl, radius, k or 0)
                stop.record()
                stop.synchronize()
                return start.elapsed_time(stop)
            kernels()
            dev = spread(windows(kernels, args.windows, args.window_seconds))
            t0 = time.perf_counter()
            want = [twin.nms(pp, ss, radius, k) for pp, ss in host]
            t_twin = (time.perf_counter() - t0) * 1e3
            same = all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, want))
            lines.append('%s points, radius %.4f, K = %s: %d of %d points survive the full NMS (%.0f %% suppressed), %d returned; lists equal '
                         'to the twin\'s: %s' % (label, radius, k, sum(len(f) for f in full), clouds * n,
                                                100.0 * (1 - sum(len(f) for f in full) / (clouds * n)), sum(len(f) for f in got), same))
            lines.append('  nms_keypoints_clouds, host wall          %10.3f (%.3f .. %.3f)' % wall)
            lines.append('  rank inverse + selection, device events  %10.3f (%.3f .. %.3f)' % dev)
            lines.append('  twin (numpy loop), host wall             %10.3f   %.0fx the device call' % (t_twin, t_twin / wall[0]))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
