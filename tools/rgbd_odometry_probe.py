"""Cost of RGB-D odometry on the device (se3et_amd.odometry) next to the numpy twin (tests/rgbd_odometry_twin.py) on the same box
(profiles/rgbd_odometry_probe.txt).

Workload: 640 x 480 uint16 depth and uint8 RGB frames of the scene of tests/rgbd_odometry_fixture.py on its 6-frame orbit, walked up and down (neighbours
differ by about 1 degree and 3 cm), the default schedule of 20, 10 and 5 iterations on three levels, method hybrid; 1 pair (2 frames) and 32 pairs
(33 frames, every pair (i, i + 1), so every inner frame is shared by two pairs).  Per workload: the device-event time of
rgbd_odometry_pairs as the median (min .. max) over --windows windows of at least --window-seconds each after a warm-up; the same for the
preparation alone (the C entry without pairs); the split of one call's kernel time between preparation, correspondence, accumulation and
solve launches from torch.profiler's device activities (left out, and said so, where the profiler reports no kernels of the library).
The twin runs the same pair once.  Recorded, not gated.  Run `python tools/rgbd_odometry_probe.py [--out FILE]` on the GPU box."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

GROUPS = (('preparation', ('rgbd_gauss', 'rgbd_down', 'rgbd_sobel')), ('correspondence', ('rgbd_claim',)), ('accumulation', ('rgbd_sums',)),
          ('solve', ('rgbd_finish', 'rgbd_init')))


def spread(values):
    return statistics.median(values), min(values), max(values)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--window-seconds', type=float, default=0.5)
    ap.add_argument('--no-twin', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rgbd_odometry_probe.txt'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('rgbd_odometry_probe: no device (the probe measures the device; there is no fallback)')
    import rgbd_odometry_fixture as F
    from se3et_amd import ops
    from se3et_amd.odometry import rgbd_odometry_pairs
    H, W = 480, 640
    K = F.intrinsics(H, W)
    arc = F.orbit_poses(6)
    poses = [arc[abs((k + 5) % 10 - 5)] for k in range(33)]             # up and down the arc: 0 1 2 3 4 5 4 3 2 1 0 1 ..
    depths, colors = F.frames(poses, H, W)
    lines = ['RGB-D odometry, %d x %d, iterations (20, 10, 5), hybrid, on %s' % (W, H, torch.cuda.get_device_name(0)),
             'event times in ms: median (min .. max) over %d windows of >= %.1f s' % (args.windows, args.window_seconds), '']

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.windows):
            calls, own, t0 = 0, 0.0, time.perf_counter()
            while time.perf_counter() - t0 < args.window_seconds or calls < 3:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                own += a.elapsed_time(b)
                calls += 1
            out.append(own / calls)
        return spread(out)

    for P in (1, 32):
        d, c = torch.from_numpy(depths[:P + 1]).cuda(), torch.from_numpy(colors[:P + 1]).cuda()
        out = rgbd_odometry_pairs(d, c, K)
        ok = int(out['success'].sum())
        whole = timed(lambda: rgbd_odometry_pairs(d, c, K))
        prep = timed(lambda: _prepare_only(ops, d, c))
        lines.append('%2d pairs, %2d frames: whole call %.3f (%.3f .. %.3f); preparation alone %.3f (%.3f .. %.3f); %d of %d pairs succeeded'
                     % ((P, P + 1) + whole + prep + (ok, P)))
        lines.append('      %.3f ms per pair; %d launches of the schedule per call' % (whole[0] / P, 3 * (35 + 2) + 2))
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                rgbd_odometry_pairs(d, c, K)
                torch.cuda.synchronize()
            totals = {name: 0.0 for name, _keys in GROUPS}
            for ev in prof.key_averages():
                for name, keys in GROUPS:
                    if any(k in ev.key for k in keys):
                        totals[name] += getattr(ev, 'device_time_total', getattr(ev, 'cuda_time_total', 0.0)) / 1e3
            if sum(totals.values()) > 0:
                lines.append('      kernel time of one call, ms: ' + ', '.join('%s %.3f' % (k, v) for k, v in totals.items()))
            else:
                lines.append('      kernel split: the profiler reported no kernels of the library; not recorded')
        except Exception as e:                                              # the split is an extra: the event times above stand without it
            lines.append('      kernel split: not recorded (%s)' % type(e).__name__)
        if P == 1:
            err = F.motion_error(out['transforms'][0].cpu().numpy(), poses[1])
            lines.append('      recovered motion off by %.4f degrees, %.3f mm' % err)
    if not args.no_twin:
        case = dict(depths=depths[:2], colors=colors[:2], K=K, pairs=[(0, 1)], T0=np.eye(4)[None], method='hybrid', iterations=(20, 10, 5),
                    max_depth_diff=0.03, **F.CONVERT)
        t0 = time.perf_counter()
        r = F.twin_results_of(case)[0]
        lines += ['', 'numpy twin, one pair, exact sums: %.1f s (success %s, %d correspondences)' % (time.perf_counter() - t0, r['success'],
                                                                                                 r['correspondences'])]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


def _prepare_only(ops, d, c):
    """the preparation launches alone: the C entry without pairs"""
    import torch
    flags = torch.ones((d.shape[0],), dtype=torch.uint8, device=d.device)
    ws = ops.rgbd_frames_workspace(d, 3)
    ops.rgbd_odometry_stack(d, c, flags, ws, True, [], [], torch.zeros((0, 4, 4), dtype=torch.float64, device=d.device), 'hybrid', (20, 10, 5))


if __name__ == '__main__':
    main()
