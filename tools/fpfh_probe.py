"""Cost of the FPFH descriptor on the device (se3et_amd.fpfh.compute_fpfh_clouds) next to the numpy twin (tests/fpfh_twin.py) on the same
box (profiles/fpfh_probe.txt).

Workloads: points of the test surface (tests/fpfh_fixture.py: z = 0.3 sin(3x) cos(2y) + 0.1 x^2 over [-1, 1]^2, analytic normals), float32
on the device, a radius search at the radius that gives about 60 neighbours (the mean is printed):
  16 x 5 000 points at radius 0.124;   1 x 20 000 points at radius 0.062.
Per workload: host wall time per call of compute_fpfh_clouds (check, grid build, count, the one read-back, fill, both passes), ended by a
synchronisation, and between device events the search (grid build, count, fill), the SPFH pass and the FPFH pass, each alone on inputs
built once.  All as the median (min .. max) over --windows windows of at least --window-seconds each after a warm-up of every shape.  The
twin runs once per workload.  The neighbour list's size is printed: the pair budget of a call.  These are recorded, not gated.
Run `python tools/fpfh_probe.py [--out FILE]` on the GPU box."""
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fpfh_probe.txt'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('fpfh_probe: no device (the probe measures the device; there is no fallback)')
    import fpfh_fixture as F
    import fpfh_twin as twin
    from se3et_amd import ops
    from se3et_amd.fpfh import compute_fpfh_clouds
    from se3et_amd.stacking import identities, lengths, stack
    lines = ['fpfh_probe: %s, median (min .. max) over %d windows of >= %.1f s, ms per call.  Recorded, not gated; the twin rows are the numpy '
             'restatement of tests/fpfh_twin.py on the same box, once per workload.' % (torch.cuda.get_device_name(0), args.windows,
                                                                                      args.window_seconds)]
    for label, clouds, n, radius in (('16 x 5k', 16, 5000, 0.124), ('1 x 20k', 1, 20000, 0.062)):
        host = [tuple(a.astype(np.float32) for a in F.surface(n, 100 + c)) for c in range(clouds)]
        pts, nrs = [torch.from_numpy(p).cuda() for p, _ in host], [torch.from_numpy(nr).cuda() for _, nr in host]
        got = compute_fpfh_clouds(pts, nrs, radius)                          # (the warm-up of this shape)
        torch.cuda.synchronize()

        def call():
            compute_fpfh_clouds(pts, nrs, radius)
            torch.cuda.synchronize()
        wall = spread(windows(call, args.windows, args.window_seconds))
        p, nr, pl = stack(pts), stack(nrs), lengths(pts)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        state = {}

        def timed(fn):
            def run():
                start.record()
                fn()
                stop.record()
                stop.synchronize()
                return start.elapsed_time(stop)
            run()
            return spread(windows(run, args.windows, args.window_seconds))

        def search():
            grid = ops.pair_grid_build(p, pl, identities(clouds), radius)
            ro = ops.pair_ball_count_stack(grid, p, pl, radius)
            state['total'] = state.get('total') or int(ro[-1])               # (the read-back of the first call only)
            state['ro'], state['pairs'] = ro, ops.pair_ball_fill_stack(grid, p, pl, radius, ro, state['total'])
        t_search = timed(search)
        spfh, fpfh = torch.empty((p.shape[0], 33), dtype=torch.float64, device=p.device), torch.empty((p.shape[0], 33), dtype=torch.float64,
                                                                                                     device=p.device)
        t_spfh = timed(lambda: ops.spfh_stack(p, nr, pl, state['ro'], state['pairs'], spfh))
        t_fpfh = timed(lambda: ops.fpfh_stack(p, spfh, pl, state['ro'], state['pairs'], fpfh))
        total = state['total']
        lines.append('%s points, radius %.3f: %d list entries, %.1f neighbours per row, %.1f MB of list (16 bytes per entry)'
                     % (label, radius, total, total / (clouds * n) - 1.0, total * 16 / 1e6))
        lines.append('  compute_fpfh_clouds, host wall                 %10.3f (%.3f .. %.3f)' % wall)
        lines.append('  search (grid, count, fill), device events      %10.3f (%.3f .. %.3f)' % t_search)
        lines.append('  SPFH pass, device events                       %10.3f (%.3f .. %.3f)   %.3f ns per list entry' % (t_spfh + (t_spfh[0] * 1e6 / total,)))
        lines.append('  FPFH pass, device events                       %10.3f (%.3f .. %.3f)   %.3f ns per list entry' % (t_fpfh + (t_fpfh[0] * 1e6 / total,)))
        if not args.no_twin:
            t0 = time.perf_counter()
            want = [twin.compute(pp, nn, radius) for pp, nn in host]
            t_twin = (time.perf_counter() - t0) * 1e3
            flagged = sum(int(w['tainted'].sum()) for w in want)
            same = sum(int((a.cpu().numpy() == w['fpfh']).all(1).sum()) for a, w in zip(got, want))
            lines.append('  twin (numpy), host wall                        %10.3f   %.0fx the device call; %d of %d rows equal to the twin\'s bit for '
                         'bit, %d rows with a flagged pair in reach' % (t_twin, t_twin / wall[0], same, clouds * n, flagged))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
