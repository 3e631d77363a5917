"""The largest deviation of se3_debug_icp_weighted_host (robust loss kernels, generalized ICP: csrc/icp_core.h on host memory) from the
float64 twin tests/icp_robust_twin.py, and, on a GPU, the cost of generalized ICP next to point-to-plane (profiles/icp_robust_probe.txt).

Deviation: over every case of tests/icp_robust_fixture.py -- three estimators x five losses x float32 / float64 on the three clean
families and the outlier family -- the largest |T - T_twin| and |rmse - rmse_twin|; tests/test_icp_robust_cpu.py's bound is 16 times the
larger, rounded up to a power of ten.  The largest condition number of the twin's 6x6 systems is recorded beside it.  No GPU needed.
Timing (with a device): 32 stacked sheet2048 pairs, float32, point-to-plane against generalized, each without a loss and with huber, at
Open3D's criteria and with both criteria at 0 (every pair makes all 30 updates; a call enqueues 63 launches either way); median
(min .. max) of --iters calls after a warm-up, host wall time ended by a device synchronise.  Recorded, not gated.
Run `python tools/icp_robust_probe.py [--iters N] [--out FILE]`; without a device the timing rows say so."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def deviation():
    import icp_robust_fixture as R
    import icp_robust_twin as W
    rows = []
    for name in sorted(R.FAMILIES):
        for mode in W.ESTIMATORS:
            for loss in W.LOSSES:
                for dtype in ('float32', 'float64'):
                    c = R.case(name, mode, loss, dtype)
                    got = R.host_weighted_icp(c['src'], c['ref'], c['T0'], c['r'], mode, c['normals'], c['src_normals'], loss, R.LOSS_K[loss])
                    t = c['twin']
                    rows.append((name, mode, loss, dtype, t['iterations'], t['status'], t['fitness'],
                                 float(np.abs(got['transform'] - t['transform']).max()), abs(got['rmse'] - t['rmse']), t['condition']))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'icp_robust_probe.txt'))
    args = ap.parse_args()
    import torch
    lines = []
    rows = deviation()
    worst = max(max(r[7], r[8]) for r in rows)
    lines.append('deviation of se3_debug_icp_weighted_host from the float64 twin over the %d fixture cases: largest %.2e (transform or rmse); '
                 'the test bound is 16 times that, rounded up to a power of ten.  Largest condition number of a 6x6 system: %.1e'
                 % (len(rows), worst, max(r[9] for r in rows)))
    for name, mode, loss, dtype, its, status, fit, dT, dr, cond in rows:
        lines.append('  %-12s %-15s %-7s %-8s %2d iterations  status %2d  fitness %.3f  |dT| %.2e  |drmse| %.2e  condition %.1e'
                     % (name, mode, loss, dtype, its, status, fit, dT, dr, cond))
    if torch.cuda.is_available():
        import icp_robust_fixture as R
        from se3et_amd import icp
        c = R.inputs('sheet2048', 'float32')
        dev = lambda a: [torch.from_numpy(a).cuda() for _ in range(32)]
        srcs, refs, nrm, snr = dev(c['src']), dev(c['ref']), dev(c['normals']), dev(c['src_normals'])
        T0 = torch.from_numpy(np.stack([c['T0']] * 32)).cuda()
        lines.insert(0, 'icp_robust_probe: %s, 32 stacked sheet2048 pairs (1900 + 2048 points each, r = %g), float32; median (min .. max) of '
                        '%d calls, ms, host wall.  `python tools/icp_robust_probe.py --iters %d`.  Recorded, not gated.'
                     % (torch.cuda.get_device_name(0), c['r'], args.iters, args.iters))
        rows = (('point_to_plane', lambda **kw: icp.icp_pairs(srcs, refs, T0, c['r'], 'point_to_plane', nrm, **kw)),
                ('point_to_plane huber', lambda **kw: icp.icp_pairs(srcs, refs, T0, c['r'], 'point_to_plane', nrm, loss='huber', loss_k=0.01, **kw)),
                ('generalized', lambda **kw: icp.generalized_icp_pairs(srcs, refs, T0, c['r'], snr, nrm, **kw)),
                ('generalized huber', lambda **kw: icp.generalized_icp_pairs(srcs, refs, T0, c['r'], snr, nrm, loss='huber', loss_k=0.01, **kw)))
        # at Open3D's criteria (a pair that has converged returns from its kernels at once), and with both criteria at 0: all 30 updates
        for what, kw in (("Open3D's criteria", {}), ('criteria 0: 30 updates', dict(relative_fitness=0.0, relative_rmse=0.0))):
            for label, fn in rows:
                out = fn(**kw)
                torch.cuda.synchronize()
                times = []
                for _ in range(args.iters):
                    t0 = time.perf_counter()
                    fn(**kw)
                    torch.cuda.synchronize()
                    times.append((time.perf_counter() - t0) * 1e3)
                lines.append('  %-22s %-24s %9.3f (%.3f .. %.3f)   %d iterations per pair'
                             % (label, what, statistics.median(times), min(times), max(times), out['iterations'].cpu().tolist()[0]))
    else:
        lines.insert(0, 'icp_robust_probe: run without a device: the deviation only')
        lines.append('32 x sheet2048, point-to-plane against generalized: not measured')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
