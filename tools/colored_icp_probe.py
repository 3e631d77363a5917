"""The largest deviation of se3_debug_color_gradient_host and se3_debug_icp_colored_host (csrc/color_gradient.hip, csrc/icp_colored_core.h
on host memory) from the float64 twin tests/colored_icp_twin.py, and, with --gpu, the cost of the gradient call and of a coloured
iteration next to point-to-plane (profiles/colored_icp_probe.txt).

Deviation (no GPU needed): over every case of tests/colored_icp_fixture.py -- four families x losses None, l2, huber, tukey x float32 /
float64, the host gradients feeding the host loop and the twin's gradients the twin's -- the largest |T - T_twin| and |rmse - rmse_twin|;
over the families' reference clouds and the edge clouds of the gradient test the largest |g - g_twin|; and the largest |g - g_known| on
the known plane.  Each bound of tests/test_colored_icp_cpu.py is 16 times its figure, rounded up to a power of ten.
Timing (--gpu): 16 stacked pairs of 5 000 + 5 000 points and one pair of 120 000 + 120 000 points of the textured sheet, float32: the
gradient call of the reference clouds (k nearest, then the gradient kernel), 30 coloured iterations (both criteria at 0, the gradients
given as zeros without a search, so that the loop alone is timed), the whole coloured call, and icp_pairs(estimation='point_to_plane')
with 30 iterations on the same inputs and normals.  Median (min .. max) of --iters calls after a warm-up, host wall time ended by a
device synchronise.  Recorded, not gated.
Run `python tools/colored_icp_probe.py [--gpu] [--iters N] [--out FILE]`."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def loop_deviation():
    import colored_icp_fixture as X
    rows = []
    for name in sorted(X.FAMILIES):
        for loss in X.LOSSES:
            for dtype in ('float32', 'float64'):
                c = X.case(name, loss, dtype)
                got, _g = X.host_case(c, loss)
                t = c['twin']
                rows.append((name, str(loss), dtype, t['iterations'], t['status'], t['fitness'],
                             float(np.abs(got['transform'] - t['transform']).max()), abs(got['rmse'] - t['rmse'])))
    return rows


def gradient_deviation():
    import colored_icp_fixture as X
    import colored_icp_twin as C
    rows = []
    for dtype in ('float32', 'float64'):
        for name in sorted(X.FAMILIES):
            c = X.gradient_case(name, dtype)
            g, _status = X.host_gradients(c['ref'], c['normals'], c['ref_colors'], c['gradient_radius'])
            rows.append((name, dtype, len(g), int((c['members'] < 4).sum()), float(np.abs(g - c['twin_gradients']).max())))
        for kind in X.CLOUD_SIZES + ('duplicates', 'sparse'):
            p, nr, col, radius = X.small_cloud(kind, dtype)
            g, _status = X.host_gradients(p, nr, col, radius)
            want, m, _margins = C.gradients(p, nr, col, radius)
            rows.append(('cloud %s' % kind, dtype, len(g), int((m < 4).sum()), float(np.abs(g - want).max()) if len(g) else 0.0))
    p, nr, col, radius, known = X.known_plane()
    g, _status = X.host_gradients(p, nr, col, radius)
    _want, m, _margins = C.gradients(p, nr, col, radius)
    return rows, float(np.abs(g[m >= 4] - known).max())


def timing(iters):
    import torch
    import colored_icp_fixture as X
    import icp_fixture as F
    from se3et_amd import icp, scan_prep
    lines = []
    for pairs, n, r in ((16, 5000, 0.05), (1, 120000, 0.02)):
        rng = np.random.default_rng(n)
        ref, nrm = F.sheet(rng, n)
        on_ref, _ = F.sheet(rng, n)
        gt = F.rigid(rng, 25.0, 0.5)
        inv = np.linalg.inv(gt)
        src = on_ref @ inv[:3, :3].T + inv[:3, 3]
        T0 = F.rigid(rng, 1.0, 0.2 * r) @ gt
        dev = lambda a: [torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).cuda() for _ in range(pairs)]
        srcs, refs, nrms = dev(src), dev(ref), dev(nrm)
        scol, rcol = dev(X.texture(on_ref[:, 0], on_ref[:, 1])), dev(X.texture(ref[:, 0], ref[:, 1]))
        T = torch.from_numpy(np.stack([T0] * pairs)).cuda()
        all30 = dict(relative_fitness=0.0, relative_rmse=0.0, max_iteration=30)
        calls = (('gradient call (k nearest 30 + gradients, radius %g)' % (2 * r), lambda: icp.color_gradient_clouds(refs, nrms, rcol, 2 * r)),
                 ('30 coloured iterations (gradients given: no search)',
                  lambda: icp.colored_icp_pairs(srcs, refs, T, r, scol, rcol, nrms, gradient_radius=0.0, **all30)),
                 ('coloured call: gradients + 30 iterations', lambda: icp.colored_icp_pairs(srcs, refs, T, r, scol, rcol, nrms, **all30)),
                 ('30 point-to-plane iterations', lambda: icp.icp_pairs(srcs, refs, T, r, 'point_to_plane', nrms, **all30)))
        lines.append('  %d pair%s of %d + %d points, r = %g, float32:' % (pairs, 's' if pairs > 1 else '', n, n, r))
        for label, fn in calls:
            out = fn()
            torch.cuda.synchronize()
            times = []
            for _ in range(iters):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            made = '   %d iterations per pair' % out['iterations'].cpu().tolist()[0] if isinstance(out, dict) else ''
            lines.append('    %-58s %9.3f (%.3f .. %.3f)%s' % (label, statistics.median(times), min(times), max(times), made))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpu', action='store_true')
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'colored_icp_probe.txt'))
    args = ap.parse_args()
    import torch          # (before the library is loaded, as the other probes do: the library then binds to the HIP runtime torch brings)
    lines = []
    rows = loop_deviation()
    lines.append('deviation of the host gradients + se3_debug_icp_colored_host from the float64 twin over the %d fixture cases: largest %.2e '
                 '(transform or rmse); the test bound is 16 times that, rounded up to a power of ten.' % (len(rows), max(max(r[6], r[7]) for r in rows)))
    for name, loss, dtype, its, status, fit, dT, dr in rows:
        lines.append('  %-12s %-6s %-8s %2d iterations  status %2d  fitness %.3f  |dT| %.2e  |drmse| %.2e' % (name, loss, dtype, its, status, fit, dT, dr))
    grows, known = gradient_deviation()
    lines.append('deviation of se3_debug_color_gradient_host from the twin over %d clouds: largest %.2e; the gradient bound is 16 times that, '
                 'rounded up to a power of ten.' % (len(grows), max(r[4] for r in grows)))
    for name, dtype, n, few, dg in grows:
        lines.append('  %-16s %-8s %5d rows  %3d with m < 4  |dg| %.2e' % (name, dtype, n, few, dg))
    lines.append('known plane (200 rows, intensity g . p + 0.7): largest |g - g_known| over the rows with m >= 4: %.2e; the known-answer bound is '
                 '16 times that, rounded up to a power of ten.' % known)
    if args.gpu:
        lines.insert(0, 'colored_icp_probe: %s; median (min .. max) of %d calls, ms, host wall.  `python tools/colored_icp_probe.py --gpu --iters %d`.  '
                        'Recorded, not gated.' % (torch.cuda.get_device_name(0), args.iters, args.iters))
        lines += timing(args.iters)
    else:
        lines.insert(0, 'colored_icp_probe: run without --gpu: the deviations only')
        lines.append('gradient call, 30 coloured iterations, point-to-plane: not measured')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
