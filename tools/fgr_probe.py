"""The figures that tests/test_fgr_cpu.py's bounds rest on, and the cost of Fast Global Registration on the device
(profiles/fgr_probe.txt).

Without a GPU: over every case of tests/fgr_fixture.py (all families, both input types) the largest |T - T_twin| of se3_debug_fgr_host
against the float64 twin tests/fgr_twin.py; the twin's own error against the ground truth per family (the known-answer tests allow five
times it); each family's largest step angle; and the largest error of the update's sine and cosine (se3_debug_fgr_sincos_host) against
numpy.sin / numpy.cos on (-4, 4).  The test bound is the largest deviation times 16, for seeds and summation order, rounded up to a power of
ten, and never above 1e-8.
With a GPU, recorded and not gated: the median (min .. max) host wall time, ended by a device synchronise, of fgr.fgr_pairs for 32 pairs of
3 000 correspondences (half of them wrong, noise 0.002), with and without the tuple test and the evaluation, and beside it
ransac.ransac_pairs at 50 000 hypotheses on the same correspondences; every shape warmed up first.
`python tools/fgr_probe.py [--iters N] [--out FILE]`; without a device the timing rows say so."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def power_of_ten_above(x):
    return 10.0 ** math.ceil(math.log10(x))


def deviation():
    import fgr_fixture as F
    rows = []
    for name in sorted(F.FAMILIES):
        for dtype in ('float32', 'float64'):
            c = F.case(name, dtype)
            got, twin = F.host_fgr(c['src'], c['ref'], c['corr'], **c['options']), c['twin']
            rows.append((name, dtype, len(twin['tuples']), len(twin['trials']), twin['status'],
                         float(np.abs(got['transform'] - twin['transform']).max()), F.transform_error(twin['transform'], c['gt']),
                         F.transform_error(got['transform'], c['gt']), twin['max_angle']))
    return rows


def series_error(n=200001):
    from se3et_amd._lib import check, lib
    x = np.linspace(-4.0, 4.0, n)[1:-1].copy()
    s, c = np.zeros_like(x), np.zeros_like(x)
    check(lib().se3_debug_fgr_sincos_host(x.ctypes.data, len(x), s.ctypes.data, c.ctypes.data), 'se3_debug_fgr_sincos_host')
    return len(x), float(max(np.abs(s - np.sin(x)).max(), np.abs(c - np.cos(x)).max()))


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
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fgr_probe.txt'))
    args = ap.parse_args()
    import torch
    rows = deviation()
    worst = max(r[5] for r in rows)
    bound = min(power_of_ten_above(16.0 * worst), 1e-8)
    lines = ['deviation of se3_debug_fgr_host from the float64 twin over the %d fixture cases: largest %.2e; the test bound is 16 times that, '
             'rounded up to a power of ten and at most 1e-8: bound %.0e' % (len(rows), worst, bound)]
    for name, dtype, ncorr, ntrials, status, dT, twin_err, host_err, angle in rows:
        lines.append('  case %-18s %-8s |C\'| %4d  kept trials %4d  status %2d  |dT| %.2e  twin error %.2e  host error %.2e  largest step angle %.4f'
                     % (name, dtype, ncorr, ntrials, status, dT, twin_err, host_err, angle))
    n, err = series_error()
    lines.append('series: largest |sin - numpy.sin|, |cos - numpy.cos| of the update\'s sine and cosine over %d points of (-4, 4): %.2e; the '
                 'test allows 1e-14' % (n, err))
    if torch.cuda.is_available():
        import fgr_fixture as F
        from se3et_amd import fgr, ransac
        P, K = 32, 3000
        pairs = [F.pair(seed=100 + p, n=K, degrees=30.0 + 4.5 * p, mismatch=0.5, noise=0.002) for p in range(P)]
        srcs = [torch.from_numpy(p[0].astype(np.float32)).cuda() for p in pairs]
        refs = [torch.from_numpy(p[1].astype(np.float32)).cuda() for p in pairs]
        corrs = [torch.from_numpy(p[2]).cuda() for p in pairs]
        lines.insert(0, 'fgr_probe: %s, %d stacked pairs of %d + %d points and %d correspondences (half wrong, noise 0.002), float32; median '
                        '(min .. max) of %d calls, ms, host wall ended by a device synchronise.  `python tools/fgr_probe.py --iters %d`.  '
                        'Recorded, not gated.' % (torch.cuda.get_device_name(0), P, K, K, K, args.iters, args.iters))
        runs = (('fgr_pairs', dict()), ('fgr_pairs, no evaluation', dict(evaluate=False)),
                ('fgr_pairs, no tuple test, no evaluation', dict(evaluate=False, tuple_test=False)))
        for label, kw in runs:
            fn = lambda: fgr.fgr_pairs(srcs, refs, corrs, **kw)
            out = fn()
            errs = [F.transform_error(T, p[3]) for T, p in zip(out['transforms'].cpu().numpy(), pairs)]
            lines.append('  %-42s %9.3f (%.3f .. %.3f)   kept trials %d .. %d, largest transform error %.1e, status %s'
                         % ((label,) + timed(fn, args.iters) + (int(out['num_tuples'].min()), int(out['num_tuples'].max()), max(errs),
                                                                sorted(set(out['status'].cpu().tolist())))))
        fn = lambda: ransac.ransac_pairs(srcs, refs, 0.025, 3, 50000, 0, correspondences=corrs)
        out = fn()
        errs = [F.transform_error(T, p[3]) for T, p in zip(out['transforms'].cpu().numpy().astype(np.float64), pairs)]
        lines.append('  %-42s %9.3f (%.3f .. %.3f)   largest transform error %.1e, smallest fitness %.3f'
                     % (('ransac_pairs, 50 000 hypotheses, r = 0.025',) + timed(fn, args.iters) + (max(errs), float(out['fitness'].min()))))
    else:
        lines.insert(0, 'fgr_probe: run without a device: the deviation only')
        lines.append('32 pairs of 3 000 correspondences, fgr_pairs and ransac_pairs at 50 000 hypotheses: not measured')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
