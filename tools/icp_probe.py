"""Cost of the ICP refinement on the device (se3et_amd.icp.icp_pairs) next to the float64 twin (tests/icp_twin.py: scipy cKDTree, numpy)
on 16 threads of the same box, and the largest deviation of the library's host entry from the twin (profiles/icp_probe.txt).

Deviation: over every case of tests/icp_fixture.py (three families, both estimations, both input types) the largest |T - T_twin| and
|rmse - rmse_twin| of se3_debug_icp_host; tests/test_icp_cpu.py's bound is 16 times the larger, rounded up to a power of ten.  This part
needs no GPU.
Workloads, each point-to-point and point-to-plane (the reference normals computed once, outside the timing), float32 on the device:
  16 x (5 000 + 5 000) points of make_pair('c2_5k', i), from the ground truth turned by 2 degrees and shifted by 3 cm, r = 0.1;
  1 x (120 000 + 120 000) points of the c3_20k box (box_surface, the pair's transform as in make_pair), the same perturbation, r = 1.0.
Per workload and estimation, median (min .. max) of --iters repetitions after a warm-up of every shape, host wall time ended by a device
synchronise, with the iterations executed per pair; the twin once per pair (--host-iters runs of the whole workload), its tree queried
with workers=16.  These are recorded, not gated.  Run `python tools/icp_probe.py [--iters N] [--out FILE]` on the GPU box; without a
device the timing rows say so."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

MODES = ('point_to_point', 'point_to_plane')


def spread(times):
    return statistics.median(times), min(times), max(times)


def deviation():
    import icp_fixture as F
    rows = []
    for name in sorted(F.FAMILIES):
        for mode in MODES:
            for dtype in ('float32', 'float64'):
                c = F.case(name, mode, dtype)
                got = F.host_icp(c['src'], c['ref'], c['T0'], c['r'], mode, c['normals'])
                t = c['twin']
                rows.append((name, mode, dtype, t['iterations'], t['fitness'], float(np.abs(got['transform'] - t['transform']).max()),
                             abs(got['rmse'] - t['rmse']), min(e['gap_margin'] for e in t['evaluations']),
                             min(e['threshold_margin'] for e in t['evaluations'])))
    return rows


def perturbed(T, seed):
    import icp_fixture as F
    return F.rigid(np.random.default_rng(seed), 2.0, 0.03) @ np.asarray(T, np.float64)


def twin_run(pairs, r, mode, normals):
    """The twin's loop with a 16-thread tree query."""
    import icp_twin as W
    return [W.icp(src, ref, T0, r, mode, n, workers=16)['iterations'] for (src, ref, T0), n in zip(pairs, normals)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'icp_probe.txt'))
    args = ap.parse_args()
    import torch
    lines = []
    rows = deviation()
    worst = max(max(r[5], r[6]) for r in rows)
    lines.append('deviation of se3_debug_icp_host from the float64 twin over the fixture cases: largest %.2e (transform or rmse); '
                 'the test bound is 16 times that, rounded up to a power of ten' % worst)
    for name, mode, dtype, its, fit, dT, dr, gap, thr in rows:
        lines.append('  %-12s %-15s %-8s %2d iterations  fitness %.3f  |dT| %.2e  |drmse| %.2e  gap margin %.1e  threshold margin %.1e'
                     % (name, mode, dtype, its, fit, dT, dr, gap, thr))
    if torch.cuda.is_available():
        from se3et_amd import icp, scan_prep
        from se3et_amd.synthetic import PAIR_PRESETS, box_surface, euler_zyx, make_pair
        small = []
        for i in range(16):
            ref, src, T = make_pair('c2_5k', i)
            small.append((src, ref, perturbed(T, i)))
        n, dims, jitter = 120000, PAIR_PRESETS['c3_20k'][1], PAIR_PRESETS['c3_20k'][2]
        R, t = euler_zyx([0.5, 0.3, 0.2]), 0.05 * np.asarray(dims)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        big = [(((box_surface(n, dims, 2, jitter) - t) @ R).astype(np.float32), box_surface(n, dims, 1, jitter), perturbed(T, 99))]
        lines.insert(0, 'icp_probe: %s, median (min .. max) of %d runs (twin rows: %d runs), ms.  Recorded, not gated; the twin rows are '
                        'scipy / numpy on 16 threads of the same box -- Open3D is not installed here and was not timed.'
                     % (torch.cuda.get_device_name(0), args.iters, args.host_iters))
        for label, pairs, r in (('16 x (5k + 5k)', small, 0.1), ('1 x (120k + 120k)', big, 1.0)):
            srcs = [torch.from_numpy(p[0]).cuda() for p in pairs]
            refs = [torch.from_numpy(p[1]).cuda() for p in pairs]
            T0 = torch.from_numpy(np.stack([p[2] for p in pairs])).cuda()
            normals = scan_prep.estimate_normals_clouds(refs)
            host_normals = [x.cpu().numpy() for x in normals]
            lines.append('%s: %d + %d points, r = %g' % (label, sum(len(p[0]) for p in pairs), sum(len(p[1]) for p in pairs), r))
            for mode in MODES:
                fn = lambda: icp.icp_pairs(srcs, refs, T0, r, mode, normals)
                out = fn()
                torch.cuda.synchronize()
                times = []
                for _ in range(args.iters):
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times.append((time.perf_counter() - t0) * 1e3)
                g = spread(times)
                times = []
                for _ in range(args.host_iters):
                    t0 = time.perf_counter()
                    twin_its = twin_run(pairs, r, mode, host_normals)
                    times.append((time.perf_counter() - t0) * 1e3)
                c = spread(times)
                lines.append('  %-15s %10.3f (%.3f .. %.3f)   host wall; iterations per pair %s, converged %s'
                             % ((mode,) + g + (out['iterations'].cpu().tolist(), out['converged'].cpu().tolist())))
                lines.append('  %-15s %10.3f (%.3f .. %.3f)   host wall: %.0fx the device call; iterations per pair %s'
                             % (('twin ' + mode[9:],) + c + (c[0] / g[0], twin_its)))
    else:
        lines.insert(0, 'icp_probe: run without a device: the deviation only')
        lines.append('16 x (5k + 5k), 1 x (120k + 120k), both estimations: not measured')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
