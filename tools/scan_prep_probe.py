"""Cost of the scan preparation on the device (se3et_amd.scan_prep: voxel downsampling, k-NN 33, normals) next to a CPU restatement on 16
threads of the same box, and the solver constant K of the normals' direction bound (profiles/scan_prep_probe.txt).

Workloads: 16 clouds of 5 000 points (make_pair('c2_5k', i) ref clouds, voxel 0.025) in one call, and one cloud of 120 000 points
(box_surface on the c3_20k box, voxel 0.3), resident on the device as float32.  Per workload and function, median (min .. max) of --iters
repetitions after a warm-up of every shape, host wall time ended by a device synchronise (voxel downsampling ends in its own read-back):
  voxel downsampling / k-NN 33 / normals   the product call: voxel_downsample_clouds, knn_clouds, estimate_normals_clouds
  CPU      the restatement, float64, --host-iters runs: np.unique on the voxel keys + np.add.at for the means; scipy cKDTree build +
           query(k=33, workers=16); the same query + the covariances (einsum) + np.linalg.eigh.
These are recorded, not gated: nobody had measured them, and Open3D itself is not installed where this runs, so the library the reference
calls cannot be timed -- the CPU rows are numpy / scipy restatements of the same work, not Open3D.
K: the largest |n x n_twin| (l1 - l0) / (2^-53 l2) of the library's host entry against the numpy twin over the fixture clouds
(tests/scan_prep_fixture.py); the fixture's DIRECTION_K is 8 times that, rounded up to a power of two.  This part needs no GPU.
Run `python tools/scan_prep_probe.py [--iters N] [--out FILE]` on the GPU box."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

KNN = 33


def spread(times):
    return statistics.median(times), min(times), max(times)


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
    return spread(times)


def host_timed(fn, iters):
    fn()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return spread(times)


def cpu_voxel(clouds, v):
    for p in clouds:
        p = p.astype(np.float64)
        i = np.floor((p - (p.min(0) - 0.5 * v)) / v).astype(np.int64)
        _, inverse, counts = np.unique(i[:, 0] | (i[:, 1] << 21) | (i[:, 2] << 42), return_inverse=True, return_counts=True)
        s = np.zeros((len(counts), 3))
        np.add.at(s, inverse.reshape(-1), p)
        s /= counts[:, None]


def cpu_knn(clouds, normals):
    from scipy.spatial import cKDTree
    for p in clouds:
        p = p.astype(np.float64)
        _, idx = cKDTree(p).query(p, k=KNN, workers=16)
        if normals:
            nb = p[idx]
            d = nb - nb.mean(1, keepdims=True)
            np.linalg.eigh(np.einsum('nki,nkj->nij', d, d) / KNN)


def solver_K():
    import scan_prep_fixture as F
    rows = []
    for name in F.CLOUDS:
        _, _, tn, w = F.twin_normals(name)
        n, _ = F.host_normals(F.cloud(name))
        K, excluded = F.direction_K(n, tn, w)
        rows.append((name, len(n), float(K.max()), int(excluded.sum()), float(((w[:, 1] - w[:, 0]) / w[:, 2]).min())))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=15)
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scan_prep_probe.txt'))
    args = ap.parse_args()
    import torch
    from se3et_amd import scan_prep as S
    from se3et_amd.synthetic import PAIR_PRESETS, box_surface, make_pair
    lines = []
    rows = solver_K()
    lines.append('solver constant K of the direction bound (host entry against the numpy twin, k = %d): largest %.3f' % (KNN, max(r[2] for r in rows)))
    for name, n, K, excluded, gap in rows:
        lines.append('  %-12s %5d rows   K %.3f   excluded %d   smallest gap (l1 - l0) / l2 %.4f' % (name, n, K, excluded, gap))
    if torch.cuda.is_available():
        _, dims, jitter = PAIR_PRESETS['c3_20k']
        workloads = [('16 x 5k', [make_pair('c2_5k', i)[0] for i in range(16)], 0.025), ('1 x 120k', [box_surface(120000, dims, 1, jitter)], 0.3)]
        lines.insert(0, 'scan_prep_probe: %s, median (min .. max) of %d runs (CPU rows: %d runs), ms.  Recorded, not gated; the CPU rows are numpy / '
                        'scipy restatements on 16 threads of the same box -- Open3D is not installed here and was not timed.'
                     % (torch.cuda.get_device_name(0), args.iters, args.host_iters))
        for label, clouds, v in workloads:
            dev = [torch.from_numpy(c).cuda() for c in clouds]
            voxels = sum(len(c) for c in S.voxel_downsample_clouds(dev, v))
            lines.append('%s: %d points, %d voxels at %g' % (label, sum(len(c) for c in clouds), voxels, v))
            for what, fn, cpu in (('voxel downsampling', lambda: S.voxel_downsample_clouds(dev, v), lambda: cpu_voxel(clouds, v)),
                                  ('k-NN %d' % KNN, lambda: S.knn_clouds(dev, KNN), lambda: cpu_knn(clouds, False)),
                                  ('normals', lambda: S.estimate_normals_clouds(dev, KNN), lambda: cpu_knn(clouds, True))):
                g, c = timed(fn, args.iters), host_timed(cpu, args.host_iters)
                lines.append('  %-20s %9.3f (%.3f .. %.3f)   host wall' % ((what,) + g))
                lines.append('  %-20s %9.3f (%.3f .. %.3f)   host wall: %.0fx the device call' % (('CPU ' + what,) + c + (c[0] / g[0],)))
    else:
        lines.insert(0, 'scan_prep_probe: run without a device: the solver constant only, NO timings were taken')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
