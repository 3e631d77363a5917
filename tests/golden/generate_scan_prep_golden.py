"""Fixture generator of the scan preparation (runs ONLY where the reference tree exists; data only travels).

Imports the genuine reference through oracle/ref_shims.py: regularize_normals (geotransformer/utils/pointcloud.py:25-37) and
modified_chamfer_distance (geotransformer/modules/registration/metrics.py:8-44).  Open3D is not installed where this runs, so the voxel
downsampling and the normal estimation have no fixture: their yardstick is the numpy twin (tests/scan_prep_twin.py).

Writes tests/golden/scan_prep.npz:
  reg/points, reg/normals (float64, row 0 with dot == 0 exactly), reg/positive, reg/negative   regularize_normals at positive=True / False
  mcd/raw (2, 300, 3), mcd/ref (2, 200, 3), mcd/src (2, 180, 3) float32, mcd/gt_transform, mcd/transform (2, 4, 4) float32,
  mcd/mean, mcd/sum (float32 scalars), mcd/none (2,) float32                                   modified_chamfer_distance per reduction
Re-run with:  python tests/golden/generate_scan_prep_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_shims  # noqa: E402

OUT = os.path.join(HERE, 'scan_prep.npz')


def main():
    import torch
    ref_shims.install()
    from geotransformer.modules.registration.metrics import modified_chamfer_distance
    from geotransformer.utils.pointcloud import regularize_normals
    from se3et_amd.synthetic import box_surface, euler_zyx
    g = np.random.default_rng(20)
    store = {}
    points = g.uniform(-1, 1, (64, 3))
    normals = g.standard_normal((64, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    points[0], normals[0] = (1.0, 2.0, 0.0), (0.0, 0.0, 1.0)                    # dot == 0: flipped for positive=True
    points[1], normals[1] = (0.5, 0.25, -0.125), (0.0, 0.0, 1.0)                # dot = 0.125 > 0
    store['reg/points'], store['reg/normals'] = points, normals
    store['reg/positive'] = regularize_normals(points, normals, positive=True)
    store['reg/negative'] = regularize_normals(points, normals, positive=False)
    assert -(points[0] * normals[0]).sum() == 0 and (store['reg/positive'][0] == -normals[0]).all()

    dims = (1.2, 1.0, 0.8)
    raw = np.stack([box_surface(300, dims, 31 + b, 0.005) for b in range(2)])
    gt = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    est = gt.copy()
    for b in range(2):
        gt[b, :3, :3], gt[b, :3, 3] = euler_zyx([0.4 + 0.1 * b, -0.2, 0.3]), (0.1, -0.05 * (b + 1), 0.2)
        est[b, :3, :3], est[b, :3, 3] = euler_zyx([0.41 + 0.1 * b, -0.19, 0.29]), (0.11, -0.05 * (b + 1), 0.19)
    ref = np.stack([box_surface(200, dims, 41 + b, 0.005) for b in range(2)])
    inv = np.linalg.inv(gt.astype(np.float64))
    src = np.stack([(box_surface(180, dims, 51 + b, 0.005).astype(np.float64) @ inv[b, :3, :3].T + inv[b, :3, 3]).astype(np.float32)
                    for b in range(2)])
    store.update({'mcd/raw': raw, 'mcd/ref': ref, 'mcd/src': src, 'mcd/gt_transform': gt, 'mcd/transform': est})
    t = [torch.from_numpy(a) for a in (raw, ref, src, gt, est)]
    for reduction in ('mean', 'sum', 'none'):
        store['mcd/' + reduction] = modified_chamfer_distance(*t, reduction=reduction).numpy()
    np.savez_compressed(OUT, **store)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)), {k: store[k] for k in ('mcd/mean', 'mcd/sum', 'mcd/none')})


if __name__ == '__main__':
    main()
