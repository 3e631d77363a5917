"""Cost of block-sparse TSDF volumes on the device (se3et_amd.tsdf_sparse) next to the uniform volume (se3et_amd.tsdf) on the same frames
(profiles/tsdf_sparse_probe.txt).

Workload: 640 x 480 uint16 depth frames of the rendered sphere of tests/tsdf_fixture.py from poses on an arc, with a wall 2 m from the
camera behind it, voxels of 5 mm and a truncation of 4 voxel lengths.  The uniform volume is 512^3 voxels (2.56 m) around the sphere; the
sparse volume takes the same frames at allocation stride 4 and has no bounds.  For 1 frame and for --frames frames, each as the median
(min .. max) over --windows windows of at least --window-seconds each after a warm-up, host wall time of calls that end in a device
synchronise: integrate into a new object (allocation included), integrate again into the same object (no new blocks), and
extract_point_clouds; then the bytes of state that each holds.  Recorded, not gated.
Run `python tools/tsdf_sparse_probe.py [--out FILE]` on the GPU box."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--window-seconds', type=float, default=0.5)
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--frames', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tsdf_sparse_probe.txt'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tsdf_sparse_probe: no device (the probe measures the device; there is no fallback)')
    import tsdf_fixture as F
    from se3et_amd.tsdf import TSDFVolumes
    from se3et_amd.tsdf_sparse import SparseTSDFVolumes
    from tsdf_probe import spread, windows
    R, H, W, NF, vl = args.resolution, 480, 640, args.frames, 0.005
    trunc = 4 * vl
    K = np.array([0.9 * W, 0.95 * W, W / 2.0 - 0.3, H / 2.0 + 0.2])
    poses = np.array(F._orbit(NF))
    depth = np.stack([np.round(np.where(lam > 0, lam, 2.0) * 1000.0).astype(np.uint16) for lam, _ in (F.render_sphere(E, K, H, W) for E in poses)])
    origin = (F.SPHERE_CENTER - R * vl / 2.0)[None]
    d = torch.from_numpy(depth).cuda()
    lines = ['tsdf_sparse_probe: %s; median (min .. max) over %d windows of >= %.1f s, ms per call, host wall ending in a synchronise.  Recorded, '
             'not gated.  %d x %d uint16 frames, voxels of %g m, truncation 4 voxel lengths; uniform: %d^3 voxels; sparse: stride 4.'
             % (torch.cuda.get_device_name(0), args.windows, args.window_seconds, W, H, vl, R)]

    def timed(fn):
        def call():
            call.out = fn()
            torch.cuda.synchronize()
        call()
        return spread(windows(call, args.windows, args.window_seconds)), call.out

    for nf in (1, NF):
        E = poses[:nf]
        make = {'sparse': lambda: SparseTSDFVolumes(1, vl, trunc, device='cuda'), 'uniform': lambda: TSDFVolumes(1, R, vl, trunc, origins=origin, device='cuda')}
        lines.append('%d frame(s)' % nf)
        for kind in ('sparse', 'uniform'):
            fresh, vol = timed(lambda: make[kind]().integrate(d[:nf], K, E))
            again, _ = timed(lambda: vol.integrate(d[:nf], K, E))
            one = make[kind]().integrate(d[:nf], K, E)                  # integrated once: what a user extracts
            ex, clouds = timed(one.extract_point_clouds)
            if kind == 'sparse':
                held, used = 8 * one.tsdf.shape[0] * 4096 + 12 * one.keys.shape[0], 8 * one.num_blocks * 4096
                note = '%d blocks, %.1f MB of state in use, %.1f MB held (storage grows geometrically)' % (one.num_blocks, used / 1e6, held / 1e6)
            else:
                note = '%.1f MB of state' % (8 * R ** 3 / 1e6)
            lines.append('  %-8s integrate, new object   %9.3f (%.3f .. %.3f)' % ((kind,) + fresh))
            lines.append('  %-8s integrate, same object  %9.3f (%.3f .. %.3f)' % ((kind,) + again))
            lines.append('  %-8s extract_point_clouds    %9.3f (%.3f .. %.3f)   %d points; %s' % ((kind,) + ex + (len(clouds[0][0]), note)))
            del vol, one, clouds
            torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
