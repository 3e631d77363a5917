"""Cost of triangle mesh extraction on the device (extract_triangle_meshes of se3et_amd.tsdf and se3et_amd.tsdf_sparse) next to the point
extraction of the same state (profiles/mesh_probe.txt).

Workload: the two scenes of tools/tsdf_sparse_probe.py after --frames frames: 640 x 480 uint16 depth frames of the rendered sphere of
tests/tsdf_fixture.py with a wall behind it, voxels of 5 mm, a truncation of 4 voxel lengths; a uniform volume of 512^3 voxels and a sparse
volume at allocation stride 4.  Each state is integrated once; then extract_point_clouds and extract_triangle_meshes are timed in
alternating windows: the median (min .. max) over --windows windows of at least --window-seconds each after a warm-up, host wall time of
calls that end in a device synchronise.  The mesh's workspace bytes are stated with it.  Recorded, not gated.
Run `python tools/mesh_probe.py [--out FILE]` on the GPU box."""
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_probe.txt'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('mesh_probe: no device (the probe measures the device; there is no fallback)')
    import tsdf_fixture as F
    from se3et_amd.mesh import mesh_edge_census
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
    lines = ['mesh_probe: %s; median (min .. max) over %d windows of >= %.1f s, ms per call, host wall ending in a synchronise, the two '
             'extractions in alternating windows.  Recorded, not gated.  %d frames of %d x %d uint16, voxels of %g m, truncation 4 voxel lengths; '
             'uniform: %d^3 voxels; sparse: stride 4.' % (torch.cuda.get_device_name(0), args.windows, args.window_seconds, NF, W, H, vl, R)]

    def synced(fn):
        def call():
            call.out = fn()
            torch.cuda.synchronize()
        call()
        return call

    make = {'sparse': lambda: SparseTSDFVolumes(1, vl, trunc, device='cuda'), 'uniform': lambda: TSDFVolumes(1, R, vl, trunc, origins=origin, device='cuda')}
    for kind in ('uniform', 'sparse'):
        vol = make[kind]().integrate(d, K, poses)
        cloud, mesh = synced(vol.extract_point_clouds), synced(vol.extract_triangle_meshes)
        times = {'cloud': [], 'mesh': []}
        for _ in range(args.windows):                                   # alternating: both see the same neighbours on the machine
            times['cloud'] += windows(cloud, 1, args.window_seconds)
            times['mesh'] += windows(mesh, 1, args.window_seconds)
        vertices, triangles = mesh.out[0][0], mesh.out[1][0]
        _, forward, backward = mesh_edge_census(triangles)
        workspace = 0 if kind == 'uniform' else 4 * vol.tsdf.shape[0] * 4096
        offsets = 16 * (R * R + 1 if kind == 'uniform' else 16 * vol.num_blocks + 1)
        lines.append('  %-8s extract_point_clouds     %9.3f (%.3f .. %.3f)   %d points' % ((kind,) + spread(times['cloud']) + (len(cloud.out[0][0]),)))
        lines.append('  %-8s extract_triangle_meshes  %9.3f (%.3f .. %.3f)   %d vertices, %d triangles, %d boundary edges, %d edges used more than twice; '
                     'workspace %.1f MB (the first-vertex plane) + %.1f MB of offsets'
                     % ((kind,) + spread(times['mesh']) + (len(vertices), len(triangles), int((backward == 0).sum()), int((forward + backward > 2).sum()),
                                                          workspace / 1e6, offsets / 1e6)))
        del vol, cloud, mesh
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
