"""Cost of the mesh queries on the device (se3et_amd/mesh_query.py, csrc/mesh_query.hip; profiles/mesh_query_probe.txt).

Workload: one sphere of radius 0.4 R written straight into a uniform volume of --resolution^3 voxels and meshed by
extract_triangle_meshes (the largest volume that tools/mesh_probe.py uses).  Timed as the median (min .. max) over --windows windows of
at least --window-seconds each after a warm run, host wall time of calls that end in a device synchronise: the build of the tree (two
passes, the sort between them and the read of the counts), a rendering of one 640 x 480 view from outside the sphere (every map), and the
closest points of --queries points spread through the volume's cube.  Recorded, not gated: nothing here is compared with itself.

The bytes of a rendering are stated only as far as they can be argued: every pixel writes its maps once (compulsory), and reads at least
the root; what a walk reads beyond that depends on the view and on the mesh, so no roofline is claimed.
Run `python tools/mesh_query_probe.py [--out FILE]` on the GPU box."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def sphere_mesh(R, vl):
    import torch
    from se3et_amd.tsdf import TSDFVolumes
    i = torch.arange(R, device='cuda', dtype=torch.float32) + 0.5 - R / 2.0 + 0.3
    r = torch.sqrt(i[:, None, None] ** 2 + i[None, :, None] ** 2 + i[None, None, :] ** 2)
    vol = TSDFVolumes(1, R, vl, 3 * vl, device='cuda')
    vol.tsdf[0].copy_(torch.clamp((r - 0.4 * R) / 3.0, -1.0, 1.0))
    vol.weight.fill_(1.0)
    del r
    vertices, triangles, _, _ = vol.extract_triangle_meshes()
    return vertices, triangles


def outside_view(R, vl, H, W):
    """one camera outside the sphere, looking at its centre: the sphere fills most of the image"""
    import tsdf_fixture as U
    from se3et_amd import mesh_query
    centre = np.full(3, R * vl / 2.0)
    E = U.look_at(centre + R * vl * np.array([0.35, -0.25, -1.0]), centre)
    return mesh_query.camera_views([0.9 * W, 0.9 * W, W / 2.0 - 0.5, H / 2.0 - 0.5], E[None])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-seconds', type=float, default=0.3)
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--queries', type=int, default=1 << 18)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_query_probe.txt'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('mesh_query_probe: no device (the probe measures the device; there is no fallback)')
    from se3et_amd import mesh_query, ops
    from tsdf_probe import spread, windows
    R, vl, H, W = args.resolution, 0.005, 480, 640
    vertices, triangles = sphere_mesh(R, vl)
    m = int(triangles[0].shape[0])
    lines = ['mesh_query_probe: %s; median (min .. max) over %d windows of >= %.1f s, ms, host wall ending in a synchronise.  Recorded, not gated.  '
             'The marching-cubes sphere of a uniform volume of %d^3 voxels: %d vertices, %d triangles.'
             % (torch.cuda.get_device_name(0), args.windows, args.window_seconds, R, int(vertices[0].shape[0]), m)]

    def synced(fn):
        def call():
            call.out = fn()
            torch.cuda.synchronize()
        call()
        return call

    build = synced(lambda: mesh_query.build_bvh_meshes(vertices, triangles))
    med, lo, hi = spread(windows(build, args.windows, args.window_seconds))
    lines.append('build_bvh_meshes: %.2f (%.2f .. %.2f) ms, %.1f M triangles/s; live %d, zero-area %d'
                 % (med, lo, hi, m / med / 1e3, build.out.live[0], build.out.zero_area[0]))
    trees = build.out
    views = outside_view(R, vl, H, W)
    maps = tuple(ops.MESH_RENDER_MAPS)
    render = synced(lambda: mesh_query.render_meshes(trees, views, [0], H, W, 0.05, 3.0 * R * vl, maps=maps))
    med, lo, hi = spread(windows(render, args.windows, args.window_seconds))
    hit = float(render.out['mask'].float().mean())
    written = H * W * (4 + 24 + 24 + 8 + 1)
    lines.append('render_meshes 640 x 480, every map: %.3f (%.3f .. %.3f) ms, %.1f M rays/s, %.0f %% of the pixels hit; compulsory bytes: %.2f MB '
                 'written (61 a pixel) and the 128-byte view, %.1f GB/s at this rate; the nodes and triangles a walk reads depend on the view'
                 % (med, lo, hi, H * W / med / 1e3, 100 * hit, written / 1e6, written / med / 1e6))
    depth_only = synced(lambda: mesh_query.render_meshes(trees, views, [0], H, W, 0.05, 3.0 * R * vl, maps=('depth',)))
    med, lo, hi = spread(windows(depth_only, args.windows, args.window_seconds))
    lines.append('render_meshes 640 x 480, depth alone: %.3f (%.3f .. %.3f) ms, %.1f M rays/s' % (med, lo, hi, H * W / med / 1e3))
    gen = torch.Generator(device='cuda').manual_seed(5)
    points = [torch.rand((args.queries, 3), generator=gen, device='cuda', dtype=torch.float64) * (R * vl)]
    closest = synced(lambda: mesh_query.closest_points_meshes(trees, points))
    med, lo, hi = spread(windows(closest, args.windows, args.window_seconds))
    lines.append('closest_points_meshes, %d points in the cube: %.2f (%.2f .. %.2f) ms, %.1f M queries/s; mean distance %.4f'
                 % (args.queries, med, lo, hi, args.queries / med / 1e3, float(closest.out['distances'][0].mean())))
    near = [vertices[0][torch.randint(0, vertices[0].shape[0], (args.queries,), generator=gen, device='cuda')]
            + 0.5 * vl * torch.randn((args.queries, 3), generator=gen, device='cuda', dtype=torch.float64)]
    close = synced(lambda: mesh_query.distance_to_meshes(trees, near))
    med, lo, hi = spread(windows(close, args.windows, args.window_seconds))
    lines.append('distance_to_meshes, %d points within a voxel of the surface (a scan against its reconstruction): %.2f (%.2f .. %.2f) ms, %.1f M queries/s'
                 % (args.queries, med, lo, hi, args.queries / med / 1e3))
    lines.append('end to end (tests/mesh_query_fixture.END_TO_END_HOST_ERROR, CPU, the two host entries): the ray-cast volume and its rendered '
                 'mesh differ by 1.0252 voxel lengths at most over 932 pixels of mesh_fixture\'s sphere; tests/test_gpu_mesh_query.py asserts 2.0 times that.')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
