"""Cost of the mesh post-processing entries on the device (se3et_amd/mesh.py, csrc/mesh_ops.hip; profiles/mesh_ops_probe.txt).

Workload: two states written straight into a uniform volume of --resolution^3 voxels and meshed by extract_triangle_meshes: `sphere`, one
sphere of radius 0.4 R, and `shells`, concentric spheres every 8 voxels (millions of triangles: the positions no longer fit the L2s).  Each
entry is timed as the median (min .. max) over --windows windows of at least --window-seconds each after a warm run, host wall time of calls
that end in a device synchronise; the smoothing step is timed between device events around one call of --steps Laplacian steps and reported
per step.  For the step the bytes are computed from the
shapes: the compulsory ones (every position read once and written once, the row offsets and the neighbour numbers read once) and those with
every gathered neighbour row counted, each over the time and as a fraction of the 8 TB/s peak.  Recorded, not gated: nothing here is compared
with itself.  For context the numpy twin's step on the `sphere` mesh is timed on the host and labelled as a CPU figure.
Run `python tools/mesh_ops_probe.py [--out FILE]` on the GPU box."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--window-seconds', type=float, default=0.3)
    ap.add_argument('--resolution', type=int, default=256)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--twin', type=int, default=1, help='0: no CPU figure')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_ops_probe.txt'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('mesh_ops_probe: no device (the probe measures the device; there is no fallback)')
    from se3et_amd import mesh, ops
    from se3et_amd.tsdf import TSDFVolumes
    from tsdf_probe import spread, windows
    R, vl = args.resolution, 0.005
    lines = ['mesh_ops_probe: %s; median (min .. max) over %d windows of >= %.1f s, ms, host wall ending in a synchronise unless it says events.  '
             'Recorded, not gated.  Meshes of a uniform volume of %d^3 voxels.' % (torch.cuda.get_device_name(0), args.windows, args.window_seconds, R)]

    def state(kind):
        i = torch.arange(R, device='cuda', dtype=torch.float32) + 0.5 - R / 2.0 + 0.3
        r = torch.sqrt(i[:, None, None] ** 2 + i[None, :, None] ** 2 + i[None, None, :] ** 2)
        d = r - 0.4 * R if kind == 'sphere' else (4.0 - torch.remainder(r, 8.0)).abs() - 2.0
        if kind == 'shells':
            d = torch.where(r < 0.47 * R, d, torch.ones_like(d))
        return torch.clamp(d / 3.0, -1.0, 1.0)

    def synced(fn):
        def call():
            call.out = fn()
            torch.cuda.synchronize()
        call()
        return call

    for kind in ('sphere', 'shells'):
        vol = TSDFVolumes(1, R, vl, 3 * vl, origins=np.zeros((1, 3)), color=False, device='cuda')
        vol.tsdf.copy_(state(kind)[None]), vol.weight.fill_(1.0)
        v, t, n, _ = vol.extract_triangle_meshes()
        del vol
        torch.cuda.empty_cache()
        N, M = len(v[0]), len(t[0])
        S = ops.StackedMeshes(v[0], t[0], [N], [M])
        inc = ops.mesh_incidence_stack(S)
        keep = [torch.rand(M, device='cuda') < 0.5]
        lines.append('  %s: %d vertices, %d triangles, %d neighbour entries (valence %.2f), %d incidences' % (kind, N, M, inc.neighbors, inc.neighbors / max(N, 1),
                                                                                                              inc.incidences))
        keys = t[0].reshape(-1) * M + torch.arange(M, device='cuda').repeat_interleave(3)
        calls = {
            'incidence (integer atomics, then a sort per row)': synced(lambda: ops.mesh_incidence_stack(S)),
            'incidence A/B: torch.sort of the 3 M (vertex, triangle) keys alone': synced(lambda: torch.sort(keys)),
            'cluster_connected_triangles_meshes (incidence, union, sort, areas)': synced(lambda: mesh.cluster_connected_triangles_meshes(v, t)),
            'components alone (tables given)': synced(lambda: ops.mesh_components_stack(S, inc)),
            'select_triangles_meshes (a random half, with normals)': synced(lambda: mesh.select_triangles_meshes(v, t, keep, n)),
            'triangle_normals_meshes': synced(lambda: mesh.triangle_normals_meshes(v, t)),
            'vertex normals alone (tables given)': synced(lambda: ops.mesh_normals_stack(S, inc, True, False, True)),
            'filter_smooth_meshes (5 taubin iterations, incidence included)': synced(lambda: mesh.filter_smooth_meshes(v, t, 5)),
            'simplify_vertex_clustering_meshes (cells of 4 voxel lengths, with normals)': synced(lambda: mesh.simplify_vertex_clustering_meshes(v, t, 4 * vl, n)),
        }
        times = {name: [] for name in calls}
        for _ in range(args.windows):
            for name, call in calls.items():
                times[name] += windows(call, 1, args.window_seconds)
        for name in calls:
            lines.append('    %-72s %9.3f (%.3f .. %.3f)' % ((name,) + spread(times[name])))
        k = calls['components alone (tables given)'].out[3]
        lines.append('    clusters: %d' % k[0])

        def step_time():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.mesh_smooth_stack(S, inc, 'laplacian', args.steps)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / args.steps
        step_time()
        steps = windows(step_time, args.windows, args.window_seconds)
        must = 24 * N + 24 * N + 8 * N + 4 * inc.neighbors
        gathered = must + 24 * inc.neighbors
        med = spread(steps)
        lines.append('    smoothing step, one lane per vertex, events over %d steps of one call        %9.4f (%.4f .. %.4f) a step: %.1f MB compulsory = %.2f TB/s '
                     '= %.3f of the 8 TB/s peak; %.1f MB with every gathered row = %.2f TB/s = %.3f of peak'
                     % ((args.steps,) + med + (must / 1e6, must / med[0] / 1e9, must / med[0] / 1e9 / (PEAK / 1e12),
                                               gathered / 1e6, gathered / med[0] / 1e9, gathered / med[0] / 1e9 / (PEAK / 1e12))))
        if kind == 'sphere' and args.twin:
            import mesh_ops_twin as twin
            hv, ht = v[0].cpu().numpy(), t[0].cpu().numpy()
            rows = twin.incidence(ht, N)[1]
            t0 = time.perf_counter()
            twin.smooth_step(hv, rows, False, 0.5)
            lines.append('    CPU figure, for context only: one step of the numpy twin on this mesh on the host (rows given)   %9.1f ms' % ((time.perf_counter() - t0) * 1e3))
        del S, inc, calls, keys
        torch.cuda.empty_cache()
    lines.append('The incidence tables are built with integer atomics and a sort per row; the key-sort line is the sort alone of the design not taken, '
                 'without the passes that would follow it.')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
