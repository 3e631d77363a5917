"""Cost of ray casting the TSDF volumes on the device (ray_cast of se3et_amd.tsdf and se3et_amd.tsdf_sparse) next to the point extraction of
the same state, and of a step of the frame-to-model tracker (profiles/raycast_probe.txt).

Workload: the two scenes of tools/mesh_probe.py after --frames frames: 640 x 480 uint16 depth frames of the rendered sphere of
tests/tsdf_fixture.py with a wall behind it, voxels of 5 mm, a truncation of 4 voxel lengths; a uniform volume of 512^3 voxels and a sparse
volume at allocation stride 4.  Each state is integrated once; then ray_cast (--views views of 640 x 480 per call, from the first poses of
the orbit; the maps are depth alone, then depth, points, normals and mask) and extract_point_clouds are timed in alternating
windows: the median (min .. max) over --windows windows of at least --window-seconds each after a warm-up, host wall time of calls that
end in a device synchronise.  The tracker runs --track-frames frames of the textured scene of tests/rgbd_odometry_fixture.py at 640 x 480 into a
sparse volume with colour; its time is the whole call over the frames.  Recorded, not gated.
Run `python tools/raycast_probe.py [--out FILE]` on the GPU box."""
import argparse
import os
import sys
import time

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
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--track-frames', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'raycast_probe.txt'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('raycast_probe: no device (the probe measures the device; there is no fallback)')
    import raycast_fixture as RF
    import tsdf_fixture as F
    from se3et_amd.tracking import track_and_integrate_rgbd
    from se3et_amd.tsdf import TSDFVolumes
    from se3et_amd.tsdf_sparse import SparseTSDFVolumes
    from tsdf_probe import spread, windows
    R, H, W, NF, NV, vl = args.resolution, 480, 640, args.frames, args.views, 0.005
    trunc = 4 * vl
    K = np.array([0.9 * W, 0.95 * W, W / 2.0 - 0.3, H / 2.0 + 0.2])
    poses = np.array(F._orbit(NF))
    rendered = [F.render_sphere(E, K, H, W) for E in poses]
    depth = np.stack([np.round(np.where(lam > 0, lam, 2.0) * 1000.0).astype(np.uint16) for lam, _ in rendered])
    origin = (F.SPHERE_CENTER - R * vl / 2.0)[None]
    d = torch.from_numpy(depth).cuda()
    lines = ['raycast_probe: %s; median (min .. max) over %d windows of >= %.1f s, ms, host wall ending in a synchronise, ray casting and the point '
             'extraction in alternating windows.  Recorded, not gated.  %d frames of %d x %d uint16, voxels of %g m, truncation 4 voxel lengths; '
             'uniform: %d^3 voxels; sparse: stride 4; %d views of %d x %d per ray_cast call, depth_min 0.1, depth_max 3.'
             % (torch.cuda.get_device_name(0), args.windows, args.window_seconds, NF, W, H, vl, R, NV, W, H)]

    def synced(fn):
        def call():
            call.out = fn()
            torch.cuda.synchronize()
        call()
        return call

    views = torch.from_numpy(poses[:NV]).cuda()
    make = {'sparse': lambda: SparseTSDFVolumes(1, vl, trunc, device='cuda'), 'uniform': lambda: TSDFVolumes(1, R, vl, trunc, origins=origin, device='cuda')}
    for kind in ('uniform', 'sparse'):
        vol = make[kind]().integrate(d, K, poses)
        cloud = synced(vol.extract_point_clouds)
        casts = {'depth': synced(lambda: vol.ray_cast(K, views, H, W, maps=('depth',))),
                 'depth, points, normals, mask': synced(lambda: vol.ray_cast(K, views, H, W, maps=('depth', 'points', 'normals', 'mask')))}
        times = {name: [] for name in list(casts) + ['cloud']}
        for _ in range(args.windows):                                   # alternating: all see the same neighbours on the machine
            times['cloud'] += windows(cloud, 1, args.window_seconds)
            for name, call in casts.items():
                times[name] += windows(call, 1, args.window_seconds)
        full = casts['depth, points, normals, mask'].out
        hit = full['mask']
        ball = torch.from_numpy(rendered[0][0] > 0).cuda() & hit[0]     # (the wall is at 2 m of every camera: only the sphere is one surface)
        off = (full['depth'][0] - torch.from_numpy(rendered[0][0]).cuda().float()).abs()[ball]
        lines.append('  %-8s extract_point_clouds                       %9.3f (%.3f .. %.3f) a call   %d points' % ((kind,) + spread(times['cloud']) + (len(cloud.out[0][0]),)))
        for name in casts:
            lines.append('  %-8s ray_cast %-32s %9.3f (%.3f .. %.3f) a view' % ((kind, '(' + name + ')') + tuple(x / NV for x in spread(times[name]))))
        lines.append('           %.4f of the pixels hit; view 0 against its input frame on the sphere: median |depth difference| %.2f mm, 90th percentile %.2f mm (the rest lies on the silhouette)'
                     % (float(hit.float().mean()), 1e3 * float(off.median()), 1e3 * float(off.quantile(0.9))))
        del vol, cloud, casts, full, hit
        torch.cuda.empty_cache()
    # the tracker: the textured sphere and plane of tests/rgbd_odometry_fixture.py along its orbit (about 1 degree and 3 cm a frame), uint8 colours
    import rgbd_odometry_fixture as O
    NT = args.track_frames
    orbit = O.orbit_poses(NT)
    td, tc = O.frames(orbit, H, W)
    td, tc, TK = torch.from_numpy(td).cuda(), torch.from_numpy(tc).cuda(), O.intrinsics(H, W)

    def track():
        t0 = time.perf_counter()
        out = track_and_integrate_rgbd([td], [tc], TK, vl, trunc)
        torch.cuda.synchronize()
        track.out = out
        return (time.perf_counter() - t0) * 1e3 / NT
    track()
    per_frame = windows(track, args.windows, args.window_seconds)
    poses_found, success, _ = track.out
    errors = RF.pose_error(list(poses_found[0].cpu().numpy()), [np.linalg.inv(E) for E in orbit])
    lines.append('  tracker  track_and_integrate_rgbd, %d frames, sparse   %9.3f (%.3f .. %.3f) a frame (ray cast, odometry of 20 + 10 + 5 iterations, '
                 'integration, one flag read) of the scene of tests/rgbd_odometry_fixture.py at %d x %d; %d of %d frames tracked, worst pose error %.3f '
                 'degrees, %.2f mm' % ((NT,) + spread(per_frame) + (W, H, int(success[0].sum()), NT) + errors))
    lines.append('Analytic anchor (tests/raycast_fixture.py, measured on the CPU): the twin\'s worst hit-depth error on the analytic sphere is %.4f '
                 'voxel lengths (a grazing ray; median 0.083).  Round trip at 32 x 24: %.6f m, %.0f %% of the valid pixels hit.'
                 % (RF.SPHERE_TWIN_ERROR, RF.ROUND_TRIP_TWIN_ERROR, 100 * RF.ROUND_TRIP_TWIN_SHARE))
    lines.append('Tracker on the 6-frame orbit at 32 x 24 through the host entries: %.4f degrees / %.3f mm at worst.  Chained frame-to-frame odometry '
                 'on the same orbit at 160 x 120: 0.3351 degrees / 5.797 mm.  The two are not comparable and neither is claimed better.' % RF.TRACKING_HOST_ERROR)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
