"""Cost of TSDF fusion on the device (se3et_amd.tsdf) next to the numpy twin (tests/tsdf_twin.py) on the same box
(profiles/tsdf_probe.txt).

Workload: volumes of 256^3 voxels of 1 / 256 m around the rendered sphere of tests/tsdf_fixture.py, 640 x 480 uint16 depth frames from
poses on an arc with a wall 2 m from the camera behind it, a truncation of 4 voxel lengths; 1 and 16 volumes, 50 frames and 1 frame a
volume, without and (1 volume) with uint8 colour.  Per workload: device-event time of ops.tsdf_integrate_stack alone and host wall time of TSDFVolumes.integrate (frame table,
finite check, launch, synchronisation) as the median (min .. max) over --windows windows of at least --window-seconds each after a
warm-up; the volume traffic of a call (tsdf and weight read for every voxel, written for the touched ones) over the event time, against
the 8 TB/s peak; the time of extract_point_clouds.  The one-pass design holds if 50 frames cost far less than 50 times one frame.  The
twin runs once on one volume with --twin-frames frames (it sweeps the volume once per frame, so its cost is linear in them).
Recorded, not gated.  Run `python tools/tsdf_probe.py [--out FILE]` on the GPU box."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

PEAK = 8.0e12


def spread(values):
    return statistics.median(values), min(values), max(values)


def windows(fn, count, seconds):
    out = []
    for _ in range(count):
        calls, own, t0 = 0, 0.0, time.perf_counter()
        while time.perf_counter() - t0 < seconds or calls < 3:
            own += fn() or 0.0
            calls += 1
        out.append(own / calls if own else (time.perf_counter() - t0) * 1e3 / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--window-seconds', type=float, default=0.5)
    ap.add_argument('--resolution', type=int, default=256)
    ap.add_argument('--frames', type=int, default=50)
    ap.add_argument('--twin-frames', type=int, default=2, help='0: no twin')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tsdf_probe.txt'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tsdf_probe: no device (the probe measures the device; there is no fallback)')
    import tsdf_fixture as F
    import tsdf_twin as twin
    from se3et_amd import ops
    from se3et_amd.tsdf import TSDFVolumes
    R, H, W, NF = args.resolution, 480, 640, args.frames
    vl = F.SPHERE_SIDE / R
    K = np.array([0.9 * W, 0.95 * W, W / 2.0 - 0.3, H / 2.0 + 0.2])
    poses = np.array(F._orbit(NF))
    rendered = [F.render_sphere(E, K, H, W) for E in poses]
    depth = np.stack([np.round(np.where(lam > 0, lam, 2.0) * 1000.0).astype(np.uint16) for lam, _ in rendered])          # a wall at 2 m behind the sphere:
    color = np.round(np.stack([c for _, c in rendered]) * 255).astype(np.uint8)                                            # free space is carved, as in a room
    del rendered
    lines = ['tsdf_probe: %s; median (min .. max) over %d windows of >= %.1f s, ms per call.  Recorded, not gated.  Volumes of %d^3 voxels, '
             '%d x %d uint16 frames, truncation 4 voxel lengths; the twin row is tests/tsdf_twin.py on the same box (%d CPUs allowed), once.'
             % (torch.cuda.get_device_name(0), args.windows, args.window_seconds, R, W, H, min(16, len(os.sched_getaffinity(0))))]
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    d1, c1 = torch.from_numpy(depth).cuda(), torch.from_numpy(color).cuda()
    events = {}
    for V, nf, with_color in ((1, NF, False), (1, 1, False), (16, NF, False), (16, 1, False), (1, NF, True)):
        d = d1[:nf].view(torch.int16).repeat(V, 1, 1).view(torch.uint16) if V > 1 else d1[:nf]          # (uint16 through its bits)
        c = c1[:nf] if with_color else None
        E = np.tile(poses[:nf], (V, 1, 1))
        vol = TSDFVolumes(V, R, vl, 4 * vl, color=with_color, device='cuda')
        counts = [nf] * V
        table = torch.from_numpy(twin.frame_table(E, K)).cuda()

        def raw():
            start.record()
            ops.tsdf_integrate_stack(vol.tsdf, vol.weight, vol.color, vl, 4 * vl, vol.origins, d, table, counts, c)
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop)

        def whole():
            vol.integrate(d, K, E, counts, c)
            torch.cuda.synchronize()

        raw(), whole()
        ev, wall = spread(windows(raw, args.windows, args.window_seconds)), spread(windows(whole, args.windows, args.window_seconds))
        touched = int((vol.weight > 0).sum())
        planes = 5 if with_color else 2
        nbytes = 4 * planes * (V * R ** 3 + touched)
        events[(V, nf, with_color)] = ev[0]
        lines.append('%d volume(s) x %d frame(s)%s: %d of %d voxels touched, %.1f MB of volume traffic a call'
                     % (V, nf, ', uint8 colour' if with_color else '', touched, V * R ** 3, nbytes / 1e6))
        lines.append('  ops.tsdf_integrate_stack, device events      %9.3f (%.3f .. %.3f)   %.2f TB/s of volume traffic, %.1f %% of 8 TB/s; '
                     '%.2f ps per voxel and frame' % (ev + (nbytes / ev[0] / 1e9, 100.0 * nbytes / (ev[0] * 1e-3) / PEAK,
                                                            ev[0] * 1e9 / (V * R ** 3 * nf))))
        lines.append('  TSDFVolumes.integrate, host wall             %9.3f (%.3f .. %.3f)' % wall)
        if nf == NF:
            def extract():
                out = vol.extract_point_clouds()
                torch.cuda.synchronize()
                extract.n = sum(len(p) for p in out[0])
            extract()
            ex = spread(windows(extract, args.windows, args.window_seconds))
            lines.append('  extract_point_clouds, host wall              %9.3f (%.3f .. %.3f)   %d points' % (ex + (extract.n,)))
        del vol
    for V in (1, 16):
        lines.append('%d volume(s): %d frames cost %.2f times one frame (%d separate sweeps would cost %d times)'
                     % (V, NF, events[(V, NF, False)] / events[(V, 1, False)], NF, NF))
    if args.twin_frames:
        n = args.twin_frames
        state = twin.new_state(R, False)
        t0 = time.perf_counter()
        twin.integrate(state, vl, 4 * vl, np.zeros(3), depth[:n], twin.frame_table(poses[:n], K))
        ms = (time.perf_counter() - t0) * 1e3
        vol = TSDFVolumes(1, R, vl, 4 * vl, device='cuda').integrate(d1[:n], K, poses[:n])
        same = F.same(vol.tsdf[0].cpu().numpy(), state['tsdf']) and F.same(vol.weight[0].cpu().numpy(), state['weight'])
        lines.append('twin (numpy), one volume, %d frames, host wall   %9.1f   %.1f ms a frame, %.0f ms for %d frames by that rate: %.0fx the '
                     'device call (%.3f); states equal: %s' % (n, ms, ms / n, ms / n * NF, NF, ms / n * NF / events[(1, NF, False)],
                                                              events[(1, NF, False)], same))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
