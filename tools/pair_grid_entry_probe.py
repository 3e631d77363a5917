"""Every device entry of the six files on the float64 pair grid -- csrc/pair_geometry.hip, voxel_downsample.hip, knn_normals.hip, icp.hip,
keypoint_nms.hip, fpfh.hip -- called once on a small stacked input, a SHA-256 of every output tensor; then the device time of each entry
at the sizes of the per-tool probes (profiles/pair_grid_layers_parent_vs_pr.txt).

Hashes.  Three stacked clouds of 257, 1 and 4 099 points, fixed seeds, once as float64 and once as float32.  The third is a lattice of
spacing 2^-4, searched in a copy of its first 1 024 points shifted by half a spacing on two axes, so exact distance ties occur.  The pair
searches look the clouds up in their partners under a rigid transform (the lattice keeps the identity); the k-NN, normals, NMS and FPFH run
on the clouds themselves, ICP registers the partners to them.  Rows that
an entry leaves unwritten (the voxel and keypoint outputs past their counts) are not hashed, nor is the grid workspace itself: the order
of the points inside a cell is the arrival order of the build's integer atomics, and no result depends on it.

Times.  16 clouds of 5 000 uniform points in the unit cube, float32 (ball radius 0.124: about 40 neighbours; NMS radius 0.62 n^(-1/3));
ICP on the 16 c2_5k pairs at r = 0.1 and on one pair of 120 000 + 120 000 points at r = 1.0, 10 iterations at most.  Device events around
one call of the se3et_amd.ops wrapper: the median of --reps calls after --warmup calls, repeated --rounds times; per entry the median (min .. max)
of the rounds' medians, us.

The library is the one SE3_LIB names (default: the in-tree build), so two builds are compared by one run each, in two processes:
  SE3_LIB=parent.so python tools/pair_grid_entry_probe.py --out a.txt && python tools/pair_grid_entry_probe.py --out b.txt
  python tools/pair_grid_entry_probe.py --compare a.txt b.txt
--compare needs no device: every hash must be equal, and each median of the second file is reported inside or outside the first's range."""
import argparse
import hashlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rigid(angle, shift):
    c, s = np.cos(angle), np.sin(angle)
    T = np.eye(4)
    T[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    T[:3, 3] = shift
    return T


def hash_inputs(dtype):
    """(clouds, partners, transforms): clouds[p] ~ transforms[p] applied to partners[p]."""
    g = np.random.default_rng(20240607)
    h = 0.0625
    lattice = (np.stack(np.meshgrid(np.arange(17), np.arange(17), np.arange(17), indexing='ij'), -1).reshape(-1, 3)[:4099] * h)
    clouds = [g.uniform(0, 1, (257, 3)), g.uniform(0, 1, (1, 3)), lattice]
    T = [rigid(0.3, [0.1, -0.2, 0.05]), rigid(-0.2, [0.0, 0.3, 0.0]), np.eye(4)]
    queries = [(c - t[:3, 3]) @ t[:3, :3] + g.normal(0, 0.01, c.shape) for c, t in zip(clouds[:2], T[:2])]
    queries.append(lattice[:1024] + np.array([h / 2, h / 2, 0.0]))
    return [c.astype(dtype) for c in clouds], [q.astype(dtype) for q in queries], np.stack(T)          # (2^-4 multiples are exact in float32)


def search_entries(torch, ops, clouds, queries, T, radius, nms_radius, voxel, k, keep):
    """Calls every entry but ICP once: the pair searches look `clouds` up in `queries` moved by T, the others run on the clouds themselves.
    keep(name, tensor) receives each output.  Returns (name, build, call) per entry for the timing: call(build()) repeats it."""
    dev = 'cuda'
    lens, qlens = [len(c) for c in clouds], [len(q) for q in queries]
    P = len(clouds)
    s, q = torch.from_numpy(np.concatenate(clouds)).to(dev), torch.from_numpy(np.concatenate(queries)).to(dev)
    Tt = torch.from_numpy(T)
    eye = torch.eye(4, dtype=torch.float64).repeat(P, 1, 1)
    g = np.random.default_rng(7)
    order = torch.from_numpy(np.concatenate([np.argsort(-g.uniform(0, 1, n), kind='stable') for n in lens])).to(dev)
    entries = [('pair_grid_build', None, lambda G: ops.pair_grid_build(q, qlens, Tt, 0.0))]

    def entry(name, build, call):
        out = call(build() if build else None)
        for label, t in out.items():
            keep('%s/%s' % (name, label), t)
        entries.append((name, build, call))
        return out

    def moved(hint):
        return lambda: ops.pair_grid_build(q, qlens, Tt, hint)

    def own(hint):
        return lambda: ops.pair_grid_build(s, lens, eye, hint)
    nn = entry('pair_nearest_neighbor_stack', moved(0.0), lambda G: dict(zip(('distances', 'indices'), ops.pair_nearest_neighbor_stack(G, s, lens))))
    ro = entry('pair_ball_count_stack', moved(radius), lambda G: {'row_offsets': ops.pair_ball_count_stack(G, s, lens, radius)})['row_offsets']
    total = int(ro[-1])
    entry('pair_ball_fill_stack', moved(radius), lambda G: {'pairs': ops.pair_ball_fill_stack(G, s, lens, radius, ro, total)})
    entry('pair_overlap_stack', None, lambda G: {'overlap': ops.pair_overlap_stack(nn['distances'], lens, radius)})
    sel = torch.cat([torch.arange(0, n, 2, device=dev) for n in qlens])
    entry('pair_info_covariance_stack', None,
          lambda G: {'covariance': ops.pair_info_covariance_stack(q, qlens, Tt, sel, [(n + 1) // 2 for n in qlens])})

    def voxels(G):
        out, _, words = ops.voxel_downsample_stack(s, lens, voxel)
        return {'words': words, 'points': out[:int(words[:P].clamp(min=0).sum())]}
    entry('voxel_downsample_stack', None, voxels)
    entry('knn_stack', own(0.0), lambda G: dict(zip(('idx', 'd2'), ops.knn_stack(G, s, lens, k))))
    normals = entry('knn_normals_stack', own(0.0), lambda G: {'normals': ops.knn_normals_stack(G, s, lens, k)})['normals']

    def nms(G):
        out, words = ops.keypoint_nms_stack(G, order, lens, nms_radius, 0)
        counts, starts = words[:P].tolist(), np.cumsum([0] + lens)
        return {'words': words, 'kept': torch.cat([out[a:a + max(c, 0)] for a, c in zip(starts, counts)])}
    entry('keypoint_nms_stack', own(nms_radius), nms)
    entry('fpfh_check_stack', None, lambda G: {'words': ops.fpfh_check_stack(s, normals, lens)})
    grid = ops.pair_grid_build(s, lens, eye, radius)
    fro = ops.pair_ball_count_stack(grid, s, lens, radius)
    pairs = ops.pair_ball_fill_stack(grid, s, lens, radius, fro, int(fro[-1]))
    spfh, fpfh = torch.zeros((len(s), 33), dtype=torch.float64, device=dev), torch.zeros((len(s), 33), dtype=torch.float64, device=dev)
    entry('spfh_stack', None, lambda G: {'spfh': ops.spfh_stack(s, normals, lens, fro, pairs, spfh)})
    entry('fpfh_stack', None, lambda G: {'fpfh': ops.fpfh_stack(s, spfh, lens, fro, pairs, fpfh)})
    return entries


def icp_entries(torch, ops, refs, srcs, T0, r, iterations, keep):
    """se3_icp_stack in both estimations, ref ~ T0 src; the reference normals are knn_normals_stack's at k = 33."""
    dev = 'cuda'
    lens, qlens = [len(c) for c in refs], [len(c) for c in srcs]
    s, q = torch.from_numpy(np.concatenate(refs)).to(dev), torch.from_numpy(np.concatenate(srcs)).to(dev)
    eye = torch.eye(4, dtype=torch.float64).repeat(len(refs), 1, 1)
    normals = ops.knn_normals_stack(ops.pair_grid_build(s, lens, eye, 0.0), s, lens, 33)
    T0 = torch.from_numpy(T0).to(dev)
    entries = []
    for mode in ('point_to_point', 'point_to_plane'):
        def call(G, mode=mode):
            return ops.icp_stack(G, q, qlens, T0, r, mode, normals, max_iteration=iterations, return_correspondences=True)
        entries.append(('icp_stack %s' % mode, lambda: ops.pair_grid_build(s, lens, eye, r), call))
        for label, t in call(entries[-1][1]()).items():
            keep('%s/%s' % (entries[-1][0], label), t)
    return entries


def measure(torch, args, lines):
    from se3et_amd import ops
    from se3et_amd.synthetic import PAIR_PRESETS, box_surface, euler_zyx, make_pair
    for dtype in ('float64', 'float32'):
        def keep(name, t):
            torch.cuda.synchronize()
            lines.append('hash %-8s %-48s %s' % (dtype, name, hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()))
        clouds, queries, T = hash_inputs(dtype)
        search_entries(torch, ops, clouds, queries, T, 0.1, 0.08, 0.1, 33, keep)
        icp_entries(torch, ops, clouds, queries, T, 0.15, 30, keep)
    if args.rounds <= 0:
        return
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(build, call):
        medians = []
        for _ in range(args.rounds):
            G = build() if build else None
            for _ in range(args.warmup):
                call(G)
            out = []
            for _ in range(args.reps):
                start.record()
                call(G)
                stop.record()
                stop.synchronize()
                out.append(start.elapsed_time(stop) * 1e3)
            medians.append(statistics.median(out))
        return statistics.median(medians), min(medians), max(medians)

    def nothing(name, t):
        pass
    g = np.random.default_rng(5)
    n = 5000
    clouds = [g.uniform(0, 1, (n, 3)).astype(np.float32) for _ in range(16)]
    T = np.stack([rigid(0.05 * i, [0.01 * i, 0.0, 0.02]) for i in range(16)])
    queries = [((c - t[:3, 3]) @ t[:3, :3]).astype(np.float32) for c, t in zip(clouds, T)]
    rows = [('16 x 5k',) + e for e in search_entries(torch, ops, clouds, queries, T, 0.124, 0.62 * n ** (-1.0 / 3.0), 0.025, 33, nothing)]
    small = [make_pair('c2_5k', i) for i in range(16)]
    m, dims, jitter = 120000, PAIR_PRESETS['c3_20k'][1], PAIR_PRESETS['c3_20k'][2]
    Tb = np.eye(4)
    Tb[:3, :3], Tb[:3, 3] = euler_zyx([0.5, 0.3, 0.2]), 0.05 * np.asarray(dims)
    big = [(box_surface(m, dims, 1, jitter).astype(np.float32), ((box_surface(m, dims, 2, jitter) - Tb[:3, 3]) @ Tb[:3, :3]).astype(np.float32), Tb)]
    for label, pairs, r in (('16 x (5k + 5k)', small, 0.1), ('1 x (120k + 120k)', big, 1.0)):
        T0 = np.stack([rigid(0.03, [0.01, 0.01, 0.0]) @ np.asarray(p[2], np.float64) for p in pairs])
        rows += [(label,) + e for e in icp_entries(torch, ops, [p[0] for p in pairs], [p[1] for p in pairs], T0, r, 10, nothing)]
    for label, name, build, call in rows:
        lines.append('time %-18s %-36s %10.1f (%.1f .. %.1f)' % ((label, name) + timed(build, call)))


def compare(a, b):
    def read(path):
        hashes, times = {}, {}
        for line in open(path):
            w = line.split()
            if w[:1] == ['hash']:
                hashes[' '.join(w[1:-1])] = w[-1]
            elif w[:1] == ['time']:
                head, tail = line[5:].rsplit('(', 1)
                lo, hi = tail.rstrip(')\n').split(' .. ')
                times[' '.join(head.split()[:-1])] = (float(head.split()[-1]), float(lo), float(hi))
        return hashes, times
    (ha, ta), (hb, tb) = read(a), read(b)
    differ = sorted(k for k in set(ha) | set(hb) if ha.get(k) != hb.get(k))
    print('hashes: %d in %s, %d in %s, %d differ%s' % (len(ha), a, len(hb), b, len(differ), ''.join('\n  ' + k for k in differ)))
    for k in ta:
        if k in tb:
            inside = ta[k][1] <= tb[k][0] <= ta[k][2]
            print('%-56s %10.1f (%.1f .. %.1f)   %10.1f (%.1f .. %.1f)   %s' % ((k,) + ta[k] + tb[k] + ('inside' if inside else 'OUTSIDE',)))
    return 1 if differ or set(ha) != set(hb) else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5, help='0: the hashes only')
    ap.add_argument('--out', default=None)
    ap.add_argument('--compare', nargs=2, metavar=('FIRST', 'SECOND'))
    args = ap.parse_args()
    if args.compare:
        raise SystemExit(compare(*args.compare))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('pair_grid_entry_probe: no device (the probe runs the device entries; there is no fallback)')
    from se3et_amd._lib import LIB_PATH
    lines = ['pair_grid_entry_probe: %s, library %s; times in us: median (min .. max) over %d rounds of the median of %d calls after %d '
             'warm-up calls' % (torch.cuda.get_device_name(0), os.path.basename(os.path.dirname(LIB_PATH)) + '/' + os.path.basename(LIB_PATH),
                                args.rounds, args.reps, args.warmup)]
    measure(torch, args, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
