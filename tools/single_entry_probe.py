"""Device time of the single-cloud / single-pair entry points of the superpoint level -- se3_knn3, se3_point_to_node_partition,
se3_superpoint_scores, se3_cross_eq_stats + _mix + _apply -- at the shapes one single-pair forward of the benchmark passes them
(profiles/single_entry_points_parent_vs_pr.txt).

One forward of a c2_5k pair through the per-module path (model.packed_inference = False: the path of the reference-shaped drop-in and of the
training step) records the arguments of the first call of every op and the shapes of all calls; each op is then repeated on those
arguments between two device events.  Per op: median (min .. max) in microseconds over --reps repetitions after --warmup calls.  The library
is the one SE3_LIB names (default: the in-tree build), so two builds are compared by running the probe once per library.  Recorded, not
gated.  Run `python tools/single_entry_probe.py [--out FILE]` on the GPU box."""
import argparse
import ctypes
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('single_entry_probe: no device (the probe measures the device; there is no fallback)')
    from se3et_amd import ops
    from se3et_amd._lib import check, lib
    from se3et_amd.data import precompute_data_stack_mode
    from se3et_amd.model import create_model, load_synthetic_weights, make_cfg
    from se3et_amd.synthetic import make_pair
    cfg = make_cfg('se3ete')
    model = load_synthetic_weights(create_model(cfg)).cuda().eval()
    b = cfg.backbone
    ref, src, _ = make_pair('c2_5k', index=1000)
    data = precompute_data_stack_mode(torch.from_numpy(np.concatenate([ref, src])).cuda(), torch.tensor([len(ref), len(src)]), b.num_stages,
                                      b.init_voxel_size, b.init_radius, cfg.neighbor_limits)
    data['features'] = torch.ones((len(ref) + len(src), 1), device='cuda')

    first, shapes = {}, {}
    keep = {name: getattr(ops, name) for name in ('cross_attention_eq', 'superpoint_scores', 'point_to_node_partition', 'geometric_embedding')}

    def recorder(name, describe):
        def wrapped(*a, **k):
            first.setdefault(name, tuple(t.detach().clone() if torch.is_tensor(t) else t for t in a))
            shapes.setdefault(name, []).append(describe(*a, **k))
            return keep[name](*a, **k)
        return wrapped
    ops.cross_attention_eq = recorder('cross_attention_eq', lambda q, k, vt, H, mode, t: 'A %d N %d M %d C %d H %d %s' % (*q.shape[:2], k.shape[1], q.shape[2], H, mode))
    ops.superpoint_scores = recorder('superpoint_scores', lambda r, s, dual: 'N %d M %d C %d dual %s' % (r.shape[0], s.shape[0], r.shape[1], bool(dual)))
    ops.point_to_node_partition = recorder('point_to_node_partition', lambda p, n, limit: 'N %d M %d limit %d' % (p.shape[0], n.shape[0], limit))
    ops.geometric_embedding = recorder('geometric_embedding', lambda p, *a, **k: 'N %d' % p.shape[0])
    model.packed_inference = False
    try:
        model(data)
    finally:
        model.packed_inference = True
        for name, f in keep.items():
            setattr(ops, name, f)
    torch.cuda.synchronize()
    for name in keep:
        if name not in first:
            raise SystemExit('single_entry_probe: the per-module forward did not call ops.%s' % name)

    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        out = []
        for _ in range(args.reps):
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            out.append(start.elapsed_time(stop) * 1e3)
        return statistics.median(out), min(out), max(out)

    pts = first['geometric_embedding'][0].contiguous()
    knn = torch.empty((pts.shape[0], 3), dtype=torch.int64, device='cuda')
    q, k, vt, H, mode, trace = first['cross_attention_eq']
    A, N, C = q.shape
    M, scale = k.shape[1], 1.0 / math.sqrt(C // H)
    partial = torch.empty((A * A, (N + 31) // 32), device='cuda')
    nparts = ctypes.c_int(0)
    out, ret, mix = keep['cross_attention_eq'](q, k, vt, H, mode, trace)
    rows = [
        ('se3_knn3', shapes['geometric_embedding'],
         lambda: check(lib().se3_knn3(pts.data_ptr(), pts.shape[0], knn.data_ptr(), ops._stream()), 'se3_knn3')),
        ('se3_point_to_node_partition', shapes['point_to_node_partition'], lambda: keep['point_to_node_partition'](*first['point_to_node_partition'])),
        ('se3_superpoint_scores', shapes['superpoint_scores'], lambda: keep['superpoint_scores'](*first['superpoint_scores'])),
        ('cross_eq stats + mix + apply', shapes['cross_attention_eq'], lambda: keep['cross_attention_eq'](q, k, vt, H, mode, trace)),
        ('se3_cross_eq_stats alone', shapes['cross_attention_eq'][:1],
         lambda: check(lib().se3_cross_eq_stats(q.data_ptr(), k.data_ptr(), A, N, M, C, H, scale, partial.data_ptr(), ctypes.byref(nparts),
                                                ops._stream()), 'se3_cross_eq_stats')),
        ('se3_cross_eq_apply alone', shapes['cross_attention_eq'][:1],
         lambda: check(lib().se3_cross_eq_apply(q.data_ptr(), k.data_ptr(), vt.data_ptr(), mix.data_ptr(), A, N, M, C, H, vt.shape[2], scale,
                                                out.data_ptr(), ops._stream()), 'se3_cross_eq_apply')),
    ]
    lines = ['single_entry_probe: %s, one c2_5k pair through the per-module forward; device events around one call on the arguments of the '
             'first call of the forward, us: median (min .. max) over %d repetitions after %d warm-up calls' % (torch.cuda.get_device_name(0), args.reps,
                                                                                                                 args.warmup)]
    for name, seen, fn in rows:
        calls = ', '.join('%s x %d' % (s, seen.count(s)) for s in dict.fromkeys(seen))
        lines.append('%-30s %9.1f (%.1f .. %.1f)   timed: %s; calls of the forward: %s' % ((name,) + timed(fn) + (seen[0], calls)))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
