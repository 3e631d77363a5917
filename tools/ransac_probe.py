"""Cost of batched RANSAC registration (se3et_amd.ransac, csrc/ransac.hip) on the C2 16-pair batch (profiles/ransac_probe.txt).

Workload: the forward outputs of the C2 16-pair batch (SE3ET-E, synthetic weights) cut to the top --num-corr correspondences by score;
a pair with fewer gets synthetic correspondences of that size instead (ransac_twin.synthetic_pair, 10 % inliers), so every pair scores
num_corr correspondences.  3DMatch config: threshold 0.05, 3 points, 50 000 iterations.
Times, with device events after warm-up:
  device   ransac_pairs on all 16 pairs (three launches);
  host     the float64 numpy twin (tests/ransac_twin.py) on ONE pair, --host-iters hypotheses scaled to the full count, for scale.
FLOP convention: 28 FLOP per (hypothesis, correspondence) residual test -- 9 FMA = 18, 3 sub, 5 for d^2 (3 mul + 2 add), 2 for the
compare and the accumulate -- against the 157.3 TFLOP/s FP32 vector peak.  Kernel times: run under `rocprofv3 --kernel-trace --stats`.
Run `python tools/ransac_probe.py [--iters N] [--out FILE]`."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ransac_twin as RT  # noqa: E402
from se3et_amd.batched import forward_pairs  # noqa: E402
from se3et_amd.data import precompute_data_stack_mode  # noqa: E402
from se3et_amd.model import create_model, load_synthetic_weights, make_cfg  # noqa: E402
from se3et_amd.ransac import ransac_pairs, sample_indices, select_correspondences  # noqa: E402
from se3et_amd.synthetic import make_pair  # noqa: E402

PEAK_FP32_VECTOR = 157.3e12
FLOP_PER_TEST = 28


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=16)
    ap.add_argument('--num-corr', type=int, default=5000)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--host-iters', type=int, default=500)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    cfg = make_cfg('se3ete')
    r = cfg.ransac
    model = load_synthetic_weights(create_model(cfg)).cuda().eval()
    b = cfg.backbone
    clouds = []
    for i in range(args.pairs):
        ref, src, _ = make_pair('c2_5k', i)
        clouds += [ref, src]
    pts = torch.from_numpy(np.concatenate(clouds, 0)).cuda()
    data = precompute_data_stack_mode(pts, torch.tensor([len(c) for c in clouds]), b.num_stages, b.init_voxel_size, b.init_radius,
                                      cfg.neighbor_limits)
    data['features'] = torch.ones((pts.shape[0], 1), device='cuda')
    with torch.no_grad():
        outs = forward_pairs(model, data)
    rng = np.random.default_rng(0)
    srcs, refs, synthetic, forward_sizes = [], [], 0, []
    for out in outs:
        ref_c, src_c, _ = select_correspondences(out, args.num_corr)
        forward_sizes.append(int(src_c.shape[0]))
        if src_c.shape[0] < args.num_corr:
            s, t, _ = RT.synthetic_pair(rng, args.num_corr, 0.10)
            src_c, ref_c = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()
            synthetic += 1
        srcs.append(src_c)
        refs.append(ref_c)
    n_total = sum(int(s.shape[0]) for s in srcs)

    def device():
        return ransac_pairs(srcs, refs, r.distance_threshold, r.num_points, r.num_iterations, seed=0)

    t_dev = timed(device, args.iters)
    tests = float(n_total) * r.num_iterations
    s0, r0 = srcs[0].cpu().numpy(), refs[0].cpu().numpy()
    t0 = time.perf_counter()
    RT.run(s0, r0, r.distance_threshold, r.num_points, sample_indices(0, len(s0), args.host_iters, r.num_points), chunk=500)
    t_host = (time.perf_counter() - t0) * r.num_iterations / args.host_iters * 1e3
    res = device()
    fit = res['fitness'].cpu().numpy()
    lines = ['ransac_probe: %d pairs x %d correspondences (%d from the C2 forward cut to the top %d by score, %d synthetic: the forward '
             'gave %s), 3DMatch config (%g, %d points, %d iterations), %s'
             % (args.pairs, args.num_corr, args.pairs - synthetic, args.num_corr, synthetic, 'min %d / max %d' % (min(forward_sizes), max(forward_sizes)),
                r.distance_threshold, r.num_points, r.num_iterations, torch.cuda.get_device_name(0)),
             'device  ransac_pairs, all pairs            %9.3f ms per batch (wall, device events, %d iterations, 3 launches)'
             % (t_dev, args.iters),
             '        %.3g residual tests per batch -> %.3g tests/s; %.3f of the 157.3 TF FP32 vector peak at %d FLOP per test (wall)'
             % (tests, tests / (t_dev * 1e-3), tests * FLOP_PER_TEST / (t_dev * 1e-3) / PEAK_FP32_VECTOR, FLOP_PER_TEST),
             'host    float64 numpy twin, ONE pair        %9.1f ms (%d hypotheses timed, scaled to %d)'
             % (t_host, args.host_iters, r.num_iterations),
             'fitness of the 16 pairs: %s' % ' '.join('%.3f' % f for f in fit)]
    print('\n'.join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
