"""Cost of the registration evaluation on the C2 16-pair batch (profiles/eval_probe.txt).

Times, with device events after warm-up:
  hip      ground-truth overlaps (se3_gt_node_overlaps_stack) + metrics (se3_registration_metrics_stack) for all 16 pairs, from the
           batch's partition (the forward computes it anyway);
  torch    today's per-pair path: training.node_correspondences + a plain-torch restatement of the reference Evaluator, pair by pair;
  forward  batched.forward_pairs alone, for scale.
Run `python tools/eval_probe.py [--iters N] [--out FILE]`; under `rocprofv3 --kernel-trace --stats` for the kernel times and launches."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from se3et_amd import functional as SF  # noqa: E402
from se3et_amd import ops  # noqa: E402
from se3et_amd.batched import forward_pairs  # noqa: E402
from se3et_amd.data import precompute_data_stack_mode  # noqa: E402
from se3et_amd.evaluation import evaluate_pairs  # noqa: E402
from se3et_amd.model import create_model, load_synthetic_weights, make_cfg  # noqa: E402
from se3et_amd.synthetic import make_pair  # noqa: E402
from se3et_amd.training import node_correspondences  # noqa: E402


def torch_evaluator(cfg, out, T, gi, go):
    """experiments/se3ete.3dmatch/loss.py:198-262 in plain torch (one pair)."""
    e = cfg.eval
    gmap = torch.zeros(out['ref_points_c'].shape[0], out['src_points_c'].shape[0], device=T.device)
    m = go > e.acceptance_overlap
    gmap[gi[m, 0], gi[m, 1]] = 1.0
    pir = gmap[out['ref_node_corr_indices'], out['src_node_corr_indices']].mean()
    d = torch.linalg.norm(out['ref_corr_points'] - SF.apply_transform(out['src_corr_points'], T), dim=1)
    ir = (d < e.acceptance_radius).float().mean()
    est = out['estimated_transform']
    tr = (est[:3, :3].T @ T[:3, :3]).trace()
    rre = torch.rad2deg(torch.arccos(((tr - 1) / 2).clamp(-1, 1)))
    rte = torch.linalg.norm(T[:3, 3] - est[:3, 3])
    sp = out['src_points']
    rmse = torch.linalg.norm(SF.apply_transform(sp, torch.inverse(T) @ est) - sp, dim=1).mean()
    return pir, ir, rre, rte, rmse, (rmse < e.rmse_threshold).float()


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
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    cfg = make_cfg('se3ete')
    model = load_synthetic_weights(create_model(cfg)).cuda().eval()
    b = cfg.backbone
    clouds, Ts = [], []
    for i in range(args.pairs):          # stacked ref0, src0, ref1, src1, ... as bench.py builds its batches
        ref, src, T = make_pair('c2_5k', i)
        clouds += [ref, src]
        Ts.append(T)
    pts = torch.from_numpy(np.concatenate(clouds, 0)).cuda()
    data = precompute_data_stack_mode(pts, torch.tensor([len(c) for c in clouds]), b.num_stages, b.init_voxel_size, b.init_radius,
                                      cfg.neighbor_limits)
    data['features'] = torch.ones((pts.shape[0], 1), device='cuda')
    T = torch.from_numpy(np.stack(Ts)).cuda()
    outs = forward_pairs(model, data)
    pf, pc = data['points'][1], data['points'][-1]
    lf, lc = data['lengths'][1].tolist(), data['lengths'][-1].tolist()
    _, nm, knn, km = ops.point_to_node_partition_stack(pf, pc, lf, lc, model.num_points_in_patch)
    r = cfg.model.ground_truth_matching_radius

    def hip():
        gt = ops.gt_node_overlaps_stack(pf, pc, lc, knn, km, nm, T, r)
        for p, out in enumerate(outs):
            out['gt_node_corr_overlap_map'] = gt.block(p)
        return evaluate_pairs(cfg, outs, T)

    oc = [0]
    for n in lc:
        oc.append(oc[-1] + n)
    knn_pts = SF.gather_rows_padded(pf, knn)

    def plain():
        res = []
        for p, out in enumerate(outs):
            a, c = slice(oc[2 * p], oc[2 * p + 1]), slice(oc[2 * p + 1], oc[2 * p + 2])
            gi, go = node_correspondences(pc[a], pc[c], knn_pts[a], knn_pts[c], T[p], r, nm[a], nm[c], km[a], km[c])
            res.append(torch_evaluator(cfg, out, T[p], gi, go))
        return res

    def forward():
        return forward_pairs(model, data)

    # the two paths agree (PIR, IR, RR exactly on these pairs; the torch restatement is the reference's arithmetic)
    h, t = hip(), plain()
    agree = all(float(h['PIR'][p]) == float(t[p][0]) and float(h['RR'][p]) == float(t[p][5]) for p in range(args.pairs))
    t_hip, t_torch, t_fwd = timed(hip, args.iters), timed(plain, args.iters), timed(forward, max(3, args.iters // 4))
    lines = ['eval_probe: C2 5k+5k pairs x %d (SE3ET-E, synthetic weights), %s' % (args.pairs, torch.cuda.get_device_name(0)),
             'hip   gt overlaps + metrics, all pairs        %8.3f ms per batch (wall, device events, %d iterations)' % (t_hip, args.iters),
             'torch node_correspondences + Evaluator/pair  %8.3f ms per batch' % t_torch,
             'forward_pairs alone                          %8.3f ms per batch' % t_fwd,
             'hip / forward = %.2f %%; torch / hip = %.1fx; PIR and RR of both paths equal: %s' % (100 * t_hip / t_fwd, t_torch / t_hip, agree)]
    print('\n'.join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
