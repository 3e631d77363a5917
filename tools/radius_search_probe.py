"""The ten radius searches of one 16-pair benchmark step (c2_5k pairs, SE3ET-E pyramid: 780 840 queries) through ops.RadiusGrid(...).search,
alone on the GPU: an event pair around every launch, the median over the repetitions per search, and the four grid builds.  One line per run;
SE3_LIB selects another build of the library, so two builds are compared by running the probe once per library on one box
(profiles/radius_select_parent_vs_pr.txt).    python tools/radius_search_probe.py [repetitions]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from se3et_amd import ops  # noqa: E402
from se3et_amd.data import stage_clouds  # noqa: E402
from se3et_amd.model import make_cfg  # noqa: E402
from se3et_amd.synthetic import make_pair  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    cfg = make_cfg('se3ete')
    b = cfg.backbone
    clouds = []
    for i in range(16):
        ref, src, _ = make_pair('c2_5k', index=i)
        clouds += [ref, src]
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    lens = torch.tensor([len(c) for c in clouds])
    P, L = stage_clouds(pts, lens, b.num_stages, b.init_voxel_size)
    jobs, r = [], b.init_radius                      # (name, query stage, support stage, radius, limit): the order of data.precompute_data_stack_mode
    for i in range(b.num_stages):
        jobs.append(('nbr%d' % i, i, i, r, cfg.neighbor_limits[i]))
        if i < b.num_stages - 1:
            jobs.append(('sub%d' % i, i + 1, i, r, cfg.neighbor_limits[i]))
            jobs.append(('up%d' % i, i, i + 1, 2 * r, cfg.neighbor_limits[i + 1]))
        r *= 2
    times, build, checksum = {j[0]: [] for j in jobs}, [], 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1) * 1e3

    for rep in range(reps + 2):                      # two warm-up rounds
        grids = {}
        for name, qs, ss, rad, lim in jobs:
            if (ss, rad) not in grids:
                grids[(ss, rad)], us = timed(lambda: ops.RadiusGrid(P[ss], L[ss], rad))
                if rep >= 2:
                    build.append(us)
            mc = torch.zeros(len(lens), dtype=torch.int32, device='cuda')
            ties = (torch.empty(P[qs].shape[0], dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda'))
            (tab, _), us = timed(lambda: grids[(ss, rad)].search(P[qs], L[qs], lim, zeroed_max_count=mc, ties=ties))
            if rep >= 2:
                times[name].append(us)
            if rep == 0:                             # the same number from two builds that compute the same tables and counts
                checksum += int(tab.sum().item() % 1000003) + int(mc.sum().item())
    per = [(name, P[qs].shape[0], float(np.median(times[name]))) for name, qs, _, _, _ in jobs]
    print('%-14s total %.0f us  build (4 grids) %.0f us  checksum %d | %s' % (
        os.path.basename(os.environ.get('SE3_LIB', 'in-tree')), sum(p[2] for p in per), 4 * float(np.median(build)), checksum,
        ' | '.join('%s %d q %.0f' % p for p in per)))


if __name__ == '__main__':
    main()
