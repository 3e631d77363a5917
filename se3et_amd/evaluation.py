"""Registration evaluation on the device: the reference's Evaluator (experiments/se3ete.3dmatch/loss.py:198-262, 3DMatch;
experiments/se3eti.kitti/loss.py:94-151, KITTI) and the ground-truth patch overlaps it feeds on (get_node_correspondences,
geotransformer/modules/registration/matching.py:230-315), both as HIP kernels for all pairs of a batch (csrc/evaluation.hip).

  Evaluator(cfg)(output_dict, data_dict)   one pair, the reference's interface: 0-dim tensors PIR, IR, RRE, RTE, RMSE, RR (3DMatch) or
                                           PIR, IR, RRE, RTE, RR (KITTI: cfg.eval has no rmse_threshold)
  evaluate_pairs(cfg, outs, transforms)    the same keys as (B,) tensors for the B output dicts of batched.forward_pairs, one metrics launch

Ground truth comes from the output dict where it is there (forward_pairs(..., ground_truth=True) leaves the dense overlap block
gt_node_corr_overlap_map; the training / emit_ground_truth path leaves gt_node_corr_indices / _overlaps); otherwise it is computed
from the dict's ref/src_points_c and ref/src_points_f: point_to_node_partition again, then the overlap kernel.  Nothing here reads
the device results back to the host."""
import torch

from . import ops as _ops

KEYS_3DMATCH = ('PIR', 'IR', 'RRE', 'RTE', 'RMSE', 'RR')
KEYS_KITTI = ('PIR', 'IR', 'RRE', 'RTE', 'RR')
_COLUMN = {k: i for i, k in enumerate(KEYS_3DMATCH)}


def _is_kitti(cfg):
    return not hasattr(cfg.eval, 'rmse_threshold')


def ground_truth(cfg, outs, transforms):
    """GroundTruthOverlaps of the pairs of `outs` (dicts with ref/src_points_c and ref/src_points_f) under transforms (B, 4, 4): the
    patches of point_to_node_partition (cfg.model.num_points_in_patch points) and cfg.model.ground_truth_matching_radius."""
    clouds_f, clouds_c = [], []
    for out in outs:
        clouds_f += [out['ref_points_f'], out['src_points_f']]
        clouds_c += [out['ref_points_c'], out['src_points_c']]
    len_f, len_c = [int(t.shape[0]) for t in clouds_f], [int(t.shape[0]) for t in clouds_c]
    points_f, points_c = torch.cat(clouds_f, 0), torch.cat(clouds_c, 0)
    _, node_masks, knn, knn_masks = _ops.point_to_node_partition_stack(points_f, points_c, len_f, len_c, cfg.model.num_points_in_patch)
    return _ops.gt_node_overlaps_stack(points_f, points_c, len_c, knn, knn_masks, node_masks, transforms,
                                       cfg.model.ground_truth_matching_radius)


def _overlap_map(out):
    """Dense (N, M) overlaps of one output dict, or None if it holds no ground truth."""
    if 'gt_node_corr_overlap_map' in out:
        return out['gt_node_corr_overlap_map']
    if 'gt_node_corr_indices' in out:
        n, m = out['ref_points_c'].shape[0], out['src_points_c'].shape[0]
        gi, go = out['gt_node_corr_indices'], out['gt_node_corr_overlaps']
        dense = torch.zeros((n, m), dtype=torch.float32, device=go.device)
        dense[gi[:, 0], gi[:, 1]] = go.float()
        return dense
    return None


@torch.no_grad()
def evaluate_pairs(cfg, outs, transforms):
    """The Evaluator's metrics for B pairs at once: outs = B output dicts (forward_pairs), transforms (B, 4, 4) ground truth.
    Returns {key: (B,) float32 device tensor}."""
    e, kitti = cfg.eval, _is_kitti(cfg)
    dev = outs[0]['ref_points_c'].device
    transforms = transforms.to(dev, torch.float32).reshape(len(outs), 4, 4)
    maps = [_overlap_map(out) for out in outs]
    if any(m is None for m in maps):
        gt = ground_truth(cfg, outs, transforms)
        maps = [gt.block(p) for p in range(len(outs))]
    pairs = [(mp, out['ref_node_corr_indices'], out['src_node_corr_indices'], out['ref_corr_points'], out['src_corr_points'],
              out['estimated_transform'], None if kitti else out['src_points']) for mp, out in zip(maps, outs)]
    rows = _ops.registration_metrics_stack(pairs, transforms, e.acceptance_overlap, e.acceptance_radius,
                                           0.0 if kitti else e.rmse_threshold, e.rre_threshold, e.rte_threshold, kitti)
    return {k: rows[:, _COLUMN[k]] for k in (KEYS_KITTI if kitti else KEYS_3DMATCH)}


class Evaluator(torch.nn.Module):
    """Drop-in for the reference's Evaluator (same name, same cfg.eval keys, same output keys as 0-dim tensors) for one pair."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.acceptance_overlap = cfg.eval.acceptance_overlap
        self.acceptance_radius = cfg.eval.acceptance_radius
        if not _is_kitti(cfg):
            self.acceptance_rmse = cfg.eval.rmse_threshold
        else:
            self.rre_threshold, self.rte_threshold = cfg.eval.rre_threshold, cfg.eval.rte_threshold

    @torch.no_grad()
    def forward(self, output_dict, data_dict):
        rows = evaluate_pairs(self.cfg, [output_dict], data_dict['transform'])
        return {k: v[0] for k, v in rows.items()}
