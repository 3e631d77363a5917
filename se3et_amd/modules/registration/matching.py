from typing import Optional

import torch

from ...training import node_correspondences


@torch.no_grad()
def get_node_correspondences(ref_nodes: torch.Tensor, src_nodes: torch.Tensor, ref_knn_points: torch.Tensor,
                             src_knn_points: torch.Tensor, transform: torch.Tensor, pos_radius: float,
                             ref_masks: Optional[torch.Tensor] = None, src_masks: Optional[torch.Tensor] = None,
                             ref_knn_masks: Optional[torch.Tensor] = None, src_knn_masks: Optional[torch.Tensor] = None):
    """Ground-truth superpoint (patch) correspondences under `transform` (geotransformer/modules/registration/matching.py:231-315;
    imported by experiments/se3ete.3dmatch/model.py:7, called at :110-121): patch pairs (M superpoints with K nearest points each,
    against N) holding at least one pair of points closer than `pos_radius`, overlap = mean of the two covered fractions.
    -> corr_indices (C, 2) int64 in row-major (ref, src) order, corr_overlaps (C,).  Absent masks mean "all valid"; they are created on the
    device of the inputs (the reference hard-codes `.cuda()`).  The node and patch distance matrices run on se3_pairwise_distance for
    float32 GPU tensors (modules/ops/pairwise_distance.py)."""
    dev = ref_nodes.device
    ones = lambda *shape: torch.ones(shape, dtype=torch.bool, device=dev)
    ref_masks = ones(ref_nodes.shape[0]) if ref_masks is None else ref_masks
    src_masks = ones(src_nodes.shape[0]) if src_masks is None else src_masks
    ref_knn_masks = ones(*ref_knn_points.shape[:2]) if ref_knn_masks is None else ref_knn_masks
    src_knn_masks = ones(*src_knn_points.shape[:2]) if src_knn_masks is None else src_knn_masks
    return node_correspondences(ref_nodes, src_nodes, ref_knn_points, src_knn_points, transform, pos_radius, ref_masks, src_masks,
                                ref_knn_masks, src_knn_masks)


@torch.no_grad()
def extract_correspondences_from_feats(ref_feats: torch.Tensor, src_feats: torch.Tensor, mutual: bool = False, bilateral: bool = False,
                                       return_feat_dist: bool = False):
    """Correspondences by nearest neighbour in feature space (geotransformer/modules/registration/matching.py:135-170) without the (N, M)
    distance matrix: se3et_amd.feature_matching on csrc/feature_nn.hip, O(N + M) memory, one host synchronisation.
    -> ref_corr_indices (K,), src_corr_indices (K,) int64 in row-major (ref, src) order [, corr_feat_dists (K,) SQUARED distances,
    recomputed as sum (x - y)^2 for each correspondence].  mutual: mutual nearest neighbours only; bilateral (ignored with mutual): the
    union of both directions, duplicates once.
    The reference passes -d^2 as log-scores to extract_correspondences_from_scores, which keeps a nearest neighbour only where
    exp(-d^2) > 0 in float32 (matching.py:40-58): a neighbour farther than d^2 ~ 104 is dropped.  That cut is reproduced here, evaluated
    as torch.exp(-d^2) > 0 on the winners' distances only; with `mutual` both directions must survive it, as both masks must hold there.
    float32 GPU tensors only; float64 or CPU inputs raise (the reference would build the matrix with torch)."""
    from ... import feature_matching as FM
    from ... import ops as _ops
    ref, src, ro, so, _nl, _ml = FM.stack_feature_pairs([ref_feats], [src_feats], 'extract_correspondences_from_feats')
    nn_src, d_src, nn_ref, d_ref = _ops.feature_nn_stack(ref, src, ro, so)
    # the exp cut: a winner whose exp(-d^2) underflows to 0 is no correspondence (the index -1 produces nothing)
    nn_src = torch.where(torch.exp(-d_src) > 0, nn_src, torch.full_like(nn_src, -1))
    nn_ref = torch.where(torch.exp(-d_ref) > 0, nn_ref, torch.full_like(nn_ref, -1))
    mode = 'mutual' if mutual else ('bilateral_mask' if bilateral else 'one_way')
    ci, cj, _bounds = _ops.feature_corr_stack(nn_src, nn_ref, ro, so, mode)
    if return_feat_dist:
        return ci, cj, torch.where(nn_src[ci] == cj, d_src[ci], d_ref[cj])
    return ci, cj
