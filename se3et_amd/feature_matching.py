"""Feature-space matching on the device: the reference's descriptor-matching helpers -- extract_correspondences_from_feats
(geotransformer/modules/registration/matching.py:135-170), extract_corr_indices_from_feats and extract_correspondences_from_feats
(geotransformer/utils/registration.py:179-234) -- as batched HIP calls (csrc/feature_nn.hip) that never build the (N, M) distance matrix.

  nearest_feature_pairs(ref_feats_list, src_feats_list)                     per pair: nn_src, sq distances, nn_ref, sq distances
  extract_correspondences_from_feats_pairs(ref_feats_list, src_feats_list, mutual, bilateral, return_feat_dist)
                                                                            per pair: ref / src correspondence indices (int64)
  extract_corr_indices_from_feats / extract_correspondences_from_feats      the reference's numpy names and signatures, one pair per call
  (the torch-named mirror is se3et_amd.modules.registration.extract_correspondences_from_feats)

The batched calls take GPU tensors only (there is no CPU path) and any number of pairs; the memory is O(N + M) per pair and a call makes
one host synchronisation (the sizes of the lists; nearest_feature_pairs makes none).

Contract (csrc/feature_nn.hip carries the same text).  For a query row x and the rows y of the other cloud of its pair:
  - candidates are ranked by v = (|x|^2 - 2 x.y) + |y|^2 in float32 (f32 MFMA products, one fixed-order norm per row); among exactly equal
    v the lowest index wins; a NaN or infinite v is never chosen; a row without a candidate (non-finite features, empty other cloud) gets
    index -1, distance +inf, and produces no correspondence;
  - the distance returned is recomputed for the winner as sum (x - y)^2 -- squared, and not the cancelling expression above;
  - results are bit-identical from run to run and for a pair alone or in any batch.
Extraction:
  one-way                 (i, nn_src(i)) for every ref row i;
  mutual                  the rows with nn_ref(nn_src(i)) == i, ascending in i;
  bilateral (pairs call)  the torch form: the union of (i, nn_src(i)) and (nn_ref(j), j), duplicates once, in row-major (i, j) order, i.e.
                          nonzero of the OR-ed masks of matching.py:52-61; the numpy drop-in keeps the numpy form
                          [arange(N), nn_ref] / [nn_src, arange(M)] with duplicates (bilateral='concat' in the pairs call).
Where this differs from the reference: the reference's numpy form searches a cKDTree in float64 and its torch form ranks the clamped
float32 matrix (x2 - 2 xy + y2 with y as the column for BOTH directions); only rows whose two best candidates lie within float32 rounding
of each other can come out differently.  The torch form's exp(-d^2) > 0 cut is applied by the torch-named mirror only."""
import numpy as np
import torch

from . import ops as _ops
from .stacking import device_offsets, gpu_rows_each, lengths, stack, upload


def stack_feature_pairs(ref_feats_list, src_feats_list, what='stack_feature_pairs'):
    """Validates per-pair (n, C) float32 GPU features and stacks them: (ref stacked, src stacked, ref offsets, src offsets -- int64 on the
    device --, ref lengths, src lengths)."""
    if len(ref_feats_list) != len(src_feats_list):
        raise ValueError('%s: one ref and one src feature array per pair' % what)
    refs, srcs = (gpu_rows_each(lst, None, '%s: %s_feats' % (what, side), 'feature matching', cols=None, dtypes=(torch.float32,))
                  for side, lst in (('ref', ref_feats_list), ('src', src_feats_list)))
    if not refs:
        raise ValueError('%s: no pairs' % what)
    C = refs[0].shape[1]
    if any(x.shape[1] != C for x in refs + srcs) or C < 1:
        raise RuntimeError('%s: all features must have the same channel count >= 1' % what)
    dev = refs[0].device
    nl, ml = lengths(refs), lengths(srcs)
    return stack(refs), stack(srcs), device_offsets(nl, dev), device_offsets(ml, dev), nl, ml


@torch.no_grad()
def nearest_feature_pairs(ref_feats_list, src_feats_list):
    """For P pairs of (N_p, C) / (M_p, C) float32 GPU features: four lists of per-pair tensors (nn_src (N_p,) int64: the nearest src row
    of every ref row, its squared distance (N_p,) float32, nn_ref (M_p,), its squared distance).  No host synchronisation."""
    ref, src, ro, so, nl, ml = stack_feature_pairs(ref_feats_list, src_feats_list, 'nearest_feature_pairs')
    nn_src, d_src, nn_ref, d_ref = _ops.feature_nn_stack(ref, src, ro, so)
    return list(torch.split(nn_src, nl)), list(torch.split(d_src, nl)), list(torch.split(nn_ref, ml)), list(torch.split(d_ref, ml))


@torch.no_grad()
def extract_correspondences_from_feats_pairs(ref_feats_list, src_feats_list, mutual=False, bilateral=False, return_feat_dist=False):
    """Correspondences of P pairs from their features: (ref_corr_indices list, src_corr_indices list[, squared feature distances list]) of
    per-pair int64 device tensors.  mutual: only mutual nearest neighbours; bilateral (ignored with mutual): both directions, True for the
    torch form (union, row-major), 'concat' for the numpy form (concatenated, duplicates kept).  Distances are SQUARED and recomputed as
    sum (x - y)^2 for each correspondence's rows."""
    ref, src, ro, so, nl, ml = stack_feature_pairs(ref_feats_list, src_feats_list, 'extract_correspondences_from_feats_pairs')
    nn_src, d_src, nn_ref, d_ref = _ops.feature_nn_stack(ref, src, ro, so)
    mode = 'mutual' if mutual else ('bilateral_concat' if bilateral == 'concat' else ('bilateral_mask' if bilateral else 'one_way'))
    ci, cj, bounds = _ops.feature_corr_stack(nn_src, nn_ref, ro, so, mode)
    sizes = np.diff(bounds).tolist()
    out = [list(torch.split(ci, sizes)), list(torch.split(cj, sizes))]
    if return_feat_dist:
        dists = []
        for p, (i, j) in enumerate(zip(*out)):
            a, b = sum(nl[:p]), sum(ml[:p])
            # an entry is (i, nn_src(i)) or (nn_ref(j), j): its distance is the one the search recomputed for that row
            dists.append(torch.where(nn_src[a + i] == j, d_src[a + i], d_ref[b + j]))
        out.append(dists)
    return tuple(out)


# ---- the reference's numpy functions: one pair, numpy in and out -------------------------------------------------------------------------------
def _upload(feats, device):
    if np.ndim(feats) != 2:
        raise ValueError('features must be (n, C)')
    return upload(feats, device, None, np.float32)


def extract_corr_indices_from_feats(ref_feats, src_feats, mutual=False, bilateral=False, device=None):
    """geotransformer.utils.registration.extract_corr_indices_from_feats: (ref_corr_indices, src_corr_indices) int64 numpy; bilateral is the
    concatenated form of the reference, duplicates kept.  The features are uploaded as float32."""
    i, j = extract_correspondences_from_feats_pairs([_upload(ref_feats, device)], [_upload(src_feats, device)], mutual=mutual,
                                                    bilateral='concat' if bilateral else False)
    return i[0].cpu().numpy(), j[0].cpu().numpy()


def extract_correspondences_from_feats(ref_points, src_points, ref_feats, src_feats, mutual=False, return_feat_dist=False, device=None):
    """geotransformer.utils.registration.extract_correspondences_from_feats: [ref_corr_points, src_corr_points(, feat_dists)] as numpy;
    feat_dists is the Euclidean distance: the square root of the recomputed squared distance (float32)."""
    out = extract_correspondences_from_feats_pairs([_upload(ref_feats, device)], [_upload(src_feats, device)], mutual=mutual,
                                                   return_feat_dist=return_feat_dist)
    i, j = out[0][0].cpu().numpy(), out[1][0].cpu().numpy()
    result = [np.asarray(ref_points)[i], np.asarray(src_points)[j]]
    if return_feat_dist:
        result.append(torch.sqrt(out[2][0]).cpu().numpy())
    return result
