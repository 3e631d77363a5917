"""RANSAC registration from correspondences on the device: the reference's registration_with_ransac_from_correspondences
(geotransformer/utils/open3d.py:169-198, Open3D's CPU RANSAC, eval.py --method ransac) as one batched HIP call for all pairs
(csrc/ransac.hip), plus the eval.py registration step for forward_pairs outputs (--method lgr / svd / ransac, --num_corr).

  ransac_pairs(src_list, ref_list, threshold, ransac_n, iterations)    (P, ...) device tensors for P pairs, three launches
  registration_with_ransac_from_correspondences(src, ref, ...)         drop-in: float64 numpy (4, 4) like result.transformation
  ransac_from_feats_pairs(src_points, ref_points, src_feats, ref_feats, ...)   descriptor matching (se3et_amd/feature_matching.py), then
                                                                       RANSAC with Open3D's edge-length and distance checkers
  registration_with_ransac_from_feats(src, ref, src_feats, ref_feats, ...)     drop-in (geotransformer/utils/open3d.py:133-166)
  select_correspondences(out, num_corr)                                eval.py's --num_corr cut (top scores, stable order)
  register_pairs(cfg, outs, method, num_corr)                          (B, 4, 4) estimated transforms of B forward_pairs dicts
  sample_indices(seed, n, num_iterations, ransac_n)                    the device sampler's indices, in numpy

Contract (restated from Open3D's pipelines/registration/Registration.cpp, versions >= 0.13, called with
TransformationEstimationPointToPoint(False), no checkers and RANSACConvergenceCriteria(num_iterations, num_iterations)):
  1. ransac_n < 3, n < ransac_n or distance_threshold <= 0: the identity with fitness 0 and RMSE 0.
  2. Each of the num_iterations hypotheses draws ransac_n correspondence indices uniformly, with replacement.
  3. It is fitted by unweighted, unscaled Kabsch (plain centroids, H = sum (s - s_)(r - r_)^T, reflection fixed by diag(1, 1, det)),
     src -> ref, in float64.
  4. It is scored against all n correspondences: i is an inlier iff |T s_i - r_i| < distance_threshold; fitness = inliers / n,
     inlier_rmse = sqrt(sum over the inliers of d^2 / inliers), 0 without inliers.
  5. A beats B iff fitness_A > fitness_B, or equal fitness and rmse_A < rmse_B.  The initial best is the identity with fitness 0 and
     RMSE 0, so a run in which no hypothesis has an inlier returns the identity.
  6. No early exit: all num_iterations hypotheses are evaluated (the criteria's confidence is clamped to 1).
  7. No refit: the winner's own fit is returned.

Where this differs from Open3D:
  - The random stream.  Open3D's is thread-dependent and not reproducible; here index j of hypothesis h is
      idx = ((splitmix64(splitmix64(seed) + h * ransac_n + j) >> 32) * n) >> 32        (uint64 wrap-around)
    with the standard splitmix64 (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB; sample_indices below).  It depends on
    (seed, h, j, n) only, so a pair's samples do not depend on its position in a batch, and the same seed gives the same result.
  - The order among equal candidates: hypotheses are ranked by (inlier count, then the smaller inlier error sum, then the lower h).  For
    equal counts the smaller error sum is the smaller RMSE, so this refines rule 5 into a total order.
  - Arithmetic: the fit is float64, rounded to float32; the test is d^2 < threshold^2 in float32 with d = R s + (t - r), and each
    hypothesis sums its inlier d^2 in float32, serially in correspondence order.  Counts are integers.  A pair's result is therefore
    bit-identical alone or in any batch, and from run to run.
  - Non-finite correspondences are never inliers; a hypothesis whose sample is non-finite has 0 inliers.

Optional checkers (Open3D's CorrespondenceCheckerBasedOnEdgeLength and ...BasedOnDistance; off by default, and then every output is
bit-identical to a call without them).  A rejected hypothesis scores 0 inliers:
  - edge_length_similarity = t: before the fit, over all pairs (a, b) of the sampled correspondences, the hypothesis is rejected if
    |s_a - s_b| < t |r_a - r_b| or |r_a - r_b| < t |s_a - s_b|, in float64;
  - check_distance: after the fit, it is rejected if a sampled correspondence has d^2 > distance_threshold^2 in the scoring arithmetic."""
import numpy as np
import torch

from . import ops as _ops
from .stacking import as_rows, device_offsets, exclusive_offsets, lengths, stack, upload

_MASK = (1 << 64) - 1
_GAMMA, _M1, _M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def _splitmix64(x):
    """Standard splitmix64 output for state x (uint64 numpy array): mix(x + 0x9E3779B97F4A7C15)."""
    z = x + np.uint64(_GAMMA)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(_M1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(_M2)
    return z ^ (z >> np.uint64(31))


def sample_indices(seed, n, num_iterations, ransac_n):
    """The device sampler in numpy: (num_iterations, ransac_n) int64 indices in [0, n),
    idx[h, j] = ((splitmix64(splitmix64(seed) + h * ransac_n + j) >> 32) * n) >> 32."""
    n, H, rn = int(n), int(num_iterations), int(ransac_n)
    if not 0 <= n < 1 << 32:
        raise ValueError('sample_indices: n = %d outside [0, 2^32)' % n)
    with np.errstate(over='ignore'):
        key = _splitmix64(np.array([int(seed) & _MASK], dtype=np.uint64))[0]
        k = key + np.arange(H, dtype=np.uint64)[:, None] * np.uint64(rn) + np.arange(rn, dtype=np.uint64)[None, :]
        u = _splitmix64(k) >> np.uint64(32)
        return ((u * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


@torch.no_grad()
def ransac_pairs(src_list, ref_list, distance_threshold, ransac_n, num_iterations, seed=0, correspondences=None, hypothesis_indices=None,
                 per_hypothesis=False, device='cuda', edge_length_similarity=None, check_distance=False):
    """RANSAC for P pairs in one batched call: src_list[p] / ref_list[p] (n_p, 3) numpy arrays or tensors, corresponding row by row, or
    -- with correspondences[p], a (K_p, 2) table of (src index, ref index) as Open3D takes it -- the pair's point clouds.  Returns
    {transforms (P, 4, 4), fitness (P,), inlier_rmse (P,), best_hypothesis (P,) int32 (-1: identity)} as device tensors (and counts /
    err_sums (P, H) with per_hypothesis).  hypothesis_indices: (P, H, ransac_n) int32 samples instead of the seeded sampler.
    edge_length_similarity / check_distance: the optional checkers of the module docstring (with per_hypothesis also passed (P, H) bool)."""
    if len(src_list) != len(ref_list) or (correspondences is not None and len(correspondences) != len(src_list)):
        raise ValueError('ransac_pairs: one src, ref (and correspondence table) per pair')
    if len(src_list) and torch.is_tensor(src_list[0]) and src_list[0].is_cuda:          # (the first src cloud's device wins over `device`:
        device = src_list[0].device                                                      # not the rule of stacking.device_of)
    srcs, refs = [], []
    for p, (s, r) in enumerate(zip(src_list, ref_list)):
        s, r = as_rows(s, device), as_rows(r, device)
        if correspondences is not None and correspondences[p] is not None:
            c = as_rows(correspondences[p], device, 2, torch.int64)
            s, r = s[c[:, 0]], r[c[:, 1]]
        elif s.shape != r.shape:
            raise ValueError('ransac_pairs: pair %d has %d src and %d ref rows' % (p, s.shape[0], r.shape[0]))
        srcs.append(s)
        refs.append(r)
    offsets = device_offsets(lengths(srcs), device)
    empty = torch.zeros((0, 3), dtype=torch.float32, device=device)
    src, ref = stack(srcs, empty), stack(refs, empty)
    if hypothesis_indices is not None and not torch.is_tensor(hypothesis_indices):
        hypothesis_indices = torch.as_tensor(np.asarray(hypothesis_indices, dtype=np.int32))
    if hypothesis_indices is not None:
        hypothesis_indices = hypothesis_indices.to(device=device, dtype=torch.int32)
    if edge_length_similarity is None and not check_distance:
        return _ops.ransac_stack(src, ref, offsets, distance_threshold, ransac_n, num_iterations, seed, hypothesis_indices, per_hypothesis)
    return _ops.ransac_stack(src, ref, offsets, distance_threshold, ransac_n, num_iterations, seed, hypothesis_indices, per_hypothesis,
                             edge_length_similarity, check_distance)


def registration_with_ransac_from_correspondences(src_points, ref_points, correspondences=None, distance_threshold=0.05, ransac_n=3,
                                                  num_iterations=10000, seed=0):
    """Drop-in for geotransformer.utils.open3d.registration_with_ransac_from_correspondences (same signature and defaults, plus the
    sampler's seed): the (4, 4) float64 numpy transform src -> ref."""
    out = ransac_pairs([src_points], [ref_points], distance_threshold, ransac_n, num_iterations, seed,
                       None if correspondences is None else [correspondences])
    return out['transforms'][0].cpu().numpy().astype(np.float64)


@torch.no_grad()
def ransac_from_feats_pairs(src_points_list, ref_points_list, src_feats_list, ref_feats_list, distance_threshold=0.05, ransac_n=3,
                            num_iterations=50000, mutual_filter=False, seed=0, edge_length_similarity=0.9, check_distance=True,
                            per_hypothesis=False):
    """Registration from descriptors for P pairs (Open3D's registration_ransac_based_on_feature_matching as
    registration_with_ransac_from_feats calls it): each SRC point is matched to its feature-nearest REF point
    (feature_matching.nearest_feature_pairs: no (N, M) matrix), then ransac_pairs runs on those correspondences with the edge-length (0.9)
    and distance checkers.  mutual_filter keeps only the correspondences whose ref point's nearest src point is the src point itself; a
    pair left with fewer than ransac_n of them falls back to all of its correspondences, as Open3D does.  The host synchronises a fixed
    number of times per call (the mutual counts, the compaction and its pair boundaries), not once per pair.  Points and features are (n, 3) /
    (n, C) float32 GPU tensors.  Returns the dict of ransac_pairs plus correspondences: per pair an (K_p, 2) int64 (src, ref) table."""
    from . import feature_matching as _fm
    P = len(src_points_list)
    if not (len(ref_points_list) == len(src_feats_list) == len(ref_feats_list) == P):
        raise ValueError('ransac_from_feats_pairs: one src / ref point and feature array per pair')
    for p in range(P):
        if src_points_list[p].shape[0] != src_feats_list[p].shape[0] or ref_points_list[p].shape[0] != ref_feats_list[p].shape[0]:
            raise ValueError('ransac_from_feats_pairs: pair %d has a different number of points and features' % p)
    nn_src, _ds, nn_ref, _dr = _fm.nearest_feature_pairs(ref_feats_list, src_feats_list)
    keep = [i >= 0 for i in nn_ref]                          # per src row: it has a ref row at all
    sizes = lengths(nn_ref)
    if mutual_filter and P:
        mutual = []
        for p in range(P):                                   # (an empty ref cloud has nothing to gather from: no mutual correspondence)
            j = torch.arange(sizes[p], dtype=torch.int64, device=nn_ref[p].device)
            mutual.append(keep[p] & (nn_src[p][nn_ref[p].clamp(min=0)] == j) if nn_src[p].shape[0] else torch.zeros_like(keep[p]))
        enough = torch.stack([m.sum() for m in mutual]).cpu().tolist()          # one read-back for all pairs
        keep = [m if c >= ransac_n else k for m, k, c in zip(mutual, keep, enough)]
    tables = []
    if P:
        rows = torch.nonzero(torch.cat(keep)).reshape(-1)    # one compaction for all pairs; rows ascend, so pairs stay contiguous
        starts = exclusive_offsets(sizes)
        cuts = torch.searchsorted(rows, torch.as_tensor(starts, dtype=torch.int64, device=rows.device)).cpu().tolist()
        all_ref = torch.cat(nn_ref)
        for p in range(P):
            j = rows[cuts[p]:cuts[p + 1]]
            tables.append(torch.stack([j - starts[p], all_ref[j]], 1))
    out = ransac_pairs(src_points_list, ref_points_list, distance_threshold, ransac_n, num_iterations, seed, correspondences=tables,
                       per_hypothesis=per_hypothesis, edge_length_similarity=edge_length_similarity, check_distance=check_distance)
    out['correspondences'] = tables
    return out


def registration_with_ransac_from_feats(src_points, ref_points, src_feats, ref_feats, distance_threshold=0.05, ransac_n=3,
                                        num_iterations=50000, val_iterations=1000, mutual_filter=False, seed=0):
    """Drop-in for geotransformer.utils.open3d.registration_with_ransac_from_feats (same signature and defaults, plus mutual_filter and the
    sampler's seed): the (4, 4) float64 numpy transform src -> ref.  Arrays are uploaded inside the call.
    val_iterations is accepted and has NO effect: in Open3D >= 0.13 that slot of RANSACConvergenceCriteria is a confidence, clamped to 1,
    so all num_iterations hypotheses are evaluated (item 6 of the contract).  The early stop of older Open3D versions after
    val_iterations validated hypotheses is not reproduced."""
    src_feats, ref_feats = np.asarray(src_feats), np.asarray(ref_feats)
    up = lambda a, w=3: upload(a, 'cuda', w, np.float32)
    out = ransac_from_feats_pairs([up(src_points)], [up(ref_points)], [up(src_feats, src_feats.shape[-1])],
                                  [up(ref_feats, ref_feats.shape[-1])], distance_threshold, ransac_n, num_iterations, mutual_filter, seed)
    return out['transforms'][0].cpu().numpy().astype(np.float64)


def select_correspondences(out, num_corr):
    """eval.py's --num_corr cut of one output dict: (ref_corr_points, src_corr_points, corr_scores) of the num_corr highest corr_scores,
    or all of them when num_corr is None or not smaller than their count.  The order is a STABLE descending sort, so equal scores keep
    the lower index first; the reference's np.argsort(-scores) (quicksort) leaves the order of ties unspecified."""
    ref, src, scores = out['ref_corr_points'], out['src_corr_points'], out['corr_scores']
    if num_corr is None or scores.shape[0] <= num_corr:
        return ref, src, scores
    order = torch.sort(scores, descending=True, stable=True).indices[:num_corr]
    return ref[order], src[order], scores[order]


@torch.no_grad()
def register_pairs(cfg, outs, method, num_corr=None, seed=0):
    """eval.py's registration step for the B output dicts of batched.forward_pairs: (B, 4, 4) device float32 transforms.
      'lgr'     the forward's estimated_transform, unchanged;
      'svd'     weighted Procrustes over each pair's (num_corr-cut) correspondences with corr_scores as weights, one launch for all pairs;
      'ransac'  ransac_pairs with cfg.ransac (distance_threshold, num_points, num_iterations) on the (num_corr-cut) correspondences."""
    if method == 'lgr':
        return torch.stack([out['estimated_transform'] for out in outs], 0)
    if method not in ('svd', 'ransac'):
        raise ValueError('register_pairs: unsupported registration method %r' % (method,))
    cut = [select_correspondences(out, num_corr) for out in outs]
    if method == 'ransac':
        r = cfg.ransac
        return ransac_pairs([c[1] for c in cut], [c[0] for c in cut], r.distance_threshold, r.num_points, r.num_iterations,
                            seed)['transforms']
    offsets = device_offsets(lengths([c[2] for c in cut]), cut[0][0].device)
    return _ops.weighted_procrustes(torch.cat([c[1] for c in cut], 0), torch.cat([c[0] for c in cut], 0),
                                    torch.cat([c[2] for c in cut], 0), offsets, eps=1e-5)
