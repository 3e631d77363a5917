"""Keypoint selection on the device: score ranking and radius non-maximum suppression, the "Sampling methods" of
geotransformer/utils/pointcloud.py:145-248 that reduce a cloud's dense points and features to the 250-5000 keypoints of the descriptor
protocol.  The NMS forms run as HIP kernels (csrc/keypoint_nms.hip on the grid of csrc/pair_grid.h) in place of the reference's Python loop
with one numpy pass per surviving point.

  nms_keypoints_clouds(points_list, scores_list, radius, num_keypoints=None)   list of int64 index tensors: the kept rows in rank order
  topk_keypoints_clouds(scores_list, num_keypoints)                            the stable ranking alone: the first num_keypoints ranks
  gather_keypoints(indices_list, *tensor_lists)                                the selected rows of points, features, scores
  random_sample_keypoints / sample_keypoints_with_scores / random_sample_keypoints_with_scores / sample_keypoints_with_nms /
  random_sample_keypoints_with_nms                                             the reference's names and signatures: one cloud, numpy in and out

The batched calls take GPU tensors only (there is no CPU path), any number of clouds per call, and chunk internally at the library's
SE3_PAIR_MAX_PAIRS clouds per launch sequence: per chunk one segmented stable sort, the grid's four launches, the rank inverse and the
selection, and ONE host synchronisation (the counts, the status word and the NaN-score flags in a single copy).

Contract (csrc/keypoint_nms.hip carries the same text).
  Rank.  The total order is score descending, then cloud-local index ascending: equal scores keep the lower index first, -0.0 equals 0.0,
    infinities order as numbers, a NaN score refuses the cloud.  The reference's np.argsort(scores)[::-1] leaves ties unspecified; the
    rule is the project's, as in ransac.select_correspondences.
  Suppression.  In rank order a point is kept iff no already kept point lies at d^2 < r^2, d^2 = (dx dx + dy dy) + dz dz in float64,
    unfused; float32 points are promoted on load; r^2 = r r in float64.  The test is strict: a pair at exactly r does not suppress, a
    duplicate of a kept point does.
  Output.  The kept points' cloud-local indices in rank order, int64.  With num_keypoints = K the first K of that list (the reference's
    early break), fewer if fewer survive; K = None: the whole list.  n = 0 gives an empty list.
  Refusals.  A non-finite point or a NaN score raises ValueError naming the cloud; radius must be positive and finite, num_keypoints,
    where given, >= 1.
  Determinism.  No atomics in the selection: a cloud's list is identical alone, anywhere in a batch, and from run to run.
  Cost.  One workgroup per cloud walks the ranks in tiles of 256; the dependency depth is the tile count whatever the input.  A radius
    far above the point spacing makes every ball walk long; in the extreme one ball holds the cloud and the walks are quadratic on one
    workgroup: correct but slow.  Choose the radius for the point spacing.  A single large cloud leaves most of the device idle.

The drop-ins reproduce the reference's guard literally: with num_points <= num_keypoints the input comes back untouched, unsorted and
without NMS.  The three random forms draw with np.random.choice on the host from numpy's global stream, as the reference does."""
import numpy as np
import torch

from . import ops as _ops
from .stacking import chunks, device_of, exclusive_offsets, gpu_rows_each, identities, lengths, stack, to_device, upload

_FAMILY = 'keypoint selection'
_STATUS = {1: 'a point is not finite', 2: 'the ranking is not a permutation of the rows'}
_FLOATS = (torch.float32, torch.float64)


def _scores_each(scores_list, dev, what):
    """Every entry a contiguous (n,) float32 or float64 GPU tensor, or RuntimeError (the strict contract of stacking.gpu_rows)."""
    out = []
    for i, s in enumerate(scores_list):
        name = '%s: scores %d' % (what, i)
        if not torch.is_tensor(s):
            raise RuntimeError('%s must be a tensor on the device (the numpy wrappers upload)' % name)
        if not s.is_cuda:
            raise RuntimeError('%s must be a GPU tensor (%s has no CPU implementation)' % (name, _FAMILY))
        if (dev is not None and dev.index is not None and s.device != dev) or s.dtype not in _FLOATS or s.dim() != 1:
            raise RuntimeError('%s must be (n,) float32 or float64 on %s, got %s %s on %s' % (name, dev or 'the GPU', tuple(s.shape), s.dtype,
                                                                                           s.device))
        out.append(s.contiguous())
    return out


def _rank_chunk(scores, sizes, dev):
    """One segmented stable ranking of a chunk's clouds.  Returns (order (total,) int64 cloud-local rank -> index, nan (clouds,) int32:
    the number of NaN scores per cloud)."""
    s = stack(scores, torch.empty((0,), dtype=torch.float32, device=dev)) + 0.0         # (-0.0 + 0.0 = 0.0)
    C = len(sizes)
    cloud = torch.repeat_interleave(torch.arange(C, device=dev), to_device(sizes, torch.int64, dev), output_size=sum(sizes))
    starts = to_device(exclusive_offsets(sizes)[:-1], torch.int64, dev)
    by_score = torch.sort(s, descending=True, stable=True).indices                      # equal scores: the lower stacked row first
    order = by_score[torch.sort(cloud[by_score], stable=True).indices]                  # ... and cloud by cloud, the score order kept
    nan = torch.zeros((C,), dtype=torch.int32, device=dev).index_add_(0, cloud, torch.isnan(s).to(torch.int32))
    return (order - starts[cloud]).contiguous(), nan


def _keep(num_keypoints, what):
    if num_keypoints is None:
        return 0
    if int(num_keypoints) != num_keypoints or int(num_keypoints) < 1:
        raise ValueError('%s: num_keypoints %r is not an integer >= 1' % (what, num_keypoints))
    return int(num_keypoints)


def _refuse_nan(what, a, nan):
    bad = [a + c for c, v in enumerate(nan) if v]
    if bad:
        raise ValueError('%s: cloud %s: a score is NaN' % (what, ', '.join(str(c) for c in bad)))


@torch.no_grad()
def nms_keypoints_clouds(points_list, scores_list, radius, num_keypoints=None, device=None):
    """Greedy radius NMS in score order for a list of clouds: points (n, 3) and scores (n,), float32 or float64 GPU tensors.  Returns the
    list of (m_c,) int64 index tensors on the device: cloud c's kept rows in rank order, at most num_keypoints of them (None: all
    survivors).  One host synchronisation per chunk of 32 clouds.  A radius far above the point spacing is correct but slow (see the
    module text)."""
    what = 'nms_keypoints_clouds'
    if len(points_list) != len(scores_list):
        raise ValueError('%s: one scores tensor per cloud: %d for %d clouds' % (what, len(scores_list), len(points_list)))
    r = float(radius)
    if not (np.isfinite(r) and r > 0):
        raise ValueError('%s: radius %r is not a positive finite number' % (what, radius))
    K = _keep(num_keypoints, what)
    dev = device_of(device, points_list, scores_list)
    pts = gpu_rows_each(points_list, dev, what + ': cloud', _FAMILY)
    scs = _scores_each(scores_list, dev, what)
    if pts:
        dev = pts[0].device
    for c, (p, s) in enumerate(zip(pts, scs)):
        if s.shape[0] != p.shape[0] or s.device != p.device:
            raise ValueError('%s: cloud %d: %d scores on %s for %d points on %s' % (what, c, s.shape[0], s.device, p.shape[0], p.device))
    out = []
    for a, b in chunks(len(pts)):
        p, pl = stack(pts[a:b]), lengths(pts[a:b])
        order, nan = _rank_chunk(scs[a:b], pl, dev)
        grid = _ops.pair_grid_build(p, pl, identities(b - a), r)
        kept, words = _ops.keypoint_nms_stack(grid, order, pl, r, K)
        words = torch.cat([words, nan]).cpu().tolist()                  # the ONE synchronisation of the chunk: counts, status, NaN flags
        counts, status = words[:b - a], words[b - a]
        _refuse_nan(what, a, words[b - a + 1:])
        if status:                                                      # (a refused cloud's count is minus its status bits)
            raise ValueError('%s: ' % what + '; '.join(
                'cloud %d: %s' % (a + c, ', '.join(t for bit, t in _STATUS.items() if -n & bit)) for c, n in enumerate(counts) if n < 0))
        offsets = exclusive_offsets(pl)
        out += [kept[offsets[c]:offsets[c] + counts[c]] for c in range(b - a)]
    return out


@torch.no_grad()
def topk_keypoints_clouds(scores_list, num_keypoints, device=None):
    """The stable ranking alone: per cloud the indices of the min(num_keypoints, n) highest scores, score descending, the lower index first
    among equal scores (None: the whole ranking).  Scores: (n,) float32 or float64 GPU tensors.  Returns a list of int64 index tensors."""
    what = 'topk_keypoints_clouds'
    K = _keep(num_keypoints, what)
    dev = device_of(device, scores_list)
    scs = _scores_each(scores_list, dev, what)
    if scs:
        dev = scs[0].device
    out = []
    for a, b in chunks(len(scs)):
        sl = lengths(scs[a:b])
        order, nan = _rank_chunk(scs[a:b], sl, dev)
        _refuse_nan(what, a, nan.cpu().tolist())
        out += [o[:K] if K else o for o in torch.split(order, sl)]
    return out


def gather_keypoints(indices_list, *tensor_lists):
    """The selected rows: for every tensor list (points, features, scores, ...) the list of t[indices] per cloud.  One list in, one list
    out; several in, a tuple of lists."""
    for lst in tensor_lists:
        if len(lst) != len(indices_list):
            raise ValueError('gather_keypoints: one tensor per cloud: %d for %d index lists' % (len(lst), len(indices_list)))
    res = tuple([t[i] for t, i in zip(lst, indices_list)] for lst in tensor_lists)
    return res[0] if len(res) == 1 else res


# ---- the reference's single-cloud functions: numpy in and out ---------------------------------------------------------------------------------
def _draw_probs(scores, what):
    """scores / np.sum(scores) in the scores' dtype, as the reference forms it; negative or non-finite scores are refused."""
    scores = np.asarray(scores)
    if not np.all(np.isfinite(scores)) or np.any(scores < 0):
        raise ValueError('%s: the scores of a weighted draw must be finite and non-negative' % what)
    return scores / np.sum(scores)


def random_sample_keypoints(points, feats, num_keypoints):
    """geotransformer.utils.pointcloud.random_sample_keypoints: a uniform draw from numpy's global stream."""
    num_points = points.shape[0]
    if num_points > num_keypoints:
        indices = np.random.choice(num_points, num_keypoints, replace=False)
        points, feats = points[indices], feats[indices]
    return points, feats


def sample_keypoints_with_scores(points, feats, scores, num_keypoints, device=None):
    """geotransformer.utils.pointcloud.sample_keypoints_with_scores: the num_keypoints highest scores, ranked on the device (equal scores:
    the lower index first)."""
    num_points = points.shape[0]
    if num_points > num_keypoints:
        indices = topk_keypoints_clouds([upload(np.asarray(scores).reshape(-1), device, cols=None)], num_keypoints)[0].cpu().numpy()
        points, feats = points[indices], feats[indices]
    return points, feats


def random_sample_keypoints_with_scores(points, feats, scores, num_keypoints):
    """geotransformer.utils.pointcloud.random_sample_keypoints_with_scores: a draw weighted by the scores from numpy's global stream."""
    num_points = points.shape[0]
    if num_points > num_keypoints:
        probs = _draw_probs(scores, 'random_sample_keypoints_with_scores')
        indices = np.random.choice(np.arange(num_points), num_keypoints, replace=False, p=probs)
        points, feats = points[indices], feats[indices]
    return points, feats


def sample_keypoints_with_nms(points, feats, scores, num_keypoints, radius, device=None):
    """geotransformer.utils.pointcloud.sample_keypoints_with_nms: the first num_keypoints survivors of the NMS in score order."""
    num_points = points.shape[0]
    if num_points > num_keypoints:
        indices = nms_keypoints_clouds([upload(points, device)], [upload(np.asarray(scores).reshape(-1), device, cols=None)], radius,
                                       num_keypoints)[0].cpu().numpy()
        points, feats = points[indices], feats[indices]
    return points, feats


def random_sample_keypoints_with_nms(points, feats, scores, num_keypoints, radius, device=None):
    """geotransformer.utils.pointcloud.random_sample_keypoints_with_nms: the full NMS on the device, then, with more than num_keypoints
    survivors, a draw over them weighted by their scores from numpy's global stream."""
    num_points = points.shape[0]
    if num_points > num_keypoints:
        s = upload(np.asarray(scores).reshape(-1), device, cols=None)
        kept = nms_keypoints_clouds([upload(points, device)], [s], radius)[0]
        both = torch.stack([kept.to(torch.float64), s[kept].to(torch.float64)]).cpu().numpy()      # indices and their scores: one copy
        indices = both[0].astype(np.int64)
        if len(indices) > num_keypoints:
            probs = _draw_probs(both[1].astype(np.asarray(scores).dtype), 'random_sample_keypoints_with_nms')
            indices = np.random.choice(indices, num_keypoints, replace=False, p=probs)
        points, feats = points[indices], feats[indices]
    return points, feats
