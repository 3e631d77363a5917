"""A float64 numpy restatement of the keypoint selection contract (se3et_amd/keypoints.py, csrc/keypoint_nms.hip), written from the contract
text alone: brute force in rank order, without tiles or a grid.

  rank_order(scores)                        score descending, then index ascending; -0.0 equals 0.0; a NaN raises ValueError
  nms(points, scores, radius, K=None)       the kept indices in rank order, int64
  nms_from_order(points, order, radius, K)  the same from a given rank -> index order
  topk(scores, K)                           the first K ranks"""
import numpy as np


def rank_order(scores):
    s = np.asarray(scores, dtype=np.float64).reshape(-1) + 0.0
    if np.isnan(s).any():
        raise ValueError('a score is NaN')
    return np.lexsort((np.arange(s.shape[0]), -s)).astype(np.int64)      # (the last key is the primary one)


def nms_from_order(points, order, radius, K=None):
    p = np.asarray(points).astype(np.float64).reshape(-1, 3)
    if not np.isfinite(p).all():
        raise ValueError('a point is not finite')
    r2 = float(radius) * float(radius)
    kept = []
    kept_points = np.empty((p.shape[0], 3))
    for i in np.asarray(order, dtype=np.int64):
        d = kept_points[:len(kept)] - p[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        if (d2 < r2).any():
            continue
        kept_points[len(kept)] = p[i]
        kept.append(int(i))
        if K is not None and len(kept) == K:
            break
    return np.asarray(kept, dtype=np.int64)


def nms(points, scores, radius, K=None):
    return nms_from_order(points, rank_order(scores), radius, K)


def topk(scores, K=None):
    order = rank_order(scores)
    return order if K is None else order[:K]
