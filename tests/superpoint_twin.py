"""Plain twin of the selections on the superpoint level (csrc/partition.hip, the index half of csrc/geo_records.hip /
csrc/geo_embedding.hip, the scores of csrc/matching.hip): numpy in int64 / float64, no torch operation that selects.

The selection twins take LATTICE clouds only: coordinates k / 8 with integer 0 <= k < 128 (superpoint_edge_fixture.py).  A squared
distance is then an integer number of 1 / 64 units below 2^16, every intermediate of the reference's float32 expression
(x2 - 2 xy + y2, pairwise_distance.py:4-30; csrc/common.h: se3_ref_sq_dist) is a multiple of 1 / 64 far below 2^24 / 64 and therefore exact
whatever is fused, ties are real ties, and the contract of csrc/partition.hip -- ascending (distance, index) -- is integer arithmetic plus
a stable sort:

  knn3(points)                                 (N, 3): entries 1..3 of every row's (distance, index) order; rank 0 is dropped WHICHEVER point
                                               it is (a duplicate with a lower index comes before the point itself, which then stays in
                                               its own row); a cloud of fewer than 4 points fills the missing entries with the row's own index
  point_to_node_partition(points, nodes, K)    every point to its nearest node, lowest index among equals; per node its own points by
                                               (distance, index), cut to K, padded with N; K may exceed N
  *_stack                                      the same per cloud: global node indices, global point indices padded with the total
                                               (knn3_stack: indices local to the cloud)
  embedding_indices / embedding                float64 indices of the geometric embedding from a GIVEN knn, and the embedding through
                                               oracle.se3et_oracle.sinusoidal and the two linear layers in float64
  superpoint_scores                            float64 restatement of exp(-clamp(2 - 2 f_r . f_s, 0)) with the dual normalisation over
                                               the present nodes
"""
import numpy as np

LATTICE = 8                  # coordinates are k / LATTICE
LATTICE_SPAN = 128           # 0 <= k < LATTICE_SPAN


def lattice_units(points):
    """(n, 3) int64 k of a lattice cloud; raises when a coordinate is off the lattice."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    k = np.rint(p * LATTICE)
    if not ((k == p * LATTICE).all() and (k >= 0).all() and (k < LATTICE_SPAN).all()):
        raise ValueError('coordinates must be k / %d with integer 0 <= k < %d' % (LATTICE, LATTICE_SPAN))
    return k.astype(np.int64)


def sq_units(a, b):
    """(len(a), len(b)) int64 squared distances in units of 1 / LATTICE^2."""
    d = lattice_units(a)[:, None, :] - lattice_units(b)[None, :, :]
    return (d * d).sum(-1)


def ref_sq_dist_f32(x, y):
    """The reference's float32 expression (x2 - 2 xy) + y2 clamped at 0, one float32 operation at a time in the order of
    csrc/common.h: se3_ref_sq_norm / se3_ref_sq_dist (the products of the dot product unfused here, fused there: on the lattice both are exact)."""
    x, y = np.asarray(x, np.float32).reshape(-1, 3), np.asarray(y, np.float32).reshape(-1, 3)
    norm = lambda p: (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    dot = (x[:, None, 0] * y[None, :, 0] + x[:, None, 1] * y[None, :, 1]) + x[:, None, 2] * y[None, :, 2]
    out = (norm(x)[:, None] - np.float32(2) * dot) + norm(y)[None, :]
    assert out.dtype == np.float32
    return np.maximum(out, np.float32(0))


def _by_distance_then_index(d):
    """Indices of a 1-D integer distance array in ascending (distance, index) order."""
    return np.argsort(d, kind='stable')


def knn3(points):
    n = len(points)
    d = sq_units(points, points)
    out = np.repeat(np.arange(n, dtype=np.int64)[:, None], 3, 1)
    for i in range(n):
        kept = _by_distance_then_index(d[i])[1:4]
        out[i, :len(kept)] = kept
    return out


def knn3_stack(points, lengths):
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    assert starts[-1] == len(points)
    parts = [knn3(points[a:b]) for a, b in zip(starts[:-1], starts[1:])]
    return np.concatenate(parts) if parts else np.zeros((0, 3), np.int64)


def nearest_node(points, nodes):
    """(N,) int64: the nearest node of every point, the lowest index among equally near ones."""
    d = sq_units(nodes, points)                                           # (M, N)
    return np.array([_by_distance_then_index(d[:, i])[0] for i in range(d.shape[1])], dtype=np.int64)


def point_to_node_partition(points, nodes, limit):
    """-> point_to_node (N,) int64, node_masks (M,) bool, node_knn_indices (M, limit) int64 padded with N, node_knn_masks (M, limit) bool."""
    n, m = len(points), len(nodes)
    d = sq_units(nodes, points)
    p2n = nearest_node(points, nodes)
    masks = np.zeros(m, dtype=bool)
    masks[p2n] = True
    knn = np.full((m, limit), n, dtype=np.int64)
    for node in range(m):
        own = np.nonzero(p2n == node)[0]                                   # ascending index
        own = own[_by_distance_then_index(d[node, own])][:limit]
        knn[node, :len(own)] = own
    return p2n, masks, knn, knn < n


def point_to_node_partition_stack(points, nodes, point_lengths, node_lengths, limit):
    """The per-cloud partition with GLOBAL node indices and GLOBAL point indices, padded with the total point count."""
    p0 = np.concatenate([[0], np.cumsum(point_lengths)]).astype(np.int64)
    m0 = np.concatenate([[0], np.cumsum(node_lengths)]).astype(np.int64)
    assert p0[-1] == len(points) and m0[-1] == len(nodes) and len(point_lengths) == len(node_lengths)
    total = int(p0[-1])
    p2n, masks, knn, knn_masks = [], [], [], []
    for c in range(len(point_lengths)):
        a, b, k, km = point_to_node_partition(points[p0[c]:p0[c + 1]], nodes[m0[c]:m0[c + 1]], limit)
        p2n.append(a + m0[c])
        masks.append(b)
        knn.append(np.where(km, k + p0[c], total))
        knn_masks.append(km)
    return np.concatenate(p2n), np.concatenate(masks), np.concatenate(knn), np.concatenate(knn_masks)


def embedding_indices(points, knn, sigma_d, sigma_a):
    """float64 d_idx (N, N) = |p_m - p_n| / sigma_d and a_idx (N, N, 3) = atan2(|ref x anc|, ref . anc) * 180 / (sigma_a pi) with
    ref_k = p_knn(n, k) - p_n, anc = p_m - p_n and atan2(0, 0) = 0."""
    p = np.asarray(points, np.float64)
    knn = np.asarray(knn, np.int64)
    anc = p[None, :, :] - p[:, None, :]                                    # (N, N, 3)
    d_idx = np.sqrt((anc * anc).sum(-1)) / sigma_d
    ref = p[knn] - p[:, None, :]                                           # (N, 3, 3)
    ref, anc = np.broadcast_arrays(ref[:, None, :, :], anc[:, :, None, :])
    sin_v = np.sqrt((np.cross(ref, anc) ** 2).sum(-1))
    cos_v = (ref * anc).sum(-1) + 0.0                                      # (-0 + 0 = +0: atan2(0, 0) = 0, never pi)
    return d_idx, np.arctan2(sin_v, cos_v) * (180.0 / (sigma_a * np.pi))


def embedding(points, knn, sigma_d, sigma_a, div_term, w_d, b_d, w_a, b_a):
    """float64 geometric embedding (N, N, C) torch tensor: W_d emb(d_idx) + b_d + max_k (W_a emb(a_idx_k) + b_a)."""
    import torch
    import torch.nn.functional as F
    from oracle import se3et_oracle as O
    d_idx, a_idx = [torch.from_numpy(np.ascontiguousarray(t)) for t in embedding_indices(points, knn, sigma_d, sigma_a)]
    div, w_d, b_d, w_a, b_a = [torch.as_tensor(t).double() for t in (div_term, w_d, b_d, w_a, b_a)]
    return F.linear(O.sinusoidal(d_idx, div), w_d, b_d) + F.linear(O.sinusoidal(a_idx, div), w_a, b_a).amax(2)


def superpoint_scores(ref, src, ref_mask=None, src_mask=None, dual=True):
    """float64 (N, M): exp(-clamp(2 - 2 f_r . f_s, 0)) of unit features, dually normalised over the PRESENT rows and columns; an entry
    whose row or column is absent is -1 (the stack kernel's marker)."""
    r, s = np.asarray(ref, np.float64), np.asarray(src, np.float64)
    rm = np.ones(len(r), bool) if ref_mask is None else np.asarray(ref_mask, bool)
    sm = np.ones(len(s), bool) if src_mask is None else np.asarray(src_mask, bool)
    e = np.exp(-np.maximum(2.0 - 2.0 * (r @ s.T), 0.0))
    e = np.where(rm[:, None] & sm[None, :], e, 0.0)
    if dual:
        with np.errstate(invalid='ignore', divide='ignore'):
            e = (e / e.sum(1, keepdims=True)) * (e / e.sum(0, keepdims=True))
    return np.where(rm[:, None] & sm[None, :], e, -1.0)
