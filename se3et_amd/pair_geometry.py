"""Ground truth of a registration pair on the device: nearest neighbour, overlap, correspondences and the gt.info record, as batched HIP
kernels (csrc/pair_geometry.hip, csrc/pair_grid.h) in place of the reference's scipy cKDTree passes on the host.

  nearest_neighbor_pairs(q_list, s_list, transforms=None, return_index=False)      get_nearest_neighbor per pair
  compute_overlap_pairs(ref_list, src_list, transforms, positive_radius)            (P,) float64
  get_correspondences_pairs(ref_list, src_list, transforms, matching_radius)        list of (n_p, 2) int64
  calibrate_ground_truth_pairs(ref_list, src_list, transforms, voxel_size, max_points, downsample)   overlaps (P,), covariances (P, 6, 6)
  modified_chamfer_distance_pairs(raw_list, ref_list, src_list, gt_transforms, transforms)   (P,) float64
  modified_chamfer_distance(raw_points, ref_points, src_points, gt_transform, transform, reduction)   the reference's metric on (B, N, 3)
  get_nearest_neighbor / compute_overlap / get_correspondences / calibrate_ground_truth   the reference's names and signatures: numpy in
                                                                                    and out, upload inside, one pair per call
  write_info_file(file_name, test_pairs)                                            the gt.info text format (benchmark.read_info_file reads it)

The batched calls take GPU tensors only (there is no CPU path), any number of pairs per call, and chunk internally at the library's
SE3_PAIR_MAX_PAIRS pairs per launch.  The query cloud of a pair is searched in the other cloud of the pair after the rigid transform.

Arithmetic contract (csrc/pair_geometry.hip carries the same text).  Everything is float64, as the reference computes it with numpy and
scipy on float64 arrays.  Inputs may be float32 or float64, on the device; they are promoted on load inside the kernels and not copied.
Transforms are (P, 4, 4) float64.
  - A transformed support point is fma(R[k][2], z, fma(R[k][1], y, R[k][0] * x)) + t[k], the expression benchmark.hip documents.
  - A distance is sqrt((dx*dx + dy*dy) + dz*dz).
  - Tests are d < r on d*d < r*r, strict: the ball query compares (dx*dx + dy*dy) + dz*dz with r*r and takes no root; the overlap and the
    gt.info selection compare the nearest-neighbour distances this library returned, squared again, with r*r.
  - This is not bit-for-bit the BLAS or k-d tree arithmetic of the reference.  Only a distance within float64 rounding of a threshold, or
    of another candidate's distance, can come out differently.
  nearest neighbour   for every query row the float64 distance to the nearest transformed support point of its own pair and that point's
      pair-local index (int64).  The search is exact; the grid is only an accelerator: the ring of cells widens until the best distance
      found is no larger than the distance to the unvisited shell, so a query far outside the support's bounding box terminates and is
      correct.  Among exactly equal distances the lowest index wins.  An empty support gives distance inf and index -1.
  overlap   count(d_nn < r) / n_ref as float64: the count is an integer and the division is done once, so it equals np.mean of the
      reference exactly; n_ref = 0 gives NaN, as np.mean of an empty array does.
  correspondences   all (i, j) with |ref_i - (R src_j + t)| < r; rows ascending in i, j ascending within a row (the order scipy's
      multi-point query_ball_point returns); int64 (n, 2), (0, 2) when there are none.  Two passes: count per row, exclusive scan, fill.
      The result does not depend on the arrival order of any atomic: a pair's rows are bit-identical whether the pair is alone or in any
      batch, and from run to run.
  gt.info record   the overlap at 5 voxel_size; the nearest-neighbour indices of the rows with d_nn < voxel_size in row order; with more
      than max_points (5000) of them the subset is drawn by the reference's one call on numpy's global generator,
      np.random.choice(nn_indices, max_points, replace=False), on the host (the pattern of SuperPointTargetGenerator: seeded runs equal the
      reference); the 6x6 covariance is sum G^T G over the selected transformed src points, G = [I3 | -[p]x] in the sign layout of
      threedmatch/utils.py:214-221, summed in a fixed order; no selected point gives the zero matrix.  The reference voxel-downsamples
      both clouds with Open3D at 0.01 first: downsample=0.01 does that on the device (se3et_amd.scan_prep.voxel_downsample_clouds, whose
      output order is its own, not Open3D's); the default None takes the clouds as given.
  modified chamfer distance   the reference's formula (modules/registration/metrics.py:8-44) in float64: per pair
      mean_i |T src_i - nn_raw(T src_i)| + mean_j |ref_j - nn_(T T_gt^-1 raw)(ref_j)|, both terms with the exact nearest neighbour above
      (no (N, M) distance matrix); T src is formed by a float64 matmul, T T_gt^-1 raw by the support transform above."""
import os

import numpy as np
import torch

from . import ops as _ops
from .stacking import chunks, device_of, gpu_rows_each, lengths, stack, transforms_of, upload

_FAMILY = 'pair ground truth'


def _chunks(q_list, s_list, transforms, device, what):
    """Validated clouds in chunks of at most ops.PAIR_MAX_PAIRS pairs: (first pair, q stacked, q lengths, s stacked, s lengths, T)."""
    if len(q_list) != len(s_list):
        raise ValueError('%s: one query and one support cloud per pair' % what)
    dev = device_of(device, q_list, s_list)
    qs = gpu_rows_each(q_list, dev, what + ': query cloud', _FAMILY)
    ss = gpu_rows_each(s_list, dev, what + ': support cloud', _FAMILY)
    T = transforms_of(transforms, len(qs), what, 'cpu', finite=True)
    for a, b in chunks(len(qs)):
        yield a, stack(qs[a:b]), lengths(qs[a:b]), stack(ss[a:b]), lengths(ss[a:b]), T[a:b]


@torch.no_grad()
def nearest_neighbor_pairs(q_list, s_list, transforms=None, return_index=False, device=None):
    """get_nearest_neighbor (geotransformer/utils/pointcloud.py:11-22) for P pairs: for every row of q_list[p] the distance to the nearest
    point of s_list[p] moved by transforms[p] (None: as given).  Returns a list of (n_p,) float64 distance tensors, and with return_index
    a second list of (n_p,) int64 indices into s_list[p]."""
    dists, idxs = [], []
    for _, q, ql, s, sl, T in _chunks(q_list, s_list, transforms, device, 'nearest_neighbor_pairs'):
        grid = _ops.pair_grid_build(s, sl, T, 0.0)
        d, i = _ops.pair_nearest_neighbor_stack(grid, q, ql)
        dists += list(torch.split(d, ql))
        idxs += list(torch.split(i, ql))
    return (dists, idxs) if return_index else dists


@torch.no_grad()
def compute_overlap_pairs(ref_list, src_list, transforms, positive_radius, device=None):
    """compute_overlap (utils/registration.py:149-155) for P pairs: the fraction of ref points whose nearest transformed src point is
    closer than positive_radius.  Returns (P,) float64 on the device."""
    out = []
    dev = device_of(device, ref_list, src_list)
    for _, q, ql, s, sl, T in _chunks(ref_list, src_list, transforms, device, 'compute_overlap_pairs'):
        grid = _ops.pair_grid_build(s, sl, T, 0.0)
        d, _i = _ops.pair_nearest_neighbor_stack(grid, q, ql)
        out.append(_ops.pair_overlap_stack(d, ql, positive_radius))
    return stack(out, torch.empty((0,), dtype=torch.float64, device=dev))


@torch.no_grad()
def get_correspondences_pairs(ref_list, src_list, transforms, matching_radius, device=None):
    """get_correspondences (utils/registration.py:161-173) for P pairs.  Returns a list of (n_p, 2) int64 device tensors [index in
    ref_list[p], index in src_list[p]], rows ascending in the ref index, then in the src index."""
    out = []
    for _, q, ql, s, sl, T in _chunks(ref_list, src_list, transforms, device, 'get_correspondences_pairs'):
        grid = _ops.pair_grid_build(s, sl, T, float(matching_radius))
        row_offsets = _ops.pair_ball_count_stack(grid, q, ql, matching_radius)
        ends = np.cumsum(ql)
        # one read-back per chunk: the pair boundaries of the correspondence list (the last is the total)
        bounds = row_offsets[torch.as_tensor(ends, dtype=torch.int64, device=q.device)].cpu().tolist()
        corr = _ops.pair_ball_fill_stack(grid, q, ql, matching_radius, row_offsets, bounds[-1])
        out += list(torch.split(corr, np.diff([0] + bounds).tolist()))
    return out


@torch.no_grad()
def calibrate_ground_truth_pairs(ref_list, src_list, transforms, voxel_size=0.006, max_points=5000, device=None, downsample=None):
    """calibrate_ground_truth (datasets/registration/threedmatch/utils.py:197-228) for P pairs.  downsample: None takes the clouds as
    given; a voxel size (the reference's 0.01) voxel-downsamples both clouds first (se3et_amd.scan_prep).  Returns (overlaps (P,) at
    5 voxel_size, covariances (P, 6, 6)) float64 on the device: the records of gt.info."""
    if downsample is not None:
        from .scan_prep import voxel_downsample_clouds
        ref_list = voxel_downsample_clouds(list(ref_list), downsample, device=device)
        src_list = voxel_downsample_clouds(list(src_list), downsample, device=device)
    overlaps, covs = [], []
    dev = device_of(device, ref_list, src_list)
    for _, q, ql, s, sl, T in _chunks(ref_list, src_list, transforms, device, 'calibrate_ground_truth_pairs'):
        grid = _ops.pair_grid_build(s, sl, T, 0.0)
        d, i = _ops.pair_nearest_neighbor_stack(grid, q, ql)
        overlaps.append(_ops.pair_overlap_stack(d, ql, 5 * voxel_size))
        close = d * d < voxel_size * voxel_size
        selected = []
        for dp, ip in zip(torch.split(close, ql), torch.split(i, ql)):
            sel = ip[dp]
            if sel.shape[0] > max_points:          # the reference's draw, on the host and on numpy's global generator
                sel = torch.from_numpy(np.random.choice(sel.cpu().numpy(), max_points, replace=False)).to(q.device)
            selected.append(sel)
        covs.append(_ops.pair_info_covariance_stack(s, sl, T, torch.cat(selected), lengths(selected)))
    return stack(overlaps, torch.empty((0,), dtype=torch.float64, device=dev)), \
        stack(covs, torch.empty((0, 6, 6), dtype=torch.float64, device=dev))


@torch.no_grad()
def modified_chamfer_distance_pairs(raw_list, ref_list, src_list, gt_transforms, transforms, device=None):
    """modified_chamfer_distance (modules/registration/metrics.py:8-44) for P pairs of (n, 3) GPU clouds: (P,) float64 on the device.  An
    empty src or ref cloud gives NaN (the mean of nothing), an empty raw cloud inf."""
    P = len(raw_list)
    if not (len(ref_list) == len(src_list) == P):
        raise ValueError('modified_chamfer_distance_pairs: one raw, ref and src cloud per pair')
    dev = device_of(device, raw_list, ref_list, src_list)
    T, G = (transforms_of(t, P, 'modified_chamfer_distance_pairs', 'cpu', finite=True) for t in (transforms, gt_transforms))
    srcs = gpu_rows_each(src_list, dev, 'modified_chamfer_distance_pairs: src cloud', _FAMILY)
    Td = T.to(dev)
    moved = [s.to(torch.float64) @ Td[p, :3, :3].T + Td[p, :3, 3] for p, s in enumerate(srcs)]
    composed = torch.matmul(T, torch.linalg.inv(G)) if P else T
    d_pq = nearest_neighbor_pairs(moved, raw_list, None, device=dev)
    d_qp = nearest_neighbor_pairs(ref_list, raw_list, composed, device=dev)
    if not P:
        return torch.zeros((0,), dtype=torch.float64, device=dev)
    return torch.stack([a.mean() + b.mean() for a, b in zip(d_pq, d_qp)])


def modified_chamfer_distance(raw_points, ref_points, src_points, gt_transform, transform, reduction='mean'):
    """The reference's signature: (B, N, 3) GPU tensors and (B, 4, 4) transforms; reduction 'mean', 'sum' or 'none'.  float64."""
    assert reduction in ['mean', 'sum', 'none']
    for name, t in (('raw_points', raw_points), ('ref_points', ref_points), ('src_points', src_points)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError('modified_chamfer_distance: %s must be a GPU tensor' % name)
        if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] != raw_points.shape[0]:
            raise RuntimeError('modified_chamfer_distance: %s must be (B, N, 3)' % name)
    out = modified_chamfer_distance_pairs(list(raw_points), list(ref_points), list(src_points), gt_transform, transform)
    return out.mean() if reduction == 'mean' else out.sum() if reduction == 'sum' else out


# ---- the reference's single-pair functions: numpy in and out -------------------------------------------------------------------------------
def get_nearest_neighbor(q_points, s_points, return_index=False, device=None):
    """geotransformer.utils.pointcloud.get_nearest_neighbor: distances (and indices) as numpy arrays."""
    d, i = nearest_neighbor_pairs([upload(q_points, device)], [upload(s_points, device)], None, True)
    return (d[0].cpu().numpy(), i[0].cpu().numpy()) if return_index else d[0].cpu().numpy()


def compute_overlap(ref_points, src_points, transform=None, positive_radius=0.1, device=None):
    """geotransformer.utils.registration.compute_overlap: a numpy float64."""
    ov = compute_overlap_pairs([upload(ref_points, device)], [upload(src_points, device)], None if transform is None else [transform],
                               positive_radius)
    return np.float64(ov.cpu().numpy()[0])


def get_correspondences(ref_points, src_points, transform, matching_radius, device=None):
    """geotransformer.utils.registration.get_correspondences: (n, 2) int64 numpy."""
    return get_correspondences_pairs([upload(ref_points, device)], [upload(src_points, device)], [transform], matching_radius)[0].cpu().numpy()


def calibrate_ground_truth(ref_points, src_points, transform, voxel_size=0.006, device=None, downsample=None):
    """threedmatch.utils.calibrate_ground_truth on point arrays (the reference takes Open3D clouds and voxel-downsamples them at 0.01
    first: downsample=0.01; None takes the clouds as given): (overlap, covariance (6, 6)) numpy float64."""
    ov, cov = calibrate_ground_truth_pairs([upload(ref_points, device)], [upload(src_points, device)], [transform], voxel_size,
                                           downsample=downsample)
    return np.float64(ov.cpu().numpy()[0]), cov[0].cpu().numpy()


def write_info_file(file_name, test_pairs):
    """Writes a gt.info: per record 'id0\\tid1\\tnum_fragments' and the covariance's 6 rows, each value as Python formats the float --
    the layout se3et_amd.benchmark.read_info_file (and the reference's) parses.  test_pairs: dicts with test_pair, num_fragments,
    covariance (6, 6)."""
    if os.path.dirname(file_name):
        os.makedirs(os.path.dirname(file_name), exist_ok=True)
    lines = []
    for rec in test_pairs:
        a, b = rec['test_pair']
        lines.append('{}\t{}\t{}\n'.format(a, b, rec['num_fragments']))
        cov = np.asarray(rec['covariance'].detach().cpu() if torch.is_tensor(rec['covariance']) else rec['covariance']).reshape(6, 6)
        for row in cov.tolist():
            lines.append('\t'.join('{}'.format(v) for v in row) + '\n')
    with open(file_name, 'w') as f:
        f.writelines(lines)
