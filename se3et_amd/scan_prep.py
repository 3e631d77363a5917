"""Scan preparation on the device: Open3D's voxel downsampling and k-NN normal estimation (geotransformer/utils/open3d.py:49-65) and
regularize_normals (utils/pointcloud.py:25-37), as batched HIP kernels (csrc/voxel_downsample.hip, csrc/knn_normals.hip on the grid of
csrc/pair_grid.h) in place of Open3D's host passes.

  voxel_downsample_clouds(points_list, voxel_size, normals_list=None)   list of (m, 3) float64 (and the list of normal means)
  knn_clouds(support_list, k, queries_list=None)                        lists of (n, k) int64 indices and (n, k) float64 squared distances
  estimate_normals_clouds(points_list, knn=33, viewpoints=None)         list of (n, 3) float64
  regularize_normals(points, normals, positive=True)                    tensor or numpy
  remove_statistical_outlier_clouds(points_list, nb_neighbors=20, std_ratio=2.0, return_stats=False)   list of kept-row index tensors, ascending
  remove_radius_outlier_clouds(points_list, nb_points, radius)          the same
  voxel_downsample / estimate_normals                                   the reference's names and signatures: one cloud, numpy in and out
  remove_statistical_outlier / remove_radius_outlier                    Open3D's names: one cloud, numpy in, (points, indices) out

The batched calls take GPU tensors only (there is no CPU path), any number of clouds per call, and chunk internally at the library's
SE3_PAIR_MAX_PAIRS clouds per launch; voxel_downsample_clouds synchronises with the host once per chunk (the output counts and the status
word in one copy).  The modified chamfer distance of the same family is se3et_amd.pair_geometry.modified_chamfer_distance.

Contract (the kernel files carry the same text).

Voxel downsampling of a cloud (points (n, 3) float32 or float64, optional normals (n, 3), voxel_size > 0).  Everything is float64; float32
inputs are promoted on load.
  - Origin: o_d = min_d - 0.5 voxel_size.  Voxel index: i_d = floor((p_d - o_d) / voxel_size), a true division, not a reciprocal multiply.
  - A cloud is refused with a clear error when an axis would need 2^21 voxels or more ((max_d - o_d) / voxel_size >= 2^21), when
    voxel_size is not a positive finite number, or when a point is non-finite (a device flag, read in the same host synchronisation that
    fetches the output counts).
  - Output row of a voxel: the float64 mean of its members; each coordinate is summed sequentially in ascending input index, then divided
    once by the count.  Normals: the same mean of the members' normals, NOT renormalised; a caller who wants unit normals normalises.
  - Output order: voxels ascend in the input index of their first member (Open3D's order is its unordered_map's and is unspecified).
  - n = 0 gives an empty output.  No float atomics: a cloud's output is bit-identical alone or anywhere in a batch, and from run to run.
  - Cost: a voxel of up to 64 members is ordered and summed by one thread (typical voxels hold 1-15 points); a larger one is ordered by
    a workgroup (quadratic in its members, shared by 256 threads) and then summed by one thread, as the fixed order demands.  A voxel
    size that puts a big cloud into a handful of voxels is correct but slow; choose the voxel size for the scan, not for the scene.

k nearest neighbours (k in [1, 64]).  For every query row the min(k, n_support) support points of its own cloud with the smallest
d^2 = (dx dx + dy dy) + dz dz, float64 and unfused; rows sorted ascending by (d^2, index): among equal distances the lower index comes
first and wins the last slot.  A cloud searched in itself returns each point as its own first neighbour (as Open3D's search does);
duplicates are ordered by index.  Missing columns hold index -1 and distance +inf.  The search is exact; the grid is only an accelerator:
the rings of cells widen until the k-th best d^2 is no larger than the bound of everything outside them.

Normals (knn = 33 by default).  Over the row's m = min(knn, n) neighbours in list order: mean = (sequential sum) / m; the six entries of
C = sum (p - mean)(p - mean)^T / m are each a sequential sum in list order, contraction off.  The normal is a unit eigenvector of C for its
smallest eigenvalue, in float64, with the canonical sign: z > 0, or z == 0 and y > 0, or z == y == 0 and x > 0.  It is exactly (0, 0, 1)
when m < 3 or C is the zero matrix (Open3D's fallback).  With viewpoints each normal is then oriented so that n . (viewpoint - p) >= 0.
Statistical outlier removal (csrc/outliers.hip carries the same text), Open3D's RemoveStatisticalOutliers including its quirks; float64,
contraction off, float32 points promoted on load.
  Per-row mean distance.  m = min(nb_neighbors, n); the row's list is knn_clouds' (the m nearest INCLUDING the row itself at d = 0,
    (d^2, index) ascending); a_i = (the sequential sum in list order of the roots of d2_t) / m.
  Cloud mean.  mean = (sum of a_i over the rows with a_i > 0) / n.
  Standard deviation.  std = sqrt((sum over the same rows of (a_i - mean)^2) / (n - 1)).
  Threshold and test.  thr = mean + std_ratio std (the product rounded, then the sum).  A row is kept iff a_i > 0 and a_i < thr.
  Summation.  Both cloud sums have the shape of csrc/fixed_sum.h: lane l of 256 adds its rows l, l + 256, .. in ascending order from 0.0
    (a row with a_i <= 0 adds nothing), then sh[l] = sh[l] + sh[l + o] for o = 128, 64, .., 1; the sum is sh[0].
  Small clouds.  n < 2 keeps nothing: n = 1 has a_0 = 0; the statistics of n = 0 and the std of n = 1 are NaN, as the formulas give.
  Arguments.  nb_neighbors in [1, SE3_KNN_MAX = 64], std_ratio positive and finite; anything else is a ValueError.  A non-finite point is
    a ValueError naming the cloud (a device flag, read with the clouds' cuts after the kernels).
  Determinism.  No float atomics: a cloud's values are bit-identical alone, anywhere in a batch, and from run to run.
Radius outlier removal: a row is kept iff the member count of its radius ball (d^2 < r r strict, r r in float64, the row itself and
duplicates included) is > nb_points: Open3D's strict test on the project's strict ball; pair_grid_build and pair_ball_count_stack, exact
integer work, no kernel of its own.  radius positive and finite, nb_points an integer >= 0.
Both filters return indices; the compaction of the mask is a nonzero on the device and one small copy of the clouds' cuts per chunk.

regularize_normals reproduces utils/pointcloud.py:25-37 literally: dot = -sum p n, direction = dot > 0 strict, so a row with dot == 0 is
flipped for positive=True.
This is not Open3D's arithmetic (single-pass cumulants and an analytic 3x3 solver; here two passes and a cyclic Jacobi iteration): only a
row whose two smallest eigenvalues are within rounding of each other, or which has a distance tie at the k-th place, can differ beyond
rounding."""
import numpy as np
import torch

from . import ops as _ops
from .stacking import chunks, device_of, gpu_rows_each, identities, lengths, mask_indices, stack, upload

_FAMILY = 'scan preparation'
_STATUS = {1: 'a point (or normal) is not finite', 2: 'an axis would need 2^21 voxels or more at this voxel size'}


@torch.no_grad()
def voxel_downsample_clouds(points_list, voxel_size, normals_list=None, device=None):
    """utils/open3d.py:57-65 voxel_downsample for a list of clouds.  Returns the list of (m_c, 3) float64 voxel means, and with normals_list
    a second list of the normals' means.  One host synchronisation per chunk of 32 clouds."""
    v = float(voxel_size)
    if not (np.isfinite(v) and v > 0):
        raise ValueError('voxel_downsample_clouds: voxel size %r is not a positive finite number' % (voxel_size,))
    if normals_list is not None and len(normals_list) != len(points_list):
        raise ValueError('voxel_downsample_clouds: one normals array per cloud')
    dev = device_of(device, points_list)
    pts = gpu_rows_each(points_list, dev, 'voxel_downsample_clouds: cloud', _FAMILY)
    nrs = gpu_rows_each(normals_list, dev, 'voxel_downsample_clouds: normals: cloud', _FAMILY) if normals_list is not None else None
    out_p, out_n = [], []
    for a, b in chunks(len(pts)):
        p, pl = stack(pts[a:b]), lengths(pts[a:b])
        nr = None
        if nrs is not None:
            if any(x.shape != y.shape for x, y in zip(pts[a:b], nrs[a:b])):
                raise ValueError('voxel_downsample_clouds: normals must have the shape of their points')
            nr = torch.cat([x.to(p.dtype) for x in nrs[a:b]], 0)
        means, nmeans, words = _ops.voxel_downsample_stack(p, pl, v, nr)
        words = words.cpu().tolist()                                   # the ONE synchronisation of the chunk: counts and status
        counts = words[:-1]
        if words[-1]:                                                  # (a refused cloud's count is minus its status bits)
            raise ValueError('voxel_downsample_clouds: ' + '; '.join(
                'cloud %d: %s' % (a + c, ', '.join(t for bit, t in _STATUS.items() if -n & bit)) for c, n in enumerate(counts) if n < 0))
        out_p += list(torch.split(means[:sum(counts)], counts))
        if nr is not None:
            out_n += list(torch.split(nmeans[:sum(counts)], counts))
    return (out_p, out_n) if normals_list is not None else out_p


@torch.no_grad()
def knn_clouds(support_list, k, queries_list=None, device=None):
    """The k nearest support points of every query row (queries_list None: every cloud searched in itself).  Returns (list of (n, k) int64
    indices, list of (n, k) float64 squared distances)."""
    if queries_list is not None and len(queries_list) != len(support_list):
        raise ValueError('knn_clouds: one query cloud per support cloud')
    dev = device_of(device, support_list, queries_list or [])
    ss = gpu_rows_each(support_list, dev, 'knn_clouds: cloud', _FAMILY)
    qs = gpu_rows_each(queries_list, dev, 'knn_clouds: queries: cloud', _FAMILY) if queries_list is not None else ss
    idxs, d2s = [], []
    for a, b in chunks(len(ss)):
        s, sl = stack(ss[a:b]), lengths(ss[a:b])
        q, ql = (s, sl) if queries_list is None else (stack(qs[a:b]), lengths(qs[a:b]))
        grid = _ops.pair_grid_build(s, sl, identities(b - a), 0.0)
        idx, d2 = _ops.knn_stack(grid, q, ql, k)
        idxs += list(torch.split(idx, ql))
        d2s += list(torch.split(d2, ql))
    return idxs, d2s


@torch.no_grad()
def estimate_normals_clouds(points_list, knn=33, viewpoints=None, device=None):
    """utils/open3d.py:49-54 estimate_normals for a list of clouds: (n, 3) float64 unit normals with the canonical sign, or, with
    viewpoints ((clouds, 3), or one (3,) for all), oriented towards them."""
    dev = device_of(device, points_list)
    pts = gpu_rows_each(points_list, dev, 'estimate_normals_clouds: cloud', _FAMILY)
    view = None
    if viewpoints is not None:
        view = torch.as_tensor(np.asarray(viewpoints.detach().cpu() if torch.is_tensor(viewpoints) else viewpoints, np.float64))
        view = view.reshape(-1, 3).expand(len(pts), 3) if view.numel() == 3 else view.reshape(-1, 3)
        if view.shape[0] != len(pts) or not bool(torch.isfinite(view).all()):
            raise ValueError('estimate_normals_clouds: one finite (3,) viewpoint per cloud')
    out = []
    for a, b in chunks(len(pts)):
        p, pl = stack(pts[a:b]), lengths(pts[a:b])
        grid = _ops.pair_grid_build(p, pl, identities(b - a), 0.0)
        out += list(torch.split(_ops.knn_normals_stack(grid, p, pl, knn, None if view is None else view[a:b]), pl))
    return out


def _refuse_points(what, a, words):
    if words[-1]:
        raise ValueError('%s: ' % what + '; '.join('cloud %d: a point is not finite' % (a + c) for c, w in enumerate(words[:-1]) if w))


@torch.no_grad()
def remove_statistical_outlier_clouds(points_list, nb_neighbors=20, std_ratio=2.0, return_stats=False, device=None):
    """Open3D's remove_statistical_outlier for a list of clouds.  Returns the list of kept-row index tensors (int64, ascending, on the
    device), and with return_stats a (clouds, 3) float64 tensor of mean, std and thr."""
    what = 'remove_statistical_outlier_clouds'
    if int(nb_neighbors) != nb_neighbors or not 1 <= int(nb_neighbors) <= _ops.KNN_MAX:
        raise ValueError("%s: nb_neighbors %r is not an integer in [1, SE3_KNN_MAX = %d]" % (what, nb_neighbors, _ops.KNN_MAX))
    ratio = float(std_ratio)
    if not (np.isfinite(ratio) and ratio > 0):
        raise ValueError('%s: std_ratio %r is not a positive finite number' % (what, std_ratio))
    dev = device_of(device, points_list)
    pts = gpu_rows_each(points_list, dev, what + ': cloud', _FAMILY)
    kept, stats = [], []
    for a, b in chunks(len(pts)):
        p, pl = stack(pts[a:b]), lengths(pts[a:b])
        words = _ops.points_check_stack(p, pl)
        grid = _ops.pair_grid_build(p, pl, identities(b - a), 0.0)
        st, mask = _ops.distance_stats_stack(_ops.knn_distance_stack(grid, p, pl, int(nb_neighbors), -1), pl, ratio)
        kept += mask_indices(mask, pl)
        _refuse_points(what, a, words.cpu().tolist())
        stats.append(st[:, :3])
    if not return_stats:
        return kept
    return kept, torch.cat(stats) if stats else torch.zeros((0, 3), dtype=torch.float64, device=dev)


@torch.no_grad()
def remove_radius_outlier_clouds(points_list, nb_points, radius, device=None):
    """Open3D's remove_radius_outlier for a list of clouds: the rows whose radius ball holds more than nb_points members, itself
    included.  Returns the list of kept-row index tensors (int64, ascending, on the device)."""
    what = 'remove_radius_outlier_clouds'
    if int(nb_points) != nb_points or int(nb_points) < 0:
        raise ValueError('%s: nb_points %r is not an integer >= 0' % (what, nb_points))
    r = float(radius)
    if not (np.isfinite(r) and r > 0):
        raise ValueError('%s: radius %r is not a positive finite number' % (what, radius))
    dev = device_of(device, points_list)
    pts = gpu_rows_each(points_list, dev, what + ': cloud', _FAMILY)
    kept = []
    for a, b in chunks(len(pts)):
        p, pl = stack(pts[a:b]), lengths(pts[a:b])
        words = _ops.points_check_stack(p, pl)
        grid = _ops.pair_grid_build(p, pl, identities(b - a), r)
        ro = _ops.pair_ball_count_stack(grid, p, pl, r)
        kept += mask_indices(ro[1:] - ro[:-1] > int(nb_points), pl)
        _refuse_points(what, a, words.cpu().tolist())
    return kept


def regularize_normals(points, normals, positive=True):
    """utils/pointcloud.py:25-37, literally, on tensors or numpy arrays: dot = -sum p n, direction = dot > 0 (strict: a row with dot == 0
    is flipped for positive=True)."""
    if torch.is_tensor(normals):
        direction = (-(points * normals).sum(dim=1, keepdim=True) > 0).to(normals.dtype)
    else:
        direction = -(points * normals).sum(axis=1, keepdims=True) > 0
    if positive:
        return normals * direction - normals * (1 - direction)
    return normals * (1 - direction) - normals * direction


# ---- the reference's single-cloud functions: numpy in and out ---------------------------------------------------------------------------------
def voxel_downsample(points, voxel_size, normals=None, device=None):
    """geotransformer.utils.open3d.voxel_downsample: points (and normals) as float64 numpy arrays."""
    if normals is None:
        return voxel_downsample_clouds([upload(points, device)], voxel_size)[0].cpu().numpy()
    p, n = voxel_downsample_clouds([upload(points, device)], voxel_size, [upload(normals, device)])
    return p[0].cpu().numpy(), n[0].cpu().numpy()


def estimate_normals(points, knn=33, device=None):
    """geotransformer.utils.open3d.estimate_normals: (n, 3) float64 numpy."""
    return estimate_normals_clouds([upload(points, device)], knn)[0].cpu().numpy()


def remove_statistical_outlier(points, nb_neighbors=20, std_ratio=2.0, device=None):
    """Open3D's remove_statistical_outlier on one cloud: (the kept points (k, 3), their row indices (k,) int64), numpy."""
    p = np.asarray(points).reshape(-1, 3)
    idx = remove_statistical_outlier_clouds([upload(p, device)], nb_neighbors, std_ratio)[0].cpu().numpy()
    return p[idx], idx


def remove_radius_outlier(points, nb_points, radius, device=None):
    """Open3D's remove_radius_outlier on one cloud: (the kept points (k, 3), their row indices (k,) int64), numpy."""
    p = np.asarray(points).reshape(-1, 3)
    idx = remove_radius_outlier_clouds([upload(p, device)], nb_points, radius)[0].cpu().numpy()
    return p[idx], idx
