"""ISS keypoints on the device: Open3D's compute_iss_keypoints (intrinsic shape signatures: the eigenvalue ratios of a point's
neighbourhood scatter matrix and a radius non-maximum test on the smallest eigenvalue), the weights-free detector of the classical
registration path, as batched HIP kernels (csrc/iss.hip, csrc/iss_core.h, csrc/cov3.h) on the searches of csrc/pair_grid.h.

  iss_keypoints_clouds(points_list, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5,
                       return_saliency=False)      list of int64 index tensors, ascending (and the list of (n,) float64 saliencies)
  model_resolution_clouds(points_list)             (clouds,) float64 on the device: mean distance to the nearest other point
  compute_iss_keypoints(points, ...)               one cloud, numpy in, (k, 3) float64 numpy out (Open3D's signature)

The batched calls take GPU tensors only (there is no CPU path): points (n, 3) float32 or float64, promoted on load; any number of clouds
per call, chunked at the library's SE3_PAIR_MAX_PAIRS clouds and, within a chunk, at PAIR_BUDGET ball-list entries (16 bytes each) per
launch sequence.  A chunk synchronises with the host once before its kernels run (the list's size and the status words in one copy; a
chunk above the budget adds one); the compaction of the mask to indices is a nonzero on the device and one small copy of the clouds'
cuts.  A radius of 0 needs the model resolution on the host before the lists can be sized: one more copy per chunk (the resolutions and
the status words together).  The kernels take a radius per cloud, so a chunk whose clouds default differently runs stacked all the same.

Contract (csrc/iss.hip carries the same text).  The structure is Open3D's ComputeISSKeypoints (geometry/keypoint/Keypoint.cpp); the
arithmetic is the project's: float64, contraction off, float32 points promoted on load, no libm call other than the square root and
division.
  Neighbourhood.  The members of a ball of radius r around row i are the points of the same cloud with d^2 < r r, d^2 = (dx dx + dy dy)
    + dz dz unfused, r r formed in float64; the test is strict.  The row itself is a member, a duplicate is a member.  m_i is the member
    count at salient_radius, c_i the member count at non_max_radius.
  Scatter matrix.  Over the m_i members in ascending cloud-local index: mean = (sequential sum) / m_i; the six entries of
    C_i = sum (p - mean)(p - mean)^T / m_i are each a sequential sum in the same order (kn_covariance: two passes).
  Eigenvalues.  Those of C_i by the cyclic Jacobi of csrc/cov3.h (the solver of the k-NN normals: kn_rotate, kJacobiSweeps sweeps over
    (0,1), (0,2), (1,2)), sorted l1 >= l2 >= l3.
  Saliency.  s_i = l3 when m_i >= min_neighbors, C_i is not the zero matrix, l2 / l1 < gamma_21, l3 / l2 < gamma_32 and l3 > 0 (true
    divisions; a comparison with NaN is false); otherwise s_i = 0.
  Selection.  Row i is a keypoint iff s_i > 0, c_i >= min_neighbors, and no member j of its non_max_radius ball has s_j > s_i.  Exactly
    equal saliencies keep both rows (Open3D's IsLocalMaxima).  The output is the keypoints' cloud-local indices, ascending, int64.
  Default radii.  A radius of 0 takes Open3D's default: salient_radius = 6 res, non_max_radius = 4 res, res the cloud's model resolution:
    (the sum over its rows of the root of the second column of a 2-nearest search) / n, summed in the fixed shape of csrc/fixed_sum.h
    (lane l of 256 adds rows l, l + 256, .. in ascending order, the 256 sums are folded in halves); n < 2 gives 0.  It is read back and
    passed to the kernels as host doubles; a resolution of 0 (n < 2, or nothing but duplicates) gives no keypoint.
  Refusals.  ValueError naming the cloud for a non-finite point (a device flag); ValueError for negative or non-finite radii, gammas that
    are not finite and positive, min_neighbors < 1.  n = 0 gives an empty list.
  Determinism.  No float atomics: a cloud's saliencies and keypoints are bit-identical alone, anywhere in a batch, and from run to run.
  Cost.  The saliency pass is linear in the ball lists: a salient radius far above the point spacing makes lists long (a ball that holds
    the cloud is quadratic, in time and in list memory, sliced at PAIR_BUDGET), and a row's wave walks its list serially, as the fixed
    order demands.  Open3D's default of 6 resolutions holds about a hundred members on a surface scan.

Where this departs from Open3D: the strict radius test, the two-pass covariance in a fixed order, the Jacobi eigenvalues in place of the
analytic solver.  None of them moves a value beyond rounding, or a decision except for a row within rounding of a gamma, of zero, or of a
neighbour's saliency."""
import numpy as np
import torch

from . import ops as _ops
from .fpfh import _radius_lists
from .stacking import chunks, device_of, gpu_rows_each, identities, lengths, mask_indices, stack, upload

_FAMILY = 'ISS'
PAIR_BUDGET = 1 << 23          # ball-list entries per launch sequence: 16 bytes each, 128 MiB
SALIENT_RESOLUTIONS, NON_MAX_RESOLUTIONS = 6.0, 4.0          # Open3D's default radii, in model resolutions


def _arguments(what, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors):
    rs, rn, g21, g32 = float(salient_radius), float(non_max_radius), float(gamma_21), float(gamma_32)
    for name, r in (('salient_radius', rs), ('non_max_radius', rn)):
        if not (np.isfinite(r) and r >= 0):
            raise ValueError('%s: %s %r is not a finite number >= 0 (0: the default from the model resolution)' % (what, name, r))
    for name, g in (('gamma_21', g21), ('gamma_32', g32)):
        if not (np.isfinite(g) and g > 0):
            raise ValueError('%s: %s %r is not a positive finite number' % (what, name, g))
    if int(min_neighbors) != min_neighbors or int(min_neighbors) < 1:
        raise ValueError('%s: min_neighbors %r is not an integer >= 1' % (what, min_neighbors))
    return rs, rn, g21, g32, int(min_neighbors)


def _resolution_stack(p, pl):
    """(clouds,) float64 on the device: the model resolutions of a chunk's stacked clouds."""
    grid = _ops.pair_grid_build(p, pl, identities(len(pl)), 0.0)
    return _ops.distance_stats_stack(_ops.knn_distance_stack(grid, p, pl, 2, 1), pl)[0][:, 3]


@torch.no_grad()
def model_resolution_clouds(points_list, device=None):
    """The model resolution of every cloud, (clouds,) float64 on the device: the mean over its rows of the distance to the nearest other
    point (a duplicate is at 0), 0 for a cloud of fewer than two points.  Nothing is read back."""
    dev = device_of(device, points_list)
    pts = gpu_rows_each(points_list, dev, 'model_resolution_clouds: cloud', _FAMILY)
    out = [_resolution_stack(stack(pts[a:b]), lengths(pts[a:b])) for a, b in chunks(len(pts))]
    return torch.cat(out) if out else torch.zeros((0,), dtype=torch.float64, device=dev)


def _chunk(p, pl, rs, rn, g21, g32, mn, words, what, a):
    """(saliencies, mask) of a chunk's stacked clouds; rs, rn: a salient and a non-max radius per cloud."""
    sal = torch.empty((p.shape[0],), dtype=torch.float64, device=p.device)
    slices, _ = _radius_lists(p, pl, rs, words, what, a, PAIR_BUDGET)
    for s, ro, pairs in slices():
        _ops.iss_saliency_stack(p, pl, ro, pairs, g21, g32, mn, sal, s)
    grid = _ops.pair_grid_build(p, pl, identities(len(pl)), max(rn, default=0.0))   # (the lists are done: the workspace is free again)
    return sal, _ops.iss_select_stack(grid, p, pl, rn, sal, mn)


@torch.no_grad()
def iss_keypoints_clouds(points_list, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5,
                         return_saliency=False, device=None):
    """ISS keypoints of a list of clouds: points (n, 3) float32 or float64 GPU tensors.  Returns the list of ascending int64 index
    tensors on the device, and with return_saliency the list of (n,) float64 saliencies.  A radius of 0 is Open3D's default, 6 and 4
    model resolutions of each cloud (see the module text)."""
    what = 'iss_keypoints_clouds'
    rs, rn, g21, g32, mn = _arguments(what, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)
    dev = device_of(device, points_list)
    pts = gpu_rows_each(points_list, dev, what + ': cloud', _FAMILY)
    keys, sals = [], []
    for a, b in chunks(len(pts)):
        p, pl = stack(pts[a:b]), lengths(pts[a:b])
        words = _ops.points_check_stack(p, pl)
        res = [0.0] * (b - a)
        if not (rs > 0 and rn > 0):
            host = torch.cat([_resolution_stack(p, pl), words.to(torch.float64)]).cpu().tolist()     # the resolutions and the status: one copy
            if host[-1]:
                raise ValueError('%s: ' % what + '; '.join('cloud %d: a point is not finite' % (a + c) for c, w in enumerate(host[b - a:-1]) if w))
            res, words = host[:b - a], torch.zeros_like(words)
        sal, mask = _chunk(p, pl, [rs if rs > 0 else SALIENT_RESOLUTIONS * x for x in res], [rn if rn > 0 else NON_MAX_RESOLUTIONS * x for x in res],
                           g21, g32, mn, words, what, a)
        keys += mask_indices(mask, pl)
        sals += list(torch.split(sal, pl))
    return (keys, sals) if return_saliency else keys


def compute_iss_keypoints(points, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, device=None):
    """One cloud, numpy in and out: the (k, 3) float64 keypoints in ascending row order (Open3D's compute_iss_keypoints returns the
    points, not their indices)."""
    _arguments('compute_iss_keypoints', salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)
    p = np.asarray(points).reshape(-1, 3)
    idx = iss_keypoints_clouds([upload(p, device)], salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)[0]
    return p[idx.cpu().numpy()].astype(np.float64)
