"""ICP refinement on the device for batched pairs: Open3D's registration_icp, point-to-point or point-to-plane, as HIP kernels that stay
resident for all pairs of a call (csrc/icp.hip, csrc/icp_core.h) in place of a k-d tree loop on the host.

  icp_pairs(src_list, ref_list, init_transforms, max_correspondence_distance, estimation, ...)   dict of device tensors for P pairs
  registration_icp(src_points, ref_points, init, max_correspondence_distance, estimation, ...)    one pair, numpy in, (4, 4) numpy out
  refine_pairs(outs, transforms, max_correspondence_distance, estimation, level)                   the output dicts of batched.forward_pairs
                                                                                                   and (B, 4, 4) transforms -> refined ones

GPU tensors only (there is no CPU path), any number of pairs per call, chunked at the library's SE3_PAIR_MAX_PAIRS pairs per launch
sequence.  Per chunk the reference-side grid is built once, every evaluation and update is enqueued without a host synchronisation, and
the initial transforms are read on the device (the output of LGR or RANSAC needs no read-back).

Contract (csrc/icp.hip carries the same text).  Pair p has a source cloud, a reference cloud and an initial transform T0_p with
ref ~ T src.  Arithmetic is float64; points and normals may be float32 or float64 and are promoted on load.
  Evaluation under T.  Every source row is moved by fma(R[k][2], z, fma(R[k][1], y, R[k][0] * x)) + t[k]; its exact nearest reference
    point q is taken, the lowest index among equal distances; d^2 = (dx dx + dy dy) + dz dz, unfused.  The row is a correspondence iff
    d^2 < r^2 with r = max_correspondence_distance (strict).  fitness = n_corr / n_src (0 for an empty source);
    inlier_rmse = sqrt(sum d^2 / n_corr), 0 without a correspondence.
  Loop (Open3D's defaults: relative_fitness = relative_rmse = 1e-6, max_iteration = 30).  E_0 = evaluate(T0).  For k = 1 ..
    max_iteration: T_k = U_k T_(k-1) with U_k estimated from the correspondences of E_(k-1); E_k = evaluate(T_k); the pair stops with
    converged = 1 when |fitness_k - fitness_(k-1)| < relative_fitness and |rmse_k - rmse_(k-1)| < relative_rmse.  iterations = the k of
    the last evaluation; max_iteration = 0 evaluates only.  The accumulated T_k is always applied to the ORIGINAL source (Open3D moves
    its copy of the cloud by each U_k in turn: a difference of rounding only).
  Point-to-point.  Kabsch without scale over the correspondences (p = T src_i, q): centroids, the 3x3 cross-covariance about the
    centroids, the rotation from the library's 3x3 solve, t = qc - R pc.
  Point-to-plane.  Residual r_i = (p - q) . n with n the reference normal of q; J_i = [p x n, n]; (sum J^T J) x = -sum J^T r by a 6x6
    Cholesky factorisation; U = [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5] (Open3D's TransformVector6dToMatrix4d), with one shared series for sin
    and cos on the host and on the device.  A step with an |angle| >= 1 rad sets the step_refused bit and ends the pair at its previous
    transform, converged = 0: a linearised step of that size is not a refinement (Open3D applies it).
  Degenerate cases.  The update is the identity -- and the pair ends at the next comparison, its result being unchanged -- with fewer
    than 3 (point-to-point) or 6 (point-to-plane) correspondences (too_few), with a system that is not positive definite, i.e. a
    Cholesky pivot not above 1e-13 of its diagonal entry (singular), and with an empty cloud (empty).  A non-finite point, normal or T0
    refuses the pair (nonfinite: a NaN transform); the other pairs of the call are unaffected.  icp_pairs raises on a refusal, naming the
    pair; the other bits are returned in `status` (ops.ICP_STATUS names them).
  Sums.  No float atomics.  Every sum over a pair's rows is formed by lane l of 256 adding rows l, l + 256, .. serially and a fixed tree
    over the lanes, so it depends on the pair's row count alone: results are bit-identical from run to run, and for a pair alone and
    anywhere in a batch.
  No robust loss kernels."""
import numpy as np
import torch

from . import ops as _ops
from .stacking import chunks, device_of, gpu_rows_each, identities, lengths, stack, transforms_of, upload


@torch.no_grad()
def icp_pairs(src_list, ref_list, init_transforms, max_correspondence_distance, estimation='point_to_point', ref_normals_list=None,
              relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, return_correspondences=False, device=None):
    """ICP of P pairs.  src_list / ref_list: (n, 3) float32 or float64 GPU tensors; init_transforms: (P, 4, 4), a device tensor of any
    float dtype (read on the device) or host arrays, ref ~ T src; estimation 'point_to_point' or 'point_to_plane', the latter with
    ref_normals_list or, without it, the normals of scan_prep.estimate_normals_clouds(ref_list).  Returns a dict of device tensors:
    transforms (P, 4, 4) float64, fitness, inlier_rmse (P,) float64, iterations, converged, status (P,) int32, and with
    return_correspondences a list of (n_p,) int64 tensors: the reference row of every source row at the final evaluation, -1 for none.
    One host synchronisation per chunk of 32 pairs: the status words, read after everything was enqueued."""
    P = len(src_list)
    if len(ref_list) != P:
        raise ValueError('icp_pairs: one source and one reference cloud per pair')
    if estimation not in _ops.ICP_MODES:
        raise ValueError('icp_pairs: estimation %r is not one of %s' % (estimation, ', '.join(sorted(_ops.ICP_MODES))))
    r = float(max_correspondence_distance)
    if not (np.isfinite(r) and r >= 0):
        raise ValueError('icp_pairs: max_correspondence_distance %r is not a finite, non-negative number' % (max_correspondence_distance,))
    if not 0 <= int(max_iteration) <= _ops.ICP_MAX_ITERATION:
        raise ValueError('icp_pairs: max_iteration %r not in [0, %d]' % (max_iteration, _ops.ICP_MAX_ITERATION))
    dev = device_of(device, src_list, ref_list)
    srcs = gpu_rows_each(src_list, dev, 'icp_pairs: source cloud', 'ICP')
    refs = gpu_rows_each(ref_list, dev, 'icp_pairs: reference cloud', 'ICP')
    if srcs:
        dev = srcs[0].device
    normals = None
    if estimation == 'point_to_plane':
        if ref_normals_list is None:
            from .scan_prep import estimate_normals_clouds
            normals = estimate_normals_clouds(refs, device=dev)
        else:
            if len(ref_normals_list) != P:
                raise ValueError('icp_pairs: one normals array per reference cloud')
            normals = gpu_rows_each(ref_normals_list, dev, 'icp_pairs: normals', 'ICP')
            if any(n.shape != q.shape for n, q in zip(normals, refs)):
                raise ValueError('icp_pairs: normals must have the shape of their reference cloud')
    if torch.is_tensor(init_transforms) and not init_transforms.is_floating_point():
        raise ValueError('icp_pairs: init_transforms must be floating point')
    T0 = transforms_of(init_transforms, P, 'icp_pairs', dev)          # (a device tensor is read on the device; no finiteness check here:
    parts, corrs = [], []                                             # the kernel refuses a non-finite T0 per pair)
    for a, b in chunks(P):
        s, sl = stack(srcs[a:b]), lengths(srcs[a:b])
        q, ql = stack(refs[a:b]), lengths(refs[a:b])
        nr = stack(normals[a:b]) if normals is not None else None
        grid = _ops.pair_grid_build(q, ql, identities(b - a), r)
        out = _ops.icp_stack(grid, s, sl, T0[a:b], r, estimation, nr, relative_fitness, relative_rmse, max_iteration, return_correspondences)
        if return_correspondences:
            corrs += list(torch.split(out.pop('correspondences'), sl))
        parts.append(out)
        status = out['status'].cpu().tolist()                          # the ONE synchronisation of the chunk
        refused = [a + p for p, w in enumerate(status) if w & _ops.ICP_STATUS['nonfinite']]
        if refused:
            raise ValueError('icp_pairs: pair %s: a point, normal or initial transform is not finite' % ', '.join(str(p) for p in refused))
    parts = parts or [_ops.icp_outputs(0, dev)]
    result = {k: stack([p[k] for p in parts]) for k in parts[0]}
    if return_correspondences:
        result['correspondences'] = corrs
    return result


def registration_icp(src_points, ref_points, init=None, max_correspondence_distance=0.05, estimation='point_to_point', ref_normals=None,
                     relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, device=None):
    """One pair, numpy in and out (the arrays are uploaded inside the call): the (4, 4) float64 transform src -> ref, refined from `init`
    (None: the identity).  The argument order follows ransac.registration_with_ransac_from_correspondences: source first."""
    init = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).reshape(4, 4)
    out = icp_pairs([upload(src_points, device)], [upload(ref_points, device)], init[None], max_correspondence_distance, estimation,
                    None if ref_normals is None else [upload(ref_normals, device)], relative_fitness, relative_rmse, max_iteration)
    return out['transforms'][0].cpu().numpy()


@torch.no_grad()
def refine_pairs(outs, transforms, max_correspondence_distance, estimation='point_to_point', level='points_f'):
    """Refines the (B, 4, 4) device transforms of ransac.register_pairs (or the forward's estimated_transform) on the clouds
    outs[b]['src_' + level] -> outs[b]['ref_' + level] of the output dicts of batched.forward_pairs.  Returns (B, 4, 4) float32 on the
    device, the form evaluation.evaluate_pairs and benchmark.evaluate_registration_log take."""
    if not torch.is_tensor(transforms) or not transforms.is_cuda:
        raise RuntimeError('refine_pairs: transforms must be a (B, 4, 4) GPU tensor')
    out = icp_pairs([o['src_' + level] for o in outs], [o['ref_' + level] for o in outs], transforms, max_correspondence_distance, estimation)
    return out['transforms'].to(torch.float32)
