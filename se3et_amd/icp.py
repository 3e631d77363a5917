"""ICP refinement on the device for batched pairs: Open3D's registration_icp, point-to-point or point-to-plane, and its
registration_generalized_icp, each with or without a robust loss kernel, as HIP kernels that stay resident for all pairs of a call
(csrc/icp.hip, csrc/icp_core.h) in place of a k-d tree loop on the host.

  icp_pairs(src_list, ref_list, init_transforms, max_correspondence_distance, estimation, ...)   dict of device tensors for P pairs
  registration_icp(src_points, ref_points, init, max_correspondence_distance, estimation, ...)    one pair, numpy in, (4, 4) numpy out
  refine_pairs(outs, transforms, max_correspondence_distance, estimation, level)                   the output dicts of batched.forward_pairs
                                                                                                   and (B, 4, 4) transforms -> refined ones
  generalized_icp_pairs(src_list, ref_list, init_transforms, max_correspondence_distance, ...)    generalized ICP, the dict of icp_pairs
  registration_generalized_icp(src_points, ref_points, init, max_correspondence_distance, ...)    one pair, numpy in, (4, 4) numpy out

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
  Loss kernels (loss=, loss_k=; None: none, and the kernels and bits of a call before the losses existed).  Open3D's RobustKernel weights
    of a scalar residual r with k = loss_k > 0:  'l2' 1;  'huber' 1 for |r| <= k, else k / |r|;  'cauchy' 1 / (1 + (r / k)^2);
    'gm' k / (k + r^2)^2;  'tukey' (1 - (r / k)^2)^2 for |r| <= k, else 0.  Every weight is continuous at its branch.  Open3D's L1Loss is
    not offered: its weight 1 / |r| is unbounded at an exact match, and 'huber' covers its use.  Iteratively reweighted least squares,
    the weights from the current evaluation; the evaluation (correspondences, fitness, inlier_rmse), the loop, the too-few counts (they
    count correspondences, not weights) and the status bits do not change.  loss='l2' runs the weight-carrying kernels with weight 1.
    Point-to-plane: w_i = w(r_i), (sum w_i J_i^T J_i) x = -sum w_i J_i^T r_i: Open3D's TransformationEstimationPointToPlane(kernel).
    Point-to-point: w_i = w(sqrt(d_i^2)) and the weighted Kabsch pc = sum w p / W, qc = sum w q / W, H = sum w (p - pc)(q - qc)^T,
      W = sum w; a W that is not > 0 is `singular` with the identity update (tukey with every correspondence beyond k).  Open3D's
      legacy point-to-point takes no kernel: this is the project's definition.
  Generalized ICP (generalized_icp_pairs; icp_pairs refuses the estimation).  Open3D's registration_generalized_icp with the
    covariances of its normals form: a point with unit normal n has C = I - (1 - eps) n n^T (= R diag(eps, 1, 1) R^T with n the first
    column of R), eps = epsilon in (0, 1], default 1e-3.  It needs the unit normals of BOTH clouds and nothing else, and does not depend
    on a normal's sign.  For a correspondence under T = [R | t]: p the moved source row, q its reference row, nt the normal of q,
    m = R ns the turned source normal, d = p - q, M = 2 I - (1 - eps)(nt nt^T + m m^T) inverted by its cofactors, A = [-[p]_x | I];
    (sum w A^T M^-1 A) x = -sum w A^T M^-1 d with the solve, the 1 rad refusal and the update matrix of point-to-plane.  At least 6
    correspondences; fitness and inlier_rmse stay Euclidean, as Open3D's result fields are; a non-finite source normal refuses the pair.
    The loss acts on the Mahalanobis residual, w = w(sqrt(d^T M^-1 d)); Open3D weights the three rows of M^(-1/2) d one by one, which
    needs a matrix square root -- with 'l2' the two systems are the same in exact arithmetic.
  No coloured ICP."""
import numpy as np
import torch

from . import ops as _ops
from .stacking import chunks, device_of, gpu_rows_each, identities, lengths, stack, transforms_of, upload


def _normals_of(given, clouds, dev, what, which, knn):
    """The (n, 3) normals of every cloud: the given list, checked, or the k-NN normals of the clouds."""
    if given is None:
        from .scan_prep import estimate_normals_clouds
        return estimate_normals_clouds(clouds, device=dev) if knn is None else estimate_normals_clouds(clouds, knn, device=dev)
    normals = gpu_rows_each(given, dev, '%s: %snormals' % (what, 'source ' if which == 'source' else ''), 'ICP')
    if any(n.shape != q.shape for n, q in zip(normals, clouds)):
        raise ValueError('%s: normals must have the shape of their %s cloud' % (what, which))
    return normals


def _icp_pairs(what, modes, src_list, ref_list, init_transforms, max_correspondence_distance, estimation, src_normals_list, ref_normals_list,
               epsilon, normal_knn, loss, loss_k, relative_fitness, relative_rmse, max_iteration, return_correspondences, device):
    """The body of icp_pairs and generalized_icp_pairs.  loss None and an estimation of ops.ICP_MODES: ops.icp_stack, the entry without
    weight code; everything else ops.icp_weighted_stack."""
    P = len(src_list)
    if len(ref_list) != P:
        raise ValueError('%s: one source and one reference cloud per pair' % what)
    if estimation not in modes:
        raise ValueError('%s: estimation %r is not one of %s' % (what, estimation, ', '.join(sorted(modes))))
    _ops.icp_loss_of(loss, loss_k, what)
    general = estimation == 'generalized'
    eps = float(epsilon)
    if general and not 0.0 < eps <= 1.0:
        raise ValueError('%s: epsilon %r is not in (0, 1]' % (what, epsilon))
    r = float(max_correspondence_distance)
    if not (np.isfinite(r) and r >= 0):
        raise ValueError('%s: max_correspondence_distance %r is not a finite, non-negative number' % (what, max_correspondence_distance))
    if not 0 <= int(max_iteration) <= _ops.ICP_MAX_ITERATION:
        raise ValueError('%s: max_iteration %r not in [0, %d]' % (what, max_iteration, _ops.ICP_MAX_ITERATION))
    if general and src_normals_list is not None and len(src_normals_list) != P:
        raise ValueError('%s: one normals array per source cloud' % what)
    dev = device_of(device, src_list, ref_list)
    srcs = gpu_rows_each(src_list, dev, '%s: source cloud' % what, 'ICP')
    refs = gpu_rows_each(ref_list, dev, '%s: reference cloud' % what, 'ICP')
    if srcs:
        dev = srcs[0].device
    normals, src_normals = None, None
    if estimation != 'point_to_point':
        if ref_normals_list is not None and len(ref_normals_list) != P:
            raise ValueError('%s: one normals array per reference cloud' % what)
        normals = _normals_of(ref_normals_list, refs, dev, what, 'reference', normal_knn)
    if general:
        src_normals = _normals_of(src_normals_list, srcs, dev, what, 'source', normal_knn)
    if torch.is_tensor(init_transforms) and not init_transforms.is_floating_point():
        raise ValueError('%s: init_transforms must be floating point' % what)
    T0 = transforms_of(init_transforms, P, what, dev)                 # (a device tensor is read on the device; no finiteness check here:
    parts, corrs = [], []                                             # the kernel refuses a non-finite T0 per pair)
    for a, b in chunks(P):
        s, sl = stack(srcs[a:b]), lengths(srcs[a:b])
        q, ql = stack(refs[a:b]), lengths(refs[a:b])
        nr = stack(normals[a:b]) if normals is not None else None
        grid = _ops.pair_grid_build(q, ql, identities(b - a), r)
        if loss is None and not general:
            out = _ops.icp_stack(grid, s, sl, T0[a:b], r, estimation, nr, relative_fitness, relative_rmse, max_iteration, return_correspondences)
        else:
            out = _ops.icp_weighted_stack(grid, s, sl, T0[a:b], r, estimation, nr, stack(src_normals[a:b]) if general else None, loss, loss_k,
                                          eps, relative_fitness, relative_rmse, max_iteration, return_correspondences)
        if return_correspondences:
            corrs += list(torch.split(out.pop('correspondences'), sl))
        parts.append(out)
        status = out['status'].cpu().tolist()                          # the ONE synchronisation of the chunk
        refused = [a + p for p, w in enumerate(status) if w & _ops.ICP_STATUS['nonfinite']]
        if refused:
            raise ValueError('%s: pair %s: a point, normal or initial transform is not finite' % (what, ', '.join(str(p) for p in refused)))
    parts = parts or [_ops.icp_outputs(0, dev)]
    result = {k: stack([p[k] for p in parts]) for k in parts[0]}
    if return_correspondences:
        result['correspondences'] = corrs
    return result


@torch.no_grad()
def icp_pairs(src_list, ref_list, init_transforms, max_correspondence_distance, estimation='point_to_point', ref_normals_list=None,
              relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, return_correspondences=False, device=None, loss=None, loss_k=None):
    """ICP of P pairs.  src_list / ref_list: (n, 3) float32 or float64 GPU tensors; init_transforms: (P, 4, 4), a device tensor of any
    float dtype (read on the device) or host arrays, ref ~ T src; estimation 'point_to_point' or 'point_to_plane', the latter with
    ref_normals_list or, without it, the normals of scan_prep.estimate_normals_clouds(ref_list).  loss: None, or 'l2', 'huber', 'cauchy',
    'gm', 'tukey' (ops.ICP_LOSSES) with its width loss_k, finite and positive ('l2' takes none); Open3D's L1Loss is not offered (see the
    module text).  Returns a dict of device tensors:
    transforms (P, 4, 4) float64, fitness, inlier_rmse (P,) float64, iterations, converged, status (P,) int32, and with
    return_correspondences a list of (n_p,) int64 tensors: the reference row of every source row at the final evaluation, -1 for none.
    One host synchronisation per chunk of 32 pairs: the status words, read after everything was enqueued."""
    return _icp_pairs('icp_pairs', _ops.ICP_MODES, src_list, ref_list, init_transforms, max_correspondence_distance, estimation, None,
                      ref_normals_list, 1e-3, None, loss, loss_k, relative_fitness, relative_rmse, max_iteration, return_correspondences, device)


@torch.no_grad()
def generalized_icp_pairs(src_list, ref_list, init_transforms, max_correspondence_distance, src_normals_list=None, ref_normals_list=None,
                          epsilon=1e-3, normal_knn=20, loss=None, loss_k=None, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30,
                          return_correspondences=False, device=None):
    """Generalized ICP of P pairs (the module text has the contract): icp_pairs' arguments, with the unit normals of BOTH clouds --
    src_normals_list / ref_normals_list, (n, 3) GPU tensors per cloud, or for a missing list scan_prep.estimate_normals_clouds(clouds,
    normal_knn) -- and epsilon in (0, 1].  loss / loss_k as icp_pairs, acting on the Mahalanobis residual.  Returns the dict of icp_pairs,
    with its chunking, its one synchronisation per chunk and its refusals."""
    return _icp_pairs('generalized_icp_pairs', ('generalized',), src_list, ref_list, init_transforms, max_correspondence_distance, 'generalized',
                      src_normals_list, ref_normals_list, epsilon, normal_knn, loss, loss_k, relative_fitness, relative_rmse, max_iteration,
                      return_correspondences, device)


def registration_icp(src_points, ref_points, init=None, max_correspondence_distance=0.05, estimation='point_to_point', ref_normals=None,
                     relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, device=None, loss=None, loss_k=None):
    """One pair, numpy in and out (the arrays are uploaded inside the call): the (4, 4) float64 transform src -> ref, refined from `init`
    (None: the identity).  The argument order follows ransac.registration_with_ransac_from_correspondences: source first."""
    init = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).reshape(4, 4)
    out = icp_pairs([upload(src_points, device)], [upload(ref_points, device)], init[None], max_correspondence_distance, estimation,
                    None if ref_normals is None else [upload(ref_normals, device)], relative_fitness, relative_rmse, max_iteration,
                    loss=loss, loss_k=loss_k)
    return out['transforms'][0].cpu().numpy()


def registration_generalized_icp(src_points, ref_points, init=None, max_correspondence_distance=0.05, src_normals=None, ref_normals=None,
                                 epsilon=1e-3, normal_knn=20, loss=None, loss_k=None, relative_fitness=1e-6, relative_rmse=1e-6,
                                 max_iteration=30, device=None):
    """registration_icp for generalized ICP: one pair, numpy in, the (4, 4) float64 transform out."""
    init = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).reshape(4, 4)
    out = generalized_icp_pairs([upload(src_points, device)], [upload(ref_points, device)], init[None], max_correspondence_distance,
                                None if src_normals is None else [upload(src_normals, device)],
                                None if ref_normals is None else [upload(ref_normals, device)], epsilon, normal_knn, loss, loss_k,
                                relative_fitness, relative_rmse, max_iteration)
    return out['transforms'][0].cpu().numpy()


@torch.no_grad()
def refine_pairs(outs, transforms, max_correspondence_distance, estimation='point_to_point', level='points_f', loss=None, loss_k=None):
    """Refines the (B, 4, 4) device transforms of ransac.register_pairs (or the forward's estimated_transform) on the clouds
    outs[b]['src_' + level] -> outs[b]['ref_' + level] of the output dicts of batched.forward_pairs.  Returns (B, 4, 4) float32 on the
    device, the form evaluation.evaluate_pairs and benchmark.evaluate_registration_log take."""
    if not torch.is_tensor(transforms) or not transforms.is_cuda:
        raise RuntimeError('refine_pairs: transforms must be a (B, 4, 4) GPU tensor')
    out = icp_pairs([o['src_' + level] for o in outs], [o['ref_' + level] for o in outs], transforms, max_correspondence_distance, estimation,
                    loss=loss, loss_k=loss_k)
    return out['transforms'].to(torch.float32)
