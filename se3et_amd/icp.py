"""ICP refinement on the device for batched pairs: Open3D's registration_icp, point-to-point or point-to-plane, and its
registration_generalized_icp, each with or without a robust loss kernel, as HIP kernels that stay resident for all pairs of a call
(csrc/icp.hip, csrc/icp_core.h) in place of a k-d tree loop on the host.

  icp_pairs(src_list, ref_list, init_transforms, max_correspondence_distance, estimation, ...)   dict of device tensors for P pairs
  registration_icp(src_points, ref_points, init, max_correspondence_distance, estimation, ...)    one pair, numpy in, (4, 4) numpy out
  refine_pairs(outs, transforms, max_correspondence_distance, estimation, level)                   the output dicts of batched.forward_pairs
                                                                                                   and (B, 4, 4) transforms -> refined ones
  generalized_icp_pairs(src_list, ref_list, init_transforms, max_correspondence_distance, ...)    generalized ICP, the dict of icp_pairs
  registration_generalized_icp(src_points, ref_points, init, max_correspondence_distance, ...)    one pair, numpy in, (4, 4) numpy out
  color_gradient_clouds(points_list, normals_list, colors_list, radius, max_nn)                   the colour gradients of a list of clouds
  colored_icp_pairs(src_list, ref_list, init_transforms, max_correspondence_distance, src_colors_list, ref_colors_list, ...)
                                                                                                   coloured ICP, the dict of icp_pairs
  registration_colored_icp(src_points, ref_points, src_colors, ref_colors, init, ...)             one pair, numpy in, (4, 4) numpy out
  multiscale_icp_pairs(src_list, ref_list, init_transforms, voxel_sizes, max_correspondence_distances, max_iterations, estimation, ...)
                                                                                                   the coarse-to-fine schedule round any estimator
  registration_multiscale_icp(src_points, ref_points, voxel_sizes, max_correspondence_distances, max_iterations, ...)   one pair, numpy

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
  Coloured ICP (colored_icp_pairs; icp_pairs refuses the estimation, as it needs colours).  Open3D's registration_colored_icp,
    TransformationEstimationForColoredICP(lambda_geometric, kernel); csrc/color_gradient.hip and csrc/icp.hip carry the same text.
    Intensity.  The intensity of a row with colour (c0, c1, c2) is ((c0 + c1) + c2) / 3.0; any finite range is accepted.
    Colour gradients (color_gradient_clouds; once per call and scale, not per iteration).  Neighbours of row i, the hybrid search with the
      rules of fpfh.py: the K = max_nn nearest rows of row i's own cloud including row i (K in [1, SE3_KNN_MAX], Open3D's 30), ascending
      by (d^2, index); of those the rows with d^2 < r^2, strict, r^2 = r r in float64; m is the size of that result; the neighbours are
      its members other than row i itself, chosen by index (Open3D drops entry 0 of the result: the rules differ only where a duplicate
      point has a lower index).  m < 4 gives the zero gradient.  One thread per row forms the sums sequentially in the list's order,
      unfused: for a neighbour j, u = p_j - p_i, s = (u . n) with dots as (a b + c d) + e f and n the normal as given, pr = u - s n,
      G += pr pr^T, h += pr (I_j - I_i); afterwards G += (m - 1)^2 n n^T (Open3D's orthogonality row (m - 1) n, right-hand side 0).
      G x = h by a 3x3 Cholesky factorisation; a pivot not above 1e-13 of its diagonal entry gives the zero gradient (ICP's rule; Open3D
      solves by LDLT without a guard).  A non-finite point, normal or colour raises ValueError naming the cloud; n = 0 gives an empty
      output; no atomics: a cloud's rows are bit-identical alone, anywhere in a batch, and from run to run.
    Estimation.  Evaluation, loop, sums, solve, update, the 1 rad refusal, the status bits and the correspondences are those above; only
      the per-correspondence term is new.  For a correspondence under T = [R | t]: p the moved source row, q its reference row, nt that
      row's normal as given, I_t its intensity, g its gradient, I_s the source row's intensity, lambda = lambda_geometric in [0, 1]
      (Open3D's default 0.968), a = sqrt(lambda), b = sqrt(1 - lambda).  Geometric row: r_g = a (p - q) . nt, J_g = a [p x nt, nt].
      Photometric row: p' = p - ((p - q) . nt) nt, I_proj = g . (p' - q) + I_t, r_c = b (I_s - I_proj), d = -(M g) with
      M = I - nt nt^T, J_c = b [p x d, d].  (sum w_g J_g J_g^T + w_c J_c J_c^T) x = -sum (w_g J_g r_g + w_c J_c r_c), w_g = w(r_g),
      w_c = w(r_c) from the loss table; loss=None gives weights 1 and no weight code.  Degenerate cases follow point-to-plane: fewer than
      6 correspondences too_few, a failed pivot singular, an empty cloud empty; a non-finite point, normal, colour, gradient or T0 sets
      nonfinite for that pair alone.
  Multi-scale schedule (multiscale_icp_pairs): Open3D's coarse-to-fine loop round any of the four estimators; its docstring has the rule.
    The colour rule of the downsampling: colours travel through the normals slot of scan_prep.voxel_downsample_clouds, which averages a
    voxel's members in the fixed order of its points and does not renormalise -- the mean colour of the voxel."""
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


def _color_counts(given, clouds, what, which):
    """The first check of a colours list, before anything is asked of the device: one array per cloud, with its row count."""
    if given is None or len(given) != len(clouds):
        raise ValueError('%s: one colours array per %s cloud' % (what, which))
    for c, (col, q) in enumerate(zip(given, clouds)):
        if len(col) != len(q):
            raise ValueError('%s: %s colours %d: %d rows for a cloud of %d' % (what, which, c, len(col), len(q)))


def _colors_of(given, clouds, dev, what, which):
    """The (n, 3) colours of every cloud of a list, checked: one per cloud, on its device, with its row count."""
    _color_counts(given, clouds, what, which)
    colors = gpu_rows_each(given, dev, '%s: %s colours' % (what, which), 'ICP')
    for c, (col, q) in enumerate(zip(colors, clouds)):
        if col.shape != q.shape or col.device != q.device:
            raise ValueError('%s: %s colours %d: %s on %s for a cloud %s on %s' % (what, which, c, tuple(col.shape), col.device, tuple(q.shape),
                                                                                  q.device))
    return colors


def _gradients(p, nr, col, pl, radius, max_nn):
    """(gradients (rows, 3) float64, status words or None) of a chunk's stacked clouds.  A radius of 0 gives zero gradients without a
    search (and without a check: no row has a member)."""
    if radius == 0.0 or p.shape[0] == 0:
        return torch.zeros((p.shape[0], 3), dtype=torch.float64, device=p.device), None
    grid = _ops.pair_grid_build(p, pl, identities(len(pl)), 0.0)
    idx, d2 = _ops.knn_stack(grid, p, pl, max_nn)
    return _ops.color_gradient_stack(p, nr, col, pl, idx, d2, radius)


def _gradient_search(radius, max_nn, what):
    """(radius, K) of a gradient search, or ValueError."""
    r = float(radius)
    if not (np.isfinite(r) and r >= 0):
        raise ValueError('%s: gradient radius %r is not a finite, non-negative number' % (what, radius))
    if int(max_nn) != max_nn or not 1 <= int(max_nn) <= _ops.KNN_MAX:
        raise ValueError("%s: max_nn %r is not an integer in [1, SE3_KNN_MAX = %d]" % (what, max_nn, _ops.KNN_MAX))
    return r, int(max_nn)


def _icp_pairs(what, modes, src_list, ref_list, init_transforms, max_correspondence_distance, estimation, src_normals_list, ref_normals_list,
               epsilon, normal_knn, loss, loss_k, relative_fitness, relative_rmse, max_iteration, return_correspondences, device, colored=None):
    """The body of icp_pairs, generalized_icp_pairs and colored_icp_pairs.  loss None and an estimation of ops.ICP_MODES: ops.icp_stack,
    the entry without weight code; 'colored': ops.icp_colored_stack, with colored = (src_colors_list, ref_colors_list, lambda_geometric,
    gradient_radius, gradient_max_nn); everything else ops.icp_weighted_stack."""
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
    if colored is not None:
        src_colors, ref_colors, lam, grad_r, grad_k = colored
        src_colors, ref_colors = _colors_of(src_colors, srcs, dev, what, 'source'), _colors_of(ref_colors, refs, dev, what, 'reference')
    if torch.is_tensor(init_transforms) and not init_transforms.is_floating_point():
        raise ValueError('%s: init_transforms must be floating point' % what)
    T0 = transforms_of(init_transforms, P, what, dev)                 # (a device tensor is read on the device; no finiteness check here:
    parts, corrs = [], []                                             # the kernel refuses a non-finite T0 per pair)
    for a, b in chunks(P):
        s, sl = stack(srcs[a:b]), lengths(srcs[a:b])
        q, ql = stack(refs[a:b]), lengths(refs[a:b])
        nr = stack(normals[a:b]) if normals is not None else None
        if colored is not None:                                        # (before the ICP grid: the two grids share the stream's workspace)
            rc = stack(ref_colors[a:b])
            grads = _gradients(q, nr, rc, ql, grad_r, grad_k)[0]
        grid = _ops.pair_grid_build(q, ql, identities(b - a), r)
        if colored is not None:
            out = _ops.icp_colored_stack(grid, s, sl, T0[a:b], r, nr, stack(src_colors[a:b]), rc, grads, lam, loss, loss_k, relative_fitness,
                                         relative_rmse, max_iteration, return_correspondences)
        elif loss is None and not general:
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
            raise ValueError('%s: pair %s: a point, normal%s or initial transform is not finite'
                             % (what, ', '.join(str(p) for p in refused), '' if colored is None else ', colour, gradient'))
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
def color_gradient_clouds(points_list, normals_list, colors_list, radius, max_nn=30, device=None):
    """The colour gradients of a list of clouds (the module text has the contract): points, normals and colours (n, 3) float32 or float64
    GPU tensors, radius > 0 and max_nn in [1, SE3_KNN_MAX] the hybrid search (a radius of 0 gives zero gradients without a search).
    Returns the list of (n_c, 3) float64 device tensors.  Chunked at 32 clouds; one host synchronisation per chunk, the status words."""
    what = 'color_gradient_clouds'
    r, K = _gradient_search(radius, max_nn, what)
    if len(normals_list) != len(points_list):
        raise ValueError('%s: one normals array per cloud' % what)
    _color_counts(colors_list, points_list, what, 'own')
    dev = device_of(device, points_list, normals_list, colors_list)
    pts = gpu_rows_each(points_list, dev, '%s: cloud' % what, 'ICP')
    nrs = _normals_of(normals_list, pts, dev, what, 'own', None)
    cols = _colors_of(colors_list, pts, dev, what, 'own')
    out = []
    for a, b in chunks(len(pts)):
        p, pl = stack(pts[a:b]), lengths(pts[a:b])
        grads, words = _gradients(p, stack(nrs[a:b]), stack(cols[a:b]), pl, r, K)
        if words is not None:
            words = words.cpu().tolist()                               # the ONE synchronisation of the chunk: the status
            if words[-1]:
                raise ValueError('%s: ' % what + '; '.join('cloud %d: %s' % (a + c, ', '.join(t for bit, t in _ops.COLOR_GRADIENT_STATUS.items()
                                                                                             if w & bit)) for c, w in enumerate(words[:-1]) if w))
        out += list(torch.split(grads, pl))
    return out


@torch.no_grad()
def colored_icp_pairs(src_list, ref_list, init_transforms, max_correspondence_distance, src_colors_list, ref_colors_list, ref_normals_list=None,
                      lambda_geometric=0.968, gradient_radius=None, gradient_max_nn=30, normal_knn=None, loss=None, loss_k=None,
                      relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, return_correspondences=False, device=None):
    """Coloured ICP of P pairs (the module text has the contract): icp_pairs' arguments, with the colours of both clouds --
    src_colors_list / ref_colors_list, (n, 3) float32 or float64 GPU tensors with the row count and on the device of their cloud -- the
    reference normals (ref_normals_list, or without it scan_prep.estimate_normals_clouds(ref_list, normal_knn)) and lambda_geometric in
    [0, 1].  The reference gradients are computed here, once per call: gradient_radius None is Open3D's 2 x max_correspondence_distance,
    gradient_max_nn its 30; a gradient radius of 0 gives zero gradients without a search.  loss / loss_k as icp_pairs, on each of the two
    residuals.  Returns the dict of icp_pairs, with its chunking, its one synchronisation per chunk and its refusals."""
    what = 'colored_icp_pairs'
    lam = float(lambda_geometric)
    if not 0.0 <= lam <= 1.0:
        raise ValueError('%s: lambda_geometric %r is not in [0, 1]' % (what, lambda_geometric))
    if len(ref_list) != len(src_list):
        raise ValueError('%s: one source and one reference cloud per pair' % what)
    _color_counts(src_colors_list, src_list, what, 'source')
    _color_counts(ref_colors_list, ref_list, what, 'reference')
    r = float(max_correspondence_distance)
    grad = _gradient_search(2.0 * r if gradient_radius is None else gradient_radius, gradient_max_nn, what) if np.isfinite(r) and r >= 0 else (0.0, 1)
    return _icp_pairs(what, ('colored',), src_list, ref_list, init_transforms, max_correspondence_distance, 'colored', None, ref_normals_list,
                      1e-3, normal_knn, loss, loss_k, relative_fitness, relative_rmse, max_iteration, return_correspondences, device,
                      colored=(src_colors_list, ref_colors_list, lam) + grad)


def registration_colored_icp(src_points, ref_points, src_colors, ref_colors, init=None, max_correspondence_distance=0.05, ref_normals=None,
                             lambda_geometric=0.968, gradient_radius=None, gradient_max_nn=30, normal_knn=None, loss=None, loss_k=None,
                             relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, device=None):
    """registration_icp for coloured ICP: one pair, numpy in, the (4, 4) float64 transform out."""
    init = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).reshape(4, 4)
    out = colored_icp_pairs([upload(src_points, device)], [upload(ref_points, device)], init[None], max_correspondence_distance,
                            [upload(src_colors, device)], [upload(ref_colors, device)],
                            None if ref_normals is None else [upload(ref_normals, device)], lambda_geometric, gradient_radius, gradient_max_nn,
                            normal_knn, loss, loss_k, relative_fitness, relative_rmse, max_iteration)
    return out['transforms'][0].cpu().numpy()


MULTISCALE_ESTIMATIONS = ('point_to_point', 'point_to_plane', 'generalized', 'colored')
_PER_SCALE = ('fitness', 'inlier_rmse', 'iterations', 'converged', 'status')


def _schedule(what, voxel_sizes, max_correspondence_distances, max_iterations):
    """The three lists of a schedule, checked: [(voxel size or None, distance, iterations)]."""
    vs, ds, its = list(voxel_sizes), list(max_correspondence_distances), list(max_iterations)
    if not (len(vs) == len(ds) == len(its) >= 1):
        raise ValueError('%s: voxel_sizes, max_correspondence_distances and max_iterations must have one length, at least 1: %d, %d, %d'
                         % (what, len(vs), len(ds), len(its)))
    if any(v is None for v in vs[:-1]):
        raise ValueError('%s: a voxel size of None (the clouds as given) is allowed only as the last entry' % what)
    sizes = [float(v) for v in vs if v is not None]
    if not all(np.isfinite(v) and v > 0 for v in sizes) or any(b >= a for a, b in zip(sizes, sizes[1:])):
        raise ValueError('%s: the voxel sizes %r must be positive, finite and strictly decreasing' % (what, vs))
    return list(zip(vs, ds, its))


@torch.no_grad()
def multiscale_icp_pairs(src_list, ref_list, init_transforms, voxel_sizes, max_correspondence_distances, max_iterations,
                         estimation='point_to_plane', src_colors_list=None, ref_colors_list=None, normal_knn=30, lambda_geometric=0.968,
                         epsilon=1e-3, loss=None, loss_k=None, relative_fitness=1e-6, relative_rmse=1e-6, device=None):
    """The coarse-to-fine schedule of Open3D's tutorial and multi_scale_icp round an estimator: estimation one of 'point_to_point',
    'point_to_plane', 'generalized', 'colored' (the last with src_colors_list / ref_colors_list).  The three lists have one length >= 1.
    For scale s, in order:
      1. both clouds of every pair are downsampled by scan_prep.voxel_downsample_clouds at voxel_sizes[s]; colours travel through its
         normals slot, which averages in the fixed order and does not renormalise (the voxel's mean colour).  None means the clouds as
         given and is allowed only as the last entry; the positive sizes are strictly decreasing (Open3D's rule);
      2. where the estimation reads normals they are estimate_normals_clouds(clouds, normal_knn) of that scale's clouds (the reference's;
         for 'generalized' both);
      3. the estimator -- icp_pairs, generalized_icp_pairs or colored_icp_pairs (gradient radius 2 x the scale's distance) -- runs with
         max_correspondence_distances[s] and max_iterations[s] from the previous scale's `transforms`, passed as the device tensor they
         are: no transform is read back between scales.
    Returns the last scale's dict plus per_scale: a list of dicts, one per scale, with that scale's transforms, fitness, inlier_rmse,
    iterations, converged and status device tensors.  Host synchronisations: per scale and per chunk of 32 pairs THREE -- the downsampling
    counts of the sources, those of the references, and the estimator's status words -- and one for a scale of None; the number does
    not grow with the pairs in a chunk.  A call with one scale and voxel_sizes=[None] returns the bits of the plain estimator's call
    with the same normals."""
    from .scan_prep import estimate_normals_clouds, voxel_downsample_clouds
    what = 'multiscale_icp_pairs'
    if estimation not in MULTISCALE_ESTIMATIONS:
        raise ValueError('%s: estimation %r is not one of %s' % (what, estimation, ', '.join(sorted(MULTISCALE_ESTIMATIONS))))
    schedule = _schedule(what, voxel_sizes, max_correspondence_distances, max_iterations)
    P = len(src_list)
    if len(ref_list) != P:
        raise ValueError('%s: one source and one reference cloud per pair' % what)
    colored = estimation == 'colored'
    if colored:
        _color_counts(src_colors_list, src_list, what, 'source')
        _color_counts(ref_colors_list, ref_list, what, 'reference')
    dev = device_of(device, src_list, ref_list)
    srcs = gpu_rows_each(src_list, dev, '%s: source cloud' % what, 'ICP')
    refs = gpu_rows_each(ref_list, dev, '%s: reference cloud' % what, 'ICP')
    if srcs:
        dev = srcs[0].device
    scols = _colors_of(src_colors_list, srcs, dev, what, 'source') if colored else None
    rcols = _colors_of(ref_colors_list, refs, dev, what, 'reference') if colored else None
    T, out, per_scale = init_transforms, None, []
    for v, r, it in schedule:
        s, q, sc, rc = srcs, refs, scols, rcols
        if v is not None and colored:                                  # (colours through the normals slot: a plain mean, not renormalised)
            (s, sc), (q, rc) = voxel_downsample_clouds(srcs, v, scols, device=dev), voxel_downsample_clouds(refs, v, rcols, device=dev)
        elif v is not None:
            s, q = voxel_downsample_clouds(srcs, v, device=dev), voxel_downsample_clouds(refs, v, device=dev)
        if estimation == 'generalized':
            out = generalized_icp_pairs(s, q, T, r, estimate_normals_clouds(s, normal_knn, device=dev),
                                        estimate_normals_clouds(q, normal_knn, device=dev), epsilon, normal_knn, loss, loss_k, relative_fitness,
                                        relative_rmse, it, device=dev)
        elif colored:
            out = colored_icp_pairs(s, q, T, r, sc, rc, estimate_normals_clouds(q, normal_knn, device=dev), lambda_geometric, None, 30, normal_knn,
                                    loss, loss_k, relative_fitness, relative_rmse, it, device=dev)
        else:
            out = icp_pairs(s, q, T, r, estimation, estimate_normals_clouds(q, normal_knn, device=dev) if estimation == 'point_to_plane' else None,
                            relative_fitness, relative_rmse, it, device=dev, loss=loss, loss_k=loss_k)
        T = out['transforms']
        per_scale.append({k: out[k] for k in ('transforms',) + _PER_SCALE})
    return dict(out, per_scale=per_scale)


def registration_multiscale_icp(src_points, ref_points, voxel_sizes, max_correspondence_distances, max_iterations, init=None,
                                estimation='point_to_plane', src_colors=None, ref_colors=None, normal_knn=30, lambda_geometric=0.968,
                                epsilon=1e-3, loss=None, loss_k=None, relative_fitness=1e-6, relative_rmse=1e-6, device=None):
    """multiscale_icp_pairs for one pair, numpy in, the (4, 4) float64 transform out."""
    init = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).reshape(4, 4)
    out = multiscale_icp_pairs([upload(src_points, device)], [upload(ref_points, device)], init[None], voxel_sizes, max_correspondence_distances,
                               max_iterations, estimation, None if src_colors is None else [upload(src_colors, device)],
                               None if ref_colors is None else [upload(ref_colors, device)], normal_knn, lambda_geometric, epsilon, loss, loss_k,
                               relative_fitness, relative_rmse)
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
