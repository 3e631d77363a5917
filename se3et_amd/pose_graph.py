"""Multiway registration on the device: Open3D's get_information_matrix_from_point_clouds and global_optimization
(GlobalOptimization.cpp: Levenberg-Marquardt with a line process, pruning, a second optimisation), and the recipe of its multiway
tutorial on top of icp.icp_pairs -- the one stage of the classical pipeline that puts the fragments of a scene into one frame and says
whether the pairwise transforms agree with each other (csrc/pose_graph.hip, csrc/pose_graph_core.h).

  information_matrix_pairs(src_list, ref_list, transforms, max_correspondence_distance)        dict of device tensors for P pairs
  get_information_matrix_from_point_clouds(src, ref, max_correspondence_distance, transformation)   one pair, numpy in, (6, 6) numpy out
  optimize_pose_graphs(graphs, ...criteria, ...option)                                         dict of device tensors and per-graph lists
  global_optimization(poses, edges, transforms, informations, uncertain, ...)                  one graph, numpy in and out
  multiway_registration(clouds, edges, init_transforms, max_correspondence_distance_coarse, max_correspondence_distance_fine, ...)

GPU tensors or numpy arrays (uploaded inside the call; there is no CPU path), any number of pairs / graphs per call, chunked at the
library's SE3_PAIR_MAX_PAIRS.  Nothing is read back except where stacking already synchronises; multiway_registration also waits where
icp_pairs does (its status words).  The whole optimisation of a chunk of graphs is ONE launch, one workgroup of 256 threads per graph.

Contract, part A: the information matrix of a pair.  Source S, reference R and T with ref ~ T src, as everywhere in icp.py.  Source row i
  has a correspondence iff its moved point has a nearest reference point with d^2 < r^2: ICP's evaluation rule, strict, the same
  arithmetic, the same search.  With q = (x, y, z) the REFERENCE point of the correspondence, in the reference frame:
    G = [[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]],   Lambda = sum G^T G
  over the correspondences; the 21 distinct entries are each taken in the order of ICP's sums over the source rows, a row without a
  correspondence adding +0; float64, contraction off.  Lambda[5][5] is the correspondence count.  A non-finite coordinate or transform
  gives a NaN matrix and the nonfinite status, an empty cloud the zero matrix and the empty status.  A pair's Lambda is bit-identical
  alone or anywhere in a batch.

Contract, part B: one pose graph.  N nodes with poses X_i (node frame -> common frame); E edges (s, t, T, Lambda, uncertain), T mapping
  node s's cloud into node t's frame: a consistent graph has X_s = X_t T.  Everything is float64 with contraction off; every square root
  is the library's correctly rounded one; every 4x4 product is (a b + c d) + e f per entry, the translation added last.
  0. Refusals, tested in this order, only the first one set: a non-finite pose, T, Lambda or option: nonfinite, NaN poses; N = 0: empty,
     nothing written; an edge index outside [0, N) or s = t: bad_index, NaN poses.  More than ops.PGO_MAX_NODES nodes or
     ops.PGO_MAX_EDGES edges is an error of the call.  E = 0 is no refusal: the right-term test stops each pass at once.
  1. Residual of an edge.  M = (T^-1 X_t^-1) X_s with the rigid inverses in closed form (R^T, -R^T t).  e = vec6(M): with
     sy = sqrt(M00^2 + M10^2); unless sy < 1e-6: alpha = atan2(M21, M22), beta = atan2(-M20, sy), gamma = atan2(M10, M00); otherwise
     alpha = atan2(-M12, M11), beta = atan2(-M20, sy), gamma = 0; e = (alpha, beta, gamma, M03, M13, M23).  atan2 is the library's own,
     one text for host and device: the argument is reduced to [0, 1] by the usual swaps and once more at tan(pi / 8), then a fixed
     series, every operation rounded on its own; within 4 ulp of the correctly rounded value.
  2. Jacobians, linearised as in Open3D.  D_0 .. D_5 the generators; with A = T^-1 X_t^-1, column i of J_s is lin6(A (D_i X_s)),
     lin6(M) = ((M21 - M12) / 2, (M02 - M20) / 2, (M10 - M01) / 2, M03, M13, M23); J_t = -J_s.
  3. Line process.  mu = preference_loop_closure max_correspondence_distance^2 (mean of Lambda[5][5] over the pass's edges).  l = 1 for
     a certain edge, (mu / (mu + e^T Lambda e))^2 for an uncertain one.
  4. Residual of the graph.  F = sum over the edges of l e^T Lambda e + (uncertain ? mu (sqrt(l) - 1)^2 : 0), in the order of ICP's sums.
  5. Linear system.  Every entry of H (6N x 6N) and b is the sum of its edges' terms l J_a^T Lambda J_c, l J_a^T Lambda e in ascending
     edge index from zero; duplicate edges each add.  (H + lambda I) delta = -b by a dense Cholesky factorisation,
     L_ij = (a_ij - sum_{k<j} L_ik L_jk) / L_jj in ascending k; the forward solve subtracts in ascending k, the backward solve in
     descending k.  A pivot that is not > 0 sets `singular` and ends the pass at the poses it had.
  6. Loop of one pass (Open3D's defaults): lambda starts at 1e-5 max |diag H|, nu at 2; each trial solves for delta, stops on
     |delta| < min_relative_increment (|x| + min_relative_increment), forms X'_i = U(delta_i) X_i (U = [Rz Ry Rx | t] with FGR's sine and
     cosine; a non-finite angle or one of 4 rad and more sets step_refused and ends the pass at X), F' with the CURRENT l, and
     rho = (F - F') / (delta . (lambda delta - b) + 1e-3).  rho > 0: stop if F - F' < min_relative_residual_increment F (X' is not
     taken); else lambda <- lambda max(lower, min(1 - (2 rho - 1)^3, upper)), nu <- 2, the trial is taken, l, H and b are formed anew, and
     max |b| < min_right_term stops.  Otherwise lambda <- lambda nu, nu <- 2 nu.  At most max_iteration_lm trials per iteration; after
     each iteration F < min_residual or it + 1 >= max_iteration stops.  csrc/pose_graph.hip spells the loop out line by line.
  7. Whole optimisation.  Pass 1 on all edges; kept = certain, or l > edge_prune_threshold; pass 2 on the kept edges from pass 1's poses,
     mu over the kept edges; with reference_node >= 0 every pose is left-multiplied by X_ref(input) X_ref(output)^-1, and the node itself
     gets its input pose exactly.  A pruned edge keeps its pass-1 confidence; its pass-2 slot is 0.
  A graph's result is bit-identical from run to run, and alone or anywhere in a batch.
  Differences from Open3D: the arc tangent and the sine and cosine (the library's series); |b| in the right-term test; the line process
  applied before the first residual; the summation orders; the dense Cholesky in place of Eigen's solver; the refusals.
  ops.PGO_STATUS names the status bits, ops.PGO_STOP the stop reasons."""
import numpy as np
import torch

from . import ops as _ops
from .stacking import as_tensor, chunks, device_of, gpu_rows_each, identities, lengths, stack, transforms_of, upload

_FAMILY = 'multiway registration'
CRITERIA = dict(max_iteration=100, max_iteration_lm=20, min_relative_increment=1e-6, min_relative_residual_increment=1e-6,
                min_right_term=1e-6, min_residual=1e-6, upper_scale_factor=2.0 / 3.0, lower_scale_factor=1.0 / 3.0)
OPTION = dict(max_correspondence_distance=0.075, edge_prune_threshold=0.25, preference_loop_closure=1.0, reference_node=-1)


@torch.no_grad()
def information_matrix_pairs(src_list, ref_list, transforms, max_correspondence_distance, device=None):
    """The information matrix of P registered pairs (part A of the module text).  src_list / ref_list: (n, 3) float32 or float64 GPU
    tensors; transforms: (P, 4, 4), a device tensor (read on the device) or host arrays, ref ~ T src.  Returns a dict of device tensors:
    information (P, 6, 6) float64, count (P,) float64 (the correspondences: information[:, 5, 5]), status (P,) int32."""
    what = 'information_matrix_pairs'
    P = len(src_list)
    if len(ref_list) != P:
        raise ValueError('%s: one source and one reference cloud per pair' % what)
    r = float(max_correspondence_distance)
    if not (np.isfinite(r) and r >= 0):
        raise ValueError('%s: max_correspondence_distance %r is not a finite, non-negative number' % (what, max_correspondence_distance))
    dev = device_of(device, src_list, ref_list)
    srcs = gpu_rows_each(src_list, dev, '%s: source cloud' % what, _FAMILY)
    refs = gpu_rows_each(ref_list, dev, '%s: reference cloud' % what, _FAMILY)
    if srcs:
        dev = srcs[0].device
    T = transforms_of(transforms, P, what, dev)
    parts = []
    for a, b in chunks(P):
        s, sl = stack(srcs[a:b]), lengths(srcs[a:b])
        q, ql = stack(refs[a:b]), lengths(refs[a:b])
        parts.append(_ops.pair_information_stack(_ops.pair_grid_build(q, ql, identities(b - a), r), s, sl, T[a:b].contiguous(), r))
    if not parts:
        parts = [{'information': torch.empty((0, 6, 6), dtype=torch.float64, device=dev), 'count': torch.empty((0,), dtype=torch.float64, device=dev),
                  'status': torch.empty((0,), dtype=torch.int32, device=dev)}]
    return {k: stack([p[k] for p in parts]) for k in parts[0]}


def get_information_matrix_from_point_clouds(src, ref, max_correspondence_distance, transformation, device=None):
    """One pair, numpy in and out (the arrays are uploaded inside the call): the (6, 6) float64 information matrix, Open3D's argument
    order."""
    T = np.asarray(transformation, dtype=np.float64).reshape(1, 4, 4)
    return information_matrix_pairs([upload(src, device)], [upload(ref, device)], T, max_correspondence_distance)['information'][0].cpu().numpy()


def _rigid_inverse(T):
    """(R^T, -R^T t) of a rigid (4, 4) device tensor: no factorisation, so nothing waits on the host."""
    out = torch.eye(4, dtype=T.dtype, device=T.device)
    out[:3, :3] = T[:3, :3].t()
    out[:3, 3] = -(T[:3, :3].t() @ T[:3, 3])
    return out


def _graph_tensors(graph, g, dev, what):
    def part(key, shape, dtype):
        if key not in graph:
            raise ValueError('%s: graph %d has no %r' % (what, g, key))
        t = as_tensor(graph[key])
        if dtype is torch.uint8 and t.dtype is torch.bool:
            t = t.to(torch.uint8)
        if dtype is torch.float64 and not t.is_floating_point():
            raise ValueError('%s: graph %d: %s must be floating point' % (what, g, key))
        return t.to(device=dev, dtype=dtype).reshape(*shape).contiguous()
    X, e = part('poses', (-1, 4, 4), torch.float64), part('edges', (-1, 2), torch.int64)
    T, L, u = part('transforms', (-1, 4, 4), torch.float64), part('informations', (-1, 6, 6), torch.float64), part('uncertain', (-1,), torch.uint8)
    if not (T.shape[0] == L.shape[0] == u.shape[0] == e.shape[0]):
        raise ValueError('%s: graph %d: one transform, one information matrix and one uncertain flag per edge' % (what, g))
    if X.shape[0] > _ops.PGO_MAX_NODES or e.shape[0] > _ops.PGO_MAX_EDGES:
        raise ValueError('%s: graph %d has %d nodes and %d edges (at most %d, %d)' % (what, g, X.shape[0], e.shape[0], _ops.PGO_MAX_NODES,
                                                                                   _ops.PGO_MAX_EDGES))
    return X, e, T, L, u


@torch.no_grad()
def optimize_pose_graphs(graphs, reference_node=-1, device=None, **options):
    """The global optimisation of G pose graphs (part B of the module text).  graphs: dicts with poses (N, 4, 4), edges (E, 2) (source
    node, target node), transforms (E, 4, 4), informations (E, 6, 6), uncertain (E,), GPU tensors or numpy arrays; options: the names of
    CRITERIA and OPTION (Open3D's GlobalOptimizationConvergenceCriteria and GlobalOptimizationOption); reference_node: one for all
    graphs, or a list of one per graph, -1 for none.  Returns a dict: status (G,) int32, info (G, 6) int32 (stop reason, iterations,
    trials of pass 1, then of pass 2), residuals (G, 2) float64 on the device, and per graph the lists poses [(N_g, 4, 4)], confidence
    [(2, E_g)], kept [(E_g,) bool] of device tensors.  A refused graph has NaN poses and does not raise."""
    what = 'optimize_pose_graphs'
    known = dict(CRITERIA, **{k: v for k, v in OPTION.items() if k != 'reference_node'})
    for k in options:
        if k not in known:
            raise ValueError('%s: unknown option %r (known: %s)' % (what, k, ', '.join(sorted(known))))
    o = dict(known, **options)
    if not 0 <= int(o['max_iteration']) <= _ops.PGO_MAX_ITERATION or not 0 <= int(o['max_iteration_lm']) <= _ops.PGO_MAX_ITERATION_LM:
        raise ValueError('%s: max_iteration in [0, %d] and max_iteration_lm in [0, %d]' % (what, _ops.PGO_MAX_ITERATION, _ops.PGO_MAX_ITERATION_LM))
    G = len(graphs)
    refs = list(reference_node) if isinstance(reference_node, (list, tuple)) else [int(reference_node)] * G
    if len(refs) != G:
        raise ValueError('%s: one reference node per graph' % what)
    dev = device_of(device, *[[v for v in g.values()] for g in graphs])
    parts = [_graph_tensors(g, i, dev, what) for i, g in enumerate(graphs)]
    for i, (X, _e, _T, _L, _u) in enumerate(parts):
        if not -1 <= refs[i] < max(X.shape[0], 0) and refs[i] != -1:
            raise ValueError('%s: graph %d: reference node %d of %d nodes' % (what, i, refs[i], X.shape[0]))
    f64 = dict(dtype=torch.float64, device=dev)
    result = {'status': [], 'info': [], 'residuals': [], 'poses': [], 'confidence': [], 'kept': []}
    for a, b in chunks(G):
        chunk = parts[a:b]
        nl, el = [int(p[0].shape[0]) for p in chunk], [int(p[1].shape[0]) for p in chunk]
        out = _ops.pose_graph_optimize_stack(stack([p[0] for p in chunk]), nl, stack([p[1] for p in chunk]), stack([p[2] for p in chunk]),
                                             stack([p[3] for p in chunk]), stack([p[4] for p in chunk]), el, refs[a:b], **o)
        for k in ('status', 'info', 'residuals'):
            result[k].append(out[k])
        result['poses'] += list(torch.split(out['poses'], nl))
        result['confidence'] += list(torch.split(out['confidence'], el, dim=1))
        result['kept'] += [k.to(torch.bool) for k in torch.split(out['kept'], el)]
    result['status'] = stack(result['status'], torch.empty((0,), dtype=torch.int32, device=dev))
    result['info'] = stack(result['info'], torch.empty((0, 6), dtype=torch.int32, device=dev))
    result['residuals'] = stack(result['residuals'], torch.empty((0, 2), **f64))
    return result


def global_optimization(poses, edges, transforms, informations, uncertain, reference_node=-1, device=None, **options):
    """One graph, numpy in and out: a dict with poses (N, 4, 4), confidence (2, E), kept (E,) bool, status, info (6,), residuals (2,)."""
    out = optimize_pose_graphs([dict(poses=np.asarray(poses, np.float64), edges=np.asarray(edges, np.int64),
                                     transforms=np.asarray(transforms, np.float64), informations=np.asarray(informations, np.float64),
                                     uncertain=np.asarray(uncertain).astype(np.uint8))], reference_node, device or 'cuda', **options)
    return {'poses': out['poses'][0].cpu().numpy(), 'confidence': out['confidence'][0].cpu().numpy(), 'kept': out['kept'][0].cpu().numpy(),
            'status': int(out['status'][0]), 'info': out['info'][0].cpu().numpy(), 'residuals': out['residuals'][0].cpu().numpy()}


@torch.no_grad()
def multiway_registration(clouds, edges=None, init_transforms=None, max_correspondence_distance_coarse=0.15,
                          max_correspondence_distance_fine=0.015, estimation='point_to_point', normals=None, device=None, **options):
    """The recipe of Open3D's multiway registration tutorial for one scene of K clouds ((n, 3) float32 / float64 GPU tensors).  edges:
    (E, 2) (source cloud, target cloud), default all i < j; (i, i + 1) is certain (odometry), the rest uncertain (loop closures).  Each
    edge runs icp.icp_pairs at the coarse and then at the fine distance, from init_transforms ((E, 4, 4), target ~ T source) or the
    identity; with estimation 'point_to_plane' the caller passes normals, one (n, 3) tensor per cloud (scan preparation is not called
    here).  The information matrices are taken at the fine distance; the node poses are chained from the odometry edges, X_0 = I,
    X_(i+1) = X_i T_(i,i+1)^-1 (a missing odometry edge leaves X_(i+1) = X_i); one optimize_pose_graphs call follows with
    max_correspondence_distance = the fine distance and reference_node = 0 (options: its other criteria and options).  Returns a dict of
    device tensors: poses (K, 4, 4) (cloud frame -> the frame of cloud 0), edges (E, 2), transforms (E, 4, 4), informations (E, 6, 6),
    uncertain (E,) bool, confidence (2, E), kept (E,) bool, fitness (E,) (of the fine ICP), status, info, residuals (of the graph)."""
    from .icp import icp_pairs
    what = 'multiway_registration'
    K = len(clouds)
    if K > _ops.PGO_MAX_NODES:
        raise ValueError('%s: %d clouds (at most %d)' % (what, K, _ops.PGO_MAX_NODES))
    if estimation != 'point_to_point' and normals is None:
        raise ValueError('%s: %s needs the normals of every cloud (scan preparation is not called here)' % (what, estimation))
    dev = device_of(device, clouds)
    pts = gpu_rows_each(clouds, dev, '%s: cloud' % what, _FAMILY)
    if pts:
        dev = pts[0].device
    if edges is None:
        edges = [(i, j) for i in range(K) for j in range(i + 1, K)]
    pairs = [(int(s), int(t)) for s, t in np.asarray(edges, np.int64).reshape(-1, 2).tolist()]
    if any(not (0 <= s < K and 0 <= t < K and s != t) for s, t in pairs):
        raise ValueError('%s: an edge names a cloud outside [0, %d) or joins a cloud with itself' % (what, K))
    if len(pairs) > _ops.PGO_MAX_EDGES:
        raise ValueError('%s: %d edges (at most %d)' % (what, len(pairs), _ops.PGO_MAX_EDGES))
    E = len(pairs)
    srcs, refs = [pts[s] for s, _t in pairs], [pts[t] for _s, t in pairs]
    ref_normals = None if normals is None or estimation == 'point_to_point' else [normals[t] for _s, t in pairs]
    T0 = transforms_of(init_transforms, E, what, dev)
    coarse = icp_pairs(srcs, refs, T0, max_correspondence_distance_coarse, estimation, ref_normals)
    fine = icp_pairs(srcs, refs, coarse['transforms'], max_correspondence_distance_fine, estimation, ref_normals)
    T = fine['transforms']
    info = information_matrix_pairs(srcs, refs, T, max_correspondence_distance_fine)['information']
    uncertain = torch.tensor([t - s != 1 for s, t in pairs], dtype=torch.bool, device=dev)
    poses = [torch.eye(4, dtype=torch.float64, device=dev)]
    odometry = {(s, t): k for k, (s, t) in reversed(list(enumerate(pairs)))}           # (the first of duplicate edges)
    for i in range(K - 1):
        k = odometry.get((i, i + 1))
        poses.append(poses[i] if k is None else poses[i] @ _rigid_inverse(T[k]))
    e = torch.tensor(pairs, dtype=torch.int64, device=dev).reshape(-1, 2)
    graph = dict(poses=torch.stack(poses[:K]) if K else torch.zeros((0, 4, 4), dtype=torch.float64, device=dev), edges=e, transforms=T,
                 informations=info, uncertain=uncertain)
    out = optimize_pose_graphs([graph], 0 if K else -1, dev, max_correspondence_distance=max_correspondence_distance_fine, **options)
    return {'poses': out['poses'][0], 'edges': e, 'transforms': T, 'informations': info, 'uncertain': uncertain,
            'confidence': out['confidence'][0], 'kept': out['kept'][0], 'fitness': fine['fitness'], 'status': out['status'],
            'info': out['info'], 'residuals': out['residuals']}
