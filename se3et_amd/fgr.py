"""Fast Global Registration on the device for batched pairs: Open3D's registration_fgr_based_on_correspondence and
registration_fgr_based_on_feature_matching (Zhou, Park, Koltun, ECCV 2016) as three HIP launches for up to SE3_PAIR_MAX_PAIRS pairs
(csrc/fgr.hip, csrc/fgr_core.h), in place of one pair at a time on the host.  The coarse method that needs no hypotheses and no inlier
threshold, beside ransac.ransac_pairs.

  fgr_pairs(src_list, ref_list, correspondences, ...)                                  dict of device tensors for P pairs
  fgr_from_feats_pairs(src_points_list, ref_points_list, src_feats_list, ref_feats_list, ...)   mutual feature matching, then fgr_pairs
  registration_fgr_based_on_correspondence(src_points, ref_points, correspondences, ...)        one pair, numpy in, (4, 4) numpy out
  registration_fgr_based_on_feature_matching(src_points, ref_points, src_feats, ref_feats, ...) one pair, numpy in, (4, 4) numpy out

GPU tensors only (there is no CPU path), any number of pairs per call, chunked at the library's SE3_PAIR_MAX_PAIRS pairs per launch
sequence.  Nothing is read back: the host synchronises only where stacking the inputs does.

Contract (one pair; csrc/fgr.hip carries the same text).  Source S (ns, 3) and reference R (nr, 3), float32 or float64, promoted to
float64 on load.  Correspondences C are (K, 2) int64 rows of (src row, ref row), as ransac_pairs takes them.  All arithmetic is float64
with contraction off.  The result is T with ref ~ T src.
  0. Refusals.  A non-finite coordinate in either cloud sets the nonfinite bit and gives a NaN transform, like ICP.  An empty cloud or
     K = 0 sets `empty` and gives the identity.  An index of C outside its cloud sets bad_index and gives a NaN transform.  They are
     tested in this order and the first that holds is the only one set (an empty cloud has no index to be wrong about).
  1. Tuple test (tuple_test; Open3D's AdvancedMatching).  Trials are t = 0 .. 100 K - 1.  Trial t draws
       a_j = ((splitmix64(splitmix64(seed) + 3 t + j) >> 32) * K) >> 32,  j = 0, 1, 2                      (uint64 wrap-around)
     which is ransac.sample_indices(seed, K, 100 K, 3)[t]: RANSAC's sampler, one text in the library.  The squared edges ls_e, lr_e are
     taken in each cloud between the points of rows C[a_0], C[a_1], C[a_2], for the edges (0, 1), (1, 2), (2, 0), each as
     (dx dx + dy dy) + dz dz.  The trial is accepted iff for all three edges ls_e tau2 < lr_e and lr_e tau2 < ls_e, with
     tau2 = tuple_scale tuple_scale rounded once.  The first maximum_tuple_count accepted trials in trial order each append C[a_0],
     C[a_1], C[a_2] to the working list C'; duplicates are kept.  Without the tuple test C' = C.
     Differences from Open3D: the random stream (Open3D's is not reproducible); and the comparison, which is on squared lengths in place
     of li tau < lj && lj < li / tau: no root and no division, so host and device agree to the bit.  Degenerate triples reject themselves
     through the strict inequalities.
  2. Too few correspondences.  |C'| < 10 gives the identity and sets too_few.
  3. Normalisation (NormalizePointCloud, over ALL rows of both clouds, not only the matched ones).  Each cloud's mean is taken in the
     order of ICP's sums (lane l of 256 adds rows l, l + 256, .. serially, then a fixed tree over the lanes) and divided by the row count;
     the clouds are centred; scale = sqrt(max over both clouds of the centred squared norm (dx dx + dy dy) + dz dz).
     use_absolute_scale False: g = scale, mu = 1; True: g = 1, mu = scale.  The centred points are divided by g.  A scale that is not
     > 0 gives the identity and sets `singular`.
  4. GNC loop (OptimizePairwiseRegistration).  The REFERENCE cloud is the moving one.  Start from M = I; run it = 0 ..
     iteration_number - 1.  For each row of C', with p the normalised source point and q' = M q the moved normalised reference point
     ((M0 q0 + M1 q1) + M2 q2, then + M3): d = p - q'; the weight is w = (mu / (d.d + mu))^2; each coordinate a has a Jacobian row J with
     J[3 + a] = -1, J[(a+1)%3] = -q'[(a+2)%3] and J[(a+2)%3] = q'[(a+1)%3].  The sums A = sum w J J^T (21 terms) and b = sum w J d_a
     (6 terms) are taken in the order of ICP's sums.  A x = -b is solved by ICP's 6x6 Cholesky factorisation; a failure sets `singular`,
     takes the identity update, and the loop goes on.  The update is U = [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5], then M <- U M.  After the
     update: if decrease_mu and it % 4 == 0 and mu > maximum_correspondence_distance, then mu <- mu / division_factor.  As in Open3D,
     maximum_correspondence_distance is compared in NORMALISED units unless use_absolute_scale: with the default it is a share of the
     clouds' radius, not a length.
     Difference from Open3D: q' is recomputed from M each iteration; Open3D moves a copy incrementally, so the rounding differs.
     Step angles.  A numpy sketch of this contract took steps of up to 1.14 rad on clean flat clouds, so ICP's 1 rad refusal is wrong
     here.  The sine and cosine of an angle with |a| < 4 come from ICP's series at a / 4, followed by two double-angle steps
     (s <- (2 s) c, c <- c c - s s), every operation rounded on its own, so host and device agree to the bit.  A non-finite angle, or
     |a| >= 4, sets step_refused; the pair then ends with the M it had.
  5. Original scale and direction.  M maps ref to src, so A_R = M_R and A_t = -M_R mean_R + g M_t + mean_S.  The rigid inverse is
     returned in closed form, (A_R^T, -A_R^T A_t).
  6. Evaluation (Open3D's returned RegistrationResult).  fitness and inlier_rmse of T at maximum_correspondence_distance are taken on
     the original clouds through the ICP entry with max_iteration = 0 (ops.icp_stack: icp.icp_pairs' evaluation); a refused pair has 0, 0.
  Results are bit-identical from run to run, and for a pair alone or in any batch.  ops.FGR_STATUS names the status bits."""
import numpy as np
import torch

from . import ops as _ops
from .stacking import chunks, device_of, gpu_rows_each, identities, lengths, stack, upload

_FAMILY = 'Fast Global Registration'


def _options(what, maximum_correspondence_distance, division_factor, iteration_number, tuple_scale, maximum_tuple_count):
    r, f, s = float(maximum_correspondence_distance), float(division_factor), float(tuple_scale)
    if not (np.isfinite(r) and r > 0):
        raise ValueError('%s: maximum_correspondence_distance %r is not a finite, positive number' % (what, maximum_correspondence_distance))
    if not (np.isfinite(f) and f >= 1):
        raise ValueError('%s: division_factor %r is not a finite number >= 1' % (what, division_factor))
    if not 0 <= int(iteration_number) <= _ops.FGR_MAX_ITERATION:
        raise ValueError('%s: iteration_number %r not in [0, %d]' % (what, iteration_number, _ops.FGR_MAX_ITERATION))
    if not 0.0 < s <= 1.0:
        raise ValueError('%s: tuple_scale %r is not in (0, 1]' % (what, tuple_scale))
    if not 0 <= int(maximum_tuple_count) <= _ops.FGR_MAX_TUPLE_COUNT:
        raise ValueError('%s: maximum_tuple_count %r not in [0, %d]' % (what, maximum_tuple_count, _ops.FGR_MAX_TUPLE_COUNT))


@torch.no_grad()
def fgr_pairs(src_list, ref_list, correspondences, maximum_correspondence_distance=0.025, division_factor=1.4, use_absolute_scale=False,
              decrease_mu=True, iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000, tuple_test=True, seed=0, evaluate=True,
              return_tuples=False, device=None):
    """Fast Global Registration of P pairs (the module text has the contract).  src_list / ref_list: (n, 3) float32 or float64 GPU
    tensors; correspondences: per pair a (K_p, 2) int64 GPU tensor of (src row, ref row).  The options are Open3D's
    FastGlobalRegistrationOption, plus the sampler's seed.  Returns a dict of device tensors: transforms (P, 4, 4) float64 (ref ~ T src),
    status (P,) int32 (a sum of the ops.FGR_STATUS bits; a refused pair has a NaN transform and does not raise), num_correspondences
    (|C'|) and num_tuples (P,) int32, mu (P,) float64 (its last value), and with evaluate fitness / inlier_rmse (P,) float64.
    return_tuples adds tuples, per pair the (|C'|, 2) int64 working list, and trials, per pair the kept trials' indices; cutting them to
    their lengths reads the counts back, the call's one synchronisation of its own."""
    what = 'fgr_pairs'
    P = len(src_list)
    if len(ref_list) != P or len(correspondences) != P:
        raise ValueError('%s: one source cloud, one reference cloud and one correspondence table per pair' % what)
    _options(what, maximum_correspondence_distance, division_factor, iteration_number, tuple_scale, maximum_tuple_count)
    dev = device_of(device, src_list, ref_list)
    srcs = gpu_rows_each(src_list, dev, '%s: source cloud' % what, _FAMILY)
    refs = gpu_rows_each(ref_list, dev, '%s: reference cloud' % what, _FAMILY)
    corrs = gpu_rows_each(correspondences, dev, '%s: correspondences' % what, _FAMILY, 2, (torch.int64,))
    if srcs:
        dev = srcs[0].device
    r = float(maximum_correspondence_distance)
    parts, tuples, trials = [], [], []
    for a, b in chunks(P):
        s, sl = stack(srcs[a:b]), lengths(srcs[a:b])
        q, ql = stack(refs[a:b]), lengths(refs[a:b])
        c, cl = stack(corrs[a:b]), lengths(corrs[a:b])
        out = _ops.fgr_stack(s, sl, q, ql, c, cl, r, division_factor, use_absolute_scale, decrease_mu, iteration_number, tuple_scale,
                             maximum_tuple_count, tuple_test, seed, return_tuples)
        if evaluate:
            ev = _ops.icp_stack(_ops.pair_grid_build(q, ql, identities(b - a), r), s, sl, out['transforms'], r, 'point_to_point', max_iteration=0)
            out['fitness'], out['inlier_rmse'] = ev['fitness'], ev['inlier_rmse']
        if return_tuples:
            nc, nt = out['num_correspondences'].cpu().tolist(), out['num_tuples'].cpu().tolist()
            if 'tuples' in out:
                tuples += [t[:n] for t, n in zip(out.pop('tuples'), nc)]
                trials += [t[:n] for t, n in zip(out.pop('trials'), nt)]
            else:
                tuples += [t[:n] for t, n in zip(corrs[a:b], nc)]
                trials += [t.new_zeros((0,)) for t in corrs[a:b]]
        parts.append(out)
    if not parts:
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        parts = [{'transforms': torch.empty((0, 4, 4), **f64), 'status': torch.empty((0,), **i32),
                  'num_correspondences': torch.empty((0,), **i32), 'num_tuples': torch.empty((0,), **i32), 'mu': torch.empty((0,), **f64)}]
        if evaluate:
            parts[0].update(fitness=torch.empty((0,), **f64), inlier_rmse=torch.empty((0,), **f64))
    result = {k: stack([p[k] for p in parts]) for k in parts[0]}
    if return_tuples:
        result['tuples'], result['trials'] = tuples, trials
    return result


@torch.no_grad()
def fgr_from_feats_pairs(src_points_list, ref_points_list, src_feats_list, ref_feats_list, **options):
    """Fast Global Registration from descriptors for P pairs (Open3D's registration_fgr_based_on_feature_matching): its cross-checked
    initial matching is feature_matching.extract_correspondences_from_feats_pairs(mutual=True), the mutual nearest neighbours in feature
    space; fgr_pairs(**options) runs on them.  Points (n, 3) float32 / float64 and features (n, C) float32 GPU tensors.  Returns the dict
    of fgr_pairs plus correspondences: per pair the (K_p, 2) int64 (src, ref) table."""
    from .feature_matching import extract_correspondences_from_feats_pairs
    P = len(src_points_list)
    if not (len(ref_points_list) == len(src_feats_list) == len(ref_feats_list) == P):
        raise ValueError('fgr_from_feats_pairs: one src / ref point and feature array per pair')
    for p in range(P):
        if src_points_list[p].shape[0] != src_feats_list[p].shape[0] or ref_points_list[p].shape[0] != ref_feats_list[p].shape[0]:
            raise ValueError('fgr_from_feats_pairs: pair %d has a different number of points and features' % p)
    ref_idx, src_idx = extract_correspondences_from_feats_pairs(ref_feats_list, src_feats_list, mutual=True) if P else ([], [])
    tables = [torch.stack([s, r], 1) for s, r in zip(src_idx, ref_idx)]
    out = fgr_pairs(src_points_list, ref_points_list, tables, **options)
    out['correspondences'] = tables
    return out


def registration_fgr_based_on_correspondence(src_points, ref_points, correspondences, device=None, **options):
    """One pair, numpy in and out (the arrays are uploaded inside the call): the (4, 4) float64 transform src -> ref from the (K, 2)
    (src row, ref row) table.  options: those of fgr_pairs.  The argument order follows
    ransac.registration_with_ransac_from_correspondences: source first."""
    options = dict(options, evaluate=False, return_tuples=False)
    corr = upload(np.asarray(correspondences).reshape(-1, 2), device, 2, np.int64)
    return fgr_pairs([upload(src_points, device)], [upload(ref_points, device)], [corr], **options)['transforms'][0].cpu().numpy()


def registration_fgr_based_on_feature_matching(src_points, ref_points, src_feats, ref_feats, device=None, **options):
    """One pair, numpy in and out: the (4, 4) float64 transform src -> ref from the clouds' descriptors ((n, C), rows are points)."""
    options = dict(options, evaluate=False, return_tuples=False)
    src_feats, ref_feats = np.asarray(src_feats), np.asarray(ref_feats)
    feats = lambda a: upload(a, device, a.shape[-1], np.float32)
    out = fgr_from_feats_pairs([upload(src_points, device)], [upload(ref_points, device)], [feats(src_feats)], [feats(ref_feats)], **options)
    return out['transforms'][0].cpu().numpy()
