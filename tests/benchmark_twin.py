"""Float64 numpy restatement of se3et_amd.benchmark's contract (eval.py's per-pair metrics and summaries), for the CPU tests and as the
reading of the kernels in csrc/benchmark.hip.  No reference code: each function restates the formula it names."""
import numpy as np

KEYS = ('PIR', 'PMR>0', 'PMR>=0.1', 'PMR>=0.3', 'PMR>=0.5', 'FMR', 'IR', 'OV', 'FMR_std', 'RR', 'mean_RRE', 'mean_RTE', 'median_RRE',
        'median_RTE')


def _mean(x):
    return float(np.sum(np.asarray(x, np.float64)) / len(x)) if len(x) else float('nan')


def _median(x):
    return float(np.median(np.asarray(x, np.float64))) if len(x) else float('nan')


def _std(x):
    return float(np.std(np.asarray(x, np.float64))) if len(x) else float('nan')


def nearest_sq_distances(q, s, chunk=2048):
    """Squared distance from every q to its nearest s (float64, brute force); inf without s."""
    q, s = np.asarray(q, np.float64), np.asarray(s, np.float64)
    out = np.full(len(q), np.inf)
    if len(s) == 0:
        return out
    for a in range(0, len(q), chunk):
        d = ((q[a:a + chunk, None, :] - s[None, :, :]) ** 2).sum(-1)
        out[a:a + chunk] = d.min(1)
    return out


def correspondences(ref, src, T, r):
    """evaluate_correspondences: overlap (nearest transformed src within r), inlier_ratio, residual, num_corr; NaN means without points."""
    T = np.asarray(T, np.float64)
    ref = np.asarray(ref, np.float64)
    moved = np.asarray(src, np.float64) @ T[:3, :3].T + T[:3, 3]
    n = len(ref)
    if n == 0:
        return dict(overlap=float('nan'), inlier_ratio=float('nan'), residual=float('nan'), num_corr=0)
    d2 = ((ref - moved) ** 2).sum(1)
    return dict(overlap=float(np.count_nonzero(nearest_sq_distances(ref, moved) < r * r)) / n,
                inlier_ratio=float(np.count_nonzero(d2 < r * r)) / n, residual=float(np.sqrt(d2).sum() / n), num_corr=n)


def sparse(ref_idx, src_idx, gt, N, M):
    """evaluate_sparse_correspondences with set semantics and the + 1e-12 denominators."""
    gt = np.asarray(gt, np.int64).reshape(-1, 2)
    g = set(map(tuple, gt.tolist()))
    p = set(zip(np.asarray(ref_idx).tolist(), np.asarray(src_idx).tolist()))
    pos = g & p
    rows = len({a for a, _ in pos}) / (len({a for a, _ in g}) + 1e-12)
    cols = len({b for _, b in pos}) / (len({b for _, b in g}) + 1e-12)
    return dict(precision=len(pos) / (len(p) + 1e-12), recall=len(pos) / (len(g) + 1e-12), hit_ratio=0.5 * (rows + cols))


def mat2quat(R):
    """nibabel.quaternions.mat2quat (Bar-Itzhack): (w, x, y, z) of K's largest eigenvalue, w >= 0."""
    Qxx, Qyx, Qzx, Qxy, Qyy, Qzy, Qxz, Qyz, Qzz = np.asarray(R, np.float64).flat
    K = np.array([[Qxx - Qyy - Qzz, 0, 0, 0],
                  [Qyx + Qxy, Qyy - Qxx - Qzz, 0, 0],
                  [Qzx + Qxz, Qzy + Qyz, Qzz - Qxx - Qyy, 0],
                  [Qyz - Qzy, Qzx - Qxz, Qxy - Qyx, Qxx + Qyy + Qzz]]) / 3.0
    vals, vecs = np.linalg.eigh(K)
    q = vecs[[3, 0, 1, 2], np.argmax(vals)]
    return -q if q[0] < 0 else q


def transform_error(T, C, E):
    """compute_transform_error: e = [t, q_xyz] of inv(T) E, e^T C e / C[0, 0]."""
    rel = np.linalg.inv(np.asarray(T, np.float64)) @ np.asarray(E, np.float64)
    e = np.concatenate([rel[:3, 3], mat2quat(rel[:3, :3])[1:]])
    C = np.asarray(C, np.float64)
    return float((e @ C) @ e / C[0, 0])


def registration_error(T, E):
    """compute_registration_error: RRE (degrees, arccos argument clipped) and RTE."""
    T, E = np.asarray(T, np.float64), np.asarray(E, np.float64)
    x = np.clip(0.5 * (np.trace(E[:3, :3].T @ T[:3, :3]) - 1.0), -1.0, 1.0)
    return float(180.0 * np.arccos(x) / np.pi), float(np.linalg.norm(T[:3, 3] - E[:3, 3]))


def group_summary(precision, ir, ov, accepted_mask, reg_mask, rre, rte, ir_thr):
    """One group's row (KEYS): registration over reg_mask pairs, accepted_mask of those accepted."""
    precision, ir, ov = (np.asarray(v, np.float64) for v in (precision, ir, ov))
    acc = np.asarray(accepted_mask, bool)
    fmr = (ir >= ir_thr).astype(np.float64)
    rr = np.asarray(rre, np.float64)[acc]
    rt = np.asarray(rte, np.float64)[acc]
    return {'PIR': _mean(precision), 'PMR>0': _mean(precision > 0), 'PMR>=0.1': _mean(precision >= 0.1),
            'PMR>=0.3': _mean(precision >= 0.3), 'PMR>=0.5': _mean(precision >= 0.5), 'FMR': _mean(fmr), 'IR': _mean(ir),
            'OV': _mean(ov), 'FMR_std': _std(fmr), 'RR': _mean(acc[np.asarray(reg_mask, bool)]), 'mean_RRE': _mean(rr),
            'mean_RTE': _mean(rt), 'median_RRE': _median(rr), 'median_RTE': _median(rt)}


def summary_3dmatch(scenes, ir_thr, rmse_thr):
    """scenes: [(name, dict of per-pair arrays precision, inlier_ratio, overlap, err, rre, rte, is_gt)] -> (per-scene rows, overall)."""
    rows = {}
    for name, d in scenes:
        is_gt = np.asarray(d['is_gt'], bool)
        acc = is_gt & (np.asarray(d['err'], np.float64) < rmse_thr ** 2)
        rows[name] = group_summary(d['precision'], d['inlier_ratio'], d['overlap'], acc, is_gt, d['rre'], d['rte'], ir_thr)
    overall = {k: _mean([r[k] for r in rows.values()]) for k in KEYS}
    overall['FMR_std'] = _std([r['FMR'] for r in rows.values()])
    return rows, overall


def summary_kitti(d, ir_thr, rre_thr, rte_thr):
    """All pairs as one group: accepted iff rre < rre_thr and rte < rte_thr."""
    rre, rte = np.asarray(d['rre'], np.float64), np.asarray(d['rte'], np.float64)
    acc = (rre < rre_thr) & (rte < rte_thr)
    return group_summary(d['precision'], d['inlier_ratio'], d['overlap'], acc, np.ones(len(acc), bool), rre, rte, ir_thr)
