"""Seeded inputs of the weighted ICP tests (robust loss kernels, generalized ICP), the twin's run over them (tests/icp_robust_twin.py) and
the call of se3_debug_icp_weighted_host.

Clean families: the three of tests/icp_fixture.py, with source normals added: the analytic sheet normal at the source point's place on
the sheet, turned into the source frame.
Outlier family: icp_fixture._pair(seed, 700, 650, 0.0) with r = 0.15, in which 130 source rows -- default_rng(1000 + seed)
.permutation(650)[:130] -- are lifted off the sheet by 0.03 + 0.03 u along the sheet frame's z (u uniform from the same generator) before
the move into the source frame: every one stays a correspondence at r, and pulls a plain least-squares step.
case(...) returns the inputs ROUNDED to the dtype the library will read and the twin's result, and asserts icp_fixture's two margins at
every evaluation.  assert_robust_is_nearer(seed) is the behaviour the losses exist for, on the twin alone."""
import ctypes
import functools

import numpy as np

import icp_fixture as F
import icp_robust_twin as W

ESTIMATORS = {'point_to_point': 0, 'point_to_plane': 1, 'generalized': 2}
LOSS_IDS = {None: -1, 'l2': 0, 'huber': 1, 'cauchy': 2, 'gm': 3, 'tukey': 4}
# the width of every loss on these unit-scale sheets with 2 mm of noise and outliers 3 to 6 cm off the surface
LOSS_K = {'l2': 1.0, 'huber': 0.01, 'cauchy': 0.01, 'gm': 1e-4, 'tukey': 0.02}
FAMILIES = dict(F.FAMILIES, outlier700=(1, 700, 650, 0.0, 0.15))
# (estimator, loss) for which a robust run must end nearer the ground truth than l2 on the outlier family.  gm and tukey at these widths
# are left out for point-to-point and generalized: their weight is already near zero at the 3 cm / 4 degree start.
ROBUST_WINS = [('point_to_plane', l) for l in ('huber', 'cauchy', 'gm', 'tukey')] + \
              [(e, l) for e in ('point_to_point', 'generalized') for l in ('huber', 'cauchy')]


def sheet_normals_at(points):
    """The sheet's analytic unit normals (z up) at the (x, y) of points given in the sheet's frame."""
    x, y, h = points[:, 0], points[:, 1], 1e-6
    zx = (F._height(x + h, y) - F._height(x - h, y)) / (2 * h)
    zy = (F._height(x, y + h) - F._height(x, y - h)) / (2 * h)
    nrm = np.stack([-zx, -zy, np.ones(len(points))], 1)
    return nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def source_normals(src, gt):
    on_sheet = src @ gt[:3, :3].T + gt[:3, 3]
    return sheet_normals_at(on_sheet) @ gt[:3, :3]                     # rows n^T R = (R^T n)^T: turned into the source frame


def outlier_pair(seed):
    """ref, ref normals, src, src normals, gt, T0, the lifted rows."""
    ref, nrm, src, gt, T0 = F._pair(seed, 700, 650, 0.0)
    rng = np.random.default_rng(1000 + seed)
    rows = rng.permutation(650)[:130]
    on_sheet = src @ gt[:3, :3].T + gt[:3, 3]
    src_nrm = sheet_normals_at(on_sheet) @ gt[:3, :3]
    on_sheet[rows, 2] += 0.03 + 0.03 * rng.random(130)
    inv = np.linalg.inv(gt)
    return ref, nrm, on_sheet @ inv[:3, :3].T + inv[:3, 3], src_nrm, gt, T0, rows


@functools.lru_cache(maxsize=None)
def inputs(name, dtype):
    """-> dict(src, ref, normals, src_normals, T0, gt, r) of `dtype` (T0 and gt stay float64), read-only."""
    seed, nref, nsrc, partial, r = FAMILIES[name]
    if name.startswith('outlier'):
        ref, nrm, src, src_nrm, gt, T0, _rows = outlier_pair(seed)
    else:
        ref, nrm, src, gt, T0 = F._pair(seed, nref, nsrc, partial)
        src_nrm = source_normals(src, gt)
    ref, nrm, src, src_nrm = (np.ascontiguousarray(a.astype(dtype)) for a in (ref, nrm, src, src_nrm))
    for a in (ref, nrm, src, src_nrm, gt, T0):
        a.setflags(write=False)
    return {'src': src, 'ref': ref, 'normals': nrm, 'src_normals': src_nrm, 'T0': T0, 'gt': gt, 'r': r}


def twin_of(c, mode, loss, **kw):
    return W.icp(c['src'], c['ref'], c['T0'], c['r'], mode, c['normals'], c['src_normals'], loss, LOSS_K[loss], **kw)


@functools.lru_cache(maxsize=None)
def case(name, mode, loss, dtype):
    """inputs(name, dtype) with `twin`: the twin's run under (mode, loss, LOSS_K[loss]), its margins asserted."""
    c = dict(inputs(name, dtype))
    twin = twin_of(c, mode, loss)
    for k, ev in enumerate(twin['evaluations']):
        assert ev['threshold_margin'] >= F.THRESHOLD_MARGIN, '%s %s %s %s: evaluation %d has a distance %.1e from r (another seed)' % (
            name, mode, loss, dtype, k, ev['threshold_margin'])
        assert ev['gap_margin'] >= F.GAP_MARGIN, '%s %s %s %s: evaluation %d has a nearest / second-nearest gap of %.1e (another seed)' % (
            name, mode, loss, dtype, k, ev['gap_margin'])
    c['twin'] = twin
    return c


def errors(T, gt):
    """(rotation angle in rad, translation distance) of T from gt."""
    R = T[:3, :3].T @ gt[:3, :3]
    return float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))), float(np.linalg.norm(T[:3, 3] - gt[:3, 3]))


def assert_robust_is_nearer(seed):
    """On the outlier family of `seed`, for every (estimator, loss) of ROBUST_WINS: the TWIN's robust result is nearer the ground truth
    than the twin's l2 result, in rotation angle and in translation distance.  -> the table of errors."""
    ref, nrm, src, src_nrm, gt, T0, _rows = outlier_pair(seed)
    c = {'src': src, 'ref': ref, 'normals': nrm, 'src_normals': src_nrm, 'T0': T0, 'r': 0.15}
    plain = {e: errors(twin_of(c, e, 'l2')['transform'], gt) for e in ESTIMATORS}
    table = {}
    for e, l in ROBUST_WINS:
        got = errors(twin_of(c, e, l)['transform'], gt)
        table[(e, l)] = got + plain[e]
        assert got[0] < plain[e][0] and got[1] < plain[e][1], 'seed %d, %s %s: %.2e rad %.2e against l2 %.2e rad %.2e (another seed)' % (
            (seed, e, l) + got + plain[e])
    return table


def host_weighted_icp(src, ref, T0, r, mode, normals=None, src_normals=None, loss=None, loss_k=1.0, epsilon=1e-3, relative_fitness=1e-6,
                      relative_rmse=1e-6, max_iteration=30, trace=False, loss_id=None):
    """se3_debug_icp_weighted_host on numpy arrays, as icp_fixture.host_icp: -> dict(transform, fitness, rmse, iterations, converged,
    status, correspondences, and with trace the (max_iteration + 1, n) table).  loss_id: a raw id in place of the name."""
    from se3et_amd._lib import check, lib
    src, ref = np.ascontiguousarray(src).reshape(-1, 3), np.ascontiguousarray(ref).reshape(-1, 3)
    assert src.dtype == ref.dtype and src.dtype in (np.float32, np.float64)
    nrm = None if normals is None else np.ascontiguousarray(normals).reshape(-1, 3)
    snr = None if src_normals is None else np.ascontiguousarray(src_normals).reshape(-1, 3)
    assert nrm is None or (nrm.dtype in (np.float32, np.float64) and nrm.shape == ref.shape)
    assert snr is None or (snr.dtype in (np.float32, np.float64) and snr.shape == src.shape)
    T0 = np.ascontiguousarray(T0, np.float64).reshape(4, 4)
    T, fit, rmse = np.zeros((4, 4)), ctypes.c_double(), ctypes.c_double()
    it, conv, status = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    corr = np.full((len(src),), -2, np.int64)
    tr = np.full((max(max_iteration, 0) + 1, len(src)), -2, np.int64) if trace else None
    ptr = lambda a: None if a is None else a.ctypes.data if a.size else ctypes.addressof(F._dummy)
    elem = lambda a: 0 if a is None else int(a.dtype == np.float64)
    check(lib().se3_debug_icp_weighted_host(ptr(src), len(src), ptr(ref), len(ref), elem(src), ptr(nrm), elem(nrm), ptr(snr), elem(snr), ptr(T0),
                                            float(r), ESTIMATORS[mode], LOSS_IDS[loss] if loss_id is None else loss_id, float(loss_k),
                                            float(epsilon), relative_fitness, relative_rmse, max_iteration, ptr(T), ctypes.byref(fit),
                                            ctypes.byref(rmse), ctypes.byref(it), ctypes.byref(conv), ctypes.byref(status), ptr(corr), ptr(tr)),
          'se3_debug_icp_weighted_host')
    out = {'transform': T, 'fitness': fit.value, 'rmse': rmse.value, 'iterations': it.value, 'converged': conv.value, 'status': status.value,
           'correspondences': corr}
    if trace:
        out['trace'] = tr
    return out
