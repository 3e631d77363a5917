"""Seeded inputs of the ICP tests, the twin's run over them, and the call of se3_debug_icp_host.

Every family is a wavy height-field sheet of unit extent (a surface that fixes all six degrees of freedom), with its analytic normals.
case(name, dtype) returns the inputs ROUNDED to the dtype the library will read (the twin sees the same values) and the twin's result,
and asserts the two margins under which the library must choose the twin's correspondence sets at every evaluation:
  - no nearest distance within 1e-7 of the threshold r,
  - no row whose nearest and second-nearest reference points are closer than 1e-9 in distance.
A seed that misses a margin fails here, loudly."""
import ctypes
import functools

import numpy as np

from icp_twin import icp as twin_icp

THRESHOLD_MARGIN, GAP_MARGIN = 1e-7, 1e-9
MODES = {'point_to_point': 0, 'point_to_plane': 1}


def _height(x, y):
    return 0.08 * np.sin(5.0 * x) * np.cos(4.0 * y) + 0.05 * np.cos(7.0 * x + 3.0 * y) + 0.1 * x * y


def sheet(rng, n, x0=0.0):
    """n points of the sheet over [x0, x0 + 1] x [0, 1] and their unit normals (z up)."""
    x, y = x0 + rng.random(n), rng.random(n)
    h = 1e-6
    zx = (_height(x + h, y) - _height(x - h, y)) / (2 * h)
    zy = (_height(x, y + h) - _height(x, y - h)) / (2 * h)
    nrm = np.stack([-zx, -zy, np.ones(n)], 1)
    return np.stack([x, y, _height(x, y)], 1), nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def rigid(rng, degrees, shift):
    """A rotation of `degrees` about a random axis and a translation of length `shift` in a random direction."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(degrees)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    t = rng.normal(size=3)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    T[:3, 3] = shift * t / np.linalg.norm(t)
    return T


def _pair(seed, nref, nsrc, partial):
    """ref, normals, src, gt (ref ~ gt src), T0 = a 4 degree / 3 cm error on gt."""
    rng = np.random.default_rng(seed)
    ref, nrm = sheet(rng, nref)
    if partial:                                        # an independent sample of the same surface, shifted along x: partial overlap
        on_ref, _ = sheet(rng, nsrc, x0=partial)
    else:                                              # a subset of the reference points
        on_ref = ref[rng.permutation(nref)[:nsrc]]
    on_ref = on_ref + 0.002 * rng.normal(size=on_ref.shape)
    gt = rigid(rng, 25.0, 0.5)
    inv = np.linalg.inv(gt)
    src = on_ref @ inv[:3, :3].T + inv[:3, 3]
    T0 = rigid(rng, 4.0, 0.03) @ gt
    return ref, nrm, src, gt, T0


# name -> (seed, reference points, source points, partial-overlap shift, r)
FAMILIES = {'sheet700': (1, 700, 650, 0.0, 0.15), 'sheet2048': (1, 2048, 1900, 0.0, 0.10), 'partial1500': (2, 1500, 1400, 0.4, 0.08)}


@functools.lru_cache(maxsize=None)
def case(name, mode, dtype):
    """-> dict(src, ref, normals, T0, gt, r, twin): arrays of `dtype` ('float32' / 'float64'; T0 and gt stay float64), read-only."""
    seed, nref, nsrc, partial, r = FAMILIES[name]
    ref, nrm, src, gt, T0 = _pair(seed, nref, nsrc, partial)
    ref, nrm, src = (np.ascontiguousarray(a.astype(dtype)) for a in (ref, nrm, src))
    twin = twin_icp(src, ref, T0, r, mode, nrm)
    for k, ev in enumerate(twin['evaluations']):
        assert ev['threshold_margin'] >= THRESHOLD_MARGIN, '%s %s %s: evaluation %d has a distance %.1e from r (another seed)' % (
            name, mode, dtype, k, ev['threshold_margin'])
        assert ev['gap_margin'] >= GAP_MARGIN, '%s %s %s: evaluation %d has a nearest / second-nearest gap of %.1e (another seed)' % (
            name, mode, dtype, k, ev['gap_margin'])
    for a in (ref, nrm, src, gt, T0):
        a.setflags(write=False)
    return {'src': src, 'ref': ref, 'normals': nrm, 'T0': T0, 'gt': gt, 'r': r, 'twin': twin}


def host_icp(src, ref, T0, r, mode, normals=None, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, trace=False):
    """se3_debug_icp_host on numpy arrays (src and ref of one dtype, float32 or float64).  -> dict(transform (4, 4), fitness, rmse,
    iterations, converged, status, correspondences (n,), and with trace the (max_iteration + 1, n) table, -2 where no evaluation was made)."""
    from se3et_amd._lib import check, lib
    src, ref = np.ascontiguousarray(src).reshape(-1, 3), np.ascontiguousarray(ref).reshape(-1, 3)
    assert src.dtype == ref.dtype and src.dtype in (np.float32, np.float64)
    nrm = None if normals is None else np.ascontiguousarray(normals).reshape(-1, 3)
    assert nrm is None or (nrm.dtype in (np.float32, np.float64) and nrm.shape == ref.shape)
    T0 = np.ascontiguousarray(T0, np.float64).reshape(4, 4)
    T, fit, rmse = np.zeros((4, 4)), ctypes.c_double(), ctypes.c_double()
    it, conv, status = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    corr = np.full((len(src),), -2, np.int64)
    tr = np.full((max(max_iteration, 0) + 1, len(src)), -2, np.int64) if trace else None
    ptr = lambda a: None if a is None else a.ctypes.data if a.size else ctypes.addressof(_dummy)
    check(lib().se3_debug_icp_host(ptr(src), len(src), ptr(ref), len(ref), int(src.dtype == np.float64), ptr(nrm),
                                   0 if nrm is None else int(nrm.dtype == np.float64), ptr(T0), float(r), MODES[mode], relative_fitness,
                                   relative_rmse, max_iteration, ptr(T), ctypes.byref(fit), ctypes.byref(rmse), ctypes.byref(it),
                                   ctypes.byref(conv), ctypes.byref(status), ptr(corr), ptr(tr)), 'se3_debug_icp_host')
    out = {'transform': T, 'fitness': fit.value, 'rmse': rmse.value, 'iterations': it.value, 'converged': conv.value, 'status': status.value,
           'correspondences': corr}
    if trace:
        out['trace'] = tr
    return out


_dummy = (ctypes.c_double * 8)()
