"""Seeded inputs of the coloured ICP tests, the twin's run over them (tests/colored_icp_twin.py) and the calls of
se3_debug_color_gradient_host and se3_debug_icp_colored_host.

Families: the three sheets of tests/icp_fixture.py carrying a smooth texture, and `flat`: an exact plane z = 0 whose texture varies in
both in-plane directions, which geometry alone cannot register.  The texture's three channels are products and sums of sinusoids of
wavelength 0.6 to 0.8 over the unit sheet: several times the gradient radius of every family (GRADIENT_RADIUS, 0.07 to 0.12, about the
reach of a row's 30 nearest), and the initial in-plane offset (3 cm and 4 degrees on the sheets, 5 cm on the plane) stays below a quarter
of it.  A source row's colour is the texture at its place on the sheet.
case(...) returns the inputs ROUNDED to the dtype the library will read and the twin's result, and asserts icp_fixture's two margins at
every evaluation and the gradient search's two margins (colored_icp_twin.gradients)."""
import ctypes
import functools

import numpy as np

import colored_icp_twin as C
import icp_fixture as F
from icp_robust_fixture import LOSS_IDS, LOSS_K

COLORED = 3                                        # SE3_ICP_COLORED
LOSSES = (None, 'l2', 'huber', 'tukey')
# name -> (seed, reference points, source points, partial-overlap shift, r); flat: an exact plane
FAMILIES = dict(F.FAMILIES, flat=(7, 800, 700, 0.0, 0.10))
GRADIENT_RADIUS = {'sheet700': 0.12, 'sheet2048': 0.07, 'partial1500': 0.08, 'flat': 0.10}
GRADIENT_MARGIN = 1e-12                            # of d^2: no listed entry this near r^2, no tie this near at the K-th place
FLAT_OFFSET = (0.04, -0.03, 2.0)                   # the plane's initial error: x, y and degrees about z


def texture(x, y):
    """(n, 3) colours of the sheet at (x, y)."""
    w = 2.0 * np.pi
    return np.stack([0.5 + 0.3 * np.sin(w * x / 0.6 + 0.4) * np.cos(w * y / 0.7), 0.5 + 0.25 * np.cos(w * (x + y) / 0.8),
                     0.4 + 0.2 * np.sin(w * y / 0.6 + 1.0)], 1)


def flat_pair(seed, nref, nsrc):
    """ref, normals, src, gt, T0 of the exact plane z = 0: the source an independent sample of its interior, T0 = FLAT_OFFSET on gt."""
    rng = np.random.default_rng(seed)
    ref = np.concatenate([rng.random((nref, 2)), np.zeros((nref, 1))], 1)
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (nref, 1))
    on_ref = np.concatenate([0.1 + 0.8 * rng.random((nsrc, 2)), np.zeros((nsrc, 1))], 1)
    gt = F.rigid(rng, 25.0, 0.5)
    inv = np.linalg.inv(gt)
    src = on_ref @ inv[:3, :3].T + inv[:3, 3]
    a = np.deg2rad(FLAT_OFFSET[2])
    off = np.eye(4)
    off[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    off[:2, 3] = np.array(FLAT_OFFSET[:2]) + 0.5 - off[:2, :2] @ np.array([0.5, 0.5])          # (the turn is about the sheet's centre)
    return ref, nrm, src, gt, off @ gt


def in_plane_error(T, c):
    """The root mean square over the source rows of the in-plane (x, y) distance between T src and gt src."""
    src = np.asarray(c['src'], np.float64)
    d = (src @ T[:3, :3].T + T[:3, 3]) - (src @ c['gt'][:3, :3].T + c['gt'][:3, 3])
    return float(np.sqrt((d[:, :2] ** 2).sum(1).mean()))


@functools.lru_cache(maxsize=None)
def inputs(name, dtype):
    """-> dict(src, ref, normals, src_colors, ref_colors, T0, gt, r, gradient_radius) of `dtype` (T0 and gt stay float64), read-only."""
    seed, nref, nsrc, partial, r = FAMILIES[name]
    ref, nrm, src, gt, T0 = flat_pair(seed, nref, nsrc) if name == 'flat' else F._pair(seed, nref, nsrc, partial)
    on_sheet = src @ gt[:3, :3].T + gt[:3, 3]
    arrays = [np.ascontiguousarray(a.astype(dtype)) for a in (src, ref, nrm, texture(on_sheet[:, 0], on_sheet[:, 1]), texture(ref[:, 0], ref[:, 1]))]
    for a in arrays + [gt, T0]:
        a.setflags(write=False)
    return dict(zip(('src', 'ref', 'normals', 'src_colors', 'ref_colors'), arrays), T0=T0, gt=gt, r=r, gradient_radius=GRADIENT_RADIUS[name])


@functools.lru_cache(maxsize=None)
def gradient_case(name, dtype):
    """inputs(name, dtype) with the twin's reference gradients, `twin_gradients` and `members`, the search margins asserted."""
    c = dict(inputs(name, dtype))
    g, m, margins = C.gradients(c['ref'], c['normals'], c['ref_colors'], c['gradient_radius'])
    assert min(margins) >= GRADIENT_MARGIN, '%s %s: gradient search margins %.1e %.1e (another seed)' % ((name, dtype) + margins)
    g.setflags(write=False)
    c.update(twin_gradients=g, members=m)
    return c


@functools.lru_cache(maxsize=None)
def case(name, loss, dtype, lambda_geometric=0.968):
    """gradient_case(name, dtype) with `twin`: the twin's loop on the twin's gradients, its margins asserted."""
    c = dict(gradient_case(name, dtype))
    twin = C.icp(c['src'], c['ref'], c['T0'], c['r'], c['normals'], c['src_colors'], c['ref_colors'], c['twin_gradients'], lambda_geometric, loss,
                 1.0 if loss is None else LOSS_K[loss])
    for k, ev in enumerate(twin['evaluations']):
        assert ev['threshold_margin'] >= F.THRESHOLD_MARGIN, '%s %s %s: evaluation %d has a distance %.1e from r (another seed)' % (
            name, loss, dtype, k, ev['threshold_margin'])
        assert ev['gap_margin'] >= F.GAP_MARGIN, '%s %s %s: evaluation %d has a nearest / second-nearest gap of %.1e (another seed)' % (
            name, loss, dtype, k, ev['gap_margin'])
    c['twin'] = twin
    return c


CLOUD_SIZES = (3, 4, 29, 30, 31, 65)               # round K = 30: below 4 members, fewer rows than K, exactly K, more


def _textured(n, seed, dtype):
    pts, nrm = F.sheet(np.random.default_rng(seed), n)
    return [np.ascontiguousarray(a.astype(dtype)) for a in (pts, nrm, texture(pts[:, 0], pts[:, 1]))]


@functools.lru_cache(maxsize=None)
def small_cloud(kind, dtype):
    """-> (points, normals, colours, radius) of the gradient's edge clouds: kind an int of CLOUD_SIZES (a radius that holds every row),
    'duplicates' (25 rows, rows 5 .. 9 copies of rows 0 .. 4: each has a duplicate of a lower index) or 'sparse' (60 rows and a radius
    that leaves some rows fewer than 4 members)."""
    if kind == 'duplicates':
        p, nr, col = _textured(25, 200, dtype)
        for a in (p, nr, col):
            a[5:10] = a[0:5]
        return p, nr, col, 0.4
    if kind == 'sparse':
        return tuple(_textured(60, 201, dtype)) + (0.12,)
    return tuple(_textured(int(kind), 100 + int(kind), dtype)) + (2.0,)


def known_plane(seed=21, n=200, radius=0.2):
    """-> (points, normals, colours, radius, g): an exact plane through (0.3, -0.2, 0.5) with unit normal nrm, whose intensity is
    g . p + 0.7 with g orthogonal to nrm: every row with 4 members and neighbours that are not collinear has the gradient g."""
    rng = np.random.default_rng(seed)
    nrm = np.array([0.36, -0.48, 0.8])
    e1 = np.cross(nrm, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    uv = rng.random((n, 2))
    pts = np.array([0.3, -0.2, 0.5]) + uv[:, :1] * e1 + uv[:, 1:] * e2
    g = 0.8 * e1 - 0.5 * e2
    I = pts @ g + 0.7
    return pts, np.tile(nrm, (n, 1)), np.stack([I, I, I], 1), radius, g


def _rows(a):
    a = np.ascontiguousarray(a).reshape(-1, 3)
    assert a.dtype in (np.float32, np.float64)
    return a


_ptr = lambda a: None if a is None else a.ctypes.data if a.size else ctypes.addressof(F._dummy)
_elem = lambda a: int(a.dtype == np.float64)


def host_gradients(points, normals, colors, radius, max_nn=30):
    """se3_debug_color_gradient_host on numpy arrays -> (gradients (n, 3) float64, status)."""
    from se3et_amd._lib import check, lib
    p, nr, col = _rows(points), _rows(normals), _rows(colors)
    assert nr.shape == p.shape and col.shape == p.shape
    out, status = np.full((len(p), 3), -7.0), ctypes.c_int(-1)
    check(lib().se3_debug_color_gradient_host(_ptr(p), _ptr(nr), _ptr(col), len(p), _elem(p), _elem(nr), _elem(col), int(max_nn), float(radius),
                                              _ptr(out), ctypes.byref(status)), 'se3_debug_color_gradient_host')
    return out, status.value


def host_colored_icp(src, ref, T0, r, normals, src_colors, ref_colors, gradients, lambda_geometric=0.968, loss=None, loss_k=1.0,
                     relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, trace=False, loss_id=None):
    """se3_debug_icp_colored_host on numpy arrays, as icp_fixture.host_icp: -> dict(transform, fitness, rmse, iterations, converged, status,
    correspondences, and with trace the (max_iteration + 1, n) table).  loss_id: a raw id in place of the name."""
    from se3et_amd._lib import check, lib
    src, ref = _rows(src), _rows(ref)
    assert src.dtype == ref.dtype
    nrm = None if normals is None else _rows(normals)
    sc, rc = _rows(src_colors), _rows(ref_colors)
    g = None if gradients is None else np.ascontiguousarray(gradients, np.float64).reshape(-1, 3)
    assert (nrm is None or nrm.shape == ref.shape) and sc.shape == src.shape and rc.shape == ref.shape and (g is None or g.shape == ref.shape)
    T0 = np.ascontiguousarray(T0, np.float64).reshape(4, 4)
    T, fit, rmse = np.zeros((4, 4)), ctypes.c_double(), ctypes.c_double()
    it, conv, status = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    corr = np.full((len(src),), -2, np.int64)
    tr = np.full((max(max_iteration, 0) + 1, len(src)), -2, np.int64) if trace else None
    check(lib().se3_debug_icp_colored_host(_ptr(src), len(src), _ptr(ref), len(ref), _elem(src), _ptr(nrm), 0 if nrm is None else _elem(nrm),
                                           _ptr(sc), _elem(sc), _ptr(rc), _elem(rc), _ptr(g), _ptr(T0), float(r), float(lambda_geometric),
                                           LOSS_IDS[loss] if loss_id is None else loss_id, float(loss_k), relative_fitness, relative_rmse,
                                           max_iteration, _ptr(T), ctypes.byref(fit), ctypes.byref(rmse), ctypes.byref(it), ctypes.byref(conv),
                                           ctypes.byref(status), _ptr(corr), _ptr(tr)), 'se3_debug_icp_colored_host')
    out = {'transform': T, 'fitness': fit.value, 'rmse': rmse.value, 'iterations': it.value, 'converged': conv.value, 'status': status.value,
           'correspondences': corr}
    if trace:
        out['trace'] = tr
    return out


def host_case(c, loss, lambda_geometric=0.968, **kw):
    """The host entries end to end on a case: the host gradients of the reference, then the host loop on them."""
    g, status = host_gradients(c['ref'], c['normals'], c['ref_colors'], c['gradient_radius'])
    assert status == 0
    return host_colored_icp(c['src'], c['ref'], c['T0'], c['r'], c['normals'], c['src_colors'], c['ref_colors'], g, lambda_geometric, loss,
                            1.0 if loss is None else LOSS_K[loss], **kw), g
