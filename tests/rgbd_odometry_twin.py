"""The contract of se3et_amd/odometry.py (csrc/rgbd_odometry.hip) in numpy: float32 arrays for the preparation, every operation rounded on
its own; float64 for the correspondences, the rows and the information matrix, in the contract's operation order; exact sums (math.fsum).
The library's host entry is held to this file by tests/test_rgbd_odometry_cpu.py."""
import math

import numpy as np

F32 = np.float32
SUMS, CHUNK, IMAGES = 29, 2048, 6
FREE = np.uint64(0xFFFFFFFFFFFFFFFF)
W_DEPTH, W_COLOR = math.sqrt(0.95), math.sqrt(0.05)
STATUS = dict(nonfinite=1, too_few=2, singular=4, empty=8, step_refused=16)
PIVOT_TOL, MAX_ANGLE = 1e-13, 1.0


# ---- preparation: float32 ----------------------------------------------------------------------------------------------------------------------
def convert_depth(raw, depth_scale=1000.0, depth_trunc=3.0, min_depth=0.0, max_depth=4.0):
    with np.errstate(all='ignore'):
        d = raw.astype(F32) / F32(depth_scale)
        d = np.where(d > F32(depth_trunc), F32(0), d)
        bad = (d <= F32(min_depth)) | (d > F32(max_depth)) | ~np.isfinite(d)
    return np.where(bad, F32(np.nan), d).astype(F32)


def convert_color(c):
    if c.ndim == 3:
        r, g, b = (c[..., k].astype(F32) for k in range(3))
        s = (F32(0.2990) * r + F32(0.5870) * g) + F32(0.1140) * b
    else:
        s = c.astype(F32)
    return (s / F32(255) if c.dtype == np.uint8 else s).astype(F32)


def _shift(a, axis):
    """(the clamped neighbour before, the clamped neighbour after) along axis"""
    p = np.pad(a, [(1, 1) if k == axis else (0, 0) for k in range(a.ndim)], mode='edge')
    n = a.shape[axis]
    return np.take(p, range(0, n), axis), np.take(p, range(2, n + 2), axis)


def _blur_axis(a, axis):
    lo, hi = _shift(a, axis)
    return (F32(0.25) * lo + F32(0.5) * a) + F32(0.25) * hi


def gaussian3(a):
    with np.errstate(invalid='ignore'):
        return _blur_axis(_blur_axis(a, 1), 0)


def mean4(a):
    H, W = a.shape[0] // 2, a.shape[1] // 2
    a = a[:2 * H, :2 * W]
    with np.errstate(invalid='ignore'):
        return ((a[0::2, 0::2] + a[0::2, 1::2]) + (a[1::2, 0::2] + a[1::2, 1::2])) * F32(0.25)


def sobel(a):
    with np.errstate(invalid='ignore'):
        lo, hi = _shift(a, 1)
        e, s = hi - lo, (lo + F32(2) * a) + hi
        e_lo, e_hi = _shift(e, 0)
        s_lo, s_hi = _shift(s, 0)
        return (e_lo + F32(2) * e) + e_hi, s_hi - s_lo


def prepare_frame(depth, color, levels, target=True, **convert):
    """The pyramid of one frame: a list of levels, each a dict I, D and (for a target) Ix, Iy, Dx, Dy, float32 (H_l, W_l)."""
    out = [dict(I=gaussian3(convert_color(color)), D=gaussian3(convert_depth(depth, **convert)))]
    for _ in range(1, levels):
        out.append(dict(I=mean4(gaussian3(out[-1]['I'])), D=mean4(out[-1]['D'])))
    for lv in out:
        if target:
            lv['Ix'], lv['Iy'] = sobel(lv['I'])
            lv['Dx'], lv['Dy'] = sobel(lv['D'])
        assert all(v.dtype == F32 for v in lv.values())
    return out


def level_intrinsics(K, l):
    return [float(k) * (1.0 / (1 << l)) for k in K]


# ---- correspondences: float64 ---------------------------------------------------------------------------------------------------------------------
def camera(K, T):
    """M = K (R K^-1) by rows and K t, in the contract's operation order (rg_camera)"""
    fx, fy, cx, cy = K
    ifx, ify, kx, ky = 1.0 / fx, 1.0 / fy, -(cx / fx), -(cy / fy)
    A = [[T[a][0] * ifx, T[a][1] * ify, (T[a][0] * kx + T[a][1] * ky) + T[a][2]] for a in range(3)]
    M = [[fx * A[0][b] + cx * A[2][b] for b in range(3)], [fy * A[1][b] + cy * A[2][b] for b in range(3)], [A[2][b] for b in range(3)]]
    return M, [fx * T[0][3] + cx * T[2][3], fy * T[1][3] + cy * T[2][3], T[2][3]]


def claim_map(src, tgt, K, T, max_depth_diff=0.03):
    """(H W,) uint64: FREE, or hi32(q_z) << 32 | source index of the winning source pixel of every target pixel"""
    T = np.asarray(T, np.float64).tolist()
    D, Dt = src['D'], tgt['D']
    H, W = D.shape
    M, Kt = camera(K, T)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    d = D.astype(np.float64)
    with np.errstate(all='ignore'):
        q = [d * ((M[a][0] * u + M[a][1] * v) + M[a][2]) + Kt[a] for a in range(3)]
        ut, vt = np.floor(q[0] / q[2] + 0.5), np.floor(q[1] / q[2] + 0.5)
        ok = ~np.isnan(D) & (q[2] > 0) & (ut >= 0) & (ut < W) & (vt >= 0) & (vt < H)
    s = np.flatnonzero(ok.reshape(-1))
    j = (vt.reshape(-1)[s].astype(np.int64) * W + ut.reshape(-1)[s].astype(np.int64))
    qz = q[2].reshape(-1)[s]
    dt = Dt.reshape(-1)[j].astype(np.float64)
    with np.errstate(invalid='ignore'):
        keep = ~np.isnan(dt) & ~(np.abs(qz - dt) > max_depth_diff)
    s, j, qz = s[keep], j[keep], qz[keep]
    key = (qz.view(np.uint64) & np.uint64(0xFFFFFFFF00000000)) | s.astype(np.uint64)
    out = np.full(H * W, FREE, np.uint64)
    np.minimum.at(out, j, key)
    return out


def correspondences(cmap):
    """(source indices, target indices) of a map, ascending target index"""
    j = np.flatnonzero(cmap != FREE)
    return (cmap[j] & np.uint64(0xFFFFFFFF)).astype(np.int64), j


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------------
def row(gx, gy, fx, fy, x, y, z):
    c0, c1 = (gx * fx) / z, (gy * fy) / z
    c2 = -((c0 * x + c1 * y) / z)
    return [y * c2 - z * c1, z * c0 - x * c2, x * c1 - y * c0, c0, c1, c2]


def pixel_rows(method, K, T, d, u, v, I_s, I_t, D_t, gI, gD, scale):
    """The rows of correspondences given by value (arrays of one length): the source depth d at pixel (u, v), the intensities, the target depth,
    the gradients (0.125 Sobel, unscaled) gI = (gx, gy), gD likewise.  Returns [(J (6 arrays), r)] : the colour row, then (hybrid) the depth row."""
    fx, fy, cx, cy = K
    T = np.asarray(T, np.float64).tolist()
    xr, yr = (u - cx) / fx, (v - cy) / fy
    p = [d * xr, d * yr, d]
    x, y, z = [((T[a][0] * p[0] + T[a][1] * p[1]) + T[a][2] * p[2]) + T[a][3] for a in range(3)]
    wi = 1.0 if method == 'color' else W_COLOR
    J = row(scale[1] * gI[0], scale[1] * gI[1], fx, fy, x, y, z)
    out = [([wi * c for c in J], wi * (scale[1] * I_t - scale[0] * I_s))]
    if method == 'hybrid':
        J = row(gD[0], gD[1], fx, fy, x, y, z)
        J[0], J[1], J[5] = J[0] - y, J[1] + x, J[5] - 1.0
        out.append(([W_DEPTH * c for c in J], W_DEPTH * (D_t - z)))
    return out


def _f64(a, idx):
    return a.reshape(-1)[idx].astype(np.float64)


def step_terms(src, tgt, K, T, cmap, scale, method):
    """(n, 29) float64: what every correspondence adds to the 29 sums, and the same with every product's absolute value (the bound's scale)"""
    s, j = correspondences(cmap)
    W = src['D'].shape[1]
    gI = [0.125 * _f64(tgt['Ix'], j), 0.125 * _f64(tgt['Iy'], j)]
    gD = [np.nan_to_num(0.125 * _f64(tgt['Dx'], j), nan=0.0), np.nan_to_num(0.125 * _f64(tgt['Dy'], j), nan=0.0)]
    rows = pixel_rows(method, K, T, _f64(src['D'], s), (s % W).astype(np.float64), (s // W).astype(np.float64), _f64(src['I'], s), _f64(tgt['I'], j),
                      _f64(tgt['D'], j), gI, gD, scale)
    terms, mags = np.zeros((len(s), SUMS)), np.zeros((len(s), SUMS))
    for J, r in rows:
        e = 0
        for a in range(6):
            for b in range(a, 6):
                terms[:, e] += J[a] * J[b]
                mags[:, e] += np.abs(J[a] * J[b])
                e += 1
        for a in range(6):
            terms[:, 21 + a] += J[a] * r
            mags[:, 21 + a] += np.abs(J[a] * r)
        terms[:, 27] += r * r
        mags[:, 27] += r * r
    terms[:, 28] = mags[:, 28] = 1.0
    return terms, mags, rows


def exact_step_sums(src, tgt, K, T, cmap, scale, method):
    """The 29 sums, exactly summed: every row's products are terms of their own (a pixel's two rows are two terms)."""
    s, _j = correspondences(cmap)
    _t, _m, rows = step_terms(src, tgt, K, T, cmap, scale, method)
    cols = [[] for _ in range(SUMS)]
    for J, r in rows:
        e = 0
        for a in range(6):
            for b in range(a, 6):
                cols[e].append(J[a] * J[b])
                e += 1
        for a in range(6):
            cols[21 + a].append(J[a] * r)
        cols[27].append(r * r)
    out = [math.fsum(np.concatenate(c).tolist()) if c else 0.0 for c in cols]
    out[28] = float(len(s))
    return np.array(out)


def normalisation(src, tgt, cmap):
    s, j = correspondences(cmap)
    if len(s) == 0:
        return None
    n = float(len(s))
    return [0.5 / (math.fsum(_f64(src['I'], s).tolist()) / n), 0.5 / (math.fsum(_f64(tgt['I'], j).tolist()) / n)]


def information(tgt, K, cmap):
    _s, j = correspondences(cmap)
    fx, fy, cx, cy = K
    W = tgt['D'].shape[1]
    d = _f64(tgt['D'], j)
    px, py, pz = d * (((j % W).astype(np.float64) - cx) / fx), d * (((j // W).astype(np.float64) - cy) / fy), d
    o, z = np.ones_like(d), np.zeros_like(d)
    G = [[z, pz, -py, o, z, z], [-pz, z, px, z, o, z], [py, -px, z, z, z, o]]
    out = np.zeros((6, 6))
    for a in range(6):
        for b in range(a, 6):
            out[a, b] = out[b, a] = math.fsum(((G[0][a] * G[0][b] + G[1][a] * G[1][b]) + G[2][a] * G[2][b]).tolist())
    return out, len(j)


# ---- the solve and the whole schedule ------------------------------------------------------------------------------------------------------------
def matrix_of(sums):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums[:21]
    return A + np.triu(A, 1).T, np.asarray(sums[21:27], np.float64)


def vector6_to_matrix(x):
    sx, cx, sy, cy, sz, cz = math.sin(x[0]), math.cos(x[0]), math.sin(x[1]), math.cos(x[1]), math.sin(x[2]), math.cos(x[2])
    return np.array([[cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz, x[3]],
                     [cy * sz, sx * sy * sz + cx * cz, cx * sy * sz - sx * cz, x[4]],
                     [-sy, sx * cy, cx * cy, x[5]], [0.0, 0.0, 0.0, 1.0]])


def update(sums, T):
    """(status, the new transform or None): the tests of the contract on exact sums, numpy's solve"""
    if not np.isfinite(sums).all():
        return STATUS['nonfinite'], None
    if sums[28] < 6:
        return STATUS['too_few'], None
    A, b = matrix_of(sums)
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return STATUS['singular'], None
    if not (np.diag(L) ** 2 > PIVOT_TOL * np.diag(A)).all():
        return STATUS['singular'], None
    x = np.linalg.solve(A, -b)
    if not (np.abs(x[:3]) < MAX_ANGLE).all():
        return STATUS['step_refused'], None
    return 0, vector6_to_matrix(x) @ np.asarray(T, np.float64)


def odometry(src, tgt, K, T0=None, method='hybrid', iterations=(20, 10, 5), max_depth_diff=0.03):
    """One pair from its two pyramids: dict(transform, success, status, information, correspondences), the contract's schedule on exact sums."""
    failed = dict(transform=np.eye(4), success=False, information=np.zeros((6, 6)), correspondences=0)
    T = np.eye(4) if T0 is None else np.asarray(T0, np.float64).copy()
    T[3] = [0.0, 0.0, 0.0, 1.0]
    if not np.isfinite(T).all():
        return dict(failed, status=STATUS['nonfinite'])
    scale = normalisation(src[0], tgt[0], claim_map(src[0], tgt[0], level_intrinsics(K, 0), T, max_depth_diff))
    if scale is None:
        return dict(failed, status=STATUS['empty'])
    levels = len(iterations)
    for l in range(levels - 1, -1, -1):
        Kl = level_intrinsics(K, l)
        for _ in range(iterations[levels - 1 - l]):
            cmap = claim_map(src[l], tgt[l], Kl, T, max_depth_diff)
            status, Tn = update(exact_step_sums(src[l], tgt[l], Kl, T, cmap, scale, method), T)
            if status:
                return dict(failed, status=status)
            T = Tn
    info, n = information(tgt[0], level_intrinsics(K, 0), claim_map(src[0], tgt[0], level_intrinsics(K, 0), T, max_depth_diff))
    return dict(transform=T, success=True, status=0, information=info, correspondences=n)
