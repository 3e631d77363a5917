"""Host twin of se3et_amd.ransac: the RANSAC contract (semantics 1-7 of the module docstring) restated in float64 numpy, for explicit
hypothesis indices.  Fits use np.linalg.svd; a hypothesis whose second singular value is below 1e-9 times the first is flagged
degenerate (its rotation is not determined by the sample, so device and twin may legitimately differ there).

Borderline allowance: device and twin may disagree on correspondence i of a hypothesis only where |d_f64 - thr| <= 1e-5 (1 + |s| + |r|).
Error sums: the device's float32 d of an inlier carries rounding of order delta_i = 1e-6 (1 + |s_i| + |r_i|) (the transform rounded to
float32, then sums of terms of the coordinates' size), so its d^2 may differ by (2 d_i + delta_i) delta_i; err_floor sums that over the
inliers of each hypothesis."""
import numpy as np

DEGENERATE = 1e-9


def fit(src, ref):
    """Unweighted Kabsch, src -> ref, of (H, k, 3) samples: (R (H, 3, 3), t (H, 3), degenerate (H,) bool)."""
    sc, rc = src.mean(1), ref.mean(1)
    Hm = np.einsum('hki,hkj->hij', src - sc[:, None], ref - rc[:, None])
    U, S, Vt = np.linalg.svd(Hm)
    V = np.transpose(Vt, (0, 2, 1))
    d = np.sign(np.linalg.det(V @ np.transpose(U, (0, 2, 1))))
    d[d == 0] = 1.0
    D = np.zeros((len(d), 3, 3))
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = d
    R = V @ D @ np.transpose(U, (0, 2, 1))
    t = rc - np.einsum('hij,hj->hi', R, sc)
    return R, t, ~(S[:, 1] > DEGENERATE * S[:, 0])      # (all-zero H included)


def distances(R, t, src, ref):
    """(H, n) float64 |R s + t - r|; NaN where a correspondence is not finite."""
    d = np.linalg.norm(np.einsum('hij,nj->hni', R, src) + t[:, None, :] - ref[None], axis=2)
    bad = ~(np.isfinite(src).all(1) & np.isfinite(ref).all(1))
    d[:, bad] = np.nan
    return d


def borderline(d, thr, src, ref):
    """(H, n) bool: correspondences within the allowance of the threshold."""
    tol = 1e-5 * (1.0 + np.linalg.norm(src, axis=1) + np.linalg.norm(ref, axis=1))
    return np.abs(d - thr) <= tol[None, :]


def run(src, ref, thr, ransac_n, hyp_idx, chunk=256):
    """RANSAC of one pair with explicit (H, ransac_n) indices.  Returns dict(transform (4, 4), fitness, rmse, best (-1: identity),
    counts (H,), err_sums (H,), degenerate (H,), R, t, n_border (H,) borderline correspondences and err_floor (H,) per hypothesis)."""
    src, ref = np.asarray(src, np.float64), np.asarray(ref, np.float64)
    n, H = src.shape[0], len(hyp_idx)
    ident = dict(transform=np.eye(4), fitness=0.0, rmse=0.0, best=-1, counts=np.zeros(H, np.int64), err_sums=np.zeros(H),
                 degenerate=np.zeros(H, bool), n_border=np.zeros(H, np.int64), err_floor=np.zeros(H))
    if ransac_n < 3 or n < ransac_n or not thr > 0 or H == 0:
        return ident
    hyp_idx = np.asarray(hyp_idx, np.int64)
    S, Rf = src[hyp_idx], ref[hyp_idx]
    finite = np.isfinite(S).all((1, 2)) & np.isfinite(Rf).all((1, 2))
    S, Rf = np.where(np.isfinite(S), S, 0.0), np.where(np.isfinite(Rf), Rf, 0.0)
    R, t, degenerate = fit(S, Rf)
    counts, errs, nb, floor = np.zeros(H, np.int64), np.zeros(H), np.zeros(H, np.int64), np.zeros(H)
    delta = 1e-6 * (1.0 + np.linalg.norm(src, axis=1) + np.linalg.norm(ref, axis=1))
    for a in range(0, H, chunk):
        d = distances(R[a:a + chunk], t[a:a + chunk], src, ref)
        inl = d < thr
        counts[a:a + chunk] = inl.sum(1)
        errs[a:a + chunk] = np.where(inl, d * d, 0.0).sum(1)
        nb[a:a + chunk] = borderline(d, thr, src, ref).sum(1)
        floor[a:a + chunk] = np.where(inl, (2 * d + delta[None]) * delta[None], 0.0).sum(1)
    counts[~finite], errs[~finite], nb[~finite], floor[~finite] = 0, 0.0, 0, 0.0
    best, bc, be = -1, 0, 0.0
    for h in range(H):               # rule 5, lowest h among equals; identity (0 inliers) first
        if counts[h] > bc or (counts[h] == bc and bc > 0 and errs[h] < be):
            best, bc, be = h, counts[h], errs[h]
    out = dict(ident, counts=counts, err_sums=errs, degenerate=degenerate, R=R, t=t, n_border=nb, err_floor=floor)
    if best >= 0:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R[best], t[best]
        out.update(transform=T, fitness=bc / n, rmse=float(np.sqrt(be / bc)), best=best)
    return out


def synthetic_pair(rng, n, inlier_ratio, sigma=0.01, extent=3.0):
    """n correspondences on a cloud `extent` metres across: a random rigid T (src -> ref), the first round(n * ratio) rows are inliers
    (ref = T src + N(0, sigma^2) per axis), the rest pair src with unrelated ref points.  Returns src, ref (float32), T (float64),
    a random permutation already applied."""
    src = rng.uniform(-extent / 2, extent / 2, (n, 3))
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    t = rng.uniform(-1, 1, 3)
    ref = src @ R.T + t
    k = int(round(n * inlier_ratio))
    ref[:k] += rng.normal(scale=sigma, size=(k, 3))
    ref[k:] = rng.uniform(-extent / 2, extent / 2, (n - k, 3)) + t
    perm = rng.permutation(n)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return src[perm].astype(np.float32), ref[perm].astype(np.float32), T
