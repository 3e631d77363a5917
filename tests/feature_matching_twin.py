"""Host twin of se3et_amd.feature_matching and of the RANSAC checkers: the contract restated in float64 numpy.

  sq_distances(x, y)            (N, M) float64 direct-difference squared distances, in row chunks
  nearest(x, y)                 per row of x: the index of the nearest row of y (lowest index among equals; -1 without a finite candidate)
                                and the squared distance (+inf for -1)
  tolerance / near_ties(x, y)   the allowance of the float32 ranking value and the rows on which it leaves the winner open
  extract(nn_src, nn_ref, mode) the four extraction modes from the two index arrays
  edge_length_ok / distance_ok / checked_run   the checkers on explicit hypothesis indices (the fit is ransac_twin's)

Allowance of the ranking value: the device ranks by v = (|x|^2 - 2 x.y) + |y|^2 in float32.  A length-C float32 dot product carries a
relative error of at most gamma_C ~ C 2^-24 of sum |x_k y_k| <= (|x|^2 + |y|^2) / 2, doubled by the factor 2, plus the two norms (each
gamma_C of itself) and the two additions: tol(i, j) = (C + 8) 2^-22 (|x_i|^2 + |y_j|^2) covers it with room for a dropped low-order
product term.  Row i with float64 winner j0 is a NEAR-TIE row if some j != j0 has d2(i, j) - d2(i, j0) < tol(i, j) + tol(i, j0); on such
a row the device may return any candidate inside that bound, on every other row it must return j0."""
import numpy as np

import ransac_twin

MODES = ('one_way', 'mutual', 'bilateral_mask', 'bilateral_concat')


def sq_distances(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = np.empty((len(x), len(y)))
    step = max(1, int(4e6 // max(1, y.size)))
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(0, len(x), step):
            diff = x[a:a + step, None, :] - y[None, :, :]
            out[a:a + step] = np.einsum('nmc,nmc->nm', diff, diff)
    return out


def _sq_distances_fast(x, y):
    """The same within float64 rounding, through one matrix product (for the 5000-row inputs): |x|^2 - 2 x.y + |y|^2."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return (x * x).sum(1)[:, None] - 2.0 * (x @ y.T) + (y * y).sum(1)[None, :]


def nearest_from_matrix(d2):
    """Argmin per row with lowest-index ties; candidates that are not finite are never chosen."""
    n, m = d2.shape
    if m == 0:
        return np.full(n, -1, np.int64), np.full(n, np.inf)
    masked = np.where(np.isfinite(d2), d2, np.inf)
    idx = masked.argmin(1).astype(np.int64)                 # numpy's argmin returns the first of equal minima
    best = masked[np.arange(n), idx]
    idx[~np.isfinite(best)] = -1
    return idx, np.where(idx >= 0, best, np.inf)


def nearest(x, y):
    return nearest_from_matrix(sq_distances(x, y))


def direct_sq_distance(x, y, idx):
    """sum (x_i - y_idx[i])^2 in float64, +inf where idx is -1."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = np.full(len(x), np.inf)
    ok = idx >= 0
    diff = x[ok] - y[idx[ok]]
    out[ok] = (diff * diff).sum(1)
    return out


def tolerance(x, y):
    """tol(i, j) as an outer sum: returns (row part (N,), column part (M,)) with tol(i, j) = row[i] + col[j]."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    k = (x.shape[1] + 8) * 2.0 ** -22
    return k * (x * x).sum(1), k * (y * y).sum(1)


def near_ties(x, y, fast=False):
    """(idx (N,), d2 of the winner (N,), near (N,) bool, allowed (N, M) bool: the candidates the device may return on each row)."""
    d2 = _sq_distances_fast(x, y) if fast else sq_distances(x, y)
    idx, best = nearest_from_matrix(d2)
    tr, tc = tolerance(x, y)
    n, m = d2.shape
    if m == 0:
        return idx, best, np.zeros(n, bool), np.zeros((n, 0), bool)
    j0 = np.maximum(idx, 0)
    bound = (tr[:, None] + tc[None, :]) + (tr + tc[j0])[:, None]
    with np.errstate(invalid='ignore'):
        allowed = (d2 - best[:, None]) < bound
    allowed[idx < 0] = False
    allowed[np.arange(n), j0] = idx >= 0
    return idx, best, allowed.sum(1) > 1, allowed


def extract(nn_src, nn_ref, mode):
    """(ref_corr_indices, src_corr_indices) int64 of one pair.  nn_src: (N,) the src index of every ref row; nn_ref: (M,)."""
    nn_src, nn_ref = np.asarray(nn_src, np.int64), np.asarray(nn_ref, np.int64)
    n, m = len(nn_src), len(nn_ref)
    i = np.arange(n)[nn_src >= 0]
    fwd = np.stack([i, nn_src[i]], 1).reshape(-1, 2)
    j = np.arange(m)[nn_ref >= 0]
    bwd = np.stack([nn_ref[j], j], 1).reshape(-1, 2)
    if mode == 'one_way':
        out = fwd
    elif mode == 'mutual':
        out = fwd[nn_ref[fwd[:, 1]] == fwd[:, 0]]
    elif mode == 'bilateral_concat':
        out = np.concatenate([fwd, bwd], 0)
    elif mode == 'bilateral_mask':
        mask = np.zeros((n, m), bool)                       # the OR of the two masks, then nonzero: row-major, duplicates once
        mask[fwd[:, 0], fwd[:, 1]] = True
        mask[bwd[:, 0], bwd[:, 1]] = True
        out = np.stack(np.nonzero(mask), 1)
    else:
        raise ValueError(mode)
    return out[:, 0].astype(np.int64), out[:, 1].astype(np.int64)


def extract_torch_form(d2, mutual=False, bilateral=False):
    """The reference's torch function on a float64 distance matrix (matching.py:135-170 through extract_correspondences_from_scores with
    exp(-d2) > 0), as masks."""
    n, m = d2.shape
    with np.errstate(under='ignore'):
        s = np.exp(-d2)
    ref_mask = np.zeros((n, m), bool)
    jm = s.argmax(1)
    ref_mask[np.arange(n), jm] = s[np.arange(n), jm] > 0
    if mutual or bilateral:
        src_mask = np.zeros((n, m), bool)
        im = s.argmax(0)
        src_mask[im, np.arange(m)] = s[im, np.arange(m)] > 0
        ref_mask = (ref_mask & src_mask) if mutual else (ref_mask | src_mask)
    return np.nonzero(ref_mask)


# ---- RANSAC checkers ---------------------------------------------------------------------------------------------------------------------
EDGE_MARGIN = 1e-12


def edge_length_ok(S, R, t):
    """S, R: (H, k, 3) sampled src / ref points.  (ok (H,), borderline (H,)): Open3D's edge-length checker over all pairs of the sample;
    borderline where a compared quantity lies within 1e-12 (|ds| + |dr|) of its limit."""
    S, R = np.asarray(S, np.float64), np.asarray(R, np.float64)
    H, k = S.shape[:2]
    ok, border = np.ones(H, bool), np.zeros(H, bool)
    for a in range(k):
        for b in range(a + 1, k):
            ds, dr = np.linalg.norm(S[:, a] - S[:, b], axis=1), np.linalg.norm(R[:, a] - R[:, b], axis=1)
            ok &= ~((ds < t * dr) | (dr < t * ds))
            margin = EDGE_MARGIN * (ds + dr)               # (a correspondence drawn twice has ds = dr = 0 exactly: decided, not borderline)
            border |= ((np.abs(ds - t * dr) <= margin) | (np.abs(dr - t * ds) <= margin)) & (ds + dr > 0)
    return ok, border


def distance_ok(Rm, tv, S, R, thr):
    """(ok (H,), borderline (H,)): no sampled correspondence farther than thr after the fit; borderline with ransac_twin's allowance."""
    d = np.linalg.norm(np.einsum('hij,hkj->hki', Rm, S) + tv[:, None, :] - R, axis=2)
    tol = 1e-5 * (1.0 + np.linalg.norm(S, axis=2) + np.linalg.norm(R, axis=2))
    return ~(d > thr).any(1), (np.abs(d - thr) <= tol).any(1)


def checked_run(src, ref, thr, ransac_n, hyp_idx, edge_t=None, check_distance=False):
    """ransac_twin.run with the checkers: adds passed (H,), open (H,) (a checker decision inside its allowance, or a degenerate fit under
    the distance checker) and zeroes the counts / error sums of rejected hypotheses; best / transform / fitness / rmse follow the total
    order among the passed hypotheses."""
    src, ref = np.asarray(src, np.float64), np.asarray(ref, np.float64)
    base = ransac_twin.run(src, ref, thr, ransac_n, hyp_idx)
    H, n = len(hyp_idx), len(src)
    idx = np.asarray(hyp_idx, np.int64).reshape(H, -1)
    if 'R' not in base:
        return dict(base, passed=np.zeros(H, bool), open=np.zeros(H, bool))
    S, R = src[idx], ref[idx]
    passed = np.isfinite(S).all((1, 2)) & np.isfinite(R).all((1, 2))
    S, R = np.where(np.isfinite(S), S, 0.0), np.where(np.isfinite(R), R, 0.0)
    open_ = np.zeros(H, bool)
    if edge_t is not None:
        ok, border = edge_length_ok(S, R, edge_t)
        passed &= ok
        open_ |= border
    if check_distance:
        ok, border = distance_ok(base['R'], base['t'], S, R, thr)
        passed &= ok
        open_ |= border | base['degenerate']
    counts, errs = np.where(passed, base['counts'], 0), np.where(passed, base['err_sums'], 0.0)
    best, bc, be = -1, 0, 0.0
    for h in range(H):
        if counts[h] > bc or (counts[h] == bc and bc > 0 and errs[h] < be):
            best, bc, be = h, counts[h], errs[h]
    out = dict(base, counts=counts, err_sums=errs, passed=passed, open=open_, best=best, transform=np.eye(4), fitness=0.0, rmse=0.0)
    if best >= 0:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = base['R'][best], base['t'][best]
        out.update(transform=T, fitness=bc / n, rmse=float(np.sqrt(be / bc)))
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def planted_features(rng, n, m, C, matches, noise=0.05, unit=True, scale=None):
    """n ref and m src descriptors: the first `matches` src rows are noisy copies of distinct ref rows, the rest are distractors; rows are
    shuffled.  unit: rows normalised to length 1; scale: per-row factors exp(U(-1, 1)) applied afterwards.  float32."""
    ref = rng.normal(size=(n, C))
    src = rng.normal(size=(m, C))
    k = min(matches, n, m)
    pick = rng.permutation(n)[:k]
    src[:k] = ref[pick] + noise * rng.normal(size=(k, C))
    src = src[rng.permutation(m)]
    if unit:
        ref /= np.linalg.norm(ref, axis=1, keepdims=True)
        src /= np.linalg.norm(src, axis=1, keepdims=True)
    if scale:
        ref *= np.exp(rng.uniform(-1, 1, (n, 1)))
        src *= np.exp(rng.uniform(-1, 1, (m, 1)))
    return ref.astype(np.float32), src.astype(np.float32)
