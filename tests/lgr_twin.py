"""Host twin of the local-to-global registration (LGR) kernels: csrc/registration.hip (weighted Procrustes, inlier votes, mutual top-k)
and csrc/kabsch.h, driven as modules/geotransformer/local_global_registration.py and batched.registration_pairs drive them.  The
contract is restated in float64 numpy from the semantics of the reference's procrustes.py and local_global_registration.py:

  Procrustes   w < 0 -> 0; w' = w / (sum w + eps); sc = sum w' s, rc = sum w' r; H = sum w' (s - sc)(r - rc)^T = U S V^T;
               R = V diag(1, 1, d = sign det(V U^T)) U^T, t = rc - R sc.  R is unique only where sigma2 + d sigma3 > 0 (rank >= 2,
               and sigma2 > sigma3 when the reflection fix applies); elsewhere any maximiser of trace(R H) over rotations is correct.  H = 0 (no
               weight, or every point the same) gives the identity.
  Gate         w_i = score_i * [ |r_i - (R s_i + t)| < radius ]  (a NaN score stays NaN: NaN * 0).
  Mutual top-k entry (i, j) is kept when it ranks below k in its row AND in its column (rank = entries strictly greater, plus equal
               entries at a lower index; masked entries take part in the ranking), its score is strictly greater than the
               threshold, and row i and column j are valid (the masks are applied last).  A NaN entry is never kept and never ranks
               ahead of another entry (no comparison with it holds).
  LGR          row-major nonzero of the mask; one hypothesis per patch with at least `correspondence_threshold` correspondences,
               voted on by all correspondences of the pair, the first maximum wins; without one, a solve on all correspondences;
               then `num_refinement_steps` gated solves on all correspondences.

Band: the device gates and votes in float32.  A residual within 1e-5 (1 + |s| + |r|) of the radius may fall either way there, so every
helper that thresholds a residual also reports those rows (the convention of tests/ransac_twin.py)."""
import numpy as np

BAND = 1e-5


def _rows(x):
    return np.asarray(x, np.float64).reshape(-1, 3)


def procrustes(src, ref, w, eps=1e-5):
    """Weighted Kabsch src -> ref of one problem.  Returns dict(T (4, 4), R, t, H, sv (3,) singular values of H, d = sign det(V U^T),
    sc, rc).  All-NaN transform where H is not finite."""
    src, ref = _rows(src), _rows(ref)
    w = np.asarray(w, np.float64).reshape(-1)
    w = np.where(w < 0, 0.0, w)
    w = w / (w.sum() + eps)
    sc, rc = w @ src, w @ ref
    H = (src - sc).T @ (w[:, None] * (ref - rc))
    out = dict(H=H, sc=sc, rc=rc)
    if not np.isfinite(H).all():
        nan = np.full((4, 4), np.nan)
        return dict(out, T=nan, R=nan[:3, :3], t=nan[:3, 3], sv=np.full(3, np.nan), d=np.nan)
    if not H.any():
        U, S, Vt = np.eye(3), np.zeros(3), np.eye(3)
    else:
        U, S, Vt = np.linalg.svd(H)
    V = Vt.T
    d = 1.0 if np.linalg.det(V @ U.T) >= 0 else -1.0
    R = V @ np.diag([1.0, 1.0, d]) @ U.T
    t = rc - R @ sc
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return dict(out, T=T, R=R, t=t, sv=S, d=d)


def optimum(sol):
    """max over rotations of trace(R H): sigma1 + sigma2 + d sigma3."""
    S = sol['sv']
    return S[0] + S[1] + sol['d'] * S[2]


def unique(sol, rel=1e-3):
    """R is well determined by H: sigma2 + d sigma3 >= rel sigma1.  (Of the signed singular values sigma1, sigma2, d sigma3 that the
    optimal R matches, the smallest pairwise sum bounds how far R moves with H; repeated singular values alone do not make R ambiguous.)"""
    S = sol['sv']
    return bool(S[0] > 0 and S[1] + sol['d'] * S[2] >= rel * S[0])


def residuals(src, ref, T):
    """float64 |r - (R s + t)| of every correspondence."""
    src, ref, T = _rows(src), _rows(ref), np.asarray(T, np.float64)
    return np.linalg.norm(ref - (src @ T[:3, :3].T + T[:3, 3]), axis=1)


def in_band(d, radius, src, ref):
    """Rows whose residual d lies within BAND (1 + |s| + |r|) of the radius."""
    tol = BAND * (1.0 + np.linalg.norm(_rows(src), axis=1) + np.linalg.norm(_rows(ref), axis=1))
    return np.abs(d - radius) <= tol


def gated_weights(src, ref, score, T, radius):
    """score * [residual under T < radius] and the band flags of the rows."""
    d = residuals(src, ref, T)
    score = np.asarray(score, np.float64)
    return score * (d < radius), in_band(d, radius, src, ref)


def count_inliers(src, ref, T, radius, lo=0, hi=None):
    """(inliers, rows in the band) of correspondences [lo, hi) under T."""
    hi = len(_rows(src)) if hi is None else hi
    s, r = _rows(src)[lo:hi], _rows(ref)[lo:hi]
    d = residuals(s, r, T)
    return int((d < radius).sum()), int(in_band(d, radius, s, r).sum())


def _rank(S, axis):
    """Number of entries of the same row (axis 2) or column (axis 1) ahead of each entry of S (B, R, C): strictly greater, or equal at
    a lower index."""
    n = S.shape[axis]
    lower = np.arange(n)[None, :] < np.arange(n)[:, None]             # [entry index, other index]: other < entry
    if axis == 2:
        a, o = S[:, :, :, None], S[:, :, None, :]                       # [b, i, j, jj]
        return ((o > a) | ((o == a) & lower[None, None])).sum(3)
    a, o = S[:, :, None, :], S[:, None, :, :]                           # [b, i, ii, j]
    return ((o > a) | ((o == a) & lower[None, :, :, None])).sum(2)


def mutual_topk(scores, row_masks, col_masks, k, threshold):
    """bool (B, R, C) mask of the mutual top-k correspondences of float32 scores (B, R, C)."""
    S = np.asarray(scores, np.float32)
    B, R, C = S.shape
    out = np.zeros((B, R, C), bool)
    chunk = max(1, (1 << 23) // (R * C * max(R, C)))
    for a in range(0, B, chunk):
        s = S[a:a + chunk]
        keep = (s > np.float32(threshold)) & (_rank(s, 2) < k) & (_rank(s, 1) < k)
        out[a:a + chunk] = keep & np.asarray(row_masks, bool)[a:a + chunk, :, None] & np.asarray(col_masks, bool)[a:a + chunk, None, :]
    return out


def lgr_pair(ref_knn, src_knn, ref_masks, src_masks, scores, k, confidence_threshold, acceptance_radius, correspondence_threshold=3,
             num_refinement_steps=5, eps=1e-5):
    """LGR of one pair from its exponentiated float32 scores (B, K, K).  Returns dict(ref_corr, src_corr, corr_scores (float32, in
    row-major order), T (4, 4), offsets (B + 1,), votes (B,) (-1 below the threshold), vote_band (B,), best (-1: degenerate branch),
    step_band: rows in the band at each refinement step)."""
    ref_knn, src_knn = np.asarray(ref_knn, np.float32), np.asarray(src_knn, np.float32)
    scores = np.asarray(scores, np.float32)
    mask = mutual_topk(scores, ref_masks, src_masks, k, confidence_threshold)
    b, r, c = np.nonzero(mask)
    ref_c, src_c, sc = ref_knn[b, r], src_knn[b, c], scores[b, r, c]
    B = scores.shape[0]
    offsets = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=B))])
    votes, vote_band = np.full(B, -1, np.int64), np.zeros(B, np.int64)
    hyps = [None] * B
    for p in range(B):
        lo, hi = offsets[p], offsets[p + 1]
        if hi - lo >= correspondence_threshold:
            hyps[p] = procrustes(src_c[lo:hi], ref_c[lo:hi], sc[lo:hi], eps)['T']
            votes[p], vote_band[p] = count_inliers(src_c, ref_c, hyps[p], acceptance_radius)
    best = int(np.argmax(votes)) if B and votes.max() >= 0 else -1
    T = hyps[best] if best >= 0 else procrustes(src_c, ref_c, sc, eps)['T']
    step_band = []
    for _ in range(num_refinement_steps):
        w, band = gated_weights(src_c, ref_c, sc, T, acceptance_radius)
        step_band.append(int(band.sum()))
        T = procrustes(src_c, ref_c, w, eps)['T']
    return dict(ref_corr=ref_c, src_corr=src_c, corr_scores=sc, T=T, offsets=offsets, votes=votes, vote_band=vote_band, best=best,
                step_band=step_band)


def decisive(res):
    """The vote cannot change with the band rows: every other hypothesis differs from the winner by more than their band rows, or
    neither has any."""
    v, bnd, w = res['votes'], res['vote_band'], res['best']
    if w < 0:
        return True
    for p in range(len(v)):
        if p == w or v[p] < 0:
            continue
        slack = bnd[p] + bnd[w]
        if slack and abs(v[p] - v[w]) <= slack:
            return False
    return True


def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


SHIFT = np.array([1.0, -0.6, 0.4])          # T2 = T1 moved by SHIFT: |T1 s - T2 s| = 1.25 for every s


def synthetic_lgr_pair(rng, kinds, K=32, noise=0.002, outlier=0.8, counts=None):
    """Patches of one pair with planted correspondences, for acceptance radius 0.1, k >= 1 and confidence threshold 0.05.  kinds[b]:
    'T1' / 'T2' (3..8 correspondences consistent with T1 / T2 = T1 moved by SHIFT), 'few' (1..2 of T1), 'none', 'outlier' (3..8 of T1
    and one correspondence `outlier` metres off both).  A planted entry is the only one of its row and column above the threshold, so
    the mutual top-k keeps exactly the planted entries of valid rows and columns.  Per-coordinate noise is uniform in +-noise, so inlier
    residuals under the planted transform stay below 2 * noise; a few rows and columns of every patch are masked.  counts: the number
    of correspondences of every patch instead of the random ones.
    Returns ref_knn (B, K, 3), src_knn, ref_masks (B, K), src_masks, log_scores (B, K, K) (float32), T1, T2 (4, 4 float64)."""
    B = len(kinds)
    T1 = np.eye(4)
    T1[:3, :3], T1[:3, 3] = random_rotation(rng), rng.uniform(-1, 1, 3)
    T2 = T1.copy()
    T2[:3, 3] += SHIFT
    src = np.zeros((B, K, 3))
    ref = rng.uniform(-2, 2, (B, K, 3))
    log_scores = np.log(rng.uniform(0.001, 0.04, (B, K, K)))
    ref_masks, src_masks = np.ones((B, K), bool), np.ones((B, K), bool)
    for b, kind in enumerate(kinds):
        src[b] = rng.uniform(-1.5, 1.5, 3) + rng.uniform(-0.3, 0.3, (K, 3))
        m = {'T1': rng.integers(3, 9), 'T2': rng.integers(3, 9), 'few': rng.integers(1, 3), 'none': 0,
             'outlier': rng.integers(3, 9) + 1}[kind] if counts is None else counts[b]
        rows, cols = rng.choice(K, m, replace=False), rng.choice(K, m, replace=False)
        T = T2 if kind == 'T2' else T1
        ref[b, rows] = src[b, cols] @ T[:3, :3].T + T[:3, 3] + rng.uniform(-noise, noise, (m, 3))
        if kind == 'outlier':       # off by `outlier` metres opposite to SHIFT: far from T1 and T2 alike
            ref[b, rows[-1]] -= outlier * SHIFT / np.linalg.norm(SHIFT)
        log_scores[b, rows, cols] = np.log(rng.uniform(0.2, 0.95, m))
        free_r, free_c = np.setdiff1d(np.arange(K), rows), np.setdiff1d(np.arange(K), cols)
        ref_masks[b, rng.choice(free_r, min(3, len(free_r)), replace=False)] = False
        src_masks[b, rng.choice(free_c, min(3, len(free_c)), replace=False)] = False
    return (ref.astype(np.float32), src.astype(np.float32), ref_masks, src_masks, log_scores.astype(np.float32), T1, T2)
