"""CPU: the float64 twin of the LGR kernels (tests/lgr_twin.py) that tests/test_gpu_registration.py holds the kernels to."""
import numpy as np
import torch

import lgr_twin as LT


def _planted(rng):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = LT.random_rotation(rng), rng.uniform(-1, 1, 3)
    return T


def test_twin_recovers_a_planted_transform():
    rng = np.random.default_rng(0)
    for n in (3, 4, 64, 1000):
        T = _planted(rng)
        src = rng.uniform(-1, 1, (n, 3))
        ref = src @ T[:3, :3].T + T[:3, 3]
        w = rng.uniform(0.1, 1, n)
        assert np.abs(LT.procrustes(src, ref, w)['R'] - T[:3, :3]).max() < 1e-9, n
        assert np.abs(LT.procrustes(src, ref, w, eps=0.0)['T'] - T).max() < 1e-9, n     # (eps shrinks the centroids, so t)
        # rows with negative weights do not count, whatever they hold
        bad = np.concatenate([ref, ref + 5.0])
        got = LT.procrustes(np.concatenate([src, src]), bad, np.concatenate([w, -w]), eps=0.0)['T']
        assert np.abs(got - T).max() < 1e-9, n


def test_twin_zero_weights_give_the_identity():
    rng = np.random.default_rng(1)
    src, ref = rng.uniform(-1, 1, (10, 3)), rng.uniform(-1, 1, (10, 3))
    assert np.array_equal(LT.procrustes(src, ref, np.zeros(10))['T'], np.eye(4))
    assert np.array_equal(LT.procrustes(src[:0], ref[:0], np.zeros(0))['T'], np.eye(4))


def test_twin_maximises_the_objective_when_h_is_rank_deficient():
    """Collinear points, one src point matched to three ref points, a single weighted row (rank 1: R is not determined), a mirrored
    plane (rank 2: it is): the twin's R must reach sigma1 + sigma2 + d sigma3, which no rotation exceeds."""
    rng = np.random.default_rng(2)
    T = _planted(rng)
    line = np.outer(rng.uniform(-1, 1, 20), [0.3, -0.5, 0.8])
    p = rng.uniform(-1, 1, 3)
    plane = rng.uniform(-1, 1, (30, 3)) * [1, 1, 0]
    cases = {
        'collinear': (line, line @ T[:3, :3].T + T[:3, 3], rng.uniform(0.1, 1, 20)),
        'shared src point': (np.repeat(p[None], 3, 0), rng.uniform(-1, 1, (3, 3)), rng.uniform(0.1, 1, 3)),
        'one weight': (plane, rng.uniform(-1, 1, (30, 3)), np.where(np.arange(30) == 4, 0.5, 0.0)),
        'mirrored plane': (plane, plane * [-1, 1, 1], np.ones(30)),
    }
    Q = np.stack([LT.random_rotation(rng) for _ in range(2000)])
    for name, (src, ref, w) in cases.items():
        sol = LT.procrustes(src, ref, w)
        R = sol['R']
        assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12, name
        best = np.trace(R @ sol['H'])
        assert abs(best - LT.optimum(sol)) <= 1e-12 * sol['sv'].sum() + 1e-300, name
        assert np.einsum('qij,ji->q', Q, sol['H']).max() <= best + 1e-12 * sol['sv'].sum() + 1e-300, name
        assert LT.unique(sol) == (name == 'mirrored plane'), name


def test_twin_matches_the_oracle_on_generic_inputs():
    from oracle import se3et_oracle as O
    rng = np.random.default_rng(3)
    src = rng.uniform(-1, 1, (8, 100, 3)).astype(np.float32)
    ref = np.stack([s @ _planted(rng)[:3, :3].T for s in src]) + rng.normal(scale=0.02, size=(8, 100, 3))
    ref = ref.astype(np.float32)
    w = rng.uniform(-0.2, 1, (8, 100)).astype(np.float32)
    want = O.weighted_procrustes(torch.from_numpy(src), torch.from_numpy(ref), torch.from_numpy(w)).numpy()
    for b in range(8):
        assert np.abs(LT.procrustes(src[b], ref[b], w[b])['T'] - want[b]).max() <= 1e-5, b


def test_twin_gate_and_count():
    """Gate: score * [residual < radius], a NaN score stays NaN (NaN * 0) and so does the solve; the band flags residuals within
    1e-5 (1 + |s| + |r|) of the radius; count_inliers over a range."""
    src = np.zeros((4, 3))
    ref = np.array([[0.05, 0, 0], [0.1, 0, 0], [0.1 + 5e-6, 0, 0], [0.3, 0, 0]])
    w, band = LT.gated_weights(src, ref, [1.0, 2.0, np.nan, np.nan], np.eye(4), 0.1)
    assert w[0] == 1 and w[1] == 0 and np.isnan(w[2]) and np.isnan(w[3])
    assert band.tolist() == [False, True, True, False]
    assert np.isnan(LT.procrustes(src, ref, w)['T'][:3]).all()
    assert LT.count_inliers(src, ref, np.eye(4), 0.1) == (1, 2)
    assert LT.count_inliers(src, ref, np.eye(4), 0.1, 1, 4) == (0, 2)
    assert LT.count_inliers(src, ref, np.eye(4), 0.1, 2, 2) == (0, 0)


def test_twin_mutual_topk_on_hand_made_matrices():
    """Ranks count the strictly greater entries and the equal ones at a lower index; masked rows still rank; the threshold is strict."""
    S = np.array([[[0.5, 0.5, 0.2], [0.5, 0.9, 0.5], [0.1, 0.5, 0.5]]], np.float32)
    ones = np.ones((1, 3), bool)
    assert LT.mutual_topk(S, ones, ones, 1, 0.05)[0].astype(int).tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 0]]
    assert LT.mutual_topk(S, ones, ones, 2, 0.05)[0].astype(int).tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 1]]
    assert LT.mutual_topk(S, ones, ones, 2, 0.5)[0].astype(int).tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]
    rows = np.array([[True, False, True]])
    assert LT.mutual_topk(S, rows, ones, 2, 0.05)[0].astype(int).tolist() == [[1, 1, 0], [0, 0, 0], [0, 0, 1]]
    # NaN: never kept, never ahead
    N = np.array([[[np.nan, 0.3, 0.2]]], np.float32)
    assert LT.mutual_topk(N, np.ones((1, 1), bool), ones, 1, 0.05)[0].astype(int).tolist() == [[0, 1, 0]]


def test_twin_mutual_topk_agrees_with_topk_and_scatter_without_ties():
    """On distinct scores the rank rule is the reference's formulation: torch.topk along rows and columns, scatter, threshold, masks."""
    rng = np.random.default_rng(4)
    for B, R, C, k in ((3, 20, 30, 3), (2, 64, 64, 2), (4, 7, 5, 6)):
        S = rng.permutation(B * R * C).reshape(B, R, C).astype(np.float32) / (B * R * C)
        rm, cm = rng.random((B, R)) > 0.2, rng.random((B, C)) > 0.2
        t = torch.from_numpy(S)
        kr, kc = min(k, C), min(k, R)
        rs, ri = t.topk(kr, dim=2)
        row = torch.zeros_like(t).scatter_(2, ri, rs) > 0.05
        cs, ci = t.topk(kc, dim=1)
        col = torch.zeros_like(t).scatter_(1, ci, cs) > 0.05
        want = (row & col & torch.from_numpy(rm)[:, :, None] & torch.from_numpy(cm)[:, None, :]).numpy()
        assert np.array_equal(LT.mutual_topk(S, rm, cm, k, 0.05), want), (B, R, C, k)


def test_twin_lgr_on_planted_pairs():
    """A mixed pair recovers T1 and the first of the tied T1 patches wins; two equal votes go to the first patch; patches below the
    correspondence threshold take the degenerate branch; no correspondence gives the identity.  No vote or gate in the band."""
    rng = np.random.default_rng(5)

    def run(*args, **kw):
        ref, src, rm, sm, log, T1, T2 = LT.synthetic_lgr_pair(rng, *args, **kw)
        res = LT.lgr_pair(ref, src, rm, sm, np.exp(log), 3, 0.05, 0.1, 3, 5)
        assert LT.decisive(res) and sum(res['step_band']) == 0
        return res, T1, T2

    res, T1, _ = run(['T2', 'outlier', 'T1', 'few', 'none', 'T1', 'T1', 'T2'])
    assert np.abs(res['T'] - T1).max() < 5e-3 and res['best'] == 2
    res, _, T2 = run(['T2', 'none', 'T1'], noise=0.0, counts=[5, 0, 5])
    assert res['votes'][0] == res['votes'][2] and res['best'] == 0 and np.abs(res['T'] - T2).max() < 1e-4
    res, T1, _ = run(['few'] * 8)
    assert res['best'] == -1 and len(res['corr_scores']) >= 3 and np.abs(res['T'] - T1).max() < 5e-3
    res, _, _ = run(['none'] * 4)
    assert len(res['corr_scores']) == 0 and np.array_equal(res['T'], np.eye(4))
