"""GPU: the local-to-global registration (LGR) kernels -- csrc/registration.hip (weighted Procrustes, inlier votes, mutual top-k mask)
and the float64 Kabsch solve of csrc/kabsch.h -- against the float64 twin of tests/lgr_twin.py.

Every weighted-Procrustes result is held to the contract whether or not its R is unique: a proper rotation (|det R - 1| and
|R R^T - I| <= 1e-6), a maximiser of the Procrustes objective (trace(R H) >= sigma1 + sigma2 + d sigma3 - 1e-6 sum(sigma) on the
twin's float64 H), and t = rc - R sc within 1e-6 (1 + max |coordinate|).  Where R is well determined (lgr_twin.unique: sigma2 +
d sigma3 >= 1e-3 sigma1) it is also held within 1e-6 of the twin's.  Residual thresholds (gates, votes) are compared outside the twin's
band; the planted cases are built so that no row falls in it, and the tests assert that."""
import itertools
import os

import numpy as np
import pytest
import torch

import lgr_twin as LT

pytestmark = pytest.mark.gpu

OFFSET_DIR = np.array([0.6, -0.48, 0.64])          # unit vector: the offsets move every case away from the origin along it
THRESHOLD = 0.05                                   # the configurations' confidence threshold


def _cuda(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _planted(rng):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = LT.random_rotation(rng), rng.uniform(-1, 1, 3)
    return T


def _solve(problems, gates=None, radius=0.0):
    """ONE weighted_procrustes launch over problems [(src, ref, w)] as segments; gates None, one (4, 4) or (S, 4, 4)."""
    from se3et_amd import functional as SF
    offsets = np.concatenate([[0], np.cumsum([len(p[2]) for p in problems])]).astype(np.int64)
    src = np.concatenate([np.asarray(p[0], np.float32).reshape(-1, 3) for p in problems])
    ref = np.concatenate([np.asarray(p[1], np.float32).reshape(-1, 3) for p in problems])
    w = np.concatenate([np.asarray(p[2], np.float32).reshape(-1) for p in problems])
    gate = None if gates is None else _cuda(gates)
    T = SF.weighted_procrustes(_cuda(src), _cuda(ref), _cuda(w), _cuda(offsets, torch.int64), gate_transform=gate, gate_radius=radius)
    return T.cpu().numpy().astype(np.float64)


def _check(T, sol, src, ref, context):
    """The contract of one solve (module docstring) against the twin's solution; returns whether R was compared."""
    R, t = T[:3, :3], T[:3, 3]
    assert np.isfinite(T).all() and np.array_equal(T[3], [0, 0, 0, 1]), context
    assert abs(np.linalg.det(R) - 1) <= 1e-6, '%s: det R = %.9f' % (context, np.linalg.det(R))
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6, '%s: R R^T - I = %.2e' % (context, np.abs(R @ R.T - np.eye(3)).max())
    S = sol['sv']
    gap = LT.optimum(sol) - np.trace(R @ sol['H'])
    assert gap <= 1e-6 * S.sum(), '%s: trace(R H) %.3e below the optimum (singular values %s)' % (context, gap, S)
    scale = 1.0 + max(np.abs(src).max(initial=0), np.abs(ref).max(initial=0))
    err = np.abs(t - (sol['rc'] - R @ sol['sc'])).max()
    assert err <= 1e-6 * scale, '%s: t off rc - R sc by %.2e' % (context, err)
    if LT.unique(sol):
        err = np.abs(R - sol['R']).max()
        assert err <= 1e-6, '%s: R off the twin by %.2e (singular values %s)' % (context, err, S)
        return True
    return False


def _cases(rng, T=None):
    """Weighted-Procrustes problems at the kernel's edges: [(name, src, ref, w, planted T)] in float32; the planted T is None for the
    mirrored ones.  T: one planted transform for every case (else one each)."""
    out = []

    def add(name, src, w, noise=0.0, mirror=False):
        Tc = _planted(rng) if T is None else T
        src = np.asarray(src, np.float32).astype(np.float64)
        M = np.diag([-1.0, 1.0, 1.0]) if mirror else np.eye(3)
        ref = (src @ M) @ Tc[:3, :3].T + Tc[:3, 3] + rng.uniform(-noise, noise, src.shape)
        out.append((name, src.astype(np.float32), ref.astype(np.float32), np.asarray(w, np.float32), None if mirror else Tc))

    for n in (0, 1, 2, 3, 4, 64, 4096, 100000):
        add('generic n=%d' % n, rng.uniform(-0.5, 0.5, (n, 3)), rng.uniform(0.05, 1, n), 0.01 if n > 4 else 0.0)
    cube = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)])
    for off in (0.0, 80.0, 1e3):
        o = off * OFFSET_DIR
        g = rng.uniform(-0.5, 0.5, (64, 3))
        w = rng.uniform(0.05, 1, 64)
        add('generic off=%g' % off, g + o, w, 0.01)
        add('mirrored off=%g' % off, g + o, w, 0.01, mirror=True)
        p = g * [1, 1, 0]
        add('planar off=%g' % off, p + o, w, 0.01)
        add('mirrored planar off=%g' % off, p + o, w, 0.01, mirror=True)
        add('planar 1e-4 thick off=%g' % off, p + [0, 0, 1] * rng.uniform(-5e-5, 5e-5, (64, 1)) + o, w)
        line = g * [1, 0, 0]
        add('collinear off=%g' % off, line + o, w)
        add('collinear + 1e-3 noise off=%g' % off, line + rng.uniform(-1e-3, 1e-3, (64, 3)) + o, w, 1e-3)
        add('isotropic off=%g' % off, cube + o, np.ones(8))
        add('near-isotropic off=%g' % off, cube * [1, 1 + 1e-4, 0.6] + o, np.ones(8))
        add('shared src point off=%g' % off, np.repeat(g[:1], 3, 0) + o, w[:3], 0.1)        # one src point, three ref points
        add('negative weights off=%g' % off, g + o, rng.uniform(-1, 1, 64), 0.01)
        add('one weight off=%g' % off, g + o, np.where(np.arange(64) == 5, w, 0), 0.01)
        add('zero weights off=%g' % off, g + o, np.zeros(64), 0.01)
    return out


def _identity_expected(name):
    return name.startswith(('generic n=0', 'zero weights'))


def test_procrustes_cases_hold_the_contract():
    """Segment lengths 0 .. 100 000, planar / collinear / mirrored / isotropic geometry, negative / single / zero weights, offsets 0, 80
    and 1e3 m, all as the segments of one launch; no weight or no row gives exactly the identity."""
    cases = _cases(np.random.default_rng(11))
    got = _solve([c[1:4] for c in cases])
    compared = []
    for T, (name, src, ref, w, _) in zip(got, cases):
        if _identity_expected(name):
            assert np.array_equal(T, np.eye(4)), name
            continue
        if _check(T, LT.procrustes(src, ref, w), src, ref, name):
            compared.append(name)
    for name in ('generic n=4', 'generic n=64', 'generic n=100000', 'generic off=1000', 'mirrored off=80', 'negative weights off=1000'):
        assert name in compared, '%s: R is expected to be unique and compared' % name


def test_procrustes_tiny_h_reaches_the_optimum():
    """H of norm 1e-12 .. 1e-9: three correspondences that share one src point (rank 1, the case the whole-forward edge tests meet),
    one non-zero weight, 3- and 4-point patches 1e-5 m across.  The eigen-solve must still rotate: the result is a Procrustes optimum,
    and the unique ones match the twin."""
    rng = np.random.default_rng(12)
    problems = []
    for off in (0.0, 1.0, 80.0):
        o = off * OFFSET_DIR
        T = _planted(rng)
        p = rng.uniform(-0.5, 0.5, 3) + o
        src = np.repeat(p[None], 3, 0)
        problems.append(('shared src point off=%g' % off, src, src @ T[:3, :3].T + T[:3, 3] + rng.uniform(-0.1, 0.1, (3, 3)),
                         rng.uniform(0.05, 1, 3)))
        g = rng.uniform(-0.5, 0.5, (16, 3)) + o
        problems.append(('one weight off=%g' % off, g, g @ T[:3, :3].T + T[:3, 3], np.where(np.arange(16) == 3, 0.7, 0.0)))
        for n in (3, 4):
            g = rng.uniform(-5e-6, 5e-6, (n, 3)) + o * 1e-5
            problems.append(('%d points 1e-5 m across off=%g' % (n, off * 1e-5), g, g @ T[:3, :3].T + T[:3, 3] * 1e-5,
                             rng.uniform(0.05, 1, n)))
    problems = [(name, np.asarray(s, np.float32), np.asarray(r, np.float32), np.asarray(w, np.float32)) for name, s, r, w in problems]
    got = _solve([p[1:] for p in problems])
    compared = [name for T, (name, src, ref, w) in zip(got, problems) if _check(T, LT.procrustes(src, ref, w), src, ref, name)]
    assert '4 points 1e-5 m across off=0' in compared


def test_procrustes_scale_sweep_is_invariant():
    """The same problems scaled by 2^-14 .. 2^14 (about 6e-5 .. 1.6e4; a 0.1 m patch becomes 6 um .. 1.6 km): scaling by a power of two
    is exact in float32 and in the kernel's float64 moments, so R must be bit-identical and t scaled exactly, and every scale holds the
    contract against the twin."""
    rng = np.random.default_rng(13)
    base = []
    for n, kind in ((3, 'generic'), (4, 'generic'), (64, 'generic'), (64, 'planar')):
        src = rng.uniform(-0.05, 0.05, (n, 3)) * ([1, 1, 0] if kind == 'planar' else 1)
        T = _planted(rng)
        ref = src @ T[:3, :3].T + 0.1 * T[:3, 3] + rng.uniform(-1e-3, 1e-3, (n, 3)) * (n > 4)
        base.append(('%s n=%d' % (kind, n), src.astype(np.float32), ref.astype(np.float32), rng.uniform(0.05, 1, n).astype(np.float32)))
    exps = list(range(-14, 15, 2))
    problems = [('%s scale 2^%d' % (name, e), s * np.float32(2.0 ** e), r * np.float32(2.0 ** e), w)
                for e in exps for name, s, r, w in base]
    got = _solve([p[1:] for p in problems]).reshape(len(exps), len(base), 4, 4)
    unit = got[exps.index(0)]
    for i, e in enumerate(exps):
        for j, (name, _, _, _) in enumerate(base):
            name, src, ref, w = problems[i * len(base) + j]
            _check(got[i, j], LT.procrustes(src, ref, w), src, ref, name)
            assert np.array_equal(got[i, j, :3, :3], unit[j, :3, :3]), '%s: R depends on the scale' % name
            assert np.array_equal(got[i, j, :3, 3], unit[j, :3, 3] * 2.0 ** e), '%s: t does not scale with the problem' % name


def _gated_problems(rng, cases, radius):
    """Each case plus a quarter of its rows again with the ref point moved 6 radii off the planted transform (same weights): the gate
    must drop exactly those.  Returns [(name, src, ref, w, T_gate float32)]."""
    out = []
    for name, src, ref, w, T in cases:
        m = len(src) // 4 + (len(src) > 0)
        far = ref[:m].astype(np.float64) + 6 * radius * OFFSET_DIR
        out.append((name, np.concatenate([src, src[:m]]), np.concatenate([ref, far.astype(np.float32)]), np.concatenate([w, w[:m]]),
                    T.astype(np.float32)))
    return out


@pytest.mark.parametrize('form', ['shared', 'per_segment'])
def test_procrustes_gated_cases_hold_the_contract(form):
    """The refinement form: weights score * [ |r - T s| < radius ] under one gate transform for all segments, or one per segment."""
    rng = np.random.default_rng(14 if form == 'shared' else 15)
    radius = 0.5
    T0 = _planted(rng)
    cases = [c for c in _cases(rng, T0 if form == 'shared' else None) if c[4] is not None]
    problems = _gated_problems(rng, cases, radius)
    gates = problems[0][4] if form == 'shared' else np.stack([p[4] for p in problems])
    got = _solve([p[1:4] for p in problems], gates, radius)
    compared = 0
    for T, (name, src, ref, w, Tg) in zip(got, problems):
        wg, band = LT.gated_weights(src, ref, w, Tg, radius)
        assert not band.any(), '%s: %d rows in the band of the gate' % (name, band.sum())
        if _identity_expected(name):
            assert np.array_equal(T, np.eye(4)), name
            continue
        compared += _check(T, LT.procrustes(src, ref, wg), src, ref, name + ' (gated)')
    assert compared >= 10


@pytest.mark.parametrize('gated', [False, True])
def test_procrustes_nan_stays_in_its_segment(gated):
    """A NaN score, src or ref coordinate makes its own segment's transform NaN (rotation and translation) and leaves the others
    bit-identical.  Gated, the NaN score sits on a row the gate drops: score * 0 is NaN, as in the reference's re-weighting."""
    rng = np.random.default_rng(16)
    T = _planted(rng)
    radius = 0.5
    problems = []
    for _ in range(5):
        src = rng.uniform(-0.5, 0.5, (300, 3))
        ref = src @ T[:3, :3].T + T[:3, 3] + rng.uniform(-0.01, 0.01, (300, 3))
        ref[:50] += 6 * radius * OFFSET_DIR
        problems.append([src.astype(np.float32), ref.astype(np.float32), rng.uniform(0.05, 1, 300).astype(np.float32)])
    gates = T.astype(np.float32) if gated else None
    clean = _solve(problems, gates, radius)
    bad = [[a.copy() for a in p] for p in problems]
    bad[1][2][7] = np.nan
    bad[2][0][100, 1] = np.nan
    bad[3][1][200, 2] = np.nan
    got = _solve(bad, gates, radius)
    for s in (1, 2, 3):
        assert np.isnan(got[s][:3]).all(), 'segment %d: %s' % (s, got[s][:3])
    for s in (0, 4):
        assert np.isfinite(clean[s]).all() and np.array_equal(got[s], clean[s]), 'segment %d changed' % s


def _turn(R, rng, max_angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(0, max_angle)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return (np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K) @ R


def test_count_inliers_and_ranges_match_the_twin():
    """4096 transforms (16 pairs x 256 hypotheses) over their pairs' ranges, with empty ranges (inside and at the end), the whole stack
    and windows that overlap the neighbouring pairs; all pairs share the planted transform, so a range read from the wrong start
    counts other pairs' inliers.  Equal to the twin outside the band, off by at most the rows in it."""
    from se3et_amd import functional as SF
    rng = np.random.default_rng(17)
    T = _planted(rng)
    radius = 0.1
    sizes = rng.integers(100, 600, 16)
    sizes[5] = 0
    total = int(sizes.sum())
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    src = rng.uniform(-1.5, 1.5, (total, 3))
    ref = src @ T[:3, :3].T + T[:3, 3] + rng.uniform(-0.05, 0.05, (total, 3))
    out = rng.random(total) < 0.4
    ref[out] += rng.uniform(-1, 1, (int(out.sum()), 3))
    src, ref = src.astype(np.float32), ref.astype(np.float32)
    Ts = np.tile(np.eye(4), (4096, 1, 1))
    for h in range(4096):
        Ts[h, :3, :3] = _turn(T[:3, :3], rng, 0.05)
        Ts[h, :3, 3] = T[:3, 3] + rng.uniform(-0.05, 0.05, 3)
    Ts = Ts.astype(np.float32)
    lo, hi = np.repeat(bounds[:-1], 256), np.repeat(bounds[1:], 256)
    for p in range(16):
        h = 256 * p
        mid = (bounds[p] + bounds[p + 1]) // 2
        lo[h], hi[h] = mid, mid                                              # empty, inside the pair
        lo[h + 1], hi[h + 1] = 0, total                                      # the whole stack
        lo[h + 2], hi[h + 2] = max(0, bounds[p] - 70), min(total, bounds[p + 1] + 70)   # overlapping both neighbours
        lo[h + 3], hi[h + 3] = total, total                                  # empty, at the end
        lo[h + 4], hi[h + 4] = mid, bounds[p + 1]                            # the second half
    votes = SF.count_inliers(_cuda(src), _cuda(ref), _cuda(Ts), radius, _cuda(lo, torch.int64), _cuda(hi, torch.int64)).cpu().numpy()
    whole = SF.count_inliers(_cuda(src), _cuda(ref), _cuda(Ts[::97]), radius).cpu().numpy()
    want = np.array([LT.count_inliers(src, ref, Ts[h], radius, lo[h], hi[h]) for h in range(4096)])
    diff = np.abs(votes.astype(np.int64) - want[:, 0])
    assert np.all(diff <= want[:, 1]), np.flatnonzero(diff > want[:, 1])[:8]
    assert np.all(diff[want[:, 1] == 0] == 0)
    assert (want[:, 1] == 0).mean() > 0.5 and want[:, 0].min() == 0 and want[:, 0].max() > 500
    assert not votes[lo == hi].any()
    for i, h in enumerate(range(0, 4096, 97)):
        c, b = LT.count_inliers(src, ref, Ts[h], radius)
        assert abs(int(whole[i]) - c) <= b, h


MT_SHAPES = [(1, 1), (1, 64), (64, 1), (64, 64), (37, 90), (127, 128), (128, 128)]


def _topk_inputs(rng, B, R, C):
    """Scores in multiples of 1/64 (ties everywhere) with about 5 % exactly at the threshold; batch 4 below 0.1 (the threshold falls
    inside the top k), batch 5 one value.  Masks: batch 0 all valid, 1 no row, 2 no column, 3 nothing, the rest 10 % masked."""
    S = (rng.integers(0, 65, (B, R, C)) / 64.0).astype(np.float32)
    S[4] = (rng.integers(0, 103, (R, C)) / 1024.0).astype(np.float32)
    S[rng.random((B, R, C)) < 0.05] = np.float32(THRESHOLD)
    S[5] = 0.5
    rm, cm = rng.random((B, R)) > 0.1, rng.random((B, C)) > 0.1
    rm[0], cm[0], rm[1], cm[2], rm[3], cm[3] = True, True, False, False, False, False
    return S, rm, cm


def _topk(S, rm, cm, k, threshold=THRESHOLD):
    from se3et_amd import functional as SF
    return SF.mutual_topk_mask(_cuda(S), _cuda(rm, torch.bool), _cuda(cm, torch.bool), k, threshold).cpu().numpy()


@pytest.mark.parametrize('shape', MT_SHAPES)
def test_mutual_topk_matches_the_twin(shape):
    """Exactly the twin's mask for k = 1, 3, C - 1, C, C + 5 (128 x 128: 64 KiB of scores in LDS, the KITTI patch size)."""
    R, C = shape
    rng = np.random.default_rng(R * 1000 + C)
    S, rm, cm = _topk_inputs(rng, 6, R, C)
    at_threshold = False
    for k in sorted({1, 3, C - 1, C, C + 5} - {0}):
        want = LT.mutual_topk(S, rm, cm, k, THRESHOLD)
        got = _topk(S, rm, cm, k)
        assert np.array_equal(got, want), (shape, k, np.argwhere(got != want)[:5].tolist())
        at_threshold |= not np.array_equal(want, LT.mutual_topk(S, rm, cm, k, np.nextafter(np.float32(THRESHOLD), np.float32(0))))
    assert at_threshold or R * C <= 64, 'no entry at the threshold reached the comparison'


def test_mutual_topk_batches():
    """Batch 0 (no launch), 1 and 4096 patch pairs of 16 x 24."""
    rng = np.random.default_rng(18)
    for B in (0, 1, 4096):
        S = (rng.integers(0, 65, (B, 16, 24)) / 64.0).astype(np.float32)
        rm, cm = rng.random((B, 16)) > 0.1, rng.random((B, 24)) > 0.1
        got = _topk(S, rm, cm, 3)
        assert got.shape == (B, 16, 24) and np.array_equal(got, LT.mutual_topk(S, rm, cm, 3, THRESHOLD)), B


def test_mutual_topk_rejects_more_than_16384_entries():
    """Host-side validation: the score block must fit 64 KiB of LDS.  Nothing is launched."""
    for R, C in ((129, 128), (1, 16385), (200, 200)):
        with pytest.raises(RuntimeError, match='16384'):
            _topk(np.zeros((1, R, C), np.float32), np.ones((1, R), bool), np.ones((1, C), bool), 3)


def test_mutual_topk_nan_is_never_kept_and_never_ranks_ahead():
    """Pinned NaN behaviour (csrc/registration.hip header): a NaN score is never kept and takes no top-k slot -- unlike torch.topk, which
    ranks NaN first."""
    rng = np.random.default_rng(19)
    S, rm, cm = _topk_inputs(rng, 6, 64, 64)
    S[rng.random(S.shape) < 0.05] = np.nan
    S[0, 0, :], S[0, :, 1] = 0.1, 0.1
    S[0, 0, 0], S[0, 0, 1] = np.nan, 0.9
    for k in (1, 3, 64):
        got = _topk(S, rm, cm, k)
        assert np.array_equal(got, LT.mutual_topk(S, rm, cm, k, THRESHOLD)), k
        assert not got[np.isnan(S)].any()
        assert got[0, 0, 1], 'the NaN in row 0 took the top slot'


def _lgr():
    from se3et_amd.modules.geotransformer.local_global_registration import LocalGlobalRegistration
    return LocalGlobalRegistration(3, 0.1, mutual=True, confidence_threshold=THRESHOLD, correspondence_threshold=3, num_refinement_steps=5)


KINDS = ['T1', 'T2', 'outlier', 'few', 'none', 'T1', 'T1', 'T2']


def _on_device(pair):
    ref, src, rm, sm, log = pair[:5]
    return _cuda(ref), _cuda(src), _cuda(rm, torch.bool), _cuda(sm, torch.bool), _cuda(log)


def _twin_of(pair, dev):
    """The twin's LGR on the device's own exp() of the scores; the planted pair must leave no vote and no gate to the band."""
    tw = LT.lgr_pair(pair[0], pair[1], pair[2], pair[3], torch.exp(dev[4]).cpu().numpy(), 3, THRESHOLD, 0.1, 3, 5)
    assert LT.decisive(tw), 'a vote within the band: %s %s' % (tw['votes'], tw['vote_band'])
    assert sum(tw['step_band']) == 0, tw['step_band']
    return tw


def _assert_matches(got, tw, context):
    ref_c, src_c, sc, T = [x.cpu().numpy() for x in got]
    assert np.array_equal(ref_c, tw['ref_corr']) and np.array_equal(src_c, tw['src_corr']), '%s: correspondences' % context
    assert np.array_equal(sc, tw['corr_scores']), '%s: correspondence scores' % context
    err = np.abs(T.astype(np.float64) - tw['T']).max()
    assert err <= 1e-5, '%s: transform off the twin by %.2e' % (context, err)


def _run_and_compare(lgr, pairs):
    """registration_pairs on all pairs at once against the twin; every pair again alone and through LocalGlobalRegistration.forward:
    bit-identical."""
    from se3et_amd.batched import registration_pairs
    dev = [_on_device(p) for p in pairs]
    batch = registration_pairs(lgr, dev)
    twins = []
    for p, (pair, d) in enumerate(zip(pairs, dev)):
        twins.append(_twin_of(pair, d))
        _assert_matches(batch[p], twins[-1], 'pair %d of %d' % (p, len(pairs)))
        alone = registration_pairs(lgr, [d])[0]
        module = lgr(*d, None)
        for a, b, c in zip(batch[p], alone, module):
            assert torch.equal(a, b) and torch.equal(b, c), 'pair %d: batch / alone / module differ' % p
    return batch, twins


@pytest.mark.parametrize('num_pairs,patches', [(1, 'equal'), (2, 'equal'), (2, 'unequal'), (16, 'equal'), (16, 'unequal')])
def test_lgr_matches_the_twin(num_pairs, patches):
    """Planted pairs (lgr_twin.synthetic_lgr_pair: patches consistent with T1 or T2, outliers, patches under the correspondence threshold,
    empty patches): the same correspondences in the same order and the transform within 1e-5.  Equal and unequal patch counts take
    both branches of the vote in batched.registration_pairs."""
    rng = np.random.default_rng(20 + num_pairs + (patches == 'unequal'))
    nb = [16] * num_pairs if patches == 'equal' else [int(n) for n in rng.integers(6, 24, num_pairs)]
    if patches == 'unequal':
        assert len(set(nb)) > 1
    pairs = [LT.synthetic_lgr_pair(rng, list(rng.choice(KINDS, n))) for n in nb]
    _run_and_compare(_lgr(), pairs)


def test_lgr_special_pairs():
    """A pair without correspondences gives exactly the identity; a pair whose patches all hold fewer than 3 correspondences takes the
    degenerate branch (a solve on all of them); a T2 and a T1 hypothesis with equal votes: the first patch (T2) wins.  Alone and in a
    batch."""
    rng = np.random.default_rng(21)
    normal = LT.synthetic_lgr_pair(rng, KINDS * 2)
    zero = LT.synthetic_lgr_pair(rng, ['none'] * 6)
    degenerate = LT.synthetic_lgr_pair(rng, ['few'] * 10)
    tie = LT.synthetic_lgr_pair(rng, ['T2', 'none', 'T1'], noise=0.0, counts=[5, 0, 5])
    batch, twins = _run_and_compare(_lgr(), [normal, zero, degenerate, tie])
    assert batch[1][0].shape[0] == 0 and torch.equal(batch[1][3].cpu(), torch.eye(4))
    assert twins[2]['best'] == -1 and batch[2][0].shape[0] >= 3
    assert np.abs(batch[2][3].cpu().numpy() - degenerate[5]).max() < 0.02
    v = twins[3]['votes']
    assert v[0] == v[2] == 5 and twins[3]['best'] == 0
    assert np.abs(batch[3][3].cpu().numpy() - tie[6]).max() < 1e-4, 'the tie did not go to the first patch (T2)'
    assert batch[0][0].shape[0] > 0 and twins[0]['best'] >= 0
    # the zero pair alone (no correspondence anywhere in the call)
    from se3et_amd.batched import registration_pairs
    alone = registration_pairs(_lgr(), [_on_device(zero)])[0]
    assert alone[0].shape == (0, 3) and torch.equal(alone[3].cpu(), torch.eye(4))


@pytest.mark.parametrize('name,radius', [('c2_se3ete_5k', 0.1), ('c3_se3eti_kitti_20k', 0.6)])
def test_gated_solve_on_stored_correspondences(golden_dir, name, radius):
    """Real correspondence distributions: the LGR correspondences and estimated_transform stored with the forward fixtures (3DMatch
    pairs 0..7, the KITTI pair), one gated solve per pair from that transform in one launch.  Rows in the band may fall either way:
    the device must match the twin for one of their assignments."""
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    pairs = []
    for p in itertools.count():
        if 'p%d/corr_src_points' % p not in g.files:
            break
        pairs.append((g['p%d/corr_src_points' % p], g['p%d/corr_ref_points' % p], g['p%d/corr_scores' % p], g['p%d/estimated_transform' % p]))
    got = _solve([p[:3] for p in pairs], np.stack([p[3] for p in pairs]), radius)
    for p, (src, ref, score, T0) in enumerate(pairs):
        w, band = LT.gated_weights(src, ref, score, T0, radius)
        rows = np.flatnonzero(band)
        assert len(rows) <= 2, '%s pair %d: %d rows in the band' % (name, p, len(rows))
        sols = []
        for flip in itertools.product((False, True), repeat=len(rows)):
            wf = w.copy()
            for r, f in zip(rows, flip):
                if f:
                    wf[r] = score[r] - wf[r]
            sols.append(LT.procrustes(src, ref, wf))
        sol = min(sols, key=lambda s: np.abs(got[p][:3, :3] - s['R']).max())
        assert _check(got[p], sol, src, ref, '%s pair %d' % (name, p)), '%s pair %d: R is not determined' % (name, p)
