"""ICP refinement without a GPU: se3_debug_icp_host (the text of csrc/icp_core.h on host memory, in the kernels' summation order) against
the independent float64 twin tests/icp_twin.py on the seeded families of tests/icp_fixture.py, and on known-answer, degenerate and edge
cases that need no twin."""
import math

import numpy as np
import pytest

import icp_fixture as F
from icp_twin import EMPTY, NONFINITE, SINGULAR, STEP_REFUSED, TOO_FEW

MODES = ('point_to_point', 'point_to_plane')
# Transforms and rmse against the twin.  profiles/icp_probe.txt records the largest deviation over all fixture cases (tools/icp_probe.py,
# no GPU needed): 4.11e-15.  The bound is 16 times that, rounded up to a power of ten -- the margin covers seeds and the summation order
# -- and may not exceed 1e-8 on these unit-scale clouds: sums of <= 2048 float64 terms through systems of condition <= 1e3 stay far below.
TWIN_BOUND = 1e-13
assert TWIN_BOUND <= 1e-8


def test_status_bits_are_the_headers():
    from se3et_amd import ops
    assert ops.ICP_STATUS == {'nonfinite': NONFINITE, 'too_few': TOO_FEW, 'singular': SINGULAR, 'empty': EMPTY, 'step_refused': STEP_REFUSED}
    assert ops.ICP_MODES == F.MODES


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', sorted(F.FAMILIES))
def test_host_entry_equals_the_twin(name, mode, dtype):
    c = F.case(name, mode, dtype)
    twin = c['twin']
    got = F.host_icp(c['src'], c['ref'], c['T0'], c['r'], mode, c['normals'], trace=True)
    evals = twin['evaluations']
    for k, ev in enumerate(evals):
        assert np.array_equal(got['trace'][k], ev['corr']), 'evaluation %d: the correspondence sets differ' % k
    assert (got['trace'][len(evals):] == -2).all(), 'the library made more evaluations than the twin'
    assert np.array_equal(got['correspondences'], evals[-1]['corr'])
    assert (got['iterations'], got['converged'], got['status']) == (twin['iterations'], twin['converged'], twin['status'])
    n_corr, n = twin['fitness_ratio']
    assert got['fitness'] == n_corr / n
    dT, drmse = np.abs(got['transform'] - twin['transform']).max(), abs(got['rmse'] - twin['rmse'])
    print('%s %s %s: %d iterations, |dT| %.2e, |drmse| %.2e' % (name, mode, dtype, got['iterations'], dT, drmse))
    assert dT <= TWIN_BOUND and drmse <= TWIN_BOUND


def test_fixture_families_cover_the_stopping_cases():
    its = {(n, m): F.case(n, m, 'float64')['twin'] for n in F.FAMILIES for m in MODES}
    assert all(t['converged'] == 1 and t['fitness'] == 1.0 for (n, m), t in its.items() if n != 'partial1500')
    assert its[('sheet2048', 'point_to_point')]['iterations'] > 10          # a long run of small steps
    worn = its[('partial1500', 'point_to_point')]                           # the converged = 0 case: max_iteration reached
    assert (worn['iterations'], worn['converged']) == (30, 0) and 0.5 < worn['fitness'] < 0.9
    assert its[('partial1500', 'point_to_plane')]['converged'] == 1


@pytest.mark.parametrize('mode', MODES)
def test_exact_recovery_of_a_known_transform(mode):
    rng = np.random.default_rng(11)
    ref, nrm = F.sheet(rng, 600)
    gt = F.rigid(rng, 30.0, 0.4)
    inv = np.linalg.inv(gt)
    src = ref[rng.permutation(600)[:500]] @ inv[:3, :3].T + inv[:3, 3]
    got = F.host_icp(src, ref, F.rigid(rng, 3.0, 0.0) @ gt, 0.1, mode, nrm, max_iteration=60)
    assert got['converged'] == 1 and got['status'] == 0 and got['fitness'] == 1.0
    assert np.abs(got['transform'] - gt).max() < 1e-10
    assert got['rmse'] < 1e-10


def _sheet_pair(seed=5, nref=300, nsrc=200):
    rng = np.random.default_rng(seed)
    ref, nrm = F.sheet(rng, nref)
    return ref, nrm, ref[rng.permutation(nref)[:nsrc]] + 0.001 * rng.normal(size=(nsrc, 3)), rng


@pytest.mark.parametrize('mode', MODES)
def test_max_iteration_zero_only_evaluates(mode):
    ref, nrm, src, rng = _sheet_pair()
    T0 = F.rigid(rng, 2.0, 0.01)
    got = F.host_icp(src, ref, T0, 0.05, mode, nrm, max_iteration=0, trace=True)
    from scipy.spatial import cKDTree
    d, j = cKDTree(ref).query(src @ T0[:3, :3].T + T0[:3, 3])
    assert np.abs(d - 0.05).min() > 1e-9
    keep = d < 0.05
    assert np.array_equal(got['transform'], T0) and (got['iterations'], got['converged'], got['status']) == (0, 0, 0)
    assert got['fitness'] == keep.sum() / len(src) and 0 < keep.sum() < len(src)
    assert abs(got['rmse'] - np.sqrt((d[keep] ** 2).sum() / keep.sum())) < 1e-15
    assert np.array_equal(got['correspondences'], np.where(keep, j, -1)) and np.array_equal(got['trace'][0], got['correspondences'])


@pytest.mark.parametrize('mode', MODES)
def test_an_exact_initial_transform_converges_at_the_first_comparison(mode):
    ref, nrm, _src, rng = _sheet_pair()
    gt = F.rigid(rng, 20.0, 0.3)
    inv = np.linalg.inv(gt)
    src = ref[:150] @ inv[:3, :3].T + inv[:3, 3]
    got = F.host_icp(src, ref, gt, 0.05, mode, nrm)
    assert (got['iterations'], got['converged'], got['status'], got['fitness']) == (1, 1, 0, 1.0)
    assert np.abs(got['transform'] - gt).max() < 1e-14 and got['rmse'] < 1e-14
    assert np.array_equal(got['correspondences'], np.arange(150))


@pytest.mark.parametrize('mode,count', [('point_to_point', 2), ('point_to_plane', 5), ('point_to_point', 3), ('point_to_plane', 6)])
def test_too_few_correspondences_give_the_identity_update(mode, count):
    ref, nrm, _src, rng = _sheet_pair()
    src = np.concatenate([ref[:count] + 0.004, ref[:7] + np.array([0.0, 0.0, 5.0])], 0)       # `count` rows near the sheet, 7 far above it
    T0 = np.eye(4)
    got = F.host_icp(src, ref, T0, 0.02, mode, nrm)
    few = count in (2, 5)
    assert got['fitness'] == count / len(src) and np.array_equal(got['correspondences'][:count], np.arange(count))
    assert (got['correspondences'][count:] == -1).all()
    if few:                                               # the identity update: unchanged, so converged at the first comparison
        assert (got['iterations'], got['converged'], got['status']) == (1, 1, TOO_FEW)
        assert np.array_equal(got['transform'], T0)
    else:                                                 # one correspondence more and the update is estimated
        assert not got['status'] & TOO_FEW and not np.array_equal(got['transform'], T0)


def test_a_planar_reference_is_singular_for_point_to_plane():
    g = np.arange(12.0) * 0.1
    ref = np.stack([np.repeat(g, 12), np.tile(g, 12), np.zeros(144)], 1)
    nrm = np.tile([0.0, 0.0, 1.0], (144, 1))
    src = ref[20:100] + np.array([0.013, -0.021, 0.004])                  # slid in the plane and lifted off it
    got = F.host_icp(src, ref, np.eye(4), 0.045, 'point_to_plane', nrm)
    assert (got['iterations'], got['converged'], got['status'], got['fitness']) == (1, 1, SINGULAR, 1.0)
    assert np.array_equal(got['transform'], np.eye(4))
    free = F.host_icp(src, ref, np.eye(4), 0.045, 'point_to_point')       # point-to-point has no such freedom: it slides back
    assert free['status'] == 0 and free['converged'] == 1 and free['rmse'] < 1e-12


@pytest.mark.parametrize('mode', MODES)
def test_all_source_points_beyond_the_distance(mode):
    ref, nrm, src, _rng = _sheet_pair()
    T0 = np.eye(4)
    T0[2, 3] = 3.0
    got = F.host_icp(src, ref, T0, 0.05, mode, nrm)
    assert (got['fitness'], got['rmse'], got['converged'], got['iterations'], got['status']) == (0.0, 0.0, 1, 1, TOO_FEW)
    assert np.array_equal(got['transform'], T0) and (got['correspondences'] == -1).all()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('which', ['src', 'ref', 'both'])
def test_empty_clouds(mode, which):
    ref, nrm, src, rng = _sheet_pair()
    if which in ('src', 'both'):
        src = src[:0]
    if which in ('ref', 'both'):
        ref, nrm = ref[:0], nrm[:0]
    T0 = F.rigid(rng, 5.0, 0.1)
    got = F.host_icp(src, ref, T0, 0.05, mode, nrm)
    assert (got['fitness'], got['rmse'], got['converged'], got['iterations'], got['status']) == (0.0, 0.0, 1, 1, EMPTY)
    assert np.array_equal(got['transform'], T0) and (got['correspondences'] == -1).all()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('where', ['src', 'ref', 'T0', 'normals'])
def test_non_finite_input_refuses_the_pair(mode, where):
    ref, nrm, src, _rng = _sheet_pair()
    ref, nrm, src, T0 = ref.copy(), nrm.copy(), src.copy(), np.eye(4)
    {'src': src, 'ref': ref, 'T0': T0, 'normals': nrm}[where][1, 2] = np.nan if mode == MODES[0] else np.inf
    got = F.host_icp(src, ref, T0, 0.05, mode, nrm)
    if where == 'normals' and mode == 'point_to_point':          # the normals are not read
        assert got['status'] == 0 and got['converged'] == 1
        return
    assert got['status'] == NONFINITE and got['converged'] == 0 and got['iterations'] == 0
    assert np.isnan(got['transform']).all() and (got['correspondences'] == -1).all()


def test_a_step_of_one_radian_is_refused():
    """Constructed so that the least-squares step is x* exactly: p_i = q_i + d_i n_i has J_i = [q_i x n_i, n_i] and residual d_i, and
    d_i = -J_i x* makes x* the solution with zero residual.  Normals near the radial direction keep q x n, and with it d, small enough
    for every p_i to stay nearest to its own q_i."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(3)
    q = rng.uniform(-1.0, 1.0, (12, 3))
    n = q / np.linalg.norm(q, axis=1, keepdims=True) + 0.1 * rng.normal(size=q.shape)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    J = np.concatenate([np.cross(q, n), n], 1)
    for angle, refused in ((1.05, True), (0.95, False)):
        x = np.array([angle, 0.1, -0.2, 0.01, 0.02, 0.03])
        p = q - (J @ x)[:, None] * n
        assert np.array_equal(cKDTree(q).query(p)[1], np.arange(12))
        got = F.host_icp(p, q, np.eye(4), 2.0, 'point_to_plane', n, max_iteration=1)
        if refused:                                      # ends at its previous transform, not converged
            assert (got['iterations'], got['converged'], got['status']) == (0, 0, STEP_REFUSED)
            assert np.array_equal(got['transform'], np.eye(4)) and np.array_equal(got['correspondences'], np.arange(12))
        else:                                            # just below: the step is taken, U = Rz Ry Rx | t of x*
            assert got['status'] == 0 and got['iterations'] == 1
            cx, sx, cy, sy, cz, sz = math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2])
            R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
                np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
            assert np.abs(got['transform'][:3, :3] - R).max() < 1e-11 and np.abs(got['transform'][:3, 3] - x[3:]).max() < 1e-11


def test_shared_sine_and_cosine_series_within_four_ulp():
    from se3et_amd._lib import check, lib
    x = np.random.default_rng(0).uniform(-1.0, 1.0, 1000)
    x[:4] = [0.0, 1e-300, -0.9999999999999999, 0.9999999999999999]
    s, c = np.zeros_like(x), np.zeros_like(x)
    check(lib().se3_debug_icp_sincos_host(x.ctypes.data, len(x), s.ctypes.data, c.ctypes.data), 'se3_debug_icp_sincos_host')
    for xi, si, ci in zip(x.tolist(), s.tolist(), c.tolist()):
        assert abs(si - math.sin(xi)) <= 4 * math.ulp(math.sin(xi)), xi
        assert abs(ci - math.cos(xi)) <= 4 * math.ulp(math.cos(xi)), xi
    bad = np.array([1.0])
    assert lib().se3_debug_icp_sincos_host(bad.ctypes.data, 1, s.ctypes.data, c.ctypes.data) != 0


def test_argument_validation_of_the_host_entry():
    ref, nrm, src, _rng = _sheet_pair()
    for kw in (dict(r=-1.0), dict(r=np.nan), dict(max_iteration=-1), dict(max_iteration=10 ** 6), dict(relative_rmse=-1.0)):
        args = dict(r=0.05, max_iteration=30, relative_rmse=1e-6)
        args.update(kw)
        with pytest.raises(RuntimeError, match='debug_icp_host'):
            F.host_icp(src, ref, np.eye(4), args['r'], 'point_to_point', None, relative_rmse=args['relative_rmse'], max_iteration=args['max_iteration'])
    with pytest.raises(RuntimeError, match='needs the reference normals'):
        F.host_icp(src, ref, np.eye(4), 0.05, 'point_to_plane', None)


def test_batched_functions_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from se3et_amd import icp
    a = torch.zeros((4, 3))
    with pytest.raises(RuntimeError, match='GPU tensor'):
        icp.icp_pairs([a], [a], np.eye(4)[None], 0.1)
    with pytest.raises(ValueError, match='estimation'):
        icp.icp_pairs([a], [a], np.eye(4)[None], 0.1, estimation='generalized')
    with pytest.raises(ValueError, match='max_correspondence_distance'):
        icp.icp_pairs([a], [a], np.eye(4)[None], float('nan'))
    with pytest.raises(ValueError, match='one source and one reference'):
        icp.icp_pairs([a], [], np.eye(4)[None], 0.1)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        icp.refine_pairs([], np.eye(4)[None], 0.1)
