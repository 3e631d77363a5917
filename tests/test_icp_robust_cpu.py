"""Robust loss kernels and generalized ICP without a GPU: se3_debug_icp_weighted_host (the text of csrc/icp_core.h on host memory, in the
kernels' summation order) against the independent float64 twin tests/icp_robust_twin.py on the families of tests/icp_robust_fixture.py,
the bit-identity of the paths that existed before the losses, and known-answer, degenerate and refused cases that need no twin."""
import numpy as np
import pytest

import icp_fixture as F
import icp_robust_fixture as R
from icp_robust_twin import ESTIMATORS, LOSSES
from icp_twin import NONFINITE, SINGULAR, TOO_FEW

# Transforms and rmse against the twin.  profiles/icp_robust_probe.txt records the largest deviation over all 120 fixture cases
# (tools/icp_robust_probe.py, no GPU needed): 7.61e-14, on generalized + gm over the partial overlap.  The bound is 16 times that, rounded
# up to a power of ten -- the margin covers seeds and the summation order -- and may not exceed 1e-8 on these unit-scale clouds: sums of
# <= 2048 float64 terms through systems of condition <= 1e5 stay far below.
TWIN_BOUND = 1e-11
assert TWIN_BOUND <= 1e-8
OLD_MODES = ('point_to_point', 'point_to_plane')


def test_losses_and_the_third_mode_are_the_headers():
    from se3et_amd import _lib, ops
    assert ops.ICP_LOSSES == {k: v for k, v in R.LOSS_IDS.items() if k is not None}
    assert ops.ICP_WEIGHTED_MODES == R.ESTIMATORS and ops.ICP_GENERALIZED == 2
    assert _lib.ENUMS['se3_icp_option']['SE3_ICP_LOSS_NONE'] == R.LOSS_IDS[None]
    assert set(ops.ICP_LOSSES) == set(LOSSES) and set(ops.ICP_WEIGHTED_MODES) == set(ESTIMATORS)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('loss', LOSSES)
@pytest.mark.parametrize('mode', ESTIMATORS)
@pytest.mark.parametrize('name', sorted(R.FAMILIES))
def test_weighted_host_entry_equals_the_twin(name, mode, loss, dtype):
    c = R.case(name, mode, loss, dtype)
    twin = c['twin']
    got = R.host_weighted_icp(c['src'], c['ref'], c['T0'], c['r'], mode, c['normals'], c['src_normals'], loss, R.LOSS_K[loss], trace=True)
    evals = twin['evaluations']
    for k, ev in enumerate(evals):
        assert np.array_equal(got['trace'][k], ev['corr']), 'evaluation %d: the correspondence sets differ' % k
    assert (got['trace'][len(evals):] == -2).all(), 'the library made more evaluations than the twin'
    assert np.array_equal(got['correspondences'], evals[-1]['corr'])
    assert (got['iterations'], got['converged'], got['status']) == (twin['iterations'], twin['converged'], twin['status'])
    n_corr, n = twin['fitness_ratio']
    assert got['fitness'] == n_corr / n
    dT, drmse = np.abs(got['transform'] - twin['transform']).max(), abs(got['rmse'] - twin['rmse'])
    print('%s %s %s %s: %d iterations, |dT| %.2e, |drmse| %.2e' % (name, mode, loss, dtype, got['iterations'], dT, drmse))
    assert dT <= TWIN_BOUND and drmse <= TWIN_BOUND


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_a_robust_loss_ends_nearer_the_ground_truth_than_l2_on_the_outlier_family(seed):
    table = R.assert_robust_is_nearer(seed)
    assert set(table) == set(R.ROBUST_WINS)


def _bits(out):
    return tuple(np.ascontiguousarray(out[k]).tobytes() for k in ('transform', 'correspondences')) + tuple(
        out[k] for k in ('fitness', 'rmse', 'iterations', 'converged', 'status'))


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('mode', OLD_MODES)
@pytest.mark.parametrize('name', sorted(R.FAMILIES))
def test_no_loss_through_the_weighted_entry_is_the_old_entry_bit_for_bit(name, mode, dtype):
    c = R.inputs(name, dtype)
    old = F.host_icp(c['src'], c['ref'], c['T0'], c['r'], mode, c['normals'], trace=True)
    new = R.host_weighted_icp(c['src'], c['ref'], c['T0'], c['r'], mode, c['normals'], c['src_normals'], None, trace=True)
    assert _bits(new) == _bits(old) and np.array_equal(new['trace'], old['trace'])
    assert old['iterations'] >= 3


@pytest.mark.parametrize('mode', OLD_MODES)
@pytest.mark.parametrize('name', sorted(R.FAMILIES))
def test_l2_through_the_weight_code_agrees_with_no_loss(name, mode):
    c = R.inputs(name, 'float64')
    none = R.host_weighted_icp(c['src'], c['ref'], c['T0'], c['r'], mode, c['normals'], None, None)
    l2 = R.host_weighted_icp(c['src'], c['ref'], c['T0'], c['r'], mode, c['normals'], None, 'l2')
    assert (l2['iterations'], l2['converged'], l2['status'], l2['fitness']) == (none['iterations'], none['converged'], none['status'], none['fitness'])
    assert np.array_equal(l2['correspondences'], none['correspondences'])
    assert np.abs(l2['transform'] - none['transform']).max() <= TWIN_BOUND and abs(l2['rmse'] - none['rmse']) <= TWIN_BOUND


def _known(seed=11, nref=600, nsrc=500):
    rng = np.random.default_rng(seed)
    ref, nrm = F.sheet(rng, nref)
    gt = F.rigid(rng, 30.0, 0.4)
    inv = np.linalg.inv(gt)
    rows = rng.permutation(nref)[:nsrc]
    return ref, nrm, ref[rows] @ inv[:3, :3].T + inv[:3, 3], nrm[rows] @ gt[:3, :3], gt, F.rigid(rng, 3.0, 0.0) @ gt


@pytest.mark.parametrize('loss', [None, 'l2', 'huber'])
def test_generalized_recovers_a_known_transform_exactly(loss):
    ref, nrm, src, snr, gt, T0 = _known()
    got = R.host_weighted_icp(src, ref, T0, 0.1, 'generalized', nrm, snr, loss, 0.01, max_iteration=60)
    assert got['converged'] == 1 and got['status'] == 0 and got['fitness'] == 1.0
    assert np.abs(got['transform'] - gt).max() < 1e-10
    assert got['rmse'] < 1e-10


@pytest.mark.parametrize('loss', [None, 'cauchy'])
def test_generalized_does_not_depend_on_the_sign_of_a_normal(loss):
    c = R.inputs('sheet700', 'float64')
    run = lambda nrm, snr: R.host_weighted_icp(c['src'], c['ref'], c['T0'], c['r'], 'generalized', nrm, snr, loss, 0.01, trace=True)
    want = run(c['normals'], c['src_normals'])
    assert want['iterations'] >= 3 and want['status'] == 0
    rng = np.random.default_rng(0)
    flip = lambda a: np.ascontiguousarray(a * rng.choice([-1.0, 1.0], size=(len(a), 1)))
    for nrm, snr in ((-c['normals'], -c['src_normals']), (flip(c['normals']), flip(c['src_normals']))):
        got = run(np.ascontiguousarray(nrm), np.ascontiguousarray(snr))
        assert _bits(got) == _bits(want) and np.array_equal(got['trace'], want['trace'])


def test_generalized_with_epsilon_one_is_the_point_to_point_fixed_point():
    """epsilon = 1: M = 2 I, and the system is the Gauss-Newton step of the point-to-point objective.  Both loops are run until they stand
    still (the criteria at 1e-15, 100 iterations), so that they are compared at their fixed point and not where a 1e-6 test stopped them."""
    c = R.inputs('sheet700', 'float64')
    kw = dict(relative_fitness=1e-15, relative_rmse=1e-15, max_iteration=100)
    general = R.host_weighted_icp(c['src'], c['ref'], c['T0'], c['r'], 'generalized', c['normals'], c['src_normals'], 'l2', epsilon=1.0, **kw)
    point = F.host_icp(c['src'], c['ref'], c['T0'], c['r'], 'point_to_point', **kw)
    assert general['status'] == 0 and point['status'] == 0 and general['fitness'] == point['fitness'] == 1.0
    assert np.array_equal(general['correspondences'], point['correspondences'])
    assert np.abs(general['transform'] - point['transform']).max() <= 1e-8


def _sheet_pair(seed=5, nref=300, nsrc=200):
    rng = np.random.default_rng(seed)
    ref, nrm = F.sheet(rng, nref)
    rows = rng.permutation(nref)[:nsrc]
    return ref, nrm, ref[rows] + 0.001 * rng.normal(size=(nsrc, 3)), nrm[rows].copy(), rng


@pytest.mark.parametrize('mode', ESTIMATORS)
def test_tukey_below_every_residual_is_singular_with_the_identity_update(mode):
    ref, nrm, src, snr, _rng = _sheet_pair()
    T0 = np.eye(4)
    T0[2, 3] = 0.01                                                # every row 1 cm above its own point: every residual near 1e-2
    got = R.host_weighted_icp(src, ref, T0, 0.05, mode, nrm, snr, 'tukey', 1e-4)
    assert (got['iterations'], got['converged'], got['status'], got['fitness']) == (1, 1, SINGULAR, 1.0)
    assert np.array_equal(got['transform'], T0)
    free = R.host_weighted_icp(src, ref, T0, 0.05, mode, nrm, snr, 'tukey', 10.0)          # a width above them all: the step is taken
    assert free['status'] == 0 and not np.array_equal(free['transform'], T0)


@pytest.mark.parametrize('mode,count', [('generalized', 5), ('generalized', 6), ('point_to_plane', 5), ('point_to_point', 2)])
def test_too_few_counts_correspondences_not_weights(mode, count):
    ref, nrm, _src, _snr, _rng = _sheet_pair()
    src = np.concatenate([ref[:count] + 0.004, ref[:7] + np.array([0.0, 0.0, 5.0])], 0)
    snr = np.concatenate([nrm[:count], nrm[:7]], 0)
    got = R.host_weighted_icp(src, ref, np.eye(4), 0.02, mode, nrm, snr, 'huber', 0.01)
    assert got['fitness'] == count / len(src) and np.array_equal(got['correspondences'][:count], np.arange(count))
    if count in (2, 5):
        assert (got['iterations'], got['converged'], got['status']) == (1, 1, TOO_FEW)
        assert np.array_equal(got['transform'], np.eye(4))
    else:
        assert not got['status'] & TOO_FEW and not np.array_equal(got['transform'], np.eye(4))


@pytest.mark.parametrize('value', [np.nan, np.inf])
def test_a_non_finite_source_normal_refuses_the_pair(value):
    ref, nrm, src, snr, _rng = _sheet_pair()
    snr[7, 1] = value
    got = R.host_weighted_icp(src, ref, np.eye(4), 0.05, 'generalized', nrm, snr, 'huber', 0.01)
    assert got['status'] == NONFINITE and got['converged'] == 0 and got['iterations'] == 0
    assert np.isnan(got['transform']).all() and (got['correspondences'] == -1).all()
    for mode in OLD_MODES:                                         # the other estimators do not read the source normals
        assert R.host_weighted_icp(src, ref, np.eye(4), 0.05, mode, nrm, snr, 'huber', 0.01)['status'] == 0


def test_argument_validation_of_the_weighted_host_entry():
    ref, nrm, src, snr, _rng = _sheet_pair()
    call = lambda mode='generalized', **kw: R.host_weighted_icp(src, ref, np.eye(4), 0.05, mode, nrm, kw.pop('snr', snr), **kw)
    for kw in (dict(loss='huber', loss_k=0.0), dict(loss='huber', loss_k=-1.0), dict(loss='tukey', loss_k=np.nan), dict(loss='tukey', loss_k=np.inf),
               dict(epsilon=0.0), dict(epsilon=1.5), dict(epsilon=np.nan), dict(loss_id=5), dict(loss_id=-2)):
        with pytest.raises(RuntimeError, match='debug_icp_weighted_host: loss'):
            call(**kw)
    assert call(loss='l2', epsilon=1.0)['status'] == 0
    with pytest.raises(RuntimeError, match='generalized needs the source normals'):
        call(snr=None)
    with pytest.raises(RuntimeError, match='generalized needs the reference normals'):
        R.host_weighted_icp(src, ref, np.eye(4), 0.05, 'generalized', None, snr)
    with pytest.raises(RuntimeError, match='mode 3'):
        from se3et_amd._lib import check, lib
        z = np.zeros(16)
        check(lib().se3_debug_icp_weighted_host(src.ctypes.data, len(src), ref.ctypes.data, len(ref), 1, None, 1, None, 1, np.eye(4).ctypes.data,
                                                0.05, 3, 0, 1.0, 1e-3, 1e-6, 1e-6, 30, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data,
                                                z.ctypes.data, z.ctypes.data, None, None), 'se3_debug_icp_weighted_host')
    with pytest.raises(RuntimeError, match='debug_icp_host: .*mode 2'):          # the old entry goes on refusing the third mode
        from se3et_amd._lib import check, lib
        z = np.zeros(16)
        check(lib().se3_debug_icp_host(src.ctypes.data, len(src), ref.ctypes.data, len(ref), 1, nrm.ctypes.data, 1, np.eye(4).ctypes.data, 0.05, 2,
                                       1e-6, 1e-6, 30, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data,
                                       None, None), 'se3_debug_icp_host')


def test_wrappers_refuse_bad_losses_cpu_tensors_and_mismatched_normals():
    import torch
    from se3et_amd import icp
    a, eye = torch.zeros((4, 3)), np.eye(4)[None]
    for kw in (dict(loss='tukey', loss_k=0.0), dict(loss='huber', loss_k=float('nan')), dict(loss='huber'), dict(loss='huber', loss_k=-1.0)):
        with pytest.raises(ValueError, match='loss_k'):
            icp.icp_pairs([a], [a], eye, 0.1, **kw)
        with pytest.raises(ValueError, match='loss_k'):
            icp.generalized_icp_pairs([a], [a], eye, 0.1, **kw)
    with pytest.raises(ValueError, match="loss 'l1' is not one of"):
        icp.icp_pairs([a], [a], eye, 0.1, loss='l1', loss_k=1.0)
    with pytest.raises(ValueError, match='estimation'):                      # icp_pairs goes on refusing the third estimation
        icp.icp_pairs([a], [a], eye, 0.1, estimation='generalized', loss='l2')
    with pytest.raises(ValueError, match='epsilon'):
        icp.generalized_icp_pairs([a], [a], eye, 0.1, epsilon=0.0)
    with pytest.raises(ValueError, match='one normals array per source cloud'):
        icp.generalized_icp_pairs([a], [a], eye, 0.1, src_normals_list=[a, a])
    with pytest.raises(RuntimeError, match='generalized_icp_pairs: source cloud 0 must be a GPU tensor'):
        icp.generalized_icp_pairs([a], [a], eye, 0.1, [a], [a])
    with pytest.raises(RuntimeError, match='GPU tensor'):
        icp.registration_generalized_icp(np.zeros((4, 3)), np.zeros((4, 3)), device='cpu')
