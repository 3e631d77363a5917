"""Coloured ICP and the multi-scale schedule without a GPU: se3_debug_color_gradient_host and se3_debug_icp_colored_host (the text of
csrc/color_gradient.hip and csrc/icp_colored_core.h on host memory, in the kernels' summation order) against the independent float64
twin tests/colored_icp_twin.py on the families of tests/colored_icp_fixture.py, and known-answer, degenerate and refused cases."""
import numpy as np
import pytest

import colored_icp_fixture as X
import colored_icp_twin as C
import icp_fixture as F
from icp_robust_fixture import host_weighted_icp
from icp_twin import NONFINITE, SINGULAR, TOO_FEW

# profiles/colored_icp_probe.txt records the largest deviations of the host entries from the twin (tools/colored_icp_probe.py, no GPU
# needed).  Each bound is 16 times its figure, rounded up to a power of ten -- the margin covers seeds and the summation order -- and may
# not exceed 1e-8 on these unit-scale clouds.
TWIN_BOUND = 1e-14            # transform and rmse over the 32 fixture cases: 3.89e-16
GRADIENT_BOUND = 1e-10        # gradients over the families' reference clouds and the edge clouds: 2.85e-12 (the (m - 1)^2 n n^T term next
                              # to projections of a few centimetres gives G a condition number near 1e5)
KNOWN_BOUND = 1e-11           # the known plane's gradient: 2.26e-13
assert max(TWIN_BOUND, GRADIENT_BOUND, KNOWN_BOUND) <= 1e-8
DTYPES = ['float32', 'float64']


def test_the_coloured_mode_has_its_own_enum_and_the_mode_tables_are_unchanged():
    from se3et_amd import _lib, ops
    assert _lib.ENUMS['se3_icp_colored_option'] == {'SE3_ICP_COLORED': X.COLORED} and ops.ICP_COLORED == X.COLORED
    assert ops.ICP_MODES == {'point_to_point': 0, 'point_to_plane': 1}
    assert ops.ICP_WEIGHTED_MODES == {'point_to_point': 0, 'point_to_plane': 1, 'generalized': 2}
    assert 'SE3_ICP_COLORED' not in _lib.ENUMS['se3_icp_option'] and 'SE3_ICP_COLORED' not in _lib.CONSTANTS


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', sorted(X.FAMILIES))
def test_host_gradients_equal_the_twin_on_the_families(name, dtype):
    c = X.gradient_case(name, dtype)
    g, status = X.host_gradients(c['ref'], c['normals'], c['ref_colors'], c['gradient_radius'])
    dg = np.abs(g - c['twin_gradients']).max()
    print('%s %s: |dg| %.2e, largest |g| %.2f' % (name, dtype, dg, np.abs(g).max()))
    assert status == 0 and dg <= GRADIENT_BOUND
    assert np.abs(g).max() > 0.5                                       # (the texture is there)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', X.CLOUD_SIZES + ('duplicates', 'sparse'))
def test_host_gradients_equal_the_twin_on_the_edge_clouds(kind, dtype):
    p, nr, col, radius = X.small_cloud(kind, dtype)
    g, status = X.host_gradients(p, nr, col, radius)
    want, m, _margins = C.gradients(p, nr, col, radius)
    assert status == 0
    few = m < 4
    assert (g[few] == 0.0).all(), 'a row with m < 4 has the zero gradient, exactly'
    assert np.abs(g - want).max() <= GRADIENT_BOUND
    if kind == 3:
        assert few.all()
    elif kind == 'sparse':
        assert few.sum() >= 1 and (~few).sum() >= 1 and np.abs(g[~few]).max() > 0.1
    else:
        assert not few.any() and np.abs(g).max() > 0.1
    if kind == 'duplicates':                                           # a duplicate is a neighbour: rows 0 .. 4 and their copies agree
        assert np.abs(g[5:10] - g[0:5]).max() <= GRADIENT_BOUND


def test_the_gradient_of_a_linear_intensity_on_a_plane_is_known():
    p, nr, col, radius, known = X.known_plane()
    g, status = X.host_gradients(p, nr, col, radius)
    _want, m, _margins = C.gradients(p, nr, col, radius)
    assert status == 0 and (m >= 4).sum() >= 150
    dg = np.abs(g[m >= 4] - known).max()
    print('known plane: |g - g_known| %.2e' % dg)
    assert dg <= KNOWN_BOUND
    assert abs(known @ nr[0]) < 1e-15


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('loss', X.LOSSES)
@pytest.mark.parametrize('name', sorted(X.FAMILIES))
def test_coloured_host_entry_equals_the_twin(name, loss, dtype):
    c = X.case(name, loss, dtype)
    twin = c['twin']
    got, _g = X.host_case(c, loss, trace=True)
    evals = twin['evaluations']
    for k, ev in enumerate(evals):
        assert np.array_equal(got['trace'][k], ev['corr']), 'evaluation %d: the correspondence sets differ' % k
    assert (got['trace'][len(evals):] == -2).all(), 'the library made more evaluations than the twin'
    assert np.array_equal(got['correspondences'], evals[-1]['corr'])
    assert (got['iterations'], got['converged'], got['status']) == (twin['iterations'], twin['converged'], twin['status'])
    n_corr, n = twin['fitness_ratio']
    assert got['fitness'] == n_corr / n
    dT, drmse = np.abs(got['transform'] - twin['transform']).max(), abs(got['rmse'] - twin['rmse'])
    print('%s %s %s: %d iterations, |dT| %.2e, |drmse| %.2e' % (name, loss, dtype, got['iterations'], dT, drmse))
    assert got['iterations'] >= 2 and dT <= TWIN_BOUND and drmse <= TWIN_BOUND


@pytest.mark.parametrize('loss', [None, 'huber'])
@pytest.mark.parametrize('name', ['sheet700', 'partial1500'])
def test_lambda_one_agrees_with_point_to_plane(name, loss):
    c = X.gradient_case(name, 'float64')
    k = 1.0 if loss is None else X.LOSS_K[loss]
    plane = host_weighted_icp(c['src'], c['ref'], c['T0'], c['r'], 'point_to_plane', c['normals'], None, loss, k)
    got = X.host_colored_icp(c['src'], c['ref'], c['T0'], c['r'], c['normals'], c['src_colors'], c['ref_colors'], c['twin_gradients'], 1.0, loss, k)
    assert (got['iterations'], got['converged'], got['status'], got['fitness']) == (plane['iterations'], plane['converged'], plane['status'],
                                                                                   plane['fitness'])
    assert plane['iterations'] >= 3 and np.array_equal(got['correspondences'], plane['correspondences'])
    assert np.abs(got['transform'] - plane['transform']).max() <= TWIN_BOUND and abs(got['rmse'] - plane['rmse']) <= TWIN_BOUND


def test_lambda_zero_with_zero_gradients_is_singular_with_the_identity_update():
    c = X.inputs('sheet700', 'float64')
    got = X.host_colored_icp(c['src'], c['ref'], c['T0'], c['r'], c['normals'], c['src_colors'], c['ref_colors'], np.zeros_like(c['ref']), 0.0)
    assert (got['iterations'], got['converged'], got['status']) == (1, 1, SINGULAR)
    assert np.array_equal(got['transform'], c['T0'])


def test_colour_registers_the_flat_sheet_that_point_to_plane_cannot():
    """Conditions, checked on the twin first: point-to-plane ends singular or with more than half of the initial in-plane error; coloured
    ICP ends with less than a tenth of it."""
    c = X.case('flat', None, 'float64')
    start = X.in_plane_error(c['T0'], c)
    assert start > 0.04
    assert X.in_plane_error(c['twin']['transform'], c) < 0.1 * start, 'the twin itself misses the condition (another texture or offset)'
    plane = host_weighted_icp(c['src'], c['ref'], c['T0'], c['r'], 'point_to_plane', c['normals'], None, None)
    assert plane['status'] & SINGULAR or X.in_plane_error(plane['transform'], c) > 0.5 * start
    got, _g = X.host_case(c, None)
    print('flat: in-plane %.2e at T0, %.2e after point-to-plane (status %d), %.2e after coloured ICP'
          % (start, X.in_plane_error(plane['transform'], c), plane['status'], X.in_plane_error(got['transform'], c)))
    assert got['status'] == 0 and got['converged'] == 1 and X.in_plane_error(got['transform'], c) < 0.1 * start


def _sheet_pair(seed=5, nref=300, nsrc=200):
    rng = np.random.default_rng(seed)
    ref, nrm = F.sheet(rng, nref)
    rows = rng.permutation(nref)[:nsrc]
    src = ref[rows] + 0.001 * rng.normal(size=(nsrc, 3))
    rcol, scol = X.texture(ref[:, 0], ref[:, 1]), X.texture(src[:, 0], src[:, 1])
    g, status = X.host_gradients(ref, nrm, rcol, 0.15)
    assert status == 0
    return ref, nrm, src, scol, rcol, g


@pytest.mark.parametrize('value', [np.nan, np.inf])
@pytest.mark.parametrize('which', ['src_colors', 'ref_colors', 'gradients', 'normals'])
def test_a_non_finite_colour_or_gradient_refuses_the_pair(which, value):
    ref, nrm, src, scol, rcol, g = _sheet_pair()
    arrays = {'normals': nrm.copy(), 'src_colors': scol.copy(), 'ref_colors': rcol.copy(), 'gradients': g.copy()}
    good = X.host_colored_icp(src, ref, np.eye(4), 0.05, **arrays)
    assert good['status'] == 0 and good['iterations'] >= 1
    arrays[which][7, 1] = value
    got = X.host_colored_icp(src, ref, np.eye(4), 0.05, **arrays)
    assert got['status'] == NONFINITE and got['converged'] == 0 and got['iterations'] == 0
    assert np.isnan(got['transform']).all() and (got['correspondences'] == -1).all()
    if which == 'ref_colors':                                          # the gradient entry refuses the cloud and computes nothing
        out, status = X.host_gradients(ref, nrm, arrays['ref_colors'], 0.15)
        assert status == 1 and (out == -7.0).all()


@pytest.mark.parametrize('count', [5, 6])
def test_too_few_counts_correspondences(count):
    ref, nrm, _src, _scol, rcol, g = _sheet_pair()
    src = np.concatenate([ref[:count] + 0.004, ref[:7] + np.array([0.0, 0.0, 5.0])], 0)
    scol = np.concatenate([rcol[:count], rcol[:7]], 0)
    got = X.host_colored_icp(src, ref, np.eye(4), 0.02, nrm, scol, rcol, g, loss='huber', loss_k=0.01)
    assert got['fitness'] == count / len(src) and np.array_equal(got['correspondences'][:count], np.arange(count))
    if count == 5:
        assert (got['iterations'], got['converged'], got['status']) == (1, 1, TOO_FEW)
        assert np.array_equal(got['transform'], np.eye(4))
    else:
        assert not got['status'] & TOO_FEW and not np.array_equal(got['transform'], np.eye(4))


def test_tukey_below_every_residual_is_singular_with_the_identity_update():
    ref, nrm, src, scol, rcol, g = _sheet_pair()
    T0 = np.eye(4)
    T0[2, 3] = 0.01                                                    # every row 1 cm above its own point; the colours 0.05 off as well
    got = X.host_colored_icp(src, ref, T0, 0.05, nrm, scol + 0.05, rcol, g, loss='tukey', loss_k=1e-4)
    assert (got['iterations'], got['converged'], got['status'], got['fitness']) == (1, 1, SINGULAR, 1.0)
    assert np.array_equal(got['transform'], T0)
    free = X.host_colored_icp(src, ref, T0, 0.05, nrm, scol + 0.05, rcol, g, loss='tukey', loss_k=10.0)
    assert free['status'] == 0 and not np.array_equal(free['transform'], T0)


def test_argument_validation_of_the_host_entries():
    ref, nrm, src, scol, rcol, g = _sheet_pair()
    call = lambda **kw: X.host_colored_icp(src, ref, np.eye(4), 0.05, kw.pop('nrm', nrm), scol, rcol, kw.pop('g', g), **kw)
    for lam in (-0.01, 1.01, np.nan, np.inf):
        with pytest.raises(RuntimeError, match='debug_icp_colored_host: lambda_geometric'):
            call(lambda_geometric=lam)
    assert call(lambda_geometric=0.0)['status'] == 0 and call(lambda_geometric=1.0)['status'] == 0
    for kw in (dict(loss='huber', loss_k=0.0), dict(loss='tukey', loss_k=np.nan), dict(loss_id=5), dict(loss_id=-2)):
        with pytest.raises(RuntimeError, match='debug_icp_colored_host: loss'):
            call(**kw)
    with pytest.raises(RuntimeError, match='coloured ICP needs the reference normals'):
        call(nrm=None)
    with pytest.raises(RuntimeError, match='coloured ICP needs the reference normals'):
        call(g=None)
    with pytest.raises(RuntimeError, match='debug_icp_colored_host: distance'):
        call(max_iteration=1001)
    for k in (0, 65):
        with pytest.raises(RuntimeError, match='debug_color_gradient_host: k %d not in' % k):
            X.host_gradients(ref, nrm, rcol, 0.1, k)
    for radius in (-1.0, np.nan, np.inf):
        with pytest.raises(RuntimeError, match='debug_color_gradient_host: radius'):
            X.host_gradients(ref, nrm, rcol, radius)
    empty = np.zeros((0, 3))
    out, status = X.host_gradients(empty, empty, empty, 0.1)
    assert out.shape == (0, 3) and status == 0
    zero, status = X.host_gradients(ref, nrm, rcol, 0.0)               # a radius of 0 has no member: every gradient is zero
    assert status == 0 and (zero == 0.0).all()


def test_wrappers_refuse_bad_arguments_before_they_ask_for_a_device():
    import torch
    from se3et_amd import icp, ops
    a, eye = torch.zeros((4, 3)), np.eye(4)[None]
    for lam in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='lambda_geometric'):
            icp.colored_icp_pairs([a], [a], eye, 0.1, [a], [a], lambda_geometric=lam)
    with pytest.raises(ValueError, match='source colours 0: 3 rows for a cloud of 4'):
        icp.colored_icp_pairs([a], [a], eye, 0.1, [a[:3]], [a])
    with pytest.raises(ValueError, match='reference colours 0: 5 rows for a cloud of 4'):
        icp.colored_icp_pairs([a], [a], eye, 0.1, [a], [torch.zeros((5, 3))])
    with pytest.raises(ValueError, match='one colours array per source cloud'):
        icp.colored_icp_pairs([a], [a], eye, 0.1, [a, a], [a])
    with pytest.raises(ValueError, match='one source and one reference cloud per pair'):
        icp.colored_icp_pairs([a, a], [a], eye, 0.1, [a, a], [a])
    with pytest.raises(ValueError, match='max_nn 65'):
        icp.colored_icp_pairs([a], [a], eye, 0.1, [a], [a], gradient_max_nn=ops.KNN_MAX + 1)
    with pytest.raises(ValueError, match='max_nn 65'):
        icp.color_gradient_clouds([a], [a], [a], 0.1, max_nn=ops.KNN_MAX + 1)
    with pytest.raises(ValueError, match='gradient radius'):
        icp.color_gradient_clouds([a], [a], [a], -1.0)
    with pytest.raises(ValueError, match='loss_k'):
        icp.colored_icp_pairs([a], [a], eye, 0.1, [a], [a], loss='huber')
    with pytest.raises(RuntimeError, match='colored_icp_pairs: source cloud 0 must be a GPU tensor'):
        icp.colored_icp_pairs([a], [a], eye, 0.1, [a], [a])
    with pytest.raises(RuntimeError, match='color_gradient_clouds: cloud 0 must be a GPU tensor'):
        icp.color_gradient_clouds([a], [a], [a], 0.1)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        icp.registration_colored_icp(np.zeros((4, 3)), np.zeros((4, 3)), np.zeros((4, 3)), np.zeros((4, 3)), device='cpu')
    with pytest.raises(ValueError, match="estimation 'colored' is not one of"):          # icp_pairs goes on refusing the estimation
        icp.icp_pairs([a], [a], eye, 0.1, estimation='colored')


def test_the_schedule_refuses_bad_lists_before_it_asks_for_a_device():
    import torch
    from se3et_amd import icp
    a, eye = torch.zeros((4, 3)), np.eye(4)[None]
    run = lambda v, d, it, **kw: icp.multiscale_icp_pairs([a], [a], eye, v, d, it, **kw)
    for v, d, it in (([0.1, 0.05], [0.2], [30, 30]), ([0.1], [0.2, 0.1], [30]), ([], [], [])):
        with pytest.raises(ValueError, match='must have one length, at least 1'):
            run(v, d, it)
    with pytest.raises(ValueError, match='allowed only as the last entry'):
        run([None, 0.05], [0.2, 0.1], [30, 30])
    for v in ([0.05, 0.1], [0.1, 0.1], [0.1, -0.05], [0.1, float('nan')]):
        with pytest.raises(ValueError, match='strictly decreasing'):
            run(v, [0.2, 0.1], [30, 30])
    with pytest.raises(ValueError, match="estimation 'plane' is not one of"):
        run([0.1], [0.2], [30], estimation='plane')
    with pytest.raises(ValueError, match='one colours array per source cloud'):
        run([0.1], [0.2], [30], estimation='colored')
    with pytest.raises(ValueError, match='reference colours 0: 3 rows for a cloud of 4'):
        run([0.1], [0.2], [30], estimation='colored', src_colors_list=[a], ref_colors_list=[a[:3]])
    with pytest.raises(RuntimeError, match='multiscale_icp_pairs: source cloud 0 must be a GPU tensor'):
        run([0.1, 0.05, None], [0.2, 0.1, 0.05], [30, 20, 10])
    with pytest.raises(RuntimeError, match='GPU tensor'):
        icp.registration_multiscale_icp(np.zeros((4, 3)), np.zeros((4, 3)), [None], [0.1], [5], device='cpu')
