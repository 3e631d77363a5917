"""Fast Global Registration without a GPU: se3_debug_fgr_host (the text of csrc/fgr_core.h on host memory, run serially over the kernels'
lanes) against the independent float64 twin tests/fgr_twin.py on the seeded families of tests/fgr_fixture.py, and on known-answer,
degenerate and edge cases.

Bounds.  profiles/fgr_probe.txt (tools/fgr_probe.py, no GPU needed) records the largest deviation of the host entry from the twin over all
fixture cases: 2.83e-15.  TWIN_BOUND is 16 times that, for seeds and summation order, rounded up to a power of ten: 1e-13; it may not
exceed 1e-8 on these unit-scale clouds (sums of <= 3000 float64 terms through 64 well-conditioned 6x6 systems stay far below).  The file
also records the twin's own error per family, which the known-answer test of the half-wrong family allows five times, each family's largest
step angle, and the series' error."""
import math

import numpy as np
import pytest

import fgr_fixture as F
from fgr_twin import BAD_INDEX, EMPTY, NONFINITE, SINGULAR, STEP_REFUSED, TOO_FEW
from se3et_amd.ransac import sample_indices

RECORD = F.probe_record()
TWIN_BOUND = RECORD['bound']
assert TWIN_BOUND <= 1e-8
CHUNK = F.CHUNK


def _same_as_twin(src, ref, corr, **options):
    """The host entry and the twin on one input: C', the kept trials and the status equal, the transform and mu within the bound."""
    got, twin = F.host_fgr(src, ref, corr, **options), F.twin_fgr(src, ref, corr, **options)
    assert np.array_equal(got['tuples'], twin['tuples']) and got['num_correspondences'] == len(twin['tuples'])
    assert np.array_equal(got['trials'], twin['trials']) and got['num_tuples'] == len(twin['trials'])
    assert got['status'] == twin['status']
    if np.isnan(twin['transform']).any():
        assert np.isnan(got['transform']).all()
    else:
        dT = np.abs(got['transform'] - twin['transform']).max()
        print('|dT| %.2e, status %d, |C\'| %d' % (dT, got['status'], got['num_correspondences']))
        assert dT <= TWIN_BOUND
    assert abs(got['mu'] - twin['mu']) <= 1e-15 * max(1.0, abs(twin['mu']))
    return got, twin


def test_constants_are_the_headers():
    from se3et_amd import ops
    assert ops.FGR_STATUS == {'nonfinite': NONFINITE, 'too_few': TOO_FEW, 'singular': SINGULAR, 'empty': EMPTY, 'step_refused': STEP_REFUSED,
                              'bad_index': BAD_INDEX}
    assert {k: ops.FGR_STATUS[k] for k in ops.ICP_STATUS} == ops.ICP_STATUS          # the shared names carry ICP's values
    assert ops.FGR_TUPLE_CHUNK == CHUNK and ops.FGR_MAX_ANGLE == 4 and ops.FGR_MAX_ITERATION == 1000
    assert 100 * ops.FGR_MAX_CORRESPONDENCES < 2 ** 31 <= 100 * (ops.FGR_MAX_CORRESPONDENCES + 1)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('name', sorted(F.FAMILIES))
def test_host_entry_equals_the_twin(name, dtype):
    c = F.case(name, dtype)
    twin = c['twin']
    got = F.host_fgr(c['src'], c['ref'], c['corr'], **c['options'])
    assert np.array_equal(got['tuples'], twin['tuples']), 'the working lists differ'
    assert np.array_equal(got['trials'], twin['trials']), 'the kept trials differ'
    assert (got['status'], got['num_correspondences'], got['num_tuples']) == (twin['status'], len(twin['tuples']), len(twin['trials']))
    dT = np.abs(got['transform'] - twin['transform']).max()
    print('%s %s: |dT| %.2e, twin error %.2e, largest step angle %.4f' % (name, dtype, dT, F.transform_error(twin['transform'], c['gt']),
                                                                          twin['max_angle']))
    assert dT <= TWIN_BOUND
    assert got['mu'] == twin['mu']                                         # the same divisions in the same order


def test_fixture_families_cover_the_large_steps_and_the_tuple_test():
    angles = {name: F.case(name, 'float64')['twin']['max_angle'] for name in F.FAMILIES}
    assert max(angles.values()) > 1.0, 'no family takes a step above 1 rad, ICP\'s refusal'
    assert all(a < 4.0 for a in angles.values())
    assert all(abs(RECORD['cases'][(name, 'float64')]['angle'] - a) < 1e-3 for name, a in angles.items())       # the file is of these families
    half = F.case('half90', 'float64')
    right = lambda corr: np.mean(np.abs(half['ref'][corr[:, 1]] - (half['src'][corr[:, 0]] @ half['gt'][:3, :3].T + half['gt'][:3, 3])).max(1) < 0.02)
    assert right(half['corr']) < 0.55 and right(half['twin']['tuples']) > 0.95          # the tuple test lifts the share of right matches
    assert 5000 < half['twin']['trials'][-1] < 15000 and len(half['twin']['trials']) == 1000


@pytest.mark.parametrize('name', ['exact30', 'exact179', 'exact120_plain', 'sheet170', 'sheet120_plain'])
def test_exact_matches_recover_the_transform(name):
    c = F.case(name, 'float64')
    got = F.host_fgr(c['src'], c['ref'], c['corr'], **c['options'])
    assert got['status'] == 0 and F.transform_error(got['transform'], c['gt']) < 1e-10


@pytest.mark.parametrize('name', ['half90', 'half150_plain'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_half_wrong_matches_recover_it_within_five_times_the_twins_error(name, dtype):
    c = F.case(name, dtype)
    got = F.host_fgr(c['src'], c['ref'], c['corr'], **c['options'])
    recorded = RECORD['cases'][(name, dtype)]['twin_error']
    err = F.transform_error(got['transform'], c['gt'])
    print('%s %s: error %.2e, the twin\'s as recorded %.2e' % (name, dtype, err, recorded))
    assert got['status'] == 0 and 0 < recorded < 2e-3 and err <= 5 * recorded


def _exact(seed=40, n=60, **kw):
    src, ref, corr, gt = F.pair(seed=seed, n=n, degrees=70.0, **kw)
    return src, ref, corr, gt


@pytest.mark.parametrize('K,few', [(9, True), (10, False)])
def test_nine_correspondences_are_too_few_and_ten_are_not(K, few):
    src, ref, corr, gt = _exact()
    got, _twin = _same_as_twin(src, ref, corr[:K], tuple_test=False)
    if few:
        assert got['status'] == TOO_FEW and np.array_equal(got['transform'], np.eye(4)) and got['num_correspondences'] == 9
    else:
        assert got['status'] == 0 and F.transform_error(got['transform'], gt) < 1e-10
    got, _twin = _same_as_twin(src, ref, corr[:K])                           # with the tuple test: all 100 K trials, the cap is not reached
    draws = sample_indices(0, K, 100 * K, 3)
    distinct = (draws[:, 0] != draws[:, 1]) & (draws[:, 1] != draws[:, 2]) & (draws[:, 2] != draws[:, 0])
    assert got['num_tuples'] == distinct.sum() < 1000 and got['status'] == 0 and F.transform_error(got['transform'], gt) < 1e-10


@pytest.mark.parametrize('K', [1, 2])
def test_one_or_two_correspondences_run_their_trials_and_accept_none(K):
    src, ref, corr, _gt = _exact()
    got, _twin = _same_as_twin(src, ref, corr[:K])                           # every triple repeats a row: an edge of length 0
    assert (got['status'], got['num_tuples'], got['num_correspondences']) == (TOO_FEW, 0, 0)
    assert np.array_equal(got['transform'], np.eye(4))


def test_coincident_points_are_singular_without_the_tuple_test_and_too_few_with_it():
    src = np.tile([0.25, -0.5, 0.75], (40, 1))          # (coordinates whose sums are exact: the mean is the point, in any order)
    corr = np.stack([np.arange(40), np.arange(40)], 1)
    got, _twin = _same_as_twin(src, src.copy(), corr, tuple_test=False)
    assert got['status'] == SINGULAR and np.array_equal(got['transform'], np.eye(4))
    got, _twin = _same_as_twin(src, src.copy(), corr)
    assert got['status'] == TOO_FEW and got['num_tuples'] == 0 and np.array_equal(got['transform'], np.eye(4))


@pytest.mark.parametrize('where', ['src', 'ref'])
@pytest.mark.parametrize('value', [np.nan, np.inf])
def test_a_non_finite_point_refuses_the_pair(where, value):
    src, ref, corr, _gt = _exact()
    {'src': src, 'ref': ref}[where][7, 1] = value                            # (a row no correspondence need name: all rows are checked)
    got, _twin = _same_as_twin(src, ref, corr[corr[:, 0] != 7][:30])
    assert got['status'] == NONFINITE and np.isnan(got['transform']).all() and got['num_correspondences'] == 0


@pytest.mark.parametrize('bad', [(3, 60), (60, 3), (-1, 3), (3, -1)])
def test_an_index_out_of_range_refuses_the_pair(bad):
    src, ref, corr, _gt = _exact()
    corr = corr.copy()
    corr[17] = bad
    for on in (True, False):
        got, _twin = _same_as_twin(src, ref, corr, tuple_test=on)
        assert got['status'] == BAD_INDEX and np.isnan(got['transform']).all() and got['num_correspondences'] == 0


@pytest.mark.parametrize('which', ['src', 'ref', 'corr'])
def test_an_empty_cloud_or_table_gives_the_identity(which):
    src, ref, corr, _gt = _exact()
    if which == 'src':
        src = src[:0]
    elif which == 'ref':
        ref = ref[:0]
    else:
        corr = corr[:0]
    got, _twin = _same_as_twin(src, ref, corr)
    assert got['status'] == EMPTY and np.array_equal(got['transform'], np.eye(4)) and got['num_correspondences'] == 0


@pytest.mark.parametrize('at_chunk_end', [False, True])
def test_a_tuple_cap_of_five_inside_a_chunk_and_at_a_chunk_end(at_chunk_end):
    src, ref, corr, kept = F.capped_table(at_chunk_end)
    got, _twin = _same_as_twin(src, ref, corr, maximum_tuple_count=5)
    assert got['num_tuples'] == 5 and got['num_correspondences'] == 15 and np.array_equal(got['trials'], kept[:5])
    assert (kept[5] >= CHUNK) == at_chunk_end and kept[4] < CHUNK
    more, _twin = _same_as_twin(src, ref, corr, maximum_tuple_count=6)      # one more: the next chunk's first when at the end
    assert np.array_equal(more['trials'], kept[:6])


def test_a_tuple_test_that_accepts_nothing_runs_every_trial():
    src, ref, corr, _gt = _exact()
    got, twin = _same_as_twin(src, 2.0 * ref, corr)                          # every edge twice as long: lr tau2 < ls never holds
    assert (got['status'], got['num_tuples'], got['num_correspondences']) == (TOO_FEW, 0, 0) and len(twin['trials']) == 0


@pytest.mark.parametrize('options', [dict(use_absolute_scale=True), dict(decrease_mu=False), dict(use_absolute_scale=True, decrease_mu=False),
                                     dict(division_factor=2.0, maximum_correspondence_distance=0.1), dict(iteration_number=3),
                                     dict(tuple_scale=0.8, seed=7)])
def test_options_against_the_twin(options):
    src, ref, corr, gt = F.pair(seed=41, n=120, degrees=80.0, mismatch=0.3, noise=0.002)
    got, _twin = _same_as_twin(src, ref, corr, **options)
    assert got['status'] == 0
    if options.get('decrease_mu') is False and not options.get('use_absolute_scale'):
        assert got['mu'] == 1.0
    if 'iteration_number' not in options:
        assert F.transform_error(got['transform'], gt) < 0.05


def test_a_step_of_four_radians_and_more_is_refused_and_the_pair_keeps_what_it_has():
    """The twin's second step on the thin line is 14.9 rad.  The first step was taken (mu was divided once) through a system of condition
    about width^-2 = 1e6, which amplifies the rounding of its sums (1e-15) to 1e-9 at the most: the transforms agree within 1e-8."""
    src, ref, corr = F.thin_line()
    got, twin = F.host_fgr(src, ref, corr, tuple_test=False), F.twin_fgr(src, ref, corr, tuple_test=False)
    assert got['status'] == twin['status'] == STEP_REFUSED and twin['max_angle'] > 10.0
    assert got['mu'] == twin['mu'] == 1.0 / 1.4                               # refused at the second step, after one division
    dT = np.abs(got['transform'] - twin['transform']).max()
    print('|dT| %.2e' % dT)
    R = got['transform'][:3, :3]
    assert dT <= 1e-8 and np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and not np.array_equal(R, np.eye(3))


def test_no_iteration_aligns_the_means():
    src, ref, corr, _gt = _exact()
    got, _twin = _same_as_twin(src, ref, corr, iteration_number=0)
    assert got['status'] == 0 and np.array_equal(got['transform'][:3, :3], np.eye(3))
    assert np.abs(got['transform'][:3, 3] - (ref.mean(0) - src.mean(0))).max() < 1e-15


def test_the_reported_trials_are_sample_indices():
    src, ref, corr, _gt = _exact(n=50)
    got = F.host_fgr(src, ref, corr, maximum_tuple_count=5000, seed=123)
    draws = sample_indices(123, 50, 100 * 50, 3)
    distinct = (draws[:, 0] != draws[:, 1]) & (draws[:, 1] != draws[:, 2]) & (draws[:, 2] != draws[:, 0])
    assert np.array_equal(got['trials'], np.nonzero(distinct)[0])            # exact matches: a trial is rejected iff it repeats a row
    assert 0 < got['num_tuples'] < 5000 and np.array_equal(got['tuples'], corr[draws[got['trials']].reshape(-1)])


def test_the_updates_sine_and_cosine_on_the_open_interval():
    from se3et_amd._lib import check, lib
    x = np.random.default_rng(0).uniform(-4.0, 4.0, 20000)
    x[:6] = [0.0, 1e-300, -3.9999999999999996, 3.9999999999999996, math.pi, -math.pi / 2]
    s, c = np.zeros_like(x), np.zeros_like(x)
    check(lib().se3_debug_fgr_sincos_host(x.ctypes.data, len(x), s.ctypes.data, c.ctypes.data), 'se3_debug_fgr_sincos_host')
    err = max(np.abs(s - np.sin(x)).max(), np.abs(c - np.cos(x)).max())
    print('largest error %.2e, recorded %.2e' % (err, RECORD['series']))
    assert err <= 1e-14 and RECORD['series'] <= 1e-14
    for bad in (4.0, -4.0, np.nan):
        b = np.array([bad])
        assert lib().se3_debug_fgr_sincos_host(b.ctypes.data, 1, s.ctypes.data, c.ctypes.data) != 0


def test_argument_validation():
    src, ref, corr, _gt = _exact()
    for kw in (dict(maximum_correspondence_distance=0.0), dict(maximum_correspondence_distance=np.nan), dict(division_factor=0.5),
               dict(iteration_number=-1), dict(iteration_number=10 ** 6), dict(tuple_scale=0.0), dict(tuple_scale=1.5),
               dict(maximum_tuple_count=-1)):
        with pytest.raises(RuntimeError, match='debug_fgr_host'):
            F.host_fgr(src, ref, corr, **kw)


def test_batched_functions_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from se3et_amd import fgr
    from se3et_amd.fpfh import global_registration_pairs
    a, c = torch.zeros((4, 3)), torch.zeros((4, 2), dtype=torch.int64)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        fgr.fgr_pairs([a], [a], [c])
    with pytest.raises(ValueError, match='one source cloud'):
        fgr.fgr_pairs([a], [a], [])
    for kw, word in ((dict(maximum_correspondence_distance=-1.0), 'maximum_correspondence_distance'), (dict(division_factor=0.9), 'division_factor'),
                     (dict(iteration_number=1001), 'iteration_number'), (dict(tuple_scale=2.0), 'tuple_scale'),
                     (dict(maximum_tuple_count=-3), 'maximum_tuple_count')):
        with pytest.raises(ValueError, match=word):
            fgr.fgr_pairs([a], [a], [c], **kw)
    with pytest.raises(ValueError, match='coarse'):
        global_registration_pairs([a], [a], 0.05, coarse='teaser')
