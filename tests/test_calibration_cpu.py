"""CPU: the neighbour-limit calibration without a GPU -- the numpy twin's rules, the host rules and the whole host path
(se3et_amd.ext) against the reference's own results (tests/golden/calibration.npz, written by generate_calibration_golden.py), the host
count search against the twin on direct calls, and the argument checks of both C entry points.  Everything is an integer: every comparison
is whole-array equality."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import calibration_twin as twin
from calibration_fixture import CASES, OVER_64, dataset, direct_cases, expected


# ---- the twin's rules on hand-made histograms -------------------------------------------------------------------------------------------
def test_twin_stop_rule_is_strict():
    h = np.zeros((3, 2, 4), np.int64)
    h[:, 0, 1] = [1000, 1000, 1]
    h[:, 1, 2] = [5000, 5000, 5000]
    assert twin.calibrate(h, 0.8, 2000)[1] == 3            # stage 0 holds exactly 2000 after two pairs: not MORE than the threshold
    assert twin.calibrate(h, 0.8, 1999)[1] == 2
    assert twin.calibrate(h[:2], 0.8, 10 ** 9)[1] == 2     # never reached: every pair enters


def test_twin_limit_rule_is_strict_and_handles_the_edges():
    h = np.array([[0, 2, 2, 4, 2], [0, 0, 0, 0, 0]])
    assert twin.limits(h, 0.8) == [3, 0]                   # cumulative 0 2 4 8 10 against 8.0: 8 is not below; an empty stage gives 0
    assert twin.limits(h, 0.81) == [4, 0]
    assert twin.limits(h, 0.0) == [0, 0]
    assert twin.limits(h, 1.0) == [4, 0]                   # only the last bin reaches the total
    assert twin.limits(np.array([[5, 0, 0]]), 1.0) == [0]


def test_twin_drops_counts_at_and_above_hist_n():
    s = np.zeros((5, 3), np.float32)                       # five coincident points: every count is 5
    hist, dropped, mc = twin.count_hist(s, s, [5], [5], 1.0, 5, [0], 1)
    assert hist.sum() == 0 and dropped.tolist() == [5] and mc.tolist() == [5]
    hist, dropped, mc = twin.count_hist(s, s, [5], [5], 1.0, 6, [0], 1)
    assert hist[0].tolist() == [0, 0, 0, 0, 0, 5] and dropped.tolist() == [0]
    assert twin.calibrate(hist[None], 0.8, 2000) == ([5], 1)


# ---- the host rules on the reference's own histograms -------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_limits_from_the_reference_histograms(name):
    from se3et_amd.data import neighbor_limits_from_histograms
    params, kwargs, want_limits, want_pairs = CASES[name]
    limits, pairs_used, hist = expected(name)
    assert limits.tolist() == want_limits and pairs_used == want_pairs and hist.shape[0] == want_pairs
    threshold = kwargs.get('sample_threshold', 2000)
    fired = hist.sum(axis=(0, 2)).min() > threshold        # (kitti, demo and dense run out of items before every stage holds enough rows)
    full = np.concatenate([hist, hist[-1:]], 0) if fired else hist          # a pair behind the stopping one changes nothing
    got, used = neighbor_limits_from_histograms(full, sample_threshold=threshold)
    np.testing.assert_array_equal(got, limits)
    assert used == pairs_used and got.dtype == np.int64
    assert twin.calibrate(full, 0.8, threshold) == (want_limits, want_pairs)


def test_host_rules_match_the_twin_on_hand_made_histograms():
    from se3et_amd.data import neighbor_limits_from_histograms
    g = np.random.default_rng(5)
    for keep in (0.0, 0.5, 0.8, 1.0):
        for threshold in (0, 40, 41, 10 ** 6):
            h = g.integers(0, 9, (6, 3, 11))
            h[:, 2] = 0                                    # an empty stage: limit 0, and the stop rule never fires
            h[:, 1, :] = h[:, 1, :] * (g.random(11) < 0.5)
            got, used = neighbor_limits_from_histograms(h, keep, threshold)
            assert (got.tolist(), used) == twin.calibrate(h, keep, threshold)
            got, used = neighbor_limits_from_histograms(h[:, :2], keep, threshold)
            assert (got.tolist(), used) == twin.calibrate(h[:, :2], keep, threshold)


# ---- the whole host path against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_host_calibration_equals_the_reference(name):
    from se3et_amd import ext
    from se3et_amd.data import registration_collate_fn_stack_mode
    params, kwargs, _, _ = CASES[name]
    limits, pairs_used, hist = expected(name)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        got, details = ext.calibrate_neighbors_stack_mode(dataset(name), registration_collate_fn_stack_mode, **params, **kwargs, return_details=True)
    np.testing.assert_array_equal(got, limits)
    assert details['pairs_used'] == pairs_used
    np.testing.assert_array_equal(details['histograms'], hist)
    over = [w for w in caught if 'SE3_MAX_NEIGHBOR_LIMIT' in str(w.message)]
    assert len(over) == (1 if name in OVER_64 else 0)
    if name == 'dense':
        assert details['dropped'][0, 0] == 13312 and details['max_count'][0, 0] >= 180
    plain = ext.calibrate_neighbors_stack_mode(dataset(name)[:1], None, **params, pairs_per_call=1) if name == 'demo' else None
    if plain is not None:
        np.testing.assert_array_equal(plain, limits)       # (the plain call returns the limits alone, as the reference)


def test_host_calibration_does_not_depend_on_pairs_per_call():
    from se3et_amd import ext
    params, kwargs, _, _ = CASES['c1']
    limits, pairs_used, hist = expected('c1')
    for ppc in (1, 3, 16):
        got, details = ext.calibrate_neighbors_stack_mode(dataset('c1'), None, **params, pairs_per_call=ppc, return_details=True)
        np.testing.assert_array_equal(got, limits)
        assert details['pairs_used'] == pairs_used
        np.testing.assert_array_equal(details['histograms'], hist)


class _Counting(list):
    reads = 0

    def __getitem__(self, i):
        self.reads += 1
        return list.__getitem__(self, i)


def test_items_are_read_lazily():
    from se3et_amd import ext
    params = CASES['c2'][0]
    ds = _Counting(dataset('c2'))
    ext.calibrate_neighbors_stack_mode(ds, None, **params, pairs_per_call=2)
    assert ds.reads == 4                                   # the rule fires at pair 3: the second group of two is the last one read


# ---- the host count search against the twin ---------------------------------------------------------------------------------------------
def _host_call(c):
    from se3et_amd import ext
    t = lambda a, dt: torch.from_numpy(np.array(a)).to(dt).contiguous()
    start = {k: t(c[k], torch.int32).clone() for k in ('hist', 'dropped', 'max_count') if k in c}
    hist = start.get('hist', torch.zeros((c['num_slots'], c['hist_n']), dtype=torch.int32))
    out = ext.radius_count_hist(t(c['q'], torch.float32), t(c['s'], torch.float32), t(c['q_lengths'], torch.int64), t(c['s_lengths'], torch.int64),
                                c['radius'], c['hist_n'], c['slots'], hist=hist, dropped=start.get('dropped'), max_count=start.get('max_count'))
    return [o.numpy() for o in out]


def _twin_call(c):
    return twin.count_hist(c['q'], c['s'], c['q_lengths'], c['s_lengths'], c['radius'], c['hist_n'], c['slots'], c['num_slots'],
                           c.get('hist'), c.get('dropped'), c.get('max_count'))


@pytest.mark.parametrize('name', list(direct_cases()))
def test_host_count_search_equals_the_twin(name):
    c = direct_cases()[name]
    want = _twin_call(c)
    for got, w in zip(_host_call(c), want):
        np.testing.assert_array_equal(got, w)
    if name.startswith('dense_hist'):
        assert want[2].max() >= 48                         # the counts reach 48 ...
        assert (want[1].sum() > 0) == (c['hist_n'] < 4096)  # ... so the small histograms drop rows
    if name == 'dense_hist1':
        assert want[0].sum() == 0 and want[1].sum() == 3000
    if name == 'nan':
        assert want[0][0, 0] == 2                          # the two NaN rows: no count, bin 0
    if name == 'empty_support':
        assert want[0][0, 0] == 10


def test_host_count_search_threads_give_the_same(monkeypatch):
    c = direct_cases()['dense_hist16']
    one = _host_call(c)
    monkeypatch.setenv('SE3_HOST_THREADS', '5')
    for a, b in zip(one, _host_call(c)):
        np.testing.assert_array_equal(a, b)


# ---- argument validation of both symbols, without a GPU ------------------------------------------------------------------------------------
def _buffers():
    pts = np.zeros((8, 3), np.float32)
    ln = (ctypes.c_int64 * 33)(*([4, 4] + [0] * 31))
    slots = (ctypes.c_int * 33)()
    out = [np.zeros((4096 * 2,), np.int32), np.zeros((2,), np.int32), np.zeros((33,), np.int32)]
    return pts, ln, slots, out


@pytest.mark.parametrize('host', [False, True])
def test_argument_validation_without_gpu(host):
    from se3et_amd import _lib
    L = _lib.lib()
    pts, ln, slots, (hist, dropped, mc) = _buffers()
    p = pts.ctypes.data
    name = b'radius_count_hist_host' if host else b'radius_count_hist'

    def call(q=p, s=p, batch=2, hist_n=16, slot_table=slots, num_slots=2, h=hist.ctypes.data, d=dropped.ctypes.data, m=mc.ctypes.data, nq=8):
        if host:
            return L.se3_radius_count_hist_host(q, nq, s, 8, ln, ln, batch, 0.1, hist_n, slot_table, num_slots, h, d, m)
        return L.se3_radius_count_hist(q, nq, s, 8, ln, ln, batch, 0.1, None, hist_n, slot_table, num_slots, h, d, m, None)

    def refused(text, **kw):
        assert call(**kw) != 0
        err = L.se3_last_error()
        assert name in err and text in err, err

    refused(b'hist_n 0', hist_n=0)
    refused(b'hist_n 4097', hist_n=4097)
    refused(b'batch 33', batch=33)
    refused(b'batch 0', batch=0)
    for kw in (dict(q=None), dict(s=None), dict(h=None), dict(d=None), dict(m=None), dict(slot_table=None)):
        refused(b'null pointer', **kw)
    bad = (ctypes.c_int * 33)(0, 2)
    refused(b'slot 2 of cloud 1', slot_table=bad)
    bad = (ctypes.c_int * 33)(-1, 0)
    refused(b'slot -1 of cloud 0', slot_table=bad)
    refused(b'lengths', nq=9)
    assert hist.sum() == 0 and dropped.sum() == 0 and mc.sum() == 0        # nothing was written
    if host:
        assert call() == 0 and hist[:16].tolist() == [0, 0, 0, 0, 8] + [0] * 11 and mc[:2].tolist() == [4, 4]        # (both clouds in slot 0)


# ---- the Python front ends -------------------------------------------------------------------------------------------------------------------
def test_foreign_collate_is_refused():
    from se3et_amd import data, ext
    params = CASES['c1'][0]
    for mod in (data, ext):
        with pytest.raises(NotImplementedError, match='collate_fn'):
            mod.calibrate_neighbors_stack_mode(dataset('c1'), lambda *a, **k: None, **params)


def test_device_path_refuses_cpu_tensors():
    from se3et_amd import data, ops
    params = CASES['c1'][0]
    item = dataset('c1')[0]
    pts = torch.from_numpy(np.concatenate([item['ref_points'], item['src_points']]))
    ln = torch.tensor([len(item['ref_points']), len(item['src_points'])])
    with pytest.raises(RuntimeError, match='GPU'):
        ops.radius_count_hist(pts, pts, ln, ln, 0.1, 16, [0, 0])
    with pytest.raises(RuntimeError, match='GPU'):
        data.neighbor_histograms(pts, ln, params['num_stages'], params['voxel_size'], params['search_radius'])
    with pytest.raises(RuntimeError, match='GPU'):
        data.calibrate_neighbors_stack_mode([item], None, **params, device='cpu')


def test_hist_n_is_the_reference_bound():
    from se3et_amd.data import calibration_hist_n
    assert calibration_hist_n(0.025, 0.0625) == 180 and calibration_hist_n(0.3, 1.275) == 607


@pytest.mark.reference
def test_fixture_regenerates_from_the_reference():
    """Where the reference tree exists: its own calibrate_neighbors_stack_mode gives the fixture's numbers again (c1 and the dropped-bin case)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import generate_calibration_golden as G
    for name in ('c1', 'dense'):
        res = G.run_case(name)
        limits, pairs_used, hist = expected(name)
        np.testing.assert_array_equal(res[name + '/limits'], limits)
        np.testing.assert_array_equal(res[name + '/hist'], hist)
        assert int(res[name + '/pairs_used']) == pairs_used
