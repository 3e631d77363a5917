"""Seeded inputs of the Fast Global Registration tests, the twin's run over them, and the call of se3_debug_fgr_host.

Families (case(name, dtype) returns the inputs ROUNDED to the dtype the library will read, so the twin sees the same values):
  boxes     400 points uniform in a box of extent (1, 0.7, 0.3), turned by 30 to 179 degrees about a random axis and shifted
  exact     every correspondence right, no noise: the transform is recovered to rounding
  half      half of the correspondences re-drawn at random, noise 0.002 on the reference: with and without the tuple test
  sheets    flat sheets of thickness 0.02: two of the three angles are weakly held at the start, which gives the loop's largest steps
The mismatch share stays at 0.5: at 0.8 and above the contract itself fails on some seeds."""
import ctypes
import functools

import numpy as np

import fgr_twin
from icp_fixture import rigid

DEFAULTS = dict(maximum_correspondence_distance=0.025, division_factor=1.4, use_absolute_scale=False, decrease_mu=True, iteration_number=64,
                tuple_scale=0.95, maximum_tuple_count=1000, tuple_test=True, seed=0)


def box(rng, n, extent=(1.0, 0.7, 0.3)):
    return rng.random((n, 3)) * np.asarray(extent)


def pair(seed, n=400, degrees=60.0, shift=0.5, mismatch=0.0, noise=0.0, extent=(1.0, 0.7, 0.3)):
    """src (n, 3), ref (n, 3) in another row order, corr (n, 2) and gt with ref ~ gt src.  `mismatch` of the correspondences point at a
    random reference row instead of their own."""
    rng = np.random.default_rng(seed)
    src = box(rng, n, extent)
    gt = rigid(rng, degrees, shift)
    order = rng.permutation(n)                                   # reference row order[i] is source row i
    ref = np.empty_like(src)
    ref[order] = src @ gt[:3, :3].T + gt[:3, 3] + noise * rng.normal(size=src.shape)
    corr = np.stack([np.arange(n), order], 1).astype(np.int64)
    wrong = rng.permutation(n)[:int(round(mismatch * n))]
    corr[wrong, 1] = rng.integers(0, n, len(wrong))
    return src, ref, corr[rng.permutation(n)], gt


# name -> (keyword arguments of pair, options that differ from DEFAULTS)
FAMILIES = {
    'exact30': (dict(seed=1, degrees=30.0), {}),
    'exact179': (dict(seed=2, degrees=179.0), {}),
    'exact120_plain': (dict(seed=3, degrees=120.0), dict(tuple_test=False)),
    'half90': (dict(seed=4, degrees=90.0, mismatch=0.5, noise=0.002), {}),
    'half150_plain': (dict(seed=5, degrees=150.0, mismatch=0.5, noise=0.002), dict(tuple_test=False)),
    'sheet170': (dict(seed=6, degrees=170.0, extent=(1.0, 0.7, 0.02)), {}),
    'sheet120_plain': (dict(seed=29, degrees=120.0, extent=(1.0, 0.7, 0.02)), dict(tuple_test=False)),      # a first step above 1 rad
    'sheet100_absolute': (dict(seed=7, degrees=100.0, extent=(1.0, 0.7, 0.02), noise=0.002), dict(use_absolute_scale=True)),
}


def options_of(**changed):
    assert set(changed) <= set(DEFAULTS)
    return dict(DEFAULTS, **changed)


def twin_fgr(src, ref, corr, **options):
    o = options_of(**options)
    o['tuple_test_on'] = o.pop('tuple_test')
    return fgr_twin.fgr(src, ref, corr, **o)


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """-> dict(src, ref, corr, gt, options, twin): arrays of `dtype` ('float32' / 'float64'; gt stays float64), read-only."""
    kw, changed = FAMILIES[name]
    src, ref, corr, gt = pair(**kw)
    src, ref = (np.ascontiguousarray(a.astype(dtype)) for a in (src, ref))
    options = options_of(**changed)
    twin = twin_fgr(src, ref, corr, **options)
    for a in (src, ref, corr, gt):
        a.setflags(write=False)
    return {'src': src, 'ref': ref, 'corr': corr, 'gt': gt, 'options': options, 'twin': twin}


CHUNK = 256                      # SE3_FGR_TUPLE_CHUNK: the trials of one step of the tuple test (tests/test_fgr_cpu.py holds it to the header)


@functools.lru_cache(maxsize=None)
def capped_table(cap_at_chunk_end):
    """-> src, ref, corr, kept: a pair whose trials are mostly rejected (0.7 of the matches wrong; only the tuple test is at stake), with
    the number of accepted trials in the first chunk 5 exactly (a cap of 5 then falls on the chunk's end) or at least 7 (it falls
    inside); kept: every accepted trial.  Seeds are searched in order, with the twin's tuple test."""
    for seed in range(200, 400):
        src, ref, corr, _gt = pair(seed=seed, n=80, degrees=50.0, mismatch=0.7)
        _tuples, kept = fgr_twin.tuple_test(src, ref, corr, 0.95, 10 ** 6, 0)
        first = int((kept < CHUNK).sum())
        if (first == 5) if cap_at_chunk_end else (first >= 7):
            return src, ref, corr, kept
    raise AssertionError('no seed with the wanted first chunk')


def thin_line(seed=4, n=12, width=1e-3):
    """-> src, ref, corr: n points within `width` of a line, matched to themselves in another order.  The turn about the line is held by
    the width alone, so the loop's second step comes out at several radians (14.9 with the defaults) and is refused."""
    rng = np.random.default_rng(seed)
    line = rng.normal(size=3)
    src = np.outer(rng.uniform(-1, 1, n), line / np.linalg.norm(line)) + width * rng.normal(size=(n, 3))
    return src, src[rng.permutation(n)], np.stack([np.arange(n), np.arange(n)], 1)


def transform_error(T, gt):
    return float(np.abs(np.asarray(T) - gt).max())


_dummy = (ctypes.c_double * 8)()


def host_fgr(src, ref, corr, **options):
    """se3_debug_fgr_host on numpy arrays (float32 or float64 each).  -> dict(transform (4, 4), status, num_correspondences, num_tuples,
    mu, tuples (|C'|, 2), trials (num_tuples,)); without the tuple test `tuples` is the table given, cut to |C'|."""
    from se3et_amd._lib import check, lib
    o = options_of(**options)
    src, ref = np.ascontiguousarray(src).reshape(-1, 3), np.ascontiguousarray(ref).reshape(-1, 3)
    assert src.dtype in (np.float32, np.float64) and ref.dtype in (np.float32, np.float64)
    corr = np.ascontiguousarray(corr, np.int64).reshape(-1, 2)
    cap = int(o['maximum_tuple_count'])
    T, status, ncorr, ntuples, mu = np.zeros((4, 4)), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_double()
    tuples, trials = np.full((3 * max(cap, 0) + 1, 2), -2, np.int64), np.full((max(cap, 0) + 1,), -2, np.int64)
    ptr = lambda a: a.ctypes.data if a.size else ctypes.addressof(_dummy)
    check(lib().se3_debug_fgr_host(ptr(src), len(src), int(src.dtype == np.float64), ptr(ref), len(ref), int(ref.dtype == np.float64), ptr(corr),
                                   len(corr), float(o['maximum_correspondence_distance']), float(o['division_factor']),
                                   int(o['use_absolute_scale']), int(o['decrease_mu']), int(o['iteration_number']), float(o['tuple_scale']), cap,
                                   int(o['tuple_test']), int(o['seed']), ptr(T), ctypes.byref(status), ctypes.byref(ncorr),
                                   ctypes.byref(ntuples), ctypes.byref(mu), ptr(tuples), ptr(trials)), 'se3_debug_fgr_host')
    n, k = ncorr.value, ntuples.value
    if o['tuple_test']:
        assert (tuples[n:] == -2).all() and (trials[k:] == -2).all(), 'rows beyond the counts were written'
        tuples, trials = tuples[:n], trials[:k]
    else:
        tuples, trials = corr[:n], trials[:0]
    return {'transform': T, 'status': status.value, 'num_correspondences': n, 'num_tuples': k, 'mu': mu.value, 'tuples': tuples,
            'trials': trials}


def probe_record():
    """What tools/fgr_probe.py recorded in profiles/fgr_probe.txt: dict(worst, bound, series, cases), cases[(name, dtype)] =
    dict(dT, twin_error, host_error, angle).  The bound is worked out here from `worst` by the rule the file states."""
    import math
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'fgr_probe.txt')).read()
    worst = float(re.search(r'fixture cases: largest (\S+);', text).group(1))
    cases = {}
    for name, dtype, dT, twin, host, angle in re.findall(
            r'^  case (\S+)\s+(float\d\d) .*\|dT\| (\S+)  twin error (\S+)  host error (\S+)  largest step angle (\S+)$', text, flags=re.M):
        cases[(name, dtype)] = dict(dT=float(dT), twin_error=float(twin), host_error=float(host), angle=float(angle))
    return {'worst': worst, 'bound': min(10.0 ** math.ceil(math.log10(16.0 * worst)), 1e-8),
            'series': float(re.search(r'of \(-4, 4\): (\S+);', text).group(1)), 'cases': cases}
