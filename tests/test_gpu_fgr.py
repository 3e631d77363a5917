"""Fast Global Registration on the device (csrc/fgr.hip, se3et_amd/fgr.py) against se3_debug_fgr_host, the same text on host memory, BIT
FOR BIT.  Shapes are the smallest at which the kernels can go wrong: correspondence counts around the too-few limit (9, 10) and around the
lane width of the sums and the chunk of the tuple test (255, 256, 257; the clouds have as many rows, so the normalisation's sums meet the
same edges), and 700 for rows beyond one pass of the lanes; tuple caps inside a chunk, at its end and never reached."""
import numpy as np
import pytest
import torch

import fgr_fixture as F
from icp_fixture import sheet

pytestmark = pytest.mark.gpu

DEV = 'cuda'
KEYS = ('transforms', 'status', 'num_correspondences', 'num_tuples', 'mu')


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device(pairs, **options):
    """fgr_pairs over (src, ref, corr) numpy triples -> per pair the dict host_fgr returns."""
    from se3et_amd import fgr
    out = fgr.fgr_pairs([_gpu(p[0]) for p in pairs], [_gpu(p[1]) for p in pairs], [_gpu(p[2]) for p in pairs], evaluate=False,
                        return_tuples=True, **options)
    host = {k: out[k].cpu().numpy() for k in KEYS}
    return [{'transform': host['transforms'][p], 'status': int(host['status'][p]), 'num_correspondences': int(host['num_correspondences'][p]),
             'num_tuples': int(host['num_tuples'][p]), 'mu': float(host['mu'][p]), 'tuples': out['tuples'][p].cpu().numpy(),
             'trials': out['trials'][p].cpu().numpy()} for p in range(len(pairs))]


def _assert_same(got, want, what=''):
    for k in ('status', 'num_correspondences', 'num_tuples'):
        assert got[k] == want[k], '%s %s: %r, %r expected' % (what, k, got[k], want[k])
    assert np.array_equal(got['tuples'], want['tuples']) and np.array_equal(got['trials'], want['trials']), what
    assert np.array_equal(got['transform'], want['transform'], equal_nan=True), '%s: |dT| %.3e' % (
        what, np.nanmax(np.abs(got['transform'] - want['transform'])))
    assert got['mu'] == want['mu'], what


def _pair_of(K, dtype, seed=50):
    src, ref, corr, _gt = F.pair(seed=seed + K, n=max(K, 60), degrees=75.0, mismatch=0.3, noise=0.002)
    return src.astype(dtype), ref.astype(dtype), corr[:K]


@pytest.mark.parametrize('tuple_test', [True, False])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('K', [9, 10, 255, 256, 257, 700])
def test_device_equals_the_host_entry(K, dtype, tuple_test):
    pair = _pair_of(K, dtype)
    got = _device([pair], tuple_test=tuple_test)[0]
    want = F.host_fgr(*pair, tuple_test=tuple_test)
    _assert_same(got, want, 'K %d %s' % (K, dtype))
    assert want['status'] == (F.fgr_twin.TOO_FEW if K == 9 and not tuple_test else 0)


def test_mixed_input_types_equal_the_host_entry():
    src, ref, corr = _pair_of(257, 'float64')
    pair = (src.astype(np.float32), ref, corr)
    _assert_same(_device([pair])[0], F.host_fgr(*pair))


def test_a_refused_step_equals_the_host_entry():
    pair = F.thin_line()
    got = _device([pair], tuple_test=False)[0]
    _assert_same(got, F.host_fgr(*pair, tuple_test=False))
    assert got['status'] == F.fgr_twin.STEP_REFUSED and got['mu'] == 1.0 / 1.4


def _six():
    """ordinary, too few, empty, refused, the cap (100) reached in the first chunk, the cap never reached"""
    ordinary = _pair_of(300, 'float32')
    few = _pair_of(2, 'float32')
    empty = (ordinary[0][:0], ordinary[1], np.zeros((0, 2), np.int64))
    bad = tuple(a.copy() for a in _pair_of(120, 'float32'))
    bad[1][5, 0] = np.nan
    src, ref, corr, _gt = F.pair(seed=77, n=256, degrees=140.0)                          # exact matches: a trial passes unless it repeats a row
    first = (src.astype(np.float32), ref.astype(np.float32), corr)
    never = (src.astype(np.float32), (2.0 * ref).astype(np.float32), corr[:40])         # twice the size: no trial passes, all 4000 are run
    return [ordinary, few, empty, bad, first, never]


def test_six_unequal_pairs_equal_themselves_alone_and_a_second_run():
    pairs = _six()
    T = F.fgr_twin
    batch = _device(pairs, maximum_tuple_count=100)
    assert [b['status'] for b in batch] == [0, T.TOO_FEW, T.EMPTY, T.NONFINITE, 0, T.TOO_FEW]
    assert [b['num_tuples'] for b in batch] == [100, 0, 0, 0, 100, 0]
    assert batch[4]['trials'][-1] < F.CHUNK <= batch[0]['trials'][-1]                   # the cap inside the first chunk, and beyond it
    assert np.isnan(batch[3]['transform']).all() and all(np.isfinite(batch[p]['transform']).all() for p in (0, 1, 2, 4, 5))
    for p, pair in enumerate(pairs):
        _assert_same(batch[p], F.host_fgr(*pair, maximum_tuple_count=100), 'pair %d against the host' % p)
        _assert_same(_device([pair], maximum_tuple_count=100)[0], batch[p], 'pair %d alone' % p)
    for p, again in enumerate(_device(pairs[::-1], maximum_tuple_count=100)[::-1]):     # a second run, the batch in another order
        _assert_same(again, batch[p], 'pair %d in the second run' % p)


@pytest.mark.parametrize('at_chunk_end', [False, True])
def test_a_tuple_cap_inside_a_chunk_and_at_a_chunk_boundary(at_chunk_end):
    src, ref, corr, kept = F.capped_table(at_chunk_end)
    for cap in (5, 6):
        got = _device([(src, ref, corr)], maximum_tuple_count=cap)[0]
        _assert_same(got, F.host_fgr(src, ref, corr, maximum_tuple_count=cap), 'cap %d' % cap)
        assert np.array_equal(got['trials'], kept[:cap])
    assert (kept[5] >= F.CHUNK) == at_chunk_end


def test_more_pairs_than_one_launch_sequence_takes():
    from se3et_amd.stacking import PAIR_MAX_PAIRS
    pairs = [_pair_of(40, 'float32', seed=300 + p) for p in range(PAIR_MAX_PAIRS + 2)]
    got = _device(pairs, maximum_tuple_count=50)
    for p in (0, PAIR_MAX_PAIRS - 1, PAIR_MAX_PAIRS, PAIR_MAX_PAIRS + 1):
        _assert_same(got[p], F.host_fgr(*pairs[p], maximum_tuple_count=50), 'pair %d' % p)


def test_from_feats_is_mutual_matching_then_fgr_pairs():
    from se3et_amd import fgr
    from se3et_amd.feature_matching import extract_correspondences_from_feats_pairs
    rng = np.random.default_rng(9)
    src, ref, _corr, _gt = F.pair(seed=90, n=300, degrees=40.0)
    feats = rng.random((300, 33)).astype(np.float32)
    ref_feats = np.empty_like(feats)
    ref_feats[_corr[np.argsort(_corr[:, 0]), 1]] = feats + 0.01 * rng.random((300, 33)).astype(np.float32)      # at each row's true match
    src_f, ref_f = _gpu(feats), _gpu(ref_feats)
    s, q = _gpu(src.astype(np.float32)), _gpu(ref.astype(np.float32))
    out = fgr.fgr_from_feats_pairs([s], [q], [src_f], [ref_f], seed=3)
    ri, si = extract_correspondences_from_feats_pairs([ref_f], [src_f], mutual=True)
    table = torch.stack([si[0], ri[0]], 1)
    assert torch.equal(out['correspondences'][0], table) and table.shape[0] >= 10
    direct = fgr.fgr_pairs([s], [q], [table], seed=3)
    for k in KEYS + ('fitness', 'inlier_rmse'):
        assert torch.equal(out[k], direct[k]), k
    assert int(out['status'][0]) == 0


def _sheet_pairs():
    pairs = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        ref, _n = sheet(rng, 900)
        gt = F.rigid(rng, 20.0, 0.2)
        inv = np.linalg.inv(gt)
        pairs.append((_gpu((ref[rng.permutation(900)[:800]] @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)), _gpu(ref.astype(np.float32))))
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _equal(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    return a == b


def test_global_registration_with_the_fgr_coarse_step():
    from se3et_amd.fpfh import global_registration_pairs
    srcs, refs = _sheet_pairs()
    kw = dict(voxel_size=0.06, icp_distance=0.09, num_iterations=2000, seed=0)
    out = global_registration_pairs(srcs, refs, coarse='fgr', **kw)
    assert set(out) == {'transforms', 'coarse_transforms', 'ransac_transforms', 'src_points', 'ref_points', 'src_normals', 'ref_normals',
                        'src_feats', 'ref_feats', 'ransac', 'fgr', 'icp'}
    assert out['ransac'] is None and out['ransac_transforms'] is None and out['icp'] is not None
    assert tuple(out['transforms'].shape) == (2, 4, 4) and out['transforms'].dtype == torch.float64
    assert bool(torch.isfinite(out['transforms']).all()) and bool(torch.isfinite(out['coarse_transforms']).all())
    assert torch.equal(out['coarse_transforms'], out['fgr']['transforms'])
    assert set(out['fgr']) == {'transforms', 'status', 'num_correspondences', 'num_tuples', 'mu', 'fitness', 'inlier_rmse', 'correspondences'}
    default, explicit = global_registration_pairs(srcs, refs, **kw), global_registration_pairs(srcs, refs, coarse='ransac', **kw)
    assert default['fgr'] is None and _equal(default, explicit)
    assert torch.equal(default['coarse_transforms'], default['ransac_transforms'])
    assert torch.equal(default['ransac_transforms'], default['ransac']['transforms'].to(torch.float64))


def test_evaluation_is_icp_without_an_iteration():
    from se3et_amd import fgr
    from se3et_amd.icp import icp_pairs
    pairs = [_pair_of(300, 'float32'), _pair_of(257, 'float32')]
    srcs, refs, corrs = ([_gpu(p[k]) for p in pairs] for k in range(3))
    out = fgr.fgr_pairs(srcs, refs, corrs, maximum_correspondence_distance=0.05)
    ev = icp_pairs(srcs, refs, out['transforms'], 0.05, max_iteration=0)
    assert torch.equal(out['fitness'], ev['fitness']) and torch.equal(out['inlier_rmse'], ev['inlier_rmse'])
    assert float(out['fitness'].min()) > 0.5 and torch.equal(ev['transforms'], out['transforms'])
    bad = pairs[1][1].copy()
    bad[3, 2] = np.inf                                                                  # a refused pair is evaluated to 0, 0 and does not raise
    out = fgr.fgr_pairs(srcs, [refs[0], _gpu(bad)], corrs, maximum_correspondence_distance=0.05)
    assert out['status'].cpu().tolist() == [0, F.fgr_twin.NONFINITE] and bool(torch.isnan(out['transforms'][1]).all())
    assert out['fitness'].cpu().tolist() == [float(ev['fitness'][0]), 0.0] and float(out['inlier_rmse'][1]) == 0.0


def test_numpy_drop_ins_return_the_transform():
    from se3et_amd import fgr
    src, ref, corr, gt = F.pair(seed=12, n=200, degrees=100.0)
    T = fgr.registration_fgr_based_on_correspondence(src, ref, corr)
    assert T.shape == (4, 4) and T.dtype == np.float64 and F.transform_error(T, gt) < 1e-10
    assert np.array_equal(T, F.host_fgr(src, ref, corr)['transform'])
    feats = np.random.default_rng(1).random((200, 33)).astype(np.float32)
    ref_feats = np.empty_like(feats)
    own = corr[np.argsort(corr[:, 0]), 1]                                               # reference row of source row i
    ref_feats[own] = feats
    T = fgr.registration_fgr_based_on_feature_matching(src, ref, feats, ref_feats)
    assert F.transform_error(T, gt) < 1e-10
