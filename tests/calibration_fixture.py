"""The cases of tests/golden/calibration.npz: the datasets the reference's calibrate_neighbors_stack_mode was run over, rebuilt from
seeds (tests/golden/generate_calibration_golden.py writes the fixture, the calibration tests read it)."""
import os

import numpy as np

from se3et_amd.synthetic import box_surface, make_pair

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURE = os.path.join(GOLDEN, 'calibration.npz')

MATCH = dict(num_stages=4, voxel_size=0.025, search_radius=0.0625)           # the 3DMatch configurations: hist_n 180
KITTI = dict(num_stages=5, voxel_size=0.3, search_radius=1.275)              # the KITTI configuration: hist_n 607

# name -> (parameters, extra keyword arguments, the limits and the number of pairs the reference used)
CASES = {
    'c2': (MATCH, {}, [10, 22, 39, 41], 3),
    'c2_all': (MATCH, {'sample_threshold': 10 ** 9}, [10, 22, 39, 41], 8),
    'c1': (MATCH, {}, [7, 16, 34, 41], 5),
    'kitti': (KITTI, {}, [17, 45, 111, 137, 74], 4),                         # (never reaches 2000 rows at stage 4)
    'demo': (MATCH, {}, [36, 34, 35, 36], 1),
    'cap': (MATCH, {}, [4, 9, 22, 13], 1),                                   # (coarsest stage capped at 2 x 2000)
    'dense': (MATCH, {}, [173, 46, 48, 48], 1),                              # (a third of the stage-0 rows has 180 or more neighbours)
}
OVER_64 = ('kitti', 'dense')


def _item(ref, src):
    ref, src = np.ascontiguousarray(ref, np.float32), np.ascontiguousarray(src, np.float32)
    return dict(ref_points=ref, src_points=src, ref_feats=np.ones((len(ref), 1), np.float32), src_feats=np.ones((len(src), 1), np.float32),
                transform=np.eye(4, dtype=np.float32))


def dataset(name):
    """The list of item dicts of one case."""
    if name in ('c2', 'c2_all'):
        return [_item(*make_pair('c2_5k', i)[:2]) for i in range(8)]
    if name == 'c1':
        return [_item(*make_pair('c1_2k', i)[:2]) for i in range(8)]
    if name == 'kitti':
        return [_item(*make_pair('c3_4k', i)[:2]) for i in range(4)]
    if name == 'cap':
        return [_item(*make_pair('cap_30k', i)[:2]) for i in range(2)]
    if name == 'demo':
        d = np.load(os.path.join(GOLDEN, 'demo_se3ete.npz'))
        return [_item(d['ref'], d['src'])]
    if name == 'dense':
        return [_item(box_surface(20000, (0.6, 0.5, 0.4), 101, 0.005), box_surface(20000, (0.6, 0.5, 0.4), 102, 0.005))]
    raise KeyError(name)


def expected(name):
    """(limits, pairs_used, per-pair histograms (pairs_used, stages, hist_n)) as the reference produced them."""
    d = np.load(FIXTURE)
    return d[name + '/limits'], int(d[name + '/pairs_used']), d[name + '/hist']


def direct_cases():
    """Direct calls of the count search that the pyramid never produces: name -> dict(q, s, q_lengths, s_lengths, radius, hist_n, slots,
    num_slots, and for the accumulation case the starting hist / dropped / max_count)."""
    g = np.random.default_rng(2024)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    cases = {}
    cases['q_ne_s'] = dict(q=f32(g.random((300 + 200, 3))), s=f32(g.random((700 + 500, 3))), q_lengths=[300, 200], s_lengths=[700, 500], radius=0.2,
                           hist_n=64, slots=[0, 1], num_slots=2)
    dense = f32(g.random((3000, 3)) * 0.5)                  # 24 000 points per unit volume: ~51 within 0.08 of an interior point
    for n in (1, 16, 4096):
        cases['dense_hist%d' % n] = dict(q=dense, s=dense, q_lengths=[1800, 1200], s_lengths=[1800, 1200], radius=0.1, hist_n=n, slots=[0, 1],
                                         num_slots=2)
    pts = f32(g.random((60, 3)))
    cases['empty_cloud'] = dict(q=pts[:50], s=pts[:50], q_lengths=[0, 50], s_lengths=[0, 50], radius=0.3, hist_n=32, slots=[0, 1], num_slots=2)
    cases['empty_support'] = dict(q=pts, s=pts[:50], q_lengths=[10, 50], s_lengths=[0, 50], radius=0.3, hist_n=32, slots=[0, 1], num_slots=2)
    cases['one_point'] = dict(q=pts[:2], s=pts[:2], q_lengths=[1, 1], s_lengths=[1, 1], radius=0.05, hist_n=8, slots=[0, 1], num_slots=2)
    dup = f32(np.concatenate([pts[:20]] * 3 + [pts[20:]]))
    cases['duplicates'] = dict(q=dup, s=dup, q_lengths=[len(dup)], s_lengths=[len(dup)], radius=0.25, hist_n=64, slots=[0], num_slots=1)
    nan = f32(g.random((400, 3)) * 0.6)
    nan[17, 0] = np.nan
    nan[250, 2] = np.nan
    cases['nan'] = dict(q=nan, s=nan, q_lengths=[200, 200], s_lengths=[200, 200], radius=0.2, hist_n=128, slots=[0, 0], num_slots=1)
    many = f32(g.random((4 * 250, 3)))
    cases['shared_prefilled'] = dict(q=many, s=many, q_lengths=[250] * 4, s_lengths=[250] * 4, radius=0.15, hist_n=24, slots=[2, 0, 2, 2], num_slots=3,
                                     hist=g.integers(0, 1000, (3, 24)).astype(np.int32), dropped=g.integers(0, 50, (3,)).astype(np.int32),
                                     max_count=np.array([0, 1000, 3, 0], np.int32))
    return cases
