"""The cases of the keypoint selection tests: the table of tests/golden/keypoints.npz (generate_keypoints_golden.py), the edge clouds that
tests/test_keypoints_cpu.py and tests/test_gpu_keypoints.py share, and the call of the library's host entry."""
import ctypes

import numpy as np

# name, points, radius, keypoints asked: uniform random clouds in the unit cube; the radius is about the mean spacing, so that a quarter
# to a half of the points are suppressed
GOLDEN_CASES = (('small', 300, 0.09, 100), ('medium', 1200, 0.058, 300), ('large', 3000, 0.04, 500))
GOLDEN_FUNCTIONS = ('random_sample_keypoints', 'sample_keypoints_with_scores', 'random_sample_keypoints_with_scores',
                    'sample_keypoints_with_nms', 'random_sample_keypoints_with_nms')
GOLDEN_SEED = 1234          # np.random.seed before every call of a random form
FEAT_DIM = 2

TILE_SIZES = (1, 2, 255, 256, 257, 513)


def random_cloud(n, seed, dtype=np.float64):
    """n uniform points in the unit cube with distinct scores, and the radius that suppresses roughly a third of them."""
    g = np.random.default_rng(seed)
    points = g.uniform(0, 1, (n, 3)).astype(dtype)
    scores = g.permutation(n).astype(np.float64) / n + 0.01
    radius = 0.62 * (1.0 / max(n, 2)) ** (1.0 / 3.0)
    return points, scores, radius


def chain(n, radius, ascending):
    """n points on a line at spacing 0.9 r: every second one survives (from the far end when the scores ascend)."""
    points = np.zeros((n, 3))
    points[:, 0] = np.arange(n) * (0.9 * radius)
    scores = np.arange(n, dtype=np.float64) if ascending else np.arange(n, 0, -1, dtype=np.float64)
    return points, scores


def three_point(first_rank, radius=0.25):
    """A suppresses B, so C at 0.9 r from B survives; far-away fillers of higher and lower scores put A, B, C at ranks first_rank .. + 2."""
    n = first_rank + 3 + 5
    points = np.zeros((n, 3))
    points[:, 1] = 100.0 + np.arange(n) * (10.0 * radius)          # the fillers: a line far from A, B, C, 10 r apart
    scores = np.empty(n)
    scores[:first_rank] = 1000.0 + np.arange(first_rank, 0, -1)
    abc = np.arange(first_rank, first_rank + 3)
    points[abc] = [[0.0, 0.0, 0.0], [0.9 * radius, 0.0, 0.0], [1.8 * radius, 0.0, 0.0]]
    scores[abc] = [30.0, 20.0, 10.0]
    scores[first_rank + 3:] = [5.0, 4.0, 3.0, 2.0, 1.0]
    shuffle = np.random.default_rng(first_rank).permutation(n)      # (the ranks come from the scores, not from the input order)
    return points[shuffle], scores[shuffle], radius, shuffle


def edge_cases():
    """(id, points, scores, radius) of every edge cloud."""
    cases = []
    for n in TILE_SIZES:
        for dtype in (np.float32, np.float64):
            p, s, r = random_cloud(n, 100 + n, dtype)
            cases.append(('tile_%d_%s' % (n, np.dtype(dtype).name), p, s, r))
    for ascending in (False, True):
        p, s = chain(600, 0.25, ascending)
        cases.append(('chain_%s' % ('ascending' if ascending else 'descending'), p, s, 0.25))
    for first in (254, 255):
        p, s, r, _ = three_point(first)
        cases.append(('three_point_%d' % first, p, s, r))
    cases.append(('exactly_r', np.array([[0.0, 0, 0], [0.25, 0, 0]]), np.array([2.0, 1.0]), 0.25))
    cases.append(('one_ulp_inside', np.array([[0.0, 0, 0], [np.nextafter(0.25, 0.0), 0, 0]]), np.array([1.0, 2.0]), 0.25))
    g = np.random.default_rng(7)
    base = g.uniform(0, 1, (40, 3))
    cases.append(('duplicates', np.concatenate([base, base, base[:10]]), g.permutation(90).astype(np.float64), 0.05))
    p, _, r = random_cloud(300, 8)
    cases.append(('equal_scores', p, np.ones(300), r))
    cases.append(('few_score_levels', p, np.floor(g.uniform(0, 4, 300)), r))
    s = np.zeros(300)
    s[::2] = -0.0
    s[5], s[6] = 1.0, -1.0
    cases.append(('signed_zeros', p, s, r))
    s = g.permutation(300).astype(np.float64)
    s[3], s[4] = np.inf, -np.inf
    cases.append(('infinite_scores', p, s, r))
    wide = g.uniform(0, 1, (300, 3))                                   # 250 cells per axis at cell = r: the cells grow beyond the radius
    cases.append(('wide_grid', np.concatenate([wide, wide[:120] + 0.5 * 0.004 / np.sqrt(3.0)]), g.permutation(420).astype(np.float64), 0.004))
    cases.append(('one_ball', 5.0 + g.uniform(0, 0.1, (300, 3)), g.permutation(300).astype(np.float64), 0.25))
    cases.append(('empty', np.zeros((0, 3)), np.zeros((0,)), 0.1))
    return cases


def host_nms(points, order, radius, K=None):
    """se3_debug_keypoint_nms_host: (kept indices int64, status)."""
    from se3et_amd._lib import check, lib
    p = np.ascontiguousarray(points)
    assert p.dtype in (np.float32, np.float64)
    order = np.ascontiguousarray(order, dtype=np.int64)
    n = p.shape[0]
    out = np.full((max(n, 1),), -1, dtype=np.int64)
    count, status = ctypes.c_int64(-1), ctypes.c_int(-1)
    dummy = np.zeros(4)
    check(lib().se3_debug_keypoint_nms_host((p if n else dummy).ctypes.data, n, 1 if p.dtype == np.float64 else 0,
                                            (order if n else dummy).ctypes.data, float(radius), 0 if K is None else int(K), out.ctypes.data,
                                            ctypes.byref(count), ctypes.byref(status)), 'se3_debug_keypoint_nms_host')
    return out[:count.value].copy(), status.value
