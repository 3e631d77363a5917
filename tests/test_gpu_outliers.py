"""Outlier removal on the device (se3et_amd/scan_prep.py, csrc/outliers.hip) against the library's host entries -- the same text on host
memory, which tests/test_outlier_cpu.py pins to the numpy twin -- bit for bit: the row values a_i, the three statistics, both masks, for
float32 and float64 inputs.  The clouds of tests/outlier_fixture.py have R - 1, R and R + 1 rows for R = 4 and R = 256."""
import numpy as np
import pytest
import torch

import outlier_fixture as F

pytestmark = pytest.mark.gpu

CLOUDS = F.clouds()
DTYPES = (np.float64, np.float32)
DEV = 'cuda'


def _gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _same(got, want):
    return np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(want))


@pytest.mark.parametrize('dtype', DTYPES, ids=['float64', 'float32'])
@pytest.mark.parametrize('name', list(CLOUDS))
def test_device_equals_the_host_entries(name, dtype):
    from se3et_amd import ops
    from se3et_amd.scan_prep import remove_radius_outlier_clouds, remove_statistical_outlier_clouds
    from se3et_amd.stacking import identities
    p, nb, ratio, nb_points, r = CLOUDS[name]
    p = p.astype(dtype)
    want, want_r = F.host_statistical(p, nb, ratio), F.host_radius(p, nb_points, r)
    t = _gpu(p)
    kept, stats = remove_statistical_outlier_clouds([t], nb, ratio, return_stats=True)
    assert kept[0].dtype == torch.int64 and kept[0].is_cuda and tuple(stats.shape) == (1, 3) and stats.dtype == torch.float64
    assert np.array_equal(kept[0].cpu().numpy(), np.flatnonzero(want['keep']))
    assert _same(stats[0].cpu().numpy(), want['stats'][:3])
    a = ops.knn_distance_stack(ops.pair_grid_build(t, [len(p)], identities(1), 0.0), t, [len(p)], nb, -1)
    assert np.array_equal(a.cpu().numpy(), want['a'])
    assert np.array_equal(remove_radius_outlier_clouds([t], nb_points, r)[0].cpu().numpy(), np.flatnonzero(want_r['keep']))


def test_batch_of_33_equals_the_single_calls():
    from se3et_amd.scan_prep import remove_radius_outlier_clouds, remove_statistical_outlier_clouds
    g = np.random.default_rng(4)
    clouds = [v[0] for n, v in CLOUDS.items() if n != 'scan']
    while len(clouds) < 33:
        clouds.append(g.uniform(0, 0.6, (20 + 7 * len(clouds), 3)))
    clouds = [p.astype(np.float32 if i % 2 else np.float64) for i, p in enumerate(clouds)]
    pts = [_gpu(p) for p in clouds]
    first, second = remove_statistical_outlier_clouds(pts, 20, 1.5, True), remove_statistical_outlier_clouds(pts, 20, 1.5, True)
    radius = remove_radius_outlier_clouds(pts, 3, 0.1)
    assert len(first[0]) == 33 and tuple(first[1].shape) == (33, 3)
    assert _same(first[1].cpu().numpy(), second[1].cpu().numpy())
    for i, p in enumerate(clouds):
        alone = remove_statistical_outlier_clouds([pts[i]], 20, 1.5, True)
        assert torch.equal(first[0][i], second[0][i]) and torch.equal(first[0][i], alone[0][0]), i
        assert _same(first[1][i].cpu().numpy(), alone[1][0].cpu().numpy()), i
        want = F.host_statistical(p, 20, 1.5)
        assert np.array_equal(first[0][i].cpu().numpy(), np.flatnonzero(want['keep'])) and _same(first[1][i].cpu().numpy(), want['stats'][:3]), i
        assert np.array_equal(radius[i].cpu().numpy(), np.flatnonzero(F.host_radius(p, 3, 0.1)['keep'])), i
    assert remove_statistical_outlier_clouds([]) == [] and remove_radius_outlier_clouds([], 3, 0.1) == []


def test_numpy_wrappers():
    from se3et_amd.scan_prep import remove_radius_outlier, remove_statistical_outlier
    p, nb, ratio, nb_points, r = CLOUDS['stray']
    pts, idx = remove_statistical_outlier(p, nb, ratio)
    assert idx.tolist() == list(range(60)) and np.array_equal(pts, p[:60])
    pts, idx = remove_radius_outlier(p, nb_points, r)
    assert np.array_equal(idx, np.flatnonzero(F.host_radius(p, nb_points, r)['keep'])) and np.array_equal(pts, p[idx])


def test_refusals():
    from se3et_amd.scan_prep import remove_radius_outlier_clouds, remove_statistical_outlier_clouds
    good = _gpu(CLOUDS['n257'][0])
    q = CLOUDS['n257'][0].copy()
    q[9, 2] = np.nan
    with pytest.raises(ValueError, match='cloud 1: a point is not finite'):
        remove_statistical_outlier_clouds([good, _gpu(q), good])
    with pytest.raises(ValueError, match='cloud 33: a point is not finite'):
        remove_radius_outlier_clouds([good[:5]] * 33 + [_gpu(q)], 3, 0.1)
    with pytest.raises(ValueError, match='nb_neighbors'):
        remove_statistical_outlier_clouds([good], 65)
    with pytest.raises(ValueError, match='std_ratio'):
        remove_statistical_outlier_clouds([good], 20, 0.0)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        remove_statistical_outlier_clouds([torch.from_numpy(CLOUDS['n257'][0])])
