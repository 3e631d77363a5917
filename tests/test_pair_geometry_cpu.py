"""CPU: the pair ground truth (se3et_amd/pair_geometry.py, csrc/pair_geometry.hip, csrc/pair_grid.h) without a GPU.

  - the numpy twin (tests/pair_geometry_twin.py) against the reference's own results in tests/golden/pair_geometry.npz, at the demands of
    tests/pair_geometry_fixture.py (indices, overlaps, correspondence lists equal; distances and covariances within derived rounding bounds);
  - the library's search core on host memory (se3_debug_pair_nearest_neighbor_host, se3_debug_pair_ball_host: the text the kernels run)
    against the twin, exactly, on the fixture cases and the edge cases;
  - argument validation of every new entry, the gt.info round trip, the refusal of CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

import pair_geometry_fixture as F
import pair_geometry_twin as twin

CASES = list(twin.CASES)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_nearest(q, s, T, dtype=np.float64):
    from se3et_amd import _lib
    q, s = np.ascontiguousarray(q, dtype).reshape(-1, 3), np.ascontiguousarray(s, dtype).reshape(-1, 3)
    T = np.ascontiguousarray(T, np.float64)
    dist, idx = np.empty(len(q), np.float64), np.empty(len(q), np.int64)
    _lib.check(_lib.lib().se3_debug_pair_nearest_neighbor_host(_ptr(q), len(q), _ptr(s), len(s), int(dtype == np.float64), _ptr(T), _ptr(dist),
                                                               _ptr(idx)), 'se3_debug_pair_nearest_neighbor_host')
    return dist, idx


def host_ball(q, s, T, radius, dtype=np.float64):
    from se3et_amd import _lib
    q, s = np.ascontiguousarray(q, dtype).reshape(-1, 3), np.ascontiguousarray(s, dtype).reshape(-1, 3)
    T = np.ascontiguousarray(T, np.float64)
    counts, total = np.empty(len(q), np.int64), np.zeros(1, np.int64)
    elem = int(dtype == np.float64)
    _lib.check(_lib.lib().se3_debug_pair_ball_host(_ptr(q), len(q), _ptr(s), len(s), elem, _ptr(T), radius, _ptr(counts), None, 0, _ptr(total)),
               'se3_debug_pair_ball_host')
    assert counts.sum() == total[0]
    out = np.full((int(total[0]), 2), -7, np.int64)
    again = np.empty(len(q), np.int64)
    _lib.check(_lib.lib().se3_debug_pair_ball_host(_ptr(q), len(q), _ptr(s), len(s), elem, _ptr(T), radius, _ptr(again), _ptr(out), len(out),
                                                   _ptr(total)), 'se3_debug_pair_ball_host')
    assert np.array_equal(again, counts) and total[0] == len(out)
    return counts, out


@pytest.mark.parametrize('name', CASES)
def test_twin_matches_the_reference(name):
    g = F.golden()
    ref, src, T = F.inputs(name)
    T = T.astype(np.float64)
    dist, idx, corr = F.twin_scan(name)
    F.check_nearest(name, dist, idx)
    F.check_overlaps(name, np.array([twin.overlap_from_distances(dist, r) for r in g[name + '/overlap_radii']]))
    F.check_correspondences(name, corr)
    for k, v in enumerate(g[name + '/voxel_sizes']):
        ov, cov, absolute, n = twin.calibrate_ground_truth(ref, src, T, float(v), seed=int(g[name + '/seeds'][k]), nn=(dist, idx))
        assert n == min(int(g[name + '/info_selected'][k]), 5000)
        F.check_info(name, k, ov, cov, absolute)


def test_fixture_runs_the_draw_path():
    g = F.golden()
    assert int(g['demo/info_selected'][1]) == 5357 and int(g['c3_20k/info_selected'][0]) == 12251
    assert int(g['demo/corr_total']) == 110302 and int(g['cap_30k/corr_total']) == 33450


@pytest.mark.parametrize('name', CASES)
def test_host_search_core_matches_the_twin_on_the_fixture_cases(name):
    ref, src, T = F.inputs(name)
    tdist, tidx, tcorr = F.twin_scan(name)
    for dtype in (np.float32, np.float64):
        dist, idx = host_nearest(ref, src, T, dtype)
        assert np.array_equal(idx, tidx) and np.array_equal(dist, tdist)
        counts, corr = host_ball(ref, src, T, twin.CASES[name][0], dtype)
        assert np.array_equal(corr, tcorr)
        assert np.array_equal(counts, np.bincount(tcorr[:, 0], minlength=len(ref)))
    F.check_nearest(name, dist, idx)
    F.check_correspondences(name, corr)


@pytest.mark.parametrize('name', list(F.edge_cases()))
def test_host_search_core_edge_cases(name):
    case = F.edge_cases()[name]
    q, s, T, r = case
    dist, idx = host_nearest(q, s, T)
    _counts, corr = host_ball(q, s, T, r)
    F.check_edge(name, case, dist, idx, corr)


def test_host_ball_at_many_radii_and_cell_sizes():
    """The walk's block of cells against brute force from radii far below the cell size to radii beyond the whole cloud."""
    ref, src, T = F.inputs('c1_2k')
    q = ref[::7]
    for r in (1e-4, 0.013, 0.21, 0.9, 5.0):
        _, corr = host_ball(q, src, T, r)
        assert np.array_equal(corr, twin.get_correspondences(q, src, T.astype(np.float64), r)), r


def test_host_ball_does_not_write_past_the_capacity():
    from se3et_amd import _lib
    ref, src, T = F.inputs('c1_2k')
    q, s, T = np.ascontiguousarray(ref[:300], np.float64), np.ascontiguousarray(src, np.float64), np.ascontiguousarray(T, np.float64)
    counts, total = np.empty(len(q), np.int64), np.zeros(1, np.int64)
    out = np.full((12, 2), -7, np.int64)
    assert _lib.lib().se3_debug_pair_ball_host(_ptr(q), len(q), _ptr(s), len(s), 1, _ptr(T), 0.05, _ptr(counts), _ptr(out), 10, _ptr(total)) == 0
    assert total[0] == counts.sum() > 10 and np.all(out[10:] == -7)


def test_argument_validation_without_gpu():
    from se3et_amd import _lib
    L = _lib.lib()
    pts = np.zeros((4, 3), np.float64)
    off, bad_off = (ctypes.c_int64 * 2)(0, 4), (ctypes.c_int64 * 2)(0, -4)
    T = np.eye(4)[None].copy()
    nanT = T.copy()
    nanT[0, 1, 3] = np.nan
    ws_bytes = L.se3_pair_grid_workspace_bytes(4, 1)
    assert ws_bytes > 0 and L.se3_pair_grid_workspace_bytes(-1, 1) == 0 and L.se3_pair_grid_workspace_bytes(4, 33) == 0
    fake = ctypes.c_void_p(256)          # a non-null "device" pointer: every call below must be refused before any launch
    p, out = _ptr(pts), _ptr(np.zeros(64))

    def refused(status, word):
        assert status != 0 and word in L.se3_last_error(), L.se3_last_error()

    refused(L.se3_pair_grid_build(None, 1, off, 1, _ptr(T), 0.0, fake, ws_bytes, None), b'null')
    refused(L.se3_pair_grid_build(fake, 1, bad_off, 1, _ptr(T), 0.0, fake, ws_bytes, None), b'offsets')
    refused(L.se3_pair_grid_build(fake, 1, off, -1, _ptr(T), 0.0, fake, ws_bytes, None), b'pairs')
    refused(L.se3_pair_grid_build(fake, 2, off, 1, _ptr(T), 0.0, fake, ws_bytes, None), b'elem')
    refused(L.se3_pair_grid_build(fake, 1, off, 1, _ptr(nanT), 0.0, fake, ws_bytes, None), b'non-finite transform')
    refused(L.se3_pair_grid_build(fake, 1, off, 1, _ptr(T), float('nan'), fake, ws_bytes, None), b'cell size')
    refused(L.se3_pair_grid_build(fake, 1, off, 1, _ptr(T), 0.0, fake, ws_bytes - 1, None), b'too small')
    refused(L.se3_pair_nearest_neighbor_stack(fake, ws_bytes, 4, fake, 1, off, 1, None, fake, None), b'null')
    refused(L.se3_pair_nearest_neighbor_stack(fake, ws_bytes - 1, 4, fake, 1, off, 1, fake, fake, None), b'too small')
    refused(L.se3_pair_nearest_neighbor_stack(fake, ws_bytes, 4, fake, 1, bad_off, 1, fake, fake, None), b'offsets')
    refused(L.se3_pair_ball_count_stack(fake, ws_bytes, 4, fake, 1, off, 1, float('inf'), fake, None), b'radius')
    refused(L.se3_pair_ball_count_stack(fake, ws_bytes, 4, fake, 1, off, 1, -1.0, fake, None), b'radius')
    refused(L.se3_pair_ball_count_stack(fake, ws_bytes, 4, fake, 1, off, 40, 0.1, fake, None), b'pairs')
    refused(L.se3_pair_ball_count_stack(fake, ws_bytes, 4, None, 1, off, 1, 0.1, fake, None), b'null')
    refused(L.se3_pair_ball_fill_stack(fake, ws_bytes, 4, fake, 1, off, 1, 0.1, fake, -1, fake, None), b'total')
    refused(L.se3_pair_ball_fill_stack(fake, ws_bytes, 4, fake, 1, off, 1, float('nan'), fake, 1, fake, None), b'radius')
    refused(L.se3_pair_ball_fill_stack(fake, ws_bytes, 4, fake, 1, off, 1, 0.1, fake, 1, None, None), b'null')
    refused(L.se3_pair_ball_fill_stack(fake, 16, 4, fake, 1, off, 1, 0.1, fake, 1, fake, None), b'too small')
    refused(L.se3_pair_overlap_stack(None, off, 1, 0.1, fake, None), b'null')
    refused(L.se3_pair_overlap_stack(fake, off, 1, float('nan'), fake, None), b'radius')
    refused(L.se3_pair_overlap_stack(fake, bad_off, 1, 0.1, fake, None), b'offsets')
    refused(L.se3_pair_info_covariance_stack(fake, 1, off, _ptr(T), None, off, 1, fake, None), b'null')
    refused(L.se3_pair_info_covariance_stack(fake, 1, off, _ptr(nanT), fake, off, 1, fake, None), b'non-finite transform')
    refused(L.se3_pair_info_covariance_stack(fake, 1, off, _ptr(T), fake, bad_off, 1, fake, None), b'offsets')
    refused(L.se3_pair_info_covariance_stack(fake, 1, off, _ptr(T), fake, off, -2, fake, None), b'pairs')
    refused(L.se3_debug_pair_nearest_neighbor_host(p, 4, p, 4, 1, None, out, out), b'null')
    refused(L.se3_debug_pair_nearest_neighbor_host(p, -1, p, 4, 1, _ptr(T), out, out), b'nq')
    refused(L.se3_debug_pair_nearest_neighbor_host(p, 4, p, 4, 1, _ptr(nanT), out, out), b'non-finite transform')
    refused(L.se3_debug_pair_ball_host(p, 4, p, 4, 1, _ptr(T), float('nan'), out, None, 0, out), b'radius')
    refused(L.se3_debug_pair_ball_host(p, 4, p, -4, 1, _ptr(T), 0.1, out, None, 0, out), b'ns')
    refused(L.se3_debug_pair_ball_host(p, 4, p, 4, 1, _ptr(T), 0.1, None, None, 0, out), b'null')
    # zero pairs are a valid, empty call
    zero = (ctypes.c_int64 * 1)(0)
    assert L.se3_pair_overlap_stack(fake, zero, 0, 0.1, fake, None) == 0
    assert L.se3_pair_grid_build(fake, 1, zero, 0, _ptr(T), 0.0, fake, L.se3_pair_grid_workspace_bytes(0, 0), None) == 0


def test_info_file_round_trip(tmp_path):
    from se3et_amd.benchmark import read_info_file
    from se3et_amd.pair_geometry import write_info_file
    g = F.golden()
    records = [dict(test_pair=[0, 1], num_fragments=60, covariance=g['demo/info_cov'][1]),
               dict(test_pair=[3, 17], num_fragments=60, covariance=torch.from_numpy(g['c3_20k/info_cov'][0])),
               dict(test_pair=[5, 6], num_fragments=37, covariance=np.zeros((6, 6)))]
    path = str(tmp_path / 'scene' / 'gt.info')
    write_info_file(path, records)
    back = read_info_file(path)
    assert len(back) == 3
    for rec, got in zip(records, back):
        assert got['test_pair'] == rec['test_pair'] and got['num_fragments'] == rec['num_fragments']
        assert got['covariance'].shape == (6, 6)
        assert np.array_equal(got['covariance'], np.asarray(rec['covariance'], np.float64).astype(np.float32))
    # a record read from a file is written back unchanged
    again = str(tmp_path / 'again.info')
    write_info_file(again, back)
    for a, b in zip(back, read_info_file(again)):
        assert a['test_pair'] == b['test_pair'] and a['num_fragments'] == b['num_fragments'] and np.array_equal(a['covariance'], b['covariance'])
    assert len(open(path).read().splitlines()) == 21


def test_product_refuses_cpu_tensors():
    from se3et_amd import pair_geometry as PG
    a, b, T = torch.zeros(8, 3), torch.ones(9, 3), torch.eye(4, dtype=torch.float64)[None]
    with pytest.raises(RuntimeError, match='GPU tensor'):
        PG.nearest_neighbor_pairs([a], [b])
    with pytest.raises(RuntimeError, match='GPU tensor'):
        PG.compute_overlap_pairs([a], [b], T, 0.1)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        PG.get_correspondences_pairs([a], [b], T, 0.1)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        PG.calibrate_ground_truth_pairs([a], [b], T)
    with pytest.raises(RuntimeError):
        PG.nearest_neighbor_pairs([a.numpy()], [b.numpy()])
