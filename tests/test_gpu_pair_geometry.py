"""GPU: the pair ground truth (se3et_amd/pair_geometry.py, csrc/pair_geometry.hip) against the reference's own results in
tests/golden/pair_geometry.npz, at the demands of tests/pair_geometry_fixture.py; float32 against float64 inputs; a pair alone against the
same pair in a stacked call; run against run; the edge cases and a 16-pair batch against the numpy twin; the numpy wrappers."""
import numpy as np
import pytest
import torch

import pair_geometry_fixture as F
import pair_geometry_twin as twin

pytestmark = pytest.mark.gpu
CASES = list(twin.CASES)


def dev(a, dtype=None):
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).cuda()


def case_tensors(name, dtype=np.float32):
    ref, src, T = F.inputs(name)
    return dev(ref, dtype), dev(src, dtype), T.astype(np.float64)


def run_case(PG, name, dtype=np.float32, seed_k=None):
    """Every function on one pair: dist, idx, overlaps, corr, and per voxel size (overlap, covariance)."""
    g = F.golden()
    ref, src, T = case_tensors(name, dtype)
    d, i = PG.nearest_neighbor_pairs([ref], [src], [T], return_index=True)
    ov = torch.stack([PG.compute_overlap_pairs([ref], [src], [T], float(r))[0] for r in g[name + '/overlap_radii']])
    corr = PG.get_correspondences_pairs([ref], [src], [T], twin.CASES[name][0])[0]
    info = []
    for k, v in enumerate(g[name + '/voxel_sizes']):
        np.random.seed(int(g[name + '/seeds'][k]))
        o, c = PG.calibrate_ground_truth_pairs([ref], [src], [T], float(v))
        info.append((o[0], c[0]))
    return d[0], i[0], ov, corr, info


@pytest.mark.parametrize('name', CASES)
def test_every_function_matches_the_reference(name):
    from se3et_amd import pair_geometry as PG
    g = F.golden()
    ref, src, T = F.inputs(name)
    d, i, ov, corr, info = run_case(PG, name)
    assert d.is_cuda and corr.is_cuda and ov.dtype == torch.float64
    F.check_nearest(name, d.cpu().numpy(), i.cpu().numpy())
    F.check_overlaps(name, ov.cpu().numpy())
    F.check_correspondences(name, corr.cpu().numpy())
    tdist, tidx, _ = F.twin_scan(name)
    for k, v in enumerate(g[name + '/voxel_sizes']):
        _, _, absolute, n = twin.calibrate_ground_truth(ref, src, T.astype(np.float64), float(v), seed=int(g[name + '/seeds'][k]), nn=(tdist, tidx))
        F.check_info(name, k, info[k][0].cpu().numpy(), info[k][1].cpu().numpy(), absolute)


@pytest.mark.parametrize('name', CASES)
def test_matches_the_twin_exactly(name):
    """Same arithmetic, same tie rule: distances and correspondence lists bit for bit."""
    from se3et_amd import pair_geometry as PG
    ref, src, T = case_tensors(name)
    tdist, tidx, tcorr = F.twin_scan(name)
    d, i = PG.nearest_neighbor_pairs([ref], [src], [T], return_index=True)
    assert np.array_equal(d[0].cpu().numpy(), tdist) and np.array_equal(i[0].cpu().numpy(), tidx)
    assert np.array_equal(PG.get_correspondences_pairs([ref], [src], [T], twin.CASES[name][0])[0].cpu().numpy(), tcorr)


@pytest.mark.parametrize('name', ['demo', 'c3_20k'])
def test_float32_and_float64_inputs_agree(name):
    from se3et_amd import pair_geometry as PG
    a, b = run_case(PG, name, np.float32), run_case(PG, name, np.float64)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    for (oa, ca), (ob, cb) in zip(a[4], b[4]):
        assert torch.equal(oa, ob) and torch.equal(ca, cb)
    # one cloud of each type in the same pair
    ref32, src32, T = case_tensors(name, np.float32)
    ref64, src64, _ = case_tensors(name, np.float64)
    d, i = PG.nearest_neighbor_pairs([ref32], [src64], [T], return_index=True)
    assert torch.equal(d[0], a[0]) and torch.equal(i[0], a[1])
    assert torch.equal(PG.get_correspondences_pairs([ref64], [src32], [T], twin.CASES[name][0])[0], a[3])


def test_alone_and_stacked_are_bit_identical_and_runs_repeat():
    from se3et_amd import pair_geometry as PG
    g = F.golden()
    tensors = [case_tensors(n) for n in CASES]
    refs, srcs, Ts = [t[0] for t in tensors], [t[1] for t in tensors], [t[2] for t in tensors]
    alone = [run_case(PG, n) for n in CASES]
    for attempt in range(2):
        d, i = PG.nearest_neighbor_pairs(refs, srcs, Ts, return_index=True)
        # a radius and a voxel size of its own per case would need one call each: the stacked calls use the demo pair's
        ov = PG.compute_overlap_pairs(refs, srcs, Ts, 0.0375)
        corr = PG.get_correspondences_pairs(refs, srcs, Ts, 0.05)
        np.random.seed(int(g['demo/seeds'][0]))
        io, ic = PG.calibrate_ground_truth_pairs(refs, srcs, Ts, 0.006)
        assert ov.shape == (5,) and ic.shape == (5, 6, 6) and len(corr) == 5
        for p, n in enumerate(CASES):
            assert torch.equal(d[p], alone[p][0]) and torch.equal(i[p], alone[p][1]), n
            if n != 'c3_20k':
                assert torch.equal(ov[p], alone[p][2][0]) and torch.equal(corr[p], alone[p][3]), n
                assert torch.equal(io[p], alone[p][4][0][0]) and torch.equal(ic[p], alone[p][4][0][1]), n
    # c3_20k at its own radii, between two other pairs
    order = ['c1_2k', 'c3_20k', 'c2_5k']
    pick = [CASES.index(n) for n in order]
    corr = PG.get_correspondences_pairs([refs[p] for p in pick], [srcs[p] for p in pick], [Ts[p] for p in pick], 0.6)
    ov = PG.compute_overlap_pairs([refs[p] for p in pick], [srcs[p] for p in pick], [Ts[p] for p in pick], 0.45)
    k = CASES.index('c3_20k')
    assert torch.equal(corr[1], alone[k][3]) and torch.equal(ov[1], alone[k][2][0])
    np.random.seed(int(g['c3_20k/seeds'][0]))
    io, ic = PG.calibrate_ground_truth_pairs([refs[k]], [srcs[k]], [Ts[k]], 0.3)
    assert torch.equal(io[0], alone[k][4][0][0]) and torch.equal(ic[0], alone[k][4][0][1])
    again = run_case(PG, 'demo')
    first = alone[CASES.index('demo')]
    assert all(torch.equal(x, y) for x, y in zip(again[:4], first[:4]))
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(again[4], first[4]))


@pytest.mark.parametrize('name', list(F.edge_cases()))
def test_edge_cases(name):
    from se3et_amd import pair_geometry as PG
    case = F.edge_cases()[name]
    q, s, T, r = case
    for dtype in (np.float64, np.float32):
        qd, sd = dev(q.reshape(-1, 3), dtype), dev(s.reshape(-1, 3), dtype)
        d, i = PG.nearest_neighbor_pairs([qd], [sd], [T], return_index=True)
        corr = PG.get_correspondences_pairs([qd], [sd], [T], r)[0]
        assert corr.dtype == torch.int64 and corr.dim() == 2 and corr.shape[1] == 2
        F.check_edge(name, case, d[0].cpu().numpy(), i[0].cpu().numpy(), corr.cpu().numpy())
    ov = PG.compute_overlap_pairs([qd], [sd], [T], r)
    want = twin.compute_overlap(q, s, T, r)
    assert ov.shape == (1,) and (np.isnan(want) and bool(torch.isnan(ov[0])) or float(ov[0]) == want)
    o, c = PG.calibrate_ground_truth_pairs([qd], [sd], [T], r)
    _, cov, absolute, n = twin.calibrate_ground_truth(q, s, T, r)
    assert np.all(np.abs(c[0].cpu().numpy() - cov) <= max(n, 1) * F.EPS * absolute)
    if n == 0:
        assert not bool(c.any())


def test_edge_cases_in_one_stacked_call():
    """All edge cases as the pairs of one call (empty clouds between full ones), at one radius."""
    from se3et_amd import pair_geometry as PG
    cases = F.edge_cases()
    qs, ss, Ts = [dev(c[0].reshape(-1, 3)) for c in cases.values()], [dev(c[1].reshape(-1, 3)) for c in cases.values()], [c[2] for c in cases.values()]
    d, i = PG.nearest_neighbor_pairs(qs, ss, Ts, return_index=True)
    corr = PG.get_correspondences_pairs(qs, ss, Ts, 0.3)
    for p, (name, (q, s, T, _r)) in enumerate(cases.items()):
        td, ti, tc = twin.scan(q, s, T, 0.3)
        assert np.array_equal(d[p].cpu().numpy(), td) and np.array_equal(i[p].cpu().numpy(), ti), name
        assert np.array_equal(corr[p].cpu().numpy(), tc), name


@pytest.mark.parametrize('rows', [1, 1023, 1024, 1025, 2049])
def test_correspondences_at_the_chunk_sizes_of_the_row_scan(rows):
    """One pair whose query row count is the length of the one-workgroup scan of row_offsets: one row, the last sizes with one row per
    thread, the first with two, an uneven multi-row size."""
    from se3et_amd import pair_geometry as PG
    rng = np.random.default_rng(rows)
    q, s, T = rng.uniform(0, 1, (rows, 3)), rng.uniform(0, 1, (2000, 3)), np.eye(4)
    corr = PG.get_correspondences_pairs([dev(q)], [dev(s)], [T], 0.1)[0].cpu().numpy()
    want = twin.scan(q, s, T, 0.1)[2]
    assert len(want) >= rows and np.array_equal(corr, want)          # (~8 support points inside every ball)


def test_sixteen_pair_batch_matches_the_twin():
    from se3et_amd import pair_geometry as PG
    from se3et_amd.synthetic import make_pair
    pairs = [make_pair('c2_5k', k) for k in range(16)]
    refs, srcs, Ts = [dev(p[0]) for p in pairs], [dev(p[1]) for p in pairs], [p[2].astype(np.float64) for p in pairs]
    d, i = PG.nearest_neighbor_pairs(refs, srcs, Ts, return_index=True)
    ov = PG.compute_overlap_pairs(refs, srcs, Ts, 0.0375).cpu().numpy()
    corr = PG.get_correspondences_pairs(refs, srcs, Ts, 0.05)
    io, ic = PG.calibrate_ground_truth_pairs(refs, srcs, Ts, 0.006)
    for p, (ref, src, T) in enumerate(pairs):
        td, ti, tc = twin.scan(ref, src, T.astype(np.float64), 0.05)
        assert np.array_equal(d[p].cpu().numpy(), td) and np.array_equal(i[p].cpu().numpy(), ti), p
        assert ov[p] == twin.overlap_from_distances(td, 0.0375), p
        assert np.array_equal(corr[p].cpu().numpy(), tc), p
        o, cov, absolute, n = twin.calibrate_ground_truth(ref, src, T.astype(np.float64), 0.006, nn=(td, ti))
        assert float(io[p]) == o and np.all(np.abs(ic[p].cpu().numpy() - cov) <= n * F.EPS * absolute), p


def test_more_pairs_than_one_launch_takes():
    from se3et_amd import ops, pair_geometry as PG
    from se3et_amd.synthetic import make_pair
    n = ops.PAIR_MAX_PAIRS + 3
    pairs = [make_pair('micro', k) for k in range(n)]
    refs, srcs, Ts = [dev(p[0]) for p in pairs], [dev(p[1]) for p in pairs], [p[2].astype(np.float64) for p in pairs]
    d, i = PG.nearest_neighbor_pairs(refs, srcs, Ts, return_index=True)
    corr = PG.get_correspondences_pairs(refs, srcs, Ts, 0.05)
    ov = PG.compute_overlap_pairs(refs, srcs, Ts, 0.0375)
    assert len(d) == len(corr) == n and ov.shape == (n,)
    for p in (0, ops.PAIR_MAX_PAIRS - 1, ops.PAIR_MAX_PAIRS, n - 1):
        td, ti, tc = twin.scan(pairs[p][0], pairs[p][1], Ts[p], 0.05)
        assert np.array_equal(d[p].cpu().numpy(), td) and np.array_equal(i[p].cpu().numpy(), ti) and np.array_equal(corr[p].cpu().numpy(), tc)
        assert float(ov[p]) == twin.overlap_from_distances(td, 0.0375)
    assert PG.nearest_neighbor_pairs([], []) == [] and PG.compute_overlap_pairs([], [], [], 0.1).shape == (0,)


def test_single_pair_wrappers_match_the_batched_calls():
    from se3et_amd import pair_geometry as PG
    g = F.golden()
    name = 'demo'
    ref, src, T = F.inputs(name)
    d, i, ov, corr, info = run_case(PG, name)
    moved = twin.transform_points(src, T.astype(np.float64))
    wd, wi = PG.get_nearest_neighbor(ref.astype(np.float64), moved, return_index=True)
    assert isinstance(wd, np.ndarray) and wd.dtype == np.float64 and wi.dtype == np.int64
    assert np.array_equal(wd, d.cpu().numpy()) and np.array_equal(wi, i.cpu().numpy())
    assert np.array_equal(PG.get_nearest_neighbor(ref, moved), wd)
    w = PG.compute_overlap(ref, src, T, positive_radius=float(g[name + '/overlap_radii'][0]))
    assert isinstance(w, np.float64) and w == float(ov[0]) == g[name + '/overlaps'][0]
    assert PG.compute_overlap(ref.astype(np.float64), moved, None, 0.1) == g[name + '/overlaps'][1]
    wc = PG.get_correspondences(ref, src, T, twin.CASES[name][0])
    assert isinstance(wc, np.ndarray) and wc.dtype == np.int64 and np.array_equal(wc, corr.cpu().numpy())
    for k, v in enumerate(g[name + '/voxel_sizes']):
        np.random.seed(int(g[name + '/seeds'][k]))
        o, c = PG.calibrate_ground_truth(ref, src, T, voxel_size=float(v))
        assert isinstance(o, np.float64) and o == float(info[k][0]) and c.shape == (6, 6) and np.array_equal(c, info[k][1].cpu().numpy())


def test_info_records_round_trip_through_the_benchmark_reader(tmp_path):
    from se3et_amd import pair_geometry as PG
    from se3et_amd.benchmark import read_info_file
    refs, srcs, Ts = zip(*[case_tensors(n) for n in ('c1_2k', 'c2_5k')])
    _, cov = PG.calibrate_ground_truth_pairs(list(refs), list(srcs), list(Ts), 0.006)
    path = str(tmp_path / 'gt.info')
    PG.write_info_file(path, [dict(test_pair=[0, k + 2], num_fragments=9, covariance=cov[k]) for k in range(2)])
    back = read_info_file(path)
    for k in range(2):
        assert back[k]['test_pair'] == [0, k + 2] and np.array_equal(back[k]['covariance'], cov[k].cpu().numpy().astype(np.float32))
