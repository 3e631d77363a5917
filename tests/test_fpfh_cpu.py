"""FPFH without a GPU: se3_debug_fpfh_host (the text of csrc/fpfh.hip and csrc/fpfh_core.h on host memory, on the neighbour lists of
se3_debug_pair_ball_host / se3_debug_knn_host) against the numpy twin (tests/fpfh_twin.py) on the clouds of tests/fpfh_fixture.py, for
float32 and float64 inputs and for the radius, k-nearest and hybrid searches.

SPFH rows are integer counts times 100 / m: equal to the twin's on every row without a flagged pair.  The twin restates the FPFH sum in the
contract's order (ascending neighbour index), so FPFH rows are demanded EQUAL as well, on every row with no flagged pair in itself or its
neighbours.  The fixtures are chosen so that the twin flags no pair at all (test_fixture_facts pins it), so no row is excluded."""
import numpy as np
import pytest

import fpfh_fixture as F
import fpfh_twin as twin

EDGES = F.edge_clouds()
DTYPES = (np.float64, np.float32)


def _compare(points, normals, radius, max_nn, ref=None):
    ref = ref or twin.compute(points, normals, radius, max_nn)
    spfh, fpfh, status = F.host_fpfh(points, normals, radius, max_nn)
    assert status == 0
    n = len(spfh)
    assert ref['flagged'].sum() <= 0.01 * n and ref['tainted'].sum() <= 0.01 * n          # the condition; the facts pin both at zero
    clean, sound = ~ref['flagged'], ~ref['tainted']
    assert np.array_equal(spfh[clean], ref['spfh'][clean])
    assert np.array_equal(spfh[clean], ref['counts'][clean] * np.where(ref['m'] > 0, 100.0 / np.maximum(ref['m'], 1), 0.0)[clean, None])
    assert np.array_equal(fpfh[sound], ref['fpfh'][sound])
    return spfh, fpfh, ref


def test_sector_constants():
    """The twenty literals of the ONE table: the library's equal the twin's, and each is within one unit in the last place of numpy's cos
    and sin.  The angle beta_k = -pi + 2 pi k / 11 is formed in numpy's extended precision (64 bits of mantissa on x86-64): rounded to
    float64 first, its own error of up to 2.2e-16 would move the cosine by several units in the last place."""
    assert np.array_equal(F.host_sectors(), twin.SECTORS)
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    pi = 4 * np.arctan(np.longdouble(1))
    beta = -pi + 2 * pi * np.arange(1, 11).astype(np.longdouble) / 11
    for got, want in ((twin.SECTORS[:, 0], np.cos(beta).astype(np.float64)), (twin.SECTORS[:, 1], np.sin(beta).astype(np.float64))):
        assert (np.abs(got - want) <= np.spacing(np.abs(want))).all()


def test_sector_rule_is_arctan2_binning():
    """The rule against clamp(floor(11 (theta + pi) / 2 pi), 0, 10) on the surface cloud's 89 590 pairs: no difference."""
    p, nr = F.cloud('surface')
    I, J = twin.pair_list(F.reference('surface_radius')['members'])
    assert len(I) == 89590
    f1, f2, x, y = twin.pair_features(p[I], nr[I], p[J], nr[J])
    want = np.clip(np.floor(11.0 * (np.arctan2(y, x) + np.pi) / (2.0 * np.pi)), 0, 10).astype(np.int64)
    assert np.array_equal(twin.theta_bin(x, y), want)


def test_fixture_facts():
    for case, (name, radius, max_nn) in F.CASES.items():
        assert F.facts(*F.cloud(name), radius, max_nn, F.reference(case)) == F.FACTS[case], case
    assert abs(F.reference('surface_radius')['m'].mean() - 59.7) < 0.05
    for name, (p, nr, radius, max_nn) in EDGES.items():
        assert F.facts(p, nr, radius, max_nn) == ((1, 1, 0) if name.startswith('pair_') else F.EDGE_FACTS[name]), name
    sizes = dict(zip(*np.unique(twin.compute(*EDGES['clusters'])['m'], return_counts=True)))
    assert sizes == {s - 1: s for s in F.CLUSTER_SIZES}                                     # rows with 0, 1, 63, 64, 65 and 300 neighbours


@pytest.mark.parametrize('dtype', DTYPES, ids=['float64', 'float32'])
@pytest.mark.parametrize('case', list(F.CASES))
def test_host_entry_equals_the_twin(case, dtype):
    name, radius, max_nn = F.CASES[case]
    p, nr = (a.astype(dtype) for a in F.cloud(name))
    spfh, fpfh, ref = _compare(p, nr, radius, max_nn, F.reference(case) if dtype == np.float64 else None)
    assert ref['flagged'].sum() == 0 and ref['tainted'].sum() == 0
    # every row with neighbours: three groups of 200
    groups = fpfh.reshape(-1, 3, twin.BINS).sum(2)
    assert (ref['m'] > 0).all() and (np.abs(groups - 200.0) <= 64 * F.U * 200.0).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=['float64', 'float32'])
@pytest.mark.parametrize('name', list(EDGES))
def test_host_entry_equals_the_twin_on_the_edges(name, dtype):
    p, nr, radius, max_nn = EDGES[name]
    spfh, fpfh, ref = _compare(p.astype(dtype), nr.astype(dtype), radius, max_nn)
    assert spfh.shape == fpfh.shape == (len(p), twin.DIM)
    assert np.array_equal(fpfh[ref['m'] == 0], np.zeros((int((ref['m'] == 0).sum()), twin.DIM)))          # no neighbour: a zero row


@pytest.mark.parametrize('name', list(F.PAIR_EDGES))
def test_pair_edges_have_their_pinned_bins(name):
    """Exact by construction: row 0 of the two-point cloud has one neighbour, so its SPFH row is 100 at the pair's three bins."""
    p, nr, (bt, b1, b2) = F.pair_edge(name)
    want = np.zeros(twin.DIM)
    want[[bt, twin.BINS + b1, 2 * twin.BINS + b2]] = 100.0
    ref = twin.compute(p, nr, F.PAIR_RADIUS)
    spfh, fpfh, status = F.host_fpfh(p, nr, F.PAIR_RADIUS)
    assert status == 0 and np.array_equal(ref['spfh'][0], want) and np.array_equal(spfh[0], want)
    if name == 'duplicate':                                                               # counted in the SPFH row, skipped in the FPFH sum
        assert np.array_equal(fpfh, spfh)
    else:
        assert fpfh[0].sum() == pytest.approx(600.0, abs=1e-9)


def test_degenerate_rows():
    for name in ('isolated', 'knn_1', 'n0', 'n1'):
        p, nr, radius, max_nn = EDGES[name]
        spfh, fpfh, status = F.host_fpfh(p, nr, radius, max_nn)
        assert status == 0 and spfh.shape == (len(p), twin.DIM) and not spfh.any() and not fpfh.any(), name
    p, nr, radius, max_nn = EDGES['one_neighbour']
    spfh, fpfh, _ = F.host_fpfh(p, nr, radius, max_nn)
    assert not spfh[2].any() and not fpfh[2].any()                                         # the isolated point
    assert sorted(spfh[0]) == [0.0] * 30 + [100.0] * 3 and fpfh[0].sum() == pytest.approx(600.0, abs=1e-9)


def test_rigid_motion():
    """The surface cloud rotated by rotvec (0.4, -0.7, 1.1), translated and permuted: its rows equal the original's within 1e-9 on rows
    without a flagged pair (measured: 1.4e-13 at most, no flagged pair in either cloud), and all 1500 mutual nearest neighbours in feature
    space are the true pairs."""
    p, nr = F.cloud('surface')
    mp, mn, perm, _, _ = F.moved_surface()
    ref, moved = F.reference('surface_radius'), twin.compute(mp, mn, 0.25)
    a, b = F.host_fpfh(p, nr, 0.25)[1], F.host_fpfh(mp, mn, 0.25)[1]
    sound = ~(moved['tainted'] | ref['tainted'][perm])
    assert sound.sum() >= 0.99 * len(p)
    worst = np.abs(b - a[perm])[sound].max()
    print('rigid motion: rows differ by at most %.3g' % worst)
    assert worst <= 1e-9
    d = (b * b).sum(1)[:, None] + (a * a).sum(1)[None] - 2.0 * b @ a.T
    to_a, to_b = d.argmin(1), d.argmin(0)
    mutual = to_b[to_a] == np.arange(len(b))
    assert mutual.sum() == 1500 and np.array_equal(to_a, perm)


def test_host_entry_refusals():
    p, nr = (a.copy() for a in F.cloud('micro'))
    for array, bad in ((p, np.nan), (nr, np.inf), (p, -np.inf)):
        keep = array[17, 1]
        array[17, 1] = bad
        assert F.host_fpfh(p, nr, 0.12)[2] == 1
        array[17, 1] = keep
    assert F.host_fpfh(p, nr, 0.12)[2] == 0
    # a list entry outside the cloud is skipped and reported, not read through
    from se3et_amd import _lib as L
    q, qn = p[:3].copy(), nr[:3].copy()
    ro, pairs = np.array([0, 2, 3, 4], np.int64), np.array([[0, 1], [0, 3], [1, -1], [2, 0]], np.int64)
    spfh, fpfh, status = np.zeros((3, 33)), np.zeros((3, 33)), np.zeros(1, np.int32)
    L.check(L.lib().se3_debug_fpfh_host(F._ptr(q), F._ptr(qn), 3, 1, 1, F._ptr(ro), F._ptr(pairs), 4, F._ptr(spfh), F._ptr(fpfh), F._ptr(status)),
            'se3_debug_fpfh_host')
    assert status[0] == 2 and spfh[0].sum() == 300.0 and not spfh[1].any() and spfh[2].sum() == 300.0


def test_refusals_before_any_launch():
    import torch
    from se3et_amd.fpfh import compute_fpfh_clouds, compute_fpfh_feature, global_registration_pairs, spfh_clouds
    p, nr = torch.zeros(4, 3), torch.zeros(4, 3)
    for fn in (compute_fpfh_clouds, spfh_clouds):
        with pytest.raises(ValueError, match='radius, max_nn or both'):
            fn([p], [nr])
        with pytest.raises(ValueError, match="above the library's limit SE3_KNN_MAX = 64"):
            fn([p], [nr], max_nn=65)
        with pytest.raises(ValueError, match='SE3_KNN_MAX'):
            fn([p], [nr], radius=0.1, max_nn=100)                                          # Open3D's tutorial value
        for radius in (0, -0.1, np.inf, np.nan):
            with pytest.raises(ValueError, match='radius'):
                fn([p], [nr], radius)
        for K in (0, -3, 2.5):
            with pytest.raises(ValueError, match='max_nn'):
                fn([p], [nr], max_nn=K)
        with pytest.raises(ValueError, match='one normals tensor per cloud'):
            fn([p, p], [nr], 0.1)
        with pytest.raises(RuntimeError, match='GPU tensor'):
            fn([p], [nr], 0.1)
        with pytest.raises(RuntimeError, match='tensor on the device'):
            fn([p.numpy()], [nr], 0.1)
    with pytest.raises(ValueError, match='dtype'):
        compute_fpfh_clouds([p], [nr], 0.1, dtype=torch.float16)
    with pytest.raises(ValueError, match='radius, max_nn or both'):
        compute_fpfh_feature(p.numpy(), nr.numpy())
    with pytest.raises(ValueError, match='voxel size'):
        global_registration_pairs([p], [p], 0.0)
    with pytest.raises(ValueError, match='one source and one reference'):
        global_registration_pairs([p], [], 0.1)
