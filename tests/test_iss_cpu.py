"""ISS keypoints without a GPU: se3_debug_iss_host (the text of csrc/iss.hip, csrc/iss_core.h and csrc/cov3.h on host memory) against the
numpy twin (tests/iss_twin.py) on the clouds of tests/iss_fixture.py, for float32 and float64 inputs.

Member counts are exact and demanded equal.  The library's eigenvalues (fixed-order sums, Jacobi sweeps) must lie within tol_i =
16 max(E, 2^-53) trace C_i of the twin's (numpy's sums, eigvalsh), E the cloud's arithmetic noise as the twin measures it.  Keypoint sets
are demanded equal on every row that is neither flagged (a saliency decision inside that tolerance) nor tainted (a flagged row in its
non_max_radius ball); at most 1 % of a cloud's rows may be either, and test_fixture_facts pins that the fixtures have none."""
import hashlib

import numpy as np
import pytest

import iss_fixture as F
import iss_twin as twin
import scan_prep_fixture as S

CLOUDS = F.edge_clouds()
DTYPES = (np.float64, np.float32)


def test_fixture_facts():
    for name in CLOUDS:
        got, want = F.facts(name), F.FACTS[name]
        assert got[:6] == want[:6], (name, got)
        assert got[5] == 0 and got[6] <= 2.0 * want[6] + 2.0 ** -52, (name, got)
    sizes = dict(zip(*np.unique(F.reference('clusters')['m'], return_counts=True)))
    assert sizes == {s: s for s in F.CLUSTER_SIZES}                          # rows with 0, 1, 63, 64, 65 and 300 members beside themselves
    assert {F.R_SALIENCY - 1, F.R_SALIENCY, F.R_SALIENCY + 1, F.R_SELECT - 1, F.R_SELECT, F.R_SELECT + 1} <= {len(v[0]) for v in CLOUDS.values()}


def _compare(name, dtype):
    p, rs, rn = CLOUDS[name]
    p = p.astype(dtype)
    ref = F.reference(name) if dtype == np.float64 else twin.compute(p, rs, rn, min_neighbors=F.MIN_NEIGHBORS)
    got = F.host_iss(p, rs, rn)
    n = len(p)
    assert got['status'] == 0
    assert np.array_equal(got['m'], ref['m']) and np.array_equal(got['c'], ref['c'])                       # exact quantities
    assert (np.abs(got['eigenvalues'] - ref['eigenvalues']) <= ref['tol'][:, None]).all()
    assert (got['eigenvalues'][ref['exact']] == 0.0).all()                                                   # zero by structure: zero bits
    unsure = ref['flagged'] | ref['tainted']
    assert unsure.sum() <= 0.01 * n
    sound = ~unsure
    assert np.array_equal(got['keypoint'][sound], ref['keypoint'][sound])
    clean = ~ref['flagged']
    assert np.array_equal(got['saliency'][clean] > 0, ref['saliency'][clean] > 0)
    assert (np.abs(got['saliency'] - ref['saliency'])[clean] <= ref['tol'][clean]).all()
    assert ((got['saliency'] == 0) | (got['saliency'] == got['eigenvalues'][:, 2])).all()                   # s is l3 or 0
    return got, ref


@pytest.mark.parametrize('dtype', DTYPES, ids=['float64', 'float32'])
@pytest.mark.parametrize('name', list(CLOUDS))
def test_host_entry_against_the_twin(name, dtype):
    _compare(name, dtype)


def test_exact_memberships():
    """A pair at exactly the radius is no member, a duplicate is; min_neighbors - 1 and min_neighbors members at each radius."""
    got = F.host_iss(*CLOUDS['exact'])
    assert got['m'].tolist() == [2, 2, 2, 2] and got['c'].tolist() == [1, 2, 2, 1]
    got = F.host_iss(*CLOUDS['min_neighbors'])
    # a group of 4, a group of 5, 4 + 3 satellites (every row's salient ball holds all 7; a satellite's non_max ball holds itself), 5 + 3
    assert got['m'].tolist() == [4] * 4 + [5] * 5 + [7] * 7 + [8] * 8
    assert got['c'].tolist() == [4] * 4 + [5] * 5 + [4] * 4 + [1] * 3 + [5] * 5 + [1] * 3
    # m = 4: no saliency; m = c = 5: keypoints; m = 7 but c = 4 or 1: a saliency and no keypoint; m = 8, c = 5: keypoints; c = 1: none
    assert (got['saliency'] > 0).tolist() == [False] * 4 + [True] * 20
    assert got['keypoint'].tolist() == [False] * 4 + [True] * 5 + [False] * 7 + [True] * 5 + [False] * 3


def test_degenerate_clusters_and_equal_saliencies():
    for name in ('planar', 'collinear', 'n0', 'n1', 'n2', 'n3', 'n4'):
        got = F.host_iss(*CLOUDS[name])
        assert not got['saliency'].any() and not got['keypoint'].any(), name
    got = F.host_iss(*CLOUDS['planar'])
    assert (got['eigenvalues'][:, 2] == 0.0).all() and (got['eigenvalues'][:, 1] > 0).all()
    got = F.host_iss(*CLOUDS['collinear'])
    assert (got['eigenvalues'][:, 1:] == 0.0).all() and (got['eigenvalues'][:, 0] > 0).all()
    # two copies an exact translation apart, inside each other's non_max ball: bit-equal saliencies, every row kept
    got = F.host_iss(*CLOUDS['copies'])
    assert (got['saliency'] > 0).all() and np.array_equal(got['saliency'][:8], got['saliency'][8:]) and got['keypoint'].all()
    # a strictly larger neighbour suppresses: lower one copy's only rival by moving a point of the other copy
    p = CLOUDS['copies'][0].copy()
    p[8, 2] += 1.0 / 64
    got = F.host_iss(p, *CLOUDS['copies'][1:])
    a, b = got['saliency'][:8], got['saliency'][8:]
    assert a[0] != b[0] and np.array_equal(got['keypoint'], np.repeat([a[0] > b[0], b[0] > a[0]], 8))


def test_gammas_and_min_neighbors_decide():
    p, rs, rn = CLOUDS['patch']
    base = F.host_iss(p, rs, rn)
    ratio = base['eigenvalues'][:, 1] / base['eigenvalues'][:, 0]
    tight = F.host_iss(p, rs, rn, gamma_21=0.5)
    assert np.array_equal(tight['saliency'] > 0, (base['saliency'] > 0) & (ratio < 0.5))
    many = F.host_iss(p, rs, rn, min_neighbors=30)
    assert np.array_equal(many['saliency'] > 0, (base['saliency'] > 0) & (base['m'] >= 30))
    assert not (many['keypoint'] & (base['c'] < 30)).any()


@pytest.mark.parametrize('name', ['patch', 'clusters', 'copies', 'n0', 'n1', 'n2', 'n257'])
def test_model_resolution(name):
    """mean over the rows of the distance to the nearest other point; a sum of non-negative terms in any order agrees with fsum to
    (n + 16) 2^-53 relative."""
    p = CLOUDS[name][0]
    got, want = F.host_resolution(p), twin.model_resolution(p)
    assert abs(got - want) <= (len(p) + 16) * F.U * want
    assert F.host_resolution(p.astype(np.float32)) == F.host_resolution(p.astype(np.float32).astype(np.float64))
    if len(p) < 2:
        assert got == 0.0


def test_host_entry_refusals():
    from se3et_amd import _lib as L
    p = CLOUDS['n257'][0].copy()
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[11, 1] = bad
        assert F.host_iss(q, 0.25, 0.15)['status'] == 1
    for kwargs in ({'gamma_21': 0.0}, {'gamma_32': np.nan}, {'gamma_21': np.inf}, {'min_neighbors': 0}):
        with pytest.raises(RuntimeError, match='debug_iss_host'):
            F.host_iss(p, 0.25, 0.15, **kwargs)
    for radii in ((-0.1, 0.1), (0.1, np.nan)):
        with pytest.raises(RuntimeError, match='radii'):
            F.host_iss(p, *radii)
    assert L.lib().se3_iss_saliency_stack(None, 1, None, 0, 0, 0, None, None, 0, 0.975, 0.975, 5, None, None) != 0
    assert L.lib().se3_pair_ball_count_radii_stack(None, 0, 0, None, 1, None, 0, None, None, None) != 0 and b'radii_stack' in L.lib().se3_last_error()


def test_refusals_before_any_launch():
    import torch
    from se3et_amd.fpfh import global_registration_pairs
    from se3et_amd.iss import compute_iss_keypoints, iss_keypoints_clouds, model_resolution_clouds
    p = torch.zeros(4, 3)
    for kwargs, word in (({'salient_radius': -1.0}, 'salient_radius'), ({'non_max_radius': np.inf}, 'non_max_radius'),
                         ({'salient_radius': np.nan}, 'salient_radius'), ({'gamma_21': 0.0}, 'gamma_21'), ({'gamma_32': -0.5}, 'gamma_32'),
                         ({'gamma_32': np.nan}, 'gamma_32'), ({'min_neighbors': 0}, 'min_neighbors'), ({'min_neighbors': 2.5}, 'min_neighbors')):
        with pytest.raises(ValueError, match=word):
            iss_keypoints_clouds([p], **kwargs)
        with pytest.raises(ValueError, match=word):
            compute_iss_keypoints(p.numpy(), **kwargs)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        iss_keypoints_clouds([p], 0.1, 0.1)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        model_resolution_clouds([p])
    with pytest.raises(ValueError, match='keypoints'):
        global_registration_pairs([p], [p], 0.1, keypoints='harris')
    with pytest.raises(ValueError, match='outlier_removal'):
        global_registration_pairs([p], [p], 0.1, outlier_removal=('median', 3, 1.0))


# the normals and covariances of se3_debug_knn_normals_host on the scan-preparation fixture, as the library returned them before
# kn_covariance, kn_rotate and the sweep loop moved into csrc/cov3.h (sha256 of the two float64 arrays' bytes, k = 33)
NORMALS_BEFORE = {
    'micro': 'be6c9791ce2ef08d337ff5140e966563ccaceddfff311484afb6e42781b57cb7',
    'c1_2k': '8fe20efd58016fcd5bc029df9bb014af9400ebb82f94cb104ac4bc7ac86dfefc',
    'c3_1500': '8408099dfe223a5262c0c5baedd5241c1ea9045715744f0790a250158c986ab8',
    'c3_gen1500': 'b6fb239f4068a3e77a79125d180e6736b82664bbf7eed3d227cdc668c5948291',
    'clusters': '06ca0b3a98758f74b6ee982caf9a7c38a13841bb821f3dec34fd81cf4da01deb',
    'collinear': 'e889332214e79e4aea80bb7a4c7b4188941275cd73d219eb55479b52d7bc3dce',
    'duplicated': 'dc4bd19f77c18f455e88c87fc52241939ede6556d5cd8340a72b57c770e5f60a',
    'identical': 'a7c02e7f925c1534e8f3ff4acb408a4ef3d96f716d9cb6697e42055ccb7fe27d',
    'lattice': '3fd3d43821672ed1c406be26f67d6a7ac98c6e8ef111911beae3e37ae2563c93',
    'n0': 'e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855',
    'n1': 'cca07ffe4acf2040c233c46b50002932022787655528202e47a2f958920d22e5',
    'n2': 'd44d56257d1dc14bde9d670ead2f50b107aba58d507eaacf43d564b3c1aaa1fc',
    'n20': 'f3df1b0237dcca15dac29780c3d76a0a01612ecc79b1e2e80674c3d544398680',
    'negative': '1b45aa1f93fdc5588a40266db6350ce15a8bdfef7ce7a2f7650c4c38180e07e7',
    'planar': '9ec4e89143b7bd9c94fa6340a2d90f674e9302fe7e2d3e32929a172630977909',
}


@pytest.mark.parametrize('name', list(S.CLOUDS) + sorted(S.edge_clouds()))
def test_shared_jacobi_header_keeps_the_normals_bits(name):
    p = S.cloud(name) if name in S.CLOUDS else S.edge_clouds()[name][0]
    n, C = S.host_normals(p)
    assert hashlib.sha256(n.tobytes() + C.tobytes()).hexdigest() == NORMALS_BEFORE[name]
